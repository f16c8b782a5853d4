"""-m gpu: the skip_rgb output head (--q_skip_rgb) and the quantiser's --q_normalize_out.
  * `ops.to_rgb` (`ccvs_to_rgb`) against float64 arithmetic (tests/golden/to_rgb_ref.py) for C from 3 to 512, with and without the
    skip input, 8^2 to 256^2 planes, a width whose half is odd (the row-tail path), batch-strided inputs; nothing outside the output
    is written;
  * SkipGANDecoder with skip_rgb (and skip_tanh) against the reference's own decoder (tests/golden/tiny_skiprgb.*, make_golden_skiprgb.py):
    frames, flows and occlusions of every level, and the has_ctx=False call;
  * Generator.generate_vid with skip_rgb against the reference's greedy run: codes, tokens, fake / rec clips, the uint8 files; the
    serial, stream and pipelined schedules agree bit for bit;
  * --step_by_step with skip_rgb: every frame equals the full-frame decode of the same tokens;
  * --q_normalize_out: the codes of the reference's encode, and z = the gathered codebook rows over their L2 norm; in an --x_state run
    the state codes estimated from that z and the greedy frame / state tokens equal the reference's."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import ref_harness as rh  # noqa: E402
import to_rgb_ref  # noqa: E402
from make_golden_skiprgb import decoder_inputs, digest, input_clip, pack_u8_reference  # noqa: E402

pytestmark = pytest.mark.gpu

PIX_TOL = 1e-3
META = json.load(open(os.path.join(HERE, "golden", "tiny_skiprgb.json")))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "tiny_skiprgb.npz"))


def _to_rgb_case(n, c, h, w, with_skip, seed, pad_c=3):
    """Inputs on the device with a batch stride larger than C H W (a channel slice of a wider tensor)."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(n, c + pad_c, h, w, generator=g)
    x = base[:, 1:1 + c]
    wt = torch.randn(3, c, 1, 1, generator=g)
    b_conv, bias = torch.randn(3, generator=g), torch.randn(1, 3, 1, 1, generator=g)
    skip = torch.randn(n, 3, h // 2, w // 2, generator=g) if with_skip else None
    return base, x, wt, b_conv, bias, skip


def _bound(x, wt, skip):
    """1e-5 of sum_k |w_k| |x_k| / sqrt(C) + |up2(skip)| + 1, per element (float64)."""
    s = 1 / np.sqrt(x.shape[1])
    mag = torch.nn.functional.conv2d(x.double().abs(), wt.double().abs() * s) + 1.0
    if skip is not None:
        mag = mag + to_rgb_ref.upsample2(skip.double().abs())
    return 1e-5 * mag


def _form(n, h, w):
    """Channel groups per quad `ccvs_to_rgb` picks for the launch (`to_rgb_form` in csrc/resample.hip)."""
    quads = n * h * -(-w // 4)
    return 4 if -(-quads // 64) >= 1024 else (16 if -(-quads // 16) >= 256 else 64)


def test_to_rgb_cases_reach_every_form():
    assert _form(2, 8, 8) == 64 and _form(1, 256, 256) == 16 and _form(4, 256, 256) == 4 and _form(2, 16, 74) == 64
    assert _form(16, 8, 8) == 64 and _form(16, 32, 32) == 16 and _form(16, 128, 128) == 4   # BAIR levels 0, 2, 4 at batch 16


@pytest.mark.parametrize("c", [8, 128])
@pytest.mark.parametrize("with_skip", [False, True])
def test_to_rgb_op_wide_launch(c, with_skip):
    """Batch 4 at 256^2: 65536 quads, the G = 4 form the large BAIR levels run (every other case here is below it)."""
    from ccvs_amd import ops
    n, h, w = 4, 256, 256
    assert _form(n, h, w) == 4
    base, x, wt, b_conv, bias, skip = _to_rgb_case(n, c, h, w, with_skip, seed=c + 17 * int(with_skip))
    got = ops.to_rgb(base.cuda()[:, 1:1 + c], (wt.cuda() / np.sqrt(c)).reshape(3, c).contiguous(), b_conv.cuda(), bias.cuda(),
                     skip=skip.cuda() if skip is not None else None)
    want = to_rgb_ref.to_rgb(x.double(), wt.double(), b_conv.double(), bias.double(), skip.double() if skip is not None else None)
    err = (got.cpu().double() - want).abs()
    assert bool((err <= _bound(x, wt, skip)).all()), (c, with_skip, err.max().item())


@pytest.mark.parametrize("c", [3, 8, 96, 128, 512])
@pytest.mark.parametrize("hw", [(8, 8), (16, 16), (32, 74), (64, 64), (256, 256)])
@pytest.mark.parametrize("with_skip", [False, True])
def test_to_rgb_op(c, hw, with_skip):
    from ccvs_amd import ops
    h, w = hw
    n = 2 if h * w * c <= 256 * 256 * 128 else 1
    base, x, wt, b_conv, bias, skip = _to_rgb_case(n, c, h, w, with_skip, seed=c * 7 + h + w + int(with_skip))
    xd = base.cuda()[:, 1:1 + c]
    assert xd.stride(0) == (c + 3) * h * w
    scale = 1 / np.sqrt(c)
    w_scaled = (wt.cuda() * scale).reshape(3, c).contiguous()
    got = ops.to_rgb(xd, w_scaled, b_conv.cuda(), bias.cuda(), skip=skip.cuda() if skip is not None else None)
    assert got.shape == (n, 3, h, w) and got.is_contiguous()
    want = to_rgb_ref.to_rgb(x.double(), wt.double(), b_conv.double(), bias.double(), skip.double() if skip is not None else None)
    err = (got.cpu().double() - want).abs()
    assert bool((err <= _bound(x, wt, skip)).all()), (c, hw, with_skip, err.max().item())


@pytest.mark.parametrize("n,c,h,w", [(3, 8, 8, 8), (2, 96, 16, 74), (1, 512, 10, 22), (2, 128, 64, 36), (1, 96, 256, 250),
                                     (4, 8, 256, 254)])
def test_to_rgb_writes_nothing_outside(n, c, h, w):
    """NaN sentinels around the output, every form (G = 64, 16 and 4 with a row tail: widths 250 and 254)."""
    from ccvs_amd import lib
    L = lib.load()
    base, x, wt, b_conv, bias, skip = _to_rgb_case(n, c, h, w, True, seed=n + c + h + w)
    xd, skd = base.cuda()[:, 1:1 + c], skip.cuda()
    w_scaled = (wt.cuda() / np.sqrt(c)).reshape(3, c).contiguous()
    bc, bb = b_conv.cuda(), bias.cuda().reshape(3).contiguous()
    m = n * 3 * h * w
    buf = torch.full((m + 2 * 1031,), float("nan"), device="cuda")
    y = buf[1031:1031 + m]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.ccvs_to_rgb(p(xd), xd.stride(0), p(w_scaled), p(bc), p(bb), p(skd), p(y), n, c, h, w,
                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    lib.check(rc, "ccvs_to_rgb")
    torch.cuda.synchronize()
    assert torch.isnan(buf[:1031]).all() and torch.isnan(buf[1031 + m:]).all()
    assert not torch.isnan(y).any()
    want = to_rgb_ref.to_rgb(x.double(), wt.double(), b_conv.double(), bias.double(), skip.double())
    err = (y.view(n, 3, h, w).cpu().double() - want).abs()
    assert bool((err <= _bound(x, wt, skip)).all()), err.max().item()


def test_to_rgb_rejects():
    from ccvs_amd import lib, ops
    x = torch.zeros(1, 8, 6, 10, device="cuda")
    w = torch.zeros(3, 8, device="cuda")
    b = torch.zeros(3, device="cuda")
    with pytest.raises(AssertionError):
        ops.to_rgb(x, w, b, b, skip=torch.zeros(1, 3, 4, 5, device="cuda"))
    with pytest.raises(lib.CcvsError):
        ops.to_rgb(x.cpu(), w, b, b)
    assert ops.to_rgb(x, w, b, b).shape == (1, 3, 6, 10)


# ------------------------------------------------------------------ decoder against the reference's
def _decoder(name):
    from ccvs_amd.tools.options import Options
    from ccvs_amd.models.skip_vid_generator.models.skip_autoencoder import SkipGANDecoder
    opt = Options().parse(load_qvid_generator=True, load_transformer=True, argv=META["argv"] + META["decoder"][name]["flags"])
    dec = SkipGANDecoder(opt["qvid_generator"]).cuda().eval()
    sd = rh.seeded_weights(META["decoder"][name]["weight_spec"], META["weight_seeds"]["g"])
    sd.update({k: v for k, v in dec.state_dict().items() if k.endswith(".kernel")})
    dec.load_state_dict(sd, strict=True)
    return dec


def _maxdiff(a, b):
    return (a.detach().float().cpu() - torch.as_tensor(b).float()).abs().max().item()


@pytest.mark.parametrize("name", sorted(META["decoder"]))
def test_skip_rgb_decoder_vs_reference(name, gold):
    dec = _decoder(name)
    z, ctx = decoder_inputs(META["decoder_inputs"])
    ctx = [[t.cuda() for t in c] for c in ctx]
    rgb, _, flows, occs, _ = dec(z.cuda(), ctx, return_all=True)
    pre = f"decoder/{name}"
    assert rgb.shape == gold[f"{pre}/rgb"].shape
    assert _maxdiff(rgb, gold[f"{pre}/rgb"]) < PIX_TOL
    for i, (f, o) in enumerate(zip(flows, occs)):
        assert _maxdiff(f, gold[f"{pre}/flow{i}"]) < PIX_TOL, i
        assert _maxdiff(o, gold[f"{pre}/occ{i}"]) < PIX_TOL, i
    rgb0 = dec(z.cuda(), ctx, has_ctx=False)[0]
    assert rgb0.shape == gold[f"{pre}/rgb_noctx"].shape == (1, 2, 3, 8, 8)
    assert _maxdiff(rgb0, gold[f"{pre}/rgb_noctx"]) < PIX_TOL
    if name == "tanh":
        assert rgb.abs().max().item() <= 1.0


def test_skip_rgb_cache_follows_weight_updates():
    dec = _decoder("rgb")
    z, ctx = decoder_inputs(META["decoder_inputs"])
    ctx = [[t.cuda() for t in c] for c in ctx]
    before = dec(z.cuda(), ctx)[0].clone()
    with torch.no_grad():
        dec.to_rgb[2].conv.conv.weight.mul_(2.0)
    after = dec(z.cuda(), ctx)[0]
    assert not torch.equal(before, after)
    with torch.no_grad():
        dec.to_rgb[2].conv.conv.weight.div_(2.0)
    assert torch.equal(dec(z.cuda(), ctx)[0], before)


# ------------------------------------------------------------------ generation against the reference's generate_vid
def _generator(gold):
    from ccvs_amd.tools.options import Options
    from ccvs_amd.helpers.generator import Generator
    m = META["gen"]
    opt = Options().parse(load_qvid_generator=True, load_transformer=True, argv=m["argv"])
    gen = Generator(opt).build_models()
    seeds = META["weight_seeds"]
    for net, sd in ((gen.vid_model.net_e, rh.seeded_weights(m["spec_e"], seeds["e"])),
                    (gen.vid_model.net_g, rh.seeded_weights(m["spec_g"], seeds["g"])),
                    (gen.vid_model.net_q, {"embedding.weight": torch.from_numpy(gold["gen/q/embedding.weight"])}),
                    (gen.transformer_model.net_t, rh.seeded_weights(m["spec_t"], seeds["t"]))):
        missing, unexpected = net.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.endswith((".kernel", ".mask")) for k in missing), (missing, unexpected)
    gen.opt.sample = False
    return gen


def _run(gen, vid, schedule):
    torch.manual_seed(META["gen"]["seed"])
    data = {"vid": vid.clone()}
    if schedule == "pipelined":
        out = gen.run_pipelined([data], rec_pass=True)[0]
    else:
        out = gen.generate_vid(data, schedule=schedule)
    torch.cuda.synchronize()
    return out


def test_skip_rgb_generate_vid_golden(gold, tmp_path):
    vid = input_clip()
    assert digest(vid.numpy()) == META["gen"]["vid_sha256"]
    gen = _generator(gold)
    outs = {s: _run(gen, vid, s) for s in ("serial", "stream", "pipelined")}
    out = outs["serial"]
    assert torch.equal(out["enc_code"].cpu(), torch.from_numpy(gold["gen/enc_code"]).long())
    assert torch.equal(out["fake"]["code"].cpu(), torch.from_numpy(gold["gen/code"]).long()), "tokens"
    want = {"real": vid, "fake": torch.from_numpy(gold["gen/fake"]), "rec": torch.from_numpy(gold["gen/rec"])}
    assert out["fake"]["vid"].shape == want["fake"].shape
    assert _maxdiff(out["fake"]["vid"], want["fake"]) < PIX_TOL
    assert _maxdiff(out["rec"]["vid"], want["rec"]) < PIX_TOL
    for s in ("stream", "pipelined"):
        assert torch.equal(outs[s]["fake"]["code"], out["fake"]["code"]), s
        for key in ("fake", "rec"):
            assert torch.equal(outs[s][key]["vid"], out[key]["vid"]), (s, key)
    gen.opt.result_path = str(tmp_path)
    gen.save_results(out, 0)
    for rel in META["gen"]["files"]:
        sub, base = rel.split("/")
        i = int(base[len("vid_"):-len(".mp4")])
        got = np.load(os.path.join(str(tmp_path), sub, base[:-len(".mp4")] + ".npy"))
        ref = pack_u8_reference(want[sub])[i].numpy()
        if sub == "real":
            assert np.array_equal(got, ref), rel
        else:   # decoded clips agree within 1e-3: a uint8 value may sit one step away where the reference's lies at a boundary
            assert np.abs(got.astype(int) - ref.astype(int)).max() <= 1, rel
            t = want[sub][i].clamp(-1, 1).add(1).div(2).mul(255).permute(0, 2, 3, 1).double().numpy()
            off = got != ref
            assert np.all(np.abs(t[off] - np.round(t[off])) < 0.3), rel


# ------------------------------------------------------------------ --q_normalize_out
def test_normalize_out_encode(gold):
    from ccvs_amd.tools.options import Options
    from ccvs_amd.models.skip_vid_generator.models.quantized_video_model import QVidModel
    m = META["norm"]
    qopt = Options().parse(load_qvid_generator=True, load_transformer=True, argv=m["argv"])["qvid_generator"]
    torch.manual_seed(0)
    qv = QVidModel(qopt, is_train=False, is_main=True).eval()
    assert qv.net_q.normalize and qv.net_e.normalize_out
    qv.net_e.load_state_dict(rh.seeded_weights(m["spec_e"], META["weight_seeds"]["e"]), strict=False)
    cb = torch.from_numpy(gold["norm/q/embedding.weight"])
    qv.net_q.load_state_dict({"embedding.weight": cb})
    enc = qv.encode(input_clip().cuda(), None, "vid", False, None, None)
    code = enc["code"].cpu()
    assert torch.equal(code, torch.from_numpy(gold["norm/code"]).long())
    # z = E[code] / ||E[code]||_2 over the channels, [B, T, C, h, w]; embed_code keeps the raw rows
    e = cb[code.view(-1)].view(2, 4, 8, 8, -1)
    want = (e / torch.norm(e, p=2, dim=-1, keepdim=True)).permute(0, 1, 4, 2, 3)
    assert enc["z"].shape == want.shape
    assert _maxdiff(enc["z"], want) < 1e-6
    assert _maxdiff(enc["z"], gold["norm/z"]) < 1e-6
    raw = qv.net_q.embed_code_nchw(code.view(-1).cuda(), 8, 8, 8)
    assert torch.equal(raw.cpu(), cb[code.view(-1)].view(8, 8, 8, -1).permute(0, 3, 1, 2))


def test_skip_rgb_step_by_step_matches_full_frame_decoder(gold):
    """`--step_by_step` with skip_rgb.  The step decoder (`vid_step_decoder`: decode one frame from the contexts so far, re-encode it,
    push its skip features) chained over the fixture's tokens gives, frame by frame, the full-frame decoder's clip of the same
    tokens -- and the reference's (`gen/fake`).  Then the whole `--step_by_step` driver runs: the conditioning frame is returned as
    given (the reference keeps the real frame), the predicted frames at full resolution."""
    vid = input_clip()
    gen = _generator(gold)
    qv = gen.vid_model
    code = torch.from_numpy(gold["gen/code"]).long().cuda()
    with torch.no_grad():
        inter = [f[:, :1] for f in qv({"vid": vid.clone()}, mode="vid_encoder")["inter"]]
        full = qv({"code": code.clone(), "inter": inter}, mode="vid_decoder")["vid"]
        step_inter = inter
        for t in range(1, full.shape[1]):
            step = qv({"code": code[:, t * 64:(t + 1) * 64].clone(), "inter": step_inter}, mode="vid_step_decoder")
            step_inter = step["inter"]
            assert step["vid"].shape == (2, 1, 3, 32, 32)
            assert _maxdiff(step["vid"][:, 0], full[:, t].cpu()) < 1e-5, t
            assert _maxdiff(step["vid"][:, 0], gold["gen/fake"][:, t]) < PIX_TOL, t
    gen.opt.step_by_step = True
    try:
        torch.manual_seed(META["gen"]["seed"])
        out = gen.generate_vid({"vid": vid.clone()}, schedule="serial")
        torch.cuda.synchronize()
    finally:
        gen.opt.step_by_step = False
    assert out["fake"]["vid"].shape == (2, 4, 3, 32, 32)
    assert torch.equal(out["fake"]["code"][:, :64].cpu(), torch.from_numpy(gold["gen/enc_code"]).long()[:, :64])
    assert torch.equal(out["fake"]["vid"][:, 0].cpu(), vid[:, 0])
    assert bool(torch.isfinite(out["fake"]["vid"]).all())


def test_normalize_out_state_run(gold):
    """--x_state with --q_normalize_out: StateModel estimates the state from the normalised z, so the state codes, and through them
    the synthesized tokens, depend on the option.  Codes, state codes, greedy frame and state tokens equal the reference's."""
    from ccvs_amd.tools.options import Options
    from ccvs_amd.helpers.generator import Generator
    m = META["state"]
    opt = Options().parse(load_qvid_generator=True, load_transformer=True, load_state_estimator=True, argv=m["argv"])
    gen = Generator(opt).build_models()
    seeds = META["weight_seeds"]
    for net, sd in ((gen.vid_model.net_e, rh.seeded_weights(META["norm"]["spec_e"], seeds["e"])),
                    (gen.vid_model.net_g, rh.seeded_weights(m["spec_g"], seeds["g"])),
                    (gen.vid_model.net_q, {"embedding.weight": torch.from_numpy(gold["norm/q/embedding.weight"])}),
                    (gen.state_model.net_s, rh.seeded_weights(m["spec_s"], seeds["s"])),
                    (gen.state_model.net_q, {"embedding.weight": torch.from_numpy(gold["state/sq/embedding.weight"])}),
                    (gen.transformer_model.net_t, rh.seeded_weights(m["spec_t"], seeds["t"] + 100))):
        missing, unexpected = net.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.endswith((".kernel", ".mask")) for k in missing), (missing, unexpected)
    assert gen.vid_model.net_q.normalize and gen.opt.state
    gen.opt.sample, gen.opt.sample_state = False, False
    vid = input_clip()
    code_of = lambda key: torch.from_numpy(gold[key]).long()
    with torch.no_grad():
        enc = gen.vid_model({"vid": vid.clone()}, mode="vid_encoder")
        st = gen.state_model(enc, mode="vid_encoder")["state_code"]
    assert torch.equal(enc["code"].cpu(), code_of("state/enc_code"))
    assert torch.equal(st.cpu(), code_of("state/state_code")), "state codes estimated from the normalised z"
    torch.manual_seed(META["gen"]["seed"])
    out = gen.generate_vid({"vid": vid.clone()}, schedule="serial")
    torch.cuda.synchronize()
    assert torch.equal(out["fake"]["code"].cpu(), code_of("state/code")), "frame tokens"
    assert torch.equal(out["fake"]["state_code"].cpu(), code_of("state/gen_state_code")), "state tokens"
    assert _maxdiff(out["fake"]["vid"], gold["state/fake"]) < PIX_TOL

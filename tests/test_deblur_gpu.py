"""-m gpu: the deblurring mode (`--x_deblurring`).
  * `ops.gaussian_blur` (`ccvs_gaussian_blur`) against the float64 restatement of torchvision's GaussianBlur (tests/golden/blur_ref.py)
    for every kernel size the mode uses, strided inputs, odd plane sizes; nothing outside the output is written;
  * `Generator.generate_vid` against the reference's own run (tests/golden/tiny_deblur.{npz,json}, make_golden_deblur.py): the
    blurred clip's codes, the greedy and the host-noise-sampled tokens, the fake / rec / blur clips and the files `save_results`
    writes; the serial, stream and `run_pipelined` schedules give the same clips, bit for bit;
  * one BAIR clip (256^2, 16 frames) blurred with sigma 10, and its encode at the full geometry against the CPU oracle."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import blur_ref  # noqa: E402
import ref_harness as rh  # noqa: E402
from make_golden_deblur import blur_sigma_of, digest, input_clip, pack_u8_reference  # noqa: E402

pytestmark = pytest.mark.gpu

PIX_TOL = 1e-3
META = json.load(open(os.path.join(HERE, "golden", "tiny_deblur.json")))


def _blur_bound(x):
    return 4e-6 * float(x.abs().max())


def _check_blur(x, k, sigma):
    from ccvs_amd import ops
    got = ops.gaussian_blur(x, k, sigma)
    assert got.is_contiguous() and got.shape == x.shape
    want = blur_ref.gaussian_blur(x.detach().cpu(), k, sigma, dtype=torch.float64)
    err = (got.cpu().double() - want).abs().max().item()
    assert err <= _blur_bound(x), (k, sigma, tuple(x.shape), err)


KS = [(3, 1.0), (7, 2.0), (9, 3.0), (13, 4.0), (13, 10.0), (3, 10.0), (13, 1.0)]


@pytest.mark.parametrize("n,c,h,w", [(256, 3, 7, 7), (1, 3, 13, 14), (16, 3, 64, 64), (2, 3, 64, 128), (1, 3, 256, 256)])
def test_gaussian_blur_op(n, c, h, w):
    g = torch.Generator().manual_seed(n * 1000 + h + w)
    x = (torch.rand(n, c, h, w, generator=g) * 2 - 1).cuda()
    for k in (3, 7, 9, 13):
        for sigma in (1.0, 2.0, 3.0, 4.0, 10.0):
            _check_blur(x, k, sigma)


def test_gaussian_blur_strided_input():
    """A channel slice of a wider tensor (batch and channel strides of its own, planes dense) and a frame view of a clip."""
    g = torch.Generator().manual_seed(5)
    base = (torch.rand(6, 5, 33, 70, generator=g) * 4 - 2).cuda()
    x = base[:, 1:4]
    assert not x.is_contiguous()
    for k, sigma in KS:
        _check_blur(x, k, sigma)
    clip = (torch.rand(2, 9, 3, 20, 36, generator=g) * 2 - 1).cuda()
    for k, sigma in KS:
        _check_blur(clip[:, 1:8].reshape(14, 3, 20, 36), k, sigma)
    _check_blur(base[:, :, :, 3:67], 7, 2.0)          # rows not dense: the wrapper makes them so


def test_gaussian_blur_writes_nothing_outside():
    from ccvs_amd import lib, ops
    L = lib.load()
    n, c, h, w = 3, 3, 29, 45
    x = (torch.rand(n, c, h, w, generator=torch.Generator().manual_seed(2)) * 2 - 1).cuda()
    for k, sigma in KS:
        buf = torch.full((n * c * h * w + 2 * 1031,), float("nan"), device="cuda")
        y = buf[1031:1031 + n * c * h * w]
        wt = ops.gaussian_kernel1d(k, sigma)
        rc = L.ccvs_gaussian_blur(ctypes.c_void_p(x.data_ptr()), x.stride(0), x.stride(1), ctypes.c_void_p(y.data_ptr()), n, c, h, w, k,
                                  (ctypes.c_float * k)(*wt.tolist()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        lib.check(rc, "ccvs_gaussian_blur")
        torch.cuda.synchronize()
        assert torch.isnan(buf[:1031]).all() and torch.isnan(buf[1031 + n * c * h * w:]).all()
        assert not torch.isnan(y).any()
        want = blur_ref.gaussian_blur(x.cpu(), k, sigma, dtype=torch.float64).reshape(-1)
        assert (y.cpu().double() - want).abs().max().item() <= _blur_bound(x)


def test_gaussian_blur_rejects():
    from ccvs_amd import lib, ops
    x = torch.zeros(1, 3, 6, 40, device="cuda")
    with pytest.raises(lib.CcvsError):
        ops.gaussian_blur(x, 13, 4.0)                 # k // 2 = 6 >= H, as F.pad(mode="reflect") rejects it
    with pytest.raises(lib.CcvsError):
        ops.gaussian_blur(x.transpose(2, 3).contiguous(), 13, 4.0)
    with pytest.raises(lib.CcvsError):
        ops.gaussian_blur(torch.zeros(1, 3, 20, 20, device="cuda"), 15, 5.0)
    ops.gaussian_blur(x, 11, 4.0)                     # k // 2 = 5 < 6: fine


# ------------------------------------------------------------------ end to end against the reference's generate_vid
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "tiny_deblur.npz"))


@pytest.fixture(scope="module")
def vid():
    v = input_clip()
    assert digest(v) == META["vid_sha256"]
    return v


def _generator(case, gold):
    from ccvs_amd.tools.options import Options
    from ccvs_amd.helpers.generator import Generator
    opt = Options().parse(load_qvid_generator=True, load_transformer=True, argv=META["argv"] + META["cases"][case]["flags"])
    gen = Generator(opt).build_models()
    seeds = META["weight_seeds"]
    ci = list(META["cases"]).index(case)
    for net, sd in ((gen.vid_model.net_e, rh.seeded_weights(META["spec_e"], seeds["e"])),
                    (gen.vid_model.net_g, rh.seeded_weights(META["spec_g"], seeds["g"])),
                    (gen.vid_model.net_q, {"embedding.weight": torch.from_numpy(gold["q/embedding.weight"])}),
                    (gen.transformer_model.net_t, rh.seeded_weights(META["cases"][case]["spec_t"], seeds["t"] + 100 * ci))):
        missing, unexpected = net.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.endswith((".kernel", ".mask")) for k in missing), (missing, unexpected)
    return gen


def _run(gen, vid, mode, schedule):
    gen.opt.sample = mode == "sampled"
    torch.manual_seed(META["seeds"][mode])
    data = {"vid": vid.clone()}
    if schedule == "pipelined":
        out = gen.run_pipelined([data], rec_pass=True)[0]
    else:
        out = gen.generate_vid(data, schedule=schedule)
    torch.cuda.synchronize()
    return out


def _maxdiff(a, b):
    return (a.detach().float().cpu() - torch.as_tensor(b).float()).abs().max().item()


@pytest.mark.parametrize("case", list(META["cases"]))
def test_deblur_generate_vid_golden(case, gold, vid, tmp_path):
    gen = _generator(case, gold)
    blurred = blur_ref.blur(vid, blur_sigma_of(META["cases"][case]["flags"]))   # bit for bit the reference's (make_golden_deblur.py)
    code_of = lambda key: torch.from_numpy(gold[key]).long()
    for mode in META["seeds"]:
        pre = f"{case}/{mode}"
        # the working set: the clip's codes and the blurred clip's codes (the ancillary stream)
        torch.manual_seed(META["seeds"][mode])
        ws = gen.condition({"vid": vid.clone()})
        assert torch.equal(ws["encoded"]["code"].cpu(), code_of(f"{pre}/enc_code"))
        assert torch.equal(ws["cropped"]["state_code"].cpu(), code_of(f"{pre}/blur_code")), "blurred-clip codes"
        assert ws["cropped"]["inter"][0].shape[1] == gen.opt.vid_len          # the whole blurred clip's skip features
        assert ws["total_len"] == 2 * gen.opt.vid_len * 64
        assert _maxdiff(ws["blur"]["vid"], blurred) < 1e-5

        outs = {s: _run(gen, vid, mode, s) for s in ("serial", "stream", "pipelined")}
        out = outs["serial"]
        assert torch.equal(out["fake"]["code"].cpu(), code_of(f"{pre}/code")), f"{pre}: tokens"
        assert _maxdiff(out["blur"], blurred) < 1e-5
        want = {"real": vid, "blur": blurred}          # the reference's float clips, where the fixture has them
        if f"{pre}/fake" in gold.files:
            want["fake"], want["rec"] = torch.from_numpy(gold[f"{pre}/fake"]), torch.from_numpy(gold[f"{case}/rec"])
            assert _maxdiff(out["fake"]["vid"], want["fake"]) < PIX_TOL
            assert _maxdiff(out["rec"]["vid"], want["rec"]) < PIX_TOL
        for s in ("stream", "pipelined"):
            assert torch.equal(outs[s]["fake"]["code"], out["fake"]["code"]), s
            for key in ("fake", "rec"):
                assert torch.equal(outs[s][key]["vid"], out[key]["vid"]), (s, key)
            assert torch.equal(outs[s]["blur"], out["blur"]), s

        # the files: real / fake / rec / blur, uint8 as the reference packed them
        gen.opt.result_path = str(tmp_path / pre)
        gen.save_results(out, 0)
        own = {"fake": out["fake"]["vid"].cpu(), "rec": out["rec"]["vid"].cpu()}
        for rel in META["cases"][case]["files"][mode]:
            sub, base = rel.split("/")
            i = int(base[len("vid_"):-len(".mp4")])
            stem = os.path.join(gen.opt.result_path, sub, base[:-len(".mp4")])
            assert os.path.exists(stem + ".npy"), f"{rel} not written"
            got = np.load(stem + ".npy")
            if sub not in want:                        # decoded clips of the sliding case: the files hold the clips returned
                assert np.array_equal(got, pack_u8_reference(own[sub])[i].numpy()), rel
                continue
            ref = pack_u8_reference(want[sub])[i].numpy()   # the reference's bytes (tests/test_deblur_host.py checks the digests)
            if sub == "real":
                assert np.array_equal(got, ref), rel
                continue
            # blurred and decoded clips: within their float bars, so a uint8 value may differ by one step, and for the blurred clip
            # (|err| ~1e-6) only where the reference's value lies at a step boundary
            assert np.abs(got.astype(int) - ref.astype(int)).max() <= 1, rel
            if sub == "blur":
                t = (want["blur"][i].clamp(-1, 1).add(1).div(2).mul(255)).permute(0, 2, 3, 1).double().numpy()
                off = got != ref
                assert np.all(np.abs(t[off] - np.round(t[off])) < 1e-3), rel
        assert sorted(os.listdir(gen.opt.result_path)) == ["blur", "fake", "real", "rec"]


def test_deblur_warm_up_draws_nothing(gold, vid):
    """`condition(draw=False)` (the pipeline's warm-up) leaves the process generator alone; `draw=True` moves it by one draw."""
    gen = _generator("whole", gold)
    torch.manual_seed(3)
    gen.condition({"vid": vid.clone()}, draw=False)
    a = torch.rand(3)
    torch.manual_seed(3)
    assert torch.equal(torch.rand(3), a)
    torch.manual_seed(3)
    gen.condition({"vid": vid.clone()})
    b = torch.rand(3)
    torch.manual_seed(3)
    torch.empty(1).uniform_(2.0, 2.0)
    assert torch.equal(torch.rand(3), b)


# ------------------------------------------------------------------ BAIR geometry
def test_deblur_bair_clip():
    from ccvs_amd.tools.options import Options, BAIR_ARGV
    from ccvs_amd.models.skip_vid_generator.models.quantized_video_model import QVidModel
    from ccvs_amd.helpers.generator import blur
    from oracle import ccvs_oracle as O
    vid = torch.rand(1, 16, 3, 256, 256, generator=torch.Generator().manual_seed(9)) * 2 - 1
    blurred = blur({"vid": vid}, blur_sigma=10, draw=False)["vid"]
    want = blur_ref.blur(vid.double(), 10)
    err = (blurred.cpu().double() - want).abs().max().item()
    assert err <= _blur_bound(vid), err

    opt = Options().parse(load_qvid_generator=True, load_transformer=True, argv=list(BAIR_ARGV))
    qopt = opt["qvid_generator"]
    torch.manual_seed(0)
    qv = QVidModel(qopt, is_train=False, is_main=True).eval()
    with torch.no_grad():
        z_e, _ = qv.net_e(blurred[:, :2].contiguous())
        cb = qv.net_q.embedding.weight
        cb.copy_((torch.randn(cb.shape, generator=torch.Generator().manual_seed(4)) * float(z_e.std())).cuda())
        code = qv({"vid": blurred}, mode="vid_encoder")["code"].cpu()
    nets = {k: {n: v.detach().cpu() for n, v in m.state_dict().items()} for k, m in (("e", qv.net_e), ("q", qv.net_q))}
    z, _ = O.encoder_forward(nets["e"], qopt, blurred.cpu())
    _, idx = O.vq_quantize(z, nets["q"]["embedding.weight"])
    want_code = idx.view(z.shape[0], -1)
    assert code.shape == want_code.shape == (1, 16 * 64)
    diff = (code != want_code).nonzero()
    if len(diff):                                   # a flip is only acceptable at a near-tie of the two nearest codewords
        zf = z.transpose(-3, -1).transpose(-3, -2).reshape(-1, z.shape[-3]).double()
        e = nets["q"]["embedding.weight"].double()
        d = (zf ** 2).sum(1, keepdim=True) + (e ** 2).sum(1) - 2 * zf @ e.t()
        for _, j in diff.tolist():
            gap = (d[j, code[0, j]] - d[j, want_code[0, j]]).abs().item()
            assert gap < 1e-4 * d[j].abs().max().item(), (j, gap)
    print(f"BAIR blur max|err| {err:.2e}; encode of the blurred clip: {len(diff)} of {code.numel()} codes differ from the CPU oracle")

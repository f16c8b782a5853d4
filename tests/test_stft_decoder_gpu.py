"""-m gpu: the STFT decoder on the MI355X, through the C ABI wrappers and the public modes.

  6. `ops.channel_head` (`ccvs_channel_head`) against float64: all six instantiations (G = 64 / 16 / 4 channel groups x four pixels or
     one per lane), every flag combination, strided batch, NaN guards;
  7. `ops.mse` (`ccvs_mse`) against numpy float64;
  8. `StftModel` `vid_decoder` / `img_decoder` against the reference's outputs (tests/golden/tiny_stft_decoder.npz), 1e-3 abs, in
     both convolution precisions;
     and a seeded `StftModel` against the values the reference's own model draws (the construction order net_e, net_d, net_q);
  9. `eval_stft_reconstruction` / `eval_state_estimator` within the bound that follows from the measured decoder difference;
 10. Drums geometry (1024 x 512 codebook, 512 channels, 8 x 2 -> 64 x 16) against the CPU composition of tests/stft_decoder_ref.py;
 11. `Generator` with `--decode_stft`: all three schedules, the files of `run()`, and nothing at all without the flag.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402
import stft_decoder_ref as R  # noqa: E402

T = torch.from_numpy
ULP = 2.0 ** -23


def _parse(argv):
    from ccvs_amd.tools.options import Options
    return Options().parse(True, True, load_state_estimator=True, load_stft_ae=True, argv=argv)


def _load(net, sd):
    own = net.state_dict()
    with torch.no_grad():
        for k, v in sd.items():
            own[k].copy_(v)


# ------------------------------------------------------------------ 6. the head kernel
def _form(n, h, w):
    """(channel groups G, pixels per lane) `ccvs_channel_head` picks for the launch (`channel_head_form` in csrc/stft.hip)."""
    px = 4 if (h * w) % 4 == 0 else 1
    items = n * (h * w // px)
    return (4 if -(-items // 64) >= 1024 else (16 if -(-items // 16) >= 256 else 64)), px


# launches wide enough for the G = 16 and the G = 4 forms, in both pixel forms (C = 13: channel ranges of unequal and of zero length)
WIDE_CASES = [(8, (64, 16), 20, 16), (8, (64, 16), 260, 4), (13, (64, 16), 24, 16), (13, (64, 16), 270, 4),
              (8, (7, 5), 120, 16), (8, (7, 5), 1900, 4), (13, (7, 5), 130, 16), (13, (7, 5), 1901, 4)]


def test_channel_head_cases_reach_every_form():
    """The six instantiations (G = 64 / 16 / 4, four pixels or one per lane) are all run under the float64 check below; the Drums
    batch of 8 clips x 45 frames takes G = 4, the shapes of the decoder tests G = 64."""
    small = {_form(n, h, w) for (h, w) in [(16, 8), (64, 16), (2, 1), (7, 5)] for n in (1, 5)}
    wide = {_form(n, h, w) for _, (h, w), n, _ in WIDE_CASES}
    assert small == {(64, 4), (64, 1)} and wide == {(16, 4), (4, 4), (16, 1), (4, 1)}
    for _, (h, w), n, g in WIDE_CASES:
        assert _form(n, h, w)[0] == g
    assert _form(8 * 45, 64, 16) == (4, 4) and _form(6, 64, 16) == (64, 4) and _form(10, 16, 8) == (64, 4)


@pytest.mark.parametrize("c,hw,n,g", WIDE_CASES)
def test_channel_head_wide_launches_against_float64(c, hw, n, g):
    assert _form(n, *hw)[0] == g
    _check_channel_head(c, hw, n)


@pytest.mark.parametrize("c", [8, 13, 512])
@pytest.mark.parametrize("hw", [(16, 8), (64, 16), (2, 1), (7, 5)])
@pytest.mark.parametrize("n", [1, 5])
def test_channel_head_against_float64(c, hw, n):
    _check_channel_head(c, hw, n)


def _check_channel_head(c, hw, n):
    """Float64 evaluation on the CPU, per-element bound 1e-5 x sum_c |w_c x_c| (+ one fp32 ulp of the result behind the tanh), a
    batch-strided input, every flag combination, NaN sentinels around the output, two runs with equal bits."""
    from ccvs_amd import ops
    h, w = hw
    g = torch.Generator().manual_seed(1000 * c + 10 * h + n)
    xs = torch.randn(n, c + 3, h, w, generator=g)          # a batch-strided input: the first c of c + 3 channels
    wt = torch.randn(1, c, 1, 1, generator=g)
    bias = torch.randn(1, generator=g) * 0.1
    scale = 1 / np.sqrt(c)
    x = xs[:, :c]
    ws = (wt * scale).reshape(c).double()                 # the fp32 product, then float64 arithmetic
    terms = ws.view(1, c, 1, 1) * x.double()
    pre = terms.sum(1, keepdim=True) + bias.double()
    mag = terms.abs().sum(1, keepdim=True)
    xg, wg, bg = xs.cuda()[:, :c], wt.cuda(), bias.cuda()
    assert xg.stride(0) == (c + 3) * h * w
    for act, tanh in ((False, False), (True, False), (True, True)):
        want = pre
        if act:
            want = torch.where(want > 0, want, 0.1 * want)
        if tanh:
            want = torch.tanh(want)
        bound = 1e-5 * mag + (ULP * want.abs() if tanh else 0.0)
        outs = []
        for _ in range(2):
            buf = torch.full((n * h * w + 64,), float("nan"), device="cuda")
            out = buf[32:32 + n * h * w].view(n, 1, h, w)
            ops.channel_head(xg, wg, scale, bg, act=act, tanh=tanh, out=out)
            torch.cuda.synchronize()
            assert torch.isnan(buf[:32]).all() and torch.isnan(buf[32 + n * h * w:]).all(), "wrote outside its output"
            outs.append(out.cpu())
        assert torch.equal(outs[0], outs[1]), "run-to-run bits differ"
        err = (outs[0].double() - want).abs()
        assert bool((err <= bound).all()), (c, hw, n, act, tanh, float((err / bound.clamp_min(1e-30)).max()))
    # no bias
    got = ops.channel_head(xg, wg, scale, None, act=False, tanh=False).cpu().double()
    assert bool(((got - (pre - bias.double())).abs() <= 1e-5 * mag).all())


# ------------------------------------------------------------------ 7. the reduction
@pytest.mark.parametrize("n", [1, 7, 4096, 2 ** 20 + 3])
def test_mse_against_float64(n):
    from ccvs_amd import ops
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ref = float(np.mean((a.numpy().astype(np.float64) - b.numpy().astype(np.float64)) ** 2))
    ag, bg = a.cuda(), b.cuda()
    got = ops.mse(ag, bg)
    assert got.shape == () and got.dtype == torch.float32 and got.is_cuda
    assert abs(float(got) - ref) <= ULP * abs(ref), (float(got), ref)
    assert torch.equal(got, ops.mse(ag, bg))
    assert float(ops.mse(ag, ag.clone())) == 0.0
    # an unaligned view takes the scalar path: same value within the same bound
    if n > 7:
        ref1 = float(np.mean((a.numpy()[1:].astype(np.float64) - b.numpy()[1:].astype(np.float64)) ** 2))
        assert abs(float(ops.mse(ag[1:], bg[1:])) - ref1) <= ULP * abs(ref1)


# ------------------------------------------------------------------ 8 / 9. the tiny fixture
@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "tiny_stft_decoder.npz"))


@pytest.fixture(scope="module")
def tiny_sm(gold):
    from ccvs_amd.models.skip_vid_generator.models.stft_model import StftModel
    sm = StftModel(_parse(rh.TINY_STATE_ARGV)["stft_ae"], is_train=False, is_main=True).eval()
    for pre, net in (("ae", sm.net_e), ("ad", sm.net_d), ("aq", sm.net_q)):
        _load(net, {k[len(pre) + 1:]: T(gold[k]) for k in gold.files if k.startswith(pre + "/")})
    return sm


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
def test_tiny_decoder_and_eval_against_the_reference(gold, tiny_sm, prec, monkeypatch):
    from ccvs_amd import ops
    monkeypatch.setattr(ops, "CONV_PRECISION", prec)
    vid_ref, img_ref = T(gold["vid_decoder"]), T(gold["img_decoder"])
    assert R.well_conditioned(vid_ref)
    codes = T(gold["state_code"])
    out = tiny_sm({"state_code": codes.clone()}, mode="vid_decoder")
    assert set(out) == {"stft"} and out["stft"].shape == vid_ref.shape and out["stft"].dtype == torch.float32
    d_vid = (out["stft"].cpu() - vid_ref).abs().max().item()
    out_i = tiny_sm({"state_code": codes[:, :2].clone()}, mode="img_decoder")
    assert set(out_i) == {"stft"} and out_i["stft"].shape == img_ref.shape
    d_img = (out_i["stft"].cpu() - img_ref).abs().max().item()
    print(f"[{prec}] tiny vid_decoder max|diff| {d_vid:.3e}  img_decoder {d_img:.3e}")
    assert d_vid <= 1e-3 and d_img <= 1e-3
    # eval_stft_reconstruction: |mean((s - p)^2) - mean((s - p_ref)^2)| <= 2 d mean|s - p_ref| + d^2, plus the fp32 rounding of the value
    stft, pred_ref, want = T(gold["stft"]), T(gold["eval_stft_pred"]), float(gold["eval_stft_reconstruction"])
    # d is measured again here, on the prediction the figure is formed from: it goes through the encoder and carries the difference
    # between the codebook rows ours returns and the reference's z + (z_q - z) (quantize.py:64), which the decode of given codes in
    # the first half does not see -- the bound follows from THIS difference
    z_q, _, info = tiny_sm.net_q(tiny_sm.net_e(stft.cuda()))
    assert torch.equal(info[2].view(2, -1).cpu(), codes), "the encoder's indices must not differ"
    d = (tiny_sm.net_d(z_q).cpu() - pred_ref).abs().max().item()
    got = tiny_sm({"stft": stft.clone()}, mode="eval_stft_reconstruction")
    assert got.shape == () and got.dtype == torch.float32 and got.is_cuda
    bound = 2 * d * float((stft - pred_ref).abs().mean()) + d * d + ULP * abs(want)
    print(f"[{prec}] eval_stft_reconstruction {float(got):.8f} reference {want:.8f} d {d:.3e} bound {bound:.3e}")
    assert d <= 1e-3 and abs(float(got) - want) <= bound
    with pytest.raises(NotImplementedError):
        tiny_sm({"stft": stft.clone()}, mode="stft_reconstruction")
    with pytest.raises(ValueError):
        tiny_sm({"stft": stft.clone()}, mode="nonsense")


def test_eval_state_estimator_against_the_reference(gold, golden_dir):
    from ccvs_amd.models.skip_vid_generator.models.state_model import StateModel
    base = np.load(os.path.join(golden_dir, "tiny_statemodel.npz"))
    sm = StateModel(_parse(rh.TINY_STATEMODEL_ARGV)["state_estimator"], is_train=False, is_main=True).eval()
    _load(sm.net_s, {k[2:]: T(base[k]) for k in base.files if k.startswith("s/")})
    _load(sm.net_q, {k[3:]: T(base[k]) for k in base.files if k.startswith("sq/")})
    z, given = T(base["z"]), T(base["given"])
    assert torch.equal(sm({"z": z.clone()}, mode="vid_encoder")["state_code"].cpu(), T(base["state_code"])), "indices must not differ"
    q_ref, want = T(gold["eval_state_q"]), float(gold["eval_state_estimator"])
    d = (sm.net_q(sm.net_s(z.cuda()).contiguous())[0].cpu() - q_ref).abs().max().item()
    got = sm({"z": z.clone(), "state": given.clone()}, mode="eval_state_estimator")
    assert got.shape == () and got.dtype == torch.float32 and got.is_cuda
    bound = 2 * d * float((given - q_ref).abs().mean()) + d * d + ULP * abs(want)
    print(f"eval_state_estimator {float(got):.8f} reference {want:.8f} d {d:.3e} bound {bound:.3e}")
    assert abs(float(got) - want) <= bound
    with pytest.raises(NotImplementedError):
        sm({"z": z.clone(), "state": given.clone()}, mode="state_estimator")


def test_seeded_stft_model_draws_the_reference_values(gold):
    """`StftModel` builds net_e, net_d, net_q in the reference's order: under the same seed the decoder and the codebook hold the
    values the reference's own StftModel holds, bit for bit (the decoder sits between the two, so net_q depends on the order)."""
    from ccvs_amd.models.skip_vid_generator.models.stft_model import StftModel
    torch.manual_seed(0)
    sm = StftModel(_parse(rh.TINY_STATE_ARGV)["stft_ae"], is_train=False, is_main=True).eval()
    for net, pre in ((sm.net_e, "ae"), (sm.net_d, "ad"), (sm.net_q, "aq")):
        keys = [k for k in gold.files if k.startswith(f"model_seed0/{pre}/")]
        assert keys, pre
        for k in keys:
            assert np.array_equal(net.state_dict()[k[len(f"model_seed0/{pre}/"):]].cpu().numpy(), gold[k]), k


# ------------------------------------------------------------------ 10. Drums geometry
def test_drums_geometry_against_the_cpu_composition():
    """Transposed 3x3 layers at widths 2 / 4 / 8 and 512 channels, the head at C = 512 on 64 x 16 pixels."""
    from ccvs_amd.tools.options import DRUMS_ARGV
    from ccvs_amd.models.skip_vid_generator.models.stft_model import StftModel
    aopt = _parse(list(DRUMS_ARGV))["stft_ae"]
    assert (aopt.stft_num, aopt.stft_size, aopt.stft_hsize, list(aopt.stft_shape)) == (1024, 512, 512, [8, 2])
    torch.manual_seed(0)
    sm = StftModel(aopt, is_train=False, is_main=True).eval()
    cpu = lambda m: {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    nets = {"ad": cpu(sm.net_d), "aq": cpu(sm.net_q)}
    R.condition_weights(None, nets["ad"], nets["aq"], 4.0, 77)
    codes = torch.randint(0, aopt.stft_num, (2, 3 * 16), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        for _ in range(4):   # as the fixture script does: the last layer doubles until the reference output is large enough
            want = R.stft_decode(nets, aopt.stft_shape, codes, "vid")
            if R.well_conditioned(want):
                break
            nets["ad"]["convs.4.0.weight"].mul_(2.0)
    _load(sm.net_d, nets["ad"])
    _load(sm.net_q, nets["aq"])
    assert want.shape == (2, 3, 1, 64, 16) and R.well_conditioned(want), (float(want.abs().max()), float((want.abs() > 0.5).float().mean()))
    got = sm({"state_code": codes.clone()}, mode="vid_decoder")["stft"].cpu()
    assert got.shape == want.shape
    per_frame = (got - want).abs().amax(dim=(2, 3, 4))
    print("Drums-size decoder, per-frame max|diff|:", [f"{v:.3e}" for v in per_frame.flatten().tolist()])
    assert float(per_frame.max()) <= 1e-3


# ------------------------------------------------------------------ 11. the generator surface
def _tiny_generator(extra):
    from ccvs_amd.helpers.generator import Generator
    torch.manual_seed(0)
    opt = _parse(rh.TINY_STATE_ARGV + ["--x_sample_noise", "device"] + extra)
    xopt = opt["transformer"]
    xopt.sample, xopt.top_k, xopt.sample_state = False, 10, False
    gen = Generator(opt).build_models()
    with torch.no_grad():
        z_e, _ = gen.vid_model.net_e(gen.synthetic_batch(2)["vid"].cuda())
        cb = gen.vid_model.net_q.embedding.weight
        cb.copy_(torch.randn(cb.shape, generator=torch.Generator().manual_seed(4)).cuda() * z_e.std())
        gen.transformer_model.net_t.s_emb.normal_(0, 0.02)
        gen.transformer_model.net_t.t_emb.normal_(0, 0.02)
        gen.transformer_model.net_t.state_s_emb.normal_(0, 0.02)
        sds = {k: {n: v.detach().cpu().clone() for n, v in getattr(gen.stft_model, "net_" + k[1]).state_dict().items()} for k in ("ae", "ad", "aq")}
        R.condition_weights(sds["ae"], sds["ad"], sds["aq"], 4.0, 9, last_factor=16.0)
        for k in ("ae", "ad", "aq"):
            _load(getattr(gen.stft_model, "net_" + k[1]), sds[k])
    return gen


def _tiny_batches(gen, n):
    out = []
    for i in range(n):
        g = torch.Generator().manual_seed(60 + i)
        level = (torch.rand(2, 4, 1, 2, 1, generator=g) * 2 - 1).repeat_interleave(8, dim=-2).repeat_interleave(8, dim=-1)
        out.append({"vid": gen.synthetic_batch(2, seed=50 + i)["vid"], "stft": (0.8 * level + 0.2 * (torch.rand(2, 4, 1, 16, 8, generator=g) * 2 - 1))})
    return out


def _clone(d):
    return {k: v.clone() for k, v in d.items()}


@pytest.mark.parametrize("keep_state", [False, True])
def test_generator_decode_stft_all_schedules(keep_state):
    extra = ["--keep_state"] if keep_state else []
    gen = _tiny_generator(extra + ["--decode_stft"])
    batches = _tiny_batches(gen, 3)
    serial = [gen.generate_vid(_clone(b), global_iter=i, schedule="serial") for i, b in enumerate(batches)]
    torch.cuda.synchronize()
    for b, out in zip(batches, serial):
        fake, rec = out["fake"], out["rec"]
        assert fake["stft"].shape == (2, 4, 1, 16, 8) and fake["stft"].dtype == torch.float32 and float(fake["stft"].abs().max()) < 1
        assert rec["stft"].shape == (2, 4, 1, 16, 8)
        want = gen.stft_model({"state_code": fake["state_code"].clone()}, mode="vid_decoder")["stft"]
        assert torch.equal(fake["stft"], want)
        given = gen.stft_model({"stft": b["stft"].clone()}, mode="vid_encoder")["state_code"]
        assert torch.equal(rec["stft"], gen.stft_model({"state_code": given}, mode="vid_decoder")["stft"])
        if keep_state:
            assert torch.equal(fake["state_code"], given) and torch.equal(fake["stft"], rec["stft"])
        else:   # the conditioning tokens, then predicted ones
            n_cond = int(gen.opt.cond_len / (64 * 4) * given.size(1))
            assert torch.equal(fake["state_code"][:, :n_cond], given[:, :n_cond]) and fake["state_code"].shape == given.shape
    assert float(serial[0]["fake"]["stft"].abs().max()) > 0.05, "conditioned weights: the decoded spectrogram is not flat"
    stream = [gen.generate_vid(_clone(b), global_iter=i, schedule="stream") for i, b in enumerate(batches)]
    piped = gen.run_pipelined((_clone(b) for b in batches), rec_pass=True)
    torch.cuda.synchronize()
    assert len(piped) == 3
    for want, a, b in zip(serial, stream, piped):
        for got in (a, b):
            assert torch.equal(got["fake"]["state_code"], want["fake"]["state_code"])
            assert torch.equal(got["fake"]["stft"], want["fake"]["stft"]) and torch.equal(got["rec"]["stft"], want["rec"]["stft"])
            assert torch.equal(got["fake"]["vid"], want["fake"]["vid"]) and torch.equal(got["rec"]["vid"], want["rec"]["vid"])
    # without the flag: no key anywhere, the same clips
    gen_off = _tiny_generator(extra)
    for i, b in enumerate(batches[:2]):
        for schedule in ("serial", "stream"):
            out = gen_off.generate_vid(_clone(b), global_iter=i, schedule=schedule)
            torch.cuda.synchronize()
            assert "stft" not in out["fake"] and "stft" not in out["rec"] and "stft" not in out
            assert torch.equal(out["fake"]["vid"], serial[i]["fake"]["vid"]) and torch.equal(out["rec"]["vid"], serial[i]["rec"]["vid"])
            assert torch.equal(out["fake"]["state_code"], serial[i]["fake"]["state_code"])
    for out in gen_off.run_pipelined((_clone(b) for b in batches), rec_pass=True):
        assert "stft" not in out["fake"] and "stft" not in out["rec"]


@pytest.mark.parametrize("mode", ["serial", "pipelined"])
def test_run_writes_the_spectrograms(tmp_path, monkeypatch, mode):
    from ccvs_amd.helpers.generator import Generator
    monkeypatch.setenv("CCVS_RUN_SCHEDULE", mode)
    feed = {}

    def next_batch(self, data_info):     # the synthetic loader has no sound: add a seeded spectrogram per batch
        i = feed.setdefault(id(self), 0)
        feed[id(self)] = i + 1
        data = next(data_info["loader_iter"])
        data["stft"] = torch.rand(2, 4, 1, 16, 8, generator=torch.Generator().manual_seed(80 + i)) * 2 - 1
        return data

    monkeypatch.setattr(Generator, "next_batch", next_batch)
    seen = {}
    real_save = Generator.save_results

    def save_results(self, out, global_iter):
        seen[global_iter] = {k: out[k]["stft"].detach().cpu().numpy() for k in ("fake", "rec") if isinstance(out.get(k), dict) and "stft" in out[k]}
        return real_save(self, out, global_iter)

    monkeypatch.setattr(Generator, "save_results", save_results)
    roots = {}
    for flag in (True, False):
        argv = rh.TINY_STATE_ARGV + ["--n_iter", "3", "--save_path", str(tmp_path / f"{mode}_{flag}")] + (["--decode_stft"] if flag else [])
        torch.manual_seed(0)
        opt = _parse(argv)
        torch.manual_seed(9)
        Generator(opt).run()
        roots[flag] = opt["transformer"].result_path
        if flag:
            assert sorted(seen) == [0, 1, 2]
            for kind in ("fake", "rec"):
                names = sorted(os.listdir(os.path.join(roots[flag], kind + "_stft")))
                assert names == [os.path.splitext(n)[0] + ".npy" for n in sorted(os.listdir(os.path.join(roots[flag], kind)))] and len(names) == 6
                for j, name in enumerate(names):
                    arr = np.load(os.path.join(roots[flag], kind + "_stft", name))
                    assert arr.dtype == np.float32 and arr.shape == (4, 16, 8)
                    assert np.array_equal(arr, seen[j // 2][kind][j % 2, :, 0])
            seen_on = dict(seen)
            seen.clear()
        else:
            assert all(v == {} for v in seen.values())
            assert not [d for d in os.listdir(roots[flag]) if d.endswith("_stft")]
    # the flag adds work, it moves nothing: the clips' files are the same bytes
    for kind in ("real", "fake", "rec"):
        for name in sorted(os.listdir(os.path.join(roots[True], kind))):
            a, b = (open(os.path.join(roots[f], kind, name), "rb").read() for f in (True, False))
            assert a == b, (kind, name)
    assert seen_on

"""-m gpu: the FVD pipeline on the GPU against the host mirrors of tests/fvd_ref.py, with random weights (the
pretrained ones are never in the repository).  Every op writes into NaN-filled outputs.

  1. `ops.fvd_prep` bit for bit against the numpy fp32 mirror; `ops.time_unfold` and `ops.maxpool3d_same` exact against the torch
     mirrors, at the sizes where their code takes another path (16-byte and 4-byte rows, borders, strided channel slices, two clips);
     `ops.i3d_head` against float64 within 1e-12 (|W| . mean|x| + |b|) per element -- both sides add the same at most 1024 x 98 fp32
     terms in float64 and differ in summation order only -- and the same bits when run twice (measured: 2.3e-16);
  2. the whole embedding against the float64 mirror: every width / 8 (2 clips, T = 9, 16, 17, 197 x 224 and 224 x 224) and the true
     widths (1 clip, T = 9, 193 x 193), in both precisions.  Bars on the worst error relative to the clip's largest |logit|: "f32" 20 x
     what torch's own fp32 CPU evaluation of the same network shows against the mirror (6.5e-7 over the six / 8 cases, 3.4e-7 at the
     true widths: 1.3e-5 and 6.8e-6; the factor allows another summation order), split-bf16 the project's 1e-4;
  3. equal real and fake clips give embeddings with the same bits and an FVD of 0; `fvd_from_videos` against the mirror's embeddings
     pushed through the reference's formula; T = 8 and missing weights raise; `main` on a tiny results/ tree of .avi files.
"""
import os
import sys
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fvd_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

BAR_SMALL = {"f32": 20 * 6.5e-7, None: 1e-4}
BAR_FULL = {"f32": 20 * 3.4e-7, None: 1e-4}
SMALL_CASES = [(t, hw) for t in (9, 16, 17) for hw in ((197, 224), (224, 224))]
FORMS = (((1, 3, 3), (1, 2, 2)), ((3, 3, 3), (2, 2, 2)), ((2, 2, 2), (2, 2, 2)), ((3, 3, 3), (1, 1, 1)), ((1, 3, 3), (1, 1, 1)))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ccvs_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def small_weights():
    return R.random_weights(11, 8)


@pytest.fixture(scope="module")
def small_models(ops, small_weights):
    from ccvs_amd.tools.tf_fvd.i3d import I3D, divided_widths
    return {prec: I3D(small_weights, prec, widths=divided_widths(8)) for prec in (None, "f32")}


@pytest.fixture(scope="module")
def small_mirror(small_weights):
    """{(T, (H, W)): (clips, the mirror's float64 embedding)}, each computed once on first use and left unchanged."""
    cache = {}

    def get(t, hw):
        if (t, hw) not in cache:
            x = R.clips((2, t, 3, *hw), 30 + SMALL_CASES.index((t, hw)))
            cache[t, hw] = (x, R.features(x, small_weights, 8))
        return cache[t, hw]
    return get


@pytest.fixture
def fvd(monkeypatch):
    from ccvs_amd.tools.tf_fvd import fvd as _fvd
    monkeypatch.delenv("CCVS_FVD_WEIGHTS", raising=False)
    _fvd.set_fvd_weights(None)
    yield _fvd
    _fvd.set_fvd_weights(None)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _same(got, want):
    return got.shape == want.shape and torch.allclose(got, want, rtol=0, atol=0, equal_nan=True)


def _rel(got, want):
    """The worst error over the clips, relative to each clip's largest |logit|."""
    return ((got - want).abs().amax(dim=1) / want.abs().amax(dim=1)).max().item()


# ------------------------------------------------------------------ 1: the ops
@pytest.mark.parametrize("h,w", [(64, 64), (224, 224), (256, 256), (37, 45)])
def test_fvd_prep_bit_for_bit(ops, h, w):
    for frames in (1, 5):
        u8 = torch.randint(0, 256, (1, frames, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(h + frames))
        for flip in (False, True):
            out = _nan(1, frames, 3, 224, 224)
            assert ops.fvd_prep(u8.cuda(), (224, 224), flip=flip, out=out) is out
            want = R.preprocess_np(u8.numpy(), (224, 224), flip=flip)
            assert np.array_equal(out.cpu().numpy(), want), (h, w, frames, flip)
    # rows that are no multiple of four pixels take the element-by-element form
    u8 = torch.randint(0, 256, (2, 9, 11, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    out = _nan(2, 3, 13, 10)
    ops.fvd_prep(u8.cuda(), (13, 10), out=out)
    assert np.array_equal(out.cpu().numpy(), R.preprocess_np(u8.numpy(), (13, 10)))


@pytest.mark.parametrize("kt,st,t", [(7, 2, 16), (7, 2, 9), (3, 1, 2), (3, 1, 3), (3, 1, 5)])
def test_time_unfold_exact(ops, kt, st, t):
    assert R.same_pad(t, kt, st)[1:] == {(7, 2, 16): (2, 3), (7, 2, 9): (3, 3)}.get((kt, st, t), (1, 1))
    for c in (3, 16, 24):
        for h, w in ((7, 7), (5, 13), (4, 28)):            # 4 x 28: whole 16-byte quads per plane; the others element by element
            g = torch.Generator().manual_seed(1000 * t + 10 * c + w)
            wide = torch.randn(2 * t, c + 8, h, w, generator=g)          # two clips: a lane that reached across clips would show
            wide[1, 5, 0, 0] = float("nan")
            for sliced in (False, True):                                # a channel-slice view is read in place
                host = wide[:, 4:4 + c] if sliced else wide[:, 4:4 + c].contiguous()
                dev = wide.cuda()[:, 4:4 + c] if sliced else host.cuda()
                assert dev.is_contiguous() != sliced
                for pad in ((0, 0, 0, 0), (2, 3, 2, 3)):
                    for relu in (False, True):
                        want = R.time_unfold(host, t, kt, st, pad, relu)
                        out = _nan(*want.shape)
                        assert ops.time_unfold(dev, t, kt, st, pad=pad, relu=relu, out=out) is out
                        assert _same(out.cpu(), want), (kt, st, t, c, h, w, sliced, pad, relu)
                        assert int(torch.isnan(want).sum()) >= 1
                for relu in (False, True):                              # the four pixel phases as channels, on bordered frames of even sides
                    pad = (2, 3 + (h + 5) % 2, 2, 3 + (w + 5) % 2)
                    want = R.time_unfold(host, t, kt, st, pad, relu, phases=2)
                    out = _nan(*want.shape)
                    assert ops.time_unfold(dev, t, kt, st, pad=pad, relu=relu, phases=2, out=out) is out
                    assert want.shape[1] == 4 * kt * c and _same(out.cpu(), want), (kt, st, t, c, h, w, sliced, pad, relu)


@pytest.mark.parametrize("kernel,stride", FORMS)
def test_maxpool3d_same_exact(ops, kernel, stride):
    for t in (1, 2, 3, 5):
        for h, w in ((7, 7), (13, 13), (14, 28)):
            g = torch.Generator().manual_seed(100 * t + w)
            x = torch.randn(2 * t, 3, h, w, generator=g)
            neg = -0.5 - x.abs()                                        # all negative: a padding that won would show as 0
            for src, relu in ((x, False), (x, True), (neg, False)):
                want = R.maxpool(src, t, kernel, stride, relu)
                out = _nan(*want.shape)
                assert ops.maxpool3d_same(src.cuda(), t, kernel, stride, relu=relu, out=out) is out
                assert _same(out.cpu(), want), (kernel, stride, t, h, w, relu)
            assert (R.maxpool(neg, t, kernel, stride) < -0.5).all()
            assert _same(ops.maxpool3d_same(x.cuda(), t, kernel, stride, relu=True).cpu(), R.maxpool(F.relu(x), t, kernel, stride)), "ReLU on read is ReLU, then the pool"
            x[t, 1, 3, 3] = float("nan")                                # in the second clip's first frame
            want = R.maxpool(x, t, kernel, stride, True)
            got = ops.maxpool3d_same(x.cuda(), t, kernel, stride, relu=True).cpu()
            assert _same(got, want) and torch.isnan(got).any() and not torch.isnan(got[:got.shape[0] // 2]).any()


@pytest.mark.parametrize("c", [1024, 128])
def test_i3d_head_vs_float64(ops, c):
    worst = 0.0
    for t in (2, 3):
        for n in (1, 3):
            g = torch.Generator().manual_seed(10 * t + n + c)
            x = torch.randn(n * t, c, 7, 7, generator=g)
            w = torch.randn(400, c, generator=g) / c ** 0.5
            b = 0.05 * torch.randn(400, generator=g)
            for relu in (False, True):
                src = F.relu(x) if relu else x
                want = R.head(src, t, w, b)
                scale = R.head(src.abs(), t, w.abs(), b.abs())          # |W| . mean|x| + |b|, per element
                out = _nan(n, 400, dtype=torch.float64)
                assert ops.i3d_head(x.cuda(), t, w.cuda(), b.cuda(), relu=relu, out=out) is out
                got = out.cpu()
                err = ((got - want).abs() / scale).max().item()
                worst = max(worst, err)
                assert err <= 1e-12, (c, t, n, relu, err)
                assert torch.equal(ops.i3d_head(x.cuda(), t, w.cuda().view(400, c, 1, 1, 1), b.cuda(), relu=relu).cpu(), got), "the same bits on every run"
    print(f"i3d_head C={c}: worst error {worst:.3e} of |W| . mean|x| + |b|")
    with pytest.raises(ValueError, match="7 x 7"):
        ops.i3d_head(torch.zeros(2, c, 7, 8).cuda(), 2, w.cuda(), b.cuda())


# ------------------------------------------------------------------ 2: the whole embedding
@pytest.mark.parametrize("precision", ["f32", None])
@pytest.mark.parametrize("t,hw", SMALL_CASES)
def test_embedding_reduced_widths_vs_mirror(small_models, small_mirror, t, hw, precision):
    """Measured on an MI355X, worst error relative to the clip's largest |logit| over the six cases: "f32" 3.5e-7 (bar 1.3e-5), split-bf16
    1.0e-5 (bar 1e-4)."""
    x, want = small_mirror(t, hw)
    got = small_models[precision].features(x.cuda())
    assert got.dtype == torch.float64 and got.is_cuda and got.shape == (2, 400)
    err = _rel(got.cpu(), want)
    print(f"i3d / 8 T={t} {hw[0]} x {hw[1]} precision={precision or 'bf16x3'}: error {err:.3e} of the largest |logit| (bar {BAR_SMALL[precision]:.1e})")
    assert err <= BAR_SMALL[precision], (t, hw, precision, err)
    assert 1 < want.abs().max() < 10


@pytest.fixture(scope="module")
def full_case():
    weights = R.random_weights(12, 1)
    x = R.clips((1, 9, 3, 193, 193), 40)
    t0 = time.time()
    want = R.features(x, weights)
    print(f"float64 mirror of the true-width network, 1 clip of 9 frames at 193 x 193: {time.time() - t0:.1f} s on the host")
    return weights, x, want


@pytest.mark.parametrize("precision", ["f32", None])
def test_embedding_true_widths_vs_mirror(ops, full_case, precision):
    """The mirror (float64 conv3d on the host) takes 0.2 to 0.5 s for this case.  Measured on an MI355X: "f32" 4.2e-7 (bar 6.8e-6),
    split-bf16 6.4e-6 (bar 1e-4)."""
    from ccvs_amd.tools.tf_fvd.i3d import I3D
    weights, x, want = full_case
    got = I3D(weights, precision).features(x.cuda()).cpu()
    err = _rel(got, want)
    print(f"i3d true widths T=9 193 x 193 precision={precision or 'bf16x3'}: error {err:.3e} of the largest |logit| (bar {BAR_FULL[precision]:.1e})")
    assert got.shape == (1, 400) and err <= BAR_FULL[precision], (precision, err)


def test_clip_sizes_raise(small_models):
    model = small_models[None]
    for shape in ((1, 8, 3, 224, 224), (1, 9, 3, 192, 224), (1, 9, 3, 224, 225)):
        with pytest.raises(ValueError):
            model.features(torch.zeros(shape).cuda())
    with pytest.raises(ValueError):
        model.features(torch.zeros(1, 9, 224, 224, 3).cuda())
    with pytest.raises(Exception, match="device tensors"):
        model.features(torch.zeros(1, 9, 3, 224, 224))


# ------------------------------------------------------------------ 3: the distance and the glue
def _clips_u8(seed, n=32, t=9, side=64):
    """Real clips, and fake ones of lower contrast with noise added: the embeddings' means and covariances both move, and the distance
    (about 16 with the / 8 random network, against a trace of 0.13) is no small difference of large terms."""
    g = torch.Generator().manual_seed(seed)
    real = torch.randint(0, 256, (n, t, side, side, 3), generator=g, dtype=torch.uint8)
    fake = (0.6 * real.float() + 40 + 10 * torch.randn(real.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    return real, fake


def _mirror_embed(u8, weights, flip):
    """The mirror in fp32 on the host: within 6.5e-7 of its float64 form (the module's docstring), against a bar of 1e-4; in float64
    these 64 clips at 224 x 224 would take the host 16 s, in fp32 they take 2."""
    x = torch.from_numpy(R.preprocess_np(u8.numpy(), (224, 224), flip=flip))         # [N, T, 3, 224, 224]
    return torch.cat([R.features(x[i:i + 16], weights, 8, torch.float32) for i in range(0, len(x), 16)]).double().numpy()


def test_fvd_from_videos_vs_mirror(fvd, small_models, small_weights):
    """32 + 32 clips of 9 frames at 64 x 64 through the / 8 network in its default precision; the mirror's embeddings go through the
    reference's own formula (scipy) where scipy imports, else through numpy's.  Measured on an MI355X: 15.68796 against the mirror's
    15.68784, a relative 7.5e-6 (bar 1e-4)."""
    real, fake = _clips_u8(3)
    with pytest.raises(NotImplementedError):
        fvd.fvd_from_videos(real, fake)
    fvd.set_fvd_weights(small_models[None])
    got = fvd.fvd_from_videos(real.numpy(), fake, channel_order="bgr")
    try:
        import scipy  # noqa: F401
        frechet = R.frechet_scipy
    except ImportError:
        from ccvs_amd.tools.utils import calculate_frechet_distance as frechet
    want = R.fvd_numpy(_mirror_embed(real, small_weights, True), _mirror_embed(fake, small_weights, True), frechet)
    print(f"fvd_from_videos: {got!r} against the mirror's {want!r}, relative error {abs(got - want) / want:.3e}")
    assert want > 0 and abs(got - want) <= 1e-4 * want
    rgb = fvd.fvd_from_videos(real, fake, channel_order="rgb")
    assert rgb > 0 and rgb != got, "the other channel order is another figure"
    # equal clips: the same bits, and a distance of 0
    e1, e2 = fvd.emb_from_videos(real, real.clone())
    assert e1.dtype == np.float64 and e1.shape == (32, 400) and np.array_equal(e1, e2)
    assert abs(fvd.compute_fvd_given_acts(e1, e2)) <= 1e-9 * np.trace(np.cov(e1, rowvar=False))
    assert abs(fvd.fvd_from_videos(real, real)) <= 1e-9 * np.trace(np.cov(e1, rowvar=False))
    # the reference's own two steps give the same embedding
    x = fvd.preprocess(real[:2], (224, 224))
    assert x.shape == (2, 9, 3, 224, 224) and torch.equal(fvd.create_id3_embedding(x).cpu(), torch.from_numpy(e1[:2]))
    with pytest.raises(ValueError, match="at least 9"):
        fvd.fvd_from_videos(real[:, :8], fake[:, :8])
    with pytest.raises(ValueError, match="batches of 16"):
        fvd.fvd_from_videos(real[:15], fake[:15])
    fvd.set_fvd_weights(None)
    with pytest.raises(NotImplementedError):
        fvd.fvd_from_videos(real, fake)


def test_main_on_avi_files(fvd, small_models, tmp_path, monkeypatch, capsys):
    from ccvs_amd.helpers.generator import save_video_batch
    real, fake = _clips_u8(4)
    for kind, clips in (("real", real), ("fake", fake)):
        d = tmp_path / "results" / "0001_fv" / kind
        os.makedirs(d)
        vid = clips.cuda().permute(0, 1, 4, 2, 3).float() / 255
        save_video_batch(vid, 32, 0, str(d), 4, True, False, [0, 1], "kinetics600", video_format="avi", return_clip=False)
    monkeypatch.chdir(tmp_path)
    files = fvd.get_video_files(os.path.join("results", "0001_fv", "real"))
    assert len(files) == 32 and files[0].endswith(".avi")
    with pytest.raises(NotImplementedError):
        fvd.main(fvd.parse_args(["--exp_tag", "fv"]))
    fvd.set_fvd_weights(small_models[None])
    capsys.readouterr()
    fvd.main(fvd.parse_args(["--exp_tag", "fv", "--mode", "both", "--size", "16"]))
    lines = capsys.readouterr().out.splitlines()
    assert "Found 32 real video files" in lines and "Found 32 fake video files" in lines and "Computing FVD with both mode" in lines
    # what the files hold (JPEG is lossy: the clips are read back) through fvd_from_videos
    real_back = fvd.load_videos(files, None, 1)
    fake_back = fvd.load_videos(fvd.get_video_files(os.path.join("results", "0001_fv", "fake")), None, 1)
    assert real_back.shape == real.shape and real_back.dtype == torch.uint8
    re_, fe_ = fvd.emb_from_videos(real_back, fake_back)
    sizes = [fvd.compute_fvd_given_acts(re_[i:i + 16], fe_[i:i + 16]) for i in (0, 16)]
    at = lines.index("Individual FVD scores")
    assert lines[at + 1] == str(sizes) and lines[at + 2] == "Mean/std of FVD across 2 runs of size 16" and lines[at + 3] == f"{np.mean(sizes)} {np.std(sizes)}"
    assert lines[at + 4] == f"FVD score: {fvd.fvd_from_videos(real_back, fake_back)}"
    with pytest.raises(NotImplementedError, match="resize"):
        fvd.main(fvd.parse_args(["--exp_tag", "fv", "--resize", "64", "64"]))

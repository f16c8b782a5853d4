"""-m gpu: LPIPS from user-supplied weights on the GPU against the float64 mirror tests/lpips_ref.py, with
random weights at VGG16's true widths (the pretrained ones are never in the repository).

  1. the new ops -- ccvs_relu_, ccvs_relu_maxpool2, ccvs_lpips_layer (and ccvs_lpips_prep, bit for bit against torch's fp32) -- against
     float64, into NaN-filled outputs, at the sizes where their code takes another path; the float64 reductions within a relative
     1e-12 (both sides reduce the same fp32 inputs in float64 and differ in summation order only) and the same bits when run twice;
  2. the whole distance against the mirror: 4 pairs at 32 x 32, 2 pairs at 37 x 45 (odd pools; block 5 on 2 x 2), 2 pairs at 96 x 128
     (aligned wide rows), in both precisions, with the chunk forced to one pair and left at its default.  Bars on the worst per-image
     relative error, their basis measured on a CPU at these shapes: "f32" 5e-6 (torch's own fp32 evaluation of the network is within
     2.4e-7 of the mirror: 20 x for the kernel's other summation order), split-bf16 1e-4 (a torch emulation hi*hi + hi*lo + lo*hi with
     fp32 accumulation is within 3.8e-6; the project's parity bar leaves 25 x);
  3. per_image(x, x) is exactly 0, per_image(x, y) = per_image(y, x) within those bars, get_lpips is the mean of per_image;
  4. the glue: metrics_from_videos / metrics_from_files / main / --print_256 with weights set, and the state without weights after
     `set_lpips_weights(None)`.

Errors measured on the GPU are recorded in DESIGN.md section 4.19.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lpips_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = {"f32": 5e-6, None: 1e-4}
SHAPES = ((4, 32, 32), (2, 37, 45), (2, 96, 128))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ccvs_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def weights():
    return R.random_weights(11)


@pytest.fixture(scope="module")
def models(ops, weights):
    """{(precision, forced one-pair chunks)}: the four networks, packed once."""
    from ccvs_amd.tools.pytorch_metrics.lpips import LPIPS
    return {(prec, one): (LPIPS(weights, prec, max_workspace_bytes=1) if one else LPIPS(weights, prec)) for prec in (None, "f32") for one in (False, True)}


@pytest.fixture(scope="module")
def cases(weights):
    """{shape: (x, y, the mirror's float64 per-image distances)}, computed once and left unchanged."""
    out = {}
    for k, (n, h, w) in enumerate(SHAPES):
        x, y = R.pair((n, 3, h, w), 20 + k)
        out[n, h, w] = (x, y, R.per_image(x, y, weights))
    return out


@pytest.fixture
def M():
    """The metrics module; whatever a test configures is gone afterwards, so that the "not available" tests of other files see no weights."""
    from ccvs_amd.tools.pytorch_metrics import metrics
    metrics.set_lpips_weights(None)
    yield metrics
    metrics.set_lpips_weights(None)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


# ------------------------------------------------------------------ 1: the ops
@pytest.mark.parametrize("n", [1, 5, 4099])
def test_relu_in_place(ops, n):
    g = torch.Generator().manual_seed(n)
    for offset in (4, 1):   # a 16-byte aligned base (quads + tail), and one that is not (element by element)
        host = torch.randn(n + 8, generator=g)
        host[offset] = -host[offset].abs()
        if n >= 5:
            host[offset + 1], host[offset + 2], host[offset + 3] = float("nan"), float("-inf"), float("inf")
        buf = host.cuda()
        assert buf.data_ptr() % 16 == 0
        x = buf[offset:offset + n]
        assert ops.relu_(x) is x
        want = host.clone().double()
        want[offset:offset + n] = torch.where(want[offset:offset + n] < 0, torch.zeros((), dtype=torch.float64), want[offset:offset + n])
        got = buf.cpu().double()
        assert torch.allclose(got, want, rtol=0, atol=0, equal_nan=True), (n, offset)      # the elements around the slice are untouched
        assert int(torch.isnan(got).sum()) == (1 if n >= 5 else 0)


def test_lpips_prep_is_torchs_fp32(ops):
    for shape, offset in (((2, 3, 32, 32), 0), ((1, 3, 5, 7), 0), ((2, 3, 8, 8), 1)):   # quads, elements, quads refused by an unaligned base
        x = torch.rand(*shape, generator=torch.Generator().manual_seed(shape[-1]))
        n = x.numel()
        xb = torch.zeros(n + 4, device="cuda")
        xd = xb[offset:offset + n].view(shape)
        xd.copy_(x)
        out = _nan(n + 4)[offset:offset + n].view(shape)
        assert ops.lpips_prep(xd, out=out) is out
        want = (x - torch.tensor(R.MEAN).view(1, 3, 1, 1)) / torch.tensor(R.STD).view(1, 3, 1, 1)
        assert torch.equal(out.cpu(), want), shape


@pytest.mark.parametrize("c", [3, 64])
def test_relu_maxpool2(ops, c):
    for h, w, offset in ((2, 2, 0), (5, 7, 0), (16, 12, 0), (16, 12, 1)):   # (16 x 12: two pixels per lane; not from an unaligned base)
        g = torch.Generator().manual_seed(100 * h + w + c)
        x = torch.randn(2, c, h, w, generator=g)
        x[0, 0, :2, :2] = -x[0, 0, :2, :2].abs() - 0.5          # a window whose maximum is negative: 0 comes out
        x[1, c - 1, 0, 1] = float("nan")                        # a NaN in a window comes out
        xb = torch.zeros(x.numel() + 4, device="cuda")
        xd = xb[offset:offset + x.numel()].view(x.shape)
        xd.copy_(x)
        out = _nan(2, c, h // 2, w // 2)
        assert ops.relu_maxpool2(xd, out=out) is out
        want = F.max_pool2d(F.relu(x.double()), 2, 2)
        got = out.cpu().double()
        assert want[0, 0, 0, 0] == 0 and torch.isnan(want[1, c - 1, 0, 0]) and int(torch.isnan(want).sum()) == 1
        assert torch.allclose(got, want, rtol=0, atol=0, equal_nan=True), (h, w, offset)
        assert int(torch.isnan(got).sum()) == 1, "every output is written"


@pytest.mark.parametrize("c", [24, 64, 512])
def test_lpips_layer_vs_float64(ops, c):
    worst = 0.0
    for hw in (1, 4, 63, 64, 65, 1024, 1024 + 3):       # (1024: several tiles of the four-positions-per-lane form; 1027: of the one-position form)
        for m in (1, 3):
            g = torch.Generator().manual_seed(1000 * c + 10 * hw + m)
            f = torch.randn(2 * m, c, hw, generator=g)             # pre-activations: half of them negative
            f[0, :, 0] = -f[0, :, 0].abs()                         # all zero behind the ReLU in x only ...
            if hw > 1:
                f[0, :, 1] = -f[0, :, 1].abs()                     # ... and in both images
                f[m, :, 1] = -f[m, :, 1].abs()
            w = torch.rand(c, generator=g)
            w[1] = -0.3                                            # one negative head weight
            for relu in (True, False):
                a, b = f[:m].double().unsqueeze(-1), f[m:].double().unsqueeze(-1)
                want = R.layer_distance(F.relu(a), F.relu(b), w) if relu else R.layer_distance(a, b, w)
                assert torch.isfinite(want).all() and (want > 0).all()
                out = _nan(m, dtype=torch.float64)
                assert ops.lpips_layer(f.cuda(), w.cuda(), relu=relu, out=out) is out
                got = out.cpu()
                err = ((got - want).abs() / want).max().item()
                worst = max(worst, err)
                assert err <= 1e-12, (c, hw, m, relu, got, want)
                assert torch.equal(ops.lpips_layer(f.cuda(), w.cuda().view(1, c, 1, 1), relu=relu).cpu(), got), "the same bits on every run"
            twice = ops.lpips_layer(f.cuda(), w.cuda(), relu=True, out=got.cuda(), accumulate=True).cpu()      # got: the relu=False result
            assert ((twice - (got + R.layer_distance(F.relu(a), F.relu(b), w))).abs() / twice).max() <= 1e-12
    print(f"lpips_layer C={c}: worst relative error {worst:.3e}")


# ------------------------------------------------------------------ 2: the whole distance
@pytest.mark.parametrize("precision", ["f32", None])
@pytest.mark.parametrize("shape", SHAPES)
def test_distance_vs_mirror(models, cases, shape, precision):
    """Measured on an MI355X, worst per-image relative error (one pair per chunk and the default chunk gave the same bits):
    "f32" 5.4e-7 at 32 x 32, 2.8e-7 at 37 x 45, 7.8e-8 at 96 x 128 (bar 5e-6); split-bf16 2.2e-6, 4.8e-6, 1.4e-6 (bar 1e-4)."""
    x, y, want = cases[shape]
    got = {}
    for one in (True, False):
        model = models[precision, one]
        assert model.chunk_pairs(*shape[1:]) == (1 if one else (2 << 30) // (1024 * shape[1] * shape[2]))
        d = model.per_image(x.cuda(), y.cuda())
        assert d.dtype == torch.float64 and d.is_cuda and d.shape == (shape[0],)
        got[one] = d.cpu()
        err = ((got[one] - want).abs() / want).max().item()
        print(f"lpips {shape} precision={precision or 'bf16x3'} one_pair_chunks={one}: worst relative error {err:.3e} (bar {BAR[precision]:.0e}), scores {want.tolist()}")
        assert err <= BAR[precision], (shape, precision, one, got[one], want)
    assert 0.02 < want.min() and want.max() < 0.5


def test_default_chunk_is_32_pairs_at_256(models):
    assert models[None, False].chunk_pairs(256, 256) == 32 and models[None, True].chunk_pairs(256, 256) == 1


# ------------------------------------------------------------------ 3: exactness and bookkeeping
@pytest.mark.parametrize("precision", ["f32", None])
def test_equal_images_swapped_images_and_the_mean(models, cases, weights, M, precision):
    x, y, want = cases[2, 37, 45]
    for one in (True, False):
        model = models[precision, one]
        assert torch.equal(model.per_image(x.cuda(), x.clone().cuda()).cpu(), torch.zeros(2, dtype=torch.float64)), "both halves pass through the same launches"
        xy, yx = model.per_image(x.cuda(), y.cuda()).cpu(), model.per_image(y.cuda(), x.cuda()).cpu()
        assert ((xy - yx).abs() / want).max() <= BAR[precision]
        mean = model(x.cuda(), y.cuda())
        assert mean.is_cuda and mean.dtype == torch.float32 and mean.dim() == 0 and mean.item() == xy.mean().float().item()
    if precision is None:
        M.set_lpips_weights(weights)
        got = M.get_lpips(x.cuda(), y.cuda())
        assert got.is_cuda and got.dim() == 0 and abs(got.item() - xy.mean().item()) <= 1e-6 * xy.mean().item()
    with pytest.raises(ValueError, match="under 32"):
        models[precision, False].per_image(torch.zeros(1, 3, 31, 64).cuda(), torch.zeros(1, 3, 31, 64).cuda())
    with pytest.raises(Exception, match="device tensors"):
        models[precision, False].per_image(x, y)


# ------------------------------------------------------------------ 4: the glue
def _clips(seed, n=32, t=3, side=32):
    g = torch.Generator().manual_seed(seed)
    real = torch.randint(0, 256, (n, t, side, side, 3), generator=g, dtype=torch.uint8)
    fake = (real.float() + 12 * torch.randn(real.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    return real, fake


def test_metrics_from_videos_with_weights(M, weights):
    """The mean over the two batches of the mirror's per-batch means, within the split-bf16 bar (the default precision).  The frames
    behind `upscale` are 161 x 161: there the mirror runs in fp32 on the host (within 2.4e-7 of its float64 form, section 2 above; in
    float64 those 128 frames would take the host a minute).  Measured on an MI355X: 1.1e-6 for every frame, 9.1e-7 and 8.9e-7 behind
    `upscale`."""
    real, fake = _clips(4)
    assert M.metrics_from_videos(real, fake)[0] is None
    M.set_lpips_weights(weights)
    lp, ssim, psnr = M.metrics_from_videos(real.numpy(), fake.numpy())
    nchw = lambda v: (v / 255).reshape(-1, 32, 32, 3).permute(0, 3, 1, 2)
    want = torch.stack([R.lpips(nchw(real[16 * i:16 * i + 16]), nchw(fake[16 * i:16 * i + 16]), weights) for i in range(2)]).mean().item()
    print(f"metrics_from_videos: lpips {lp.item():.9f}, mirror {want:.9f}, relative error {abs(lp.item() - want) / want:.3e}")
    assert abs(lp.item() - want) <= BAR[None] * want
    assert np.isfinite(ssim.item()) and np.isfinite(psnr.item())
    lp_k, ssim_k, _ = M.metrics_from_videos(real, fake, idx=[0, 2])
    assert len(lp_k) == len(ssim_k) == 2
    up = lambda v, t: F.interpolate((v[:, t] / 255).permute(0, 3, 1, 2), size=[161, 161], mode="bilinear")
    for k, t in enumerate([0, 2]):
        want_k = torch.stack([R.lpips(up(real[16 * i:16 * i + 16], t), up(fake[16 * i:16 * i + 16], t), weights, torch.float32) for i in range(2)]).mean().item()
        print(f"metrics_from_videos idx {t}: lpips {lp_k[k].item():.9f}, mirror {want_k:.9f}, relative error {abs(lp_k[k].item() - want_k) / want_k:.3e}")
        assert abs(lp_k[k].item() - want_k) <= BAR[None] * want_k
    M.set_lpips_weights(None)
    assert M.metrics_from_videos(real, fake)[0] is None
    with pytest.raises(NotImplementedError):
        M.get_lpips(None, None)


def test_main_and_print_256_with_weights(M, weights, tmp_path, monkeypatch, capsys):
    real, fake = _clips(5, n=16)
    for kind, clips in (("real", real), ("fake", fake)):
        d = tmp_path / "results" / "0001_lp" / kind
        os.makedirs(d)
        for i in range(16):
            np.save(d / f"vid_{i:05d}.npy", clips[i].numpy())
    path = tmp_path / "lpips_vgg16.pt"
    torch.save(weights, path)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("CCVS_LPIPS_WEIGHTS", raising=False)
    M.main(M.parse_args(["--exp_tag", "lp"]))
    assert "LPIPS scores: not available (needs pretrained weights)" in capsys.readouterr().out.splitlines()
    M.main(M.parse_args(["--exp_tag", "lp", "--lpips_weights", str(path)]))
    lines = capsys.readouterr().out.splitlines()
    at = lines.index("Mean/std of LPIPS across 1 runs")
    assert lines[at - 2] == "Individual LPIPS scores" and "Individual SSIM scores" in lines and not any("not available" in s for s in lines)
    lp, _, _ = M.metrics_from_videos(real, fake)
    assert lines[at + 1] == f"{np.mean([lp])!s} {np.std([lp])!s}" and 0.01 < lp.item() < 1
    M.main(M.parse_args(["--exp_tag", "lp", "--idx", "0", "2"]))
    lines = capsys.readouterr().out.splitlines()
    assert "Individual LPIPS-0 scores" in lines and "Mean/std of LPIPS-1 across 1 runs" in lines
    # the environment variable names the file when nothing else does; it is read on first use
    M.set_lpips_weights(None)
    monkeypatch.setenv("CCVS_LPIPS_WEIGHTS", str(path))
    x, y = R.pair((2, 3, 32, 32), 6)
    assert M.get_lpips(x.cuda(), y.cuda()).item() > 0
    monkeypatch.delenv("CCVS_LPIPS_WEIGHTS")
    M.set_lpips_weights(None)
    with pytest.raises(NotImplementedError):
        M.get_lpips(None, None)
    # --print_256: the reference's full line, all three metrics
    M.set_lpips_weights(str(path))
    big_r, big_f = _clips(7, n=512, t=1)      # two groups of 256 clips: the standard deviations over the groups exist
    capsys.readouterr()
    lp, ssim, psnr = M.metrics_from_videos(big_r, big_f, print_256=True, batch_size=128)
    line = capsys.readouterr().out.splitlines()[-1]
    assert line.startswith(f"(256) LPIPS is: {lp} (+- ") and f"), SSIM is {ssim} (+- " in line and f"), PSNR is {psnr} (+- " in line

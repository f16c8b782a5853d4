"""not gpu: the deblurring mode's host side -- the plain-torch stand-in for torchvision's GaussianBlur (tests/golden/blur_ref.py) pinned
against hand-written arithmetic, the kernel-size rule, the sigma draw, and construction of the generator and transformer with
`--x_deblurring` (`--layout` still raises, and so does `--step_by_step` with the mode)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import blur_ref  # noqa: E402
import ref_harness as rh  # noqa: E402

DEBLUR_FLAGS = ["--x_deblurring", "--x_state_size", "64", "--x_state_num", "1024"]


def test_kernel_size_rule():
    want = {1: 3, 2: 7, 3: 9, 4: 13, 5: 13, 6: 13, 7: 13, 8: 13, 9: 13, 10: 13, 11: 13, 12: 13}
    for s, k in want.items():
        assert blur_ref.kernel_size(s) == k, s
    from ccvs_amd.helpers.generator import blur_kernel_size
    for s in range(1, 13):
        assert blur_kernel_size(s) == blur_ref.kernel_size(s)


@pytest.mark.parametrize("k,sigma", [(3, 1.0), (7, 2.0), (9, 3.0), (13, 4.0), (13, 10.0)])
def test_weights_symmetric_normalised(k, sigma):
    w = blur_ref.gaussian_kernel1d(k, sigma)
    assert w.dtype == torch.float32 and w.shape == (k,)
    assert torch.equal(w, w.flip(0))
    assert abs(w.double().sum().item() - 1.0) < 1e-6
    assert bool((w[: k // 2] < w[1: k // 2 + 1]).all())
    x = np.linspace(-(k - 1) / 2, (k - 1) / 2, k)
    pdf = np.exp(-0.5 * (x / sigma) ** 2)
    np.testing.assert_allclose(w.numpy(), pdf / pdf.sum(), rtol=1e-6, atol=0)
    from ccvs_amd import ops
    assert torch.equal(ops.gaussian_kernel1d(k, sigma), w)


def test_constant_image_unchanged():
    img = torch.full((2, 3, 16, 20), 0.375)
    for k in (3, 7, 9, 13):
        out = blur_ref.gaussian_blur(img, k, 10.0)
        assert out.shape == img.shape
        assert (out - img).abs().max().item() < 1e-6


def _numpy_reflect_conv(x, k, sigma):
    """Reflect padding and the 2-D filter written out by hand, in float64 with the float32 weights."""
    w = blur_ref.gaussian_kernel1d(k, sigma).double().numpy()
    r = k // 2
    h, wd = x.shape

    def refl(i, n):
        return -i if i < 0 else (2 * (n - 1) - i if i >= n else i)

    out = np.zeros((h, wd))
    for y in range(h):
        for xx in range(wd):
            acc = 0.0
            for i in range(k):
                for j in range(k):
                    acc += w[i] * w[j] * x[refl(y + i - r, h), refl(xx + j - r, wd)]
            out[y, xx] = acc
    return out


@pytest.mark.parametrize("k,sigma,h,w", [(3, 1.0, 5, 6), (7, 2.0, 9, 8), (13, 10.0, 7, 7), (13, 4.0, 15, 14)])
def test_reflect_convolution_by_hand(k, sigma, h, w):
    x = torch.rand(1, 1, h, w, generator=torch.Generator().manual_seed(k + h)) * 2 - 1
    want = _numpy_reflect_conv(x[0, 0].double().numpy(), k, sigma)
    got64 = blur_ref.gaussian_blur(x, k, sigma, dtype=torch.float64)[0, 0].numpy()
    np.testing.assert_allclose(got64, want, rtol=0, atol=1e-12)            # every pixel, the border rows and columns included
    got32 = blur_ref.gaussian_blur(x, k, sigma)[0, 0].double().numpy()
    np.testing.assert_allclose(got32, want, rtol=0, atol=2e-6)


def test_reflect_needs_larger_plane():
    with pytest.raises(RuntimeError):
        blur_ref.gaussian_blur(torch.zeros(1, 1, 6, 6), 13, 4.0)


def test_one_generator_draw_per_call():
    img = torch.rand(2, 3, 8, 8)
    torch.manual_seed(5)
    blur_ref.GaussianBlur(7, 2)(img)
    after = torch.rand(4)
    torch.manual_seed(5)
    torch.empty(1).uniform_(2.0, 2.0)
    assert torch.equal(torch.rand(4), after)
    torch.manual_seed(5)
    assert not torch.equal(torch.rand(4), after)
    torch.manual_seed(5)
    blur_ref.GaussianBlur(7, 2)(img)
    blur_ref.GaussianBlur(7, 2)(img)
    two = torch.rand(4)
    torch.manual_seed(5)
    torch.empty(1).uniform_(2.0, 2.0)
    torch.empty(1).uniform_(2.0, 2.0)
    assert torch.equal(torch.rand(4), two)
    assert torch.empty(1).uniform_(10.0, 10.0).item() == 10.0


def _opt(extra):
    from ccvs_amd.tools.options import Options
    return Options().parse(load_qvid_generator=True, load_transformer=True, argv=rh.TINY_ARGV + extra)


def test_generator_accepts_deblurring():
    from ccvs_amd.helpers.generator import Generator
    opt = _opt(DEBLUR_FLAGS)
    xopt = opt["transformer"]
    assert xopt.deblurring and xopt.state_size == 64 and xopt.state_num == 1024 and xopt.blur_sigma == 10
    gen = Generator(opt)
    assert gen.opt.deblurring
    assert not gen._host_noise_streams_ok()                                # an ancillary stream: the inline noise path


def test_transformer_constructs_with_deblurring(monkeypatch):
    monkeypatch.setattr(torch.nn.Module, "cuda", lambda self, *a, **k: self)
    from ccvs_amd.models.skip_vid_generator.models.transformer_model import Transformer
    xopt = _opt(DEBLUR_FLAGS)["transformer"]
    tr = Transformer(xopt, is_train=False, is_main=True)
    net = tr.net_t
    assert tuple(net.state_s_emb.shape) == (1, 64, xopt.n_embd)
    assert net.tok_emb.weight.shape[0] == xopt.z_num
    assert net.state_tok_emb.weight.shape[0] == 1024


def test_layout_and_step_by_step_still_raise():
    from ccvs_amd.helpers.generator import Generator
    with pytest.raises(NotImplementedError):
        Generator(_opt(["--layout"]))
    with pytest.raises(NotImplementedError):
        Generator(_opt(DEBLUR_FLAGS + ["--step_by_step"]))


def test_fixture_bytes_follow_from_what_is_stored():
    """tests/golden/tiny_deblur.npz keeps neither the input clip, nor the blurred clip, nor the uint8 files the reference wrote: the
    input is regenerated from its seed, the blurred clip is `blur_ref.blur` of it, and every file the reference wrote -- real and blur
    of every run, fake and rec where the fixture holds the float clips -- has the digest of `pack_u8_reference` of its float clip."""
    import json
    from make_golden_deblur import blur_sigma_of, digest, input_clip, pack_u8_reference
    meta = json.load(open(os.path.join(HERE, "golden", "tiny_deblur.json")))
    gold = np.load(os.path.join(HERE, "golden", "tiny_deblur.npz"))
    vid = input_clip()
    assert digest(vid) == meta["vid_sha256"]
    checked = 0
    for case, spec in meta["cases"].items():
        clips = {"real": vid, "blur": blur_ref.blur(vid, blur_sigma_of(spec["flags"]))}
        for mode, files in spec["files"].items():
            have = dict(clips)
            if f"{case}/{mode}/fake" in gold.files:
                have["fake"] = torch.from_numpy(gold[f"{case}/{mode}/fake"])
                have["rec"] = torch.from_numpy(gold[f"{case}/rec"])
            assert sorted({rel.split("/")[0] for rel in files}) == ["blur", "fake", "real", "rec"]
            for rel, sha in files.items():
                sub, base = rel.split("/")
                if sub in have:
                    assert digest(pack_u8_reference(have[sub])[int(base[len("vid_"):-len(".mp4")])]) == sha, (case, mode, rel)
                    checked += 1
    assert checked == 2 * 2 * 2 * 2 + 2 * 2 * 2   # real + blur: 2 cases x 2 runs x 2 clips; fake + rec: the whole-sequence case

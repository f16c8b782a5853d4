"""Host tests of the FVD pipeline: everything that needs no GPU.

  1. the float64 mirror tests/fvd_ref.py against an independently written module-by-module build (nn.Conv3d / nn.MaxPool3d modules with
     the PyTorch ports' own padding rule and zero-padded pools) and against hand-computed SAME paddings for n = 224, 193, 16, 9 at every
     (k, s) the network uses; the clip sizes the network accepts;
  2. the stacked-channel identity -- a k_t-tap 3-D convolution is a 2-D convolution over time-stacked frames -- against F.conv3d for the
     7^3 stride-2 stem and a 3^3 unit; the mirror's pool propagates a NaN and never lets the padding win;
  3. the numpy fp32 mirror of the preprocess: known answers at identity size and at a 2 x upscale, the channel flip;
  4. the loader and the converter: a synthetic state dict in the port's layout round-trips, the folded BatchNorm equals BatchNorm applied
     after the convolution, a missing key and a wrong shape are named;
  5. the state without weights; the command's arguments; `--resize` raises;
  6. `lib.FVD_EXPORTS` equals what include/ccvs_hip_fvd.h declares, the built library exports it, the lists are disjoint, the ABI is 6,
     bad arguments are refused before any launch;
  7. `calculate_frechet_distance` (numpy only) against a closed form, and against the reference's scipy formula where scipy imports:
     full rank (1024 and 2048 samples of 400 dimensions) within a relative 1e-9, rank-deficient (256 samples, the reference's default
     `--size`) within 1e-6.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import fvd_ref as R  # noqa: E402


@pytest.fixture
def fvd(monkeypatch):
    from ccvs_amd.tools.tf_fvd import fvd as _fvd
    monkeypatch.delenv("CCVS_FVD_WEIGHTS", raising=False)
    _fvd.set_fvd_weights(None)
    yield _fvd
    _fvd.set_fvd_weights(None)


# ------------------------------------------------------------------ 1: the mirror
HAND_PADS = {   # (n, k, s): (out, before, after), worked out by hand from out = ceil(n / s), total = max((out - 1) s + k - n, 0)
    (224, 7, 2): (112, 2, 3), (224, 3, 2): (112, 0, 1), (224, 3, 1): (224, 1, 1), (224, 2, 2): (112, 0, 0), (224, 1, 1): (224, 0, 0), (224, 1, 2): (112, 0, 0),
    (193, 7, 2): (97, 3, 3), (193, 3, 2): (97, 1, 1), (193, 3, 1): (193, 1, 1), (193, 2, 2): (97, 0, 1), (193, 1, 1): (193, 0, 0), (193, 1, 2): (97, 0, 0),
    (16, 7, 2): (8, 2, 3), (16, 3, 2): (8, 0, 1), (16, 3, 1): (16, 1, 1), (16, 2, 2): (8, 0, 0), (16, 1, 1): (16, 0, 0), (16, 1, 2): (8, 0, 0),
    (9, 7, 2): (5, 3, 3), (9, 3, 2): (5, 1, 1), (9, 3, 1): (9, 1, 1), (9, 2, 2): (5, 0, 1), (9, 1, 1): (9, 0, 0), (9, 1, 2): (5, 0, 0),
}


def test_same_padding_by_hand():
    from ccvs_amd import ops
    for (n, k, s), want in HAND_PADS.items():
        assert R.same_pad(n, k, s) == want, (n, k, s)
        assert ops.same_pad(n, k, s) == want, (n, k, s)
    x = torch.zeros(1, 1, 9, 193, 224)
    assert R.pad_same(x, (7, 7, 7), (2, 2, 2), 0.0).shape == (1, 1, 15, 199, 229)
    assert R.pad_same(x, (1, 3, 3), (1, 2, 2), 0.0).shape == (1, 1, 9, 195, 225)


class _Unit(nn.Module):
    """A unit as the PyTorch ports write it: padding computed per axis in forward, by their rule."""

    def __init__(self, cin, cout, k, stride=1, bias=False, relu=True):
        super().__init__()
        self.k, self.s, self.relu = k, stride, relu
        self.conv3d = nn.Conv3d(cin, cout, k, stride=stride, padding=0, bias=bias).double()

    def _pad(self, n):
        return max(self.k - self.s, 0) if n % self.s == 0 else max(self.k - n % self.s, 0)

    def forward(self, x):
        pads = []
        for n in reversed(x.shape[2:]):
            p = self._pad(n)
            pads += [p // 2, p - p // 2]
        y = self.conv3d(F.pad(x, pads))
        return F.relu(y) if self.relu else y


class _Pool(nn.Module):
    """The ports' MaxPool3dSamePadding: zero padding (its inputs are behind a ReLU)."""

    def __init__(self, k, s):
        super().__init__()
        self.k, self.s = k, s
        self.pool = nn.MaxPool3d(k, s, padding=0)

    def forward(self, x):
        pads = []
        for n, k, s in zip(reversed(x.shape[2:]), reversed(self.k), reversed(self.s)):
            p = max(k - s, 0) if n % s == 0 else max(k - n % s, 0)
            pads += [p // 2, p - p // 2]
        return self.pool(F.pad(x, pads))


class _Mixed(nn.Module):
    def __init__(self, cin, o):
        super().__init__()
        self.b0, self.b1a, self.b1b = _Unit(cin, o[0], 1), _Unit(cin, o[1], 1), _Unit(o[1], o[2], 3)
        self.b2a, self.b2b = _Unit(cin, o[3], 1), _Unit(o[3], o[4], 3)
        self.b3a, self.b3b = _Pool((3, 3, 3), (1, 1, 1)), _Unit(cin, o[5], 1)

    def forward(self, x):
        return torch.cat([self.b0(x), self.b1b(self.b1a(x)), self.b2b(self.b2a(x)), self.b3b(self.b3a(x))], dim=1)


def _independent(weights, div):
    d = lambda c: c // div
    layers = [
        ("Conv3d_1a_7x7", _Unit(3, d(64), 7, 2)), ("MaxPool3d_2a_3x3", _Pool((1, 3, 3), (1, 2, 2))), ("Conv3d_2b_1x1", _Unit(d(64), d(64), 1)),
        ("Conv3d_2c_3x3", _Unit(d(64), d(192), 3)), ("MaxPool3d_3a_3x3", _Pool((1, 3, 3), (1, 2, 2))),
        ("Mixed_3b", _Mixed(d(192), [d(c) for c in (64, 96, 128, 16, 32, 32)])), ("Mixed_3c", _Mixed(d(256), [d(c) for c in (128, 128, 192, 32, 96, 64)])),
        ("MaxPool3d_4a_3x3", _Pool((3, 3, 3), (2, 2, 2))),
        ("Mixed_4b", _Mixed(d(128 + 192 + 96 + 64), [d(c) for c in (192, 96, 208, 16, 48, 64)])),
        ("Mixed_4c", _Mixed(d(192 + 208 + 48 + 64), [d(c) for c in (160, 112, 224, 24, 64, 64)])),
        ("Mixed_4d", _Mixed(d(160 + 224 + 64 + 64), [d(c) for c in (128, 128, 256, 24, 64, 64)])),
        ("Mixed_4e", _Mixed(d(128 + 256 + 64 + 64), [d(c) for c in (112, 144, 288, 32, 64, 64)])),
        ("Mixed_4f", _Mixed(d(112 + 288 + 64 + 64), [d(c) for c in (256, 160, 320, 32, 128, 128)])),
        ("MaxPool3d_5a_2x2", _Pool((2, 2, 2), (2, 2, 2))),
        ("Mixed_5b", _Mixed(d(256 + 320 + 128 + 128), [d(c) for c in (256, 160, 320, 32, 128, 128)])),
        ("Mixed_5c", _Mixed(d(256 + 320 + 128 + 128), [d(c) for c in (384, 192, 384, 48, 128, 128)])),
    ]
    net = nn.ModuleDict(dict(layers))
    net["logits"] = _Unit(d(384 + 384 + 128 + 128), 400, 1, bias=True, relu=False)
    sd = {}
    for k, v in weights.items():
        unit, kind = k.rsplit(".", 1)
        if unit == "logits" and kind == "weight":
            v = v.reshape(400, -1, 1, 1, 1)
        sd[f"{unit}.conv3d.{kind}"] = v.double()
    for name, m in net.named_modules():      # the folded offset is the convolution's bias here
        if isinstance(m, _Unit) and m.conv3d.bias is None:
            m.conv3d.bias = nn.Parameter(torch.zeros(m.conv3d.out_channels, dtype=torch.float64))
    net.load_state_dict(sd)
    return net, [n for n, _ in layers]


def test_mirror_equals_an_independent_build():
    assert len(R.unit_shapes()[0]) == 57 and R.unit_shapes()[1] == 1024
    weights = R.random_weights(3, 8)
    net, order = _independent(weights, 8)
    x = R.clips((1, 9, 3, 193, 200), 5)
    taps = {}
    want = R.features(x, weights, 8, taps=taps)
    with torch.no_grad():
        h = x.double().permute(0, 2, 1, 3, 4)
        for name in order:
            h = net[name](h)
            if name in taps:
                assert h.shape == taps[name].shape and torch.allclose(h, taps[name], rtol=1e-12, atol=1e-12), name
        assert h.shape == (1, 128, 2, 7, 7)
        got = net["logits"](F.avg_pool3d(h, (2, 7, 7), stride=1)).squeeze(3).squeeze(3).mean(2)
    assert got.shape == want.shape == (1, 400)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    assert 0.5 < want.abs().max() < 20 and taps["Mixed_5c"].mean() > 0.1, "the random weights keep the activations O(1)"


def test_clip_sizes():
    from ccvs_amd.tools.tf_fvd.i3d import I3D
    for t, h, w in ((9, 193, 193), (16, 224, 224), (40, 224, 193)):
        I3D.check_clip(t, h, w)
    for t, h, w in ((8, 224, 224), (16, 192, 224), (16, 224, 225), (16, 64, 64)):
        with pytest.raises(ValueError):
            I3D.check_clip(t, h, w)
    time = lambda t: R.same_pad(R.same_pad(R.same_pad(t, 7, 2)[0], 3, 2)[0], 2, 2)[0]
    side = lambda n: R.same_pad(R.same_pad(R.same_pad(R.same_pad(R.same_pad(n, 7, 2)[0], 3, 2)[0], 3, 2)[0], 3, 2)[0], 2, 2)[0]
    assert time(16) == 2 and time(9) == 2 and time(8) == 1 and time(17) == 3
    assert [side(n) for n in (192, 193, 224, 225)] == [6, 7, 7, 8]


# ------------------------------------------------------------------ 2: the stacked-channel identity
@pytest.mark.parametrize("k,stride,cin,cout,t,h,w", [(7, 2, 3, 8, 16, 20, 23), (7, 2, 3, 8, 9, 21, 20), (3, 1, 6, 5, 5, 9, 11), (3, 1, 4, 5, 2, 7, 7)])
def test_conv3d_is_conv2d_over_time_stacked_frames(k, stride, cin, cout, t, h, w):
    from ccvs_amd import ops
    g = torch.Generator().manual_seed(k * 100 + t)
    x = torch.randn(2, t, cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cout, cin, k, k, k, generator=g, dtype=torch.float64)
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    want = R.conv_same(x.permute(0, 2, 1, 3, 4), wt, b, stride).permute(0, 2, 1, 3, 4)          # [2, To, cout, Ho, Wo]
    (_, hb, ha), (_, wb, wa) = R.same_pad(h, k, stride), R.same_pad(w, k, stride)
    u = R.time_unfold(x.reshape(2 * t, cin, h, w), t, k, stride, pad=(hb, ha, wb, wa))
    got = F.conv2d(u, R.stack_weight(wt), b, stride=stride)
    assert got.shape == (2 * want.shape[1], cout, *want.shape[3:])
    assert torch.allclose(got, want.reshape(got.shape), rtol=1e-12, atol=1e-12)
    if stride == 2:
        # the stride in the channels too: one more zero row / column where the bordered side is odd, the four pixel phases as channels,
        # and a stride-1 convolution with ceil(k / 2) taps a side -- the form the stem runs in (and `ops.stack_conv3d_weight` packs)
        ha, wa = ha + (h + hb + ha) % 2, wa + (w + wb + wa) % 2
        u2 = R.time_unfold(x.reshape(2 * t, cin, h, w), t, k, stride, pad=(hb, ha, wb, wa), phases=2)
        assert u2.shape == (got.shape[0], 4 * k * cin, (h + hb + ha) // 2, (w + wb + wa) // 2)
        w2 = R.stack_weight(wt, phases=2)
        assert w2.shape == (cout, 4 * k * cin, 4, 4) and torch.equal(w2, ops.stack_conv3d_weight(wt, phases=2))
        got2 = F.conv2d(u2, w2, b)
        assert got2.shape == got.shape and torch.allclose(got2, got, rtol=1e-12, atol=1e-12)
    assert torch.equal(R.stack_weight(wt), ops.stack_conv3d_weight(wt))


def test_mirror_pool_padding_never_wins_and_nan_comes_out():
    x = -1 - torch.rand(6, 2, 5, 5, dtype=torch.float64)          # two clips of three frames, all negative
    for kernel, stride in (((1, 3, 3), (1, 2, 2)), ((3, 3, 3), (2, 2, 2)), ((2, 2, 2), (2, 2, 2)), ((3, 3, 3), (1, 1, 1)), ((1, 3, 3), (1, 1, 1))):
        y = R.maxpool(x, 3, kernel, stride)
        assert (y < -1).all(), "a zero padding would have won"
        assert (R.maxpool(x, 3, kernel, stride, relu=True) == 0).all()
    x[4, 1, 2, 2] = float("nan")
    y = R.maxpool(x, 3, (3, 3, 3), (1, 1, 1))
    assert torch.isnan(y[3:, 1, 1:4, 1:4]).all() and int(torch.isnan(y).sum()) == 27 and not torch.isnan(y[:3]).any(), "the NaN stays inside its clip"


# ------------------------------------------------------------------ 3: the preprocess
def test_preprocess_mirror_known_answers():
    g = np.random.default_rng(0)
    u8 = g.integers(0, 256, (2, 3, 8, 6, 3), dtype=np.uint8)
    same = R.preprocess_np(u8, (8, 6))
    want = (np.float32(2) * u8.astype(np.float32)) / np.float32(255) - np.float32(1)
    assert same.dtype == np.float32 and same.shape == (2, 3, 3, 8, 6) and np.array_equal(same, np.moveaxis(want, -1, -3))
    assert np.array_equal(R.preprocess_np(u8, (8, 6), flip=True), same[:, :, ::-1])
    up = R.preprocess_np(u8, (16, 12))
    v = np.moveaxis(u8.astype(np.float64), -1, -3)                                       # [2, 3, 3, 8, 6]
    rows = np.stack([v[..., i // 2, :] if i % 2 == 0 else (v[..., i // 2, :] + v[..., min(i // 2 + 1, 7), :]) / 2 for i in range(16)], axis=-2)
    both = np.stack([rows[..., j // 2] if j % 2 == 0 else (rows[..., j // 2] + rows[..., min(j // 2 + 1, 5)]) / 2 for j in range(12)], axis=-1)
    assert np.array_equal(both * 4, np.round(both * 4)), "halves and quarters of integers: exact in fp32"
    assert np.array_equal(up, (np.float32(2) * both.astype(np.float32)) / np.float32(255) - np.float32(1))
    assert np.array_equal(up[..., ::2, ::2], same), "even positions are the source pixels"
    assert up.min() >= -1 and up.max() <= 1


# ------------------------------------------------------------------ 4: the loader and the converter
def test_fold_load_and_convert_round_trip(tmp_path):
    from ccvs_amd.tools.tf_fvd import i3d
    widths = i3d.divided_widths(8)
    convs, (cin, classes) = i3d.units(widths)
    assert [(n, a, b, k) for n, a, b, k in convs] == R.unit_shapes(8)[0] and (cin, classes) == (128, 400)
    assert i3d.units()[0] == R.unit_shapes(1)[0] and len(i3d.units()[0]) == 57 and i3d.units()[1] == (1024, 400)
    sd = R.random_port_state_dict(4, 8)
    folded = i3d.fold_state_dict(sd, widths)
    assert sorted(folded) == sorted(R.random_weights(0, 8))
    # the folded unit equals BatchNorm (eps 1e-3, running statistics) applied after the convolution
    x = torch.randn(1, 12, 3, 5, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(1))     # Mixed_3b.b1b reads 96 / 8 channels
    name = "Mixed_3b.b1b"
    bn = nn.BatchNorm3d(16, eps=1e-3).double().eval()
    bn.load_state_dict({k: sd[f"{name}.bn.{k}"].double() if k != "num_batches_tracked" else sd[f"{name}.bn.{k}"] for k in bn.state_dict()})
    with torch.no_grad():
        want = bn(F.conv3d(x, sd[f"{name}.conv3d.weight"].double(), padding=1))
    got = F.conv3d(x, folded[f"{name}.weight"].double(), folded[f"{name}.bias"].double(), padding=1)
    assert (got - want).abs().max() <= 1e-6 * want.abs().max()                   # (the folded weights are rounded to fp32)
    # the loader takes the folded dict and the file the converter writes; the port's own dict is sent to the converter
    a = i3d.load_i3d_weights(folded, widths)
    with pytest.raises(ValueError, match="convert it"):
        i3d.load_i3d_weights(sd, widths)
    src, dst = tmp_path / "port.pt", tmp_path / "i3d.pt"
    torch.save(sd, src)
    c = i3d.convert(str(src), str(dst), widths)
    d = i3d.load_i3d_weights(str(dst), widths)
    for k in a:
        assert a[k].dtype == torch.float32 and torch.equal(a[k], folded[k]) and torch.equal(a[k], c[k]) and torch.equal(a[k], d[k]), k
    assert a["logits.weight"].shape == (400, 128)
    args = i3d.parse_args(["--state_dict", "a.pt", "--out", "b.pt"])
    assert (args.state_dict, args.out) == ("a.pt", "b.pt")
    # what is wrong is named
    missing = {k: v for k, v in sd.items() if k != "Mixed_4e.b2a.bn.running_var"}
    with pytest.raises(ValueError, match=r"Mixed_4e\.b2a\.bn\.running_var"):
        i3d.fold_state_dict(missing, widths)
    wrong = dict(folded)
    wrong["Mixed_5b.b3b.weight"] = torch.zeros(16, 104, 3, 3, 3)
    with pytest.raises(ValueError, match=r"Mixed_5b\.b3b\.weight is \(16, 104, 3, 3, 3\), not \(16, 104, 1, 1, 1\)"):
        i3d.load_i3d_weights(wrong, widths)
    with pytest.raises(ValueError, match=r"Conv3d_1a_7x7\.weight is \(8, 3, 7, 7, 7\), not \(64, 3, 7, 7, 7\)"):
        i3d.load_i3d_weights(folded)                                             # the true widths are the default
    with pytest.raises(ValueError, match="logits.bias"):
        i3d.load_i3d_weights({k: v for k, v in folded.items() if k != "logits.bias"}, widths)
    with pytest.raises(ValueError, match="dict"):
        i3d.load_i3d_weights(_saved(tmp_path, [1, 2]), widths)


def _saved(tmp_path, obj):
    p = tmp_path / "obj.pt"
    torch.save(obj, p)
    return str(p)


# ------------------------------------------------------------------ 5: without weights; the command
def test_without_weights_everything_raises(fvd):
    clips = np.zeros((16, 9, 8, 8, 3), dtype=np.uint8)
    for call in (lambda: fvd.create_id3_embedding(None), lambda: fvd.fvd_from_videos(clips, clips), lambda: fvd.emb_from_videos(clips, clips),
                 lambda: fvd.emb_from_files(["a.avi"] * 16, ["b.avi"] * 16, None, 1)):
        with pytest.raises(NotImplementedError, match="set_fvd_weights, CCVS_FVD_WEIGHTS or --fvd_weights"):
            call()


def test_arguments_and_resize(fvd):
    args = fvd.parse_args(["--exp_tag", "x"])
    assert (args.mode, args.size, args.real_folder, args.fake_folder, args.resize, args.fvd_weights, args.channel_order, args.num_workers) == (
        "size", 256, "real", "fake", None, None, "bgr", 8)
    args = fvd.parse_args(["--exp_tag", "x", "--mode", "both", "--size", "16", "--fvd_weights", "w.pt", "--channel_order", "rgb", "--resize", "64", "64"])
    assert (args.mode, args.size, args.fvd_weights, args.channel_order, args.resize) == ("both", 16, "w.pt", "rgb", [64, 64])
    with pytest.raises(NotImplementedError, match="resize"):
        fvd.load_videos(["a.avi"], [64, 64], 1)
    with pytest.raises(ValueError, match="channel_order"):
        fvd.preprocess(np.zeros((1, 9, 8, 8, 3), dtype=np.uint8), (224, 224), "gbr")


def test_fvd_size_and_full_print_the_references_lines(fvd, capsys):
    g = np.random.default_rng(1)
    real, fake = g.normal(size=(64, 6)), g.normal(size=(64, 6)) + 0.5
    got = fvd.fvd_size(real, fake, 32)
    full = fvd.fvd_full(real, fake)
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "Individual FVD scores" and lines[1] == str(got) and lines[2] == "Mean/std of FVD across 2 runs of size 32"
    assert lines[3] == f"{np.mean(got)} {np.std(got)}" and lines[4] == f"FVD score: {full}"
    assert len(got) == 2 and got[0] == fvd.compute_fvd_given_acts(real[:32], fake[:32]) and full == fvd.compute_fvd_given_acts(torch.from_numpy(real), fake)


# ------------------------------------------------------------------ 6: the C ABI
def test_fvd_symbols_declared_and_exported(tmp_path):
    from ccvs_amd import lib
    header = open(os.path.join(ROOT, "include", "ccvs_hip_fvd.h")).read()
    assert re.search(r'^#include "ccvs_hip_fvd.h"', open(os.path.join(ROOT, "include", "ccvs_hip.h")).read(), re.M)
    declared = sorted(set(re.findall(r"^(?:int64_t|int) (ccvs_[a-zA-Z0-9_]+)\s*\(", header, re.M)))
    assert declared == sorted(lib.FVD_EXPORTS) == ["ccvs_fvd_prep", "ccvs_i3d_head", "ccvs_maxpool3d_same", "ccvs_time_unfold"]
    others = (set(lib.EXPORTS) | set(lib.EVAL_EXPORTS) | set(lib.INPUT_EXPORTS) | set(lib.GEMM_EXPORTS) | set(lib.OUTPUT_EXPORTS) | set(lib.DECODE_EXPORTS)
              | set(lib.VIDEO_EXPORTS) | set(lib.OUTPUT_SAMPLED_EXPORTS) | set(lib.LPIPS_EXPORTS))
    assert not set(lib.FVD_EXPORTS) & others and len(lib.EXPORTS) == 51
    handle = ctypes.CDLL(lib.LIB_PATH)
    for sym in lib.FVD_EXPORTS:
        assert hasattr(handle, sym), sym
    c = tmp_path / "p.c"
    c.write_text('#include "ccvs_hip.h"\nvoid* p[] = {' + ", ".join("(void*)" + s for s in lib.FVD_EXPORTS) + "};\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "p.o")], check=True)
    L = lib.load()
    assert L.ccvs_abi_version() == 6
    # refused before any GPU call
    one = ctypes.c_void_p(16)
    bad = [
        (L.ccvs_fvd_prep(None, one, 1, 8, 8, 224, 224, 0, None), "null pointer"),
        (L.ccvs_fvd_prep(one, one, 0, 8, 8, 224, 224, 0, None), "0 frames"),
        (L.ccvs_time_unfold(one, 64, 16, one, 1, 9, 4, 4, 4, 8, 2, 0, 0, 0, 0, 1, 0, None), "kt 8"),
        (L.ccvs_time_unfold(one, 64, 16, one, 1, 9, 4, 4, 4, 3, 3, 0, 0, 0, 0, 1, 0, None), "st 3"),
        (L.ccvs_time_unfold(one, 64, 8, one, 1, 9, 4, 4, 4, 3, 1, 0, 0, 0, 0, 1, 0, None), "strides"),
        (L.ccvs_time_unfold(one, 64, 16, one, 1, 9, 4, 4, 4, 3, 1, 9, 0, 0, 0, 1, 0, None), "borders"),
        (L.ccvs_time_unfold(one, 64, 16, one, 1, 9, 4, 4, 4, 3, 1, 1, 0, 0, 0, 2, 0, None), "phases"),
        (L.ccvs_time_unfold(one, 64, 16, one, 1, 9, 4, 4, 4, 3, 1, 0, 0, 0, 0, 3, 0, None), "phases"),
        (L.ccvs_maxpool3d_same(one, one, 1, 9, 4, 7, 7, 3, 3, 1, 1, 1, 1, 0, None), "kernel (3,3,1)"),
        (L.ccvs_maxpool3d_same(one, one, 1, 9, 4, 7, 7, 3, 3, 3, 2, 1, 1, 0, None), "stride (2,1,1)"),
        (L.ccvs_maxpool3d_same(one, one, 0, 9, 4, 7, 7, 3, 3, 3, 1, 1, 1, 0, None), "empty tensor"),
        (L.ccvs_i3d_head(one, one, one, one, 1, 1, 128, 49, 400, 0, None), "T 1"),
        (L.ccvs_i3d_head(one, one, one, one, 1, 2, 4097, 49, 400, 0, None), "C 4097"),
        (L.ccvs_i3d_head(one, one, None, one, 1, 2, 128, 49, 400, 0, None), "null pointer"),
    ]
    for rc, _ in bad:
        assert rc != 0
    assert "null pointer" in L.ccvs_last_error().decode()
    assert L.ccvs_time_unfold(one, 64, 16, one, 1, 9, 4, 4, 4, 3, 1, 1, 0, 0, 0, 2, 0, None) != 0 and "phases 2" in L.ccvs_last_error().decode()


# ------------------------------------------------------------------ 7: the Frechet distance
def test_frechet_distance_closed_forms():
    from ccvs_amd.tools.utils import calculate_frechet_distance
    a, b = np.array([4.0, 9.0, 0.0, 1.0]), np.array([1.0, 16.0, 25.0, 0.0])
    m1, m2 = np.array([1.0, 2.0, 3.0, 4.0]), np.array([0.0, 2.0, 5.0, 4.0])
    want = 5.0 + ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()                 # commuting (diagonal) covariances, zero variances included
    assert abs(calculate_frechet_distance(m1, np.diag(a), m2, np.diag(b)) - want) <= 1e-12 * want
    g = np.random.default_rng(2)
    q, _ = np.linalg.qr(g.normal(size=(4, 4)))
    # rotated, the covariances still commute; a zero eigenvalue comes back as a rounding error e, and sqrt(e) ~ 1e-8 is what the
    # square root of a singular matrix can give: the rank-deficient bar is 1e-6
    assert abs(calculate_frechet_distance(m1, q @ np.diag(a) @ q.T, m2, q @ np.diag(b) @ q.T) - want) <= 1e-6 * want
    a, b = a + np.array([0, 0, 2.0, 0]), b + np.array([0, 0, 0, 3.0])
    want = 5.0 + ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()
    assert abs(calculate_frechet_distance(m1, q @ np.diag(a) @ q.T, m2, q @ np.diag(b) @ q.T) - want) <= 1e-12 * want
    s = g.normal(size=(50, 8))
    s = np.cov(s, rowvar=False)
    assert abs(calculate_frechet_distance(m1[:1].repeat(8), s, m1[:1].repeat(8), s)) <= 1e-12 * np.trace(s)


@pytest.mark.parametrize("samples,bar", [(1024, 1e-9), (2048, 1e-9), (256, 1e-6)])
def test_frechet_distance_vs_the_references_scipy_formula(samples, bar):
    """Measured on a CPU: 7e-14 and 8e-14 at full rank; 9.5e-9 with 256 samples of 400 dimensions, where the covariances have rank 255,
    scipy's square root comes out complex and the reference drops the imaginary part."""
    pytest.importorskip("scipy")
    from ccvs_amd.tools.utils import calculate_frechet_distance
    g = np.random.default_rng(samples)
    mix = g.normal(size=(400, 400)) / 20
    real = g.normal(size=(samples, 400)) @ mix + g.normal(size=400)
    fake = 1.1 * g.normal(size=(samples, 400)) @ (mix + g.normal(size=(400, 400)) / 100) + g.normal(size=400)
    want = R.fvd_numpy(real, fake, R.frechet_scipy)
    got = R.fvd_numpy(real, fake, calculate_frechet_distance)
    print(f"frechet {samples} x 400: {got!r} against scipy's {want!r}, relative error {abs(got - want) / want:.3e} (bar {bar:.0e})")
    assert want > 1 and abs(got - want) <= bar * want

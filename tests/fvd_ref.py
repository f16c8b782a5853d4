"""Spec mirror of the FVD pipeline (the reference's tools/tf_fvd/fvd.py and the Kinetics-400 RGB Inception-I3D it loads, restated;
ccvs_amd/tools/tf_fvd/i3d.py states the network) on the host: the network in float64 torch with F.conv3d / F.max_pool3d on explicitly
SAME-padded tensors, the preprocess in numpy fp32 step by step, the reference's Frechet distance with scipy where scipy imports, and a
generator of random folded weights.

The weights are NOT the pretrained ones (those are never in the repository): He initialisation on the folded convolutions,
std = sqrt(2 / (Cin k^3)), offsets 0.05 randn, keeps the activations O(1) through all 57 units; the logits are std = sqrt(1 / Cin).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

STEM = (("Conv3d_1a_7x7", 64, 7, 2), ("Conv3d_2b_1x1", 64, 1, 1), ("Conv3d_2c_3x3", 192, 3, 1))
MIXED = (("Mixed_3b", (64, 96, 128, 16, 32, 32)), ("Mixed_3c", (128, 128, 192, 32, 96, 64)), ("Mixed_4b", (192, 96, 208, 16, 48, 64)),
         ("Mixed_4c", (160, 112, 224, 24, 64, 64)), ("Mixed_4d", (128, 128, 256, 24, 64, 64)), ("Mixed_4e", (112, 144, 288, 32, 64, 64)),
         ("Mixed_4f", (256, 160, 320, 32, 128, 128)), ("Mixed_5b", (256, 160, 320, 32, 128, 128)), ("Mixed_5c", (384, 192, 384, 48, 128, 128)))
CLASSES = 400
# the pools between the blocks: in front of the named block, (kernel, stride)
POOL_BEFORE = {"Conv3d_2b_1x1": ((1, 3, 3), (1, 2, 2)), "Mixed_3b": ((1, 3, 3), (1, 2, 2)), "Mixed_4b": ((3, 3, 3), (2, 2, 2)), "Mixed_5b": ((2, 2, 2), (2, 2, 2))}


def same_pad(n, k, s):
    """TensorFlow's SAME: (out, before, after)."""
    out = math.ceil(n / s)
    total = max((out - 1) * s + k - n, 0)
    return out, total // 2, total - total // 2


def pad_same(x, kernel, stride, value):
    """x [N, C, T, H, W] padded for a SAME window `kernel` / `stride` with `value`."""
    pads = []
    for n, k, s in zip(reversed(x.shape[2:]), reversed(kernel), reversed(stride)):     # F.pad wants the last axis first
        _, before, after = same_pad(n, k, s)
        pads += [before, after]
    return F.pad(x, pads, value=value)


def conv_same(x, w, b, stride):
    k = tuple(w.shape[2:])
    return F.conv3d(pad_same(x, k, (stride,) * 3, 0.0), w, b, stride=stride)


def pool_same(x, kernel, stride):
    """TensorFlow's SAME max pool: the padding never wins."""
    return F.max_pool3d(pad_same(x, kernel, stride, float("-inf")), kernel, stride)


def widths(div=1):
    """(stem widths, mixed widths, classes) with every width divided by `div`."""
    return tuple(c // div for _, c, _, _ in STEM), tuple((name, tuple(c // div for c in o)) for name, o in MIXED), CLASSES


def unit_shapes(div=1):
    """[(unit, Cin, Cout, k)] in network order and the logits' Cin."""
    stem, mixed, _ = widths(div)
    out, cin = [], 3
    for (name, _, k, _), c in zip(STEM, stem):
        out.append((name, cin, c, k))
        cin = c
    for name, o in mixed:
        out += [(f"{name}.b0", cin, o[0], 1), (f"{name}.b1a", cin, o[1], 1), (f"{name}.b1b", o[1], o[2], 3), (f"{name}.b2a", cin, o[3], 1),
                (f"{name}.b2b", o[3], o[4], 3), (f"{name}.b3b", cin, o[5], 1)]
        cin = o[0] + o[2] + o[4] + o[5]
    return out, cin


def random_weights(seed, div=1):
    """The folded weight dict `load_i3d_weights` takes, fp32 from a seed: `<unit>.weight` [Cout, Cin, k, k, k], `<unit>.bias`,
    `logits.weight` [400, C], `logits.bias`."""
    g = torch.Generator().manual_seed(seed)
    shapes, cin = unit_shapes(div)
    w = {}
    for name, ci, co, k in shapes:
        w[f"{name}.weight"] = torch.randn(co, ci, k, k, k, generator=g) * math.sqrt(2.0 / (ci * k ** 3))
        w[f"{name}.bias"] = 0.05 * torch.randn(co, generator=g)
    w["logits.weight"] = torch.randn(CLASSES, cin, generator=g) * math.sqrt(1.0 / cin)
    w["logits.bias"] = 0.05 * torch.randn(CLASSES, generator=g)
    return w


def random_port_state_dict(seed, div=1):
    """A state dict in the PyTorch port's layout (conv3d.weight + bn.*, logits.conv3d.*) with non-trivial BatchNorm statistics."""
    g = torch.Generator().manual_seed(seed)
    shapes, cin = unit_shapes(div)
    sd = {}
    for name, ci, co, k in shapes:
        sd[f"{name}.conv3d.weight"] = torch.randn(co, ci, k, k, k, generator=g) * math.sqrt(2.0 / (ci * k ** 3))
        sd[f"{name}.bn.weight"] = 0.5 + torch.rand(co, generator=g)
        sd[f"{name}.bn.bias"] = 0.1 * torch.randn(co, generator=g)
        sd[f"{name}.bn.running_mean"] = 0.1 * torch.randn(co, generator=g)
        sd[f"{name}.bn.running_var"] = 0.5 + torch.rand(co, generator=g)
        sd[f"{name}.bn.num_batches_tracked"] = torch.tensor(7)
    sd["logits.conv3d.weight"] = torch.randn(CLASSES, cin, 1, 1, 1, generator=g) * math.sqrt(1.0 / cin)
    sd["logits.conv3d.bias"] = 0.05 * torch.randn(CLASSES, generator=g)
    return sd


def features(x, weights, div=1, dtype=torch.float64, taps=None):
    """x [N, T, 3, H, W] in [-1, 1] -> [N, 400], the time-averaged logits, computed in `dtype`.  taps: a dict that receives every
    block's output (behind its ReLU) by name."""
    h = x.to(dtype).permute(0, 2, 1, 3, 4)     # [N, 3, T, H, W]
    W = lambda name: (weights[f"{name}.weight"].to(dtype), weights[f"{name}.bias"].to(dtype))
    unit = lambda v, name, stride=1: F.relu(conv_same(v, *W(name), stride))
    for name, _, _, stride in STEM:
        if name in POOL_BEFORE:
            h = pool_same(h, *POOL_BEFORE[name])
        h = unit(h, name, stride)
        if taps is not None:
            taps[name] = h
    for name, _ in MIXED:
        if name in POOL_BEFORE:
            h = pool_same(h, *POOL_BEFORE[name])
        h = torch.cat([unit(h, f"{name}.b0"), unit(unit(h, f"{name}.b1a"), f"{name}.b1b"), unit(unit(h, f"{name}.b2a"), f"{name}.b2b"),
                       unit(pool_same(h, (3, 3, 3), (1, 1, 1)), f"{name}.b3b")], dim=1)
        if taps is not None:
            taps[name] = h
    assert h.shape[3:] == (7, 7), h.shape
    h = F.avg_pool3d(h, (2, 7, 7), stride=1)                                                                 # VALID: [N, C, T' - 1, 1, 1]
    logits = F.conv3d(h, weights["logits.weight"].to(dtype).reshape(CLASSES, -1, 1, 1, 1), weights["logits.bias"].to(dtype))
    return logits.squeeze(4).squeeze(3).mean(dim=2)


def head(x, t, weight, bias):
    """The head alone in float64: x [N t, C, 7, 7] -> [N, K]."""
    nt, c = x.shape[:2]
    h = x.double().view(nt // t, t, c, 7, 7).permute(0, 2, 1, 3, 4)
    h = F.avg_pool3d(h, (2, 7, 7), stride=1)
    logits = F.conv3d(h, weight.double().reshape(weight.shape[0], c, 1, 1, 1), bias.double())
    return logits.squeeze(4).squeeze(3).mean(dim=2)


def time_unfold(x, t, kt, st=1, pad=(0, 0, 0, 0), relu=False, phases=1):
    """The time-stacked frames a kt-tap convolution reads: x [N t, C, H, W] -> [N To, kt C, H + pt + pb, W + pl + pr]; channel j C + c of
    output frame t' is channel c of the clip's frame t' st + j - before, zeros outside the clip and in the border.  phases=2: the four
    pixel phases of the bordered frame as channels (F.pixel_unshuffle's order), [N To, 4 kt C, Hp / 2, Wp / 2]."""
    nt, c, h, w = x.shape
    n = nt // t
    to, before, after = same_pad(t, kt, st)
    v = F.relu(x) if relu else x
    v = F.pad(v.reshape(n, t, c, h, w), (pad[2], pad[3], pad[0], pad[1], 0, 0, before, after))       # zero frames in front and behind
    frames = [torch.cat([v[:, o * st + j] for j in range(kt)], dim=1) for o in range(to)]             # [n, kt C, Hp, Wp] each
    out = torch.stack(frames, dim=1).reshape(n * to, kt * c, h + pad[0] + pad[1], w + pad[2] + pad[3])
    return out if phases == 1 else F.pixel_unshuffle(out, phases)


def stack_weight(w, phases=1):
    """[Cout, Cin, kt, k, k] -> the 2-D weight [Cout, kt Cin, k, k] over time-stacked channels; phases=2: the weight of the stride-1
    convolution over the four pixel phases that equals the stride-2 one, [Cout, 4 kt Cin, ceil(k / 2), ceil(k / 2)]."""
    co, ci, kt, kh, kw = w.shape
    w2 = w.permute(0, 2, 1, 3, 4).reshape(co, kt * ci, kh, kw)
    if phases == 1:
        return w2
    w2 = F.pad(w2, (0, kw % 2, 0, kh % 2))                   # an even kernel: a zero last tap
    return F.pixel_unshuffle(w2, 2)                          # tap (2 a + py, 2 b + px) of channel q -> tap (a, b) of channel 4 q + 2 py + px


def maxpool(x, t, kernel, stride, relu=False):
    """The SAME max pool on the frames-as-batch layout: x [N t, C, H, W] -> [N To, C, Ho, Wo]."""
    nt, c, h, w = x.shape
    v = (F.relu(x) if relu else x).reshape(nt // t, t, c, h, w).permute(0, 2, 1, 3, 4)
    y = pool_same(v, kernel, stride).permute(0, 2, 1, 3, 4)
    return y.reshape(-1, c, *y.shape[3:])


def preprocess_np(u8, size=(224, 224), flip=False):
    """fvd.py:34-51 in numpy fp32, every step rounded on its own: uint8 [..., H, W, 3] -> fp32 [..., 3, OH, OW]."""
    f32 = np.float32
    u8 = np.asarray(u8)
    h, w = u8.shape[-3:-1]
    oh, ow = size

    def axis(n_in, n_out):
        scale = f32(n_in) / f32(n_out)
        src = np.arange(n_out, dtype=f32) * scale
        i0 = np.floor(src).astype(np.int64)
        i1 = np.minimum(i0 + 1, n_in - 1)
        return i0, i1, (src - i0.astype(f32)).astype(f32)

    y0, y1, fy = axis(h, oh)
    x0, x1, fx = axis(w, ow)
    v = u8.astype(f32)
    if flip:
        v = v[..., ::-1]
    fx = fx[:, None]
    fy = fy[:, None, None]
    tl, tr = v[..., y0, :, :][..., :, x0, :], v[..., y0, :, :][..., :, x1, :]
    bl, br = v[..., y1, :, :][..., :, x0, :], v[..., y1, :, :][..., :, x1, :]
    top = tl + (tr - tl) * fx
    bot = bl + (br - bl) * fx
    out = top + (bot - top) * fy
    out = (f32(2) * out) / f32(255) - f32(1)
    assert out.dtype == f32
    return np.ascontiguousarray(np.moveaxis(out, -1, -3))


def frechet_scipy(mu1, sigma1, mu2, sigma2):
    """The reference's tools/utils.py:65-116 formula, as it runs (scipy's sqrtm of the product, imaginary part dropped)."""
    from scipy import linalg
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    assert np.isfinite(covmean).all()
    if np.iscomplexobj(covmean):
        covmean = covmean.real
    return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean)


def fvd_numpy(acts_1, acts_2, frechet):
    """fvd.py:136-143 with the given Frechet distance."""
    a1, a2 = np.asarray(acts_1, dtype=np.float64), np.asarray(acts_2, dtype=np.float64)
    return frechet(np.mean(a1, axis=0), np.cov(a1, rowvar=False), np.mean(a2, axis=0), np.cov(a2, rowvar=False))


def clips(shape, seed):
    """x uniform in [-1, 1), fp32 [N, T, 3, H, W]."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * 2 - 1

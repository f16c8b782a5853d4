"""Host mirror of the decoder's motion export (ccvs_amd/csrc/flowviz.hip, include/ccvs_hip_flowviz.h), written
from the formulas, in torch on the CPU: `export` (one frame's slot of the motion buffer), `clip_max` (per-clip largest flow magnitude)
and `render` (the two uint8 clips), each in float64 or fp32 (`dtype`), and `edge_sensitive`, the pixels at which an fp32 evaluation
may legitimately land on the other side of a truncation.

The fp32 forms keep the kernels' operation order: every product, sum, quotient and square root is one rounded fp32 operation (torch
tensor ops do not fuse), so everything but `atan2` and `exp` is the kernels' arithmetic bit for bit.
"""
import math

import numpy as np
import torch


def export(fo, k, flow_mult, dtype=torch.float64):
    """fo [B * k, 3, H, W] (flow | occlusion logit) -> [B, 3, H, W]: context 0's flow times flow_mult, and the mask of the blend
    (reference skip_autoencoder.py:255-263): conf_j = 1 - sigmoid(occ_j) + 1e-6, occ = sum occ_j conf_j / sum conf_j (k > 1),
    mask = sigmoid(occ)."""
    f = fo.to(dtype)
    n, _, h, w = f.shape
    b = n // k
    flow = f[0::k, :2] * flow_mult
    occs = f[:, 2].reshape(b, k, h, w)
    if k > 1:
        conf = 1 - torch.sigmoid(occs) + 1e-6
        occ = (occs * conf).sum(dim=1) / conf.sum(dim=1)
    else:
        occ = occs[:, 0]
    return torch.cat([flow, torch.sigmoid(occ).unsqueeze(1)], dim=1)


def _sqrt(x):
    """The correctly rounded square root.  torch's CPU sqrt of an fp32 tensor is not that on every host (one ulp off on an AVX512
    machine, where numpy's of the same bits is right): fp32 goes through float64 and is rounded once more, which for a square root
    gives the correctly rounded fp32 result (53 >= 2 * 24 + 2 bits)."""
    if x.dtype == torch.float32:
        with np.errstate(all="ignore"):
            return torch.from_numpy(np.sqrt(x.contiguous().numpy().astype(np.float64)).astype(np.float32))
    return torch.sqrt(x)


def _div(a, b):
    """The correctly rounded quotient, fp32 through float64 for the same reason (the bound holds for a quotient too)."""
    if a.dtype == torch.float32:
        a, b = torch.broadcast_tensors(a, b)
        with np.errstate(all="ignore"):
            return torch.from_numpy((a.contiguous().numpy().astype(np.float64) / b.contiguous().numpy().astype(np.float64)).astype(np.float32))
    return a / b


def magnitude(motion, dtype=torch.float32):
    fx, fy = motion[:, :, 0].to(dtype), motion[:, :, 1].to(dtype)
    return _sqrt(fx * fx + fy * fy)


def clip_max(motion, dtype=torch.float32):
    """[B, T, 3, H, W] -> [B]: the largest finite sqrt(fx^2 + fy^2) of each clip, 0 where there is none."""
    mag = magnitude(motion, dtype)
    mag = torch.where(torch.isfinite(mag), mag, torch.zeros_like(mag))
    return mag.flatten(1).amax(dim=1)


def _theta(fx, fy):
    return (1 + torch.atan2(fy, fx) / np.pi) / 2


def colours(motion, max_px, lut, dtype=torch.float32):
    """(rgb [B, T, H, W, 3] in [0, 1], idx [B, T, H, W]): r = min(1, |f| / max_px), theta = (1 + atan2(fy, fx) / pi) / 2,
    idx = min(int(theta * 128), 127), rgb = clamp(r * lut[idx], 0, 1); black (and bin 0) where max_px is not > 0 or a component is not
    finite."""
    m = motion.to(dtype)
    fx, fy = m[:, :, 0], m[:, :, 1]
    mp = max_px.to(dtype).view(-1, 1, 1, 1).expand_as(fx)
    ok = (mp > 0) & torch.isfinite(fx) & torch.isfinite(fy)
    one = torch.ones((), dtype=dtype)
    safe = torch.where(ok, mp, one)
    r = torch.where(ok, torch.minimum(_div(magnitude(motion, dtype), safe), one), torch.zeros((), dtype=dtype))
    theta = _theta(torch.where(ok, fx, one), torch.where(ok, fy, one))
    idx = torch.where(ok, (theta * 128).to(torch.int64).clamp(0, 127), torch.zeros((), dtype=torch.int64))
    return (r.unsqueeze(-1) * lut.to(dtype)[idx]).clamp(0, 1), idx


def render(motion, max_px, lut, dtype=torch.float32):
    """(flow_u8, occ_u8, idx): uint8 [B, T, H, W, 3] twice and the colour bin of every pixel.  A byte is (uint8)(v * 255), truncated, of
    `colours`' rgb and of clamp(mask, 0, 1) (0 for a NaN mask)."""
    rgb, idx = colours(motion, max_px, lut, dtype)
    flow_u8 = (rgb * 255).to(torch.uint8)
    mask = torch.nan_to_num(motion[:, :, 2].to(dtype), nan=0.0).clamp(0, 1)
    occ_u8 = (mask * 255).to(torch.uint8).unsqueeze(-1).expand(*mask.shape, 3).contiguous()
    return flow_u8, occ_u8, idx


def edge_sensitive(motion, max_px, lut):
    """bool [B, T, H, W]: pixels where, in float64, theta * 128 is within 1e-3 of an integer, or |f| / max_px within 1e-6 of 1, or a
    byte's value r * lut * 255 / mask * 255 within 1e-3 of an integer -- there an fp32 evaluation with another atan2 or exp may pick
    the neighbouring bin or byte.  A value every precision computes exactly is no edge: a channel whose table entry is 0, the product
    1 * 1 of a saturated radius with a table entry 1, a mask of exactly 0 or 1.  Black pixels (max_px not > 0, a non-finite
    component) have none."""
    m = motion.double()
    fx, fy, mk = m[:, :, 0], m[:, :, 1], m[:, :, 2]
    mp = max_px.double().view(-1, 1, 1, 1).expand_as(fx)
    ok = (mp > 0) & torch.isfinite(fx) & torch.isfinite(fy)
    one = torch.ones((), dtype=torch.float64)
    fx, fy, mp = torch.where(ok, fx, one), torch.where(ok, fy, one), torch.where(ok, mp, one)
    q = torch.sqrt(fx * fx + fy * fy) / mp
    r = q.clamp(max=1.0)
    t128 = _theta(fx, fy) * 128
    near = lambda v: (v - v.round()).abs() < 1e-3
    flag = near(t128) | ((q - 1).abs() < 1e-6)
    l64 = lut.double()[t128.to(torch.int64).clamp(0, 127)]
    exact = (l64 == 0) | ((l64 == 1) & (r.unsqueeze(-1) == 1))
    flag = flag | (near(r.unsqueeze(-1) * l64 * 255) & ~exact).any(dim=-1)
    flag = flag & ok
    mk = torch.nan_to_num(mk, nan=0.0).clamp(0, 1)
    return flag | (near(mk * 255) & (mk != 0) & (mk != 1))


def make_motion(b, t, h, w, seed, lut, max_px, scale=(0.05, 20.0), clean=True):
    """A random motion buffer [B, T, 3, H, W] fp32 -- flow magnitudes log-uniform in `scale` pixels, any direction, masks uniform in
    (0, 1).  clean: none of its pixels is edge-sensitive at `max_px` -- a flagged pixel is drawn again (the mirror alone decides)."""
    g = torch.Generator().manual_seed(seed)

    def draw():
        mag = torch.exp(torch.empty(b, t, h, w).uniform_(math.log(scale[0]), math.log(scale[1]), generator=g))
        ang = torch.empty(b, t, h, w).uniform_(-math.pi, math.pi, generator=g)
        return torch.stack([mag * torch.cos(ang), mag * torch.sin(ang), torch.empty(b, t, h, w).uniform_(0.01, 0.99, generator=g)], dim=2)

    motion = draw()
    if not clean:
        return motion
    mp = torch.full((b,), float(max_px))
    for _ in range(20):
        bad = edge_sensitive(motion, mp, lut)
        if not bad.any():
            return motion
        motion = torch.where(bad.unsqueeze(2), draw(), motion)
    raise AssertionError("make_motion: still edge-sensitive pixels after 20 redraws")

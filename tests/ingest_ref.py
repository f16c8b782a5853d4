"""NumPy restatement of the input stage's arithmetic, for the tests only -- the product does not import it.

Pillow's 8-bit bilinear resampler (`ImagingResample`, Resample.c), per axis `in` -> `out` samples:
    scale = in / out, filterscale = max(scale, 1), support = filterscale, ksize = 2 * ceil(support) + 1
    center = (x + 0.5) * scale, xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), in) - xmin
    w_i = max(0, 1 - |(i + xmin - center + 0.5) / filterscale|) in double, divided by their sum; k_i = int(w_i * 2^22 + 0.5)
    out = clip(((1 << 21) + sum_i k_i p_i) >> 22, 0, 255)
horizontal pass first, rounded to uint8, then the vertical one; a pass whose size does not change is skipped.  The tables are built with
Python floats (doubles) one output sample at a time, the way Resample.c does it -- not the vectorised construction of
`ccvs_amd.ops.resample_tables`, which tests/test_ingest_host.py compares with this one."""
import math

import numpy as np

PRECISION_BITS = 22

# (source (Hs, Ws), crop box (top, left, h, w) or None, output (Ho, Wo)): each the smallest shape that can go wrong in its own way
SHAPES = [
    ((5, 7), None, (3, 2)),            # smallest two-pass case
    ((1, 9), None, (4, 4)),            # one source row
    ((3, 3), None, (64, 64)),          # ~21x upscale, clipped bounds at every edge
    ((37, 53), None, (16, 16)),        # odd row bytes, non-integer downscale
    ((96, 96), None, (128, 128)),      # Drums' real geometry
    ((64, 48), None, (64, 17)),        # horizontal pass only
    ((19, 64), None, (8, 64)),         # vertical pass only
    ((64, 64), None, (64, 64)),        # neither pass
    ((300, 200), None, (64, 42)),      # 4.7x downscale, ksize 11
    ((130, 270), None, (70, 141)),     # several tiles both ways, ragged edges
    ((400, 24), None, (3, 24)),        # one output row's support is 269 source rows
    ((41, 67), (3, 5, 32, 57), (16, 29)),   # odd crop offset; bounds must stop at the box
]


def shape_id(shape):
    (hs, ws), box, (ho, wo) = shape
    return f"{hs}x{ws}" + ("" if box is None else "_box" + "_".join(str(v) for v in box)) + f"_to_{ho}x{wo}"


def source(shape, frames=1):
    """The seeded random uint8 frames [frames, Hs, Ws, 3] of a shape (a smooth image would hide rounding errors).  Frame 0 is the one
    tests/golden/ingest_pil.npz holds Pillow's output for.  RandomState's stream is frozen by NumPy's compatibility policy."""
    (hs, ws), _, (ho, wo) = shape
    rng = np.random.RandomState(1000003 * hs + 1009 * ws + 31 * ho + wo)
    return rng.randint(0, 256, size=(frames, hs, ws, 3)).astype(np.uint8)


def tables(in_size, out_size):
    """(coef int32 [out, ksize], bounds int32 [out, 2]) of one axis: precompute_coeffs + normalize_coeffs_8bpc of Resample.c."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    coef = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)          # int(): truncation towards zero, as the C cast
        xmax = min(int(center + support + 0.5), in_size) - xmin
        ws, ww = [], 0.0
        for x in range(xmax):
            a = abs((x + xmin - center + 0.5) * ss)
            w = 1.0 - a if a < 1.0 else 0.0
            ws.append(w)
            ww += w
        for x in range(xmax):
            w = ws[x] / ww if ww != 0.0 else ws[x]
            coef[xx, x] = int(-0.5 + w * (1 << PRECISION_BITS)) if w < 0 else int(0.5 + w * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return coef, bounds


def resample_axis(img, out_size, axis):
    """One rounded pass along `axis` of a uint8 array."""
    img = np.moveaxis(img, axis, 0)
    coef, bounds = tables(img.shape[0], out_size)
    out = np.empty((out_size,) + img.shape[1:], dtype=np.uint8)
    src = img.astype(np.int64)
    for o in range(out_size):
        lo, n = int(bounds[o, 0]), int(bounds[o, 1])
        k = coef[o, :n].astype(np.int64).reshape((n,) + (1,) * (img.ndim - 1))
        s = (1 << (PRECISION_BITS - 1)) + (k * src[lo:lo + n]).sum(axis=0)
        out[o] = np.clip(s >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize(img, size):
    """`PIL.Image.resize((Wo, Ho), BILINEAR)` of uint8 [..., H, W, 3] (the leading axes are frames)."""
    ho, wo = int(size[0]), int(size[1])
    h, w = img.shape[-3], img.shape[-2]
    if wo != w:
        img = resample_axis(img, wo, img.ndim - 2)
    if ho != h:
        img = resample_axis(img, ho, img.ndim - 3)
    return np.ascontiguousarray(img)


def crop(img, box):
    top, left, h, w = box
    assert 0 <= top and 0 <= left and top + h <= img.shape[-3] and left + w <= img.shape[-2], (box, img.shape)
    return img[..., top:top + h, left:left + w, :]


def stage(img, box, size):
    """One stage of a plan: crop to `box` (None: the whole frame), then resize to `size` (None: the box's size)."""
    if box is not None:
        img = crop(img, box)
    return resize(img, size) if size is not None else np.ascontiguousarray(img)


def run_plan(img, plan):
    for box, size in plan:
        img = stage(img, box, size)
    return img


def normalize(u8, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)):
    """ToTensor + Normalize of uint8 [..., H, W, 3] by torch on the CPU, where the reference's transforms run: fp32 [..., 3, H, W]."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(u8))
    t = t.permute(*range(t.dim() - 3), -1, -3, -2).to(torch.float32).div(255)
    m = torch.tensor(mean, dtype=torch.float32)[:, None, None]
    s = torch.tensor(std, dtype=torch.float32)[:, None, None]
    return (t - m) / s

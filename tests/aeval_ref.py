"""Test-side yardstick of the frame autoencoder's validation figures: float64 restatements of the three reductions behind
`eval_img_to_img_generator` (quantized_video_model.py:460-480, quantize.py:59-68), the bounds the tests hold the GPU to, the input
clip and the readers of tests/golden/tiny_aeval.npz (tests/golden/make_golden_aeval.py).  Never imported by the product."""
import json
import math
import os

import numpy as np
import torch

LINES = ("plain", "norm")          # TINY_ARGV, TINY_ARGV + ["--q_normalize_out"]
PIX_TOL = 1e-3                     # the bar tests/test_e2e_gpu.py holds decoded pixels to
ENC_TOL = 1e-4                     # the bar it holds the encoder's features to
MIN_GAP = 1e-4                     # ten times the 1e-5 the GPU encoder is held to at the codes: no code can flip
BETA = 0.25                        # QVidModel's commitment weight (quantized_video_model.py:143)
CLIP_SEED, CLIP_SCALE = 79, 3.0


def frames(seed=CLIP_SEED, scale=CLIP_SCALE):
    """8 frames [8, 3, 32, 32] built like `_clip()` of tests/test_transformer_loss_gpu.py: flat 8 x 8 patches under a little noise
    (uniform noise is averaged away by the encoder: every position gets one code and every figure is degenerate)."""
    g = torch.Generator().manual_seed(seed)
    level = (torch.rand(2, 4, 3, 4, 4, generator=g) * 2 - 1).repeat_interleave(8, dim=-2).repeat_interleave(8, dim=-1)
    vid = (scale * (0.8 * level + 0.2 * (torch.rand(2, 4, 3, 32, 32, generator=g) * 2 - 1))).clamp(-1, 1)
    return vid.reshape(8, 3, 32, 32)


def l1_mean64(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).mean())


def vq_stats64(z_nchw, idx, codebook, row_scale=None):
    """(mean over every element of (s * E[idx[p]][c] - z[n, c, p])^2, counts [n_e]) in float64; z [N, C, ...], idx in (n, hw) order.
    An index outside [0, n_e) is not counted and makes the mean NaN."""
    z = np.asarray(z_nchw, dtype=np.float64)
    n, c = z.shape[:2]
    z = z.reshape(n, c, -1)
    cb = np.asarray(codebook, dtype=np.float64)
    idx = np.asarray(idx).reshape(-1).astype(np.int64)
    ok = (idx >= 0) & (idx < cb.shape[0])
    counts = np.bincount(idx[ok], minlength=cb.shape[0])
    if not ok.all():
        return float("nan"), counts
    rows = cb[idx]
    if row_scale is not None:
        rows = rows * np.asarray(row_scale, dtype=np.float64)[idx][:, None]
    zq = rows.reshape(n, -1, c).transpose(0, 2, 1)
    return float(((zq - z) ** 2).mean()), counts


def row_scale64(codebook):
    return 1.0 / np.sqrt((np.asarray(codebook, dtype=np.float64) ** 2).sum(axis=1))


def perplexity64(counts, total):
    """quantize.py:67-68 in float64, its `+ 1e-10` included."""
    p = np.asarray(counts, dtype=np.float64) / float(total)
    return float(np.exp(-(p * np.log(p + 1e-10)).sum()))


def top2_gap64(z_nchw, codebook):
    """Smallest difference between the two smallest squared distances to the codebook, over all positions (float64)."""
    z = np.asarray(z_nchw, dtype=np.float64)
    zf = np.moveaxis(z.reshape(z.shape[0], z.shape[1], -1), 1, 2).reshape(-1, z.shape[1])
    cb = np.asarray(codebook, dtype=np.float64)
    d = ((zf[:, None, :] - cb[None, :, :]) ** 2).sum(axis=2)
    d.sort(axis=1)
    return float((d[:, 1] - d[:, 0]).min())


def quant_loss_bound(max_dz, ref_loss, beta=BETA, delta=ENC_TOL):
    """Each element of (z_q - z)^2 moves by at most 2 |z_q - z| delta + delta^2 when z moves by delta, so the mean does; times
    (1 + beta); plus 1e-6 relative for the reference's own fp32 mean."""
    return (1.0 + beta) * (2.0 * max_dz * delta + delta * delta) + 1e-6 * abs(ref_loss)


def perplexity_bound(n_used, perplexity):
    """An fp32 sum of n same-sign terms is off by at most (n - 1) 2^-24 of its value, plus a few ulp from `log`: the entropy H is
    off by (n_used + 4) 2^-24 H, and so is exp(H), relatively."""
    return (n_used + 4) * 2.0 ** -24 * math.log(perplexity) * perplexity


def conditions(gold, line, n_e):
    """The fixture's conditions (make_golden_aeval.py asserts them, the host test re-asserts them on the file)."""
    used = int(np.unique(gold[f"{line}/code"]).size)
    ppl = float(gold[f"{line}/perplexity"])
    assert float(gold[f"{line}/min_gap"]) >= MIN_GAP, (line, float(gold[f"{line}/min_gap"]))
    assert used >= 4 and 2.0 <= ppl <= n_e - 1, (line, used, ppl)
    assert float(gold[f"{line}/l1"]) >= 10 * PIX_TOL, (line, float(gold[f"{line}/l1"]))


def load_gold(golden_dir):
    gold = np.load(os.path.join(golden_dir, "tiny_aeval.npz"))
    return gold, json.loads(str(gold["lines"]))


def weights(golden_dir, gold, line, prefix):
    """The `e` / `q` / `g` state dict of a line: from the fixture where it holds one, from tiny_e2e.npz otherwise."""
    pre = f"{line}/w/{prefix}/"
    own = {k[len(pre):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(pre)}
    if own:
        return own
    e2e = np.load(os.path.join(golden_dir, "tiny_e2e.npz"))
    return {k[len(prefix) + 1:]: torch.from_numpy(e2e[k]) for k in e2e.files if k.startswith(prefix + "/")}

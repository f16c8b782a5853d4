#!/usr/bin/env python3
"""Time `ops.gaussian_blur` (`ccvs_gaussian_blur`) at the deblurring mode's BAIR shape: batch 16 x 16 frames x 3 x 256^2, kernel 13
(sigma 10), against the HBM estimate of 8 bytes per output pixel (GPU box only; run under `rocprofv3 --kernel-trace --stats` for the
kernel's own time)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccvs_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--k", type=int, default=13)
    ap.add_argument("--sigma", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    x = torch.rand(a.batch * a.frames, 3, a.size, a.size, device="cuda") * 2 - 1
    for _ in range(3):
        ops.gaussian_blur(x, a.k, a.sigma)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        ops.gaussian_blur(x, a.k, a.sigma)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.reps
    nbytes = 8.0 * x.numel()
    print(f"gaussian_blur [{a.batch * a.frames}, 3, {a.size}, {a.size}] k={a.k}: {ms:.4f} ms per call (events, incl. launch), "
          f"{nbytes / 1e6:.1f} MB compulsory traffic, {nbytes / ms / 1e9:.2f} TB/s")


if __name__ == "__main__":
    main()

"""Time the STFT decoder's output head (`ops.channel_head`: 1 x 1 convolution to one channel + LeakyReLU + tanh in one pass) against
the same layer sent through `ops.conv2d` with one output channel followed by a separate tanh pass, and against a plain device copy of
the bytes the head must move; and `ops.mse` on the decoded spectrograms.  Shapes: the Drums decoder's last layer (C = 512, 64 x 16)
for 6 frames (2 clips x 3 frames) and for a batch of 8 clips x 45 frames.  Prints one line per shape and a JSON summary."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccvs_amd import ops  # noqa: E402
from to_rgb_bench import timed  # noqa: E402


def main():
    rows = []
    c, h, w = 512, 64, 16
    for n in (6, 360):
        x = torch.randn(n, c, h, w, device="cuda")
        wt = torch.randn(1, c, 1, 1, device="cuda")
        b = torch.randn(1, device="cuda") * 0.1
        scale = c ** -0.5
        packed = ops.pack_conv_weight(wt)
        nbytes = 4 * (x.numel() + n * h * w)
        src = torch.empty(nbytes // 8, device="cuda")
        dst = torch.empty_like(src)
        y = ops.channel_head(x, wt, scale, b, act=True, tanh=True)
        y2 = torch.tanh(ops.conv2d(x, packed, b, 1, 1, act=True))
        diff = float((y - y2).abs().max())
        t_head, t_head_best = timed(lambda: ops.channel_head(x, wt, scale, b, act=True, tanh=True))
        t_conv, _ = timed(lambda: torch.tanh(ops.conv2d(x, packed, b, 1, 1, act=True)))
        t_cp, _ = timed(lambda: dst.copy_(src))
        t_mse, _ = timed(lambda: ops.mse(y, y2))
        row = {"N": n, "C": c, "H": h, "W": w, "MB": nbytes / 1e6, "head_ms": t_head, "head_best_ms": t_head_best,
               "head_TBps": nbytes / t_head / 1e9, "conv_tanh_ms": t_conv, "copy_ms": t_cp, "copy_TBps": nbytes / t_cp / 1e9,
               "mse_ms": t_mse, "mse_MB": 8 * y.numel() / 1e6, "mse_GBps": 8 * y.numel() / t_mse / 1e6, "max_abs_head_vs_conv": diff}
        rows.append(row)
        print(f"N {n:4d} C {c} {h}x{w}  {nbytes / 1e6:8.1f} MB  channel_head {t_head:.4f} ms ({row['head_TBps']:.2f} TB/s)"
              f"  conv2d(1 ch)+tanh {t_conv:.4f} ms  copy {t_cp:.4f} ms ({row['copy_TBps']:.2f} TB/s)"
              f"  mse {row['mse_MB']:.2f} MB {t_mse:.4f} ms ({row['mse_GBps']:.1f} GB/s)  max|head - conv| {diff:.2e}")
    print(json.dumps({"shapes": rows}))


if __name__ == "__main__":
    main()

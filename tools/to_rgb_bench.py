"""Time `ops.to_rgb` (the skip_rgb head's ToRGB) at BAIR's decoder levels, batch 16, against a plain device copy of the same bytes
(what the launch must read and write: x, the skip input, y).  Prints one line per level and a JSON summary."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccvs_amd import ops  # noqa: E402
from ccvs_amd.tools.options import BAIR_ARGV, Options  # noqa: E402


def timed(fn, reps=50, inner=20):
    """ms per call: `inner` back-to-back launches between two events, so that the GPU never waits for the host's launch overhead
    (tens of microseconds through the Python wrapper: more than a coarse level's kernel); median and best of `reps`."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main(n=16):
    q = Options().parse(load_qvid_generator=True, load_transformer=True, argv=list(BAIR_ARGV))["qvid_generator"]
    levels = len(q.necf_mult)
    rows = []
    for i in range(levels):
        c = q.necf * q.necf_mult[-1 - i]
        h = q.max_dim // 2 ** (levels - 1 - i)
        x = torch.randn(n, c, h, h, device="cuda")
        w = torch.randn(3, c, device="cuda")
        b = torch.randn(3, device="cuda")
        skip = torch.randn(n, 3, h // 2, h // 2, device="cuda") if i else None
        nbytes = 4 * (x.numel() + (skip.numel() if skip is not None else 0) + n * 3 * h * h)
        src = torch.empty(nbytes // 8, device="cuda")
        dst = torch.empty_like(src)
        t_rgb, t_rgb_best = timed(lambda: ops.to_rgb(x, w, b, b, skip=skip))
        t_cp, _ = timed(lambda: dst.copy_(src))     # reads and writes nbytes / 2 each: nbytes of traffic
        row = {"level": i, "C": c, "H": h, "MB": nbytes / 1e6, "to_rgb_ms": t_rgb, "to_rgb_best_ms": t_rgb_best, "copy_ms": t_cp,
               "to_rgb_TBps": nbytes / t_rgb / 1e9, "copy_TBps": nbytes / t_cp / 1e9, "of_copy": t_cp / t_rgb}
        rows.append(row)
        print(f"level {i}: C {c:4d} {h:3d}^2  {nbytes / 1e6:8.1f} MB  to_rgb {t_rgb:.4f} ms ({row['to_rgb_TBps']:.2f} TB/s)"
              f"  copy {t_cp:.4f} ms ({row['copy_TBps']:.2f} TB/s)  ratio {row['of_copy']:.2f}")
    print(json.dumps({"batch": n, "levels": rows}))


if __name__ == "__main__":
    main()

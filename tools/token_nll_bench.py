"""Time the transformer loss's kernels (`ops.token_nll` + `ops.mean_f32`: per-token NLL over the teacher-forced logits, then the mean)
against a device-to-device copy of the same logits bytes (the roofline the project prices HBM-bound kernels against) and against
`torch.nn.functional.cross_entropy` on the same GPU tensor (what the parent commit's user had to call).  Shapes: BAIR, 16 clips x 1023
positions of 1024 logits (67 MB: it fits the chip's 256 MB last-level cache, so its rates are not HBM rates), and Kinetics, 20480 rows of
16384 logits (1.34 GB).  Prints one line per shape and a JSON summary; `python tools/token_nll_bench.py > profiles/token_nll.txt`."""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccvs_amd import ops  # noqa: E402
from to_rgb_bench import timed  # noqa: E402


def main():
    rows = []
    for name, m, v in (("bair", 16 * 1023, 1024), ("kinetics", 20480, 16384)):
        g = torch.Generator(device="cuda").manual_seed(m)
        logits = torch.randn(m, v, device="cuda", generator=g) * 3
        target = torch.randint(0, v, (m,), device="cuda", generator=g)
        dst = torch.empty_like(logits)
        nbytes = 4 * m * v                                   # the logits, read once; targets and results are 12 B per row
        ours = ops.mean_f32(ops.token_nll(logits, target))
        aten = F.cross_entropy(logits, target)
        want = F.cross_entropy(logits.double(), target)
        t_nll, t_nll_best = timed(lambda: ops.token_nll(logits, target))
        t_both, _ = timed(lambda: ops.mean_f32(ops.token_nll(logits, target)))
        t_cp, _ = timed(lambda: dst.copy_(logits))
        t_aten, _ = timed(lambda: F.cross_entropy(logits, target))
        row = {"shape": name, "rows": m, "V": v, "MB": nbytes / 1e6, "token_nll_ms": t_nll, "token_nll_best_ms": t_nll_best,
               "token_nll_TBps": nbytes / t_nll / 1e9, "nll_plus_mean_ms": t_both, "copy_ms": t_cp, "copy_read_TBps": nbytes / t_cp / 1e9,
               "aten_cross_entropy_ms": t_aten, "ours_over_copy": t_both / t_cp, "aten_over_ours": t_aten / t_both,
               "err_ours_vs_f64": abs(ours.item() - want.item()), "err_aten_vs_f64": abs(aten.item() - want.item())}
        rows.append(row)
        print(f"{name:9s} {m} x {v}  {nbytes / 1e6:8.1f} MB  token_nll {t_nll:.4f} ms ({row['token_nll_TBps']:.2f} TB/s read)  + mean {t_both:.4f} ms"
              f"  copy {t_cp:.4f} ms ({row['copy_read_TBps']:.2f} TB/s read, as much written)  aten cross_entropy {t_aten:.4f} ms"
              f"  ours / copy {row['ours_over_copy']:.2f}  aten / ours {row['aten_over_ours']:.2f}"
              f"  |ours - f64| {row['err_ours_vs_f64']:.1e}  |aten - f64| {row['err_aten_vs_f64']:.1e}")
        del logits, dst
        torch.cuda.empty_cache()
    print(json.dumps({"shapes": rows}))


if __name__ == "__main__":
    main()

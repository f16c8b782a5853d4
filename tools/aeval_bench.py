"""Time the three reductions behind the frame autoencoder's validation figures (`ops.l1_mean`, `ops.vq_stats`, `ops.code_perplexity`) at
the BAIR shapes, each with the bytes it moves, against a device-to-device copy of the same bytes (the roofline the project prices
HBM-bound kernels against) and against the aten expression the parent commit's user had to write.  l1_mean: 256 frames of 3 x 256^2
(two arrays of 201 MB, read once); vq_stats: N = 256, C = 512, HW = 64, n_e = 1024 (z 33.5 MB read once, the 2 MB codebook gathered
from L2, 131 KB of indices: it fits the chip's 256 MB last-level cache, so its rate is not an HBM rate).  Prints one line per kernel and
a JSON summary; `python tools/aeval_bench.py > profiles/aeval.txt`."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccvs_amd import ops  # noqa: E402
from to_rgb_bench import timed  # noqa: E402


def main():
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = []
    # ---- l1_mean
    a = torch.rand(256, 3, 256, 256, device="cuda", generator=g) * 2 - 1
    b = torch.rand(256, 3, 256, 256, device="cuda", generator=g) * 2 - 1
    nbytes = 2 * 4 * a.numel()
    want = (a.double() - b.double()).abs().mean().item()
    ours = ops.l1_mean(a, b).item()
    t, best = timed(lambda: ops.l1_mean(a, b))
    t_cp, _ = timed(lambda: b.copy_(a))                      # reads half the bytes, writes as many
    a2 = a.clone()
    t_aten, _ = timed(lambda: torch.mean(torch.abs(a2 - b)))
    rows.append({"kernel": "l1_mean", "elements": a.numel(), "MB": nbytes / 1e6, "ms": t, "best_ms": best, "TBps": nbytes / t / 1e9,
                 "copy_same_bytes_ms": t_cp, "aten_ms": t_aten, "rel_err_vs_f64": abs(ours - want) / want})
    print(f"l1_mean   {a.numel()} elements  {nbytes / 1e6:7.1f} MB read  {t:.4f} ms ({nbytes / t / 1e9:.2f} TB/s)  copy of {nbytes / 2e6:.1f} MB "
          f"{t_cp:.4f} ms ({nbytes / t_cp / 1e9:.2f} TB/s read + written)  aten mean(abs(a - b)) {t_aten:.4f} ms  rel err vs f64 "
          f"{abs(ours - want) / want:.1e}")
    del a, b, a2
    torch.cuda.empty_cache()
    # ---- vq_stats + code_perplexity
    n, c, hw, n_e = 256, 512, 64, 1024
    z = torch.randn(n, c, 8, 8, device="cuda", generator=g)
    cb = torch.randn(n_e, c, device="cuda", generator=g)
    idx = torch.randint(0, n_e, (n * hw,), device="cuda", generator=g)
    nbytes = 4 * z.numel() + 4 * cb.numel() + 8 * idx.numel() + 4 * n_e
    rowsq = cb[idx].view(n, hw, c).transpose(1, 2).reshape(z.shape)
    want = ((rowsq.double() - z.double()) ** 2).mean().item()
    m, counts = ops.vq_stats(z, idx, cb)
    assert torch.equal(counts.long(), torch.bincount(idx, minlength=n_e))
    t, best = timed(lambda: ops.vq_stats(z, idx, cb))
    dst = torch.empty_like(z)
    t_cp, _ = timed(lambda: dst.copy_(z))
    t_aten, _ = timed(lambda: torch.mean((cb[idx].view(n, hw, c).transpose(1, 2).reshape(z.shape) - z) ** 2))
    rows.append({"kernel": "vq_stats", "N": n, "C": c, "HW": hw, "n_e": n_e, "MB": nbytes / 1e6, "ms": t, "best_ms": best,
                 "TBps": nbytes / t / 1e9, "copy_of_z_ms": t_cp, "aten_ms": t_aten, "rel_err_vs_f64": abs(m.item() - want) / want})
    print(f"vq_stats  N {n} C {c} HW {hw} n_e {n_e}  {nbytes / 1e6:7.1f} MB  {t:.4f} ms ({nbytes / t / 1e9:.2f} TB/s; memset, kernel and "
          f"final sum)  copy of z {t_cp:.4f} ms  aten gather + mse {t_aten:.4f} ms  rel err vs f64 {abs(m.item() - want) / want:.1e}")
    for n_e2 in (1024, 16384):
        cnt = torch.randint(0, 40, (n_e2,), device="cuda", generator=g).int()
        total = int(cnt.sum().item())
        t, best = timed(lambda: ops.code_perplexity(cnt, total))
        rows.append({"kernel": "code_perplexity", "n_e": n_e2, "bytes": 4 * n_e2, "ms": t, "best_ms": best})
        print(f"code_perplexity  n_e {n_e2}  {4 * n_e2} B  {t:.4f} ms")
    print(json.dumps({"kernels": rows}))


if __name__ == "__main__":
    main()

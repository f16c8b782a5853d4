"""Worker of tests/test_gemm_forms_gpu.py::test_gemm_sequence_fallback_row_blocked_vs_float64: whole-sequence GEMMs (plain, residual,
LayerNorm-folded + GELU) under whatever CCVS_GEMM_SEQ_DENSE the parent set (the library reads the switch once per process); inputs,
packed LayerNorm operands and results to the .npz named on the command line."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccvs_amd import ops  # noqa: E402

g = torch.Generator().manual_seed(23)
out = {}
for m, n, k in ((300, 130, 48), (1000, 1024, 1040)):   # ragged M / N with an odd stage count; 8 row tiles with an odd deep K
    s = f"{m}_{n}_{k}"
    x = torch.randn(m, k, generator=g) * 0.7 + 0.3
    w = torch.randn(n, k, generator=g) * (1 / k ** 0.5)
    b = torch.randn(n, generator=g)
    res = torch.randn(m, n, generator=g)
    gamma, beta = 1 + 0.3 * torch.randn(k, generator=g), 0.2 * torch.randn(k, generator=g)
    packed = ops.pack_ln_linear(w, b, gamma, beta)
    xc, wc, bc, rc, pk = x.cuda(), w.cuda(), b.cuda(), res.cuda(), [t.cuda() for t in packed]
    out[f"plain_{s}"] = ops.gemm_nt(xc, wc, bc, ops.EPI_NONE | ops.GEMM_SEQ)
    out[f"resout_{s}"] = ops.gemm_nt(xc, wc, bc, ops.EPI_RESIDUAL | ops.GEMM_SEQ, residual=rc)
    out[f"ln_{s}"] = ops.gemm_ln(xc, *pk, epilogue=ops.EPI_GELU | ops.GEMM_SEQ)
    for name, t in (("x", x), ("w", w), ("b", b), ("res", res), ("wg", packed[0]), ("bb", packed[1]), ("s", packed[2])):
        out[f"{name}_{s}"] = t
torch.cuda.synchronize()
np.savez(sys.argv[1], **{k: v.detach().cpu().numpy() for k, v in out.items()})

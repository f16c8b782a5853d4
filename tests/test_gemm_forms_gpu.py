"""-m gpu: the whole-sequence GEMM (`gemm_seq_kernel`, gpt.hip: prefill, teacher-forced forward, re-prefill of a slid window) at
the op level, against float64 torch on the CPU: every epilogue, the folded LayerNorm, the QKV scatter into the caches, at shapes
chosen for the kernel's own branches -- the XCD-swizzled tile order (row tiles % 8 == 0), an odd number of 16-deep K stages (the
`break` out of the two-stage loop), ragged M and N (clamped DMA rows / columns, masked epilogue), a strided x (ldx > K) and
strided out / residual (ldy > N) -- and the row-blocked form it falls back to under CCVS_GEMM_SEQ_DENSE=0.

Tolerance.  The kernel is fp32 on v_mfma_f32_32x32x2_f32: exact products, one fp32 accumulator chain of K / 2 steps per output.
Its rounding error is at most gamma_{K/2} * A with A = |x| @ |w|^T (+ |bias| + |residual|), the sum of the magnitudes of what is
added (Higham, Accuracy and Stability of Numerical Algorithms, 3.1); for these zero-mean operands the partial sums grow like
sqrt(k) and the errors behave as a random walk, so the observed error is ~1e-7 * A.  The check is |got - want| <= 1e-5 * A per
element: two orders of magnitude of headroom, while a wrong tile, a stale or doubled K stage or a clamped row leaking into the
output is an O(1) fraction of A.  The LayerNorm fold (y = rstd (x @ wg^T - mean s) + bb) is bounded the same way with
A = rstd (|x| @ |wg|^T + |mean| |s|) + |bb|."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REL = 1e-5


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ccvs_amd import ops as _ops
    return _ops


def check(got, want, scale, what):
    """|got - want| <= REL * scale elementwise (want, scale: float64 on the CPU)."""
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), what
    ratio = ((got - want).abs() / scale).max().item()
    assert ratio <= REL, f"{what}: max |err| / A = {ratio:.3e} > {REL:.0e}"


def operands(g, m, n, k, x_slice=False, shift=False):
    """x [m,k] fp32 on the GPU (a column slice of a wider tensor when x_slice: ldx = k + 32, base 16 floats in; rows of mean ~0.3
    when shift), w [n,k], bias, res."""
    if x_slice:
        wide = torch.randn(m, k + 32, generator=g)
        if shift:
            wide = wide * 0.7 + 0.3
        x_cpu = wide[:, 16:16 + k]
        x = wide.cuda()[:, 16:16 + k]
        assert x.stride(0) == k + 32
    else:
        x_cpu = torch.randn(m, k, generator=g)
        if shift:
            x_cpu = x_cpu * 0.7 + 0.3
        x = x_cpu.cuda()
    w = torch.randn(n, k, generator=g) * (1 / k ** 0.5)
    b = torch.randn(n, generator=g)
    res = torch.randn(m, n, generator=g)
    return x_cpu, x, w, b, res


def out_view(m, n, sliced):
    """The output (or residual) buffer: dense, or columns [8, 8 + n) of a NaN-filled [m, n + 24] tensor (ldy > N)."""
    if not sliced:
        return None, None
    big = torch.full((m, n + 24), float("nan"), device="cuda")
    return big, big[:, 8:8 + n]


def untouched(big, n):
    """Columns outside [8, 8 + n) of an out_view buffer are still NaN: the masked epilogue wrote nothing past N."""
    if big is not None:
        rest = torch.cat([big[:, :8], big[:, 8 + n:]], dim=1)
        assert torch.isnan(rest).all(), "the GEMM wrote outside its output columns"


# (M, N, K, x a column slice, out / residual column slices)
#   M: 129 (one row past a tile), 300 (ragged third tile), 1000 (8 row tiles: swizzled order, ragged last tile), 1024 (8 full
#      tiles, swizzled), 2048 (16 tiles: two rounds of the swizzled order), 2049 (17 tiles, plain order, 1 row in the last);  N: 96 (< one tile), 130 (2 columns in the second
#      tile), 1024, 3072;  K: 16 (one stage), 48 (3: odd), 1024, 1040 (65: odd), 4096
NT_SHAPES = [(129, 96, 16, False, False), (300, 130, 48, True, False), (1000, 1024, 1040, False, True),
             (1024, 3072, 1024, False, False), (2049, 130, 4096, True, True), (1000, 96, 48, True, True),
             (2048, 130, 48, False, False)]


@pytest.mark.parametrize("m,n,k,xs,ys", NT_SHAPES)
def test_gemm_nt_sequence_form_vs_float64(ops, m, n, k, xs, ys):
    """ops.gemm_nt(..., E | GEMM_SEQ) for E in {none, GELU (erf form: F.gelu), residual} against x @ w^T + b in float64."""
    g = torch.Generator().manual_seed(m * 7 + n * 3 + k)
    x_cpu, x, w, b, res = operands(g, m, n, k, xs)
    x64, w64 = x_cpu.double(), w.double()
    z = x64 @ w64.t() + b.double()
    a = x64.abs() @ w64.abs().t() + b.double().abs()
    wc, bc = w.cuda(), b.cuda()
    SEQ = ops.GEMM_SEQ

    big, out = out_view(m, n, ys)
    got = ops.gemm_nt(x, wc, bc, ops.EPI_NONE | SEQ, out=out)
    check(got, z, a, f"none {m}x{n}x{k}")
    untouched(big, n)

    big, out = out_view(m, n, ys)
    got = ops.gemm_nt(x, wc, bc, ops.EPI_GELU | SEQ, out=out)
    check(got, F.gelu(z), 1.2 * a + 1e-3, f"gelu {m}x{n}x{k}")   # |gelu'| <= 1.13; + the erf's own rounding
    untouched(big, n)

    big, out = out_view(m, n, ys)
    if ys:   # residual with the same row stride as the output (ops.gemm_nt's contract), in a buffer of its own
        rbig = torch.full((m, n + 24), float("nan"), device="cuda")
        rbig[:, 8:8 + n] = res.cuda()
        r = rbig[:, 8:8 + n]
    else:
        r = res.cuda()
    got = ops.gemm_nt(x, wc, None, ops.EPI_RESIDUAL | SEQ, residual=r, out=out)
    check(got, x64 @ w64.t() + res.double(), x64.abs() @ w64.abs().t() + res.double().abs(), f"residual {m}x{n}x{k}")
    untouched(big, n)


def ln_reference(x_cpu, packed, eps=1e-5):
    """The folded LayerNorm + Linear in float64 from the packed operands themselves: (want, A)."""
    wg, bb, s = (t.double().cpu() for t in packed)
    x64 = x_cpu.double()
    mean = x64.mean(dim=1, keepdim=True)
    rstd = 1 / torch.sqrt(x64.var(dim=1, unbiased=False, keepdim=True) + eps)
    want = rstd * (x64 @ wg.t() - mean * s) + bb
    a = rstd * (x64.abs() @ wg.abs().t() + mean.abs() * s.abs()) + bb.abs()
    return want, a


LN_SHAPES = [(129, 96, 16, False), (300, 130, 48, True), (1000, 1024, 1040, False), (1024, 130, 4096, True), (2049, 1024, 1024, False)]


@pytest.mark.parametrize("m,n,k,xs", LN_SHAPES)
def test_gemm_ln_sequence_form_vs_float64(ops, m, n, k, xs):
    """ops.gemm_ln(..., E | GEMM_SEQ): the row statistics come from the x stages in LDS (`ln_accum` on the staged quads), not
    from the x rows -- checked on non-zero-mean rows, an odd stage count and a strided x, against LayerNorm in float64."""
    g = torch.Generator().manual_seed(m + 11 * n + k)
    x_cpu, x, w, b, _ = operands(g, m, n, k, xs, shift=True)
    gamma, beta = 1 + 0.3 * torch.randn(k, generator=g), 0.2 * torch.randn(k, generator=g)
    packed = ops.pack_ln_linear(w, b, gamma, beta)
    # the fold is LayerNorm + Linear: the float64 fold agrees with the float64 composition (up to the packed fp32 operands)
    want, a = ln_reference(x_cpu, packed)
    direct = F.layer_norm(x_cpu.double(), (k,), gamma.double(), beta.double()) @ w.double().t() + b.double()
    assert ((want - direct).abs() / a).max().item() < 1e-6
    pk = [t.cuda() for t in packed]
    got = ops.gemm_ln(x, *pk, epilogue=ops.EPI_NONE | ops.GEMM_SEQ)
    check(got, want, a, f"ln {m}x{n}x{k}")
    out = torch.full((m, n + 24), float("nan"), device="cuda")
    got = ops.gemm_ln(x, *pk, epilogue=ops.EPI_GELU | ops.GEMM_SEQ, out=out[:, 8:8 + n])
    check(got, F.gelu(want), 1.2 * a + 1e-3, f"ln gelu {m}x{n}x{k}")
    untouched(out, n)


@pytest.mark.parametrize("pos0,pos_dev,tmax", [(0, None, 100), (5, 7, 128), (28, None, 128)])
def test_gemm_ln_qkv_multi_tile(ops, pos0, pos_dev, tmax):
    """ops.gemm_ln_qkv with B * Tq = 300 rows (3 row tiles, batch rows straddling them) and N = 3C = 768 (6 column tiles: q, K
    and V each over two): q, the K / V cache slots [pos, pos + Tq) with pos = pos0 (+ *pos_dev), and every other slot still its
    NaN sentinel.  Cases: pos 0 with Tmax == Tq, a device-resident offset, and pos0 + Tq == Tmax (the last slot written)."""
    B, Tq, C, H = 3, 100, 256, 4
    D = C // H
    g = torch.Generator().manual_seed(pos0 + tmax)
    x = torch.randn(B * Tq, C, generator=g) * 0.7 + 0.3
    w, b = torch.randn(3 * C, C, generator=g) / C ** 0.5, torch.randn(3 * C, generator=g)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    packed = ops.pack_ln_linear(w, b, gamma, beta)
    want, a = ln_reference(x, packed)
    kc = torch.full((B, H, tmax, D), float("nan"), device="cuda")
    vc = torch.full((B, H, tmax, D), float("nan"), device="cuda")
    pd = torch.tensor([pos_dev], dtype=torch.int32, device="cuda") if pos_dev is not None else None
    q = ops.gemm_ln_qkv(x.cuda(), *[t.cuda() for t in packed], kc, vc, B, Tq, pos0, pd)
    pos = pos0 + (pos_dev or 0)
    assert pos + Tq <= tmax
    check(q, want[:, :C], a[:, :C], "q")
    heads = lambda t: t.view(B, Tq, H, D).transpose(1, 2)   # [B*Tq, C] -> [B, H, Tq, D]
    check(kc[:, :, pos:pos + Tq], heads(want[:, C:2 * C]), heads(a[:, C:2 * C]), "k cache")
    check(vc[:, :, pos:pos + Tq], heads(want[:, 2 * C:]), heads(a[:, 2 * C:]), "v cache")
    for cache in (kc, vc):
        assert torch.isnan(cache[:, :, :pos]).all() and torch.isnan(cache[:, :, pos + Tq:]).all(), "a slot outside [pos, pos + Tq) was written"


def test_gemm_sequence_fallback_row_blocked_vs_float64(tmp_path):
    """CCVS_GEMM_SEQ_DENSE=0: whole-sequence calls take `gemm16_rb_kernel<4>` instead.  The library reads the switch once per process,
    so tests/gemm_seq_worker.py runs the calls in a child process with the switch off (inputs and outputs to an .npz); the
    results are checked here against float64 with the bound of the module docstring."""
    path = str(tmp_path / "seq_rb.npz")
    env = dict(os.environ, CCVS_GEMM_SEQ_DENSE="0")
    subprocess.run([sys.executable, os.path.join(HERE, "gemm_seq_worker.py"), path], env=env, check=True, timeout=600)
    d = np.load(path)
    shapes = sorted({key.split("_", 1)[1] for key in d.files if key.startswith("x_")})
    assert len(shapes) == 2
    for s in shapes:
        x, w, b, res = (torch.from_numpy(d[f"{t}_{s}"]).double() for t in ("x", "w", "b", "res"))
        a = x.abs() @ w.abs().t()
        check(torch.from_numpy(d[f"plain_{s}"]), x @ w.t() + b, a + b.abs(), f"rb plain {s}")
        check(torch.from_numpy(d[f"resout_{s}"]), x @ w.t() + b + res, a + b.abs() + res.abs(), f"rb residual {s}")
        packed = [torch.from_numpy(d[f"{t}_{s}"]) for t in ("wg", "bb", "s")]
        want, aln = ln_reference(x, packed)
        check(torch.from_numpy(d[f"ln_{s}"]), F.gelu(want), 1.2 * aln + 1e-3, f"rb ln gelu {s}")

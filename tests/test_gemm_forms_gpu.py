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
A = rstd (|x| @ |wg|^T + |mean| |s|) + |bb|.  That A is the size of the fold's own intermediates on the raw activations: it
grows with |mean| / std exactly as such a fold loses accuracy, so it says nothing about rows of large mean (and these suites draw
mean 0.3, std 0.7).  The bound that does not depend on a row's mean, and the rows that need it, are in tests/ln_fold_ref.py and
tests/test_ln_fold_gpu.py.

The decode forms (single-position calls, no GEMM_SEQ: `gemm16_kernel<1,1,4>` up to 32 rows or under 32 columns, `gemm16_kernel<2,2,1>`
up to 256 rows, `gemm16_rb_kernel<4>` beyond) get the same treatment below: `plan` transcribes the library's K partition (`gemm_kz`,
`gemm16_plan`) so that every shape of DECODE_NT / DECODE_LN / DECODE_QKV states the branch it is there for -- form, K slices per
workgroup (ks) and across workgroups (kz), unrolled K batches and remainder steps per slice -- and a shape that stops reaching it
fails when this module is imported, GPU or not.  Every output buffer starts as NaN, views have their margins checked, the split-K
shapes run twice interleaved on one stream (the workspace's counters and slabs between launches of different shapes), the Tq = 1
QKV scatter is checked slot by slot, and rows 0..15 of a split-K GEMM must not depend on how many rows share the launch.
The decode forms run fp32 chains of K / 4 steps or fewer (v_mfma_f32_16x16x4_f32) and add at most 4 x 4 slice sums (8 in the
row-blocked form) on top, fewer roundings per output than the whole-sequence form's: the same 1e-5 * A holds.  The reference alone,
a plain fp32 torch product of each DECODE_NT / DECODE_LN shape on the CPU, stays far below it against float64 (largest |err| / A over all shapes and epilogues: 2.3e-7)."""
import functools
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


# ---------------------------------------------------------------------------------------------------------------------------
# Decode forms: single-position calls (no GEMM_SEQ)
# ---------------------------------------------------------------------------------------------------------------------------
def plan(M, N, K, ln, seq=False):
    """A transcription of gpt.hip's `gemm_kz` + `gemm16_plan` for a call with a workspace (ops.gemm_nt always passes one; the
    LayerNorm forms never do, which is the `not ln`): (form, ks, kz, full_batches, remainder_steps) -- the kernel form, the K
    slices over a workgroup's waves and over workgroups, and what one slice of K / (ks kz) elements runs: unrolled batches of
    16 U and 16-deep remainder steps, U = 4 for the one-block form, 1 for the 2 x 2 tile, 8 for the row-blocked form.  It reads
    nothing from the library: if the plan changes, this is the test to update."""
    cdiv = lambda a, b: -(-a // b)
    WAVES, KZ_MAX, KZ_MIN_K, DECODE_MAX_M, WS_TILES = 4, 4, 2048, 256, 1024
    decode = not seq and M <= DECODE_MAX_M
    tiles = cdiv(N, 16)
    kz = 1
    if decode and not ln and tiles * cdiv(DECODE_MAX_M, 16) <= WS_TILES:   # every 16 x 16 block of any decode launch owns a slab and a counter
        while K >= KZ_MIN_K and kz < KZ_MAX and tiles * kz * 2 <= 256 and K % (16 * WAVES * kz * 2) == 0:
            kz *= 2
    ks = WAVES if decode else 8
    while ks > 1 and K % (16 * ks * kz) != 0:
        ks >>= 1
    if seq:
        return "seq", ks, kz, None, None   # the dense kernel has K stages, no batches (and no ks: CCVS_GEMM_SEQ_DENSE=0 gives "rb")
    form = ("tile2" if M > 32 and N >= 32 else "tile1") if decode else "rb"
    step = 16 * {"tile1": 4, "tile2": 1, "rb": 8}[form]
    kper = K // (ks * kz)
    return form, ks, kz, kper // step, (kper % step) // 16


# (M, N, K, x a column slice, out / residual column slices, the plan the shape is there for)
DECODE_NT = [
    (5, 50, 16, True, True, ("tile1", 1, 1, 0, 1)),           # one remainder step, no full batch; ragged M and N
    (16, 16, 48, False, False, ("tile1", 1, 1, 0, 3)),        # three remainder steps
    (23, 40, 96, True, True, ("tile1", 2, 1, 0, 3)),          # ks 2 (waves 2, 3 idle); two row blocks, the second ragged
    (32, 130, 1040, True, False, ("tile1", 1, 1, 16, 1)),     # 16 full batches + 1 remainder step; M = 32 stays on the one-block form
    (33, 16, 64, False, True, ("tile1", 4, 1, 0, 1)),         # M > 32 but N < 32: one-block form, three row blocks
    (33, 32, 64, True, True, ("tile2", 4, 1, 1, 0)),          # smallest 2 x 2 tile; the second tile row holds one row, its second row block is skipped
    (48, 1024, 2048, False, True, ("tile2", 4, 4, 8, 0)),     # 64 column tiles: kz 4 under the 2 x 2 tile
    (16, 1040, 2304, True, False, ("tile1", 4, 1, 9, 0)),     # 65 column tiles: one past what the workspace covers at 256 rows, kz 1
    (16, 1024, 2304, True, True, ("tile1", 4, 4, 2, 1)),      # 64 column tiles: kz 4, slices of 144 = 2 full batches + 1 remainder step
    (16, 528, 2176, False, False, ("tile1", 4, 2, 4, 1)),     # K % 256 != 0: kz 2 and not 4, slices of 272 = 4 full batches + 1 remainder step
    (16, 2064, 2048, False, True, ("tile1", 4, 1, 8, 0)),     # 129 column tiles, kz 1
    (40, 200, 2176, True, True, ("tile2", 4, 2, 17, 0)),      # kz 2, ragged N under the 2 x 2 tile with split-K
    (23, 520, 4096, True, False, ("tile1", 4, 4, 4, 0)),      # kz 4 with ragged M and N on the one-block form
    (128, 2048, 2048, False, False, ("tile2", 4, 1, 32, 0)),  # 128 column tiles x 8 row blocks = 1024 blocks: kz 1 (kz 2 while kz depended on M)
    (256, 1024, 2048, True, True, ("tile2", 4, 4, 8, 0)),     # all 1024 workspace tiles x 4 slabs, the last counter; M at GEMM_DECODE_MAX_M
    (257, 130, 48, True, True, ("rb", 1, 1, 0, 3)),           # row-blocked form, remainder only, one row in the last 64-row group
    (260, 40, 1152, False, True, ("rb", 8, 1, 1, 1)),         # row-blocked form, ks 8, one full batch + one remainder step
]
# (M, N, K, plan): x always strided, rows of non-zero mean; the LayerNorm form never splits K across workgroups
DECODE_LN = [
    (5, 50, 16, ("tile1", 1, 1, 0, 1)), (16, 16, 48, ("tile1", 1, 1, 0, 3)), (23, 40, 96, ("tile1", 2, 1, 0, 3)),
    (32, 130, 1040, ("tile1", 1, 1, 16, 1)), (33, 16, 64, ("tile1", 4, 1, 0, 1)), (33, 32, 64, ("tile2", 4, 1, 1, 0)),
    (48, 96, 1024, ("tile2", 4, 1, 16, 0)), (257, 130, 48, ("rb", 1, 1, 0, 3)), (260, 40, 1152, ("rb", 8, 1, 1, 1)),
]
# (B, C, H, Tmax, pos0, pos_dev, plan of the [B, 3C, C] LayerNorm GEMM)
DECODE_QKV = [
    (16, 64, 4, 9, 5, 3, ("tile1", 4, 1, 0, 1)),      # last slot of the cache, device-resident offset
    (40, 48, 3, 8, 0, None, ("tile2", 1, 1, 3, 0)),   # 2 x 2 tile whose 32 columns straddle the q / K boundary at column 48
    (23, 80, 2, 8, 2, 1, ("tile1", 1, 1, 1, 1)),      # D = 40: a 16-column block straddles two heads
    (260, 64, 4, 8, 1, 2, ("rb", 4, 1, 0, 1)),        # the row-blocked form's scatter; B > 256
]
# rows 0..15 of an M = 16 launch against the same rows of these M: the row blocks of the workspace up to its last, both tiles
INVARIANT_NK = [(2048, 2048), (1040, 2304), (1024, 2304), (1024, 2048)]
INVARIANT_M = [128, 144, 256]


def _check_tables():
    """Every shape reaches the plan it states: run on import, so it holds without a GPU."""
    for m, n, k, _, _, want in DECODE_NT:
        assert plan(m, n, k, False) == want, ("gemm_nt", m, n, k, plan(m, n, k, False), want)
    for m, n, k, want in DECODE_LN:
        assert plan(m, n, k, True) == want and want[2] == 1, ("gemm_ln", m, n, k, plan(m, n, k, True), want)
    for b, c, _, _, _, _, want in DECODE_QKV:
        assert plan(b, 3 * c, c, True) == want and want[2] == 1, ("gemm_ln_qkv", b, c, plan(b, 3 * c, c, True), want)
    assert plan(16, 1024, 4096, True)[2] == 1 and plan(16, 1024, 4096, False)[2] == 4   # deep K: only the plain form splits
    assert sum(xs for _, _, _, xs, _, _ in DECODE_NT) * 2 >= len(DECODE_NT) and sum(ys for _, _, _, _, ys, _ in DECODE_NT) * 2 >= len(DECODE_NT)
    # the N boundaries of kz: 64 | 65 column tiles (the workspace), 128 | 129 (what `tiles * kz * 2 <= 256` alone would grant)
    assert [plan(16, 16 * t, 2048, False)[2] for t in (64, 65, 128, 129)] == [4, 1, 1, 1]
    for n, k in INVARIANT_NK:   # a row's K partition is a function of N and K alone
        assert len({plan(m, n, k, False)[1:3] for m in [1, 16] + INVARIANT_M}) == 1, (n, k)
    assert len(SPLIT_K) == 6 and len({(m, n) for m, n, _, _ in SPLIT_K}) == 6


SPLIT_K = [(m, n, k, xs) for m, n, k, xs, _, want in DECODE_NT if want[2] > 1]
_check_tables()


def nan_out(m, n, sliced):
    """out_view, with the dense output NaN-filled too: an element the kernel never writes cannot pass on pool memory."""
    big, out = out_view(m, n, sliced)
    return big, out if sliced else torch.full((m, n), float("nan"), device="cuda")


@functools.lru_cache(maxsize=None)
def nt_case(m, n, k, xs):
    """Operands of a DECODE_NT shape on the GPU and its float64 references on the CPU, built once and shared (read-only)."""
    g = torch.Generator().manual_seed(m * 7 + n * 3 + k)
    x_cpu, x, w, b, res = operands(g, m, n, k, xs)
    x64, w64 = x_cpu.double(), w.double()
    return dict(x=x, w=w.cuda(), b=b.cuda(), res=res, xw=x64 @ w64.t(), axw=x64.abs() @ w64.abs().t(), b64=b.double(), res64=res.double())


@pytest.mark.parametrize("m,n,k,xs,ys,want", DECODE_NT)
def test_gemm_nt_decode_forms_vs_float64(ops, m, n, k, xs, ys, want):
    """ops.gemm_nt(..., E) for E in {none, GELU, residual} on the decode forms against float64, into NaN-filled buffers."""
    assert plan(m, n, k, False) == want
    c = nt_case(m, n, k, xs)
    z, a = c["xw"] + c["b64"], c["axw"] + c["b64"].abs()

    big, out = nan_out(m, n, ys)
    got = ops.gemm_nt(c["x"], c["w"], c["b"], ops.EPI_NONE, out=out)
    assert got is out
    check(got, z, a, f"none {m}x{n}x{k}")
    untouched(big, n)

    big, out = nan_out(m, n, ys)
    got = ops.gemm_nt(c["x"], c["w"], c["b"], ops.EPI_GELU, out=out)
    check(got, F.gelu(z), 1.2 * a + 1e-3, f"gelu {m}x{n}x{k}")
    untouched(big, n)

    big, out = nan_out(m, n, ys)
    if ys:   # residual with the same row stride as the output, in a buffer of its own
        rbig = torch.full((m, n + 24), float("nan"), device="cuda")
        rbig[:, 8:8 + n] = c["res"].cuda()
        r = rbig[:, 8:8 + n]
    else:
        r = c["res"].cuda()
    got = ops.gemm_nt(c["x"], c["w"], None, ops.EPI_RESIDUAL, residual=r, out=out)
    check(got, c["xw"] + c["res64"], c["axw"] + c["res64"].abs(), f"residual {m}x{n}x{k}")
    untouched(big, n)
    assert torch.equal(r.cpu(), c["res"]), "the residual was written"


@pytest.mark.parametrize("m,n,k,want", DECODE_LN)
def test_gemm_ln_decode_forms_vs_float64(ops, m, n, k, want):
    """ops.gemm_ln on the decode forms: the row statistics come from the K slices' own loads (`ln_accum` in the batches and in
    the remainder steps, summed over the waves) -- non-zero-mean rows, a strided x, plain into a dense NaN buffer and GELU into a view."""
    assert plan(m, n, k, True) == want and want[2] == 1
    g = torch.Generator().manual_seed(m + 11 * n + k)
    x_cpu, x, w, b, _ = operands(g, m, n, k, True, shift=True)
    gamma, beta = 1 + 0.3 * torch.randn(k, generator=g), 0.2 * torch.randn(k, generator=g)
    packed = ops.pack_ln_linear(w, b, gamma, beta)
    ref, a = ln_reference(x_cpu, packed)
    pk = [t.cuda() for t in packed]
    _, out = nan_out(m, n, False)
    check(ops.gemm_ln(x, *pk, epilogue=ops.EPI_NONE, out=out), ref, a, f"ln {m}x{n}x{k}")
    big, out = nan_out(m, n, True)
    check(ops.gemm_ln(x, *pk, epilogue=ops.EPI_GELU, out=out), F.gelu(ref), 1.2 * a + 1e-3, f"ln gelu {m}x{n}x{k}")
    untouched(big, n)


def test_gemm_split_k_workspace_between_shapes(ops):
    """The six split-K shapes, each twice, interleaved on one stream (A B C A C B D E F D F E): a 16 x 16 block's slabs and arrival
    counter sit at (row block) * cdiv(N, 16) + column block, so launches of different N and M reuse one another's counters and
    slabs in another arrangement.  Every result meets the float64 bound and equals the first run of its shape bit for bit: a
    counter left non-zero leaves NaN behind (nobody draws the last ticket), a slab read before its store misses the bound."""
    order = [0, 1, 2, 0, 2, 1, 3, 4, 5, 3, 5, 4]
    first = {}
    for step, (i, j) in enumerate(zip(order, order[1:] + [None])):
        m, n, k, xs = SPLIT_K[i]
        assert j is None or SPLIT_K[j][:2] != (m, n)
        assert plan(m, n, k, False)[2] > 1
        c = nt_case(m, n, k, xs)
        _, out = nan_out(m, n, False)
        got = ops.gemm_nt(c["x"], c["w"], c["b"], ops.EPI_NONE, out=out)
        check(got, c["xw"] + c["b64"], c["axw"] + c["b64"].abs(), f"launch {step}: {m}x{n}x{k}")
        if i in first:
            assert torch.equal(got, first[i]), f"launch {step}: {m}x{n}x{k} differs from the first run of its shape"
        else:
            first[i] = got


@pytest.mark.parametrize("B,C,H,tmax,pos0,pos_dev,want", DECODE_QKV)
def test_gemm_ln_qkv_decode_form(ops, B, C, H, tmax, pos0, pos_dev, want):
    """ops.gemm_ln_qkv with Tq = 1, what every decode step runs: q and the one written slot of both caches against float64,
    every other slot still NaN."""
    assert plan(B, 3 * C, C, True) == want
    D = C // H
    g = torch.Generator().manual_seed(B + C + pos0)
    x = torch.randn(B, C, generator=g) * 0.7 + 0.3
    w, b = torch.randn(3 * C, C, generator=g) / C ** 0.5, torch.randn(3 * C, generator=g)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    packed = ops.pack_ln_linear(w, b, gamma, beta)
    ref, a = ln_reference(x, packed)
    kc = torch.full((B, H, tmax, D), float("nan"), device="cuda")
    vc = torch.full((B, H, tmax, D), float("nan"), device="cuda")
    q = torch.full((B, C), float("nan"), device="cuda")
    pd = torch.tensor([pos_dev], dtype=torch.int32, device="cuda") if pos_dev is not None else None
    got = ops.gemm_ln_qkv(x.cuda(), *[t.cuda() for t in packed], kc, vc, B, 1, pos0, pd, out=q)
    assert got is q
    pos = pos0 + (pos_dev or 0)
    assert pos < tmax
    check(q, ref[:, :C], a[:, :C], "q")
    check(kc[:, :, pos], ref[:, C:2 * C].view(B, H, D), a[:, C:2 * C].view(B, H, D), "k cache")
    check(vc[:, :, pos], ref[:, 2 * C:].view(B, H, D), a[:, 2 * C:].view(B, H, D), "v cache")
    for cache in (kc, vc):
        assert torch.isnan(cache[:, :, :pos]).all() and torch.isnan(cache[:, :, pos + 1:]).all(), "a slot other than pos was written"


def rows_vs_m(ops, n, k):
    """Rows 0..15 of gemm_nt at M = 16 against the same rows of the INVARIANT_M launches, plain and residual epilogues:
    [(M, epilogue, differing elements)] of the launches that differ."""
    g = torch.Generator().manual_seed(n + k)
    _, x, w, b, res = operands(g, max(INVARIANT_M), n, k)
    w, b, res = w.cuda(), b.cuda(), res.cuda()

    def run(m):
        outs = [nan_out(m, n, False)[1] for _ in range(2)]
        ops.gemm_nt(x[:m], w, b, ops.EPI_NONE, out=outs[0])
        ops.gemm_nt(x[:m], w, None, ops.EPI_RESIDUAL, residual=res[:m], out=outs[1])
        assert all(torch.isfinite(o).all() for o in outs), (m, n, k)
        return [o[:16] for o in outs]

    base = run(16)
    return [(m, name, int((got != want).sum())) for m in INVARIANT_M for name, got, want in zip(("none", "residual"), run(m), base)
            if not torch.equal(got, want)]


@pytest.mark.parametrize("n,k", INVARIANT_NK)
def test_gemm_rows_do_not_depend_on_m_under_split_k(ops, n, k):
    """A row's K partition, hence its bits, is a function of N and K only -- the grouped decode step relies on it to equal one
    step per batch.  (2048, 2048) is the shape at which kz used to follow M: kz 2 up to 128 rows, 1 beyond -- 128 column tiles
    times more than 8 row blocks did not fit the workspace.)"""
    assert len({plan(m, n, k, False)[1:3] for m in [16] + INVARIANT_M}) == 1
    assert rows_vs_m(ops, n, k) == []

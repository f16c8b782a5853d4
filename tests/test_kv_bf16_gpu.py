"""-m gpu: the kernels of the bf16 KV-cache mode (ccvs_amd/csrc/attention.hip: `kv_append_bf16_kernel`, `attention_prefill_kernel<D, KvBf16>`,
`attention_decode_bf16_kernel<D>`; their bodies, shared with the fp32 kernels, in ccvs_amd/csrc/attention_core.h) through `ops.kv_append_bf16` and
`ops.attention_bf16`, against tests/kv_bf16_ref.py: stored bits against the integer rounding, outputs against the float64 attention over
the ROUNDED cache within the derived per-element bound of tests/attention_ref.py (a bf16 value is an exact fp32 value: the bound holds
unchanged).  Geometry and poisoning are those of tests/test_attention_forms_gpu.py: B = 2, H = 3, q the middle third of a NaN-filled
[B,Tq,3HD] buffer, every cache row that must not be read NaN, D in {16, 32, 64}.

  append          Tq in {1, 5}, host and device position, a strided source view, positions at Tmax - 1 and one beyond (skipped, the poison
                  behind it survives), rows outside the appended range keep their poison.
  decode sweep    every length 1 .. 2 BATCH + 1 (BATCH = 8192 / D rows, from the kernel's constants, pinned) and three lengths ending at
                  3 BATCH + 5, by host and by device position (bit-identical), each in the APPENDING form (row L-1 of the cache starts
                  as NaN and must end as the rounded row) and in the pre-appended form: same output bits.
  prefill grid    Tq x pos0 around the 32-key tile, the 32-query block and the 128-query workgroup; exact end or NaN tail.
  score patterns  unit, q x 8, key 0 dominant, rising; both forms.
  cross-form      query t of a prefill against the decode step at pos0 + t, within the sum of the two bounds.
  row groups      three groups with different device-resident lengths in ONE launch (grp_rows = 2), appending: each group against float64
                  at its length, bit-identical to one launch per group; exactly the rounded rows at each group's position are written.
  CU budget       each launch form once under a stream CU mask into poisoned outputs: same results as unmasked.
  dtype guards    a mixed-dtype call raises ValueError and writes nothing.

MUTATIONS of the kernels (then in a file of their own, attention_kv16.hip; the statements are the ones attention_core.h holds for the bf16
policy), each built once by hand into a library of its own and run against this file and
tests/test_kv_bf16_step_gpu.py on an MI355X (41 tests; none is committed):
  * truncation instead of round-to-nearest-even (`bf16_rne` returns u >> 16): 31 fail -- append (the stored bits), the decode sweep (the
    appended rows are not the reference rounding), every test that attends through the appending form, and in the step file the layer-0
    cache against the rounding of the fp32 cache and the chain's stored K row against the rounded GEMM row.  The prefill grid passes: it
    reads caches that the test itself rounded.
  * the current position's row taken un-rounded (score and value of row L-1 from the fp32 rows): 26 fail -- the decode sweep (appending
    and pre-appended outputs differ, and the output leaves the bound of the reference over the rounded cache), score patterns, cross-form,
    row groups, CU budget, and the chain's logits against the per-op composition on the stored cache.  Append and layer-0 bits pass: what is
    STORED is still right.
  * the `j < L` select of the PV pass removed: 25 fail -- every decode length that is no multiple of the slot stride counts row L-1 again
    (sweep, patterns, cross-form, row groups, CU budget) and the Transformer's greedy stream no longer is the argmax of its own
    teacher-forced logits.  The step file's exact comparisons pass: every form makes the same mistake.
  * K and V row pointers swapped in the appending form: 29 fail -- the sweep (stored rows and outputs), patterns, cross-form, row groups, CU
    budget, layer-0 cache bits, the chain against the composition, the Transformer stream."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_ref as R  # noqa: E402
import kv_bf16_ref as K  # noqa: E402

pytestmark = pytest.mark.gpu

B, H = 2, 3
DS = (16, 32, 64)
NAN = float("nan")
BF16_NAN = 0x7fc0


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ccvs_amd import ops as _ops
    return _ops


def decode_batch(d):
    """Rows per register batch of attention_decode_item<D, KvBf16, false> (attention_decode_bf16_kernel), from its own constants (EPL = 8
    head dims per lane, AU = 4 rows in flight); pinned so that a
    change of the kernel's batching fails here instead of silently moving the edges out of the sweep."""
    epl = 8
    lpk = d // epl          # lanes per key row
    kpi = 64 // lpk         # key rows per wave-instruction
    au = 32 // epl          # rows per lane in flight
    batch = 4 * kpi * au    # NW = 4 waves
    assert batch == 8192 // d == {16: 512, 32: 256, 64: 128}[d]
    return batch


def q_view(q):
    """q [B,H,Tq,D] fp32 (CPU) -> the [B,Tq,H*D] middle third of a NaN-filled [B,Tq,3*H*D] buffer on the GPU."""
    b, h, tq, d = q.shape
    buf = torch.full((b, tq, 3 * h * d), NAN, device="cuda")
    view = buf[..., h * d:2 * h * d]
    view.copy_(q.transpose(1, 2).reshape(b, tq, h * d))
    return view


def qkv_rows(q, k, v, t):
    """Row t of q, k, v [B,H,T,D] (CPU) as the three thirds of one [B,1,3*H*D] buffer on the GPU: what a decode step's QKV GEMM leaves."""
    b, h, _, d = q.shape
    buf = torch.cat([x[:, :, t].reshape(b, 1, h * d) for x in (q, k, v)], dim=-1).cuda()
    c = h * d
    return buf[..., :c], buf[..., c:2 * c], buf[..., 2 * c:]


def cache16(x, tmax):
    """x [B,H,L,D] fp32 (CPU) -> bf16 [B,H,tmax,D] on the GPU holding the reference rounding of x, rows L.. NaN."""
    b, h, length, d = x.shape
    c = torch.full((b, h, tmax, d), NAN, device="cuda", dtype=torch.bfloat16)
    c[:, :, :length] = K.bf16_round(x).cuda().to(torch.bfloat16)    # exact: the values are bf16 already
    return c


def heads(out, d):
    b, t, hd = out.shape
    return out.view(b, t, hd // d, d).transpose(1, 2)


def reference(q, k, v, pos0):
    """float64 on the GPU over the ROUNDED cache."""
    return R.attention_ref(q.cuda().double(), K.bf16_round(k).cuda().double(), K.bf16_round(v).cuda().double(), pos0)


def check(got, want, tol, what):
    g = heads(got, want.shape[-1]).double()
    assert g.shape == want.shape, (what, g.shape, want.shape)
    assert torch.isfinite(g).all().item(), f"{what}: non-finite output (an unwritten cache row or a padding lane leaked)"
    ratio = ((g - want).abs() / tol).max().item()
    print(f"{what}: max err/tol = {ratio:.4f}")
    assert ratio <= 1.0, f"{what}: max err/tol = {ratio:.4f}"
    return ratio


# ------------------------------------------------------------------ 1 append
@pytest.mark.parametrize("d", DS)
def test_append_rounds_and_scatters(ops, d):
    tmax = 11
    g = torch.Generator().manual_seed(40 + d)
    for tq, pos0, dev in [(1, 0, False), (1, 4, True), (5, 3, False), (5, 6, True), (1, tmax - 1, False), (1, tmax - 1, True), (2, tmax - 1, True)]:
        src = torch.full((B, tq, 3 * H * d), NAN)
        kv = torch.randn(B, tq, 2 * H * d, generator=g) * torch.exp2(torch.randint(-20, 20, (B, tq, 2 * H * d), generator=g).float())
        src[..., H * d:] = kv
        src = src.cuda()
        kview, vview = src[..., H * d:2 * H * d], src[..., 2 * H * d:]     # strided: row stride 3 H D
        kc = torch.full((B, H, tmax, d), NAN, device="cuda", dtype=torch.bfloat16)
        vc = torch.full((B, H, tmax, d), NAN, device="cuda", dtype=torch.bfloat16)
        if dev:   # (the host sees positions 0 .. tq only: the device word moves them, here up to one row beyond the cache)
            ops.kv_append_bf16(kview, vview, kc, vc, 0, torch.tensor([pos0], dtype=torch.int32, device="cuda"))
        else:
            ops.kv_append_bf16(kview, vview, kc, vc, pos0)
        for cache, col in ((kc, 0), (vc, H * d)):
            want = torch.full((B, H, tmax, d), BF16_NAN, dtype=torch.int32)
            rows = K.bf16_bits(kv[..., col:col + H * d].contiguous()).view(B, tq, H, d).permute(0, 2, 1, 3)
            n = min(tq, tmax - pos0)      # a position at or beyond Tmax is skipped
            want[:, :, pos0:pos0 + n] = rows[:, :, :n]
            got = K.bits_of(cache.cpu())
            assert torch.equal(got, want), (d, tq, pos0, dev, (got != want).nonzero()[:4].tolist())
    # refused on the host: positions beyond the cache, nothing written
    kc = torch.full((B, H, tmax, d), NAN, device="cuda", dtype=torch.bfloat16)
    x = torch.zeros(B, 2, H * d, device="cuda")
    from ccvs_amd import lib
    with pytest.raises(lib.CcvsError, match="exceed cache"):
        ops.kv_append_bf16(x, x, kc, kc.clone(), tmax - 1)
    assert torch.isnan(kc).all().item()


# ------------------------------------------------------------------ 2 decode sweep
def decode_growing(ops, q, k, v, tmax, first, pd):
    """Decode calls at lengths first .. tmax.  The appending form runs on a cache whose rows >= L-1 are NaN and writes row L-1 itself;
    the pre-appended form runs on a second cache whose row L-1 was written by plain torch indexing (the reference rounding).
    -> (appending by host position, appending by device position, pre-appended by host position, pre-appended by device position), each
    [B, n, H*D]; the appending caches at the end.  No sync inside."""
    kc_a, vc_a = cache16(k[:, :, :first - 1], tmax), cache16(v[:, :, :first - 1], tmax)
    kc_d, vc_d = kc_a.clone(), vc_a.clone()
    kc_p, vc_p = kc_a.clone(), vc_a.clone()
    k16, v16 = K.bf16_round(k).cuda().to(torch.bfloat16), K.bf16_round(v).cuda().to(torch.bfloat16)
    outs = [[], [], [], []]
    for length in range(first, tmax + 1):
        qrow, krow, vrow = qkv_rows(q, k, v, length - 1)
        outs[0].append(ops.attention_bf16(qrow, kc_a, vc_a, length - 1, kv_new=(krow, vrow)))
        outs[1].append(ops.attention_bf16(qrow, kc_d, vc_d, 0, pd[length - 1:length], kv_new=(krow, vrow)))
        kc_p[:, :, length - 1] = k16[:, :, length - 1]
        vc_p[:, :, length - 1] = v16[:, :, length - 1]
        qv = q_view(q[:, :, length - 1:length])
        outs[2].append(ops.attention_bf16(qv, kc_p, vc_p, length - 1))
        outs[3].append(ops.attention_bf16(qv, kc_p, vc_p, 0, pd[length - 1:length]))
    return [torch.cat(o, 1) for o in outs], (kc_a, vc_a, kc_d, vc_d)


@pytest.mark.parametrize("d", DS)
def test_decode_every_length_both_forms(ops, d):
    batch = decode_batch(d)
    worst = 0.0
    for tmax, first in [(2 * batch + 1, 1), (3 * batch + 5, 3 * batch + 3)]:
        q, k, v = R.make_inputs("unit", B, H, tmax, tmax, d, seed=1000 + d + tmax)
        pd = torch.arange(tmax, dtype=torch.int32, device="cuda")
        (app_h, app_d, pre_h, pre_d), caches = decode_growing(ops, q, k, v, tmax, first, pd)
        want, tol = reference(q[:, :, first - 1:], k, v, first - 1)
        worst = max(worst, check(app_h, want, tol, f"decode D={d} L={first}..{tmax} appending"))
        check(pre_h, want, tol, f"decode D={d} L={first}..{tmax} pre-appended")
        assert torch.equal(app_h, app_d) and torch.equal(pre_h, pre_d), "host position and device position differ"
        assert torch.equal(app_h, pre_h), "the appending and the pre-appended form differ"
        for cache, src in zip(caches, (k, v, k, v)):   # every row the appending calls wrote is the reference rounding, bit for bit
            assert torch.equal(K.bits_of(cache.cpu()), K.bf16_bits(src)), "appended rows are not the reference rounding"
    print(f"decode D={d}: largest err/tol = {worst:.4f}")


# ------------------------------------------------------------------ 3 prefill grid
PREFILL_TQ = (2, 31, 32, 33, 127, 128, 129, 257)
PREFILL_POS0 = (0, 1, 31, 32, 33, 95)


@pytest.mark.parametrize("d", DS)
def test_prefill_grid(ops, d):
    worst = 0.0
    for tq in PREFILL_TQ:
        for pos0 in PREFILL_POS0:
            length = pos0 + tq
            tmax = length if pos0 % 2 == 0 else length + 37    # the cache ends exactly at the last query, or has a NaN tail
            q, k, v = R.make_inputs("unit", B, H, tq, length, d, seed=2000 + 7 * tq + pos0)
            qv, kc, vc = q_view(q), cache16(k, tmax), cache16(v, tmax)
            got = ops.attention_bf16(qv, kc, vc, pos0)
            got_dev = ops.attention_bf16(qv, kc, vc, 0, torch.tensor([pos0], dtype=torch.int32, device="cuda"))
            want, tol = reference(q, k, v, pos0)
            worst = max(worst, check(got, want, tol, f"prefill D={d} Tq={tq} pos0={pos0} Tmax={tmax}"))
            assert torch.equal(got, got_dev), "host position and device position differ"
    print(f"prefill D={d}: largest err/tol = {worst:.4f}")


# ------------------------------------------------------------------ 4 score patterns
@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("d", DS)
def test_score_patterns(ops, d, pattern):
    for form, tq, pos0 in [("prefill", 129, 127), ("decode", 1, decode_batch(d))]:
        length = pos0 + tq
        q, k, v = R.make_inputs(pattern, B, H, tq, length, d, seed=200 + d)
        R.pattern_property(pattern, q, k, pos0)
        want, tol = reference(q, k, v, pos0)
        got = ops.attention_bf16(q_view(q), cache16(k, length + 37), cache16(v, length + 37), pos0)
        check(got, want, tol, f"{form} D={d} {pattern}")
        if form == "decode":
            kc, vc = cache16(k[:, :, :pos0], length + 37), cache16(v[:, :, :pos0], length + 37)
            k1 = k[:, :, pos0:].transpose(1, 2).reshape(B, 1, H * d).cuda()
            v1 = v[:, :, pos0:].transpose(1, 2).reshape(B, 1, H * d).cuda()
            app = ops.attention_bf16(q_view(q), kc, vc, pos0, kv_new=(k1, v1))
            assert torch.equal(app, got), f"decode D={d} {pattern}: the appending form differs"


# ------------------------------------------------------------------ 5 cross-form
@pytest.mark.parametrize("d", DS)
def test_prefill_row_equals_decode_step(ops, d):
    tq, pos0 = 97, 40
    length = pos0 + tq
    q, k, v = R.make_inputs("unit", B, H, tq, length, d, seed=3000 + d)
    qv = q_view(q)
    pre = ops.attention_bf16(qv, cache16(k, length + 37), cache16(v, length + 37), pos0)
    kc, vc = cache16(k[:, :, :pos0], length + 37), cache16(v[:, :, :pos0], length + 37)
    steps = []
    for t in range(tq):
        krow, vrow = k[:, :, pos0 + t].reshape(B, 1, H * d).cuda(), v[:, :, pos0 + t].reshape(B, 1, H * d).cuda()
        steps.append(ops.attention_bf16(qv[:, t:t + 1], kc, vc, pos0 + t, kv_new=(krow, vrow)))
    dec = torch.cat(steps, 1)
    want, tol = reference(q, k, v, pos0)
    check(pre, want, tol, f"cross-form D={d} prefill")
    check(dec, want, tol, f"cross-form D={d} decode")
    ratio = ((heads(pre, d).double() - heads(dec, d).double()).abs() / (2 * tol)).max().item()
    print(f"cross-form D={d}: max |prefill - decode| / (tol_p + tol_d) = {ratio:.4f}")
    assert ratio <= 1.0


# ------------------------------------------------------------------ 6 row groups
@pytest.mark.parametrize("d", DS)
def test_row_groups_with_their_own_lengths(ops, d):
    """Three groups of two rows, each at its own device-resident length, in ONE launch of the decode kernel (grp_rows = 2: the launch
    form of the grouped decode step), appending: against the float64 reference of every group at its length, bit-identical to one
    launch per group, and the rows written are the rounded rows at each group's own position -- nothing else of the caches moves."""
    batch = decode_batch(d)
    rows, tmax = 6, batch + 40
    lens = [batch + 1, 7, batch - 1]            # cache lengths AFTER the append, one per group
    q, k, v = R.make_inputs("unit", rows, H, 1, tmax, d, seed=4000 + d)
    kc = torch.full((rows, H, tmax, d), NAN, device="cuda", dtype=torch.bfloat16)
    vc = kc.clone()
    newk, newv = torch.zeros(rows, 1, H * d), torch.zeros(rows, 1, H * d)
    for g, n in enumerate(lens):
        sl = slice(2 * g, 2 * g + 2)
        kc[sl, :, :n - 1] = K.bf16_round(k[sl, :, :n - 1]).cuda().to(torch.bfloat16)
        vc[sl, :, :n - 1] = K.bf16_round(v[sl, :, :n - 1]).cuda().to(torch.bfloat16)
        newk[sl] = k[sl, :, n - 1].reshape(2, 1, H * d)
        newv[sl] = v[sl, :, n - 1].reshape(2, 1, H * d)
    buf = torch.cat([q.transpose(1, 2).reshape(rows, 1, H * d), newk, newv], dim=-1).cuda()
    c = H * d
    qv, kn, vn = buf[..., :c], buf[..., c:2 * c], buf[..., 2 * c:]
    # one launch per group through the op (a group is a batch of its own there) ...
    per_group = []
    for g, n in enumerate(lens):
        sl = slice(2 * g, 2 * g + 2)
        kg, vg = kc[sl].clone(), vc[sl].clone()
        per_group.append(ops.attention_bf16(qv[sl], kg, vg, 0, torch.tensor([n - 1], dtype=torch.int32, device="cuda"), kv_new=(kn[sl], vn[sl])))
        want, tol = R.attention_ref(q[sl].cuda().double(), K.bf16_round(k[sl, :, :n]).cuda().double(), K.bf16_round(v[sl, :, :n]).cuda().double(), n - 1)
        check(per_group[-1], want, tol, f"row group {g} D={d} L={n}")
    # ... and all three in one launch
    before_k, before_v = K.bits_of(kc.cpu()), K.bits_of(vc.cpu())
    pos = torch.tensor([n - 1 for n in lens], dtype=torch.int32, device="cuda")
    got = ops.attention_bf16(qv, kc, vc, 0, pos, kv_new=(kn, vn), grp_rows=2)
    assert torch.equal(got, torch.cat(per_group, 0)), "rows of a grouped launch differ from their group run alone"
    for cache, before, new in ((kc, before_k, newk), (vc, before_v, newv)):
        want = before.clone()
        for g, n in enumerate(lens):
            want[2 * g:2 * g + 2, :, n - 1] = K.bf16_bits(new[2 * g:2 * g + 2, 0].contiguous()).view(2, H, d)
        assert torch.equal(K.bits_of(cache.cpu()), want), "a grouped append wrote the wrong rows"
    # the pre-appended form on the caches the grouped launch left: same bits
    assert torch.equal(ops.attention_bf16(qv, kc, vc, 0, pos, grp_rows=2), got)


# ------------------------------------------------------------------ 7 CU budget
@pytest.mark.parametrize("d", DS)
def test_under_a_cu_budget(ops, d):
    """Each launch form once on a stream with a CU budget (`ops.stream_cu_limit`: the stream's CU mask), into poisoned outputs: the
    same bits as on the unbudgeted stream."""
    batch = decode_batch(d)
    q, k, v = R.make_inputs("unit", B, H, 130, 130 + batch, d, seed=5000 + d)
    tmax = 130 + batch + 3

    def run():
        res = []
        qv = q_view(q)
        kc, vc = cache16(k[:, :, :batch], tmax), cache16(v[:, :, :batch], tmax)
        kview = k[:, :, batch:].transpose(1, 2).reshape(B, 130, H * d).cuda()
        vview = v[:, :, batch:].transpose(1, 2).reshape(B, 130, H * d).cuda()
        ops.kv_append_bf16(kview[:, :129], vview[:, :129], kc, vc, batch)
        res += [kc.clone(), vc.clone()]
        res.append(ops.attention_bf16(qv[:, :129], kc, vc, batch))                                                   # prefill
        res.append(ops.attention_bf16(qv[:, 129:], kc, vc, batch + 129, kv_new=(kview[:, 129:], vview[:, 129:])))     # decode, appending
        res.append(ops.attention_bf16(qv[:, 129:], kc, vc, batch + 129))                                             # decode, pre-appended
        res += [kc, vc]
        return res

    plain = run()
    side = torch.cuda.Stream()
    ops.stream_cu_limit(side, 8)
    try:
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            masked = run()
        torch.cuda.current_stream().wait_stream(side)
    finally:
        ops.stream_cu_limit(side, 0)
    torch.cuda.synchronize()
    for i, (a, b_) in enumerate(zip(plain, masked)):
        if a.dtype == torch.bfloat16:
            assert torch.equal(K.bits_of(a.cpu()), K.bits_of(b_.cpu())), i
        else:
            assert torch.isfinite(b_).all().item() and torch.equal(a, b_), i
    want, tol = reference(q[:, :, :129], k[:, :, :batch + 129], v[:, :, :batch + 129], batch)
    check(masked[2], want, tol, f"budgeted prefill D={d}")
    want, tol = reference(q[:, :, 129:], k, v, batch + 129)
    check(masked[3], want, tol, f"budgeted decode D={d}")
    assert torch.equal(masked[3], masked[4])


# ------------------------------------------------------------------ 8 dtype guards
def test_mixed_dtype_calls_raise_and_write_nothing(ops):
    d, tmax = 16, 9
    k32 = torch.full((B, H, tmax, d), NAN, device="cuda")
    k16 = torch.full((B, H, tmax, d), NAN, device="cuda", dtype=torch.bfloat16)
    x = torch.ones(B, 1, H * d, device="cuda")
    calls = [
        lambda: ops.kv_append_bf16(x, x, k32, k32, 0),
        lambda: ops.kv_append_bf16(x, x, k16, k32, 0),
        lambda: ops.attention_bf16(x, k32, k32, 0),
        lambda: ops.attention_bf16(x, k16, k32, 0, kv_new=(x, x)),
        lambda: ops.kv_append(x, x, k16, k16, 0),
        lambda: ops.attention(x, k16, k16, 0),
        lambda: ops.attention(x, k32, k16, 0),
        lambda: ops.kv_append_bf16(x.double(), x.double(), k16, k16, 0),
        lambda: ops.attention_bf16(x, k16, k16, 0, kv_new=(x.half(), x.half())),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
    xs = torch.ones(B * 1, H * d, device="cuda")
    with pytest.raises(ValueError):
        ops.gemm_ln_qkv(xs, torch.ones(3 * H * d, H * d, device="cuda"), torch.ones(3 * H * d, device="cuda"), torch.ones(3 * H * d, device="cuda"),
                        k16, k16, B, 1, 0)
    with pytest.raises(ValueError, match="Tq = 1"):
        ops.attention_bf16(torch.ones(B, 2, H * d, device="cuda"), k16, k16, 0, kv_new=(x, x))
    torch.cuda.synchronize()
    assert torch.isnan(k32).all().item() and torch.isnan(k16).all().item(), "a refused call wrote into a cache"

"""-m gpu: both forms of the KV-cached causal attention (`attention_prefill_kernel<16|32|64, KvF32>`, `attention_decode_kernel<16|32|64>`,
ccvs_amd/csrc/attention.hip; their bodies in attention_core.h, shared with the bf16 caches) through `ops.attention`, against the float64 reference and the derived per-element bound of tests/attention_ref.py
(what the bound can and cannot tell apart is tests/test_attention_ref_host.py).

Every case has B = 2 and H = 3 (H is no power of two: b = bh / H matters), q is the middle third of a [B, Tq, 3*H*D] buffer whose
other thirds are NaN (the strided view that the fused QKV output is), every cache row that a valid call must not use is NaN,
and every element is asserted |got - want| <= tol; the largest err / tol of each case is printed.

  decode sweep   every length 1 .. 2*BATCH + 1 of a cache that grows by one written row per call (BATCH = the decode form's
                 register batch, 4 waves x 64 / (D/4) rows x 4: every residue of L modulo the slot stride is the last valid
                 row once, with the first unwritten row right behind it; the last length fills the cache), by host position
                 and by device-resident position, bit-identical; three lengths ending at 3*BATCH + 5.
  prefill grid   Tq x pos0 around the 32-key tile, the 32-query wave block and the 128-query workgroup, the cache ending
                 exactly at pos0 + Tq (the min(.., Tmax) of ntiles, the clamp row on the last tile) or with a NaN tail.
  score patterns unit, q x 8, key 0 dominant, scores rising with the key index (attention_ref.make_inputs says what each is
                 meant to reach), both forms.
  cross-form     query t of a prefill against the decode step at position pos0 + t: mingpt._layers switches between the forms
                 by tq and a clip's tokens pass through both.

What a broken guard would do here, by the host test's mutations (unit scale: each exceeds tol by 10 x to 10^4 x):
  * decode, the `j < L` select of the PV pass gone: every tail slot of the last batch adds the clamped row L-1 once more, a key
    counted twice or more (at least the weight that "one key dropped" removes), at every length that is no multiple of the
    slot stride; the clamp `min(.., L-1)` off by one instead reads the NaN row L: the finiteness assertion of that length.
  * prefill, the staging of rows >= pos0 + Tq: `fetch` guards them twice, the address clamp and the `written` zero-fill.
    Without both, every odd-pos0 case stages NaN rows and 0 x NaN reaches the PV product: the finiteness assertion.  Without
    the zero-fill alone the tail holds copies of the last written row, every one of them with p = 0 by the score select: the
    result is bit for bit the same and no test can or should tell; the select one key too long is "mask one key longer".
  * prefill, `acc_o *= alpha` gone or skipped by a wrong `rescale`: "no rescale between tiles", every case of two tiles or more
    whose maximum is not in tile 0, and the rising pattern in every tile.

Measured on an MI355X, largest err / tol over all cases of this file: prefill 0.053 / 0.040 / 0.026 and decode 0.022 / 0.013 /
0.0055 for D = 16 / 32 / 64 (torch's fp32 attention on a CPU: at most 0.05)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

B, H = 2, 3
DS = (16, 32, 64)
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ccvs_amd import ops as _ops
    return _ops


def decode_batch(d):
    """Rows per register batch of attention_decode_item<D, KvF32, COH> (attention_core.h), from its own constants; the values are pinned so that a change of the
    kernel's batching fails here instead of silently moving the edges out of the sweep."""
    lpk = d // 4            # lanes per key row
    kpi = 64 // lpk         # key rows per wave-instruction
    batch = 16 * kpi        # NW = 4 waves x AU = 4 rows in flight per lane
    assert batch == {16: 256, 32: 128, 64: 64}[d]
    return batch


def q_view(q):
    """q [B,H,Tq,D] fp32 (CPU) -> the [B,Tq,H*D] middle third of a NaN-filled [B,Tq,3*H*D] buffer on the GPU."""
    b, h, tq, d = q.shape
    buf = torch.full((b, tq, 3 * h * d), NAN, device="cuda")
    view = buf[..., h * d:2 * h * d]
    view.copy_(q.transpose(1, 2).reshape(b, tq, h * d))
    assert view.stride() == (tq * 3 * h * d, 3 * h * d, 1)
    return view


def cache(x, tmax):
    """x [B,H,L,D] fp32 (CPU) -> [B,H,tmax,D] on the GPU, rows L.. NaN."""
    b, h, length, d = x.shape
    c = torch.full((b, h, tmax, d), NAN, device="cuda")
    c[:, :, :length] = x.cuda()
    return c


def heads(out, d):
    """[B,T,H*D] -> [B,H,T,D]."""
    b, t, hd = out.shape
    return out.view(b, t, hd // d, d).transpose(1, 2)


def reference(q, k, v, pos0):
    """float64 on the GPU from the fp32 inputs (their conversion is exact)."""
    return R.attention_ref(q.cuda().double(), k.cuda().double(), v.cuda().double(), pos0)


def check(got, want, tol, what):
    """got [B,T,H*D] fp32; want, tol [B,H,T,D] float64.  Returns max err / tol."""
    g = heads(got, want.shape[-1]).double()
    assert g.shape == want.shape, (what, g.shape, want.shape)
    assert torch.isfinite(g).all().item(), f"{what}: non-finite output (an unwritten cache row or a padding lane leaked)"
    ratio = ((g - want).abs() / tol).max().item()
    print(f"{what}: max err/tol = {ratio:.4f}")
    assert ratio <= 1.0, f"{what}: max err/tol = {ratio:.4f}"
    return ratio


def decode_growing(ops, qv, k, v, tmax, first, pd):
    """Decode calls at lengths first .. tmax on caches whose rows >= L are NaN: row L-1 is written (plain torch indexing) right
    before the two calls at length L, by host position and by device position.  Returns both [B, n, H*D], no sync inside."""
    kg, vg = k.cuda(), v.cuda()
    kc, vc = cache(k[:, :, :first - 1], tmax), cache(v[:, :, :first - 1], tmax)
    by_host, by_dev = [], []
    for length in range(first, tmax + 1):
        kc[:, :, length - 1] = kg[:, :, length - 1]
        vc[:, :, length - 1] = vg[:, :, length - 1]
        qrow = qv[:, length - 1:length]
        by_host.append(ops.attention(qrow, kc, vc, length - 1))
        by_dev.append(ops.attention(qrow, kc, vc, 0, pd[length - 1:length]))
    return torch.cat(by_host, 1), torch.cat(by_dev, 1)


@pytest.mark.parametrize("d", DS)
def test_decode_every_length_on_a_growing_poisoned_cache(ops, d):
    batch = decode_batch(d)
    worst = 0.0
    for tmax, first in [(2 * batch + 1, 1), (3 * batch + 5, 3 * batch + 3)]:
        # one causal problem: the query of length L is row L-1 and sees keys 0 .. L-1
        q, k, v = R.make_inputs("unit", B, H, tmax, tmax, d, seed=1000 + d + tmax)
        pd = torch.arange(tmax, dtype=torch.int32, device="cuda")
        got_h, got_d = decode_growing(ops, q_view(q), k, v, tmax, first, pd)
        want, tol = reference(q[:, :, first - 1:], k, v, first - 1)
        assert got_h.shape[1] == tmax - first + 1
        worst = max(worst, check(got_h, want, tol, f"decode D={d} L={first}..{tmax}"))
        assert torch.isfinite(got_d).all().item()
        assert torch.equal(got_h, got_d), "host position and device position differ"
    print(f"decode D={d}: largest err/tol = {worst:.4f}")


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
            qv, kc, vc = q_view(q), cache(k, tmax), cache(v, tmax)
            got = ops.attention(qv, kc, vc, pos0)
            got_dev = ops.attention(qv, kc, vc, 0, torch.tensor([pos0], dtype=torch.int32, device="cuda"))
            want, tol = reference(q, k, v, pos0)
            worst = max(worst, check(got, want, tol, f"prefill D={d} Tq={tq} pos0={pos0} Tmax={tmax}"))
            assert torch.equal(got, got_dev), "host position and device position differ"
    print(f"prefill D={d}: largest err/tol = {worst:.4f}")


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("d", DS)
def test_score_patterns(ops, d, pattern):
    for form, tq, pos0 in [("prefill", 129, 127), ("decode", 1, decode_batch(d))]:
        length = pos0 + tq
        q, k, v = R.make_inputs(pattern, B, H, tq, length, d, seed=200 + d)
        R.pattern_property(pattern, q, k, pos0)
        got = ops.attention(q_view(q), cache(k, length + 37), cache(v, length + 37), pos0)
        want, tol = reference(q, k, v, pos0)
        check(got, want, tol, f"{form} D={d} {pattern}")


@pytest.mark.parametrize("d", DS)
def test_prefill_row_equals_decode_step(ops, d):
    """|prefill[t] - decode[t]| <= tol_prefill[t] + tol_decode[t]: both forms compute the same float64 problem, so each has the
    same bound, and each is also held to it on its own."""
    tq, pos0 = 97, 40
    length = pos0 + tq
    q, k, v = R.make_inputs("unit", B, H, tq, length, d, seed=3000 + d)
    qv = q_view(q)
    pre = ops.attention(qv, cache(k, length + 37), cache(v, length + 37), pos0)
    # decode: the same cache, on a copy whose rows beyond each position are NaN (written one by one as the position advances)
    kg, vg = k.cuda(), v.cuda()
    kc, vc = cache(k[:, :, :pos0], length + 37), cache(v[:, :, :pos0], length + 37)
    steps = []
    for t in range(tq):
        kc[:, :, pos0 + t] = kg[:, :, pos0 + t]
        vc[:, :, pos0 + t] = vg[:, :, pos0 + t]
        steps.append(ops.attention(qv[:, t:t + 1], kc, vc, pos0 + t))
    dec = torch.cat(steps, 1)
    want, tol = reference(q, k, v, pos0)
    check(pre, want, tol, f"cross-form D={d} prefill")
    check(dec, want, tol, f"cross-form D={d} decode")
    ratio = ((heads(pre, d).double() - heads(dec, d).double()).abs() / (2 * tol)).max().item()
    print(f"cross-form D={d}: max |prefill - decode| / (tol_p + tol_d) = {ratio:.4f}")
    assert ratio <= 1.0

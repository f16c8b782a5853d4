"""No GPU: the host reference of the token pick (tests/pick_ref.py) against what it has to agree with before tests/test_pick_gpu.py
may rely on it -- Random123's known answers of Philox4x32-10, the reference's top_k_logits (ties, -inf, both zeros around the k-th
value), torch.multinomial under the same generator, and an fp32 emulation of the kernel over the GPU module's own case table: the
margin accepts every fp32 pick, and at most 2 % of a case's rows have an fp32 pick other than the float64 argmax (the condition on
the inputs that keeps the margin from hiding a kernel that picks at random among near-best entries)."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ccvs_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pick_ref as R  # noqa: E402


def _round_u32(c, k):
    """The kernel's round function (gpt.hip: philox_first), transcribed with numpy uint32 wrap-around and a 64-bit product for
    __umulhi."""
    c0, c1, c2, c3 = (np.uint32(x) for x in c)
    k0, k1 = np.uint32(k[0]), np.uint32(k[1])
    with np.errstate(over="ignore"):
        for _ in range(10):
            hi0, lo0 = np.uint32((np.uint64(0xD2511F53) * np.uint64(c0)) >> np.uint64(32)), np.uint32(0xD2511F53) * c0
            hi1, lo1 = np.uint32((np.uint64(0xCD9E8D57) * np.uint64(c2)) >> np.uint64(32)), np.uint32(0xCD9E8D57) * c2
            c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
            k0, k1 = k0 + np.uint32(0x9E3779B9), k1 + np.uint32(0xBB67AE85)
    return tuple(int(x) for x in (c0, c1, c2, c3))


KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert tuple(int(w) for w in R.philox4x32_10(*ctr, *key)) == want
    assert _round_u32(ctr, key) == want
    # vectorised over c0: the known counter among others
    c0 = np.array([5, ctr[0], 7], dtype=np.uint64)
    got = R.philox4x32_10(c0, ctr[1], ctr[2], ctr[3], *key)
    assert tuple(int(w[1]) for w in got) == want and int(got[0][0]) != want[0]


def test_uniform_rounds_as_a_uint32_to_float_conversion_and_an_fp32_add():
    """Exact rational arithmetic, rounded to nearest even, at the words where the two roundings matter: below 2^23 the sum is exact,
    from 2^23 on the 0.5 is a tie or absorbed, from 2^24 on the conversion itself rounds; 0xffffffff gives u = 1."""
    from fractions import Fraction

    def rne(fr):   # nearest fp32 of a positive rational, ties to even
        e = fr.numerator.bit_length() - fr.denominator.bit_length()
        if Fraction(2) ** e > fr:
            e -= 1
        q = fr / Fraction(2) ** (e - 23)
        n = q.numerator // q.denominator
        rem = q - n
        if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
            n += 1
        return float(Fraction(n) * Fraction(2) ** (e - 23))

    words = [0, 1, 2, 2**22 + 1, 2**23 - 1, 2**23, 2**23 + 1, 2**23 + 2, 2**24 - 1, 2**24, 2**24 + 1, 2**24 + 3, 2**25 + 2, 2**25 + 6,
             2**31 - 1, 2**31 + 128, 2**31 + 384, 2**32 - 129, 2**32 - 128, 2**32 - 1]
    got = R.uniform_f32(np.array(words, dtype=np.uint64))
    want = [rne(Fraction(rne(Fraction(w)) if w else 0) + Fraction(1, 2)) * 2.0 ** -32 for w in words]
    assert got.dtype == np.float32 and [float(x) for x in got] == want
    assert float(got[-1]) == 1.0 and float(got[0]) == 2.0 ** -33
    noise = R.exp1_noise(4096, 3, 0, 0, 1, 2)
    assert noise.dtype == np.float64 and (noise >= R.NOISE_FLOOR).all() and 0.9 < noise.mean() < 1.1
    # a launch's block: row b draws at global row row0 + b mod 2^32
    block = R.philox_noise(4, 300, (1, 2, 0xfffffffe, 7, 9))
    assert np.array_equal(block, np.stack([R.exp1_noise(300, r, 7, 9, 1, 2) for r in (0xfffffffe, 0xffffffff, 0, 1)]))
    assert not np.array_equal(R.exp1_noise(300, 0, 7, 9, 1, 2), R.exp1_noise(300, 0, 9, 7, 1, 2))


def _zero_rows(V, k, g):
    """Rows with both zeros around the k-th value: k - 1 positive values, then the k-th value +0.0 with -0.0 elsewhere, the
    reverse, and an all-zero row of mixed signs."""
    rows = []
    for kth, other in ((0.0, -0.0), (-0.0, 0.0)):
        r = -1.0 - torch.rand(V, generator=g)
        order = torch.randperm(V, generator=g)
        r[order[:k - 1]] = torch.linspace(2.0, 0.5, k - 1) if k > 1 else r[order[:0]]
        r[order[k - 1]] = kth
        r[order[k:k + max(1, (V - k) // 3)]] = other
        rows.append(r)
    z = torch.zeros(V)
    z[torch.randperm(V, generator=g)[:V // 2]] = -0.0
    rows.append(z)
    return torch.stack(rows)


@pytest.mark.parametrize("V", [5, 200, 1000])
def test_kept_is_top_k_logits(V):
    g = torch.Generator().manual_seed(V)
    for top_k in (1, 3, V - 1, V, V + 5):
        lg = torch.cat([R.case_logits(V, top_k, rows=32), _zero_rows(V, min(top_k, V - 1), g)])
        for T in R.TEMPERATURES:
            xs, mask = R.kept(lg, T, top_k)
            want_xs = lg / T
            assert np.array_equal(xs, want_xs.numpy(), equal_nan=True)
            want = O.top_k_logits(want_xs, min(top_k, V)) > float("-inf")
            # (the reference writes -inf over what it drops; an entry that is -inf to begin with is kept by `kept` when the k-th
            #  value is -inf and carries no probability either way)
            assert np.array_equal(mask & np.isfinite(xs), want.numpy()), (V, top_k, T)
    lg = _zero_rows(V, 3, g)
    xs, mask = R.kept(lg, 1.0, 3)
    zeros = (lg == 0).numpy()
    assert (mask[:, :][zeros]).all() and mask[2].all(), "-0.0 == +0.0 at the k-th value"
    assert np.signbit(xs[zeros]).any() and not np.signbit(xs[zeros]).all()
    assert R.kept(lg, 1.0, None)[1].all() and R.kept(lg, 1.0, 0)[1].all()


def test_argmax_of_scores_is_torch_multinomial():
    """The cases of tests/test_ops_gpu.py::test_sample_topk and the tie / edge tests next to it: argmax(scores64) with the host's
    Exp(1) noise == torch.multinomial on the reference's probabilities under the same generator."""
    torch.manual_seed(0)
    lg = torch.randn(16, 1024)
    sets = [(lg, 100, 0.9, 123)]
    for V, k in ((200, 7), (1000, 50)):
        sets += [(R.case_logits(V, k, rows=32), k, T, 5 + V) for T in (1.0, 0.7)]
    for lg, k, T, seed in sets:
        B, V = lg.shape
        probs = torch.softmax(O.top_k_logits(lg / T, k), -1)
        g1, g2 = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed)
        want = torch.multinomial(probs, 1, generator=g1).view(-1)
        noise = torch.empty(B, V).exponential_(1, generator=g2)
        xs, mask = R.kept(lg, T, k)
        s, d = R.scores64(xs, mask, noise.double().numpy())
        assert np.array_equal(s.argmax(1), want.numpy())
        assert R.accept(want.numpy(), s, d, R.C_HOST, mask).all() and not R.margin_only(want.numpy(), s, d, R.C_HOST).any()


def test_accept_rejects_what_is_wrong():
    xs, mask = R.kept(torch.tensor([[0.0, 1.0, 1.0, -1.0, float("-inf")]]), 1.0, 3)
    s, d = R.scores64(xs, mask)
    assert mask.tolist() == [[True, True, True, False, False]]
    assert R.accept([1], s, d, R.C_HOST, mask).all()
    for wrong in (2, 0, 3, 4, 5, -1, 0x7fffffff):      # the higher index of a tie, a lower score, masked, -inf, out of range
        assert not R.accept([wrong], s, d, R.C_HOST).any(), wrong
    s2, d2 = R.scores64(xs, np.ones_like(mask), np.array([[1.0, 1.0, 1.0 - 2.0 ** -26, 1.0, 1.0]]))
    assert R.accept([1], s2, d2, R.C_HOST).all() and R.margin_only([1], s2, d2, R.C_HOST).all() and R.accept([2], s2, d2, R.C_HOST).all()
    assert 0 < R.figure([1], s2, d2, R.C_HOST)[0] < 0.1
    idx = np.array([[1, 2, 0, 3, 4]])
    e = np.exp(np.array([-1.0, 0.0, 0.0])) / (2 + np.exp(-1.0))
    with np.errstate(divide="ignore"):
        logp = np.log(np.concatenate([e[[1, 2, 0]], [0.0, 0.0]]))[None]
    ok, _, mo, lerr = R.topn_accept(idx, logp, xs, mask, None, R.C_HOST)
    assert ok.all() and not mo.any() and lerr.max() < 1e-6
    ok, _, _, lerr = R.topn_accept(np.array([[2, 1, 0, 4, 3]]), logp + 1e-5, xs, mask, None, R.C_HOST)
    assert ok.tolist() == [[False, True, True, False, True]] and lerr[0, 0] > 1


def _philox32(B, V):
    """The kernel's own fp32 noise: fmaxf(-logf(u), 1e-30f)."""
    k0, k1, row0, step, call = R.PHILOX_WORDS
    w = R.philox4x32_10(np.arange(V, dtype=np.uint64)[None], (row0 + np.arange(B, dtype=np.uint64))[:, None], step, call, k0, k1)[0]
    return np.maximum(-np.log(R.uniform_f32(w)), np.float32(1e-30)).astype(np.float32)


_NOISE = {}


def _noises(B, V):
    """(host fp32, Philox fp32, Philox float64) noise of a [B, V] case: drawn once per shape."""
    if (B, V) not in _NOISE:
        _NOISE.clear()
        p32 = _philox32(B, V)
        _NOISE[(B, V)] = (R.case_noise(V, rows=B), p32, R.philox_noise(B, V, R.PHILOX_WORDS) if B <= R.ROWS else p32.astype(np.float64))
    return _NOISE[(B, V)]


def _self_check(lg, top_k, T, what):
    B, V = lg.shape
    xs, mask = R.kept(lg, T, top_k)
    n32, p32, p64 = _noises(B, V)
    worst = 0
    for noise32, noise64, c in ((None, None, R.C_HOST), (n32, n32.double().numpy(), R.C_HOST), (torch.from_numpy(p32), p64, R.C_PHILOX)):
        pick = R.emulate_fp32(xs, mask, noise32)
        s, d = R.scores64(xs, mask, noise64)
        assert R.accept(pick, s, d, c, mask).all(), what
        n_mo = int(R.margin_only(pick, s, d, c).sum())
        assert n_mo <= R.MARGIN_ONLY_CAP * B, (what, n_mo)
        worst = max(worst, n_mo)
    return worst


@pytest.mark.parametrize("V,top_k,T", R.SELF_CHECK)
def test_margin_self_check_on_random_logits(V, top_k, T):
    lg = torch.randn(512, V, generator=torch.Generator().manual_seed(V)) * 2
    _self_check(lg, top_k, T, (V, top_k, T))


@pytest.mark.parametrize("V", R.PICK_VOCABS)
def test_margin_self_check_on_the_gpu_cases(V):
    """Every input set of tests/test_pick_gpu.py::test_pick_vs_float64."""
    assert (R.V_PICK_MAX + 16 + 256) * 4 == 160 * 1024 and (2 * R.V_TOPN_MAX + 16 + 256) * 4 <= 160 * 1024 < (2 * R.V_TOPN_MAX + 2 + 16 + 256) * 4
    for v, top_k, T in R.CASES:
        if v == V:
            _self_check(R.case_logits(V, top_k), top_k, T, (V, top_k, T))


@pytest.mark.parametrize("V", R.TOPN_VOCABS)
def test_margin_self_check_on_the_topn_cases(V):
    for v, top_k, T in R.TOPN_CASES:
        if v == V:
            _self_check(R.case_logits(V, top_k, rows=R.TOPN_ROWS), top_k, T, (V, top_k, T))

"""-m gpu: the token pick (gpt.hip: sample_topk_row through `ops.sample_topk`, its Philox form and the pick phase of the decode step;
sample_topn_kernel through `ops.sample_topn`) against the float64 reference and the Philox mirror of tests/pick_ref.py -- every
single pick, not a histogram.  What the reference is, how the margin `m` is derived and why at most 2 % of a case's rows may differ
from the float64 argmax is in that module; tests/test_pick_host.py checks the reference itself and runs an fp32 emulation of the
kernel over the same case table (`pick_ref.CASES`, `TOPN_CASES`).

1  single pick, greedy / host noise / Philox with immediate words, V in {1, 5, 255, 256, 257, 1000, 16384} and the largest V the
   launcher accepts (40688; 40689 raises), top_k in {None, 1, 7, V - 1, V, V + 5}, temperatures {0.7, 1.0, 1.3}; logits random,
   quantised (exact ties), tied at the k-th value, constant, with -inf entries; a row-strided logits view and a strided `out` whose
   gaps keep their poison.  The Philox words (key0, key1, row0, step, call) are swept one by one against the mirror, row0 + b
   wrapping past 2^32 and step = 0xffffffff included.
2  sample_topn, n in {1, 3, V}: every round against the best of what is left, log p within its bound, no index twice, n = 1 equal to
   the single pick.
3  signed zeros at the k-th value: -0.0 == +0.0, as in the reference's float comparison.
4  rows with NaN / +inf / -inf throughout: every index inside [0, V), token 0 (top-n: 0, 1, ..., n - 1), finite rows of the same
   launch untouched.
5  the pick inside the decode step (graph replay, eager, persistent), one and three row groups: every generated token accepted for
   the logits of a teacher-forced per-op pass and the mirror's draw at (row_offset[g] + row in group, step, call, key[g]); the
   device-resident counters; a clip's tokens do not depend on its batch slot.
6  the launchers' argument errors.

Every case prints its largest (1 - s64[pick] / s64[best]) / m, its number of margin-only rows and, for top-n, its largest log p
error over the bound (run with -s to see them).

Observed on an MI355X (worst over all cases):
  single pick (355 case lines: tests 1, 3 and 5 and the word sweep): largest (1 - s64[pick] / s64[best]) / m = 0.000 and 0 margin-only
  rows in every case -- every pick is the float64 argmax; the margin was never needed.
  top-n picks (72 case lines): the same, 0.000 and 0 margin-only picks.
  top-n log p, largest error over the bound: 0.495 (V = 257, top_k = 256, T = 0.7, n = 257: the least probable entries), 0.407
  (V = 257, top_k = None, n = 257), 0.34 at n <= 3 (V = 1000, top_k = 999, host noise), 0.30 at V = 5, below 0.2 from V = 16384 on.
  With log p = logf(e_i / sum e), as the kernel formed it before this change, the same cases gave 1.75, 1.38, 0.93 and 0.88: the
  n = 257 rounds missed the bound (see `test_topn_log_p_vs_float64`).  The step form (words from `state`) and the immediate
  form agree with the mirror in every launch form and row layout: no pick of tests 1 and 5 was off.

On the parent of this change (`if (bi >= V) bi = 0`, the `-0.0` key, the top-n fallback and the double log p not yet in gpt.hip):
  case 4: `index outside [0, 300): [239, 2147483647, 2147483647, 2147483647, 101, 2147483647, ...]` from the single pick, both top_k
  (`test_non_finite_rows_return_token_0`);
  case 3: `zeros row 0 T=1.0 philox step 0: rows [0, 1, 2, 3, 4, 5, 6, 10] picked [249, 189, 162, 189, 256, 249, 189, 256], float64
  argmax [135, 200, 237, 73, 36, 30, 3, 242]` -- the -0.0 entries next to a k-th value of +0.0 are never drawn (both temperatures);
  case 2: `top-n V=257 top_k=None T=1.0 n=257 greedy: log p off by 1.38 bounds at (row, round) [[0, 170], [0, 199], [1, 250],
  [1, 252]]` (1.75 at top_k = 256, T = 0.7);
  cases 1 and 5 turned up nothing: the parent's stream is the mirror's.

Mutations of gpt.hip, each tried once by hand:
  `row0 + brow` -> `b` in the Philox counter: fails the Philox cases of test 1 at every V from 5 on (row0 = 32), the word sweep, test 5 in all 12 cases
  (one and three groups), the slot test, and the Philox parts of tests 3 and 4;
  `step` and `call` swapped: fails test 1 (every V from 5 on), the word sweep, test 5 in all 12 cases, test 3;
  `+ 0.5f` dropped from u: NOT OBSERVABLE at these sizes -- no case changes.  The half matters below a word of 2^24 only and moves
  -log u by less than 2^-24 of itself unless the word is tiny, i.e. the noise huge and the entry never picked;
  `>= thr` -> `> thr`: fails the tied and quantised rows of test 1 (every V from 5 on), test 2, the zero rows of test 3, 9 of the 12 cases of test 5."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pick_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = -7
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ccvs_amd import ops as _ops
    return _ops


def _strided(lg):
    """(row-strided logits view on a NaN-poisoned buffer, strided `out` view, its buffer)."""
    B, V = lg.shape
    buf = torch.full((B, V + 13), NAN, device="cuda")
    buf[:, :V] = lg.cuda()
    out_buf = torch.full((3 * B,), POISON, dtype=torch.int64, device="cuda")
    return buf[:, :V], out_buf[::3], out_buf


def _gaps_poisoned(out_buf):
    o = out_buf.view(-1, 3)
    return bool((o[:, 1:] == POISON).all())


_NOISE = {}


def _noise(B, V):
    """(host noise fp32 on the device, the same in float64, Philox mirror float64) of a [B, V] case."""
    if (B, V) not in _NOISE:
        _NOISE.clear()
        n32 = R.case_noise(V, rows=B)
        _NOISE[(B, V)] = (n32.cuda(), n32.double().numpy(), R.philox_noise(B, V, R.PHILOX_WORDS))
    return _NOISE[(B, V)]


def _judge(what, pick, s, d, c, mask, cap_rows=None):
    pick = pick.cpu().numpy()
    ok = R.accept(pick, s, d, c, mask)
    fig, mo = R.figure(pick, s, d, c), R.margin_only(pick, s, d, c)
    print(f"pick {what}: largest (1 - s[pick] / s[best]) / m = {fig.max():.3f}, margin-only rows {int(mo.sum())} of {len(pick)}")
    bad = np.nonzero(~ok)[0]
    assert ok.all(), f"{what}: rows {bad[:8].tolist()} picked {pick[bad[:8]].tolist()}, float64 argmax {s.argmax(1)[bad[:8]].tolist()}"
    assert mo.sum() <= R.MARGIN_ONLY_CAP * (len(pick) if cap_rows is None else cap_rows), f"{what}: {int(mo.sum())} margin-only rows"
    return float(fig.max()), int(mo.sum())


def _single_pick_case(ops, V, top_k, T):
    lg = R.case_logits(V, top_k)
    B = lg.shape[0]
    xs, mask = R.kept(lg, T, top_k)
    ndev, n64, p64 = _noise(B, V)
    view, out, out_buf = _strided(lg)
    for name, kw, noise64, c in (("greedy", {}, None, R.C_HOST), ("host noise", dict(noise=ndev), n64, R.C_HOST),
                                 ("philox", dict(philox=R.PHILOX_WORDS), p64, R.C_PHILOX)):
        out_buf.fill_(POISON)
        got = ops.sample_topk(view, top_k, T, out=out, **kw)
        assert got.data_ptr() == out.data_ptr() and _gaps_poisoned(out_buf), "the pick wrote between the elements of a strided `out`"
        s, d = R.scores64(xs, mask, noise64)
        _judge(f"V={V} top_k={top_k} T={T} {name}", got, s, d, c, mask)
        if name == "greedy":
            assert torch.equal(got, ops.sample_topk(lg.cuda(), top_k, T)), "dense and row-strided logits give different picks"


@pytest.mark.parametrize("V", [v for v in R.PICK_VOCABS if v != R.V_PICK_MAX])
def test_pick_vs_float64(ops, V):
    for v, top_k, T in R.CASES:
        if v == V:
            _single_pick_case(ops, V, top_k, T)


def test_pick_at_the_vocabulary_cap(ops):
    """The largest vocabulary the launchers take -- (V + 272) words for the single pick, (2 V + 272) for the n picks, 160 KB of LDS --
    is picked right; one more raises with the launcher's message and writes nothing."""
    from ccvs_amd.lib import CcvsError
    for v, top_k, T in R.CASES:
        if v == R.V_PICK_MAX:
            _single_pick_case(ops, v, top_k, T)
    for v, top_k, T in R.TOPN_CASES:
        if v == R.V_TOPN_MAX:
            _topn_case(ops, v, top_k, T)
    out = torch.full((2,), POISON, dtype=torch.int64, device="cuda")
    lg = torch.zeros(2, R.V_PICK_MAX + 1, device="cuda")
    with pytest.raises(CcvsError, match=f"ccvs_sample_topk: vocabulary {R.V_PICK_MAX + 1} too large"):
        ops.sample_topk(lg, 7, 1.0, out=out)
    with pytest.raises(CcvsError, match=f"ccvs_sample_topk_philox: vocabulary {R.V_PICK_MAX + 1} too large"):
        ops.sample_topk(lg, 7, 1.0, out=out, philox=R.PHILOX_WORDS)
    with pytest.raises(CcvsError, match=f"ccvs_sample_topn: vocabulary {R.V_TOPN_MAX + 1} too large"):
        ops.sample_topn(lg[:, :R.V_TOPN_MAX + 1].contiguous(), 7, 1.0, 2)
    torch.cuda.synchronize()
    assert (out == POISON).all()


SWEEP = [("base", R.PHILOX_WORDS)] + [(f"{name}={val:#x}", R.PHILOX_WORDS[:i] + (val,) + R.PHILOX_WORDS[i + 1:])
                                      for i, name, vals in ((2, "row0", (0, 0xfffffff0, 0xffffffff)), (3, "step", (0, 1, 2, 0xffffffff)),
                                                            (4, "call", (0, 3, 5, 0xffffffff)), (0, "key0", (0, 0xffffffff, 0xabcdef01)),
                                                            (1, "key1", (0, 0x80000000, 0x01234567)))
                                      for val in vals]


def test_pick_philox_words_against_the_mirror(ops):
    """Each of the five immediate words on its own: the picks are those of the mirror's draws at counter (j, row0 + b mod 2^32, step,
    call), key (key0, key1) -- row0 = 0xfffffff0 wraps from row 16 on, step = 0xffffffff is the word of a call's first pick, call = 3
    and step = 2 exchange the base's two values -- and every variant draws other tokens than the base."""
    V, top_k, T = 1000, 50, 1.0
    lg = R.case_logits(V, top_k)
    B = lg.shape[0]
    xs, mask = R.kept(lg, T, top_k)
    dev = lg.cuda()
    picks = {}
    for name, words in SWEEP:
        got = ops.sample_topk(dev, top_k, T, philox=words)
        s, d = R.scores64(xs, mask, R.philox_noise(B, V, words))
        _judge(f"philox {name}", got, s, d, R.C_PHILOX, mask)
        picks[name] = got.cpu()
    for name, got in picks.items():
        if name != "base":
            assert (got != picks["base"]).float().mean() > 0.5, f"{name} draws the base's tokens"
    assert torch.equal(picks["row0=0xfffffff0"][16:32], ops.sample_topk(dev[16:32], top_k, T, philox=R.PHILOX_WORDS[:2] + (0,) + R.PHILOX_WORDS[3:]).cpu())


_TOPN = {}


def _topn_case(ops, V, top_k, T):
    """The picks of one case, n in {1, 3, V (small V)}, greedy and host noise; -> [(what, largest log p error / bound, where)] (the
    log p figures are asserted by the log p tests, so that a miss there does not hide a pick)."""
    if (V, top_k, T) in _TOPN:
        return _TOPN[(V, top_k, T)]
    lg = R.case_logits(V, top_k, rows=R.TOPN_ROWS)
    xs, mask = R.kept(lg, T, top_k)
    n32 = R.case_noise(V, rows=R.TOPN_ROWS)
    dev, ndev = lg.cuda(), n32.cuda()
    figures = []
    for n in (1, 3, V):
        if n == V and V > 300:
            continue
        for name, noise, noise64 in (("greedy", None, None), ("host noise", ndev, n32.double().numpy())):
            idx, logp = ops.sample_topn(dev, top_k, T, n, noise=noise)
            ok, fig, mo, lerr = R.topn_accept(idx.cpu().numpy(), logp.cpu().numpy(), xs, mask, noise64, R.C_HOST)
            what = f"top-n V={V} top_k={top_k} T={T} n={n} {name}"
            print(f"pick {what}: largest (1 - s[pick] / s[best]) / m = {fig.max():.3f}, margin-only picks {int(mo.sum())} of {mo.size}, "
                  f"largest log p error / bound = {lerr.max():.3f}")
            assert ok.all(), f"{what}: (row, round) {np.argwhere(~ok)[:8].tolist()}"
            assert mo.sum() <= R.MARGIN_ONLY_CAP * mo.size, what
            srt = np.sort(idx.cpu().numpy(), axis=1)
            assert (srt[:, 1:] != srt[:, :-1]).all() and srt.min() >= 0 and srt.max() < V, f"{what}: an index twice"
            if n == 1:
                assert torch.equal(idx[:, 0], ops.sample_topk(dev, top_k, T, noise=noise)), f"{what}: n = 1 is not the single pick"
            figures.append((what, float(lerr.max()), np.argwhere(lerr > 1)[:4].tolist()))
    _TOPN[(V, top_k, T)] = figures
    return figures


def _assert_logp(figures):
    for what, worst, where in figures:
        assert worst <= 1.0, f"{what}: log p off by {worst:.2f} bounds at (row, round) {where}"


@pytest.mark.parametrize("V", [v for v in R.TOPN_VOCABS if v != R.V_TOPN_MAX])
def test_topn_vs_float64(ops, V):
    for v, top_k, T in R.TOPN_CASES:
        if v == V:
            _topn_case(ops, V, top_k, T)


@pytest.mark.parametrize("V", R.TOPN_VOCABS)
def test_topn_log_p_vs_float64(ops, V):
    """log p of every pick against float64 log(e_i / sum e) within (|d_i| + c + V / 256 + 9) * 2^-24 (pick_ref.topn_accept).

    With log p = logf(e_i / sum e) the kernel missed this at V = 257 (observed on an MI355X): with n = V the rounds that reach the
    least probable entries were off by up to 1.38 bounds (top_k = None, T = 1.0: (row, round) (0, 170), (0, 199), (1, 250), (1, 252))
    and 1.75 bounds (top_k = 256, T = 0.7).  The bound carries the roundings in front of the logarithm but not `logf`'s own: where
    |log p| is in [8, 16) one ulp of the RESULT is 2^-20 = 16 * 2^-24, against a bound of about (|d| + 16) * 2^-24 = 25 * 2^-24 there.
    The kernel now forms (x_i - max) - log(sum e) in double from the fp32 values: the difference is exact, the pick's own expf and
    division drop out, and what is left is the error of the fp32 sum and one rounding to fp32, at most |log p| * 2^-24 <=
    (|d_i| + log V) * 2^-24.  Observed since: 0.495 bounds at the worst (V = 257, top_k = 256, n = 257)."""
    for v, top_k, T in R.TOPN_CASES:
        if v == V:
            _assert_logp(_topn_case(ops, V, top_k, T))


def _zero_rows(V, k, g):
    """k - 1 positive values, the k-th value +0.0 with -0.0 elsewhere; the reverse; zeros of mixed signs throughout."""
    rows = []
    for kth, other in ((0.0, -0.0), (-0.0, 0.0)):
        r = -1.0 - torch.rand(V, generator=g)
        order = torch.randperm(V, generator=g)
        r[order[:k - 1]] = torch.linspace(2.0, 0.5, k - 1)
        r[order[k - 1]] = kth
        r[order[k:k + (V - k) // 3]] = other
        rows.append(r)
    z = torch.zeros(V)
    z[torch.randperm(V, generator=g)[:V // 2]] = -0.0
    rows.append(z)
    return torch.stack(rows)


@pytest.mark.parametrize("T", [1.0, 0.7])
def test_signed_zeros_at_the_kth_value(ops, T):
    """The k-th largest scaled logit is +0.0 with -0.0 entries elsewhere, and the reverse; a row of zeros of both signs.  The reference
    masks `out < v[-1]`, a float comparison: both zeros are kept.  The support of 4096 Philox draws per row is exactly the kept set
    (each draw also judged against the mirror); host-noise and greedy picks of both kernels are accepted against it."""
    V, k, B, steps = 260, 5, 1024, 4
    rows = _zero_rows(V, k, torch.Generator().manual_seed(5))
    xs3, mask3 = R.kept(rows, T, k)
    assert mask3.sum(1).tolist() == [k + (V - k) // 3, k + (V - k) // 3, V]
    assert all(np.signbit(xs3[i][mask3[i]]).any() and not np.signbit(xs3[i][mask3[i]]).all() for i in range(3))
    for i in range(3):
        lg = rows[i].expand(B, V).contiguous().cuda()
        xs, mask = np.broadcast_to(xs3[i], (B, V)), np.broadcast_to(mask3[i], (B, V))
        seen = np.zeros(V, dtype=bool)
        for step in range(steps):
            words = (0x1234, 0xbeef, 17, step, 2)
            got = ops.sample_topk(lg, k, T, philox=words)
            s, d = R.scores64(xs, mask, R.philox_noise(B, V, words))
            _judge(f"zeros row {i} T={T} philox step {step}", got, s, d, R.C_PHILOX, mask)
            seen[got.cpu().numpy()] = True
        missing = np.nonzero(mask3[i] & ~seen)[0]
        assert np.array_equal(seen, mask3[i]), f"row {i}: kept entries never drawn {missing[:8].tolist()} (values {xs3[i][missing[:8]].tolist()})"
    # host noise and greedy, both kernels: 64 rows, the three kinds in turn
    lg = rows.repeat(22, 1)[:64]
    xs, mask = R.kept(lg, T, k)
    ndev, n64, _ = _noise(64, V)
    for name, noise, noise64 in (("greedy", None, None), ("host noise", ndev, n64)):
        s, d = R.scores64(xs, mask, noise64)
        _judge(f"zeros T={T} {name}", ops.sample_topk(lg.cuda(), k, T, noise=noise), s, d, R.C_HOST, mask)
        idx, logp = ops.sample_topn(lg.cuda(), k, T, 3, noise=noise)
        ok, _, mo, lerr = R.topn_accept(idx.cpu().numpy(), logp.cpu().numpy(), xs, mask, noise64, R.C_HOST)
        assert ok.all() and (lerr <= 1.0).all() and mo.sum() <= R.MARGIN_ONLY_CAP * mo.size, f"zeros T={T} top-n {name}"


def _bad_rows(V, g):
    """Row -> why it has no winner.  Rows 0, 4 and 9 are finite."""
    lg = torch.randn(10, V, generator=g) * 2
    lg[1, 17] = NAN                                   # one NaN
    lg[2, V - 1] = INF                                # one +inf
    lg[3, 3], lg[3, 200] = INF, INF                   # +inf twice
    lg[5] = -INF
    lg[5, 100] = NAN                                  # NaN with -inf
    lg[6] = -INF                                      # -inf throughout
    lg[7] = NAN                                       # NaN throughout
    lg[8, 0], lg[8, 5] = NAN, INF
    return lg, [1, 2, 3, 5, 6, 7, 8], [0, 4, 9]


@pytest.mark.parametrize("top_k", [None, 7])
def test_non_finite_rows_return_token_0(ops, top_k):
    """A NaN or +inf logit, or a row of -inf throughout, makes every score of the row NaN: no score compares greater than any other.
    The rule of gpt.hip's header comment: such a row returns token 0 (as vq_argmin_kernel does, and torch.argmax on an all-NaN row),
    sample_topn returns 0, 1, ..., n - 1 -- never an index outside [0, V) --, and the finite rows of the same launch keep the bits
    they have in a launch of their own."""
    V, T, n = 300, 0.9, 3
    lg, bad, fine = _bad_rows(V, torch.Generator().manual_seed(9))
    assert torch.argmax(torch.full((4,), NAN)) == 0
    dev = lg.cuda()
    noise = R.case_noise(V, rows=10).cuda()
    k0, k1, row0, step, call = R.PHILOX_WORDS
    for name, kw in (("greedy", {}), ("host noise", dict(noise=noise)), ("philox", dict(philox=R.PHILOX_WORDS))):
        got = ops.sample_topk(dev, top_k, T, **kw).cpu()
        assert ((got >= 0) & (got < V)).all(), f"{name}: index outside [0, {V}): {got.tolist()}"
        assert (got[bad] == 0).all(), f"{name}: {got.tolist()}"
        for b in fine:
            alone = dict(kw)
            if "noise" in kw:
                alone["noise"] = noise[b:b + 1].contiguous()
            if "philox" in kw:
                alone["philox"] = (k0, k1, row0 + b, step, call)
            assert torch.equal(ops.sample_topk(dev[b:b + 1], top_k, T, **alone).cpu(), got[b:b + 1]), f"{name}: finite row {b} changed"
        if name == "philox":
            continue
        idx, logp = ops.sample_topn(dev, top_k, T, n, **kw)
        idx, logp = idx.cpu(), logp.cpu()
        assert ((idx >= 0) & (idx < V)).all(), f"top-n {name}: index outside [0, {V})"
        assert torch.equal(idx[bad], torch.arange(n).expand(len(bad), n)), f"top-n {name}: {idx[bad].tolist()}"
        fi, fl = ops.sample_topn(dev[fine].contiguous(), top_k, T, n, **({"noise": noise[fine].contiguous()} if "noise" in kw else {}))
        assert torch.equal(fi.cpu(), idx[fine]) and torch.equal(fl.cpu(), logp[fine]), f"top-n {name}: finite rows changed"
        assert all(len(set(r)) == n for r in idx.tolist())
    # a NaN with the sign bit set sorts below every number: under a top-k mask it is dropped like a small logit; in range either way
    neg = lg[fine].clone()
    neg[:, 11] = torch.tensor([0xffc00000 - 2**32], dtype=torch.int32).view(torch.float32)
    got = ops.sample_topk(neg.cuda(), top_k, T, noise=noise[:3].contiguous()).cpu()
    idx, _ = ops.sample_topn(neg.cuda(), top_k, T, V, noise=noise[:3].contiguous())
    assert ((got >= 0) & (got < V)).all() and torch.equal(idx.cpu().sort(1)[0], torch.arange(V).expand(3, V))
    # n = V on rows without a winner: every index once, in order
    idx, _ = ops.sample_topn(dev[bad].contiguous(), top_k, T, V)
    assert torch.equal(idx.cpu(), torch.arange(V).expand(len(bad), V))


# ------------------------------------------------------------------ the pick inside the decode step

T0, N_NEW, VOCAB, TOP_K = 4, 12, 200, 20
KEYS = [(0x1234567 + 977 * g, 0xabcdef01 ^ (g << 7)) for g in range(3)]
ROW_OFFSETS = [32, 1000, 0xffffffff]      # the second row of the last group wraps to global row 0


def _gpt():
    from ccvs_amd.models.skip_vid_generator.models import mingpt
    torch.manual_seed(5)
    net = mingpt.GPT(vocab_size=VOCAB, block_size=512, num_blocks=32, n_layer=1, n_head=2, n_embd=32, emb_mode="temporal", shape=(4, 4)).cuda()
    for p in net.parameters():
        p.data.add_(0.3 * torch.randn_like(p))
    return net


def _generate(net, codes, keys, offsets, call, form):
    """-> (tokens [B, T0 + N_NEW] on the host, {widx, len, state} after the call)."""
    net.drop_engine_state()
    net.persistent_step = form == "persistent"
    if len(keys) > 1:
        net.noise_key, net.row_offset = list(keys), list(offsets)
    else:
        net.noise_key, net.row_offset = keys[0], offsets[0]
    net.noise_call = call
    out = net.generate(codes, N_NEW, sample=True, top_k=TOP_K, noise="device", use_graph=form != "eager")
    net.check_steps()
    torch.cuda.synchronize()
    c = net._cache
    after = {"widx": c["widx"].cpu(), "len": c["len_dev"].cpu(), "state": c["state"].cpu().view(-1, 8)}
    assert net.noise_call == call + 1
    net.noise_key, net.row_offset, net.persistent_step = None, 0, False
    return out.cpu(), after


def _teacher_forced_logits(net, tokens):
    """The logits in front of every pick: prefill + step() of the per-op engine on the generated tokens.  [N_NEW, B, V] float32."""
    net.drop_engine_state()
    dev = tokens.cuda()
    net.begin(dev.shape[0], T0 + N_NEW)
    logits = [net.prefill(dev[:, :T0].contiguous()).cpu()]
    for i in range(1, N_NEW):
        logits.append(net.step(dev[:, T0 + i - 1:T0 + i]).cpu())
    return torch.stack(logits)


@pytest.mark.parametrize("form", ["graph", "eager", "persistent"])
@pytest.mark.parametrize("groups,call", [(1, 0), (3, 0), (3, 5), (1, 5)])
def test_decode_step_picks_against_the_mirror(ops, groups, call, form):
    net = _gpt()
    B, per = 6, 6 // groups
    codes = torch.randint(0, VOCAB, (B, T0), generator=torch.Generator().manual_seed(1)).cuda()
    keys, offsets = KEYS[:groups], ROW_OFFSETS[:groups]
    tokens, after = _generate(net, codes, keys, offsets, call, form)
    assert torch.equal(tokens[:, :T0], codes.cpu()) and ((tokens >= 0) & (tokens < VOCAB)).all()
    logits = _teacher_forced_logits(net, tokens)
    worst, n_mo = 0.0, 0
    for i in range(N_NEW):
        step = 0xffffffff if i == 0 else i - 1
        xs, mask = R.kept(logits[i], 1.0, TOP_K)
        noise = np.stack([R.exp1_noise(VOCAB, offsets[b // per] + b % per, step, call, *keys[b // per]) for b in range(B)])
        s, d = R.scores64(xs, mask, noise)
        f, m = _judge(f"decode {form} groups={groups} call={call} token {i}", tokens[:, T0 + i], s, d, R.C_PHILOX, mask, cap_rows=B * N_NEW)
        worst, n_mo = max(worst, f), n_mo + m
    assert n_mo <= R.MARGIN_ONLY_CAP * B * N_NEW
    # the device-resident counters: each advanced once per step, the ticket word back at 0, the Philox words in place
    assert after["widx"].tolist() == [T0 + N_NEW] * groups and after["len"].tolist() == [T0 + N_NEW - 1] * groups
    st = after["state"].to(torch.int64) & 0xffffffff
    for g in range(groups):
        assert st[g, [0, 2, 3, 4, 5, 6]].tolist() == [N_NEW - 1, 0, call, keys[g][0], keys[g][1], offsets[g]], (g, st[g].tolist())


def test_decode_step_tokens_do_not_depend_on_the_batch_slot(ops):
    """Rows 2..3 of a six-row batch, generated alone under the words they have there (one group: row_offset + 2; three groups of two:
    the middle group's own key and offset), give the same tokens."""
    net = _gpt()
    codes = torch.randint(0, VOCAB, (6, T0), generator=torch.Generator().manual_seed(1)).cuda()
    whole, _ = _generate(net, codes, KEYS[:1], [32], 0, "graph")
    alone, _ = _generate(net, codes[2:4].contiguous(), KEYS[:1], [34], 0, "graph")
    assert torch.equal(whole[2:4], alone), "one group: rows 2..3 alone draw other tokens"
    assert not torch.equal(whole[0:2, T0:], alone[:, T0:])
    stacked, _ = _generate(net, codes, KEYS, ROW_OFFSETS, 0, "graph")
    for g in range(3):
        alone, _ = _generate(net, codes[2 * g:2 * g + 2].contiguous(), KEYS[g:g + 1], ROW_OFFSETS[g:g + 1], 0, "eager")
        assert torch.equal(stacked[2 * g:2 * g + 2], alone), f"three groups: group {g} alone draws other tokens"


def test_pick_argument_errors(ops):
    """temperature <= 0, n > V, n < 1, a null `out`: each raises with the launcher's message, and nothing is written."""
    from ccvs_amd import lib
    L = lib.load()
    p, st = ops._p, ops._stream
    V = 40
    lg = torch.zeros(2, V, device="cuda")
    out = torch.full((2,), POISON, dtype=torch.int64, device="cuda")
    idx = torch.full((2, V + 1), POISON, dtype=torch.int64, device="cuda")
    logp = torch.full((2, V + 1), -1.0, device="cuda")
    for T in (0.0, -1.0, NAN):
        with pytest.raises(lib.CcvsError, match="ccvs_sample_topk: bad arguments"):
            ops.sample_topk(lg, 7, T, out=out)
        with pytest.raises(lib.CcvsError, match="ccvs_sample_topk_philox: bad arguments"):
            ops.sample_topk(lg, 7, T, out=out, philox=R.PHILOX_WORDS)
        with pytest.raises(lib.CcvsError, match="ccvs_sample_topn: bad arguments"):
            lib.check(L.ccvs_sample_topn(p(lg), V, p(None), p(idx), p(logp), 2, V, 7, T, 2, st()), "ccvs_sample_topn")
    for n in (V + 1, 0, -3):
        with pytest.raises(lib.CcvsError, match="ccvs_sample_topn: bad arguments"):
            lib.check(L.ccvs_sample_topn(p(lg), V, p(None), p(idx), p(logp), 2, V, 7, 1.0, n, st()), "ccvs_sample_topn")
    with pytest.raises(lib.CcvsError, match="ccvs_sample_topk: null pointer"):
        lib.check(L.ccvs_sample_topk(p(lg), V, p(None), p(None), 1, 2, V, 7, 1.0, st()), "ccvs_sample_topk")
    with pytest.raises(lib.CcvsError, match="ccvs_sample_topk_philox: null pointer"):
        lib.check(L.ccvs_sample_topk_philox(p(lg), V, p(None), 1, 2, V, 7, 1.0, 1, 2, 3, 4, 5, st()), "ccvs_sample_topk_philox")
    with pytest.raises(lib.CcvsError, match="ccvs_sample_topn: null pointer"):
        lib.check(L.ccvs_sample_topn(p(lg), V, p(None), p(None), p(logp), 2, V, 7, 1.0, 2, st()), "ccvs_sample_topn")
    torch.cuda.synchronize()
    assert (out == POISON).all() and (idx == POISON).all() and (logp == -1.0).all()

"""Host reference of the token pick (gpt.hip: sample_topk_row, sample_topn_kernel): numpy and torch only, no GPU.

What the kernels compute (get_icode, transformer_model.py:395-409): xs = logit / temperature in fp32, the top-k mask (every value
equal to the k-th largest kept, -0.0 == +0.0), softmax, then argmax(p) (greedy) or argmax(p / Exp(1) noise) (== torch.multinomial);
the noise is given by the host or drawn in the kernel from Philox4x32-10.

philox4x32_10    the generator (Salmon et al., SC'11; known answers of Random123 in tests/test_pick_host.py).
exp1_noise       the kernel's draw, step by step: counter (element j, row, step, call), key (k0, k1), output word 0,
                 u = (float32(word) + 0.5f) * 2^-32 in fp32 -- the conversion and the addition round as the device's do, the
                 multiplication is exact --, noise = max(-log(float64(u)), float32(1e-30)).
kept             the top-k set as the reference defines it, decided on the fp32 values xs exactly.
scores64         exp(float64(xs) - max) on the kept set, divided by the noise; the row total is a common factor and is left out.
accept           a pick i is right iff kept[i] and s64[i] >= s64[best] * (1 - m), m = (|d_i| + |d_best| + c) * 2^-24, d = xs - max
                 in float64: |d| * 2^-24 is the rounding of the fp32 subtraction carried through exp (d exp(d) / exp(d) = d);
                 c counts, for the two entries compared, expf's error, the two divisions (by the total and by the noise: half
                 an ulp each) and, where the kernel draws the noise, logf's error: c = 2 * (E + 1) for greedy picks and host
                 noise, 2 * (E + 1 + L) for Philox noise.  Among entries of EQUAL float64 score the lowest index is the only
                 right answer (the kernel's tie rule, torch.argmax's).
topn_accept      the same rule for n rounds, each against the best of what the earlier rounds left, and log p against float64
                 log(e_i / sum e) within (|d_i| + c + V / 256 + 9) * 2^-24: V / 256 + 9 counts the additions of the kernel's
                 per-thread (V / 256), butterfly (6) and four-wave (3) sum.

E and L, the errors of the device's expf and logf in ulp: the ROCm installation this was written against ships no table of HIP
device-math accuracy (no document under its share/ or include/ trees states ulp figures), so both are taken as 2 ulp.

`CASES` / `case_logits` / `case_noise` are the inputs of tests/test_pick_gpu.py; tests/test_pick_host.py runs an fp32 emulation of
the kernel over the same table, so that the margin is known to accept a correct fp32 pick and to be narrower than the gaps between
the scores of these inputs (at most 2 % of a case's rows may have an fp32-plausible pick other than the float64 argmax)."""
import numpy as np
import torch

EXPF_ULP = 2.0
LOGF_ULP = 2.0
C_HOST = 2 * (EXPF_ULP + 1.0)                # greedy and host noise
C_PHILOX = 2 * (EXPF_ULP + 1.0 + LOGF_ULP)   # noise drawn in the kernel
EPS = 2.0 ** -24
NOISE_FLOOR = float(np.float32(1e-30))
MARGIN_ONLY_CAP = 0.02

_M32 = np.uint64(0xffffffff)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of counter (c0, c1, c2, c3), key (k0, k1) -> the four output words, uint64 arrays holding 32-bit values
    (vectorised over whatever the arguments broadcast to)."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.asarray(a, dtype=np.uint64) & _M32 for a in (c0, c1, c2, c3, k0, k1)])
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2              # 32 x 32 -> 64 bits: no overflow
        hi0, lo0 = p0 >> _S32, p0 & _M32
        hi1, lo1 = p1 >> _S32, p1 & _M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + w0) & _M32, (k1 + w1) & _M32
    return c0, c1, c2, c3


def uniform_f32(words):
    """u = (float32(word) + 0.5f) * 2^-32 as the device forms it: uint32 -> fp32 rounds to nearest even (here: exact in float64,
    then one rounding), the fp32 addition rounds again (it is absorbed from 2^24 on), the multiplication is exact.  (0, 1]."""
    f = np.asarray(words, dtype=np.uint64).astype(np.float64).astype(np.float32)
    return (f + np.float32(0.5)) * np.float32(2.0 ** -32)


def exp1_noise(V, row, step, call, k0, k1):
    """float64 [V]: the Exp(1) draw of every element of global row `row` (taken mod 2^32) at (step, call) under key (k0, k1)."""
    w = philox4x32_10(np.arange(V, dtype=np.uint64), int(row) & 0xffffffff, int(step) & 0xffffffff, int(call) & 0xffffffff,
                      int(k0) & 0xffffffff, int(k1) & 0xffffffff)[0]
    return np.maximum(-np.log(uniform_f32(w).astype(np.float64)), NOISE_FLOOR)


def philox_noise(B, V, words):
    """float64 [B, V]: the draws of a `sample_topk(philox=words)` launch, words = (key0, key1, row0, step, call)."""
    k0, k1, row0, step, call = (int(w) & 0xffffffff for w in words)
    rows = (np.uint64(row0) + np.arange(B, dtype=np.uint64)) & _M32          # row0 + b wraps at 2^32
    w = philox4x32_10(np.arange(V, dtype=np.uint64)[None], rows[:, None], step, call, k0, k1)[0]
    return np.maximum(-np.log(uniform_f32(w).astype(np.float64)), NOISE_FLOOR)


def scaled(logits, temperature):
    """xs = float32(logit) / float32(temperature), numpy fp32 [B, V]."""
    lg = logits.detach().cpu().numpy() if isinstance(logits, torch.Tensor) else np.asarray(logits)
    with np.errstate(all="ignore"):
        return (lg.astype(np.float32) / np.float32(temperature)).astype(np.float32)


def kept(logits, temperature, top_k):
    """(xs fp32 [B, V], mask bool [B, V]): xs >= the k-th largest of its row by float comparison -- ties kept, -0.0 == +0.0 --,
    everything when top_k is None, <= 0 or >= V."""
    xs = scaled(logits, temperature)
    V = xs.shape[1]
    if top_k is None or top_k <= 0 or top_k >= V:
        return xs, np.ones(xs.shape, dtype=bool)
    kth = np.sort(xs, axis=1)[:, V - top_k][:, None]
    return xs, xs >= kth


def scores64(xs, mask, noise64=None):
    """(s64, d64) [B, V]: d = float64(xs) - row maximum; s = exp(d) on the kept set and 0 elsewhere, divided by the noise."""
    x = xs.astype(np.float64)
    with np.errstate(all="ignore"):
        d = x - x.max(axis=1, keepdims=True)
        s = np.where(mask, np.exp(d), 0.0)
        if noise64 is not None:
            s = s / np.asarray(noise64, dtype=np.float64)
    return s, d


def _judge(pick, s, d, c):
    """Rows of one round.  -> (ok, figure, margin_only): figure = (1 - s[pick] / s[best]) / m."""
    B = s.shape[0]
    rows = np.arange(B)
    pick = np.asarray(pick).astype(np.int64)
    inside = (pick >= 0) & (pick < s.shape[1])
    pi = np.where(inside, pick, 0)
    best = s.argmax(axis=1)                      # the lowest index among equal scores
    sb, si = s[rows, best], s[rows, pi]
    di, db = np.abs(d[rows, pi]), np.abs(d[rows, best])
    with np.errstate(all="ignore"):
        m = np.where(np.isfinite(di) & np.isfinite(db), (di + db + c) * EPS, 0.0)     # a -inf logit has score 0 exactly: no margin
        ok = inside & (si >= sb * (1.0 - m)) & ((si != sb) | (pi == best))
        ok &= (si > 0) | (sb <= 0)                                   # a masked entry only where nothing else is left
        figure = np.where(sb > 0, (1.0 - si / np.where(sb > 0, sb, 1.0)) / np.where(m > 0, m, 1.0), 0.0)
    figure = np.where(pi == best, 0.0, figure)
    return ok, figure, inside & (pi != best)


def accept(pick, s64, d64, c, mask=None):
    """bool [B]: the pick of every row is right (module docstring).  `mask`: the kept set, where the caller wants membership
    asserted on its own (a kept entry is the only kind with a positive score)."""
    ok = _judge(pick, s64, d64, c)[0]
    if mask is not None:
        p = np.clip(np.asarray(pick).astype(np.int64), 0, s64.shape[1] - 1)
        ok = ok & mask[np.arange(s64.shape[0]), p]
    return ok


def figure(pick, s64, d64, c):
    """float [B]: (1 - s64[pick] / s64[best]) / m, the share of the margin a pick uses (0 where pick == argmax)."""
    return _judge(pick, s64, d64, c)[1]


def margin_only(pick, s64, d64, c):
    """bool [B]: rows whose pick is not argmax(s64) (right only by the margin, if accepted)."""
    return _judge(pick, s64, d64, c)[2]


def topn_accept(idx, logp, xs, mask, noise64, c):
    """n picks per row, best first.  -> (ok [B, n], figure [B, n], margin_only [B, n], logp_err / bound [B, n]).
    Round r is judged against the scores the earlier rounds left; once the kept set is used up every score left is 0 and the
    lowest index left is the answer.  log p of a masked entry is -inf on both sides."""
    idx = np.asarray(idx).astype(np.int64)
    logp = np.asarray(logp).astype(np.float64)
    B, n = idx.shape
    V = xs.shape[1]
    rows = np.arange(B)
    s, d = scores64(xs, mask, noise64)
    e = scores64(xs, mask, None)[0]
    with np.errstate(all="ignore"):
        want_logp = np.log(e / e.sum(axis=1, keepdims=True))
    s = s.copy()
    ok, fig, mo, lerr = (np.zeros((B, n), dtype=t) for t in (bool, np.float64, bool, np.float64))
    for r in range(n):
        ok[:, r], fig[:, r], mo[:, r] = _judge(idx[:, r], s, d, c)
        p = np.clip(idx[:, r], 0, V - 1)
        w, g = want_logp[rows, p], logp[:, r]
        bound = (np.abs(np.where(np.isfinite(d[rows, p]), d[rows, p], 0.0)) + c + V / 256.0 + 9.0) * EPS
        with np.errstate(all="ignore"):
            lerr[:, r] = np.where(np.isfinite(w), np.abs(g - w) / bound, np.where(g == w, 0.0, np.inf))
        s[rows, p] = -1.0                         # taken
    return ok, fig, mo, lerr


# ------------------------------------------------------------------ the inputs of tests/test_pick_gpu.py

V_PICK_MAX = 160 * 1024 // 4 - (16 + 256)        # ccvs_sample_topk: PICK_SMEM_WORDS(V) * 4 <= 160 KB
V_TOPN_MAX = (160 * 1024 // 4 - (16 + 256)) // 2   # ccvs_sample_topn: (2 V + 16 + 256) * 4 <= 160 KB
TEMPERATURES = (0.7, 1.0, 1.3)
PICK_VOCABS = (1, 5, 255, 256, 257, 1000, 16384, V_PICK_MAX)
TOPN_VOCABS = (5, 257, 1000, 16384, V_TOPN_MAX)
ROWS = 64
TOPN_ROWS = 32
PHILOX_WORDS = (0x01234567, 0xabcdef01, 32, 3, 2)   # key0, key1, row0, step, call: all different, so a swap shows
# the host margin self-check of the issue: randn * 2 logits, 512 rows each
SELF_CHECK = ((200, 7, 0.7), (1000, 50, 1.0), (16384, 100, 0.9), (5, 3, 1.3))


def top_ks(V):
    """top_k in {None, 1, 7, V - 1, V, V + 5}, where it is a count."""
    out = []
    for k in (None, 1, 7, V - 1, V, V + 5):
        if (k is None or k >= 1) and k not in out:
            out.append(k)
    return out


CASES = [(V, k, TEMPERATURES[i % 3]) for V in PICK_VOCABS for i, k in enumerate(top_ks(V))] + \
        [(V, 7, T) for V in (5, 257, 1000) for T in TEMPERATURES]
TOPN_CASES = [(V, k, TEMPERATURES[(i + 1) % 3]) for V in TOPN_VOCABS for i, k in enumerate((None, 7, V - 1))]


def case_logits(V, top_k, rows=ROWS):
    """fp32 [rows, V] of one case: randn * 2; then rows quantised to halves (exact ties everywhere, at the k-th value too);
    rows tied at the k-th value as `_tied_rows` of tests/test_ops_gpu.py builds them (k - 1 values above, the k-th value and 1, 2,
    V // 4 more equal to it, the rest below); one constant row; rows with a third of the entries -inf; one row with a single
    finite entry."""
    g = torch.Generator().manual_seed(7919 * V + (0 if top_k is None else top_k))
    lg = torch.randn(rows, V, generator=g) * 2
    q0, t0, c0, i0 = rows - 16, rows - 8, rows - 5, rows - 4
    lg[q0:t0] = torch.round(lg[q0:t0] * 2) / 2
    k = min(7 if top_k is None else top_k, V)
    for r, ties in zip(range(t0, c0), (1, 2, V // 4)):
        row = torch.rand(V, generator=g) * 2 - 3
        order = torch.randperm(V, generator=g)
        if k > 1:
            row[order[:k - 1]] = torch.linspace(2.0, 0.5, k - 1)
        row[order[k - 1:k + min(ties, V - k)]] = 0.25
        lg[r] = row
    lg[c0] = 0.75
    for r in range(i0, rows - 1):
        lg[r, torch.randperm(V, generator=g)[:V // 3]] = float("-inf")
    lg[rows - 1] = float("-inf")
    lg[rows - 1, int(torch.randint(0, V, (1,), generator=g))] = 0.5
    return lg


def case_noise(V, rows=ROWS):
    """fp32 Exp(1) noise [rows, V] from torch's generator (what torch.multinomial consumes)."""
    return torch.empty(rows, V).exponential_(1, generator=torch.Generator().manual_seed(104729 + V))


def emulate_fp32(xs, mask, noise32=None):
    """The kernel's arithmetic in torch fp32 on a CPU: exp(xs - max), sum, the divisions, argmax (first of equal scores)."""
    x = torch.from_numpy(xs)
    e = torch.where(torch.from_numpy(mask), torch.exp(x - x.max(dim=1, keepdim=True)[0]), torch.zeros(()))
    p = e / e.sum(dim=1, keepdim=True)
    if noise32 is not None:
        p = p / noise32
    best = p.max(dim=1, keepdim=True)[0]
    return (p == best).int().argmax(dim=1).numpy()    # the lowest index of the maximum

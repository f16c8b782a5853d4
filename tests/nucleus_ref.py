"""Host reference of nucleus (top-p) sampling in the token pick (gpt.hip: sample_topk_row's TOPP form; include/ccvs_hip_sampling.h):
numpy only, no GPU.  Builds on tests/pick_ref.py: the scaled logits, the top-k set, the scores, the noise mirror and the acceptance
rule of a pick are that module's.

The definition.  Per row, on the fp32 values xs = logit / temperature and the top-k set K of `pick_ref.kept`:
    E_j = exp(float64(xs_j) - max) on K,  T = sum E,  G_j = (sum of E_i over i in K with xs_i > xs_j, by float comparison) / T;
entry j is in the nucleus iff j in K and G_j < p, p = float64(float32(top_p)) -- the ABI carries top_p as a float, the definition
applies to that float.  Entries of equal xs share one G (-0.0 == +0.0).  G does not increase along the descending order of xs, so
the nucleus is a prefix of that order.

`nucleus(xs, mask_topk, p)` decides on xs exactly, with masses in float64, and returns three masks: certainly in (G_j < p - m_j),
certainly out (not in K, or G_j > p + m_j) and UNCERTAIN (|G_j - p| <= m_j).  The margin m_j is derived from the kernel's own
arithmetic, not from its results:

  the kernel's mass of entry i is q_i = floor(e_i * 2^46) / 2^46 with e_i = expf(fl32(xs_i - max)).
    * the fp32 subtraction: fl32(d_i) = d_i (1 + eps), |eps| <= 2^-24, d_i = xs_i - max; carried through exp that is a relative error
      of |d_i| * 2^-24 (d exp(d) / exp(d) = d);
    * expf: `pick_ref.EXPF_ULP` ulp of the result; one ulp of an fp32 value is at most 2^-23 of it: 2 * EXPF_ULP * 2^-24;
    so e_i = E_i (1 + delta_i), |delta_i| <= w_i = (|d_i| + 2 * EXPF_ULP) * 2^-24 (the max itself is an fp32 value: exact);
    * the accumulation: the scaling by 2^46 is exact, the truncation loses less than 2^-46 per entry, the integer sums nothing.
  With A_j = sum of E_i above j (n_j entries), A'_j and T' the kernel's sums, |K| = the size of the top-k set:
    |A'_j - A_j| <= a_j = sum_{above j} E_i w_i + n_j 2^-46,      |T' - T| <= t = sum_K E_i w_i + |K| 2^-46,
    A'/T' - A/T = ((A' - A) T - A (T' - T)) / (T T'),  so  |G'_j - G_j| <= (a_j + G_j t) / T * (T / T'),  and T / T' <= 1 + 2^-16
    (t / T is of the order 2^-20).
    * the decision G' < p is made as A' 2^46 < ceil(fl64(p * fl64(T' 2^46))): the conversion of T' 2^46 < 2^62 to double and the
      product round by 2^-53 each, the ceiling moves the right-hand side by less than one unit, 2^-46; divided by T' >= 1 that is
      at most p * 2^-52 + 2^-46 on G'.
  m_j = ((a_j + G_j t) / T) * (1 + 2^-16) + p * 2^-52 + 2^-46.
  (The reference's own float64 sums are off by about |K| * 2^-53 of T: below the 2^-46 terms, which are counted per entry.)

A pick is right (`accept`) iff there is a threshold inside the uncertain band for which `pick_ref.accept` accepts it on the set
{certainly in} + {uncertain, xs >= threshold}: the kernel's set is a prefix of the descending order, so these few sets -- the
certain nucleus alone, and one more per distinct uncertain value -- are all it can be.

`CASES` / `case_logits` are the inputs of tests/test_nucleus_gpu.py; tests/test_nucleus_host.py runs an fp32 emulation of the kernel
(`emulate_fp32`) over the same table and checks that at most `pick_ref.MARGIN_ONLY_CAP` of a case's rows have an uncertain entry at
all.  That share decides which p goes with which vocabulary: a band of about 10^-6 around p is hit by some G_j in most rows once
single entries near the boundary carry less than that, i.e. at p = 0.9 and 0.999 on the whole of a large vocabulary; there the
large p go with top_k = 7 and the whole vocabulary gets the small ones."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pick_ref as R  # noqa: E402

MASS_BITS = 46                                   # gpt.hip: TOPP_MASS_SCALE = 2^46
QUANT = 2.0 ** -MASS_BITS
W_EXPF = 2.0 * R.EXPF_ULP                        # expf's error in units of 2^-24
TOPP_EXTRA_WORDS = 2 * 262                       # 64-bit words behind the top-k form's block: 256 mass bins, 4 wave totals, 2 of the selected bin
V_TOPP_MAX = max(v for v in range(1, 160 * 1024 // 4) if ((v + 16 + 256 + 1) & ~1) + TOPP_EXTRA_WORDS <= 160 * 1024 // 4)   # PICK_TOPP_SMEM_WORDS(V) * 4 <= 160 KB
TOP_PS = (0.1, 0.5, 0.9, 0.999)
VOCABS = tuple(V_TOPP_MAX if v == R.V_PICK_MAX else v for v in R.PICK_VOCABS)
ROWS = R.ROWS


def p_of(top_p):
    """float64(float32(top_p)): the threshold the definition applies to."""
    return float(np.float32(top_p))


def masses(xs, mask_topk):
    """-> (E, d, G, m) float64 [B, V]: E = exp(d) on the top-k set (0 elsewhere), d = xs - row maximum, G as defined, m = the margin
    without its p * 2^-52 term.  Outside the top-k set G = inf."""
    x = xs.astype(np.float64)
    B, V = x.shape
    with np.errstate(all="ignore"):
        d = x - x.max(axis=1, keepdims=True)
        E = np.where(mask_topk, np.exp(d), 0.0)
        w = np.where(E > 0, (np.abs(d) + W_EXPF) * R.EPS, 0.0)      # a -inf logit has mass 0 exactly
    G = np.full((B, V), np.inf)
    m = np.zeros((B, V))
    for b in range(B):
        idx = np.nonzero(mask_topk[b])[0]
        order = idx[np.argsort(-x[b, idx], kind="stable")]
        xv, Ev, Wv = x[b, order], E[b, order], E[b, order] * w[b, order]
        first = np.searchsorted(-xv, -xv, side="left")                # the first entry of each run of equal values (-0.0 == +0.0)
        cE = np.concatenate(([0.0], np.cumsum(Ev)))
        cW = np.concatenate(([0.0], np.cumsum(Wv)))
        T = cE[-1]
        g = cE[first] / T
        a = cW[first] + first * QUANT
        t = cW[-1] + len(order) * QUANT
        G[b, order] = g
        m[b, order] = (a + g * t) / T * (1.0 + 2.0 ** -16) + QUANT
    return E, d, G, m


def nucleus(xs, mask_topk, p):
    """-> (certainly in, certainly out, uncertain) bool [B, V] for threshold p (module docstring)."""
    p = p_of(p)
    _, _, G, m = masses(xs, mask_topk)
    m = m + p * 2.0 ** -52
    with np.errstate(all="ignore"):
        sure_in = mask_topk & (G < p - m)
        sure_out = ~mask_topk | (G > p + m)
    return sure_in, sure_out, ~sure_in & ~sure_out


def candidates(xs, sure_in, uncertain, b):
    """The sets row b's nucleus can be: the certain nucleus, and one more per distinct uncertain value (descending)."""
    sets = [sure_in[b]]
    for t in np.unique(xs[b][uncertain[b]])[::-1]:
        sets.append(sure_in[b] | (uncertain[b] & (xs[b] >= t)))
    return sets


def accept(pick, xs, mask_topk, p, noise64, c):
    """bool [B]: every row's pick is right for SOME nucleus inside the uncertain band (module docstring)."""
    pick = np.asarray(pick).astype(np.int64)
    sure_in, _, unc = nucleus(xs, mask_topk, p)
    s, d = R.scores64(xs, sure_in, noise64)
    ok = R.accept(pick, s, d, c, sure_in)
    for b in np.nonzero(unc.any(axis=1))[0]:
        for kept in candidates(xs, sure_in, unc, b)[1:]:
            if ok[b]:
                break
            nz = None if noise64 is None else np.asarray(noise64)[b:b + 1]
            sb, db = R.scores64(xs[b:b + 1], kept[None], nz)
            ok[b] = R.accept(pick[b:b + 1], sb, db, c, kept[None])[0]
    return ok


def transformers_rule(xs, mask_topk, p):
    """The `transformers` TopPLogitsWarper restated (sort ascending, cumulative softmax, remove where cumsum <= 1 - p, keep the last),
    after top-k, in float64: bool [B, V].  For inputs WITHOUT ties (a sort has no rule for them)."""
    p = p_of(p)
    x = np.where(mask_topk, xs.astype(np.float64), -np.inf)
    order = np.argsort(x, axis=1, kind="stable")                       # ascending
    xs_sorted = np.take_along_axis(x, order, axis=1)
    prob = np.exp(xs_sorted - xs_sorted[:, -1:])
    prob /= prob.sum(axis=1, keepdims=True)
    remove = np.cumsum(prob, axis=1) <= 1.0 - p
    remove[:, -1] = False
    out = np.zeros(x.shape, dtype=bool)
    np.put_along_axis(out, order, ~remove, axis=1)
    return out & mask_topk


def emulate_fp32(xs, mask_topk, p, noise32=None):
    """The kernel's arithmetic on a CPU: e = exp(xs - max) in torch fp32, integer masses floor(e 2^46), the set {G_int < ceil(p T_int)},
    then the pick on it -- e / (the fp32 total of the top-k set) / noise, the first of equal scores.  -> (picks [B], set bool [B, V])."""
    x = torch.from_numpy(xs)
    e = torch.where(torch.from_numpy(mask_topk), torch.exp(x - x.max(dim=1, keepdim=True)[0]), torch.zeros(()))
    q = np.floor(e.numpy().astype(np.float64) * 2.0 ** MASS_BITS).astype(np.uint64)
    B, V = xs.shape
    keep = np.zeros((B, V), dtype=bool)
    for b in range(B):
        idx = np.nonzero(mask_topk[b])[0]
        order = idx[np.argsort(-xs[b, idx].astype(np.float64), kind="stable")]
        xv = xs[b, order].astype(np.float64)
        first = np.searchsorted(-xv, -xv, side="left")
        cq = np.concatenate((np.zeros(1, dtype=np.uint64), np.cumsum(q[b, order], dtype=np.uint64)))   # < 2^62: exact
        P = int(np.ceil(p_of(p) * float(int(cq[-1]))))
        keep[b, order] = cq[first] < np.uint64(P)
    s = torch.where(torch.from_numpy(keep), e, torch.zeros(())) / e.sum(dim=1, keepdim=True)
    if noise32 is not None:
        s = s / noise32
    best = s.max(dim=1, keepdim=True)[0]
    return (s == best).int().argmax(dim=1).numpy(), keep


# ------------------------------------------------------------------ the inputs of tests/test_nucleus_gpu.py

def two_level_row(V, n, a, g):
    """n entries at a (at random places), the rest at a - 1."""
    row = torch.full((V,), a - 1.0)
    row[torch.randperm(V, generator=g)[:n]] = a
    return row


def case_logits(V, top_k, rows=ROWS):
    """fp32 [rows, V]: `pick_ref.case_logits` (random, quantised with exact ties, tied at the k-th value, constant, with -inf) with
    its first rows replaced by the two kinds the nucleus adds: two-level rows (1, 2, V // 3 and V - 1 entries at 0.5, the rest at
    -0.5) and two more constant rows."""
    lg = R.case_logits(V, top_k, rows)
    g = torch.Generator().manual_seed(15485863 + V)
    for r, n in enumerate((1, 2, V // 3, V - 1)):
        lg[r] = two_level_row(V, min(max(n, 1), V), 0.5, g)
    lg[4] = -3.25
    lg[5] = 0.0
    return lg


def _cases():
    """(V, top_k, temperature, p).  Each vocabulary with top_k in {None, 7, V - 1}; p over {0.1, 0.5, 0.9, 0.999} in turn up to
    V = 1000; from 16384 on the whole vocabulary (top_k None, V - 1) takes p = 0.1 and 0.5 and top_k = 7 the large ones (module
    docstring: the share of rows with an uncertain entry)."""
    out, i = [], 0
    for V in VOCABS:
        for k in (None, 7, V - 1):
            if k is not None and k < 1:                 # (V = 1; top_k = 7 >= V keeps everything, as None does)
                continue
            if V >= 16384:
                ps = (0.9, 0.999) if k == 7 else ((0.1,) if k is None else (0.5,))
            else:
                ps = (TOP_PS[i % 4], TOP_PS[(i + 2) % 4])
            for p in ps:
                out.append((V, k, R.TEMPERATURES[i % 3], p))
                i += 1
    return out


CASES = _cases()

"""Float64 reference of the KV-cached causal attention (`ccvs_attention`, attention.hip) with a derived per-element error bound, the
wrong references that the bound has to tell from the right one, and the score patterns shared by the host and the GPU tests.
Plain torch, runs anywhere.

The operation (mingpt.py:67-77 over a cache): query t of `q [B,H,Tq,D]` sits at position pos0 + t and sees keys 0 .. pos0 + t of
`k, v [B,H,L,D]`:

    s      = q k^T / sqrt(D), masked          p = softmax(s)          out = p @ v

The bound, from float64 magnitudes only, eps = 2**-24 (unit roundoff of fp32):

    A      = p @ |v|
    smag_t = max over visible j of  (|q| |k|^T)_tj / sqrt(D)
    R_t    = sum_j p_tj * (max_j s_tj - s_tj)          L_t = number of visible keys
    tol    = (2 (D + 4) eps smag_t  +  eps (L_t + 2 R_t + 16)) * A  + 1e-12

  * One fp32 score is a sum of D products plus the roundings of the scale (and of the log2(e) factor that the prefill form folds
    into q): |ds_tj| <= (D + 4) eps (|q| |k|^T)_tj / sqrt(D) <= (D + 4) eps smag_t, whatever the order of the sum.
  * With exact exponentials, p~_j = p_j e^{ds_j} / sum_i p_i e^{ds_i}: the error enters through the numerator and through the
    normaliser, so |p~_j - p_j| <= 2 max|ds| p_j to first order, and |sum_j (p~_j - p_j) v_j| <= 2 (D + 4) eps smag_t A.
  * The exponent's argument s_j - max is rounded once (relative eps, absolute eps (max - s_j)) and so perturbs p_j by the factor
    e^{eps (max - s_j)}: through numerator and normaliser again, 2 eps sum_j p_j (max - s_j) A = 2 R_t eps A.  (The online
    softmax of the prefill form subtracts a running max and rescales by exp(m_old - m_new); the arguments it rounds are no
    larger than max - s_j.)
  * The fp32 sums over the L_t keys, of p v for the output and of p for the normaliser, in any order and any grouping into
    tiles or lanes, cost at most eps L_t A together to first order (each is gamma_{L_t - 1} of its magnitude sum; the pairwise
    and tiled orders the kernels use stay far below the chain's bound, which leaves room for both).
  * 16 eps A covers what is left and does not grow with the problem: the exponential itself (v_exp_f32 and expf are good to a
    few ulp), the final division, the rescale factors of the online softmax, and the store.
  * 1e-12 only keeps the comparison meaningful where A underflows; it is far below one fp32 ulp of any output here.

This is a derivation, not a measurement, and nothing in it is fitted to what a kernel returns."""
import math

import torch

EPS32 = 2.0 ** -24


def visible(tq, length, pos0, device=None):
    """[Tq, L] bool: key j is visible to query t iff j <= pos0 + t."""
    j = torch.arange(length, device=device).view(1, length)
    t = torch.arange(tq, device=device).view(tq, 1)
    return j <= pos0 + t


def masked_attention(q, k, v, vis, scale=None):
    """softmax(q k^T * scale, keys outside `vis` removed) v in the dtype of the operands; a query that sees no key gives 0."""
    d = q.shape[-1]
    s = (q @ k.transpose(-2, -1)) * (1.0 / math.sqrt(d) if scale is None else scale)
    s = s.masked_fill(~vis, float("-inf"))
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - torch.where(torch.isinf(m), torch.zeros_like(m), m))
    z = e.sum(-1, keepdim=True)
    return (e / torch.where(z > 0, z, torch.ones_like(z))) @ v


def attention_ref(q, k, v, pos0):
    """q [B,H,Tq,D], k, v [B,H,L,D] float64 (every row of k and v finite; L >= pos0 + Tq) -> (out, tol), both [B,H,Tq,D] float64."""
    assert q.dtype == k.dtype == v.dtype == torch.float64
    tq, d = q.shape[-2:]
    length = k.shape[-2]
    assert pos0 >= 0 and pos0 + tq <= length
    vis = visible(tq, length, pos0, q.device)
    rs = 1.0 / math.sqrt(d)
    s = ((q @ k.transpose(-2, -1)) * rs).masked_fill(~vis, float("-inf"))
    smax = s.amax(-1, keepdim=True)
    p = torch.softmax(s, -1)
    out = p @ v
    a = p @ v.abs()
    smag = ((q.abs() @ k.abs().transpose(-2, -1)) * rs).masked_fill(~vis, 0.0).amax(-1, keepdim=True)
    r = (p * (smax - s).masked_fill(~vis, 0.0)).sum(-1, keepdim=True)
    nvis = vis.sum(-1).to(torch.float64).view(tq, 1)
    tol = (2 * (d + 4) * EPS32 * smag + EPS32 * (nvis + 2 * r + 16)) * a + 1e-12
    return out, tol


# ---------------------------------------------------------------- wrong references (float64), for the host test of the bound
def wrong_mask_longer(q, k, v, pos0):
    """Every query sees one key more; the row after the last written one is zero in K and V (uninitialised but finite)."""
    z = torch.zeros_like(k[..., :1, :])
    k1, v1 = torch.cat([k, z], -2), torch.cat([v, z], -2)
    return masked_attention(q, k1, v1, visible(q.shape[-2], k1.shape[-2], pos0 + 1, q.device))


def wrong_mask_shorter(q, k, v, pos0):
    """Every query that sees more than one key loses its last one."""
    tq, length = q.shape[-2], k.shape[-2]
    vis, short = visible(tq, length, pos0, q.device), visible(tq, length, pos0 - 1, q.device)
    return masked_attention(q, k, v, torch.where(short.any(-1, keepdim=True), short, vis))


def wrong_dropped_key(q, k, v, pos0, j):
    """Key j is skipped by every query (queries that would see nothing else keep it)."""
    vis = visible(q.shape[-2], k.shape[-2], pos0, q.device)
    drop = vis.clone()
    drop[:, j] = False
    return masked_attention(q, k, v, torch.where(drop.any(-1, keepdim=True), drop, vis))


def wrong_scale(q, k, v, pos0):
    """Scores scaled by 1 / sqrt(D + 1)."""
    d = q.shape[-1]
    return masked_attention(q, k, v, visible(q.shape[-2], k.shape[-2], pos0, q.device), scale=1.0 / math.sqrt(d + 1))


def online_softmax(q, k, v, pos0, rescale=True, tile=32):
    """The prefill form's online softmax restated in float64: keys in tiles of `tile`, running max m and sum l, the output
    accumulator and l multiplied by alpha = exp(m_old - m_new) when the max moves.  rescale=False omits that factor on the
    output accumulator (the wrong reference); with it the result equals `masked_attention` to float64 rounding."""
    tq, d = q.shape[-2:]
    length = k.shape[-2]
    vis = visible(tq, length, pos0, q.device)
    s = ((q @ k.transpose(-2, -1)) / math.sqrt(d)).masked_fill(~vis, float("-inf"))
    m = torch.full(q.shape[:-1] + (1,), float("-inf"), dtype=q.dtype, device=q.device)
    l = torch.zeros_like(m)
    acc = torch.zeros_like(q)
    for j0 in range(0, length, tile):
        st = s[..., j0:j0 + tile]
        m_new = torch.maximum(m, st.amax(-1, keepdim=True))
        m_use = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
        alpha = torch.exp(m - m_use)
        e = torch.exp(st - m_use)
        l = l * alpha + e.sum(-1, keepdim=True)
        acc = (acc * alpha if rescale else acc) + e @ v[..., j0:j0 + tile, :]
        m = m_new
    return acc / torch.where(l > 0, l, torch.ones_like(l))


# ---------------------------------------------------------------- inputs shared by the host and the GPU tests
PATTERNS = ("unit", "q8", "key0", "rising")


def make_inputs(pattern, b, h, tq, length, d, seed):
    """fp32 q [B,H,Tq,D], k, v [B,H,L,D] on the CPU, built from a seeded generator and from each other only.

    unit    q, k, v ~ N(0, 1): scores ~ N(0, 1).
    q8      q scaled by 8: scores ~ N(0, 64), sharp softmaxes (the exp2-domain scores of the prefill form, expf(ps - gmax) of
            the decode form, far from 0).
    key0    every query gets the common component 6 u (u a unit vector per (b, h)), the keys are 0.25 N(0, 1) and key 0 is
            c sqrt(D) dir, dir the direction of the mean query, with c computed from the float64 scores so that key 0 beats every
            other key of every query by at least 1.  Meant to reach: the running max of the prefill form is set in tile 0 and
            never moves, alpha == 1 in every lane of a full wave and the wave-uniform `rescale` shortcut is taken for every
            later tile (a wave with lanes past Tq still rescales: those lanes have alpha = 0).
    rising  same queries, and key j gains j c sqrt(D) dir with c from the float64 scores so that every full 32-key tile's
            maximum exceeds the previous tile's by at least 1 for every query.  Meant to reach: the running max moves in every
            tile, every tile rescales.  (A ragged last tile may or may not move it.)
    Whether the shortcut was taken cannot be observed from outside; `pattern_property` checks the stated property of the scores."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(b, h, tq, d, generator=g)
    k = torch.randn(b, h, length, d, generator=g)
    v = torch.randn(b, h, length, d, generator=g)
    if pattern == "unit":
        return q, k, v
    if pattern == "q8":
        return q * 8, k, v
    u = torch.randn(b, h, 1, d, generator=g)
    q = q + 6 * u / u.norm(dim=-1, keepdim=True)
    k = k * 0.25
    qd, kd = q.double(), k.double()
    dirn = qd.mean(-2, keepdim=True)
    dirn = dirn / dirn.norm(dim=-1, keepdim=True)                     # [B,H,1,D]
    proj = (qd * dirn).sum(-1)                                         # [B,H,Tq]  q_t . dir
    assert proj.min().item() > 0.5, "the common component does not dominate the queries"
    s = (qd @ kd.transpose(-2, -1)) / math.sqrt(d)                     # scores of the random keys
    if pattern == "key0":
        c = ((s[..., 1:].amax(-1) + 1.0) / proj).amax(-1).view(b, h, 1)   # score of key 0 = c (q_t . dir)
        k[..., 0, :] = (c * math.sqrt(d) * dirn[..., 0, :]).float()
        return q, k, v
    assert pattern == "rising"
    spread = (s.amax(-1) - s.amin(-1) + 1.0) / (32.0 * proj)           # a tile later = 32 c (q_t . dir) more
    c = spread.amax(-1).view(b, h, 1, 1)
    k = (kd + torch.arange(length, dtype=torch.float64).view(1, 1, length, 1) * c * math.sqrt(d) * dirn).float()
    return q, k, v


def pattern_property(pattern, q, k, pos0):
    """Assert on the float64 scores of fp32 inputs what `make_inputs` says key0 / rising are meant to reach."""
    tq, d = q.shape[-2:]
    length = k.shape[-2]
    vis = visible(tq, length, pos0)
    s = ((q.double() @ k.double().transpose(-2, -1)) / math.sqrt(d)).masked_fill(~vis, float("-inf"))
    if pattern == "key0":
        assert length > 1 and (s[..., 0] - s[..., 1:].amax(-1)).min().item() > 0.5
    elif pattern == "rising":
        full = (pos0 + 1) // 32     # tiles that every query sees whole
        assert full >= 2
        tmax = s[..., :full * 32].reshape(s.shape[:-1] + (full, 32)).amax(-1)
        assert (tmax[..., 1:] - tmax[..., :-1]).min().item() > 0.5

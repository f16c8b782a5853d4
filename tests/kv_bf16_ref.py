"""Reference of the bf16 KV-cache mode (include/ccvs_hip_kv16.h): the rounding written out in integer arithmetic, attention over a
rounded cache through tests/attention_ref.py, and the op-level cost of the mode in float64.  Plain torch, runs anywhere.

ROUNDING.  Round to nearest, ties to even, on the fp32 bit pattern u:  bits = (u + 0x7fff + ((u >> 16) & 1)) >> 16, a NaN gives 0x7fc0.
The carry of the addition moves a mantissa of all ones into the exponent, so the largest finite fp32 becomes inf; denormals, zeros and
infinities need no case of their own.  `test_kv_bf16_host.py` checks it against `torch.Tensor.to(torch.bfloat16)`.

A bf16 value IS an fp32 value (its low 16 bits are zero), so attention over the stored cache is `attention_ref` on the rounded K and V,
and the derived per-element bound of that file holds unchanged for the kernels that read a bf16 cache: they widen exactly and compute in
fp32.

COST OF THE MODE at op level, float64, per query t (the figure DESIGN.md 4.28 quotes):

    |attn(q, K, V) - attn(q, rnd K, rnd V)|  <=  (e^{2 delta_t} - 1 + 2^-9) max|v|,      delta_t = 2^-9 scale max_j sum_d |q_td k_jd|

(j over the visible keys).  A score moves by at most sum_d |q_d| |rnd k_jd - k_jd| scale; with every score within delta of its exact
value each softmax weight changes by a factor inside [e^{-2 delta}, e^{2 delta}], so sum_j |p'_j - p_j| <= e^{2 delta} - 1, and the
values move by their own rounding.  The 2^-9 is the rounding error of a bf16 value as the issue states it; the worst single element
can be off by 2^-8 of its magnitude (8 significant bits), a sum over D dims of independent errors stays far inside: the bound is CHECKED
on the inputs the tests use (test_kv_bf16_host.py), not assumed."""
import math

import torch

import attention_ref as R


def bf16_bits(x):
    """fp32 tensor -> int32 tensor of the 16-bit patterns (0 .. 0xffff) of the values rounded to bfloat16."""
    assert x.dtype == torch.float32
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    r = (u + 0x7fff + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7fffffff) > 0x7f800000
    return torch.where(nan, torch.full_like(r, 0x7fc0), r).to(torch.int32)


def bits_of(t):
    """bf16 tensor -> int32 tensor of its 16-bit patterns."""
    assert t.dtype == torch.bfloat16
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xffff


def bf16_round(x):
    """fp32 tensor -> fp32 tensor of the values a bf16 cache returns for it."""
    return (bf16_bits(x) << 16).to(torch.int32).view(torch.float32)


def truncate(x):
    """The wrong rounding: the low 16 bits dropped."""
    return (x.contiguous().view(torch.int32) & ~0xffff).view(torch.float32)


def attention_rounded_ref(q, k, v, pos0):
    """q, k, v fp32 (attention_ref's shapes) -> (out, tol) float64 of the attention over the ROUNDED k and v."""
    return R.attention_ref(q.double(), bf16_round(k).double(), bf16_round(v).double(), pos0)


def mode_cost(q, k, v, pos0):
    """-> (|attn(q,K,V) - attn(q,rnd K,rnd V)|, its bound), both [B,H,Tq,D] float64 (the bound is per query, broadcast over D)."""
    qd, kd, vd = q.double(), k.double(), v.double()
    tq, d = q.shape[-2:]
    vis = R.visible(tq, k.shape[-2], pos0, q.device)
    exact = R.masked_attention(qd, kd, vd, vis)
    stored = R.masked_attention(qd, bf16_round(k).double(), bf16_round(v).double(), vis)
    sabs = (qd.abs() @ kd.abs().transpose(-2, -1)) / math.sqrt(d)
    delta = 2.0 ** -9 * sabs.masked_fill(~vis, 0.0).amax(-1, keepdim=True)
    bound = (torch.expm1(2 * delta) + 2.0 ** -9) * vd.abs().amax()
    return (exact - stored).abs(), bound.expand_as(exact)

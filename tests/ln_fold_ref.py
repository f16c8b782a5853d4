"""Float64 reference of LayerNorm + Linear as the transformer runs it -- folded into the GEMM (gpt.hip, "LayerNorm is folded in
algebraically") -- with a per-element bound that does NOT depend on a row's mean, the row patterns on which a fold can lose its
accuracy, and fp32 emulations of two folds that do (the wrong references the bound has to tell from the right one).  Plain torch,
runs anywhere.

The operation, from the UNFOLDED operands W [N,K], b [N], gamma, beta [K] (never from the packed wg, bb, s):

    xhat = (x - mean) / sqrt(var + eps)          want = (xhat gamma + beta) @ W^T + b

The bound, per element, from float64 magnitudes only:

    |got - want| <= REL * A,     REL = 1e-5,     A = ((|xhat| + 1) |gamma| + |beta|) @ |W|^T + |b|

  * (|xhat| |gamma| + |beta|) @ |W|^T + |b| is the sum of the magnitudes of what a Linear applied to a LayerNorm adds up: the
    rounding error of an fp32 chain of K terms is at most K eps times it and, for errors that behave as a random walk, about
    sqrt(K) eps: 3.8e-6 at K = 4096 with eps = 2^-24, below REL (tests/test_gemm_forms_gpu.py bounds the plain GEMM the same
    way and observes ~1e-7).
  * The `+ 1`: the mean and the variance are sums of K fp32 terms as well.  Summed from terms of the size of the row's spread,
    the mean is off by about eps sqrt(K) std and the variance by about eps sqrt(K) var: xhat moves by about eps sqrt(K) (1 +
    |xhat| / 2), whatever the row's mean is.  One unit of xhat per element, times |gamma| |W|, carries that with the same
    sqrt(K) eps <= 3.8e-6 < REL.
  * Nothing in A grows with |mean| / std.  LayerNorm itself does not depend on the mean; an implementation whose error does --
    a one-pass variance `sum x^2 / K - mean^2` (eps (mean / std)^2 of the variance), an accumulator `x @ W'^T - mean * s`
    (eps |mean| / std of the output) -- exceeds the bound where the rows have a large mean, and that is what it is for.  The
    bound of tests/test_gemm_forms_gpu.py, A = rstd (|x| @ |wg|^T + |mean| |s|) + |bb|, is the size of that fold's own
    intermediates and loosens exactly as the fold loses accuracy.
  * A GELU behind the Linear: 1.2 A + 1e-3 (|gelu'| <= 1.13, plus the erf's own rounding), as tests/test_gemm_forms_gpu.py.

This is a derivation, not a measurement, and nothing in it is fitted to what a kernel returns.  What the fp32 reference itself
(torch's F.linear(F.layer_norm(x)) on the CPU) leaves of it is asserted in tests/test_ln_fold_host.py: it stays inside on every
pattern with a factor 1.5 to spare (0.16 of the bound at K >= 1024 on P2; at K = 64 it reached 0.97 on P2, so the host test draws
P2 around 500 there -- torch sums the raw x, and its mean of 64 values around 1e3 is good to an ulp of 1e3, 6e-5 of the row's std).

Row patterns, cycled over the rows (row r has pattern r % 7) so that every row block of every kernel form holds several:

    P0  N(0.3, 0.7)              what the other suites draw
    P1  N(100, 1)                |mean| / std = 1e2
    P2  N(1e3, 1)                |mean| / std = 1e3: a residual stream with a large shared offset
    P3  N(3, 0.01)               small spread around a moderate mean
    P4  constant 1e3 / 3         var = 0: the output is beta @ W^T + b
    P5  x[0] = 1, rest N(0, 1e-3)      the row's FIRST element is its outlier: |x0 - mean| / std ~ sqrt(K)
    P6  x[0] = -200, rest N(100, 1)    the same with a large mean

P5 and P6 are there against a cure that is worse than the disease: shifting a row by its first element removes the cancellation
of P1..P4 and creates it where that element is the outlier (a one-pass variance then loses K eps)."""
import torch
import torch.nn.functional as F

REL = 1e-5
LN_EPS = 1e-5
PATTERNS = ("P0 N(0.3,0.7)", "P1 N(100,1)", "P2 N(1e3,1)", "P3 N(3,0.01)", "P4 const 1e3/3", "P5 x0=1 rest N(0,1e-3)", "P6 x0=-200 rest N(100,1)")
NP = len(PATTERNS)


def pattern_rows(m, k, seed, p2_mean=1e3):
    """x [m, k] fp32 on the CPU, row r of pattern r % 7 (seeded).  `p2_mean`: the mean of the P2 rows, for the host test at K = 64,
    where torch's own fp32 LayerNorm leaves too little of the bound at 1e3 (tests/test_ln_fold_host.py); the GPU tests keep 1e3."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(m, k, generator=g, dtype=torch.float64)
    x = torch.empty(m, k, dtype=torch.float64)
    for r in range(m):
        p = r % NP
        if p == 0:
            x[r] = 0.3 + 0.7 * z[r]
        elif p == 1:
            x[r] = 100 + z[r]
        elif p == 2:
            x[r] = p2_mean + z[r]
        elif p == 3:
            x[r] = 3 + 0.01 * z[r]
        elif p == 4:
            x[r] = 1e3 / 3
        elif p == 5:
            x[r] = 1e-3 * z[r]
            x[r, 0] = 1.0
        else:
            x[r] = 100 + z[r]
            x[r, 0] = -200.0
    return x.float()


def linear_operands(n, k, seed):
    """W [n,k] ~ N(0, 1/k), b ~ N(0,1), gamma ~ 1 + 0.3 N, beta ~ 0.2 N: fp32 on the CPU, as the other GEMM suites draw them."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k, generator=g) / k ** 0.5
    b = torch.randn(n, generator=g)
    gamma = 1 + 0.3 * torch.randn(k, generator=g)
    beta = 0.2 * torch.randn(k, generator=g)
    return w, b, gamma, beta


def ln_linear_ref(x, w, b, gamma, beta, eps=LN_EPS):
    """(want, A) in float64 from fp32 (or any) operands: Linear(LayerNorm(x)) and the mean-independent magnitude A above."""
    x64, w64, b64, g64, be64 = (t.detach().double().cpu() for t in (x, w, b, gamma, beta))
    mean = x64.mean(dim=1, keepdim=True)
    var = ((x64 - mean) ** 2).mean(dim=1, keepdim=True)
    xhat = (x64 - mean) / torch.sqrt(var + eps)
    want = (xhat * g64 + be64) @ w64.t() + b64
    a = ((xhat.abs() + 1) * g64.abs() + be64.abs()) @ w64.abs().t() + b64.abs()
    return want, a


def gelu_ref(want, a):
    """The reference and the bound's magnitude behind a GELU epilogue."""
    return F.gelu(want), 1.2 * a + 1e-3


def fractions(got, want, a):
    """Largest |got - want| / (REL A) per pattern: a list of 7 floats (NaN for a pattern without rows; inf where got is not finite).
    got [m, ...]: row r (dim 0) has pattern r % 7."""
    got = got.detach().double().cpu()
    assert got.shape == want.shape == a.shape, (got.shape, want.shape, a.shape)
    frac = ((got - want).abs() / (REL * a)).reshape(got.shape[0], -1)
    frac = torch.where(torch.isfinite(got.reshape(got.shape[0], -1)), frac, torch.full_like(frac, float("inf")))
    return [frac[p::NP].max().item() if frac[p::NP].numel() else float("nan") for p in range(NP)]


def show(what, fr):
    print(f"{what}: max |err| / (REL A) per pattern = [" + ", ".join(f"P{p} {v:.3g}" for p, v in enumerate(fr)) + "]")


def check(got, want, a, what):
    """Print the per-pattern fractions, then assert every one is at most 1 (and the output finite).  Returns them."""
    fr = fractions(got, want, a)
    show(what, fr)
    worst = max(v for v in fr if v == v)
    assert worst <= 1.0, f"{what}: max |err| / (REL A) = {worst:.3g} > 1 (per pattern: {[f'{v:.3g}' for v in fr]})"
    return fr


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 on the CPU: the right one, and the wrong references
# ---------------------------------------------------------------------------------------------------------------------------
def torch_fp32(x, w, b, gamma, beta, eps=LN_EPS):
    """torch's own fp32 LayerNorm + Linear on the CPU."""
    return F.linear(F.layer_norm(x, (x.shape[1],), gamma, beta, eps), w, b)


def pack(w, b, gamma, beta):
    """(wg, bb, s) fp32 = (W gamma, b + W beta, rowsum(W gamma)): what ops.pack_ln_linear hands the kernels."""
    wg = (w * gamma.view(1, -1)).contiguous()
    bb = b + (w.double() @ beta.double()).float()
    s = wg.double().sum(dim=1).float()
    return wg, bb, s


def fold_fp32(x, w, b, gamma, beta, shift="none", eps=LN_EPS, chains=64):
    """The one-pass fold, every operation rounded to fp32:  rstd (d @ wg^T - mean s) + bb  with  mean = sum d / K,
    var = max(sum d^2 / K - mean^2, 0), on d = x - c:
        shift "none"    c = 0                 the fold on the raw activations
        shift "first"   c = x[:, :1]          the row's first element
        shift "quad"    c = mean(x[:, :4])    the mean of the row's first four elements
    `chains` partial sums per row (as many lanes / K slices accumulate side by side in a kernel), each a sequential fp32 chain,
    then added up in order."""
    m, k = x.shape
    wg, bb, s = pack(w, b, gamma, beta)
    if shift == "none":
        d = x.clone()
    elif shift == "first":
        d = x - x[:, :1]
    elif shift == "quad":
        d = x - ((x[:, 0:1] + x[:, 1:2]) + (x[:, 2:3] + x[:, 3:4])) * 0.25
    else:
        raise ValueError(shift)
    chains = min(chains, k)
    assert k % chains == 0
    steps = k // chains
    dv = d.view(m, steps, chains)
    sx = torch.zeros(m, chains)
    sxx = torch.zeros(m, chains)
    acc = torch.zeros(m, wg.shape[0], chains)
    wv = wg.view(-1, steps, chains)
    for i in range(steps):   # one fp32 rounding per add and per product
        sx = sx + dv[:, i]
        sxx = sxx + dv[:, i] * dv[:, i]
        acc = acc + dv[:, i].unsqueeze(1) * wv[:, i].unsqueeze(0)
    a1, b1, y = sx[:, 0].clone(), sxx[:, 0].clone(), acc[:, :, 0].clone()
    for c in range(1, chains):
        a1 = a1 + sx[:, c]
        b1 = b1 + sxx[:, c]
        y = y + acc[:, :, c]
    mean = (a1 / k).unsqueeze(1)
    var = torch.clamp((b1 / k).unsqueeze(1) - mean * mean, min=0.0)
    rstd = torch.rsqrt(var + eps)
    return rstd * (y - mean * s.unsqueeze(0)) + bb.unsqueeze(0)

"""-m gpu: the quantiser's argmin (`vq_argmin_kernel`, csrc/vq.hip) judged against float64 distances, at the shapes the
golden cases never launch: partial and image-straddling 32-row tiles, channel counts off the unroll step, codebooks whose
32-code blocks do not divide among the 4 waves, every (wave, register, lane half) code position, ties, non-finite rows,
and the padded codebook of `VectorQuantizer`.

The judge.  The kernel returns indices only, so an index is judged by the float64 distance of the code it names.  With
u = 2^-24 (fp32 unit roundoff), z a row and e a code, both fp32 C-vectors, the kernel evaluates

    d = fl(fl(zz + ee) - 2 * acc),   zz = fl(sum z_k^2),  ee = fl(sum e_k^2),  acc = fl(sum z_k e_k).

A sum of C rounded products carries at most C roundings per term (first order in u), whatever the order of the additions:
|zz - |z|^2| <= C u |z|^2, |ee - |e|^2| <= C u |e|^2 and |acc - z.e| <= C u sum|z_k e_k| <= C u |z||e| (Cauchy-Schwarz).
The two roundings of the combination each cost at most u times a quantity bounded by |z|^2 + |e|^2 + 2|z||e|.  Summed,

    |d - D| <= C u (|z|^2 + |e|^2 + 2|z||e|) + 2 u (|z| + |e|)^2 = (C + 2) u (|z| + |e|)^2 <= E_r,
    E_r = (C + 2) * 2^-24 * (|z_r| + max_j |e_j|)^2.

If the kernel prefers code g over the float64 minimiser m then d_g <= d_m, so D_g - D_m <= 2 E_r; the rule allows 4 E_r
because the matrix instruction's internal rounding is not documented step by step.  A row whose float64 top-2 gap exceeds
4 E_r therefore has one admissible answer, the float64 argmin; the others are "ambiguous", and a case may hold at most 5 %
of them, so that the margin cannot hide a wrong kernel.

Ambiguous share of every case (float64, CPU; a property of the inputs alone):

    z shape            n_e    random   near
    (3, 6, 5, 7)       64     0 %      0 %   (105 rows)
    (1, 4, 1, 3)       32     0 %      0 %   (3 rows)
    (70, 16, 1, 1)     96     0 %      0 %   (70 rows)
    (2, 18, 3, 11)     160    0 %      0 %   (66 rows)
    (5, 34, 4, 4)      96     0 %      0 %   (80 rows)
    (2, 2, 9, 9)       32     0 %      0 %   (162 rows)
    (1, 1024, 2, 3)    64     0 %      0 %   (6 rows)
    (4, 512, 8, 8)     16384  3.12 %   0 %   (8 of 256 rows)
    (33, 512, 1, 1)    1024   3.03 %   0 %   (1 of 33 rows)
    module, 50 codes (3, 6, 5, 7) and flat [4, 5, 6]: 0 %, random and near; the non-finite case's clean input: 0 %
    module with one row of 105 scaled by 1e18 or 1e20: 0.95 % (that row: every code is within E_r of every other)
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24     # fp32 unit roundoff
MARGIN = 4.0       # in units of E_r
CAP = 0.05         # largest admissible share of ambiguous rows per case


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ccvs_amd import ops as _ops
    return _ops


# ------------------------------------------------------------------ inputs and the float64 judge
def rows_to_nchw(zf, shape):
    n, c, h, w = shape
    return zf.view(n, h, w, c).permute(0, 3, 1, 2).contiguous()


def nchw_to_rows(z):
    return z.permute(0, 2, 3, 1).reshape(-1, z.shape[1])


def make_inputs(shape, n_e, kind, seed):
    """Codebook 0.3 N(0,1); z either 0.3 N(0,1) ("random") or a codebook row + 0.15 N(0,1) ("near", like a trained encoder)."""
    g = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    rows = n * h * w
    cb = 0.3 * torch.randn(n_e, c, generator=g)
    if kind == "random":
        zf = 0.3 * torch.randn(rows, c, generator=g)
    else:
        zf = cb[torch.randint(0, n_e, (rows,), generator=g)] + 0.15 * torch.randn(rows, c, generator=g)
    return rows_to_nchw(zf, shape), cb


def distances64(z, cb):
    """D[r, j] = |z_r|^2 + |e_j|^2 - 2 z_r.e_j and E_r, in float64 from the fp32 inputs."""
    zf, e = nchw_to_rows(z).double(), cb.double()
    D = (zf ** 2).sum(1, keepdim=True) + (e ** 2).sum(1) - 2.0 * zf @ e.t()
    E = (cb.shape[1] + 2) * U * (zf.norm(dim=1) + e.norm(dim=1).max()) ** 2
    return D, E


class Ref:
    """The float64 verdict on one case: minimiser, minimum, and which rows are ambiguous.  Computed once, never modified."""

    def __init__(self, z, cb):
        D, E = distances64(z, cb)
        two = D.topk(2, dim=1, largest=False) if D.shape[1] > 1 else None
        self.D, self.E = D, E
        self.dmin, self.argmin = D.min(dim=1)
        self.ambiguous = (two.values[:, 1] - two.values[:, 0]) <= MARGIN * E
        self.share = self.ambiguous.double().mean().item()


def judge(got, ref, n_e, label):
    got = got.cpu()
    rows = ref.D.shape[0]
    assert got.shape == (rows,) and got.dtype == torch.int64, (got.shape, got.dtype)
    bad = ((got < 0) | (got >= n_e)).nonzero().flatten().tolist()
    assert not bad, f"{label}: rows {bad[:8]} out of [0, {n_e}): {got[bad[:8]].tolist()}"
    print(f"{label}: {rows} rows, ambiguous share {100 * ref.share:.2f} %")
    assert ref.share <= CAP, f"{label}: {100 * ref.share:.2f} % of the rows are ambiguous, the inputs do not judge the kernel"
    excess = ref.D.gather(1, got[:, None])[:, 0] - ref.dmin
    worst = int((excess - MARGIN * ref.E).argmax())
    assert excess[worst] <= MARGIN * ref.E[worst], (
        f"{label}: row {worst} got code {int(got[worst])}, {excess[worst]:.3e} above the float64 minimum "
        f"(code {int(ref.argmin[worst])}); 4 E_r = {MARGIN * ref.E[worst]:.3e}")
    wrong = (~ref.ambiguous & (got != ref.argmin)).nonzero().flatten().tolist()
    assert not wrong, (f"{label}: unambiguous rows {wrong[:8]} got {got[wrong[:8]].tolist()}, "
                       f"float64 argmin {ref.argmin[wrong[:8]].tolist()}")


def run(ops, z, cb):
    cbd = cb.cuda()
    return ops.vq_argmin(z.cuda(), cbd.t().contiguous(), (cbd ** 2).sum(1))


# ------------------------------------------------------------------ ragged tiles, depth and width
CASES = [
    # ragged rows and tiles that straddle images
    ((3, 6, 5, 7), 64),        # 105 rows: last tile holds 9; HW = 35
    ((1, 4, 1, 3), 32),        # fewer than 32 rows, one 32-code block: three waves idle
    ((70, 16, 1, 1), 96),      # HW = 1 (the flat path), 3 blocks among 4 waves
    ((2, 18, 3, 11), 160),     # HW = 33, C = 18 off the unroll step, 5 blocks: wave 0 runs twice
    ((5, 34, 4, 4), 96),       # HW = 16: two images per tile
    ((2, 2, 9, 9), 32),        # C = 2: one MFMA step
    # depth and width
    ((1, 1024, 2, 3), 64),     # the LDS maximum
    ((4, 512, 8, 8), 16384),   # the Kinetics codebook: 128 blocks per wave
    ((33, 512, 1, 1), 1024),   # one full tile and one row
]


@functools.lru_cache(maxsize=None)
def case(i, kind):
    shape, n_e = CASES[i]
    z, cb = make_inputs(shape, n_e, kind, i)
    return z, cb, Ref(z, cb)


@pytest.mark.parametrize("kind", ["random", "near"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{'x'.join(map(str, s))}-{n}" for s, n in CASES])
def test_argmin_float64_margin(ops, i, kind):
    """Every row's code lies within 4 E_r of the float64 minimum, unambiguous rows equal the float64 argmin, and at most 5 %
    of a case's rows are ambiguous (shares in the module docstring)."""
    z, cb, ref = case(i, kind)
    judge(run(ops, z, cb), ref, cb.shape[0], f"{tuple(z.shape)} n_e={cb.shape[0]} {kind}")


@pytest.mark.parametrize("i,kind", [(0, "random"), (3, "near"), (7, "random")])
def test_same_bits_twice(ops, i, kind):
    z, cb, _ = case(i, kind)
    a = run(ops, z, cb)
    b = run(ops, z, cb)
    assert torch.equal(a, b)


# ------------------------------------------------------------------ every code position
@pytest.mark.parametrize("n_e", [32, 160, 1024])
@pytest.mark.parametrize("order", ["identity", "permuted"])
def test_every_code_position(ops, n_e, order):
    """z_r = e_{t_r} exactly, one row per code, [n_e/32, 18, 4, 8]: row r returns t_r (t_r = r, and a permutation so that the
    tile position of a row and the position of its code differ).  Pins the (wave, register, lane half) -> code mapping and a
    minimum found in the last block of the last wave.  The nearest other code is about 2 C 0.09 = 3 away, E_r about 1e-5."""
    g = torch.Generator().manual_seed(100 + n_e)
    c = 18
    cb = 0.3 * torch.randn(n_e, c, generator=g)
    t = torch.arange(n_e) if order == "identity" else torch.randperm(n_e, generator=g)
    z = rows_to_nchw(cb[t].clone(), (n_e // 32, c, 4, 8))
    ref = Ref(z, cb)
    assert torch.equal(ref.argmin, t) and not ref.ambiguous.any()
    got = run(ops, z, cb).cpu()
    bad = (got != t).nonzero().flatten().tolist()
    assert not bad, f"rows {bad[:8]}: got {got[bad[:8]].tolist()}, want {t[bad[:8]].tolist()}"


# ------------------------------------------------------------------ ties
@pytest.mark.parametrize("codes", [(1, 9),          # one lane, two registers
                                   (1, 5),          # the two lane halves
                                   (5, 37),         # two waves
                                   (5, 133),        # one wave, a later iteration
                                   (31, 159),       # the last code
                                   (12, 44, 76),    # three waves
                                   (44, 76, 108)])  # three waves, none of them the first
def test_ties_keep_lowest_index(ops, codes):
    """Equal codebook rows give bit-equal distances; every row of z is that codebook row, over a full and a partial tile:
    the lowest of the tied indices comes back, as from torch.argmin."""
    g = torch.Generator().manual_seed(7)
    n_e, c = 160, 18
    cb = 0.3 * torch.randn(n_e, c, generator=g)
    for k in codes[1:]:
        cb[k] = cb[codes[0]]
    z = rows_to_nchw(cb[codes[0]].expand(40, c).contiguous(), (40, c, 1, 1))
    esq = (cb.cuda() ** 2).sum(1).cpu()
    assert all(esq[k] == esq[codes[0]] for k in codes)
    got = run(ops, z, cb).cpu()
    assert (got == codes[0]).all(), f"tie {codes}: got {got.unique().tolist()}"


# ------------------------------------------------------------------ non-finite rows
def test_non_finite_rows_return_zero(ops):
    """A row whose every distance is NaN or +inf returns 0 like torch.argmin (not an unset 2^31 - 1), and leaves the other
    rows of its tile and of the next one as they are without it.  40 rows as [2, 6, 4, 5]: tiles of 32 and 8 rows."""
    shape, n_e = (2, 6, 4, 5), 64
    z, cb = make_inputs(shape, n_e, "random", 11)
    clean = run(ops, z, cb).cpu()
    judge(clean, Ref(z, cb), n_e, "non-finite, clean input")
    zf = nchw_to_rows(z).clone()
    poisoned = [3, 17, 35]
    zf[3] = float("nan")
    zf[17, 2] = float("inf")
    zf[35] = float("-inf")
    got = run(ops, rows_to_nchw(zf, shape), cb).cpu()
    assert ((got >= 0) & (got < n_e)).all(), f"out of [0, {n_e}): {got[(got < 0) | (got >= n_e)].tolist()}"
    assert got[poisoned].tolist() == [0, 0, 0], got[poisoned].tolist()
    keep = torch.ones(40, dtype=torch.bool)
    keep[poisoned] = False
    assert torch.equal(got[keep], clean[keep])


# ------------------------------------------------------------------ the module
def make_quantizer(n_e, c, seed, **kw):
    from ccvs_amd.models.skip_vid_generator.modules.quantize import VectorQuantizer
    q = VectorQuantizer(n_e, c, 0.25, **kw).cuda()
    cb = 0.3 * torch.randn(n_e, c, generator=torch.Generator().manual_seed(seed))
    with torch.no_grad():
        q.embedding.weight.copy_(cb)
    return q, cb


@pytest.mark.parametrize("kind", ["random", "near"])
def test_module_padded_codebook(ops, kind):
    """VectorQuantizer(50, 6): the tables are padded to 64 codes, 14 of them at +inf.  `indices` passes the rule against the 50
    real codes on a [3, 6, 5, 7] map and on a flat [4, 5, 6] list of vectors (HW = 1)."""
    q, cb = make_quantizer(50, 6, 21)
    assert q._tables()[0].shape == (6, 64) and torch.isinf(q._tables()[1][50:]).all()
    z, _ = make_inputs((3, 6, 5, 7), 50, kind, 21)   # same seed: "near" rows sit near this codebook
    judge(q.indices(z.cuda()), Ref(z, cb), 50, f"module (3, 6, 5, 7) {kind}")
    flat, _ = make_inputs((20, 6, 1, 1), 50, kind, 21)
    judge(q.indices(flat.view(4, 5, 6).cuda()), Ref(flat, cb), 50, f"module flat [4, 5, 6] {kind}")


@pytest.mark.parametrize("scale", [1e18, 1e20])
def test_module_huge_row_stays_in_vocabulary(ops, scale):
    """A row scaled by 1e18 (every code at the same fp32 distance) or by 1e20 (|z|^2 overflows: +inf on every code, real or
    padding) still returns one of the 50 real codes, and the other rows are judged as usual."""
    q, cb = make_quantizer(50, 6, 21)
    z, _ = make_inputs((3, 6, 5, 7), 50, "random", 22)
    z[1, :, 2, 3] *= scale
    if scale == 1e20:
        assert torch.isinf((z[1, :, 2, 3] ** 2).sum())
    got = q.indices(z.cuda())
    assert int(got.max()) < 50 and int(got.min()) >= 0, (int(got.min()), int(got.max()))
    judge(got, Ref(z, cb), 50, f"module, one row x {scale:g}")


def test_module_forward_normalize(ops):
    """forward(normalize=True) = gather, then divide by the channel norm: within 2 ulp of fp32 of the float64 quotient per
    element (sum of 6 squares, square root, division: each rounded once).  Indices come back as [N*H*W, 1]."""
    q, cb = make_quantizer(50, 6, 21, normalize=True)
    z, _ = make_inputs((3, 6, 5, 7), 50, "near", 21)
    zq, loss, (perplexity, onehot, idx) = q(z.cuda())
    assert loss is None and perplexity is None and onehot is None
    assert idx.shape == (105, 1) and idx.dtype == torch.int64 and zq.shape == z.shape
    judge(idx[:, 0], Ref(z, cb), 50, "module forward")
    rows = cb.double()[idx[:, 0].cpu()]
    want = rows_to_nchw(rows / rows.norm(dim=1, keepdim=True), z.shape).numpy()
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(zq.cpu().double().numpy() - want) / ulp
    print(f"normalize: max error {err.max():.3f} ulp")
    assert err.max() <= 2.0, f"{err.max():.3f} ulp"


@pytest.mark.parametrize("shape", [(2, 5, 7), (9,), (4, 3)])
def test_module_embed_code(ops, shape):
    q, cb = make_quantizer(50, 6, 21)
    code = torch.randint(0, 50, shape, generator=torch.Generator().manual_seed(5))
    got = q.embed_code(code.cuda()).cpu()
    assert got.shape == (*shape, 6)
    assert torch.equal(got, cb[code])


def test_module_tables_follow_the_weight(ops):
    """Writing the embedding weight in place invalidates the packed (transposed, padded) tables: rows that sit on codes of the
    new codebook are quantised with the new codebook."""
    q, cb = make_quantizer(50, 6, 21)
    z, _ = make_inputs((3, 6, 5, 7), 50, "near", 21)
    judge(q.indices(z.cuda()), Ref(z, cb), 50, "module, first codebook")
    g = torch.Generator().manual_seed(23)
    cb2 = 0.3 * torch.randn(50, 6, generator=g)
    with torch.no_grad():
        q.embedding.weight.copy_(cb2)
    t = torch.randint(0, 50, (105,), generator=g)
    z2 = rows_to_nchw(cb2[t].clone(), (3, 6, 5, 7))
    ref2 = Ref(z2, cb2)
    assert torch.equal(ref2.argmin, t) and not ref2.ambiguous.any()
    assert (Ref(z2, cb).argmin != t).any()     # the stale tables would answer differently
    assert torch.equal(q.indices(z2.cuda()).cpu(), t)

"""-m gpu: `ccvs_token_nll` and `ccvs_mean_f32` through the C ABI against numpy float64.

Every case runs on poisoned memory: the outputs start as NaN, and every logits row the call does not list, every column >= ncols of
the rows it does, and the floats in front of and behind the logits are NaN -- a read outside the contract shows in the result.

Launch forms of `ccvs_token_nll` (csrc/metrics.hip: team per row x load width) and the cases of `FORMS` that reach them:
  a wave per row, 16-byte loads      ncols 1, 5, 64, 1024; 7 of ld 1024 with a row list; 33 x 3000 rows
  a wave per row, 4-byte loads       ncols 1024 of ld 1027; ncols 5 from a base offset by one float
  a workgroup per row (16 per lane), 16-byte loads    ncols 1025, 1027 of ld 1028 (the quad across ncols column by column), 4096
  a workgroup per row (16 per lane), 4-byte loads     ncols 1027 of ld 1027
  a workgroup per row (64 per lane), 16-byte loads    ncols 4097 of ld 4100, 16384; the real head shape 254 x 16384
  a workgroup per row (64 per lane), 4-byte loads     ncols 16384 from a base offset by one float
Bound: 1e-5 abs per token and for the mean, |logit| <= 80 (results below 64: half an fp32 ulp is 3.8e-6, the fp32 sum of ncols
exponentials in a fixed tree adds about 1e-6)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-5
PAD = 37   # poisoned floats in front of and behind the logits


def _ref_nll(logits, rows, target, ncols):
    """float64: logsumexp(row[:ncols]) - row[target]; NaN for a target outside [0, ncols)."""
    out = np.full(len(target), np.nan)
    for m, (r, t) in enumerate(zip(rows, target)):
        x = logits[r, :ncols].astype(np.float64)
        mx = x.max()
        if 0 <= t < ncols:
            out[m] = mx + np.log(np.exp(x - mx).sum()) - x[t]
    return out


def _call(logits, ld, rows, target, ncols, offset=0):
    """logits: float32 [R, ld] numpy, already NaN wherever the call must not read.  Returns (per-token fp32, mean fp32) as numpy."""
    from ccvs_amd import lib
    L = lib.load()
    R = logits.shape[0]
    # 16-byte aligned allocation; the logits start PAD4 + offset floats in, PAD4 a multiple of 4, so `offset` alone decides alignment
    pad4 = (PAD + 3) // 4 * 4
    buf = torch.full((pad4 + offset + R * ld + PAD,), float("nan"), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[pad4 + offset: pad4 + offset + R * ld]
    view.copy_(torch.from_numpy(logits.reshape(-1)))
    n = len(target)
    out = torch.full((n + 2,), float("nan"), dtype=torch.float32, device="cuda")    # one guard float on each side
    mean = torch.full((3,), float("nan"), dtype=torch.float32, device="cuda")
    tgt = torch.tensor(np.asarray(target), dtype=torch.int64, device="cuda")
    rws = None if rows is None else torch.tensor(np.asarray(rows), dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = ctypes.c_void_p
    lib.check(L.ccvs_token_nll(vp(view.data_ptr()), ld, vp(rws.data_ptr()) if rws is not None else vp(0), vp(tgt.data_ptr()), n, ncols,
                               vp(out.data_ptr() + 4), stream), "ccvs_token_nll")
    lib.check(L.ccvs_mean_f32(vp(out.data_ptr() + 4), n, vp(mean.data_ptr() + 4), stream), "ccvs_mean_f32")
    torch.cuda.synchronize()
    o, mn = out.cpu().numpy(), mean.cpu().numpy()
    assert np.isnan(o[0]) and np.isnan(o[-1]) and np.isnan(mn[0]) and np.isnan(mn[2]), "a write outside the outputs"
    return o[1:-1].copy(), mn[1]


def _case(n_rows, ncols, ld, rows=None, seed=0, scale=4.0):
    """Random logits in [-80, 80] for the listed rows (all R = n_rows rows when rows is None), NaN elsewhere; random targets with
    the first and the last column among them."""
    g = np.random.default_rng(seed)
    listed = list(range(n_rows)) if rows is None else list(rows)
    R = max(listed) + 2 if rows is not None else n_rows       # with a list: at least one unlisted row behind the last
    logits = np.full((R, ld), np.nan, dtype=np.float32)
    for r in set(listed):
        logits[r, :ncols] = np.clip(g.normal(0, scale, ncols), -80, 80).astype(np.float32)
    target = g.integers(0, ncols, len(listed))
    target[0] = 0
    target[-1] = ncols - 1
    return logits, listed, target


def _check(logits, ld, rows, listed, target, ncols, offset=0):
    got, mean = _call(logits, ld, rows, target, ncols, offset)
    want = _ref_nll(logits, listed, target, ncols)
    err = np.abs(got.astype(np.float64) - want).max()
    merr = abs(float(mean) - want.mean())
    print(f"ncols {ncols} ld {ld} rows {len(target)} offset {offset}: per-token max|err| {err:.2e}, mean err {merr:.2e}")
    assert not np.isnan(got).any(), "NaN: a read outside the listed rows / the first ncols columns"
    assert err <= TOL and merr <= TOL
    # the mean: float64 sum of the kernel's own fp32 values, rounded once -- exactly numpy's
    assert np.float32(got.astype(np.float64).mean()) == mean
    return got, mean


# (ncols, ld, offset): the row-width cases and the launch form each reaches (module docstring)
FORMS = [(1, 4, 0), (5, 8, 0), (64, 64, 0), (1024, 1024, 0), (1024, 1027, 0), (5, 8, 1), (1025, 1028, 0), (1027, 1028, 0), (4096, 4096, 0),
         (1027, 1027, 0), (4097, 4100, 0), (16384, 16384, 0), (16384, 16384, 1)]


@pytest.mark.parametrize("ncols,ld,offset", FORMS)
def test_token_nll_row_widths(ncols, ld, offset):
    logits, listed, target = _case(5, ncols, ld, seed=ncols + ld + offset)   # 5 rows: the last workgroup of the wave form is part empty
    got, _ = _check(logits, ld, None, listed, target, ncols, offset)
    if ncols == 1:
        assert (got == 0.0).all()


def test_token_nll_state_head_columns_and_row_list():
    """7 of 1024 columns (the state head reads :state_num of a z_num-wide row), rows with gaps, out of order, one repeated."""
    rows = [9, 2, 5, 2, 14, 0]
    logits, listed, target = _case(len(rows), 7, 1024, rows=rows, seed=3)
    got, _ = _check(logits, 1024, rows, listed, target, 7)
    swapped = np.array(target)                  # the repeated row's two targets exchanged
    swapped[1], swapped[3] = target[3], target[1]
    again, _ = _check(logits, 1024, rows, listed, swapped, 7)
    assert again[1] == got[3] and again[3] == got[1]
    # a wide row through the list as well: 1027 of ld 1028
    logits, listed, target = _case(4, 1027, 1028, rows=[3, 0, 6, 3], seed=4)
    _check(logits, 1028, [3, 0, 6, 3], listed, target, 1027)


@pytest.mark.parametrize("n_rows", [1, 3000])
def test_token_nll_row_counts(n_rows):
    """3000 rows: more than one pass of the 1024-thread mean, 750 workgroups of the wave form."""
    logits, listed, target = _case(n_rows, 33, 36, seed=n_rows)
    _check(logits, 36, None, listed, target, 33)


@pytest.mark.parametrize("ncols,ld", [(64, 64), (1027, 1028), (5000, 5000)])
def test_token_nll_values(ncols, ld):
    """Rows at +80 and at -80 (no overflow: both give log(ncols)), a row that is -inf but for two columns, a constant row, targets in
    the first and the last column."""
    logits = np.full((6, ld), np.nan, dtype=np.float32)
    logits[0, :ncols] = 80.0
    logits[1, :ncols] = -80.0
    logits[2, :ncols] = -np.inf
    logits[2, 1], logits[2, ncols - 1] = 1.5, -0.25
    logits[3, :ncols] = 0.375
    g = np.random.default_rng(ncols)
    logits[4, :ncols] = g.uniform(-80, 80, ncols).astype(np.float32)      # the whole range in one row
    logits[5, :ncols] = g.normal(0, 1, ncols).astype(np.float32)
    target = [0, ncols - 1, ncols - 1, ncols // 2, int(np.argmax(logits[4, :ncols])), ncols - 1]   # (results stay below 64)
    got, _ = _check(logits, ld, None, list(range(6)), target, ncols)
    for m in (0, 1, 3):
        assert abs(float(got[m]) - np.log(ncols)) <= TOL
    assert abs(float(got[2]) - (1.75 + np.log1p(np.exp(-1.75)))) <= TOL   # log(e^1.5 + e^-0.25) + 0.25
    # the -inf columns as targets: +inf, as the reference's F.cross_entropy gives
    assert np.isposinf(_call(logits, ld, None, [0, 0, 0, 0, 0, 0], ncols)[0][2])


@pytest.mark.parametrize("ncols,ld", [(33, 36), (1027, 1027), (16384, 16384)])
def test_token_nll_targets_outside_the_row_give_nan(ncols, ld):
    logits, listed, target = _case(6, ncols, ld, seed=11)
    good = _check(logits, ld, None, listed, target, ncols)[0]
    bad = np.array(target)
    bad[1], bad[4] = -1, ncols
    got, mean = _call(logits, ld, None, bad, ncols)
    assert np.isnan(got[1]) and np.isnan(got[4]) and np.isnan(mean)
    keep = [0, 2, 3, 5]
    assert np.array_equal(got[keep], good[keep]), "the rows beside a bad target changed"


def test_token_nll_same_bits_on_every_run():
    for ncols, ld in ((1024, 1024), (1027, 1027), (16384, 16384)):
        logits, listed, target = _case(7, ncols, ld, seed=5)
        a, ma = _call(logits, ld, None, target, ncols)
        b, mb = _call(logits, ld, None, target, ncols)
        assert a.tobytes() == b.tobytes() and ma.tobytes() == mb.tobytes()


def test_token_nll_rejects():
    from ccvs_amd import lib, ops
    x = torch.zeros(2, 16388, device="cuda")
    t = torch.zeros(2, dtype=torch.int64, device="cuda")
    with pytest.raises(lib.CcvsError):
        ops.token_nll(x, t)                       # more than 16384 columns: a row no longer fits the registers
    ops.token_nll(x, t, ncols=16384)
    with pytest.raises(lib.CcvsError):
        ops.mean_f32(torch.zeros(3))              # CPU tensor


def test_token_nll_real_head_shape():
    """The full-size GPT head: 2 x 127 teacher-forced rows of 16384 logits through the ops (the logits themselves:
    test_real_geometry_gpu.py)."""
    from ccvs_amd import ops
    g = torch.Generator().manual_seed(6)
    logits = torch.randn(2 * 127, 16384, generator=g) * 3
    target = torch.randint(0, 16384, (2 * 127,), generator=g)
    nll = ops.token_nll(logits.cuda(), target.cuda())
    mean = ops.mean_f32(nll)
    x = logits.double()
    want = torch.logsumexp(x, dim=1) - x[torch.arange(2 * 127), target]
    assert nll.shape == (254,) and mean.dim() == 0 and mean.dtype == torch.float32
    assert (nll.cpu().double() - want).abs().max().item() <= TOL
    assert abs(mean.item() - want.mean().item()) <= TOL

"""-m gpu: the three reductions behind the frame autoencoder's validation figures, at op level against float64 on the CPU
(tests/aeval_ref.py).  The C entry points are called on buffers the test owns: every output and workspace is pre-filled with NaN
(`counts` with garbage), inputs and outputs are followed by NaN guard regions.

  ccvs_l1_mean          n in {1, 3, 1023, 1024, 1025, 4097} and 40001 (three stage-1 partials), both views offset by one element
                        (the 4-byte path), one NaN element; within 2^-22 relative of float64 (one rounding to fp32; the float64
                        accumulation error is orders below it); two runs give the same bits.
  ccvs_vq_stats         (N, C, HW, n_e) in {(1,1,1,24), (3,2,100,50), (2,16,64,32), (5,512,64,1024), (1,8,257,16384)}, with and
                        without row_scale: counts == np.bincount exactly (whatever `counts` held before), the mean within 2^-22
                        relative; an index n_e and an index -1 are not counted, make the mean NaN and touch no guard.
  ccvs_code_perplexity  uniform counts over 24 / 1024 / 16384 codes, one code only, random histograms with empty bins; within
                        4 * 2^-24 relative of the float64 formula, its + 1e-10 included.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import aeval_ref as A  # noqa: E402

pytestmark = pytest.mark.gpu

REL = 2.0 ** -22
GUARD = 64
NAN = float("nan")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(values, offset=0):
    """`values` (fp32 numpy) on the device at element `offset` of a NaN-filled buffer with GUARD NaNs behind it: (view, buffer)."""
    n = values.size
    buf = torch.full((offset + n + GUARD,), NAN, dtype=torch.float32, device="cuda")
    buf[offset:offset + n] = torch.from_numpy(np.ascontiguousarray(values).reshape(-1)).cuda()
    return buf[offset:offset + n], buf


def _guard_intact(buf, offset, n):
    return bool(torch.isnan(buf[:offset]).all() and torch.isnan(buf[offset + n:]).all())


# ---------------------------------------------------------------------------------------------------------------- l1_mean
def _l1(a, b, offset=0):
    """ccvs_l1_mean on guarded copies of a, b at element `offset`: (fp32 result, number of stage-1 partials)."""
    from ccvs_amd import lib
    L = lib.load()
    da, bufa = _guarded(a, offset)
    db, bufb = _guarded(b, offset)
    n = a.size
    ws_bytes = int(L.ccvs_l1_workspace_bytes(n))
    assert ws_bytes % 8 == 0 and ws_bytes >= 8
    ws = torch.full((ws_bytes // 8 + 2,), NAN, dtype=torch.float64, device="cuda")
    out = torch.full((3,), NAN, dtype=torch.float32, device="cuda")
    lib.check(L.ccvs_l1_mean(_ptr(da), _ptr(db), _ptr(out[1:]), _ptr(ws), n, _stream()), "ccvs_l1_mean")
    o = out.cpu().numpy()
    assert np.isnan(o[0]) and np.isnan(o[2]), "a write outside the output"
    w = ws.cpu().numpy()
    assert np.isnan(w[-2:]).all(), "a write behind the workspace"
    assert _guard_intact(bufa, offset, n) and _guard_intact(bufb, offset, n)
    return o[1], ws_bytes // 8


def _pair(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)


@pytest.mark.parametrize("n", [1, 3, 1023, 1024, 1025, 4097, 40001])
def test_l1_mean_against_float64(n):
    from ccvs_amd import ops
    a, b = _pair(n, n)
    want = A.l1_mean64(a, b)
    got, parts = _l1(a, b)
    print(f"n {n}: {got!r} / {want!r} rel {abs(float(got) - want) / want:.2e}, {parts} partial(s)")
    assert got.dtype == np.float32 and abs(float(got) - want) <= REL * want
    assert parts == (3 if n == 40001 else 1)
    again, _ = _l1(a, b)
    assert again.tobytes() == got.tobytes(), "two runs differ"
    # the op: a 0-dim fp32 device tensor with the same bits
    res = ops.l1_mean(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    assert res.is_cuda and res.dim() == 0 and res.dtype == torch.float32 and res.cpu().numpy().tobytes() == got.tobytes()


@pytest.mark.parametrize("n", [4097, 40001])
def test_l1_mean_unaligned_views(n):
    a, b = _pair(n, 7 + n)
    want = A.l1_mean64(a, b)
    got, _ = _l1(a, b, offset=1)       # both bases 4 bytes past a 16-byte boundary: element loads
    assert abs(float(got) - want) <= REL * want
    assert _l1(a, b, offset=1)[0].tobytes() == got.tobytes()


def test_l1_mean_nan_and_zero():
    a, b = _pair(40001, 3)
    assert _l1(a, a.copy())[0] == 0.0
    for at in (0, 20000, 40000):       # first quad, a middle workgroup, the tail behind the last whole quad
        c = a.copy()
        c[at] = np.nan
        assert np.isnan(_l1(c, b)[0]) and np.isnan(_l1(b, c)[0])


# ---------------------------------------------------------------------------------------------------------------- vq_stats
SHAPES = [(1, 1, 1, 24), (3, 2, 100, 50), (2, 16, 64, 32), (5, 512, 64, 1024), (1, 8, 257, 16384)]


def _vq_inputs(N, C, HW, n_e, seed):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((N, C, HW)).astype(np.float32)
    cb = rng.standard_normal((n_e, C)).astype(np.float32)
    idx = rng.integers(0, n_e, size=N * HW).astype(np.int64)
    scale = (0.5 + rng.random(n_e)).astype(np.float32)
    return z, idx, cb, scale


def _vq(z, idx, cb, scale, fill=7):
    """ccvs_vq_stats on guarded buffers, `counts` pre-filled with `fill`: (fp32 mean, counts)."""
    from ccvs_amd import lib
    L = lib.load()
    N, C, HW = z.shape
    n_e = cb.shape[0]
    dz, bufz = _guarded(z)
    dcb, bufcb = _guarded(cb)
    dsc, bufsc = _guarded(scale) if scale is not None else (None, None)
    didx = torch.from_numpy(idx).cuda()
    cbuf = torch.full((n_e + GUARD,), NAN, dtype=torch.float32, device="cuda")   # int32 counts in front of a NaN guard
    counts = cbuf[:n_e].view(torch.int32)
    counts.fill_(fill)
    ws_bytes = int(L.ccvs_vq_stats_workspace_bytes(N, C, HW))
    assert ws_bytes == 8 * (-(-N * HW // 64)) * (-(-C // 64))
    ws = torch.full((ws_bytes // 8 + 2,), NAN, dtype=torch.float64, device="cuda")
    out = torch.full((3,), NAN, dtype=torch.float32, device="cuda")
    lib.check(L.ccvs_vq_stats(_ptr(dz), _ptr(didx), _ptr(dcb), _ptr(dsc) if dsc is not None else ctypes.c_void_p(0), _ptr(out[1:]),
                              _ptr(counts), _ptr(ws), N, C, HW, n_e, _stream()), "ccvs_vq_stats")
    o = out.cpu().numpy()
    assert np.isnan(o[0]) and np.isnan(o[2]), "a write outside the output"
    assert np.isnan(ws.cpu().numpy()[-2:]).all(), "a write behind the workspace"
    assert bool(torch.isnan(cbuf[n_e:]).all()), "a write behind counts"
    assert _guard_intact(bufz, 0, z.size) and _guard_intact(bufcb, 0, cb.size)
    return o[1], counts.cpu().numpy()


@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_vq_stats_against_float64(shape, with_scale):
    from ccvs_amd import ops
    N, C, HW, n_e = shape
    z, idx, cb, scale = _vq_inputs(*shape, seed=sum(shape))
    scale = scale if with_scale else None
    want, want_counts = A.vq_stats64(z, idx, cb, scale)
    got, counts = _vq(z, idx, cb, scale)
    print(f"{shape} scale {with_scale}: mean {got!r} / {want!r} rel {abs(float(got) - want) / want:.2e}")
    assert np.array_equal(counts, want_counts) and counts.dtype == np.int32
    assert abs(float(got) - want) <= REL * want
    again, counts2 = _vq(z, idx, cb, scale, fill=-123456)
    assert again.tobytes() == got.tobytes() and np.array_equal(counts2, want_counts)
    # the op: device tensors with the same bits
    m, c = ops.vq_stats(torch.from_numpy(z).cuda().view(N, C, HW, 1), torch.from_numpy(idx).cuda(), torch.from_numpy(cb).cuda(),
                        None if scale is None else torch.from_numpy(scale).cuda())
    assert m.is_cuda and m.dim() == 0 and m.dtype == torch.float32 and m.cpu().numpy().tobytes() == got.tobytes()
    assert c.dtype == torch.int32 and c.shape == (n_e,) and np.array_equal(c.cpu().numpy(), want_counts)


def test_vq_stats_unaligned_codebook():
    """A codebook whose base is not 16-byte aligned takes the entry-by-entry gather."""
    from ccvs_amd import lib
    L = lib.load()
    N, C, HW, n_e = 2, 16, 64, 32
    z, idx, cb, _ = _vq_inputs(N, C, HW, n_e, seed=5)
    want, want_counts = A.vq_stats64(z, idx, cb)
    dcb, _ = _guarded(cb, offset=1)
    dz, didx = torch.from_numpy(z).cuda(), torch.from_numpy(idx).cuda()
    counts = torch.full((n_e,), 7, dtype=torch.int32, device="cuda")
    ws = torch.full((int(L.ccvs_vq_stats_workspace_bytes(N, C, HW)) // 8,), NAN, dtype=torch.float64, device="cuda")
    out = torch.full((1,), NAN, dtype=torch.float32, device="cuda")
    lib.check(L.ccvs_vq_stats(_ptr(dz), _ptr(didx), _ptr(dcb), ctypes.c_void_p(0), _ptr(out), _ptr(counts), _ptr(ws), N, C, HW, n_e,
                              _stream()), "ccvs_vq_stats")
    assert abs(out.item() - want) <= REL * want and np.array_equal(counts.cpu().numpy(), want_counts)


@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("shape", [(3, 2, 100, 50), (2, 16, 64, 32), (1, 8, 257, 16384)], ids=lambda s: "x".join(map(str, s)))
def test_vq_stats_indices_outside_the_codebook(shape, with_scale):
    N, C, HW, n_e = shape
    z, idx, cb, scale = _vq_inputs(*shape, seed=11 + sum(shape))
    idx[3], idx[-2] = n_e, -1
    want, want_counts = A.vq_stats64(z, idx, cb, scale if with_scale else None)
    assert np.isnan(want) and want_counts.sum() == idx.size - 2
    got, counts = _vq(z, idx, cb, scale if with_scale else None)      # (the guards behind counts, z and the codebook are checked inside)
    assert np.isnan(got) and np.array_equal(counts, want_counts)


# ---------------------------------------------------------------------------------------------------------------- code_perplexity
def _perplexity(counts, total):
    from ccvs_amd import lib, ops
    out = torch.full((3,), NAN, dtype=torch.float32, device="cuda")
    d = torch.from_numpy(np.asarray(counts, dtype=np.int32)).cuda()
    lib.check(lib.load().ccvs_code_perplexity(_ptr(d), d.numel(), int(total), _ptr(out[1:]), _stream()), "ccvs_code_perplexity")
    o = out.cpu().numpy()
    assert np.isnan(o[0]) and np.isnan(o[2])
    res = ops.code_perplexity(d, total)
    assert res.is_cuda and res.dim() == 0 and res.dtype == torch.float32 and res.cpu().numpy().tobytes() == o[1].tobytes()
    return float(o[1])


def _histograms():
    rng = np.random.default_rng(9)
    cases = {f"uniform{n}": np.full(n, 3) for n in (24, 1024, 16384)}
    one = np.zeros(1024, dtype=np.int64)
    one[5] = 100
    cases["one_code"] = one
    for n in (50, 1024, 16384):
        h = rng.integers(0, 40, size=n)
        h[rng.random(n) < 0.7] = 0          # most bins empty
        h[n // 2] += 1                      # (never all of them)
        cases[f"random{n}"] = h
    return cases


@pytest.mark.parametrize("name", list(_histograms()))
def test_code_perplexity_against_float64(name):
    counts = _histograms()[name]
    total = int(counts.sum())
    want = A.perplexity64(counts, total)
    got = _perplexity(counts, total)
    print(f"{name}: {got!r} / {want!r} rel {abs(got - want) / want:.2e}")
    assert abs(got - want) <= 4 * 2.0 ** -24 * want
    if name.startswith("uniform"):
        assert abs(got - counts.size) <= 1e-5 * counts.size
    if name == "one_code":
        assert abs(got - 1.0) <= 1e-6

"""-m gpu: the 7x7 cost volume against the REFERENCE'S OWN correlation kernel.

The reference keeps this op only as GPU kernel text (modules/correlation.py:11-100); `oracle/build_ref_correlation.py` compiles
that text unchanged into `oracle/_ref/libccvs_ref_correlation.so` and `oracle/ref_correlation.py` launches it as the reference's
`_FunctionCorrelation.forward` does.  These tests fail (never skip) when that library is missing.

One bound everywhere.  With `exact` the float64 result and S = sum_c |a_c b_c| / C (both from `O.correlation` in float64), every
float32 result satisfies |got - exact| <= (C + 4) 2^-24 S + 1e-30; leaky_relu(0.1) is 1-Lipschitz, so the same bound holds after
it.  Where S = 0 (every sample in the zero padding) the result must be exactly 0.

  1. `O.correlation` (float64), `ref_harness.correlation_bruteforce` (float64) and the fixtures `corr/s1`, `corr/s2` of ops.npz
     against the reference kernel; the reference kernel is deterministic.
  2. Every launch form of `ccvs_correlation7x7` (one- and two-pixel tiles, strides 1 and 2, channel tails, first_div, lrelu)
     against the reference kernel and float64; the two-pixel form bit-equal to the one-pixel form (CCVS_CORR_PAIR=0 in a
     child process); nothing outside the output written.
  3. Every call the decoder makes for one BAIR 256^2 frame and one Kinetics 64^2 frame, recorded and replayed on the reference.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ccvs_oracle as O
from oracle import ref_correlation as R

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import ref_harness as rh  # noqa: E402  (importing it loads nothing)
from corr_form_worker import FORM_CASES, STRIDES, form_inputs, run_forms  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def ref_lib():
    return R.load()   # raises, naming build(), when oracle/_ref/ holds no library


def exact_and_scale(first, second, s):
    """float64 result and S of the bound, on the GPU."""
    a, b = first.double(), second.double()
    return O.correlation(a, b, s), O.correlation(a.abs(), b.abs(), s)


def check(got, exact, scale, c, what, lrelu=False):
    got = got.double().to(exact.device)
    want = F.leaky_relu(exact, 0.1) if lrelu else exact
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    tol = (c + 4) * U * scale + 1e-30
    err = (got - want).abs()
    bad = ~(err <= tol) | ((scale == 0) & (got != 0))
    if bad.any():
        idx = tuple(int(i) for i in bad.nonzero()[0])
        worst = float((err / tol).max())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first at {idx}: "
                             f"got {float(got[idx])!r}, float64 {float(want[idx])!r}, bound {float(tol[idx]):.3e}; "
                             f"worst err/bound {worst:.3g}")


def rand_pair(n, c, h, w, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    first = torch.randn(n, c, h, w, generator=g, device="cuda") * 0.9 + 0.2
    second = torch.randn(n, c, h, w, generator=g, device="cuda") * 1.1 - 0.1
    return first, second


def launch_form(wo):
    """The dispatch rule of ccvs_correlation7x7 (flow.hip) with the default CCVS_CORR_PAIR."""
    return "x2 (8x64, two pixels per lane)" if wo % 2 == 0 and wo >= 64 else "x1 (8x32)"


# ------------------------------------------------------------------ 1. the oracle and both stand-ins vs the reference kernel
ORACLE_C = (1, 3, 8, 9, 24, 31, 32, 33, 48, 96, 130)
ORACLE_HW = ((1, 1), (3, 5), (7, 7), (9, 11), (33, 17), (40, 70), (64, 130), (127, 129), (128, 256))
BRUTE_MAX = 400_000   # C*H*W up to which the CPU brute force runs every channel count; above it only C in BRUTE_BIG
BRUTE_BIG = (3, 33)


@pytest.mark.parametrize("s", (1, 2))
@pytest.mark.parametrize("hw", ORACLE_HW, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_oracle_and_bruteforce_vs_reference_kernel(hw, s):
    h, w = hw
    for c in ORACLE_C:
        first, second = rand_pair(2, c, h, w, seed=c * 7919 + h * 131 + w + 17 * s)   # two different images per batch entry
        ref = R.ref_correlation(first, second, s)
        exact, scale = exact_and_scale(first, second, s)
        what = f"C={c} {h}x{w} s={s}"
        check(ref, exact, scale, c, "reference kernel vs O.correlation(float64) " + what)
        if c * h * w <= BRUTE_MAX or c in BRUTE_BIG:
            brute = rh.correlation_bruteforce(first.double().cpu(), second.double().cpu(), s)
            check(ref, brute.cuda(), scale, c, "reference kernel vs correlation_bruteforce(float64) " + what)


def test_reference_kernel_reproduces_golden_and_is_deterministic(golden_dir):
    gold = np.load(os.path.join(golden_dir, "ops.npz"))
    a, b = torch.from_numpy(gold["corr/a"]).cuda(), torch.from_numpy(gold["corr/b"]).cuda()
    c = a.shape[1]
    for s in (1, 2):
        ref = R.ref_correlation(a, b, s)
        _, scale = exact_and_scale(a, b, s)
        check(ref, torch.from_numpy(gold[f"corr/s{s}"]).double().cuda(), scale, c, f"reference kernel vs ops.npz corr/s{s}")
    for s in (1, 2):
        first, second = rand_pair(2, 130, 64, 130, seed=5 + s)
        r1 = R.ref_correlation(first, second, s)
        r2 = R.ref_correlation(first, second, s)
        assert torch.equal(r1, r2), f"reference kernel not deterministic at s={s}"


# ------------------------------------------------------------------ 2. every launch form of the product kernel
def _form_check(i, case, s, lrelu, got):
    c, h, w, div = case
    first, second = (t.cuda() for t in form_inputs(i, case))
    rep = first.repeat_interleave(div, 0)
    ref = R.ref_correlation(rep, second, s)
    exact, scale = exact_and_scale(rep, second, s)
    what = f"C={c} {h}x{w} s={s} first_div={div} lrelu={lrelu} Wo={-(-w // s)} form {launch_form(-(-w // s))}"
    check(got, exact, scale, c, "ccvs_correlation7x7 vs float64 " + what, lrelu=lrelu)
    check(F.leaky_relu(ref, 0.1) if lrelu else ref, exact, scale, c, "reference kernel vs float64 " + what, lrelu=lrelu)
    ref_l = F.leaky_relu(ref, 0.1) if lrelu else ref
    tol = 2 * (c + 4) * U * scale + 1e-30
    assert ((got.double() - ref_l.double()).abs() <= tol).all(), "ccvs_correlation7x7 vs reference kernel " + what


def test_every_launch_form_vs_reference_kernel():
    got = run_forms()
    forms = {(s, launch_form(-(-case[2] // s))) for case in FORM_CASES for s in STRIDES}
    assert len(forms) == 4, forms   # both tile forms at both strides
    for i, case in enumerate(FORM_CASES):
        for s in STRIDES:
            for lrelu in (False, True):
                _form_check(i, case, s, lrelu, got[f"{i}_s{s}_l{int(lrelu)}"])


def test_pair_form_bits_equal_single_pixel_form(tmp_path):
    """The two-pixel form adds the channels in the one-pixel form's order (flow.hip): the same bits.  The library reads
    CCVS_CORR_PAIR once per process, so tests/corr_form_worker.py runs every case with it off in a child process."""
    path = str(tmp_path / "corr_single.npz")
    env = dict(os.environ, CCVS_CORR_PAIR="0")
    subprocess.run([sys.executable, os.path.join(HERE, "corr_form_worker.py"), path], env=env, check=True, timeout=300)
    single = np.load(path)
    got = run_forms()
    assert sorted(single.files) == sorted(got)
    n_pair, differ = 0, []
    for i, case in enumerate(FORM_CASES):
        c, h, w, div = case
        first, second = (t.cuda() for t in form_inputs(i, case))
        for s in STRIDES:
            wo = -(-w // s)
            n_pair += 2 * (wo % 2 == 0 and wo >= 64)
            exact, scale = exact_and_scale(first.repeat_interleave(div, 0), second, s)
            for lrelu in (0, 1):
                key = f"{i}_s{s}_l{lrelu}"
                one = torch.from_numpy(single[key])
                check(one, exact, scale, c, f"CCVS_CORR_PAIR=0 {key} C={c} {h}x{w} s={s}", lrelu=bool(lrelu))
                a, b = got[key].cpu(), one
                if a.numpy().tobytes() != b.numpy().tobytes():
                    ne = (a.view(torch.int32) != b.view(torch.int32))
                    idx = tuple(int(j) for j in ne.nonzero()[0])
                    differ.append(f"{key} (C, H, W, div = {case}, form {launch_form(wo)}): {int(ne.sum())} of {ne.numel()} differ, "
                                  f"max |diff| {float((a - b).abs().max()):.3e}, first at {idx}: {float(a[idx])!r} vs {float(b[idx])!r}")
    assert not differ, "default and CCVS_CORR_PAIR=0 differ:\n" + "\n".join(differ)
    assert n_pair >= 12, n_pair


@pytest.mark.parametrize("s,c,h,w,div", [(2, 9, 17, 256, 3), (1, 7, 15, 65, 2), (1, 17, 9, 128, 1), (2, 33, 14, 125, 15)])
def test_correlation_c_abi_writes_only_its_output(s, c, h, w, div):
    """ccvs_correlation7x7 into a NaN-filled buffer larger than the output, at an offset: the output equals ops.correlation7x7's
    and not one element outside it is written."""
    from ccvs_amd import lib, ops
    n = 2 * div
    g = torch.Generator(device="cuda").manual_seed(s * 100 + c)
    first = torch.randn(n // div, c, h, w, generator=g, device="cuda")
    second = torch.randn(n, c, h, w, generator=g, device="cuda")
    ho, wo = -(-h // s), -(-w // s)
    size, off = n * 49 * ho * wo, 97
    buf = torch.full((off + size + 131,), float("nan"), device="cuda")
    lib.check(lib.load().ccvs_correlation7x7(ops._p(first), ops._p(second), ctypes.c_void_p(buf.data_ptr() + 4 * off), n, c, h, w,
                                             s, div, 1, ops._stream()), "ccvs_correlation7x7")
    want = ops.correlation7x7(first, second, s, first_div=div, lrelu=True)
    assert torch.equal(buf[off:off + size].view(n, 49, ho, wo), want), launch_form(wo)
    assert torch.isnan(buf[:off]).all() and torch.isnan(buf[off + size:]).all(), f"written outside the output ({launch_form(wo)})"
    exact, scale = exact_and_scale(first.repeat_interleave(div, 0), second, s)
    check(want, exact, scale, c, f"C={c} {h}x{w} s={s}", lrelu=True)


# ------------------------------------------------------------------ 3. every call the decoder makes
def _record_calls(monkeypatch):
    from ccvs_amd import ops
    calls, real = [], ops.correlation7x7

    def wrapped(first, second, stride, first_div=1, lrelu=False):
        out = real(first, second, stride, first_div=first_div, lrelu=lrelu)
        calls.append((first.detach().clone(), second.detach().clone(), int(stride), int(first_div), bool(lrelu), out.clone()))
        return out

    monkeypatch.setattr(ops, "correlation7x7", wrapped)
    return calls


def _replay(calls, name):
    for j, (first, second, s, div, lrelu, got) in enumerate(calls):
        n, c, h, w = second.shape
        rep = first.repeat_interleave(div, 0)
        ref = R.ref_correlation(rep, second, s)
        exact, scale = exact_and_scale(rep, second, s)
        wo = -(-w // s)
        print(f"{name} call {j}: first {tuple(first.shape)} second {tuple(second.shape)} stride {s} first_div {div} lrelu {lrelu}"
              f" -> {tuple(got.shape)}, form {launch_form(wo)}<{s}>")
        what = f"{name} call {j} (C={c} {h}x{w} s={s} div={div})"
        check(got, exact, scale, c, "decoder's correlation vs float64 " + what, lrelu=lrelu)
        check(F.leaky_relu(ref, 0.1) if lrelu else ref, exact, scale, c, "reference kernel vs float64 " + what, lrelu=lrelu)


def _corr_blocks(net_g):
    return sum(1 for ib in net_g.inter_blocks if ib.matching.use_corr)


def _decode_frame(argv, vid, k, monkeypatch):
    from ccvs_amd.models.skip_vid_generator.models.quantized_video_model import QVidModel
    from ccvs_amd.tools.options import Options
    opt = Options().parse(load_qvid_generator=True, load_transformer=True, argv=list(argv))
    torch.manual_seed(0)
    qv = QVidModel(opt["qvid_generator"], is_train=False, is_main=True).eval()
    enc = qv({"vid": vid.clone()}, mode="vid_encoder")
    ctx = [[f[:, j:j + 1] for f in enc["inter"]] for j in range(k)]
    calls = _record_calls(monkeypatch)
    with torch.no_grad():
        qv.net_g(enc["z"][:, k:k + 1].contiguous(), ctx, return_all=True, inter_pre_warping=False)
    torch.cuda.synchronize()
    monkeypatch.undo()
    return qv, calls


def test_bair_decoder_frame_correlations_vs_reference_kernel(monkeypatch):
    """BAIR 256^2, B = 1, 3 contexts: one frame through the eager decoder; every cost volume it builds (the finer levels at stride
    2) replayed on the reference kernel."""
    from ccvs_amd.tools.options import BAIR_ARGV
    vid = torch.rand(1, 4, 3, 256, 256, generator=torch.Generator().manual_seed(1)) * 2 - 1
    qv, calls = _decode_frame(BAIR_ARGV, vid, 3, monkeypatch)
    assert len(calls) == _corr_blocks(qv.net_g) >= 4, len(calls)
    assert {c[2] for c in calls} == {1, 2}, [c[2] for c in calls]
    assert all(c[3] == 3 and c[4] for c in calls)
    _replay(calls, "BAIR")


def test_kinetics_decoder_frame_correlations_vs_reference_kernel(monkeypatch):
    """Kinetics 64^2, B = 2, all 8 contexts of the ring: every cost volume of one decoder frame replayed on the reference kernel."""
    from ccvs_amd.tools.options import KINETICS_ARGV
    vid = torch.rand(2, 9, 3, 64, 64, generator=torch.Generator().manual_seed(1)) * 2 - 1
    qv, calls = _decode_frame(KINETICS_ARGV, vid, 8, monkeypatch)
    assert len(calls) == _corr_blocks(qv.net_g) >= 4, len(calls)
    assert all(c[3] == 8 and c[4] for c in calls)
    _replay(calls, "Kinetics")

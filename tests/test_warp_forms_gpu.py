"""-m gpu: every instantiation of the flow decoder's gather kernels (flow.hip) through `ops.backwarp`, `ops.backwarp_p8`,
`ops.backwarp_proj` and `ops.warp_fuse_blend`, against the float64 mirror and the derived per-element bound of tests/warp_ref.py
(what the bound can and cannot tell apart is tests/test_warp_ref_host.py, on the same tensors).

  launch forms   9 x 13 (W % 4 != 0: one pixel per lane), 12 x 20 (four pixels, plain order), 16 x 64 (four pixels, 64 x 16 tiles);
                 the guard `expect` pins the instantiation each case must select, `warp_ref.launched` restates the launchers'
                 conditions: backwarp_kernel<1|4>, backwarp_p8_kernel, warp_proj_kernel<16|24|48|96>, warp_proj4_kernel<16|24>,
                 warp_fuse_blend_kernel, warp_fuse_blend4_kernel -- 15 with the plain and tiled orders counted separately.
  shapes         2 frames; 10 channels (a ragged chunk for 16 and for 8 channels per thread); k = 1, 2 and CCVS_MAX_CTX contexts
                 for the fusion / blend, 2 otherwise; 40 -> 10 (padded to 16), 24, 48, 96 channels for warp + projection;
                 8 and 24 channels for the packed back-warp.
  operands       every context is a channel slice of its own NaN-filled buffer with its own batch stride; outputs are channel
                 slices (back-warp, fusion / blend), the middle rows (projection) or the middle (packed) of NaN-filled buffers,
                 and what lies outside must still be NaN afterwards.
  value regimes  noise (flows randn * 4, mult 1/2: the regime of the older tests, the baseline of the ratios); lattice (every pair
                 of -2.5, -1, -1 + 2^-10, -1/2, 0, 2, 2.25, n - 1, n - 1/2, n - 2^-10, n, n + 1.5 in x and y, sources randn + 2,
                 mult 1 and mult 1/2 with doubled flows); far (rows and a block at +-(W + 5), +-300, +-1e4, +-1e9: exact zeros, and
                 lrelu(bias) exactly after the projection; finite flows only -- the reference's result for a non-finite
                 coordinate is not defined and nothing is asserted about it); large (smooth +-0.4 W inside the image, sources
                 x 50: where delta_pos x G is largest); saturated (fusion / blend: occlusion logits of +-100, +-30, +-12: finite
                 everywhere, and `dec` to within the bound where every context is at >= +30).

Every element is asserted |got - mirror| <= bound; the largest err / bound of each case is printed.

Measured on an MI355X, largest err / bound over all cases of this file (records, not thresholds):
  backwarp_kernel<1> 0.12, <4> plain 0.18, tiled 0.16 (noise 0.15, lattice 0.09, far 0.18, large 0.10);
  warp_proj_kernel<16|24|48|96> 0.028 / 0.033 / 0.049 / 0.056, warp_proj4_kernel<16> 0.047 plain, 0.049 tiled, <24> 0.036, 0.044;
  warp_fuse_blend_kernel 0.48, warp_fuse_blend4_kernel 0.51 plain, 0.57 tiled (all three at saturated, k = 1: one rounding of
  sigmoid next to 1; noise 0.37, lattice 0.38, far 0.40, large 0.14); backwarp_p8_kernel: no bit differs.
  The reference's own fp32 arithmetic on a CPU: back-warp 0.15, projection 0.056, fusion / blend 0.57."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 64                    # floats in front of and behind the packed back-warp's buffer (keeps its 16-byte alignment)
WORST = {}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ccvs_amd import ops as _ops
    yield _ops
    for name in sorted(WORST):
        print(f"worst err / bound  {name:34s} {WORST[name]:.4f}")


def expect(op, form, cout=None):
    """The instantiation a case of this file must launch; fails when a dispatch rule (or the default pixel order) has moved."""
    h, w = R.FORMS[form]
    order = {"quad": "[plain]", "tiled": "[tiled]"}.get(form)
    if op == "backwarp":
        want = "backwarp_kernel<1>" if form == "one" else "backwarp_kernel<4>" + order
    elif op == "backwarp_p8":
        want = "backwarp_p8_kernel"
    elif op == "fuse_blend":
        want = "warp_fuse_blend_kernel" if form == "one" else "warp_fuse_blend4_kernel" + order
    else:
        pad = {10: 16, 24: 24, 48: 48, 96: 96}[cout]
        want = f"warp_proj_kernel<{pad}>" if form == "one" or pad > 24 else f"warp_proj4_kernel<{pad}>" + order
    got = R.launched(op, h, w, cout=cout)
    assert got == want, f"{op} at {h} x {w} launches {got}, this case is here for {want}"
    return want


def ctx_views(ctxs):
    """Each context as the channel slice [1 : 1 + C] of its own NaN-filled buffer of C + 2 + j channels: k different batch strides."""
    views = []
    for j, t in enumerate(ctxs):
        nf, c, h, w = t.shape
        buf = torch.full((nf, c + 2 + j, h, w), NAN, device="cuda")
        view = buf[:, 1:1 + c]
        view.copy_(t)
        assert view.stride() == ((c + 2 + j) * h * w, h * w, w, 1)
        views.append(view)
    return views


def channel_slice(n, c, h, w, fill=None):
    whole = torch.full((n, c + 5, h, w), NAN, device="cuda")
    view = whole[:, 3:3 + c]
    if fill is not None:
        view.copy_(fill)
    return whole, view


def untouched(whole, view, what):
    assert not torch.isnan(view).any(), f"{what}: {int(torch.isnan(view).sum())} of {view.numel()} outputs are NaN"
    assert int(torch.isnan(whole).sum()) == whole.numel() - view.numel(), f"{what}: wrote outside its output view"


def within(kernel, what, got, ref):
    got = got.detach().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    ratio = R.worst_ratio(got, ref["want"], ref["tol"])
    print(f"{kernel} {what}: largest err / bound {ratio:.4f}")
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)
    assert ratio <= 1.0, f"{kernel} {what}: largest err / bound {ratio:.4f}"
    return got


def test_all_instantiations_are_launched():
    got = set()
    for c in R.cases():
        got.add(expect(c.op, c.form, cout=c.var))
    assert got == R.ALL_INSTANTIATIONS and len(got) == 15, sorted(R.ALL_INSTANTIATIONS ^ got)
    assert R.k_values()[-1] == R.max_ctx()


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("form", list(R.FORMS))
def test_backwarp(ops, form, regime):
    case = R.Case("backwarp", form, regime, R.C_WARP)
    kernel = expect("backwarp", form)
    ref = R.reference(case)
    inp = ref["inp"]
    n = R.NF * inp["k"]
    whole, view = channel_slice(n, case.var, inp["H"], inp["W"])
    ops.backwarp(ctx_views(inp["ctxs"]), inp["flow"].cuda(), inp["mult"], out=view)
    untouched(whole, view, f"{kernel} {regime}")
    got = within(kernel, regime, view, ref)
    far = ref["far"].unsqueeze(1).expand_as(got)
    assert bool((got[far] == 0).all()), "a sample far outside the image is not exactly 0"
    if regime in R.ZERO_REGIMES:
        assert far.any()


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("form", list(R.FORMS))
def test_warp_proj(ops, form, regime):
    for cout in (10, 24, 48, 96) if form != "tiled" else (10, 24):
        case = R.Case("warp_proj", form, regime, cout)
        kernel = expect("warp_proj", form, cout=cout)
        ref = R.reference(case)
        inp = ref["inp"]
        n, h, w = R.NF * inp["k"], inp["H"], inp["W"]
        w_t, cpad = ops.pack_proj_weight(inp["weight"].cuda())
        assert f"<{cpad}>" in kernel
        whole = torch.full((n + 2, cout, h, w), NAN, device="cuda")
        view = whole[1:n + 1]
        ops.backwarp_proj(ctx_views(inp["ctxs"]), inp["flow"].cuda(), inp["mult"], w_t, cpad, inp["bias"].cuda(), cout, out=view)
        untouched(whole, view, f"{kernel} {regime}")
        got = within(kernel, f"{regime} Cout {cout}", view, ref)
        far = ref["far"].unsqueeze(1).expand_as(got)
        due = torch.nn.functional.leaky_relu(inp["bias"], 0.1).view(1, -1, 1, 1).expand_as(got)
        assert torch.equal(got[far], due[far]), "far outside the image the projection is not lrelu(bias) exactly"


@pytest.mark.parametrize("regime", R.REGIMES + ("saturated",))
@pytest.mark.parametrize("form", list(R.FORMS))
def test_warp_fuse_blend(ops, form, regime):
    for k in R.k_values():
        case = R.Case("fuse_blend", form, regime, k)
        kernel = expect("fuse_blend", form)
        ref = R.reference(case)
        inp = ref["inp"]
        whole, view = channel_slice(R.NF, R.C_WARP, inp["H"], inp["W"], fill=inp["dec"].cuda())
        ops.warp_fuse_blend(view, ctx_views(inp["ctxs"]), inp["flow"].cuda(), inp["occ"].cuda(), inp["mult"], k)
        untouched(whole, view, f"{kernel} {regime} k {k}")
        got = within(kernel, f"{regime} k {k}", view, ref)
        if regime == "saturated":
            keep = (inp["occ"].view(R.NF, k, 1, inp["H"], inp["W"]) >= 30).all(1).expand_as(got)
            assert keep.any()
            assert bool(((got.double() - inp["dec"].double()).abs()[keep] <= ref["tol"][keep]).all()), "every context occluded: not dec"


def split8(v):
    """`split8` of csrc/common.h on the host: round to nearest even to bf16, then the remainder again."""
    hi = v.to(torch.bfloat16)
    lo = (v - hi.float()).to(torch.bfloat16)
    return hi, lo


def packed(t):
    """fp32 [N,C,H,W] (CPU) -> int16 bit patterns [N, C/8, 2, H, W, 8] of the split-bf16 packed form."""
    n, c, h, w = t.shape
    hi, lo = split8(t)
    units = [p.view(n, c // 8, 8, h, w).permute(0, 1, 3, 4, 2) for p in (hi, lo)]
    return torch.stack(units, dim=2).contiguous().view(torch.int16)


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("form", ["quad", "tiled"])
def test_backwarp_p8(ops, form, regime):
    for c in (8, 24):
        case = R.Case("backwarp_p8", form, regime, c)
        expect("backwarp_p8", form)
        plain = expect("backwarp", form)
        ref = R.reference(case)
        inp = ref["inp"]
        n, h, w = R.NF * inp["k"], inp["H"], inp["W"]
        views = ctx_views(inp["ctxs"])
        fo = torch.cat([inp["flow"], inp["occ"]], dim=1)
        fod = fo.cuda()
        bw = within(plain, f"{regime} C {c}", ops.backwarp(views, fod[:, :2].contiguous(), inp["mult"]), ref)
        numel = n * (c + 8) * h * w
        whole = torch.full((numel + 2 * GUARD,), NAN, device="cuda")
        p8 = ops.backwarp_p8(views, fod, inp["mult"], out=whole[GUARD:GUARD + numel])
        torch.cuda.synchronize()
        assert p8.shape == (n, c + 8, h, w) and p8.data.data_ptr() == whole[GUARD:].data_ptr()
        assert torch.isnan(whole[:GUARD]).all() and torch.isnan(whole[GUARD + numel:]).all(), "wrote outside its buffer"
        got = p8.data.cpu().view(torch.bfloat16).view(n, c // 8 + 1, 2, h, w, 8).view(torch.int16)
        want = packed(torch.cat([bw, fo, torch.zeros(n, 5, h, w)], dim=1))
        assert torch.equal(got[:, :c // 8], want[:, :c // 8]), "hi / lo planes are not the split of ops.backwarp's output"
        assert torch.equal(got[:, c // 8, ..., :3], packed(torch.cat([fo, torch.zeros(n, 5, h, w)], dim=1))[:, 0, ..., :3]), "flow / occlusion"
        assert bool((got[:, c // 8, ..., 3:] == 0).all()), "the five padding channels are not zero"
        WORST["backwarp_p8_kernel (bits differing)"] = 0.0

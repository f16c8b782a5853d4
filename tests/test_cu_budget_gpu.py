"""-m gpu: every launch form that consults the CU budget of its stream (`ccvs_stream_cu_limit`, `limited_grid` in csrc/common.h), at op
level, into memory the test owns and has poisoned.

With a budget the HBM-bound kernels stop being "one workgroup per block": they become `cu_limit x per_cu` persistent workgroups that
stride over the blocks (GRID_WALK_BEGIN, the grid-stride loops).  That form carries code the unbudgeted launch never runs -- the barrier
that guards LDS re-use between two blocks of one workgroup, the `continue` inside the walk, the block -> (bx, by, bz) decomposition,
the quad-pixel tile order under a stride, the ragged last pass.  Every case here

  (a) equals a float64 CPU reference of the operation (oracle/ccvs_oracle.py on .double() inputs, or a plain torch expression) for
      budgets of 1 and 3 CUs, within the tolerance the op's own test uses (tests/test_ops_gpu.py, test_skip_rgb_gpu.py,
      test_stft_decoder_gpu.py, test_deblur_gpu.py);
  (b) equals the unbudgeted launch bit for bit (same side stream, a poisoned buffer of its own; the budgeted launches run first);
  (c) leaves no poison behind: float outputs start as NaN, uint8 outputs as 0x55, a P8Act's data as 0xFF bytes (NaN in both bf16
      halves); what lies outside a channel-slice `out=` view stays poisoned.

A case is valid only if the walk loops: `walks(blocks, per_cu)` mirrors the launcher's block count (a guard on the inputs, not the
thing under test) and asserts at least 2 x per_cu + 1 blocks (three passes with a budget of one CU) and a ragged last pass for one of
the two budgets, so a later change of a tile size fails here instead of silently un-testing the loop.

`limited_grid` call site (kernel) -> case:
  resample.hip  blur4x4_tile_kernel ........ test_upfirdn2d[blur-pad22], [blur-pad11]
                upsample2x2_kernel ......... test_upfirdn2d[upsample2x2]
                upsample2_kernel ........... test_upfirdn2d[upsample2]
                down2_tile_kernel .......... test_upfirdn2d[down2_tile-pad22], [down2_tile-pad11]
                down2_kernel ............... test_upfirdn2d[down2]
                upfirdn2d_generic_kernel ... test_upfirdn2d[generic]
                dwconvT4x4s2_kernel<4 / 2 / 1> .... test_dwconvT[w16], [w18], [w17]
                to_rgb_kernel<64 / 16 / 4> . test_to_rgb[G64*], [G16*], [G4*]
  stft.hip      channel_head_kernel<64 / 16 / 4, 4> ... test_channel_head[G64], [G16], [G4];  <64, 1> ... [G64-px1]
  misc.hip      pack_u8_kernel, pack_u8_norm_kernel ... test_pack_u8
  blur.hip      gaussian_blur_kernel ....... test_gaussian_blur
  flow.hip      correlation7x7_kernel<1 / 2> ... test_correlation[one-s1], [one-s1-div2-lrelu], [one-s2]
                correlation7x7x2_kernel<1 / 2> . test_correlation[pair-s1], [pair-s2]
                backwarp_kernel<1> / <4> (plain, tiled) ......... test_backwarp[*-one], [*-quad], [*-tiled]
                warp_fuse_blend_kernel / warp_fuse_blend4_kernel .... test_warp_fuse_blend[*-one], [*-quad], [*-tiled]
                warp_proj_kernel / warp_proj4_kernel ................ test_backwarp_proj[one], [quad], [tiled]
                backwarp_p8_kernel ......... test_backwarp_p8
                tap_shift_add_kernel<4> / <1> .................. test_conv_heads[*-w4], [*-odd]
The packed-input / packed-output convolutions (chunked 1-D launches under `ccvs_conv_desc.cu_limit`) are the last test."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ccvs_oracle as O

pytestmark = pytest.mark.gpu

F = torch.nn.functional
LIMS = (1, 3)
ULP = 2.0 ** -23
_SIDE = []


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ccvs_amd import ops as _ops
    return _ops


def budgeted(lim, fn):
    """fn() on the module's side stream under a budget of `lim` CUs (0: none), behind everything queued on the current stream."""
    from ccvs_amd import ops as _ops
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream())
    side = _SIDE[0]
    _ops.stream_cu_limit(side, lim)
    try:
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            res = fn()
        torch.cuda.synchronize()
        return res
    finally:
        _ops.stream_cu_limit(side, 0)


def cd(a, b):
    return -(-a // b)


def walks(blocks, per_cu):
    """The guard: a launch of `blocks` blocks whose `limited_grid` has `per_cu` as its third argument loops under the budgets of LIMS."""
    assert blocks >= 2 * per_cu + 1, f"does not loop: {blocks} blocks, {per_cu} workgroups per CU: fewer than three passes with one CU"
    grids = [min(blocks, lim * per_cu) for lim in LIMS]
    assert any(blocks % g for g in grids), f"does not loop raggedly: {blocks} blocks are whole passes of {grids} workgroups"


def poison(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def check(launch, make_out, want, bound, what):
    """launch(view) fills `view`; make_out() -> (the poisoned buffer, the view of it the op writes).  (a), (b), (c) of the module
    docstring for the budgets of LIMS; the budgeted launches run before the unbudgeted one."""
    got = {}
    for lim in LIMS + (0,):
        whole, view = make_out()
        budgeted(lim, lambda: launch(view))
        left = int(torch.isnan(whole).sum())
        assert not torch.isnan(view).any(), f"{what}: budget {lim}: {int(torch.isnan(view).sum())} of {view.numel()} outputs never written"
        assert left == whole.numel() - view.numel(), f"{what}: budget {lim}: wrote outside its output view"
        got[lim] = view
    for lim in LIMS:
        assert torch.equal(got[lim], got[0]), f"{what}: a budget of {lim} CUs changes the result"
        err = (got[lim].cpu().double() - want).abs()
        ratio = float((err / bound).max()) if torch.is_tensor(bound) else float(err.max()) / bound
        print(f"{what}: budget {lim}: max |error| {float(err.max()):.3e}, {ratio:.3f} of the bound")
        assert bool((err <= bound).all()), f"{what}: budget {lim}: max |error| {float(err.max()):.3e}, {ratio:.3f} of the bound"


def dense(*shape):
    def make():
        t = poison(*shape)
        return t, t
    return make


def channel_slice(n, c_all, c0, c, h, w):
    def make():
        t = poison(n, c_all, h, w)
        return t, t[:, c0:c0 + c]
    return make


# ------------------------------------------------------------------ FIR resampling
def fir_launch(shape, up, down, pad):
    """(kernel, blocks) of `ccvs_upfirdn2d` (csrc/resample.hip); per_cu = 8 throughout."""
    n, c, h, w = shape
    nc = n * c
    ho, wo = (h * up + pad[0] + pad[1] - 4) // down + 1, (w * up + pad[0] + pad[1] - 4) // down + 1
    if up == 1 and down == 1:
        return "blur4x4_tile", cd(wo, 64) * cd(ho, 32) * nc
    if up == 2 and down == 1 and pad == (2, 1):
        return ("upsample2x2", cd(nc * h * (w // 2), 256)) if w % 2 == 0 else ("upsample2", cd(nc * h * w, 256))
    if up == 1 and down == 2 and wo >= 32 and ho >= 8:
        return "down2_tile", cd(wo, 64) * cd(ho, 16) * nc
    if up == 1 and down == 2:
        return "down2", cd(nc * ho * cd(wo, 4), 256)
    return "generic", cd(nc * ho * wo, 256)


@pytest.mark.parametrize("kernel,shape,up,down,pad", [
    ("blur4x4_tile", (3, 7, 40, 70), 1, 1, (2, 2)), ("blur4x4_tile", (3, 7, 40, 70), 1, 1, (1, 1)),
    ("upsample2x2", (3, 5, 24, 26), 2, 1, (2, 1)), ("upsample2", (3, 5, 24, 25), 2, 1, (2, 1)),
    ("down2_tile", (2, 5, 40, 132), 1, 2, (2, 2)), ("down2_tile", (2, 5, 40, 132), 1, 2, (1, 1)),
    ("down2", (6, 7, 26, 62), 1, 2, (1, 1)),      # 13 x 31 outputs per plane: below the tile form's 32 columns, a row tail of 3
    ("generic", (3, 5, 24, 25), 2, 2, (2, 1)),
], ids=["blur-pad22", "blur-pad11", "upsample2x2", "upsample2", "down2_tile-pad22", "down2_tile-pad11", "down2", "generic"])
def test_upfirdn2d(ops, kernel, shape, up, down, pad):
    """Tolerance 1e-5, as test_upfirdn2d_oracle; activation, residual and output scale in the epilogue."""
    got_kernel, blocks = fir_launch(shape, up, down, pad)
    assert got_kernel == kernel
    walks(blocks, 8)
    g = torch.Generator().manual_seed(sum(shape) + 10 * up + down + pad[0])
    x = torch.randn(*shape, generator=g)
    ref = O.upfirdn2d(x.double(), O.make_fir_kernel(gain=2.0).double(), up=up, down=down, pad=pad)
    res = torch.randn(ref.shape, generator=g)
    want = (F.leaky_relu(ref, 0.1) + res.double()) * 0.5
    xd, rd = x.cuda(), res.cuda()
    check(lambda out: ops.upfirdn2d(xd, up=up, down=down, pad=pad, gain=2.0, act=True, residual=rd, out_scale=0.5, out=out),
          dense(*ref.shape), want, 1e-5, kernel)


@pytest.mark.parametrize("w,h,sliced", [(16, 12, False), (18, 12, True), (17, 13, False)], ids=["w16", "w18", "w17"])
def test_dwconvT(ops, w, h, sliced):
    """Four, two and one input pixel per thread; one case into a channel slice of a wider tensor.  Tolerance 1e-5, as test_dwconvT."""
    n, c = 10, 9
    per_thread = 4 if w % 4 == 0 else (2 if w % 2 == 0 else 1)
    assert (c * h * w) % 4 == 0 or per_thread != 4      # the four-pixel form also needs a batch stride that is a multiple of 4
    walks(cd(n * c * h * (w // per_thread), 256), 8)
    g = torch.Generator().manual_seed(w)
    x, wt = torch.randn(n, c, h, w, generator=g), torch.randn(c, 1, 4, 4, generator=g)
    want = O.dw_convT_x2(x.double(), wt.double())
    xd, wd = x.cuda(), wt.cuda()
    make = channel_slice(n, c + 5, 3, c, 2 * h, 2 * w) if sliced else dense(n, c, 2 * h, 2 * w)
    check(lambda out: ops.dwconvT4x4s2(xd, wd, out=out), make, want, 1e-5, f"dwconvT x{per_thread}")


# ------------------------------------------------------------------ the channel-group heads
def group_form(items):
    """`to_rgb_form` / `channel_head_form`: (channel groups G, blocks) of a launch of `items` quads / items; per_cu = 8."""
    if cd(items, 64) >= 1024:
        return 4, cd(items, 64)
    if cd(items, 16) >= 256:
        return 16, cd(items, 16)
    return 64, cd(items, 4)


@pytest.mark.parametrize("G,shape,with_skip", [
    (64, (7, 24, 8, 8), False), (64, (7, 24, 8, 8), True), (64, (6, 24, 8, 10), True),
    (16, (4, 16, 64, 64), False), (16, (4, 16, 64, 64), True), (4, (1, 8, 512, 512), False), (4, (1, 8, 512, 512), True),
], ids=["G64", "G64-skip", "G64-skip-w10", "G16", "G16-skip", "G4", "G4-skip"])
def test_to_rgb(ops, G, shape, with_skip):
    """Per-element bound 1e-5 (sum_k |w_k x_k| + |up2(skip)| + 1), as tests/test_skip_rgb_gpu.py; the reference is the plain torch
    expression of ToRGB in float64."""
    n, c, h, w = shape
    got_g, blocks = group_form(n * h * cd(w, 4))
    assert got_g == G
    walks(blocks, 8)
    g = torch.Generator().manual_seed(n + c + h + w + int(with_skip))
    x, wt = torch.randn(n, c, h, w, generator=g), torch.randn(3, c, 1, 1, generator=g)
    b_conv, bias = torch.randn(3, generator=g), torch.randn(1, 3, 1, 1, generator=g)
    skip = torch.randn(n, 3, h // 2, w // 2, generator=g) if with_skip else None
    scale = 1 / math.sqrt(c)
    fir = O.make_fir_kernel(gain=4.0).double()
    want = F.conv2d(x.double(), wt.double() * scale, bias=b_conv.double()) + bias.double()
    mag = F.conv2d(x.double().abs(), wt.double().abs() * scale) + 1.0
    if with_skip:
        want = want + O.upfirdn2d(skip.double(), fir, up=2, pad=(2, 1))
        mag = mag + O.upfirdn2d(skip.double().abs(), fir, up=2, pad=(2, 1))
    xd, w_scaled, bc, bb = x.cuda(), (wt.cuda() * scale).reshape(3, c).contiguous(), b_conv.cuda(), bias.cuda()
    sd = skip.cuda() if with_skip else None
    check(lambda out: ops.to_rgb(xd, w_scaled, bc, bb, skip=sd, out=out), dense(n, 3, h, w), want, 1e-5 * mag, f"to_rgb<{G}>")


@pytest.mark.parametrize("G,shape,flags", [
    (64, (7, 24, 8, 8), (True, True)), (64, (5, 13, 7, 5), (True, False)), (16, (4, 16, 64, 64), (False, False)),
    (4, (1, 8, 512, 512), (True, True)),
], ids=["G64", "G64-px1", "G16", "G4"])
def test_channel_head(ops, G, shape, flags):
    """Per-element bound 1e-5 sum_c |w_c x_c| (+ one fp32 ulp of the result behind the tanh), as tests/test_stft_decoder_gpu.py."""
    n, c, h, w = shape
    px = 4 if (h * w) % 4 == 0 else 1
    got_g, blocks = group_form(n * (h * w // px))
    assert got_g == G
    walks(blocks, 8)
    act, tanh = flags
    g = torch.Generator().manual_seed(n + c + h + w)
    x, wt, bias = torch.randn(n, c, h, w, generator=g), torch.randn(1, c, 1, 1, generator=g), torch.randn(1, generator=g) * 0.1
    scale = 1 / np.sqrt(c)
    terms = (wt * scale).reshape(1, c, 1, 1).double() * x.double()       # the fp32 product, then float64 arithmetic
    want = terms.sum(1, keepdim=True) + bias.double()
    if act:
        want = torch.where(want > 0, want, 0.1 * want)
    if tanh:
        want = torch.tanh(want)
    bound = 1e-5 * terms.abs().sum(1, keepdim=True) + (ULP * want.abs() if tanh else 0.0)
    xd, wd, bd = x.cuda(), wt.cuda(), bias.cuda()
    check(lambda out: ops.channel_head(xd, wd, scale, bd, act=act, tanh=tanh, out=out), dense(n, 1, h, w), want, bound,
          f"channel_head<{G},{px}>")


# ------------------------------------------------------------------ uint8 packs
def test_pack_u8(ops):
    """Byte-exact against the oracle's fp32 expressions, as test_gpt_embed_pack / tests/test_reference_scripts_gpu.py do (a truncation
    has no tolerance); a byte still holding the 0x55 fill where the reference has another value was never written."""
    shape = (3, 3, 3, 37, 41)
    walks(cd(9 * 37 * 41, 256), 8)
    vid = torch.randn(*shape, generator=torch.Generator().manual_seed(7)) * 1.5
    vd = vid.cuda()
    std, mean = (0.229, 0.224, 0.225), (0.485, 0.456, 0.406)
    for name, want, launch in (("pack_u8", O.pack_u8(vid), lambda out: ops.pack_u8(vd, out=out)),
                               ("pack_u8_norm", O.pack_u8_imagenet(vid), lambda out: ops.pack_u8_norm(vd, std, mean, out=out))):
        got = {}
        for lim in LIMS + (0,):
            out = torch.full((3, 3, 37, 41, 3), 0x55, dtype=torch.uint8, device="cuda")
            budgeted(lim, lambda: launch(out))
            got[lim] = out.cpu()
        for lim in LIMS:
            assert torch.equal(got[lim] == 0x55, want == 0x55), f"{name}: budget {lim}: fill bytes left in the output"
            assert torch.equal(got[lim], got[0]), f"{name}: a budget of {lim} CUs changes the result"
            assert torch.equal(got[lim], want), name


# ------------------------------------------------------------------ cost volume
def corr_launch(n, h, w, stride):
    """(form, blocks, per_cu) of `ccvs_correlation7x7` (csrc/flow.hip)."""
    ho, wo = cd(h, stride), cd(w, stride)
    if wo % 2 == 0 and wo >= 64:
        return "pair", cd(wo, 64) * cd(ho, 8) * n, 4
    return "one", cd(wo, 32) * cd(ho, 8) * n, 8 if stride == 1 else 4


@pytest.mark.parametrize("form,shape,stride,div", [
    ("one", (5, 11, 20, 40), 1, 1), ("one", (6, 11, 20, 40), 1, 2), ("one", (5, 11, 36, 70), 2, 1),
    ("pair", (5, 11, 20, 72), 1, 1), ("pair", (5, 11, 36, 132), 2, 1),
], ids=["one-s1", "one-s1-div2-lrelu", "one-s2", "pair-s1", "pair-s2"])
def test_correlation(ops, form, shape, stride, div):
    """C = 11 leaves a channel-chunk tail of 3; tolerance 1e-5, as test_correlation_properties."""
    n, c, h, w = shape
    got_form, blocks, per_cu = corr_launch(n, h, w, stride)
    assert got_form == form
    walks(blocks, per_cu)
    g = torch.Generator().manual_seed(w + stride + div)
    a, b = torch.randn(n // div, c, h, w, generator=g), torch.randn(n, c, h, w, generator=g)
    want = O.correlation(a.repeat_interleave(div, dim=0).double(), b.double(), stride)
    if div > 1:
        want = F.leaky_relu(want, 0.1)
    ad, bd = a.cuda(), b.cuda()
    check(lambda out: ops.correlation7x7(ad, bd, stride, first_div=div, lrelu=div > 1, out=out), dense(*want.shape), want, 1e-5,
          f"correlation {form} s{stride}")


# ------------------------------------------------------------------ warps
WARP_FORMS = {"one": (9, 13), "quad": (32, 36), "tiled": (32, 64)}     # W % 4 != 0; W % 4 == 0, plain order; W % 64 == 0 and H % 16 == 0


def warp_blocks(n, c, h, w, cch4, cch1=16):
    """blocks of the warp launchers' 3-D walk (pixel blocks, channel chunks, images): `launch_backwarp`, `launch_warp_fuse_blend`."""
    if w % 4 == 0:
        return cd(h * w // 4, 256) * cd(c, cch4) * n
    return cd(h * w, 256) * cd(c, cch1) * n


def warp_inputs(nf, k, c, h, w, seed):
    """k contexts [nf, C, H, W] and the flows of the nf k pairs in (frame, context) order: a few pixels, past all four borders."""
    g = torch.Generator().manual_seed(seed)
    ctxs = [torch.randn(nf, c, h, w, generator=g) for _ in range(k)]
    flow = torch.randn(nf * k, 2, h, w, generator=g) * 1.5
    flow[0, :, 0, 0] = 1e4                 # far outside: zeros
    flow[1, 0, :, 0] = -0.25               # only the right tap inside
    flow[1, 0, :, w - 1] = 0.25            # only the left tap inside
    stacked = torch.stack(ctxs, dim=1).reshape(nf * k, c, h, w)
    return ctxs, stacked, flow


@pytest.mark.parametrize("form", ["one", "quad", "tiled"])
@pytest.mark.parametrize("source", ["tensor", "list"])
def test_backwarp(ops, source, form):
    """C = 40: three / five channel chunks in the walk; k = 2 contexts; the tensor form into a channel slice.  Tolerance 1e-4, as
    test_backwarp_oracle."""
    h, w = WARP_FORMS[form]
    nf, k, c, mult = (3, 2, 40, 2.0) if form == "one" else (2, 2, 40, 2.0)
    walks(warp_blocks(nf * k, c, h, w, 8), 8)
    ctxs, stacked, flow = warp_inputs(nf, k, c, h, w, seed=h + w)
    want = O.backwarp(stacked.double(), flow.double() * mult, O.backwarp_grid(h, w).double())
    src = stacked.cuda() if source == "tensor" else [t.cuda() for t in ctxs]
    fd = flow.cuda()
    make = channel_slice(nf * k, c + 4, 2, c, h, w) if source == "tensor" else dense(nf * k, c, h, w)
    check(lambda out: ops.backwarp(src, fd, mult, out=out), make, want, 1e-4, f"backwarp {source} {form}")


@pytest.mark.parametrize("form", ["one", "quad", "tiled"])
@pytest.mark.parametrize("source", ["tensor", "list"])
def test_warp_fuse_blend(ops, source, form):
    """k = 3, in place on a channel slice of the decoder feature: the other channels keep their NaN fill, the slice holds none.
    Tolerance 1e-4, as test_warp_fuse_blend."""
    h, w = WARP_FORMS[form]
    n, k, c, mult = (6, 3, 40, 2.0) if form == "one" else (3, 3, 40, 2.0)
    walks(warp_blocks(n, c, h, w, 8), 8)
    ctxs, stacked, flows = warp_inputs(n, k, c, h, w, seed=2 * h + w)
    g = torch.Generator().manual_seed(h)
    occs, dec = torch.randn(n * k, 1, h, w, generator=g), torch.randn(n, c, h, w, generator=g)
    warped = O.backwarp(stacked.double(), flows.double() * mult, O.backwarp_grid(h, w).double())
    confs = (1 - torch.sigmoid(occs.double())).view(n, k, 1, h, w) + 1e-6
    wi = (warped.view(n, k, c, h, w) * confs).sum(1) / confs.sum(1)
    m = torch.sigmoid((occs.double().view(n, k, 1, h, w) * confs).sum(1) / confs.sum(1))
    want = m * dec.double() + (1 - m) * wi
    src = stacked.cuda() if source == "tensor" else [t.cuda() for t in ctxs]
    fd, od, dd = flows.cuda(), occs.cuda(), dec.cuda()

    def make():
        t = poison(n, c + 6, h, w)
        t[:, 3:3 + c] = dd
        return t, t[:, 3:3 + c]
    check(lambda view: ops.warp_fuse_blend(view, src, fd, od, mult, k), make, want, 1e-4, f"warp_fuse_blend {source} {form}")


@pytest.mark.parametrize("form", ["one", "quad", "tiled"])
def test_backwarp_proj(ops, form):
    """40 -> 10 channels (padded to the 16-channel instantiation), k = 2; blocks = pixel blocks x images, per_cu = 4.  Tolerance
    1e-4, as test_backwarp_proj_fused."""
    h, w = WARP_FORMS[form]
    nf, k, c, cout, mult = 5, 2, 40, 10, 2.0
    walks((cd(h * w // 4, 256) if w % 4 == 0 else cd(h * w, 256)) * nf * k, 4)
    ctxs, stacked, flow = warp_inputs(nf, k, c, h, w, seed=3 * h + w)
    g = torch.Generator().manual_seed(w)
    wt, bias = torch.randn(cout, c, 1, 1, generator=g), torch.randn(cout, generator=g)
    warped = O.backwarp(stacked.double(), flow.double() * mult, O.backwarp_grid(h, w).double())
    want = F.leaky_relu(O.equal_conv2d(warped, wt.double(), bias.double()), 0.1)
    w_t, cpad = ops.pack_proj_weight(wt.cuda())
    assert cpad == 16
    cd_, fd, bd = [t.cuda() for t in ctxs], flow.cuda(), bias.cuda()
    check(lambda out: ops.backwarp_proj(cd_, fd, mult, w_t, cpad, bd, cout, out=out), dense(nf * k, cout, h, w), want, 1e-4,
          f"backwarp_proj {form}")


def test_backwarp_p8(ops):
    """The back-warp into the packed input of the first Subpixel convolution, decoded with P8Act.float() as its own test
    (test_backwarp_p8_feeds_the_first_subpixel_convolution) does.  That test has no CPU reference to borrow: the bound here is the
    back-warp's 1e-4 (test_backwarp_oracle, the sibling that draws the same samples) plus the packing's own 2e-5 max |value| + 1e-7
    of that test.  The data buffer starts as 0xFF bytes."""
    nf, k, c, h, w, mult = 2, 3, 32, 40, 64, 2.0
    n = nf * k
    walks(cd(h * w // 4, 256) * (c // 8 + 1) * n, 8)
    ctxs, stacked, flow = warp_inputs(nf, k, c, h, w, seed=11)
    occ = torch.randn(n, 1, h, w, generator=torch.Generator().manual_seed(12))
    fo = torch.cat([flow, occ], dim=1)
    warped = O.backwarp(stacked.double(), flow.double() * mult, O.backwarp_grid(h, w).double())
    want = torch.cat([warped, fo.double(), torch.zeros(n, 5, h, w, dtype=torch.float64)], dim=1)
    bound = 1e-4 + 2e-5 * float(want.abs().max()) + 1e-7
    cd_, fod = [t.cuda() for t in ctxs], fo.cuda()
    got = {}
    for lim in LIMS + (0,):
        data = torch.empty(n * (c + 8) * h * w, dtype=torch.float32, device="cuda")
        data.view(torch.uint8).fill_(0xFF)
        p8 = budgeted(lim, lambda: ops.backwarp_p8(cd_, fod, mult, out=data))
        assert p8.data.data_ptr() == data.data_ptr() and p8.shape == (n, c + 8, h, w)
        left = int((data.view(torch.int32) == -1).sum())
        assert left == 0, f"backwarp_p8: budget {lim}: {left} of {data.numel()} dwords never written"
        got[lim] = p8
    for lim in LIMS:
        assert torch.equal(got[lim].data.view(torch.uint8), got[0].data.view(torch.uint8)), f"a budget of {lim} CUs changes the result"
        dec = got[lim].float().cpu().double()
        err = (dec - want).abs()
        print(f"backwarp_p8: budget {lim}: max |error| {float(err.max()):.3e}, bound {bound:.3e}")
        assert not torch.isnan(dec).any() and float(err.max()) <= bound
        assert torch.equal(dec[:, c + 3:], want[:, c + 3:])


# ------------------------------------------------------------------ flow / occlusion heads
@pytest.mark.parametrize("precision,n,hw", [("bf16x3", 4, (32, 48)), ("bf16x3", 3, (19, 37)), ("f32", 10, (16, 36)), ("f32", 6, (13, 19))],
                         ids=["bf16x3-w4", "bf16x3-odd", "f32-w4", "f32-odd"])
def test_conv_heads(ops, precision, n, hw):
    """The 9 x 9 flow / occ heads: `ccvs_tap_shift_add` behind the convolution (itself chunked by the stream's budget), vertical taps
    (split-bf16) and horizontal ones ("f32"), four pixels per lane and one, plain and accumulating, into the [flow | occ] tail of a
    wider tensor.  Tolerance 2e-4, as test_flow_occ_heads_vs_torch."""
    k, c = 9, 32
    h, w = hw
    walks(cd(n * 3 * h * w // 4, 256) if w % 4 == 0 else cd(n * 3 * h * w, 256), 8)
    assert (7 * h * w) % 4 == 0 or w % 4 != 0            # the four-pixel form needs a batch stride that is a multiple of 4
    g = torch.Generator().manual_seed(h * 100 + w)
    feat = torch.randn(n, c, h, w, generator=g)
    fw, ow, b3 = torch.randn(2, c, k, k, generator=g), torch.randn(1, c, k, k, generator=g), torch.randn(3, generator=g)
    base = torch.randn(n, 3, h, w, generator=g)
    conv = F.conv2d(feat.double(), torch.cat([fw, ow]).double() / math.sqrt(c * k * k), bias=b3.double(), padding=k // 2)
    pk = ops.pack_head_weights(fw.cuda(), ow.cuda(), precision)
    fd, bd, based = feat.cuda(), b3.cuda(), base.cuda()
    check(lambda out: ops.conv_heads(fd, pk, bd, out, accumulate=False), channel_slice(n, 7, 4, 3, h, w), conv, 2e-4,
          f"conv_heads {precision}")

    def make():
        t = poison(n, 7, h, w)
        t[:, 4:] = based
        return t, t[:, 4:]
    check(lambda out: ops.conv_heads(fd, pk, bd, out, accumulate=True), make, base.double() + conv, 2e-4,
          f"conv_heads {precision} accumulate")


# ------------------------------------------------------------------ Gaussian blur
def test_gaussian_blur(ops):
    """k = 11, sigma 4 on 70 x 90 planes (ragged tiles in both directions); bound 4e-6 max |x|, as tests/test_deblur_gpu.py; the
    reference is reflect padding and the k x k correlation in float64 with the float32 weights cast exactly."""
    n, c, h, w, k, sigma = 5, 3, 70, 90, 11, 4.0
    walks(cd(w, 64) * cd(h, 32) * n * c, 8)
    x = torch.rand(n, c, h, w, generator=torch.Generator().manual_seed(4)) * 2 - 1
    w1 = ops.gaussian_kernel1d(k, sigma).double()
    want = F.conv2d(F.pad(x.double(), [k // 2] * 4, mode="reflect"), torch.outer(w1, w1).expand(c, 1, k, k), groups=c)
    xd = x.cuda()
    check(lambda out: ops.gaussian_blur(xd, k, sigma, out=out), dense(n, c, h, w), want, 4e-6 * float(x.abs().max()), "gaussian_blur")


# ------------------------------------------------------------------ packed convolutions
@pytest.mark.parametrize("mode", ["0", "3"])
def test_packed_convolutions_under_a_budget(tmp_path, mode):
    """The InterBlock chain's packed (P8) layers with `ccvs_conv_desc.cu_limit` = 3 and 61 against 0, in a child process per
    persistent-tile mode (`CCVS_CONV_PT` is read once per process; tests/conv_pt_worker.py budget): the fp32-input layer with a packed
    output and a shared pre-activation image (99 -> 128, pre_div 3), a packed-input layer (128 -> 64) and a packed-input-and-output
    layer (64 -> 32), at (N, H, W) = (6, 40, 64).

    Which kernel a budget selects (`launch_conv_bf16`, csrc/conv2d_bf16_kernels.h): the persistent-tile kernel refuses any launch with
    a budget (`conv_pt_ok`), and so do the 512-pixel tile and the two-workgroups-per-CU form, so in BOTH modes a budget runs the
    256-pixel producer / consumer kernel as consecutive 1-D chunks of cu_limit x occupancy workgroups (at least 8): the aligned-row
    staging form with the packed K tail for 99 -> 128, the LDS-DMA form with the written-out 3 x 3 tap loop for the packed inputs.
    Without a budget mode 0 runs the same kernels as one 3-D grid; mode 3 would hand 3 x 3 layers to the persistent-tile kernel, but
    only from two tiles per CU up, which 6 images of 40 x 64 do not reach -- the mode then only proves that the switch does not
    change what a budgeted launch computes.
    (The exact-fp32 MFMA kernel, csrc/conv2d.hip, ignores the budget: no case for it.)

    Budgeted results equal the unbudgeted one bit for bit (packed data compared as bytes); the unbudgeted one is within 2e-4 of
    torch.nn.functional.conv2d in float64 on the decoded inputs."""
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    here = os.path.dirname(os.path.abspath(__file__))
    path = str(tmp_path / f"budget_pt{mode}.npz")
    subprocess.run([sys.executable, os.path.join(here, "conv_pt_worker.py"), path, "budget"], env=dict(os.environ, CCVS_CONV_PT=mode),
                   check=True, timeout=600)
    z = np.load(path)
    T = lambda key: torch.from_numpy(z[key]).double()
    # which kernels ran (ops.conv_last_launch() per result): 6 images of 40 x 64 are 60 tiles, so the dispatcher halves every layer's channel
    # block to 32 (MB = 1) -- never persistent tiles, a budget of 3 in chunks, no budget in one launch
    records = json.loads(str(z["records"]))
    forms = {"l1": "pc TW=32 MB=1 NTY=3 PP=2 WPC=1 ktail=3 ", "l2": "pc TW=32 MB=1 NTY=-83 PP=2 WPC=1 ktail=0 ", "l3": "pc TW=32 MB=1 NTY=-83 PP=2 WPC=1 ktail=0 "}
    for name, form in forms.items():
        for lim in (3, 61, 0):
            rec = records[f"{name}_{lim}"]
            assert rec.startswith(form) and rec.endswith(" zi=3" if name == "l1" else " zi=0"), (name, lim, rec)
            chunks = int(rec.split(" chunks=")[1].split()[0])
            assert (chunks == 1) if lim == 0 else (chunks > 1 or lim == 61), (name, lim, rec)

    def decode(data, c):   # P8Act.float()
        n, h, w = 6, 40, 64
        u = torch.from_numpy(data).view(torch.bfloat16).view(n, c // 8, 2, h, w, 8).float()
        return (u[:, :, 0] + u[:, :, 1]).permute(0, 1, 4, 2, 3).reshape(n, c, h, w).double()

    def ref(x, name, cin):
        conv = F.conv2d(x, T(f"w_{name}") / math.sqrt(cin * 9), bias=T(f"b_{name}"), padding=1)
        if name == "l1":
            conv = conv + T("pre").repeat_interleave(3, dim=0)
        return F.leaky_relu(conv, 0.1)
    cases = [("l1", T("x"), 99, 128, True), ("l2", decode(z["in_l2"], 128), 128, 64, False), ("l3", decode(z["in_l3"], 64), 64, 32, True)]
    for name, x, cin, cout, packed in cases:
        base = z[f"{name}_0"]
        for lim in (3, 61):
            assert np.array_equal(z[f"{name}_{lim}"].view(np.uint8), base.view(np.uint8)), f"{name}: cu_limit {lim} changes the result"
        got = decode(base, cout) if packed else torch.from_numpy(base).double()
        err = float((got - ref(x, name, cin)).abs().max())
        print(f"mode {mode} {name}: max |error| {err:.3e}")
        assert err <= 2e-4, (name, err)

"""-m gpu: every instantiation the convolution dispatchers can select without persistent tiles, at the op level, by kernel name and
against float64.

`ops.conv_last_launch()` (`ccvs_conv_last_launch`, host code in the launchers) says which kernel a call launched: the kernel, every
template argument by value, `p.ktail`, the number of 1-D chunks, whether the XCD tile order is on, `zi`.  Every row of `ROWS` holds the
record it expects, the call, and the branch it is there for; a case asserts the record FIRST -- a dispatcher heuristic that moves a
shape to another kernel fails the row instead of silently un-testing the form (the `mb` halving of conv2d_bf16.hip had done that to
tests/test_ops_gpu.py::test_conv_tall_tile_shapes) -- and then the result against a float64 CPU reference.

The table (conv2d_bf16_kernels.h `launch_conv_bf16<TW, MB>`, conv2d.hip `launch_conv<TW, MB>`; TW = tile width 8 / 16 / 32 by output
width, MB = 32-channel blocks per workgroup, halved while a launch has fewer than 256 workgroups -- hence the many tiny images):
  pc NTY 3 / 1    aligned rows (3 x 3 pad 1 / kh = 1; W % 4 == 0, TW >= 16): TW {16, 32} x MB {1, 2, 4}; the packed K tail r = Cin % 16 in
                  {1, 2, 3} (`CB_KTAIL`) at each of MB 1, 2, 4.  `pc TW=32 MB=4 NTY=3` with fp32 output needs Cin > 64, `pc TW=32 MB=2 NTY=3
                  PP=2 WPC=1` Cin > 64 and fewer than 32 output rows (or a CU budget): Cin <= 64 takes WPC = 2, 32 rows the 512-pixel tile.
  WPC 2           `<32, 2, 3, 2, 2>`, two workgroups per CU: Cin <= 64, with each K tail and without.
  PP 4            the 512-pixel tile `<32, 2, 3, 4>`, `<32, 2, 1, 4>`, `<32, 2, -83, 4>`: >= 32 output rows; each again under a CU budget of 3,
                  which must take the PP = 2 form in chunks and give the same bits.
  pc NTY 0 / -2   scalar staging, one / two pixel passes per tap row: TW {8, 16, 32} x MB {1, 2, 4}.  NTY -2 needs a halo tile of more than
                  kh x 256 elements: at MB >= 2 (at most 3 taps per row) only the 1 x 3 kernel has one; 3 x 3 stride 2 has 5 passes and fits
                  the LDS at MB = 1 only (MB 2 / 4 take the synchronous kernel).
  pc NTY -8 / -83 packed (P8) input, generic / written-out 3 x 3: TW {8, 16, 32} x MB {1, 2, 4}, fp32 and packed output.  `-83` has no MB = 4
                  (launch_conv_bf16: "the written-out form spills"): 3 x 3 at MB = 4 takes `-8`.
  sync            `conv2d_bf16x3_kernel<TW, MB, 8>`: 1 x 1 stride 2 and transposed (odd input sizes: four parity classes of different
                  extent), TW {8, 16, 32} x MB {1, 2, 4}.
  f32             `conv2d_mfma_kernel<TW, MB>`, TW {8, 16, 32} x MB {1, 2}: stride 1, stride 2, transposed, the k x 1 head.
Not reachable here, by design: the persistent-tile kernel (`pt ...`: >= 512 tile units on whole 32-column tiles; every row has a width
that is no multiple of 32, and the case asserts that no record starts with `pt`).

Every family has a row with the XCD order off and one with it on, a ragged Cout at MB >= 2, and the shared pre-activation image
(`pre`, `pre_div` = 3, `zi` = 3).  The epilogue y = [y +] (act(conv + pre[n // pre_div] + bias) [+ res]) * out_scale runs whole, into
channel-slice `out=` / `residual=` views whose margins keep their NaN, once per store routine (`EPI`): the LDS-staged fp32 store of `pc`
at PP = 2 and PP = 4, the packed-output store (pre, bias, act), the synchronous kernel's and the fp32-MFMA kernel's -- each at MB >= 2
with act, without, and with accumulate.  Outputs start as NaN (packed outputs as 0xFF bytes = bf16 NaN); packed inputs are packed on
the host from a known fp32 tensor of 16-bit values (`operands`), the reference is taken on the values they decode to -- that tensor --
and the same call on the fp32 tensor must give the same bits.

Reference: `torch.nn.functional.conv2d` / `conv_transpose2d` on `.double()` operands, the weight as the fp32 product
`weight * (1 / sqrt(Cin kh kw))` that `pack_conv_weight` forms.

Tolerance, split-bf16.  Each operand is hi + lo, both rounded to bf16 (8 significant bits): |x - hi - lo| <= 2^-16 |x|.  The kernel
forms hi hi + hi lo + lo hi and drops lo lo <= 2^-16 |x w|, so a product is within 3 * 2^-16 of exact (two operand errors and the
dropped term; second-order terms are below 2^-30).  The products are added into fp32 accumulators: s additions, each rounding by at
most 2^-24 of a partial sum that A bounds, add at most s * 2^-24 * A, with s = 3 * kh * kw * CinPad (three products per tap and channel
of the padded K depth) + 4 (bias, pre, residual, old y) -- the worst case of Higham 3.1, taken per product so that it does not depend on
how the matrix unit orders the 16 products of an instruction.  The check is per element
    |got - want| <= (3 * 2^-16 + s * 2^-24) * A,   A = (conv(|x|, |w|) + |bias| + |pre| [+ |res|]) * out_scale [+ |old y|]
in float64 (the activation, leaky ReLU 0.1, is 1-Lipschitz and keeps the bound); a packed output adds 2^-16 |want| (its own hi + lo).
Exact-fp32 kernel: 1e-5 * A, the bound and the argument of tests/test_gemm_forms_gpu.py.  Budgeted against unbudgeted and packed
input against the fp32 input it decodes to: the same bits.
K = Cin kh kw stays small (<= 729) on purpose: the error of the split falls like 1 / sqrt(K) relative to A, and with it the margin to a
kernel that loses one of the three products -- a CPU emulation of the three-product split alone (float64 accumulation, the largest
of 4096 x 64 outputs on normal operands) gives |err| / A of 1.7e-5 at K = 8, 5.6e-6 at K = 72 and 1.2e-6 at K = 729 against the
bound's 4.6e-5, and 3.3e-3, 1.3e-3, 4.5e-4 with one cross product dropped.
Observed on an MI355X, largest |err| / A per family over all rows (each case prints its own): pc NTY 3 7.1e-6 (WPC 2 6.2e-6, PP 4
1.7e-6), NTY 1 1.6e-5 (PP 4 1.5e-5), NTY 0 1.6e-5, NTY -2 1.1e-5, NTY -83 5.2e-6 (PP 4 4.9e-6), NTY -8 9.9e-6, sync 1.6e-5 -- the
largest are the K = 8 rows, at the emulation's own figure -- and 2.1e-7 for the exact-fp32 kernel.  No row fails on the kernels as they
are.  Mutations, each run once by hand against this table: the second `CB_KTAIL` step skipped fails exactly the 15 rows with ktail 2 or
3 (|err| / A 0.03 ... 0.25); `r_ + 1` for `r_` in `CB_KTAIL`'s `q / r_` fails exactly the 19 rows with a K tail (0.06 ... 0.39).
The `fa[.][1] * fb[.][pp][0]` MFMA of `CB_TAP` dropped for m >= 1 fails the 52 pc rows with PP = 2, WPC = 1 and MB >= 2 against float64
(|err| / A 5.8e-4 ... 3.1e-3, first bad element in channel 32) and the five PP = 4 rows through their budgeted PP = 2 twin's bits; the
MB = 1, WPC = 2 (a tap loop of its own), sync and f32 rows pass, as they must.  The whole module: 126 rows + the coverage check in
about 3 s, references included."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SPLIT = 3 * 2.0 ** -16
F32_REL = 1e-5


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ccvs_amd import ops as _ops
    assert _ops.CONV_PRECISION == "bf16x3" and _ops.CONV_CU_LIMIT == 0
    return _ops


def case(n, cin, h, w, cout, k, **opt):
    """One call: (N, Cin, H, W, Cout, kh) and kw, stride, pad (default 1 for a 3 x 3 stride-1 kernel, else 0), transposed, precision,
    in_p8 / out_p8, pre_div (0: no pre image), act, res, acc, out_scale, views (channel-slice out= / residual= views), x_slice
    (channel-slice input view), budget (record expected under CONV_CU_LIMIT = 3, same bits)."""
    c = dict(n=n, cin=cin, h=h, w=w, cout=cout, k=k, kw=k, stride=1, pad=None, transposed=False, precision="bf16x3", in_p8=False,
             out_p8=False, pre_div=0, act=False, res=False, acc=False, out_scale=1.0, views=False, x_slice=False, budget=None)
    assert set(opt) <= set(c), opt
    c.update(opt)
    if c["pad"] is None:
        c["pad"] = 1 if (k == 3 and c["kw"] == 3 and c["stride"] == 1 and not c["transposed"]) else 0
    return c


def pc(tw, mb, nty, pp=2, wpc=1, ktail=0, chunks=1, xcd=0, zi=0):
    return f"pc TW={tw} MB={mb} NTY={nty} PP={pp} WPC={wpc} ktail={ktail} chunks={chunks} xcd={xcd} zi={zi}"


def sync(tw, mb, xcd=0, zi=0):
    return f"sync TW={tw} MB={mb} chunks=1 xcd={xcd} zi={zi}"


def f32(tw, mb):
    return f"f32 TW={tw} MB={mb}"


T = dict(transposed=True, stride=2)
S2 = dict(stride=2)
ROWS = [
    # ---- pc, aligned rows, 3 x 3 (NTY 3): TW {16, 32} x MB {1, 2, 4}, K tail 1 / 2 / 3 at each MB
    (pc(16, 1, 3, ktail=1), case(16, 33, 8, 12, 32, 3), "TW 16, MB 1, K tail r = 1: one tail step; 16 workgroups, XCD order off"),
    (pc(16, 1, 3, ktail=3, xcd=1), case(64, 19, 8, 12, 64, 3), "MB halved to 1 (128 workgroups), r = 3: two tail steps, 11 valid K in the second"),
    (pc(32, 1, 3, ktail=2), case(16, 34, 12, 20, 32, 3), "TW 32, MB 1, r = 2: second tail step with two valid K in one lane half, none in the other"),
    (pc(16, 2, 3, ktail=2, xcd=1), case(256, 18, 8, 12, 64, 3), "TW 16, MB 2, r = 2; 256 workgroups, XCD order on"),
    (pc(16, 2, 3, ktail=1, zi=3), case(258, 17, 8, 12, 40, 3, pre_div=3, act=True), "MB 2, r = 1, ragged Cout 40 of 64, shared pre image (zi 3), 258 workgroups"),
    (pc(32, 2, 3, ktail=3, xcd=1), case(128, 67, 12, 20, 64, 3), "TW 32, MB 2, PP 2, WPC 1 (Cin > 64, 12 rows), r = 3"),
    (pc(16, 4, 3, xcd=1), case(256, 8, 8, 12, 128, 3), "TW 16, MB 4, half a K chunk (Cin 8), no tail"),
    (pc(16, 4, 3, ktail=2, xcd=1), case(256, 66, 8, 12, 128, 3), "TW 16, MB 4, r = 2"),
    (pc(16, 4, 3, ktail=3), case(258, 67, 8, 12, 104, 3), "TW 16, MB 4, r = 3, ragged Cout 104 of 128"),
    (pc(32, 4, 3, ktail=1, xcd=1), case(128, 65, 12, 20, 128, 3), "TW 32, MB 4 (fp32 output: Cin > 64), r = 1"),
    (pc(32, 4, 3, xcd=1), case(128, 80, 12, 20, 128, 3), "TW 32, MB 4, five whole K chunks"),
    # ---- pc, aligned rows, kh = 1 (NTY 1)
    (pc(16, 1, 1), case(16, 8, 8, 12, 32, 1), "1 x 1, TW 16, MB 1"),
    (pc(16, 2, 1, xcd=1), case(256, 24, 8, 12, 64, 1), "1 x 1, TW 16, MB 2, one and a half K chunks"),
    (pc(16, 4, 1, zi=3), case(258, 8, 8, 12, 128, 1, pre_div=3), "1 x 1, TW 16, MB 4, shared pre image"),
    (pc(32, 1, 1), case(4, 32, 9, 24, 27, 1, kw=9, pad=4), "the 1 x 9 head on aligned rows: nine taps per row (MB 1 only), ragged Cout 27"),
    (pc(32, 2, 1, xcd=1), case(128, 8, 12, 20, 64, 1), "1 x 1, TW 32, MB 2, under 32 rows: PP 2"),
    (pc(32, 4, 1), case(129, 8, 12, 20, 128, 1), "1 x 1, TW 32, MB 4; 258 workgroups"),
    # ---- two workgroups per CU (WPC 2): Cin <= 64
    (pc(32, 2, 3, wpc=2, xcd=1), case(128, 8, 12, 20, 64, 3), "WPC 2 without a K tail"),
    (pc(32, 2, 3, wpc=2, ktail=2, xcd=1), case(128, 18, 12, 20, 64, 3), "WPC 2, r = 2"),
    (pc(32, 2, 3, wpc=2, ktail=1, zi=3), case(129, 33, 12, 20, 128, 3, pre_div=3, act=True), "WPC 2 from MB 4 (128 channels, Cin <= 64), r = 1, pre image; 516 workgroups"),
    (pc(32, 2, 3, wpc=2, ktail=3), case(129, 19, 12, 20, 40, 3), "WPC 2, r = 3, ragged Cout 40 of 64, 258 workgroups"),
    # ---- the 512-pixel tile (PP 4); each again under a CU budget
    (pc(32, 2, 3, pp=4, xcd=1), case(32, 80, 32, 36, 64, 3, budget=pc(32, 2, 3, chunks=32)), "<32, 2, 3, 4>: Cin > 64, 32 rows; 128 workgroups"),
    (pc(32, 2, 3, pp=4, ktail=3), case(13, 99, 37, 100, 64, 3, act=True, budget=pc(32, 2, 3, ktail=3, chunks=33)),
     "ragged 37 x 100, 13 images, r = 3: the last tile row has 5 of 16 lines, the last column 4 of 32; 156 workgroups"),
    (pc(32, 2, 3, pp=4, ktail=2, zi=3), case(33, 66, 32, 36, 40, 3, pre_div=3, budget=pc(32, 2, 3, ktail=2, chunks=33, zi=3)),
     "PP 4, r = 2, ragged Cout, pre image in the (group, tile, image) order"),
    (pc(32, 2, 1, pp=4, xcd=1), case(32, 8, 32, 36, 64, 1, budget=pc(32, 2, 1, chunks=32)), "<32, 2, 1, 4>: 1 x 1"),
    (pc(32, 2, -83, pp=4, xcd=1), case(32, 16, 32, 36, 64, 3, in_p8=True, out_p8=True, act=True, budget=pc(32, 2, -83, chunks=32)),
     "<32, 2, -83, 4>: packed in and out"),
    # ---- pc, scalar staging in one pass per tap row (NTY 0)
    (pc(8, 1, 0), case(16, 8, 8, 8, 32, 3), "TW 8 (never aligned rows), MB 1"),
    (pc(8, 2, 0, xcd=1), case(256, 8, 4, 4, 64, 3), "TW 8, MB 2, 4 x 4 images"),
    (pc(8, 4, 0, zi=3), case(258, 8, 4, 4, 104, 3, pre_div=3, act=True), "TW 8, MB 4, ragged Cout, pre image"),
    (pc(16, 1, 0), case(16, 10, 9, 13, 32, 3, pad=0), "3 x 3 with pad 0, W % 4 != 0, TW 16, MB 1"),
    (pc(16, 2, 0, xcd=1), case(256, 8, 6, 10, 64, 3), "W = 10: rows not 16-byte aligned, TW 16, MB 2"),
    (pc(16, 4, 0, xcd=1), case(256, 8, 6, 10, 128, 3, x_slice=True), "channel-slice input view, TW 16, MB 4"),
    (pc(32, 1, 0), case(4, 32, 9, 21, 27, 9, kw=1, pad=4), "the 9 x 1 head: nine tap rows, TW 32, MB 1"),
    (pc(32, 2, 0, xcd=1), case(128, 8, 12, 18, 64, 3), "W = 18 (the WPC 2 choice falls back to scalar staging), TW 32, MB 2"),
    (pc(32, 4, 0, xcd=1), case(128, 8, 12, 18, 128, 1), "1 x 1 on unaligned rows, TW 32, MB 4"),
    (pc(32, 4, 0, xcd=1), case(128, 8, 12, 18, 128, 3, out_p8=True, act=True), "scalar staging into the packed-output store, MB 4 (packed output: no WPC 2)"),
    # ---- pc, scalar staging in two passes per tap row (NTY -2)
    (pc(32, 1, -2), case(4, 16, 17, 37, 32, 3, **S2), "3 x 3 stride 2: 17 x 65 halo, 5 passes; MB 1 (MB 2 / 4 do not fit the LDS)"),
    (pc(32, 1, -2), case(4, 10, 9, 21, 27, 1, kw=5, pad=2), "the 1 x 5 head on unaligned rows, MB 1"),
    (pc(8, 1, -2), case(16, 8, 4, 6, 32, 1, kw=3, pad=1), "1 x 3: 32 x 10 halo for one tap row, TW 8, MB 1"),
    (pc(8, 2, -2, xcd=1), case(256, 8, 4, 6, 64, 1, kw=3, pad=1), "1 x 3, TW 8, MB 2"),
    (pc(8, 4, -2, xcd=1), case(256, 8, 4, 6, 128, 1, kw=3, pad=1), "1 x 3, TW 8, MB 4"),
    (pc(16, 1, -2), case(16, 8, 4, 10, 32, 1, kw=3, pad=1), "1 x 3, TW 16, MB 1"),
    (pc(16, 2, -2, zi=3), case(258, 8, 4, 10, 40, 1, kw=3, pad=1, pre_div=3), "1 x 3, TW 16, MB 2, ragged Cout, pre image"),
    (pc(16, 4, -2, xcd=1), case(256, 8, 4, 10, 128, 1, kw=3, pad=1), "1 x 3, TW 16, MB 4"),
    (pc(32, 2, -2, xcd=1), case(128, 8, 10, 18, 64, 1, kw=3, pad=1), "1 x 3, TW 32, MB 2"),
    (pc(32, 4, -2), case(129, 8, 10, 18, 128, 1, kw=3, pad=1), "1 x 3, TW 32, MB 4, 258 workgroups"),
]

# ---- pc, packed input: the written-out 3 x 3 (NTY -83: MB 1, 2) and the generic form (NTY -8: 1 x 1 at MB 1, 2; 3 x 3 at MB 4), TW {8, 16, 32},
# each with fp32 and with packed output
_P8_IMG = {8: (4, 4), 16: (8, 12), 32: (12, 20)}   # one tile per image (two at TW 32)
for _tw, (_h, _w) in _P8_IMG.items():
    for _mb in (1, 2, 4):
        _n = 16 if _mb == 1 else (128 if _tw == 32 else 256)
        for _o8 in (False, True):
            _what = f"TW {_tw}, MB {_mb}, " + ("packed" if _o8 else "fp32") + " output"
            if _mb != 4:
                ROWS.append((pc(_tw, _mb, -83, xcd=int(_mb > 1)), case(_n, 16, _h, _w, 32 * _mb, 3, in_p8=True, out_p8=_o8, act=True), "packed input, written-out 3 x 3, " + _what))
                ROWS.append((pc(_tw, _mb, -8, xcd=int(_mb > 1)), case(_n, 24, _h, _w, 32 * _mb, 1, in_p8=True, out_p8=_o8), "packed input, 1 x 1 (odd number of 8-channel groups), " + _what))
            else:
                ROWS.append((pc(_tw, 4, -8, xcd=1), case(_n, 16, _h, _w, 128, 3, in_p8=True, out_p8=_o8, act=True), "packed input, 3 x 3 at MB 4 (no written-out form), " + _what))
ROWS += [
    (pc(16, 2, -83, zi=3), case(258, 8, 8, 12, 40, 3, in_p8=True, pre_div=3, act=True), "packed input, ragged Cout 40 of 64, pre image, 258 workgroups"),
    (pc(32, 1, -8), case(4, 32, 9, 21, 27, 1, kw=9, pad=4, in_p8=True), "packed input, the 1 x 9 head (nine taps per row, MB 1)"),
    (pc(32, 2, -83, xcd=1), case(32, 16, 32, 36, 64, 3, in_p8=True), "packed input, 32 rows, fp32 output: stays on the 256-pixel tile"),
]

# ---- the synchronous kernel: 1 x 1 stride 2 and transposed, TW {8, 16, 32} x MB {1, 2, 4}
_S2_IMG = {8: (7, 7), 16: (15, 23), 32: (15, 39)}    # -> 4 x 4, 8 x 12, 8 x 20
_T_IMG = {8: (7, 5), 16: (7, 9), 32: (7, 17)}        # odd sizes -> 15 x 11, 15 x 19, 15 x 35: classes of 8 x 6 / 7 x 6 / 8 x 5 / 7 x 5 ...
for _tw in (8, 16, 32):
    for _mb in (1, 2, 4):
        ROWS.append((sync(_tw, _mb, xcd=int(_mb > 1)), case(16 if _mb == 1 else 256, 8, *_S2_IMG[_tw], 32 * _mb, 1, **S2), f"1 x 1 stride 2, TW {_tw}, MB {_mb}"))
        ROWS.append((sync(_tw, _mb, xcd=int(_mb > 1)), case(4 if _mb == 1 else 64, 8, *_T_IMG[_tw], 32 * _mb, 3, **T), f"transposed, odd input size, TW {_tw}, MB {_mb}"))
ROWS += [
    (sync(16, 2, zi=3), case(258, 8, 15, 23, 40, 1, pre_div=3, act=True, **S2), "stride 2, ragged Cout 40 of 64, pre image (zi 3), 258 workgroups"),
    (sync(32, 2, xcd=1), case(256, 16, 17, 37, 64, 3, **S2), "3 x 3 stride 2 at MB 2: the two-pass form does not fit the LDS"),
    (sync(16, 4), case(65, 8, 8, 8, 104, 3, **T), "transposed, even input size, ragged Cout 104 of 128, 260 workgroups"),
    # ---- the exact-fp32 kernel
    (f32(8, 1), case(4, 8, 8, 8, 32, 3, precision="f32"), "fp32 MFMA, stride 1, TW 8, MB 1"),
    (f32(8, 2), case(4, 8, 7, 5, 70, 3, precision="f32", **T), "fp32 MFMA, transposed, odd input, ragged Cout 70 of 128, TW 8, MB 2"),
    (f32(16, 1), case(4, 16, 19, 25, 32, 3, precision="f32", **S2), "fp32 MFMA, 3 x 3 stride 2, TW 16, MB 1"),
    (f32(16, 2), case(4, 16, 9, 4, 64, 9, kw=1, pad=4, precision="f32"), "fp32 MFMA, the 9 x 1 head, TW 16, MB 2"),
    (f32(32, 1), case(3, 10, 9, 21, 27, 3, precision="f32", pre_div=3, act=True), "fp32 MFMA, stride 1, TW 32, MB 1, pre image"),
    (f32(32, 2), case(4, 8, 23, 39, 64, 1, precision="f32", **S2), "fp32 MFMA, 1 x 1 stride 2, TW 32, MB 2"),
    (f32(16, 2), case(4, 7, 7, 9, 64, 3, precision="f32", **T), "fp32 MFMA, transposed, TW 16, MB 2"),
]

# ---- the whole epilogue into channel-slice views, once per store routine: act, no act, accumulate
_FULL = dict(pre_div=3, res=True, out_scale=1 / math.sqrt(2), views=True)
EPI = []
for _var, _o in (("act", dict(act=True)), ("no act", dict(act=False)), ("accumulate", dict(act=True, acc=True))):
    EPI += [
        (pc(16, 4, 3, ktail=2, zi=3), case(258, 18, 8, 12, 104, 3, **_FULL, **_o), f"LDS-staged fp32 store of pc at PP 2, MB 4, ragged Cout: {_var}"),
        (pc(32, 2, 3, pp=4, zi=3), case(33, 80, 32, 36, 64, 3, **_FULL, **_o), f"the same store at PP 4: {_var}"),
        (sync(16, 4, xcd=1), case(66, 8, 8, 8, 104, 3, **T, **_FULL, **_o), f"the synchronous kernel's store, transposed, MB 4, ragged Cout: {_var}"),
        (sync(16, 2, zi=3), case(258, 8, 15, 23, 64, 1, **S2, **_FULL, **_o), f"the synchronous kernel's store, stride 2, MB 2, image order of the pre group: {_var}"),
        (f32(32, 2), case(6, 8, 12, 20, 70, 3, precision="f32", **_FULL, **_o), f"the fp32-MFMA kernel's store, MB 2, ragged Cout: {_var}"),
    ]
    if _var != "accumulate":   # packed output: no residual, no accumulate (ccvs_conv2d_bf16x3 refuses them)
        EPI += [
            (pc(32, 4, 3, ktail=2, zi=3), case(129, 18, 12, 20, 128, 3, out_p8=True, pre_div=3, **_o), f"packed-output store, MB 4 (pre, bias, act only): {_var}"),
            (pc(16, 2, 3, zi=3), case(258, 8, 8, 12, 40, 3, out_p8=True, pre_div=3, **_o), f"packed-output store, MB 2, ragged Cout 40 of 64: {_var}"),
        ]
ROWS += EPI
del EPI


def pack_p8(x):
    """fp32 [n, c, h, w] -> the packed activation buffer ops.P8Act describes: [n][c / 8][hi | lo][h][w] units of 8 bf16."""
    n, c, h, w = x.shape
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    u = torch.stack([hi, lo], 0).view(2, n, c // 8, 8, h, w).permute(1, 2, 0, 4, 5, 3).contiguous()
    return u.view(-1).view(torch.float32)


def p8_poison(numel):
    """A packed-output buffer of 0xFF bytes: every bf16 of it a NaN."""
    return torch.full((numel,), -1, dtype=torch.int32, device="cuda").view(torch.float32)


def operands(ops, c, seed):
    """The operands of a case on the CPU (fp32; x as the values the kernel sees) and the arguments of its call."""
    g = torch.Generator().manual_seed(1000 + seed)
    n, cin, h, w, cout, kh, kw = (c[f] for f in ("n", "cin", "h", "w", "cout", "k", "kw"))
    if c["transposed"]:
        ho, wo = 2 * h + kh - 2, 2 * w + kw - 2
    else:
        ho, wo = (h + 2 * c["pad"] - kh) // c["stride"] + 1, (w + 2 * c["pad"] - kw) // c["stride"] + 1
    wide = torch.randn(n, cin + (5 if c["x_slice"] else 0), h, w, generator=g)
    x = wide[:, 3:3 + cin] if c["x_slice"] else wide
    wt = torch.randn(cout, cin, kh, kw, generator=g)
    b = torch.randn(cout, generator=g)
    pre = torch.randn(n // c["pre_div"], cout, ho, wo, generator=g) if c["pre_div"] else None
    res = torch.randn(n, cout, ho, wo, generator=g) if c["res"] else None
    old = torch.randn(n, cout, ho, wo, generator=g) if c["acc"] else None
    if c["in_p8"]:
        # the known fp32 tensor: values of 16 significant bits (hi + lo of the random ones), packed as the kernel's own split of them (a
        # pair whose lo is half a unit of hi is not the split of its sum when hi is odd: about 2 pairs in 1000 of a first packing,
        # and the fp32 path then drops another lo * lo) -- the bytes decode to x exactly and the fp32 path splits x into the same pairs
        x = ops.P8Act(pack_p8(x), n, cin, h, w).float()
        x8 = ops.P8Act(pack_p8(x).cuda(), n, cin, h, w)
        assert torch.equal(x8.float().cpu(), x)     # the values the packed bytes decode to
        x_dev = x8
    else:
        x_dev = wide.cuda()[:, 3:3 + cin] if c["x_slice"] else x.cuda()
    return dict(x=x, w=wt, b=b, pre=pre, res=res, old=old, x_dev=x_dev, ho=ho, wo=wo)


def reference(c, o):
    """(want, A) in float64: the epilogue on the exact convolution, and the sum of the magnitudes of everything added."""
    scale = 1 / math.sqrt(c["cin"] * c["k"] * c["kw"])
    ws = (o["w"].float() * scale).double()           # the fp32 product pack_conv_weight forms
    xd = o["x"].double()
    if c["transposed"]:
        conv = lambda a, b_: F.conv_transpose2d(a, b_.transpose(0, 1), stride=2)
    else:
        conv = lambda a, b_: F.conv2d(a, b_, stride=c["stride"], padding=c["pad"])
    want = conv(xd, ws) + o["b"].double().view(1, -1, 1, 1)
    mag = conv(xd.abs(), ws.abs()) + o["b"].double().abs().view(1, -1, 1, 1)
    if o["pre"] is not None:
        p = o["pre"].double().repeat_interleave(c["pre_div"], dim=0)
        want, mag = want + p, mag + p.abs()
    if c["act"]:
        want = F.leaky_relu(want, 0.1)
    if o["res"] is not None:
        want, mag = want + o["res"].double(), mag + o["res"].double().abs()
    osc = float(np.float32(c["out_scale"]))
    want, mag = want * osc, mag * osc
    if o["old"] is not None:
        want, mag = want + o["old"].double(), mag + o["old"].double().abs()
    return want, mag


def launch(ops, c, o, pk, x_dev):
    """One call on fresh poisoned outputs -> (result on the GPU, record, the whole output buffer when it is a view)."""
    n, cout, ho, wo = c["n"], c["cout"], o["ho"], o["wo"]
    big = None
    if c["out_p8"]:
        out = p8_poison(n * cout * ho * wo)
    elif c["views"]:
        big = torch.full((n, cout + 5, ho, wo), float("nan"), device="cuda")
        out = big[:, 2:2 + cout]
    else:
        out = torch.full((n, cout, ho, wo), float("nan"), device="cuda")
    if c["acc"]:
        out.copy_(o["old"])
    res = None
    if o["res"] is not None:
        res = torch.full((n, cout + 3, ho, wo), float("nan"), device="cuda")[:, 1:1 + cout] if c["views"] else torch.empty(n, cout, ho, wo, device="cuda")
        res.copy_(o["res"])
    got = ops.conv2d(x_dev, pk, o["b"].cuda(), cout, c["k"], stride=c["stride"], pad=c["pad"], transposed=c["transposed"], act=c["act"],
                     residual=res, out_scale=c["out_scale"], out=out, accumulate=c["acc"], pre=o["pre"].cuda() if o["pre"] is not None else None,
                     pre_div=c["pre_div"] or 1, out_p8=c["out_p8"])
    return got, ops.conv_last_launch(), big


def bits(t):
    """The result's bit pattern (a packed result: its buffer)."""
    return (t if isinstance(t, torch.Tensor) else t.data).contiguous().view(torch.int32)


FIGURES = {}


@pytest.mark.parametrize("i", range(len(ROWS)), ids=[f"{i:03d}-{r[0].replace(' ', '_')}" for i, r in enumerate(ROWS)])
def test_conv_form(ops, i):
    record, c, why = ROWS[i]
    o = operands(ops, c, i)
    pk = ops.pack_conv_weight(o["w"].cuda(), c["precision"])
    got, rec, big = launch(ops, c, o, pk, o["x_dev"])
    assert not rec.startswith("pt"), (rec, why)
    assert rec == record, f"row {i} ({why}): launched `{rec}`, the row is there for `{record}`"
    want, mag = reference(c, o)
    val = (got.float() if c["out_p8"] else got).double().cpu()
    assert val.shape == want.shape, (why, val.shape, want.shape)
    assert torch.isfinite(val).all(), f"row {i} ({why}): NaN left in the output -- an element was not written"
    if c["precision"] == "f32":
        rel = F32_REL
    else:
        s = 3 * c["k"] * c["kw"] * 16 * -(-c["cin"] // 16) + 4
        rel = SPLIT + s * 2.0 ** -24
    err = (val - want).abs()
    ratio = (err / mag).max().item()
    FIGURES[i] = ratio
    print(f"conv-form row {i:3d} {record:62s} max |err| / A = {ratio:.3e} (bound {rel:.3e})")
    bound = rel * mag + (2.0 ** -16 * want.abs() if c["out_p8"] else 0.0)
    bad = err > bound
    assert not bad.any(), (f"row {i} ({why}): {int(bad.sum())} elements beyond the bound, max |err| / A = {ratio:.3e} > {rel:.3e} "
                           f"at {tuple(int(v) for v in torch.nonzero(bad)[0])}")
    if big is not None:
        assert torch.isnan(big[:, :2]).all() and torch.isnan(big[:, 2 + c["cout"]:]).all(), f"row {i} ({why}): wrote outside the output's channel slice"
    if c["in_p8"]:
        # the same call on the fp32 tensor the packed bytes decode to (another staging mode of the same arithmetic): the same bits
        same, rec32, _ = launch(ops, c, o, pk, o["x"].cuda())
        assert "NTY=-8" not in rec32, rec32
        assert torch.equal(bits(same), bits(got)), f"row {i} ({why}): packed input `{rec}` and fp32 input `{rec32}` differ"
    if c["budget"]:
        ops.CONV_CU_LIMIT = 3
        try:
            lim, rec_b, _ = launch(ops, c, o, pk, o["x_dev"])
        finally:
            ops.CONV_CU_LIMIT = 0
        assert rec_b == c["budget"], f"row {i} ({why}): under a CU budget of 3 launched `{rec_b}`, expected `{c['budget']}`"
        assert torch.equal(bits(lim), bits(got)), f"row {i} ({why}): budgeted `{rec_b}` and unbudgeted `{rec}` differ"


def test_table_covers_every_form():
    """The table names every instantiation the module's docstring lists (a row removed or re-pointed later fails here, GPU or not in
    the selection)."""
    have = {r[0].split(" chunks")[0].replace(" ktail=1", " ktail=0").replace(" ktail=2", " ktail=0").replace(" ktail=3", " ktail=0") for r in ROWS}
    need = set()
    for tw in (16, 32):
        for mb in (1, 2, 4):
            need |= {f"pc TW={tw} MB={mb} NTY={nty} PP=2 WPC=1 ktail=0" for nty in (3, 1)}
    for tw in (8, 16, 32):
        for mb in (1, 2, 4):
            need.add(f"pc TW={tw} MB={mb} NTY=0 PP=2 WPC=1 ktail=0")
            need.add(f"pc TW={tw} MB={mb} NTY=-8 PP=2 WPC=1 ktail=0")
            need.add(f"sync TW={tw} MB={mb}")
            if mb != 4:
                need.add(f"pc TW={tw} MB={mb} NTY=-83 PP=2 WPC=1 ktail=0")
                need.add(f"f32 TW={tw} MB={mb}")
            need.add(f"pc TW={tw} MB={mb} NTY=-2 PP=2 WPC=1 ktail=0")
    need |= {"pc TW=32 MB=2 NTY=3 PP=2 WPC=2 ktail=0", "pc TW=32 MB=2 NTY=3 PP=4 WPC=1 ktail=0", "pc TW=32 MB=2 NTY=1 PP=4 WPC=1 ktail=0",
             "pc TW=32 MB=2 NTY=-83 PP=4 WPC=1 ktail=0"}
    assert need <= have, sorted(need - have)
    tails = {(r[0].split(" MB=")[1].split(" ")[0], r[0].split("ktail=")[1].split(" ")[0]) for r in ROWS if r[0].startswith("pc")}
    assert {(mb, kt) for mb in "124" for kt in "123"} <= tails, "each K tail at each MB"

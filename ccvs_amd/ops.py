"""Tensor-level wrappers over the C ABI (include/ccvs_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every call below hands raw
device pointers and sizes to libccvs_hip.so.  There is no fallback: a CPU tensor or a missing
library raises.
"""
import ctypes as C
import math

import torch

from . import lib as _lib

ACT_NONE, ACT_LRELU = 0, 1
EPI_NONE, EPI_GELU, EPI_RESIDUAL = 0, 1, 2
GEMM_SEQ = 0x100   # CCVS_GEMM_SEQ: whole-sequence call (OR-ed into the epilogue word)


class KernelTimer:
    """HIP-event bracket around individual launches of one kernel on the current stream
    (used by bench.py for the roofline of the dominant kernel; off by default)."""

    def __init__(self):
        self.records = []  # (name, algorithmic flops, start event, end event)
        self._open = None

    def begin(self, name, flops=0.0, nbytes=0.0, side=0.0, tag=None):
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        self._open = (name, flops, e0, nbytes, side, tag)

    def end(self):
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        name, flops, e0, nbytes, side, tag = self._open
        self.records.append((name, flops, e0, e1, nbytes, side, tag))

    def summary(self, name):
        """(launches, total algorithmic flops, total milliseconds) -- call after a device sync."""
        rec = [r for r in self.records if r[0] == name]
        return len(rec), sum(r[1] for r in rec), sum(r[2].elapsed_time(r[3]) for r in rec)

    def total_bytes(self, name):
        """Algorithmic bytes (inputs read once + outputs written once) of the launches called `name`."""
        return sum(r[4] for r in self.records if r[0] == name)

    def total_side_bytes(self, name):
        """The other operands of the same launches, each counted once: weights (split-bf16: 4 bytes per element), the residual,
        the pre-activation addend (`pre`: one image per `pre_div` outputs) and the old output of an accumulating launch."""
        return sum(r[5] for r in self.records if r[0] == name)


KERNEL_TIMER = None  # set to a KernelTimer() to time conv launches
# Packed split-bf16 intermediates in the conv -> conv chains of the InterBlocks (P8Act): 49|99 -> 128 -> 64 -> 32 -> heads.  Bit-identical
# to fp32 intermediates.  ON since round 4: the consumers stage by LDS-DMA with no conversion (128->64 at
# 256^2 298 -> 382 TFLOP/s on the 512-pixel tile, 64->32 205 -> 250), the producers' packed epilogue no longer waits on vector memory
# between its stores (it cost them 20 % in round 3: that, not the format, made P8 a net loss then); a BAIR batch's convolutions 617 ->
# 570 ms alone, the default bench line 190.7 -> 200.4 frames/s on one box (profiles/r04_conv_p8_ab.txt).
CONV_P8 = True
# The back-warp in front of the first Subpixel convolution does NOT write that convolution's packed input (`backwarp_p8`, an entry
# point the decoder does not call): the convolution gains (99->128 at 256^2 268 -> 306 TFLOP/s, 13 ms per decode) what the packed
# back-warp loses (3.85 against 2.9 ms per 120 x 96 x 256^2 call in its best form of three -- one pixel per lane, four pixels per
# lane, four pixels + LDS transposition); the line 197.0 against 197.1 frames/s (profiles/r04_p8_warp_ab.txt)


def conv_persistent_tiles(mode=-1):
    """Which 3 x 3 layers of the split-bf16 convolution run as resident workgroups (`ccvs_conv_persistent_tiles`: bit 0 fp32-input
    128-channel layers, bit 1 packed-input layers); process-wide, returns the previous mode (mode < 0: query).  The library's default
    is 1; `helpers/pipeline.py` sets 0 while a run has several batches in flight.  `CCVS_CONV_PT` in the environment overrides both."""
    return int(_lib.load().ccvs_conv_persistent_tiles(int(mode)))


def conv_last_launch():
    """Which kernel the calling thread's last successful convolution call launched (`ccvs_conv_last_launch`, host code only): e.g.
    `pc TW=32 MB=2 NTY=3 PP=4 WPC=1 ktail=2 chunks=1 xcd=1 zi=0`, `sync TW=16 MB=1 chunks=1 xcd=0 zi=0`,
    `pt MB=4 PP=2 p8in=0 ktail=3 xcd=1 zi=0`, `f32 TW=8 MB=2`; "" before the first one.  Tests assert it per case."""
    return _lib.load().ccvs_conv_last_launch().decode()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.CcvsError("ccvs_amd ops need device tensors: the HIP path has no CPU fallback")


def _rows_dense(t):
    return t.stride(-1) == 1 and t.stride(-2) == t.shape[-1]


def _as_rows_dense(t):
    return t if _rows_dense(t) else t.contiguous()


# ------------------------------------------------------------------ convolution
# Arithmetic of the convolution kernels:
#   "bf16x3": split-bf16, 3 products per fp32 product on v_mfma_f32_32x32x16_bf16 (default)
#   "f32"   : exact fp32 on v_mfma_f32_32x32x2_f32
CONV_PRECISION = "bf16x3"
# Explicit `ccvs_conv_desc.cu_limit` of the convolution launches (0 = the budget of the stream, see `stream_cu_limit`); tests.
CONV_CU_LIMIT = 0


class PackedConv:
    """Kernel-ready weights of one convolution (built once per parameter version).  `ktail`: the same weights with the
    last 16-channel chunk in the packed-tail order (`ccvs_conv_desc.w_ktail`), or None."""
    __slots__ = ("kind", "data", "cin", "cout", "cout_pad", "k", "kw", "ktail")

    def __init__(self, kind, data, cin, cout, cout_pad, k, kw=None, ktail=None):
        self.kind, self.data, self.cin, self.cout, self.cout_pad, self.k = kind, data, cin, cout, cout_pad, k
        self.kw = k if kw is None else kw
        self.ktail = ktail


class P8Act:
    """A split-bf16 packed activation (`ccvs_conv_desc.in_p8 / out_p8`): logical [n, c, h, w] fp32 values stored as
    [n][c/8][hi|lo][h][w] units of 8 bf16 -- what the convolution kernel stages in LDS, so a conv -> conv chain moves its
    intermediate tensors with no conversion work.  `data` is an opaque float32 buffer of n*c*h*w elements."""
    __slots__ = ("data", "n", "c", "h", "w")

    def __init__(self, data, n, c, h, w):
        self.data, self.n, self.c, self.h, self.w = data, n, c, h, w

    @property
    def shape(self):
        return (self.n, self.c, self.h, self.w)

    def float(self):
        """Decode to an fp32 [n,c,h,w] tensor (hi + lo) -- tests / debugging only."""
        u = self.data.view(torch.bfloat16).view(self.n, self.c // 8, 2, self.h, self.w, 8).float()
        v = u[:, :, 0] + u[:, :, 1]                                   # [n, g, h, w, 8]
        return v.permute(0, 1, 4, 2, 3).reshape(self.n, self.c, self.h, self.w).contiguous()


def pack_conv_weight(weight, precision=None, scale=None):
    """[Cout,Cin,k,k] parameter -> PackedConv, with the EqualConv2d scale 1/sqrt(Cin*k*k) multiplied in
    first (the same fp32 product as `weight * scale`, skip_autoencoder.py:44,55,58).
      f32   : [k*k][Cin][CoutPad] fp32
      bf16x3: [k*k][CinPad/8][hi|lo][CoutPad][8] bf16, w = hi + lo (both round-to-nearest-even)"""
    precision = precision or CONV_PRECISION
    cout, cin, kh, kw = weight.shape
    if scale is None:
        scale = 1 / math.sqrt(cin * kh * kw)
    w = (weight.detach().float() * scale).permute(2, 3, 1, 0).reshape(kh * kw, cin, cout)
    if precision == "f32":
        cpad = -(-cout // 64) * 64 if cout >= 64 else 32 * (-(-cout // 32))
        out = torch.zeros(kh * kw, cin, cpad, dtype=torch.float32, device=weight.device)
        out[:, :, :cout] = w
        return PackedConv("f32", out.contiguous(), cin, cout, cpad, kh, kw)
    if precision != "bf16x3":
        raise ValueError(f"unknown conv precision {precision!r}")
    cpad = 32 * (-(-cout // 32))
    cinp = 16 * (-(-cin // 16))
    full = torch.zeros(kh * kw, cinp, cpad, dtype=torch.float32, device=weight.device)
    full[:, :cin, :cout] = w
    hi = full.to(torch.bfloat16)
    lo = (full - hi.float()).to(torch.bfloat16)
    lay = lambda t: t.view(kh * kw, cinp // 8, 8, cpad).permute(0, 1, 3, 2)
    out = torch.stack([lay(hi), lay(lo)], dim=2).contiguous()  # [tap][cg][2][cpad][8]
    ktail = None
    r = cin % 16
    if kh == 3 and kw == 3 and 1 <= r <= 3 and cin > 16:
        # Packed K tail (include/ccvs_hip.h, ccvs_conv_desc.w_ktail): the last chunk's 9 taps x r channels as ceil(9r/16)
        # steps whose K position kk of step j holds (tap t, channel c) with 16 j + kk = t r + c; rest of the chunk zero.
        tail = torch.zeros(kh * kw, 16, cpad, dtype=torch.float32, device=weight.device)   # [tap slot j][kk][cout]
        q = torch.arange(9 * r, device=weight.device)
        tail.view(-1, cpad)[q] = full[q // r, cin - r + q % r]
        full_t = full.clone()
        full_t[:, cinp - 16:] = tail
        hi_t = full_t.to(torch.bfloat16)
        lo_t = (full_t - hi_t.float()).to(torch.bfloat16)
        ktail = torch.stack([lay(hi_t), lay(lo_t)], dim=2).contiguous()
    return PackedConv("bf16x3", out, cin, cout, cpad, kh, kw, ktail=ktail)


def conv2d(x, w_packed, bias, cout, k, stride=1, pad=0, transposed=False, act=False, residual=None,
           out_scale=1.0, out=None, accumulate=False, pre=None, pre_div=1, out_p8=False):
    """y = [y +] (act(conv(x) [+ pre[n // pre_div]] + bias) [+ residual]) * out_scale.
    x may be a P8Act (packed split-bf16 input); out_p8=True returns one (split-bf16 kernel only)."""
    in_p8 = isinstance(x, P8Act)
    if in_p8:
        _need_gpu(x.data, w_packed.data, bias, residual, out, pre)
        assert w_packed.kind == "bf16x3" and stride == 1 and not transposed
    else:
        _need_gpu(x, w_packed.data, bias, residual, out, pre)
        x = _as_rows_dense(x)
    n, cin, h, w = x.shape
    assert w_packed.k == k and w_packed.cin == cin and w_packed.cout == cout, (w_packed.k, w_packed.cin, w_packed.cout, k, cin, cout)
    kw = w_packed.kw
    if transposed:
        ho, wo = 2 * h + k - 2, 2 * w + k - 2
    else:
        ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - kw) // stride + 1
    dev = x.data.device if in_p8 else x.device
    if out_p8:
        assert w_packed.kind == "bf16x3" and cout % 8 == 0 and residual is None and not accumulate
        if out is None:
            out = torch.empty(n * cout * ho * wo, dtype=torch.float32, device=dev)
        else:   # the packed buffer itself (tests hand in a poisoned one): opaque float32, n*cout*ho*wo elements
            assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n * cout * ho * wo, (out.shape, (n, cout, ho, wo))
    elif out is None:
        out = torch.empty(n, cout, ho, wo, dtype=torch.float32, device=dev)
    if not out_p8:
        assert out.shape == (n, cout, ho, wo) and _rows_dense(out), (out.shape, (n, cout, ho, wo))
    d = _lib.ConvDesc()
    d.N, d.Cin, d.Hin, d.Win = n, cin, h, w
    d.in_p8, d.out_p8 = (1 if in_p8 else 0), (1 if out_p8 else 0)
    if not in_p8:
        d.in_sN, d.in_sC = x.stride(0), x.stride(1)
    d.Cout, d.CoutPad, d.Hout, d.Wout = cout, w_packed.cout_pad, ho, wo
    if not out_p8:
        d.out_sN, d.out_sC = out.stride(0), out.stride(1)
    if residual is not None:
        residual = _as_rows_dense(residual)
        assert residual.shape == out.shape
        d.res_sN, d.res_sC = residual.stride(0), residual.stride(1)
    if pre is not None:
        pre = _as_rows_dense(pre)
        assert pre.shape == (n // pre_div, cout, ho, wo) and n % pre_div == 0, (pre.shape, out.shape, pre_div)
        d.pre, d.pre_sN, d.pre_sC, d.pre_div = pre.data_ptr(), pre.stride(0), pre.stride(1), pre_div
    d.kh, d.kw = k, kw
    d.stride, d.pad, d.transposed = stride, pad, 1 if transposed else 0
    d.act = ACT_LRELU if act else ACT_NONE
    d.accumulate = 1 if accumulate else 0
    d.out_scale = out_scale
    d.cu_limit = CONV_CU_LIMIT
    kt = getattr(w_packed, "ktail", None)
    if kt is not None and stride == 1 and not transposed and not in_p8:
        d.w_ktail = kt.data_ptr()
    L = _lib.load()
    prof = KERNEL_TIMER
    if prof is not None:
        macs = n * cout * cin * k * kw * (h * w if transposed else ho * wo)
        side = 4.0 * (cin * cout * k * kw + n * cout * ho * wo * ((residual is not None) + bool(accumulate))
                      + (n // pre_div * cout * ho * wo if pre is not None else 0))
        prof.begin("conv2d_" + w_packed.kind, flops=2.0 * macs, nbytes=4.0 * (n * cin * h * w + n * cout * ho * wo), side=side,
                   tag=(n, cin, h, w, cout, k, kw, stride, int(bool(transposed)), int(in_p8), int(bool(out_p8)), int(pre is not None),
                        int(residual is not None), int(bool(accumulate))))
    fn = L.ccvs_conv2d if w_packed.kind == "f32" else L.ccvs_conv2d_bf16x3
    _lib.check(fn(_p(x.data if in_p8 else x), _p(w_packed.data), _p(bias), _p(residual), _p(out), C.byref(d), _stream()),
               "ccvs_conv2d[" + w_packed.kind + "]")
    if prof is not None:
        prof.end()
    return P8Act(out, n, cout, ho, wo) if out_p8 else out


def pack_head_weights(flow_w, occ_w, precision=None):
    """flow_head [2,C,k,k] + occ_head [1,C,k,k] -> PackedConv of an equivalent convolution with 3k outputs whose second
    half is ccvs_tap_shift_add: split-bf16: a 1 x k kernel (row ky*3+co = tap row ky of output co; all k taps of a row
    in one step of the kernel); f32: a k x 1 kernel (row kx*3+co = tap column kx of output co)."""
    precision = precision or CONV_PRECISION
    w = torch.cat([flow_w.detach(), occ_w.detach()], dim=0).float()          # [3, C, k(y), k(x)]
    _, cin, k, _ = w.shape
    if precision == "bf16x3":
        wt = w.permute(2, 0, 1, 3).reshape(3 * k, cin, 1, k).contiguous()      # [(ky,co), C, 1, kx]
    else:
        wt = w.permute(3, 0, 1, 2).reshape(3 * k, cin, k, 1).contiguous()      # [(kx,co), C, ky, 1]
    return pack_conv_weight(wt, precision, scale=1 / math.sqrt(cin * k * k))


def conv_heads(feat, w_packed, bias3, out, accumulate, flops_cb=None):
    """The fused flow/occ heads: MFMA convolution to 3k maps, then the tap sum along the other axis into
    `out` ([N,3,H,W] view, batch stride free)."""
    vertical = w_packed.k == 1 and w_packed.kw > 1
    k = w_packed.kw if vertical else w_packed.k
    n, _, h, w = feat.shape
    t = conv2d(feat, w_packed, None, 3 * k, w_packed.k, pad=k // 2)             # [N,3k,H+k-1,W] or [N,3k,H,W+k-1]
    assert out.shape == (n, 3, h, w) and _planes_dense(out)
    L = _lib.load()
    _lib.check(L.ccvs_tap_shift_add(_p(t), _p(bias3), _p(out), out.stride(0), n, k, h, w, 1 if accumulate else 0,
                                    1 if vertical else 0, _stream()), "ccvs_tap_shift_add")
    return out


# ------------------------------------------------------------------ resampling
def upfirdn2d(x, up=1, down=1, pad=(0, 0), gain=1.0, act=False, residual=None, out_scale=1.0, out=None):
    """(act(upfirdn2d(x, outer([1,3,3,1]) / 64 * gain, up, down, pad)) [+ residual]) * out_scale (`ccvs_upfirdn2d`).
    out: optional contiguous fp32 [N,C,Ho,Wo] tensor to write into (default: a new one)."""
    _need_gpu(x, residual, out)
    x = x.contiguous()
    n, c, h, w = x.shape
    ho = (h * up + pad[0] + pad[1] - 4) // down + 1
    wo = (w * up + pad[0] + pad[1] - 4) // down + 1
    y = torch.empty(n, c, ho, wo, dtype=torch.float32, device=x.device) if out is None else out
    assert y.shape == (n, c, ho, wo) and y.is_contiguous() and y.dtype == torch.float32, (tuple(y.shape), (n, c, ho, wo))
    if residual is not None:
        residual = residual.contiguous()
        assert residual.shape == y.shape
    L = _lib.load()
    _lib.check(L.ccvs_upfirdn2d(_p(x), _p(y), _p(residual), n * c, h, w, up, down, pad[0], pad[1], gain,
                                ACT_LRELU if act else ACT_NONE, out_scale, _stream()), "ccvs_upfirdn2d")
    return y


def _planes_dense(t):
    """[N,C,H,W] whose channel planes are dense and consecutive (only the batch stride is free)."""
    return _rows_dense(t) and (t.shape[1] == 1 or t.stride(1) == t.shape[2] * t.shape[3])


def dwconvT4x4s2(x, w, out=None):
    _need_gpu(x, w, out)
    if not _planes_dense(x):
        x = x.contiguous()
    n, c, h, ww = x.shape
    if out is None:
        out = torch.empty(n, c, 2 * h, 2 * ww, dtype=torch.float32, device=x.device)
    assert out.shape == (n, c, 2 * h, 2 * ww) and _planes_dense(out)
    L = _lib.load()
    _lib.check(L.ccvs_dwconvT4x4s2(_p(x), x.stride(0), _p(w.contiguous()), _p(out), out.stride(0), n, c, h, ww, _stream()),
               "ccvs_dwconvT4x4s2")
    return out


def gaussian_kernel1d(k, sigma):
    """torchvision's `_get_gaussian_kernel1d` (0.8.1): float32 linspace / exp / sum, normalised."""
    half = (k - 1) * 0.5
    x = torch.linspace(-half, half, steps=k)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return pdf / pdf.sum()


def gaussian_blur(x, k, sigma, out=None):
    """transforms.GaussianBlur(kernel_size=k, sigma=sigma)(x) of [N,C,H,W] fp32 (helpers/generator.py:381-390 `blur`): reflect
    padding, the separable k x k Gaussian (`ccvs_gaussian_blur`).  x may have any batch / channel strides; the result is contiguous.
    out: optional contiguous fp32 [N,C,H,W] tensor to write into (default: a new one)."""
    _need_gpu(x, out)
    assert x.dtype == torch.float32 and x.dim() == 4
    if not _rows_dense(x):
        x = x.contiguous()
    n, c, h, w = x.shape
    wt = gaussian_kernel1d(int(k), float(sigma))
    wbuf = (C.c_float * int(k))(*wt.tolist())
    if out is None:
        out = torch.empty(n, c, h, w, dtype=torch.float32, device=x.device)
    assert out.shape == (n, c, h, w) and out.is_contiguous() and out.dtype == torch.float32
    _lib.check(_lib.load().ccvs_gaussian_blur(_p(x), x.stride(0), x.stride(1), _p(out), n, c, h, w, int(k), wbuf, _stream()),
               "ccvs_gaussian_blur")
    return out


def to_rgb(x, w_scaled, b_conv, bias, skip=None, out=None):
    """ToRGB.forward(x, skip) of the skip_rgb head (skip_autoencoder.py:298-306), one `ccvs_to_rgb` launch:
    ((conv1x1(x, w_scaled) + b_conv) + bias) + Upsample(skip).  x [N,C,H,W] (channel planes dense, any batch stride); w_scaled
    [3,C] = EqualConv2d weight * scale; b_conv [3]; bias [3] or [1,3,1,1]; skip [N,3,H/2,W/2] or None.  Returns [N,3,H,W]."""
    _need_gpu(x, w_scaled, b_conv, bias, skip, out)
    assert x.dtype == torch.float32 and x.dim() == 4
    if not _planes_dense(x):
        x = x.contiguous()
    n, c, h, w = x.shape
    assert w_scaled.shape == (3, c) and w_scaled.is_contiguous() and b_conv.numel() == 3 and bias.numel() == 3
    if skip is not None:
        skip = skip.contiguous()
        assert skip.shape == (n, 3, h // 2, w // 2) and h % 2 == 0 and w % 2 == 0, (tuple(skip.shape), tuple(x.shape))
    if out is None:
        out = torch.empty(n, 3, h, w, dtype=torch.float32, device=x.device)
    assert out.shape == (n, 3, h, w) and out.is_contiguous()
    _lib.check(_lib.load().ccvs_to_rgb(_p(x), x.stride(0), _p(w_scaled), _p(b_conv.contiguous()), _p(bias.contiguous()), _p(skip),
                                       _p(out), n, c, h, w, _stream()), "ccvs_to_rgb")
    return out


def channel_head(x, weight, scale, bias=None, act=True, tanh=False, out=None):
    """A 1 x 1 EqualConv2d to ONE channel with its epilogue, one `ccvs_channel_head` launch (the StftDecoder's last ConvLayer and the
    tanh behind it, skip_autoencoder.py:550,555): tanh(lrelu(bias + sum_c (weight[c] * scale) x[:, c])), the LeakyReLU(0.1) with `act`,
    the tanh with `tanh`.  x [N,C,H,W] (channel planes dense, any batch stride); weight: C values ([1,C,1,1] or [C]); bias [1] or None.
    Returns [N,1,H,W]."""
    _need_gpu(x, weight, bias, out)
    assert x.dtype == torch.float32 and x.dim() == 4 and weight.dtype == torch.float32
    if not _planes_dense(x):
        x = x.contiguous()
    n, c, h, w = x.shape
    assert weight.numel() == c and weight.is_contiguous() and (bias is None or bias.numel() == 1), (tuple(weight.shape), c)
    if out is None:
        out = torch.empty(n, 1, h, w, dtype=torch.float32, device=x.device)
    assert out.shape == (n, 1, h, w) and out.is_contiguous() and out.dtype == torch.float32
    _lib.check(_lib.load().ccvs_channel_head(_p(x), x.stride(0), _p(weight), float(scale), _p(bias), _p(out), n, c, h, w,
                                             1 if act else 0, 1 if tanh else 0, _stream()), "ccvs_channel_head")
    return out


# ------------------------------------------------------------------ cost volume / warp
def correlation7x7(first, second, stride, first_div=1, lrelu=False, out=None):
    """The 7 x 7 cost volume [N,49,ceil(H/stride),ceil(W/stride)] of second [N,C,H,W] against first [N/first_div,C,H,W]
    (`ccvs_correlation7x7`), LeakyReLU(0.1) with `lrelu`.  out: optional contiguous fp32 tensor of that shape to write into
    (default: a new one)."""
    _need_gpu(first, second, out)
    first, second = first.contiguous(), second.contiguous()
    n, c, h, w = second.shape
    assert first.shape[0] * first_div == n and first.shape[1:] == second.shape[1:]
    ho, wo = -(-h // stride), -(-w // stride)
    if out is None:
        out = torch.empty(n, 49, ho, wo, dtype=torch.float32, device=second.device)
    assert out.shape == (n, 49, ho, wo) and out.is_contiguous() and out.dtype == torch.float32
    L = _lib.load()
    _lib.check(L.ccvs_correlation7x7(_p(first), _p(second), _p(out), n, c, h, w, stride, first_div, 1 if lrelu else 0, _stream()),
               "ccvs_correlation7x7")
    return out


def _ctx_list(ctxs):
    """k context tensors [N,C,H,W] (channel planes dense, any batch stride) -> (`ccvs_ctx_list`, tensors kept alive)."""
    assert 1 <= len(ctxs) <= _lib.MAX_CTX
    cl = _lib.CtxList()
    cl.k = len(ctxs)
    keep = []
    n, c, h, w = ctxs[0].shape
    for j, t in enumerate(ctxs):
        _need_gpu(t)
        assert t.shape == (n, c, h, w) and t.dtype == torch.float32
        if not (t.stride(3) == 1 and t.stride(2) == w and t.stride(1) == h * w):
            t = t.contiguous()
        keep.append(t)
        cl.p[j] = t.data_ptr()
        cl.sN[j] = t.stride(0)
    return cl, keep


def backwarp(x, flow, flow_mult=1.0, out=None):
    """x: a tensor [N,C,H,W], or a LIST of k context tensors [N/k,C,H,W] standing for the batch of N pairs in (frame, context)
    order -- read in place, no stacked copy."""
    _need_gpu(flow, out)
    if not _planes_dense(flow):
        flow = flow.contiguous()
    L = _lib.load()
    if isinstance(x, (list, tuple)):
        cl, keep = _ctx_list(x)
        nf, c, h, w = keep[0].shape
        n = nf * cl.k
        assert flow.shape == (n, 2, h, w)
        if out is None:
            out = torch.empty(n, c, h, w, dtype=torch.float32, device=flow.device)
        assert _rows_dense(out)
        _lib.check(L.ccvs_backwarp_ctx(C.byref(cl), h * w, _p(flow), flow.stride(0), flow_mult, _p(out), out.stride(0), out.stride(1),
                                       n, c, h, w, _stream()), "ccvs_backwarp_ctx")
        return out
    _need_gpu(x)
    x = _as_rows_dense(x)
    n, c, h, w = x.shape
    assert flow.shape == (n, 2, h, w)
    if out is None:
        out = torch.empty(n, c, h, w, dtype=torch.float32, device=x.device)
    assert _rows_dense(out)
    _lib.check(L.ccvs_backwarp(_p(x), x.stride(0), x.stride(1), _p(flow), flow.stride(0), flow_mult, _p(out), out.stride(0),
                               out.stride(1), n, c, h, w, _stream()), "ccvs_backwarp")
    return out


def pack_proj_weight(weight):
    """1x1 EqualConv2d weight [Cout,Cin,1,1] -> (w_t [Cin][CoutPad] with the 1/sqrt(Cin) scale multiplied in, CoutPad) for
    `backwarp_proj`; None when Cout has no instantiation."""
    cout, cin = weight.shape[:2]
    pads = [p_ for p_ in (16, 24, 48, 96) if p_ >= cout]
    if not pads:
        return None
    w = (weight.detach().float().view(cout, cin) * (1 / math.sqrt(cin))).t()
    out = torch.zeros(cin, pads[0], dtype=torch.float32, device=weight.device)
    out[:, :cout] = w
    return out.contiguous(), pads[0]


def backwarp_p8(ctxs, flow_occ, flow_mult, out=None):
    """[backwarp(ctx, flow * flow_mult) | flow | occ | 0 x 5] for the list of k context tensors [N/k,C,H,W] (see `backwarp`) as a P8Act of
    C + 8 channels (`ccvs_backwarp_p8_ctx`): the packed input of the first Subpixel convolution.  flow_occ: [N,3,H,W].
    out: optional flat contiguous float32 buffer of N (C + 8) H W elements that becomes the P8Act's `data` (default: a new one)."""
    _need_gpu(flow_occ, out)
    if not _planes_dense(flow_occ):
        flow_occ = flow_occ.contiguous()
    cl, keep = _ctx_list(ctxs)
    nf, c, h, w = keep[0].shape
    n = nf * cl.k
    assert flow_occ.shape == (n, 3, h, w) and c % 8 == 0 and w % 4 == 0
    if out is None:
        out = torch.empty(n * (c + 8) * h * w, dtype=torch.float32, device=flow_occ.device)
    assert out.shape == (n * (c + 8) * h * w,) and out.is_contiguous() and out.dtype == torch.float32
    L = _lib.load()
    _lib.check(L.ccvs_backwarp_p8_ctx(C.byref(cl), h * w, _p(flow_occ), flow_occ.stride(0), flow_mult, _p(out), n, c, h, w, _stream()),
               "ccvs_backwarp_p8_ctx")
    return P8Act(out, n, c + 8, h, w)


def backwarp_proj(ctxs, flow, flow_mult, w_t, cout_pad, bias, cout, act=True, out=None):
    """act(bias + W . backwarp(ctx, flow * flow_mult)) for the list of k context tensors [N/k,C,H,W] (see `backwarp`):
    [N,cout,H,W], the warped tensor is never materialised (`ccvs_backwarp_proj_ctx`).  out: optional contiguous fp32 [N,cout,H,W]
    tensor to write into (default: a new one)."""
    _need_gpu(flow, w_t, bias, out)
    if not _planes_dense(flow):
        flow = flow.contiguous()
    cl, keep = _ctx_list(ctxs)
    nf, c, h, w = keep[0].shape
    n = nf * cl.k
    assert flow.shape == (n, 2, h, w) and w_t.shape == (c, cout_pad)
    if out is None:
        out = torch.empty(n, cout, h, w, dtype=torch.float32, device=flow.device)
    assert out.shape == (n, cout, h, w) and out.is_contiguous() and out.dtype == torch.float32
    L = _lib.load()
    _lib.check(L.ccvs_backwarp_proj_ctx(C.byref(cl), h * w, _p(flow), flow.stride(0), flow_mult, _p(w_t), _p(bias), _p(out), n, c, cout, cout_pad,
                                        h, w, ACT_LRELU if act else ACT_NONE, _stream()), "ccvs_backwarp_proj_ctx")
    return out


def warp_fuse_blend(dec, ctx, flows, occs, flow_mult, k):
    """In place on `dec` (a channel-slice view [N,C,H,W] of the decoder feature).  ctx: [N*k,C,H,W], or a list of k
    context tensors [N,C,H,W] read in place."""
    _need_gpu(dec, flows, occs)
    assert _rows_dense(dec)
    flows = flows if _planes_dense(flows) else flows.contiguous()
    occs = occs if _planes_dense(occs) else occs.contiguous()
    n, c, h, w = dec.shape
    assert flows.shape == (n * k, 2, h, w) and occs.shape == (n * k, 1, h, w)
    L = _lib.load()
    if isinstance(ctx, (list, tuple)):
        cl, keep = _ctx_list(ctx)
        assert cl.k == k and keep[0].shape == (n, c, h, w)
        _lib.check(L.ccvs_warp_fuse_blend_ctx(_p(dec), dec.stride(0), dec.stride(1), C.byref(cl), _p(flows), flows.stride(0), _p(occs),
                                              occs.stride(0), flow_mult, n, c, h, w, _stream()), "ccvs_warp_fuse_blend_ctx")
        return dec
    _need_gpu(ctx)
    ctx = ctx.contiguous()
    assert ctx.shape == (n * k, c, h, w)
    _lib.check(L.ccvs_warp_fuse_blend(_p(dec), dec.stride(0), dec.stride(1), _p(ctx), _p(flows), flows.stride(0), _p(occs),
                                      occs.stride(0), flow_mult, n, k, c, h, w, _stream()), "ccvs_warp_fuse_blend")
    return dec


# ------------------------------------------------------------------ Matching variants
def pack_deform_weight(weight, precision=None):
    """DeformConv2d weight [C,C,3,3] (plain, no EqualConv2d scale) -> PackedConv in the convolution's layout for `deform_conv3x3`."""
    return pack_conv_weight(weight, precision, scale=1.0)


def deform_conv3x3(ctxs, flow, flow_mult, w_packed, bias, occ=None, toff=None, act=False):
    """torchvision.ops.DeformConv2d(C, C, 3, padding=1) of the list of k context tensors [N/k,C,H,W] (see `backwarp`) with one offset per
    pixel, flow * flow_mult read as (row, column) offsets -- Matching's `deform(inter, offset)` (`ccvs_deform_conv3x3_ctx`), then
    [* (1 - sigmoid(occ))] [+ toff] [LeakyReLU(0.1)] in its epilogue.  flow [N,2,H,W], occ [N,1,H,W], toff [N,C,H,W]: [N,C,H,W]."""
    _need_gpu(flow, w_packed.data, bias, occ, toff)
    if not _planes_dense(flow):
        flow = flow.contiguous()
    if occ is not None and not _planes_dense(occ):
        occ = occ.contiguous()
    if toff is not None:
        toff = _as_rows_dense(toff)
    cl, keep = _ctx_list(ctxs)
    nf, c, h, w = keep[0].shape
    n = nf * cl.k
    assert flow.shape == (n, 2, h, w) and w_packed.k == 3 and w_packed.kw == 3 and w_packed.cin == c and w_packed.cout == c
    assert occ is None or occ.shape == (n, 1, h, w)
    assert toff is None or toff.shape == (n, c, h, w)
    out = torch.empty(n, c, h, w, dtype=torch.float32, device=flow.device)
    prec = {"f32": 0, "bf16x3": 1}[w_packed.kind]
    prof = KERNEL_TIMER
    if prof is not None:
        prof.begin("deform_" + w_packed.kind, flops=2.0 * n * c * c * 9 * h * w, nbytes=4.0 * (2 * n * c * h * w + 2 * n * h * w),
                   side=4.0 * 9 * c * c, tag=(n, c, h, w))
    L = _lib.load()
    _lib.check(L.ccvs_deform_conv3x3_ctx(C.byref(cl), h * w, _p(flow), flow.stride(0), float(flow_mult), _p(w_packed.data), w_packed.cout_pad,
                                         prec, _p(bias), _p(occ), occ.stride(0) if occ is not None else 0, _p(toff),
                                         toff.stride(0) if toff is not None else 0, toff.stride(1) if toff is not None else 0, _p(out),
                                         out.stride(0), out.stride(1), n, c, h, w, ACT_LRELU if act else ACT_NONE, _stream()),
               "ccvs_deform_conv3x3_ctx")
    if prof is not None:
        prof.end()
    return out


def gconvT4x4s2(x, w, out=None):
    """nn.ConvTranspose2d(G, G * mult, 4, stride=2, padding=1, groups=G, bias=False) with weight w [G, mult, 4, 4] (Matching.upsample_toff):
    x [N,G,H,W] -> [N,G*mult,2H,2W] (`ccvs_gconvT4x4s2`)."""
    _need_gpu(x, w, out)
    if not _planes_dense(x):
        x = x.contiguous()
    n, g, h, ww = x.shape
    assert w.shape[0] == g and w.shape[2:] == (4, 4)
    mult = w.shape[1]
    if out is None:
        out = torch.empty(n, g * mult, 2 * h, 2 * ww, dtype=torch.float32, device=x.device)
    assert out.shape == (n, g * mult, 2 * h, 2 * ww) and _rows_dense(out)
    L = _lib.load()
    _lib.check(L.ccvs_gconvT4x4s2(_p(x), x.stride(0), _p(w.detach().contiguous()), _p(out), out.stride(0), out.stride(1), n, g, mult, h, ww,
                                  _stream()), "ccvs_gconvT4x4s2")
    return out


def flow_mask_toff_(x, occ=None, toff=None, act=False):
    """In place on x [N,C,H,W]: x = act(x [* (1 - sigmoid(occ))] [+ toff]) -- Matching's masked-flow / trade-off steps after the plain
    back-warp (`ccvs_flow_mask_toff`)."""
    _need_gpu(x, occ, toff)
    assert _rows_dense(x)
    n, c, h, w = x.shape
    if occ is not None:
        occ = occ if _planes_dense(occ) else occ.contiguous()
        assert occ.shape == (n, 1, h, w)
    if toff is not None:
        toff = _as_rows_dense(toff)
        assert toff.shape == (n, c, h, w)
    L = _lib.load()
    _lib.check(L.ccvs_flow_mask_toff(_p(x), x.stride(0), x.stride(1), _p(occ), occ.stride(0) if occ is not None else 0, _p(toff),
                                     toff.stride(0) if toff is not None else 0, toff.stride(1) if toff is not None else 0, n, c, h, w,
                                     ACT_LRELU if act else ACT_NONE, _stream()), "ccvs_flow_mask_toff")
    return x


# ------------------------------------------------------------------ vector quantiser
def vq_argmin(z, codebook_t, e_sq):
    """z [N,C,H,W] -> int64 [N*H*W] (n,h,w raster order)."""
    _need_gpu(z, codebook_t, e_sq)
    z = z.contiguous()
    n, c = z.shape[:2]
    hw = z.shape[2] * z.shape[3]
    idx = torch.empty(n * hw, dtype=torch.int64, device=z.device)
    L = _lib.load()
    _lib.check(L.ccvs_vq_argmin(_p(z), _p(codebook_t), _p(e_sq), _p(idx), n, c, hw, codebook_t.shape[1], _stream()), "ccvs_vq_argmin")
    return idx


def embed_gather(code, codebook, n, hw):
    """code int64 [n*hw] -> z [n, C, hw]."""
    _need_gpu(code, codebook)
    code = code.contiguous()
    n_e, c = codebook.shape
    z = torch.empty(n, c, hw, dtype=torch.float32, device=codebook.device)
    L = _lib.load()
    _lib.check(L.ccvs_embed_gather(_p(code), _p(codebook), _p(z), n, c, hw, n_e, _stream()), "ccvs_embed_gather")
    return z


def l2_normalize_channels_(x):
    """x [n, C, h, w] (dense) /= its L2 norm over the channels, in place (`normalize_out`, skip_autoencoder.py:348-349)."""
    _need_gpu(x)
    assert x.is_contiguous() and x.dtype == torch.float32 and x.dim() == 4
    n, c, h, w = x.shape
    L = _lib.load()
    _lib.check(L.ccvs_l2_normalize_channels(_p(x), n, c, h * w, _stream()), "ccvs_l2_normalize_channels")
    return x


# ------------------------------------------------------------------ transformer
def gpt_embed(idx, tok_emb, pos_table, pos0=0, pos_off=None, pos_dev=None):
    """idx int64 [B,Tq] (row stride free) -> x [B*Tq, C]; positional row = pos_off[b] + pos0 (+ *pos_dev) + t."""
    _need_gpu(idx, pos_off, tok_emb, pos_table, pos_dev)
    b, tq = idx.shape
    assert idx.stride(1) == 1 or tq == 1
    c = tok_emb.shape[1]
    x = torch.empty(b * tq, c, dtype=torch.float32, device=tok_emb.device)
    L = _lib.load()
    _lib.check(L.ccvs_gpt_embed(_p(idx), idx.stride(0), _p(pos_off), pos0, _p(pos_dev), tq, _p(tok_emb), _p(pos_table), _p(x), b, c,
                                tok_emb.shape[0], _stream()), "ccvs_gpt_embed")
    return x


def layernorm(x, gamma, beta, out=None):
    _need_gpu(x, gamma, beta)
    rows, c = x.shape
    assert x.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    L = _lib.load()
    _lib.check(L.ccvs_layernorm(_p(x), _p(gamma), _p(beta), _p(out), rows, c, _stream()), "ccvs_layernorm")
    return out


def gemm_nt(x, w, bias=None, epilogue=EPI_NONE, residual=None, out=None):
    """y = epilogue(x @ w.T + bias); x [M,K] (row stride free), w [N,K] contiguous."""
    _need_gpu(x, w, bias, residual, out)
    m, k = x.shape
    n = w.shape[0]
    assert x.stride(1) == 1 and w.is_contiguous() and w.shape[1] == k
    if out is None:
        out = torch.empty(m, n, dtype=torch.float32, device=x.device)
    assert out.stride(1) == 1
    if residual is not None:
        assert residual.stride(1) == 1 and residual.stride(0) == out.stride(0)
    L = _lib.load()
    _lib.check(L.ccvs_gemm_nt(_p(x), x.stride(0), _p(w), _p(bias), _p(residual), _p(out), out.stride(0), m, n, k, epilogue,
                              _p(_gemm_workspace(x.device)), _stream()), "ccvs_gemm_nt")  # workspace is per (device, stream)
    return out


_GEMM_WS = {}


def _gemm_workspace(device):
    """Zero-initialised split-K workspace (slabs + arrival counters), one per (device, stream): calls on
    one stream are ordered and the reducer leaves the counters at zero, but two streams (the parallel
    decode lanes of GPT.generate) may run the same GEMM concurrently and must not share slabs."""
    key = (device, torch.cuda.current_stream().cuda_stream)
    ws = _GEMM_WS.get(key)
    if ws is None:
        ws = _GEMM_WS[key] = torch.zeros(int(_lib.load().ccvs_gemm_workspace_bytes()), dtype=torch.uint8, device=device)
    return ws


def pack_ln_linear(weight, bias, gamma, beta):
    """Fold a LayerNorm (gamma, beta) into the Linear (weight [N,K], bias [N]) that follows it:
    returns (W*gamma, bias + W@beta, rowsum(W*gamma)) -- see ccvs_gemm_ln in include/ccvs_hip.h."""
    w = weight.detach().float()
    wg = (w * gamma.detach().float().view(1, -1)).contiguous()
    b = bias.detach().float() if bias is not None else torch.zeros(w.shape[0], device=w.device)
    bb = (b + w.double().matmul(beta.detach().double()).float()).contiguous()
    s = wg.double().sum(dim=1).float().contiguous()
    return wg, bb, s


def gemm_ln(x, wg, bb, s, eps=1e-5, epilogue=EPI_NONE, out=None):
    """epilogue(LayerNorm(x) @ W.T + b) with the LayerNorm folded into (wg, bb, s) = pack_ln_linear(...)."""
    _need_gpu(x, wg, bb, s, out)
    m, k = x.shape
    n = wg.shape[0]
    assert x.stride(1) == 1 and wg.is_contiguous() and wg.shape[1] == k
    if out is None:
        out = torch.empty(m, n, dtype=torch.float32, device=x.device)
    L = _lib.load()
    _lib.check(L.ccvs_gemm_ln(_p(x), x.stride(0), _p(wg), _p(bb), _p(s), eps, _p(out), out.stride(0), m, n, k, epilogue, _stream()),
               "ccvs_gemm_ln")
    return out


def gemm_ln_qkv(x, wg, bb, s, kcache, vcache, b, tq, pos0, pos_dev=None, eps=1e-5, out=None):
    """ln1 + fused QKV projection: returns q [b*tq, C] (`out`, dense, when given); K / V go straight into the caches."""
    _need_gpu(x, wg, bb, s, kcache, vcache, pos_dev, out)
    _need_cache_dtype("gemm_ln_qkv", torch.float32, kcache, vcache)
    c = x.shape[1]
    _, h, tmax, d = kcache.shape
    assert x.shape[0] == b * tq and x.stride(1) == 1 and wg.shape == (3 * c, c) and h * d == c
    q = out if out is not None else torch.empty(b * tq, c, dtype=torch.float32, device=x.device)
    assert q.shape == (b * tq, c) and q.dtype == torch.float32 and q.is_contiguous()   # the C ABI takes q with row stride C
    L = _lib.load()
    _lib.check(L.ccvs_gemm_ln_qkv(_p(x), x.stride(0), _p(wg), _p(bb), _p(s), eps, _p(q), _p(kcache), _p(vcache), b, tq, c, h, pos0,
                                  _p(pos_dev), tmax, _stream()), "ccvs_gemm_ln_qkv")
    return q


def tile_weight(w):
    """W [N,K] -> the tiled layout of the decode GEMMs (include/ccvs_hip_gemm.h, ccvs_gemm_tiled), flat [ceil(N / 16) * 16 * K]: N padded to
    whole column tiles by repeating the last row, then block (ct, kb) of 16 rows x 16 columns = 256 contiguous floats at
    (ct * K / 16 + kb) * 256, float 4 * (li + 16 g) + j of a block = W[16 ct + li][16 kb + 4 g + j]."""
    w = w.detach()
    n, k = w.shape
    assert w.dtype == torch.float32 and k % 16 == 0
    npad = -(-n // 16) * 16
    if npad != n:
        w = torch.cat([w, w[-1:].expand(npad - n, k)], dim=0)
    return w.reshape(npad // 16, 16, k // 16, 4, 4).permute(0, 2, 3, 1, 4).contiguous().view(-1)


def gemm_tiled_max_rows():
    """The most rows of a GEMM -- hence of a decode step -- that reads tiled weights (`ccvs_gemm_tiled_max_rows`)."""
    return int(_lib.load().ccvs_gemm_tiled_max_rows())


def gemm_tiled(x, wt, n, bias=None, epilogue=EPI_NONE, residual=None, out=None, ln_s=None, eps=1e-5, kcache=None, vcache=None, pos0=0,
               pos_dev=None):
    """One decode GEMM on `wt` = tile_weight(W [n,K]) (`ccvs_gemm_tiled`): gemm_nt (ln_s None), gemm_ln (ln_s = the packed row sums,
    bias = the packed bias) or gemm_ln_qkv with one position per row (kcache / vcache given: `out` is q).  Bit-identical to those."""
    _need_gpu(x, wt, bias, residual, out, ln_s, kcache, vcache, pos_dev)
    m, k = x.shape
    assert x.stride(1) == 1 and wt.is_contiguous() and wt.numel() == -(-n // 16) * 16 * k
    if out is None:
        out = torch.empty(m, k if kcache is not None else n, dtype=torch.float32, device=x.device)
    assert out.stride(1) == 1
    if residual is not None:
        assert residual.stride(1) == 1 and residual.stride(0) == out.stride(0)
    h = tmax = 0
    if kcache is not None:
        _, h, tmax, d = kcache.shape
        assert n == 3 * k and h * d == k and out.shape == (m, k) and out.is_contiguous() and kcache.shape[0] == m
    ws = _gemm_workspace(x.device) if ln_s is None else None   # (as gemm_nt / gemm_ln: only the plain form splits K over workgroups)
    L = _lib.load()
    _lib.check(L.ccvs_gemm_tiled(_p(x), x.stride(0), _p(wt), _p(bias), _p(residual), _p(ln_s), eps, _p(out), out.stride(0), m, n, k, epilogue,
                                 _p(kcache), _p(vcache), h, pos0, _p(pos_dev), tmax, _p(ws), _stream()), "ccvs_gemm_tiled")
    return out


def kv_append(k, v, kcache, vcache, pos0, pos_dev=None):
    """k, v [B,Tq,H*D] views (row stride shared) -> caches [B,H,Tmax,D] at pos0 (+ *pos_dev).."""
    _need_cache_dtype("kv_append", torch.float32, kcache, vcache)
    b, tq, hd = k.shape
    _, h, tmax, d = kcache.shape
    assert k.stride(2) == 1 and v.stride() == k.stride()
    L = _lib.load()
    _lib.check(L.ccvs_kv_append(_p(k), _p(v), k.stride(0), k.stride(1), _p(kcache), _p(vcache), b, h, tq, pos0, _p(pos_dev), tmax, d,
                                _stream()), "ccvs_kv_append")


def attention(q, kcache, vcache, pos0, pos_dev=None):
    """q [B,Tq,H*D] view -> out [B,Tq,H*D]; query t sees cache positions 0..pos0(+*pos_dev)+t."""
    _need_cache_dtype("attention", torch.float32, kcache, vcache)
    b, tq, hd = q.shape
    _, h, tmax, d = kcache.shape
    assert q.stride(2) == 1
    out = torch.empty(b, tq, hd, dtype=torch.float32, device=q.device)
    L = _lib.load()
    _lib.check(L.ccvs_attention(_p(q), q.stride(0), q.stride(1), _p(kcache), _p(vcache), _p(out), b, h, tq, pos0, _p(pos_dev), tmax, d,
                                _stream()), "ccvs_attention")
    return out


KV_DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def check_kv_dtype(kv_dtype):
    """The KV cache's element type as torch names it, from "fp32" / "bf16" (`--x_kv_dtype`) or a torch dtype.  ValueError for the rest."""
    if kv_dtype in KV_DTYPES:
        return KV_DTYPES[kv_dtype]
    if kv_dtype in KV_DTYPES.values():
        return kv_dtype
    raise ValueError(f"kv_dtype must be one of {sorted(KV_DTYPES)}, got {kv_dtype!r}")


def _need_cache_dtype(name, want, *caches):
    """An op never reinterprets a cache: the fp32 ops take fp32 caches, the `*_bf16` ops bf16 caches."""
    for c in caches:
        if c.dtype != want:
            raise ValueError(f"{name}: the KV cache is {c.dtype}, this op reads and writes {want} caches")
        if not c.is_contiguous():
            raise ValueError(f"{name}: the KV cache must be contiguous")


def kv_append_bf16(k, v, kcache, vcache, pos0, pos_dev=None):
    """`kv_append` on bf16 caches (`ccvs_kv_append_bf16`, include/ccvs_hip_kv16.h): k, v fp32 [B,Tq,H*D] views (strides shared) are
    rounded to bf16 (round to nearest even: `.to(torch.bfloat16)`) into the caches [B,H,Tmax,D] at pos0 (+ *pos_dev)..; a position at or
    beyond Tmax is skipped."""
    _need_cache_dtype("kv_append_bf16", torch.bfloat16, kcache, vcache)
    _need_gpu(k, v, kcache, vcache, pos_dev)
    if k.dtype != torch.float32 or v.dtype != torch.float32:
        raise ValueError("kv_append_bf16: k and v are the fp32 rows of the QKV GEMM")
    b, tq, hd = k.shape
    _, h, tmax, d = kcache.shape
    assert k.stride(2) == 1 and v.stride() == k.stride() and h * d == hd and kcache.shape == vcache.shape and kcache.shape[0] == b
    L = _lib.load()
    _lib.check(L.ccvs_kv_append_bf16(_p(k), _p(v), k.stride(0), k.stride(1), _p(kcache), _p(vcache), b, h, tq, pos0, _p(pos_dev), tmax, d,
                                     _stream()), "ccvs_kv_append_bf16")


def attention_bf16(q, kcache, vcache, pos0, pos_dev=None, kv_new=None, grp_rows=0):
    """`attention` over bf16 caches (`ccvs_attention_bf16`): q fp32 [B,Tq,H*D] view -> out fp32 [B,Tq,H*D]; every stored value is widened
    exactly and the arithmetic is fp32.  kv_new = (k, v), fp32 [B,1,H*D] views of one stride (Tq = 1 only): the APPENDING decode form --
    the call rounds those rows into the caches at pos0 (+ *pos_dev) and attends to the rounded values; None: the caches hold that position.
    grp_rows > 0 (Tq = 1): row groups of a grouped decode step -- pos_dev is int32 [B / grp_rows], one cache length per group."""
    _need_cache_dtype("attention_bf16", torch.bfloat16, kcache, vcache)
    _need_gpu(q, kcache, vcache, pos_dev)
    if q.dtype != torch.float32:
        raise ValueError("attention_bf16: q is fp32")
    b, tq, hd = q.shape
    _, h, tmax, d = kcache.shape
    assert q.stride(2) == 1 and h * d == hd and kcache.shape == vcache.shape and kcache.shape[0] == b
    kn = vn = None
    kv_sb = 0
    if kv_new is not None:
        kn, vn = kv_new
        _need_gpu(kn, vn)
        if kn.dtype != torch.float32 or vn.dtype != torch.float32:
            raise ValueError("attention_bf16: kv_new holds the fp32 rows of the QKV GEMM")
        if tq != 1:
            raise ValueError("attention_bf16: kv_new is for the decode form (Tq = 1)")
        assert kn.shape == (b, 1, hd) and vn.shape == kn.shape and kn.stride(2) == 1 and vn.stride() == kn.stride()
        kv_sb = kn.stride(0)
    if grp_rows:
        assert pos_dev is not None and pos_dev.dtype == torch.int32 and pos_dev.is_contiguous() and pos_dev.numel() * grp_rows == b
    out = torch.empty(b, tq, hd, dtype=torch.float32, device=q.device)
    L = _lib.load()
    _lib.check(L.ccvs_attention_bf16(_p(q), q.stride(0), q.stride(1), _p(kn), _p(vn), kv_sb, _p(kcache), _p(vcache), _p(out), b, h, tq, pos0,
                                     _p(pos_dev), int(grp_rows), tmax, d, _stream()), "ccvs_attention_bf16")
    return out


def check_top_p(top_p):
    """The nucleus threshold of a sampler: None for "off" (None and 1.0), a float inside (0, 1) otherwise.  ValueError for the rest."""
    if top_p is None:
        return None
    p = float(top_p)
    if p == 1.0:
        return None
    if not 0.0 < p < 1.0:   # (a NaN fails both comparisons)
        raise ValueError(f"top_p must be None, 1.0 (both: off) or inside (0, 1), got {top_p!r}")
    return p


def sample_topp_max_vocab():
    """The largest vocabulary the nucleus form of the pick takes (`ccvs_sample_topp_max_vocab`; host only)."""
    return int(_lib.load().ccvs_sample_topp_max_vocab())


def sample_topk(logits, top_k, temperature, noise=None, out=None, philox=None, *, top_p=None):
    """logits [B,V] -> int64 [B]; noise None = greedy, else argmax(p / noise).  philox = (key0, key1, row0, step, call):
    draw the Exp(1) noise in the kernel, keyed by the global clip index row0 + b (ccvs_sample_topk_philox).
    top_p inside (0, 1): nucleus sampling after the top-k mask (`ccvs_sample_topp` / `ccvs_sample_topp_philox`, include/ccvs_hip_sampling.h);
    None or 1.0: off -- the calls above, as before."""
    top_p = check_top_p(top_p)
    _need_gpu(logits, noise, out)
    b, v = logits.shape
    assert logits.stride(1) == 1
    if out is None:
        out = torch.empty(b, dtype=torch.int64, device=logits.device)
    if top_p is not None:
        L = _lib.load()
        k = 0 if top_k is None else int(top_k)
        if philox is not None:
            assert noise is None
            k0, k1, row0, step, call = (int(t) & 0xffffffff for t in philox)
            _lib.check(L.ccvs_sample_topp_philox(_p(logits), logits.stride(0), _p(out), out.stride(0), b, v, k, float(temperature), top_p,
                                                 k0, k1, row0, step, call, _stream()), "ccvs_sample_topp_philox")
            return out
        if noise is not None:
            assert noise.shape == (b, v) and noise.is_contiguous()
        _lib.check(L.ccvs_sample_topp(_p(logits), logits.stride(0), _p(noise), _p(out), out.stride(0), b, v, k, float(temperature), top_p,
                                      _stream()), "ccvs_sample_topp")
        return out
    if philox is not None:
        assert noise is None
        k0, k1, row0, step, call = (int(t) & 0xffffffff for t in philox)
        L = _lib.load()
        _lib.check(L.ccvs_sample_topk_philox(_p(logits), logits.stride(0), _p(out), out.stride(0), b, v, 0 if top_k is None else int(top_k),
                                             float(temperature), k0, k1, row0, step, call, _stream()), "ccvs_sample_topk_philox")
        return out
    if noise is not None:
        assert noise.shape == (b, v) and noise.is_contiguous()
    L = _lib.load()
    _lib.check(L.ccvs_sample_topk(_p(logits), logits.stride(0), _p(noise), _p(out), out.stride(0), b, v,
                                  0 if top_k is None else int(top_k), float(temperature), _stream()), "ccvs_sample_topk")
    return out


def sample_topn(logits, top_k, temperature, n, noise=None):
    """logits [B,V] -> (picks int64 [B,n], log p float [B,n]): the n best of the top-k softmax (noise None) or of probs / noise
    (torch.multinomial without replacement), best first (`ccvs_sample_topn`: the proposals of beam search)."""
    _need_gpu(logits, noise)
    b, v = logits.shape
    assert logits.stride(1) == 1 and 1 <= n <= v
    if noise is not None:
        assert noise.shape == (b, v) and noise.is_contiguous()
    idx = torch.empty(b, n, dtype=torch.int64, device=logits.device)
    logp = torch.empty(b, n, dtype=torch.float32, device=logits.device)
    L = _lib.load()
    _lib.check(L.ccvs_sample_topn(_p(logits), logits.stride(0), _p(noise), _p(idx), _p(logp), b, v, 0 if top_k is None else int(top_k),
                                  float(temperature), int(n), _stream()), "ccvs_sample_topn")
    return idx, logp


class GptDecodeStep:
    """A filled `ccvs_gpt_decode` descriptor (include/ccvs_hip.h) plus the tensors it points at.
    `launch()` enqueues one whole decode step on the current stream."""

    def __init__(self, layers, B, C, H, Tmax, ln_eps, tok_emb, pos_table, pos_off, head, tok, codes, widx, length,
                 x, q, att, h, logits, noise, top_k, temperature, state, rng=False, groups=1, noise_stream=None, persistent=False,
                 tiled=None, top_p=None, kv_dtype=torch.float32):
        """top_p: nucleus sampling in the step's pick (`ccvs_gpt_decode.top_p`; None or 1.0: off).
        kv_dtype: the type of every layer's kcache / vcache.  bf16: `launch()` calls `ccvs_gpt_decode_step_bf16kv` (include/ccvs_hip_kv16.h),
        `q` is [B,3C] (the whole QKV output of a step), and `persistent` is refused.
        tiled: None, or ([{qkv_w, proj_w, fc_w, fc2_w} per layer], head_w) = `tile_weight` of the matrices in `layers` / `head`: the
        step then reads those (`ccvs_gpt_decode.w_tiled`); the row-major ones still give the shapes."""
        hw, hb, hs = head
        self.kv_dtype = check_kv_dtype(kv_dtype)
        kv16 = self.kv_dtype == torch.bfloat16
        if kv16 and persistent:
            raise ValueError("the persistent decode step (CCVS_DECODE_PERSISTENT=1, `ccvs_gpt_decode.persistent`) reads fp32 KV caches only: "
                             "not together with a bf16 KV cache (--x_kv_dtype bf16)")
        keep = [tok_emb, pos_table, hw, hb, hs, tok, codes, widx, length, x, q, att, h, logits, noise, state, noise_stream]
        for t in keep:
            if t is not None:
                _need_gpu(t)
        f32 = [tok_emb, pos_table, hw, hb, hs, x, q, att, h, logits] + ([noise] if noise is not None else [])
        assert all(t.dtype == torch.float32 and t.is_contiguous() for t in f32)
        assert tok.dtype == torch.int64 and tok.numel() == B and tok.is_contiguous() and codes.dtype == torch.int64 and codes.stride(1) == 1
        assert widx.dtype == torch.int32 and length.dtype == torch.int32 and state.dtype == torch.int32
        assert groups >= 1 and B % groups == 0 and widx.numel() == groups and length.numel() == groups and state.numel() == 8 * groups
        assert widx.is_contiguous() and length.is_contiguous() and state.is_contiguous()
        if noise_stream is not None:   # device table of `groups` device pointers (ccvs_gpt_decode.noise_stream)
            assert noise is None and noise_stream.dtype == torch.int64 and noise_stream.numel() == groups and noise_stream.is_contiguous()
        arr = (_lib.GptLayer * len(layers))()
        for i, lay in enumerate(layers):
            for name, t in lay.items():
                t = t.detach()
                _need_gpu(t)
                if name in ("kcache", "vcache"):
                    _need_cache_dtype("GptDecodeStep", self.kv_dtype, t)
                    assert t.shape == (B, H, Tmax, C // H), (name, t.shape)
                else:
                    assert t.dtype == torch.float32 and t.is_contiguous(), name
                if tiled is not None and name in tiled[0][i]:
                    n_k, t = t.shape, tiled[0][i][name]
                    _need_gpu(t)
                    assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == -(-n_k[0] // 16) * 16 * n_k[1], name
                keep.append(t)
                setattr(arr[i], name, _p(t))
        F = layers[0]["fc_w"].shape[0]
        assert x.shape == (B, C) and h.shape == (B, F) and logits.shape == (B, hw.shape[0])
        assert q.shape == (B, 3 * C if kv16 else C) and att.shape == (B, C), (q.shape, att.shape)
        self.ws = _gemm_workspace(x.device)
        d = _lib.GptDecode()
        d.B, d.C, d.H, d.F, d.n_layer, d.Tmax, d.vocab, d.V = B, C, H, F, len(layers), Tmax, tok_emb.shape[0], hw.shape[0]
        d.ln_eps = ln_eps
        d.layers = arr
        d.tok_emb, d.pos_table, d.pos_off = _p(tok_emb.detach()), _p(pos_table), int(pos_off)
        d.head_w, d.head_b, d.head_s = _p(hw), _p(hb), _p(hs)
        if tiled is not None:
            assert all(set(t) == {"qkv_w", "proj_w", "fc_w", "fc2_w"} for t in tiled[0]) and len(tiled[0]) == len(layers)
            _need_gpu(tiled[1])
            assert tiled[1].dtype == torch.float32 and tiled[1].is_contiguous() and tiled[1].numel() == -(-hw.shape[0] // 16) * 16 * C
            keep.append(tiled[1])
            d.head_w, d.w_tiled = _p(tiled[1]), 1
        d.tok, d.codes, d.codes_sB = _p(tok), _p(codes), codes.stride(0)
        d.widx, d.len = _p(widx), _p(length)
        d.x, d.q, d.att, d.h, d.logits = _p(x), _p(q), _p(att), _p(h), _p(logits)
        d.noise = _p(noise)
        d.rng = 1 if (rng and noise is None and noise_stream is None) else 0
        d.noise_stream = _p(noise_stream)
        d.top_k, d.temperature = 0 if top_k is None else int(top_k), float(temperature)
        d.top_p = check_top_p(top_p) or 0.0
        d.workspace, d.state = _p(self.ws), _p(state)
        d.groups = groups
        self.desc, self._arr, self._keep = d, arr, keep
        self.persistent = bool(persistent)
        if self.persistent:
            # ONE launch per step (gpt.hip: gpt_step_kernel): its phase table lives in a device buffer of ours, written once, here
            # (a synchronous copy on the current stream: descriptors are built outside graph capture)
            L = _lib.load()
            self.program = torch.empty(int(L.ccvs_gpt_program_bytes(len(layers))), dtype=torch.uint8, device=x.device)
            d.persistent, d.program = 1, _p(self.program)
            import ctypes   # (`C` is the embedding width in this scope)
            _lib.check(L.ccvs_gpt_decode_prepare(ctypes.byref(d), _stream()), "ccvs_gpt_decode_prepare")

    def launch(self):
        L = _lib.load()
        if self.kv_dtype == torch.bfloat16:
            _lib.check(L.ccvs_gpt_decode_step_bf16kv(C.byref(self.desc), _stream()), "ccvs_gpt_decode_step_bf16kv")
        else:
            _lib.check(L.ccvs_gpt_decode_step(C.byref(self.desc), _stream()), "ccvs_gpt_decode_step")

    def status(self):
        """Persistent step: synchronise the current stream and raise if a grid barrier of any step launched with this workspace gave
        up (a workgroup that never became resident): the tokens of that step are invalid."""
        if self.persistent:
            L = _lib.load()
            _lib.check(L.ccvs_gpt_decode_status(_p(self.ws), _stream()), "ccvs_gpt_decode_status")


def stream_cu_limit(stream, cu_limit):
    """`ccvs_stream_cu_limit`: kernels launched on `stream` (a torch.cuda.Stream) from now on occupy at most cu_limit CUs
    (0: no budget)."""
    L = _lib.load()
    _lib.check(L.ccvs_stream_cu_limit(C.c_void_p(stream.cuda_stream), int(cu_limit)), "ccvs_stream_cu_limit")


def pack_u8_norm(vid, std, mean, out=None):
    """[..., 3, H, W] fp32 -> [..., H, W, 3] uint8 with the imagenet de-normalisation of helpers/generator.py:303-305 in front:
    v*std[c], + mean[c], clamp(0, 1), x255, truncate (each step rounded on its own: byte-exact with the reference's ops).
    out: optional contiguous uint8 [..., H, W, 3] tensor to write into (default: a new one)."""
    _need_gpu(vid, out)
    vid = vid.contiguous()
    lead = vid.shape[:-3]
    h, w = vid.shape[-2:]
    n = int(math.prod(lead)) if len(lead) else 1
    if out is None:
        out = torch.empty(*lead, h, w, 3, dtype=torch.uint8, device=vid.device)
    assert out.shape == (*lead, h, w, 3) and out.is_contiguous() and out.dtype == torch.uint8
    s3, m3 = (C.c_float * 3)(*[float(v) for v in std]), (C.c_float * 3)(*[float(v) for v in mean])
    L = _lib.load()
    _lib.check(L.ccvs_pack_u8_norm(_p(vid), _p(out), n, h, w, s3, m3, _stream()), "ccvs_pack_u8_norm")
    return out


def psnr(x, y, data_range=1.0):
    """Per-image PSNR of [N, C, H, W] fp32 tensors, piq.psnr's formula (tools/pytorch_metrics/metrics.py:24-25): [N] fp32."""
    _need_gpu(x, y)
    assert x.shape == y.shape and x.dim() == 4 and x.dtype == y.dtype == torch.float32, (x.shape, y.shape)
    x, y = x.contiguous(), y.contiguous()
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().ccvs_psnr(_p(x), _p(y), _p(out), x.shape[0], x[0].numel(), float(data_range), _stream()), "ccvs_psnr")
    return out


def mse(a, b):
    """F.mse_loss(a, b): mean((a - b)^2) of two fp32 tensors of one shape, float64 inside, as a 0-dim fp32 tensor on the device
    (`ccvs_mse`; nothing is synchronised)."""
    _need_gpu(a, b)
    assert a.shape == b.shape and a.dtype == b.dtype == torch.float32 and a.numel() > 0, (a.shape, b.shape)
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty((), dtype=torch.float32, device=a.device)
    _lib.check(_lib.load().ccvs_mse(_p(a), _p(b), _p(out), a.numel(), _stream()), "ccvs_mse")
    return out


def token_nll(logits2d, target, rows=None, ncols=None):
    """Per-token NLL over selected rows of teacher-forced logits (`ccvs_token_nll`): out[m] = logsumexp(logits2d[r, :ncols]) -
    logits2d[r, target[m]] with r = rows[m] (int32 device tensor; None: r = m), as fp32 [n_rows].  logits2d: [M, V] fp32 with dense
    columns (any row stride); ncols defaults to V.  A target outside [0, ncols) gives NaN for its row -- nothing is synchronised to
    raise, as the reference's F.cross_entropy would."""
    _need_gpu(logits2d, target, rows)
    assert logits2d.dim() == 2 and logits2d.dtype == torch.float32 and logits2d.stride(1) == 1, (logits2d.shape, logits2d.stride())
    ncols = logits2d.shape[1] if ncols is None else int(ncols)
    assert 0 < ncols <= logits2d.shape[1], (ncols, logits2d.shape)
    target = target.reshape(-1).to(torch.int64).contiguous()
    n_rows = target.numel()
    if rows is not None:
        assert rows.dtype == torch.int32 and rows.dim() == 1 and rows.is_contiguous() and rows.numel() == n_rows, (rows.shape, n_rows)
    else:
        assert n_rows == logits2d.shape[0], (n_rows, logits2d.shape)
    out = torch.empty(n_rows, dtype=torch.float32, device=logits2d.device)
    _lib.check(_lib.load().ccvs_token_nll(_p(logits2d), logits2d.stride(0), _p(rows), _p(target), n_rows, ncols, _p(out), _stream()),
               "ccvs_token_nll")
    return out


def mean_f32(x):
    """Mean of an fp32 tensor as a 0-dim fp32 tensor on the device, float64 inside (`ccvs_mean_f32`; nothing is synchronised)."""
    _need_gpu(x)
    assert x.dtype == torch.float32 and x.numel() > 0, (x.dtype, x.shape)
    x = x.contiguous()
    out = torch.empty((), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().ccvs_mean_f32(_p(x), x.numel(), _p(out), _stream()), "ccvs_mean_f32")
    return out


def l1_mean(a, b):
    """torch.mean(torch.abs(a - b)) of two fp32 tensors of one shape, float64 inside, as a 0-dim fp32 tensor on the device
    (`ccvs_l1_mean`: a grid of workgroups, partial sums added in index order; nothing is synchronised)."""
    _need_gpu(a, b)
    assert a.shape == b.shape and a.dtype == b.dtype == torch.float32 and a.numel() > 0, (a.shape, b.shape)
    a, b = a.contiguous(), b.contiguous()
    L = _lib.load()
    out = torch.empty((), dtype=torch.float32, device=a.device)
    ws = torch.empty(int(L.ccvs_l1_workspace_bytes(a.numel())), dtype=torch.uint8, device=a.device)
    _lib.check(L.ccvs_l1_mean(_p(a), _p(b), _p(out), _p(ws), a.numel(), _stream()), "ccvs_l1_mean")
    return out


def vq_stats(z_nchw, idx, codebook, row_scale=None):
    """The quantiser's diagnostics (`ccvs_vq_stats`): (mean_sq, counts).  z_nchw [N, C, H, W] fp32, idx int64 [N*H*W] in (n, h, w)
    order, codebook [n_e, C] fp32, row_scale [n_e] fp32 or None.  mean_sq: 0-dim fp32, the mean over every element of
    (s * codebook[idx[p]][c] - z[n, c, p])^2 with s = row_scale[idx[p]] or 1, float64 inside; counts: int32 [n_e], how often each
    code occurs.  An index outside [0, n_e) is not counted and gives a NaN mean -- nothing is synchronised to raise."""
    _need_gpu(z_nchw, idx, codebook, row_scale)
    assert z_nchw.dim() == 4 and z_nchw.dtype == torch.float32 and z_nchw.numel() > 0, (z_nchw.shape, z_nchw.dtype)
    assert codebook.dim() == 2 and codebook.dtype == torch.float32 and codebook.shape[1] == z_nchw.shape[1], (codebook.shape, z_nchw.shape)
    z, codebook = z_nchw.contiguous(), codebook.contiguous()
    n, c = z.shape[:2]
    hw = z.shape[2] * z.shape[3]
    n_e = codebook.shape[0]
    idx = idx.reshape(-1).to(torch.int64).contiguous()
    assert idx.numel() == n * hw, (idx.shape, z.shape)
    if row_scale is not None:
        assert row_scale.dtype == torch.float32 and row_scale.shape == (n_e,) and row_scale.is_contiguous(), (row_scale.shape, n_e)
    L = _lib.load()
    mean_sq = torch.empty((), dtype=torch.float32, device=z.device)
    counts = torch.empty(n_e, dtype=torch.int32, device=z.device)
    ws = torch.empty(int(L.ccvs_vq_stats_workspace_bytes(n, c, hw)), dtype=torch.uint8, device=z.device)
    _lib.check(L.ccvs_vq_stats(_p(z), _p(idx), _p(codebook), _p(row_scale), _p(mean_sq), _p(counts), _p(ws), n, c, hw, n_e, _stream()),
               "ccvs_vq_stats")
    return mean_sq, counts


def code_perplexity(counts, total):
    """exp(-sum_j p_j log(p_j + 1e-10)) with p_j = counts[j] / total (quantize.py:67-68) of an int32 [n_e] device histogram, float64
    inside, as a 0-dim fp32 tensor on the device (`ccvs_code_perplexity`; nothing is synchronised)."""
    _need_gpu(counts)
    assert counts.dim() == 1 and counts.dtype == torch.int32 and counts.numel() > 0 and int(total) > 0, (counts.shape, counts.dtype, total)
    counts = counts.contiguous()
    out = torch.empty((), dtype=torch.float32, device=counts.device)
    _lib.check(_lib.load().ccvs_code_perplexity(_p(counts), counts.numel(), int(total), _p(out), _stream()), "ccvs_code_perplexity")
    return out


def ssim_planes(x, y, data_range=2.0):
    """skimage 0.17.2 `structural_similarity` (defaults) of every 2-D plane of [..., H, W] fp32 tensors: [...] fp64
    (tools/pytorch_metrics/metrics.py:15-22; data_range 2 = what skimage takes for float planes when none is given)."""
    _need_gpu(x, y)
    assert x.shape == y.shape and x.dim() >= 2 and x.dtype == y.dtype == torch.float32, (x.shape, y.shape)
    x, y = x.contiguous(), y.contiguous()
    h, w = x.shape[-2:]
    planes = x.numel() // (h * w)
    out = torch.empty(planes, dtype=torch.float64, device=x.device)
    L = _lib.load()
    step = 65535   # planes per call
    ws = torch.empty(int(L.ccvs_ssim_workspace_bytes(min(planes, step), h, w)), dtype=torch.uint8, device=x.device)
    xf, yf = x.view(planes, h, w), y.view(planes, h, w)
    for p0 in range(0, planes, step):
        n = min(step, planes - p0)
        _lib.check(L.ccvs_ssim(_p(xf[p0:]), _p(yf[p0:]), _p(out[p0:]), _p(ws), n, h, w, float(data_range), _stream()), "ccvs_ssim")
    return out.view(x.shape[:-2])


def resize_bilinear(x, size):
    """F.interpolate(x, size=size, mode='bilinear') (align_corners False) of [..., H, W] fp32 (tools/pytorch_metrics/metrics.py:124)."""
    _need_gpu(x)
    assert x.dtype == torch.float32 and x.dim() >= 2
    x = x.contiguous()
    h, w = x.shape[-2:]
    oh, ow = int(size[0]), int(size[1])
    out = torch.empty(*x.shape[:-2], oh, ow, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().ccvs_resize_bilinear(_p(x), _p(out), x.numel() // (h * w), h, w, oh, ow, _stream()), "ccvs_resize_bilinear")
    return out


# ------------------------------------------------------------------ LPIPS (include/ccvs_hip_lpips.h)
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def lpips_prep(x, out=None, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """(x - mean[c]) / std[c] of [N, 3, H, W] fp32 images, a true fp32 division like torch's (`ccvs_lpips_prep`).  out: optional
    contiguous fp32 [N, 3, H, W] tensor to write into (default: a new one)."""
    _need_gpu(x, out)
    assert x.dim() == 4 and x.shape[1] == 3 and x.dtype == torch.float32 and x.numel() > 0, (x.shape, x.dtype)
    x = x.contiguous()
    if out is None:
        out = torch.empty_like(x)
    assert out.shape == x.shape and out.dtype == torch.float32 and out.is_contiguous() and out.data_ptr() != x.data_ptr(), (out.shape, x.shape)
    m3, s3 = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
    _lib.check(_lib.load().ccvs_lpips_prep(_p(x), _p(out), x.shape[0] * 3, x.shape[2] * x.shape[3], m3, s3, _stream()), "ccvs_lpips_prep")
    return out


def relu_(x):
    """nn.ReLU in place on a dense fp32 tensor (`ccvs_relu_`); a NaN stays a NaN.  Returns x."""
    _need_gpu(x)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.numel() > 0, (x.dtype, x.shape, x.stride())
    _lib.check(_lib.load().ccvs_relu_(_p(x), x.numel(), _stream()), "ccvs_relu_")
    return x


def relu_maxpool2(x, out=None):
    """nn.MaxPool2d(2, 2)(nn.ReLU()(x)) of [..., H, W] fp32 in one read (`ccvs_relu_maxpool2`): floor mode, a NaN in a window comes
    out.  out: optional contiguous fp32 [..., H // 2, W // 2] tensor to write into."""
    _need_gpu(x, out)
    assert x.dtype == torch.float32 and x.dim() >= 2 and x.shape[-2] >= 2 and x.shape[-1] >= 2 and x.numel() > 0, (x.dtype, x.shape)
    x = x.contiguous()
    h, w = x.shape[-2:]
    if out is None:
        out = torch.empty(*x.shape[:-2], h // 2, w // 2, dtype=torch.float32, device=x.device)
    assert out.shape == (*x.shape[:-2], h // 2, w // 2) and out.dtype == torch.float32 and out.is_contiguous(), (out.shape, x.shape)
    _lib.check(_lib.load().ccvs_relu_maxpool2(_p(x), _p(out), x.numel() // (h * w), h, w, _stream()), "ccvs_relu_maxpool2")
    return out


def lpips_layer(f, w, relu=True, out=None, accumulate=False):
    """The LPIPS distance of one tapped layer (`ccvs_lpips_layer`).  f: [2 M, C, ...] fp32, the features (relu=True: the pre-activations,
    ReLU applied on read) of M images x followed by those of the M images y; w: the layer's linear head, C fp32 values.  Returns float64
    [M]: per pair the mean over the positions of sum_c w[c] (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2, float64 inside, the same
    bits on every run.  out: float64 [M] to write into; accumulate=True adds to what it holds (the sum over the layers)."""
    _need_gpu(f, w, out)
    assert f.dim() >= 2 and f.dtype == torch.float32 and f.shape[0] % 2 == 0 and f.numel() > 0, (f.shape, f.dtype)
    f = f.contiguous()
    m, c = f.shape[0] // 2, f.shape[1]
    hw = f[0, 0].numel()
    w = w.reshape(-1).contiguous()
    assert w.dtype == torch.float32 and w.numel() == c, (w.shape, w.dtype, c)
    if out is None:
        assert not accumulate
        out = torch.empty(m, dtype=torch.float64, device=f.device)
    assert out.shape == (m,) and out.dtype == torch.float64 and out.is_contiguous(), (out.shape, out.dtype, m)
    L = _lib.load()
    ws = torch.empty(int(L.ccvs_lpips_layer_workspace_bytes(m, hw)), dtype=torch.uint8, device=f.device)   # (0 bytes for M > 65535: the call refuses)
    _lib.check(L.ccvs_lpips_layer(_p(f), _p(w), _p(out), _p(ws), m, c, hw, int(bool(relu)), int(bool(accumulate)), _stream()), "ccvs_lpips_layer")
    return out


# ------------------------------------------------------------------ FVD / I3D (include/ccvs_hip_fvd.h)
def same_pad(n, k, s):
    """TensorFlow's SAME geometry of one axis: (out, before, after) = (ceil(n / s), total // 2, total - total // 2) with
    total = max((out - 1) s + k - n, 0)."""
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return out, total // 2, total - total // 2


def fvd_prep(u8, size=(224, 224), flip=False, out=None):
    """fvd.py:34-51 `preprocess` (`ccvs_fvd_prep`): uint8 [..., H, W, 3] -> fp32 [..., 3, OH, OW], TF1's resize_bilinear
    (align_corners False, no half-pixel centres) then (2 v) / 255 - 1, each step rounded to fp32 on its own.  flip=True reverses the
    channel order.  out: optional contiguous fp32 tensor of that shape to write into."""
    _need_gpu(u8, out)
    assert u8.dtype == torch.uint8 and u8.dim() >= 3 and u8.shape[-1] == 3 and u8.numel() > 0, (u8.dtype, u8.shape)
    u8 = u8.contiguous()
    h, w = u8.shape[-3:-1]
    oh, ow = int(size[0]), int(size[1])
    shape = (*u8.shape[:-3], 3, oh, ow)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=u8.device)
    assert out.shape == shape and out.dtype == torch.float32 and out.is_contiguous(), (out.shape, shape)
    _lib.check(_lib.load().ccvs_fvd_prep(_p(u8), _p(out), u8.numel() // (h * w * 3), h, w, oh, ow, int(bool(flip)), _stream()), "ccvs_fvd_prep")
    return out


def time_unfold(x, t, kt, st=1, pad=(0, 0, 0, 0), relu=False, phases=1, out=None):
    """The time-stacked input of a kt-tap, stride-st 3-D convolution with SAME padding in time (`ccvs_time_unfold`).  x: [N t, C, H, W]
    fp32, clips of t frames (a channel-slice view is read in place) -> [N To, kt C, H + pt + pb, W + pl + pr], To = ceil(t / st): channel
    j C + c of output frame t' is channel c of the clip's frame t' st + j - before, zeros outside the clip; pad = (pt, pb, pl, pr) zero
    border rows and columns; relu=True writes max(x, 0).  phases=2 also splits the bordered frame (even sides) into its four pixel
    phases: [N To, 4 kt C, Hp / 2, Wp / 2], channel (j C + c) 4 + 2 py + px holding the pixels (2 y + py, 2 x + px), the input of a
    stride-2 convolution written as a stride-1 one (`stack_conv3d_weight`).  out: optional contiguous fp32 tensor of that shape."""
    _need_gpu(x, out)
    assert x.dim() == 4 and x.dtype == torch.float32 and x.numel() > 0 and x.shape[0] % t == 0, (x.shape, x.dtype, t)
    if not (_rows_dense(x) and x.stride(1) >= x.shape[2] * x.shape[3] and x.stride(0) >= x.stride(1) * x.shape[1]):
        x = x.contiguous()
    nt, c, h, w = x.shape
    pt, pb, pl, pr = (int(v) for v in pad)
    hp, wp = h + pt + pb, w + pl + pr
    assert phases == 1 or (phases == 2 and hp % 2 == 0 and wp % 2 == 0), (phases, hp, wp)
    to = same_pad(t, kt, st)[0]
    shape = (nt // t * to, kt * c * phases * phases, hp // phases, wp // phases)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    assert out.shape == shape and out.dtype == torch.float32 and out.is_contiguous(), (out.shape, shape)
    _lib.check(_lib.load().ccvs_time_unfold(_p(x), x.stride(0), x.stride(1), _p(out), nt // t, t, c, h, w, kt, st, pt, pb, pl, pr, phases,
                                            int(bool(relu)), _stream()), "ccvs_time_unfold")
    return out


def stack_conv3d_weight(w, phases=1):
    """[Cout, Cin, kt, k, k] -> the 2-D weight over `time_unfold`'s channels: [Cout, kt Cin, k, k], or for phases=2 (a stride-2
    convolution as a stride-1 one over the four pixel phases) [Cout, 4 kt Cin, ceil(k / 2), ceil(k / 2)] with tap (a, b) of channel
    (j Cin + c) 4 + 2 py + px = w[:, c, j, 2 a + py, 2 b + px], zero where that lies outside the kernel."""
    co, ci, kt, kh, kw = w.shape
    if phases == 1:
        return w.permute(0, 2, 1, 3, 4).reshape(co, kt * ci, kh, kw)
    assert phases == 2 and kh == kw, (phases, w.shape)
    k2 = (kh + 1) // 2
    wp = torch.zeros(co, ci, kt, 2 * k2, 2 * k2, dtype=w.dtype, device=w.device)
    wp[:, :, :, :kh, :kw] = w
    return wp.view(co, ci, kt, k2, 2, k2, 2).permute(0, 2, 1, 4, 6, 3, 5).reshape(co, kt * ci * 4, k2, k2)


def maxpool3d_same(x, t, kernel, stride, relu=False, out=None):
    """A 3-D max pool with TensorFlow's SAME geometry (`ccvs_maxpool3d_same`).  x: [N t, C, H, W] fp32, clips of t frames -> [N To, C,
    Ho, Wo] with ceil(n / s) per axis; kernel (1,3,3), (3,3,3) or (2,2,2), stride (1,2,2), (2,2,2) or (1,1,1).  Padding never wins (a
    window is clipped to the clip); relu=True pools max(x, 0); a NaN in a window comes out, as in torch.  out: optional contiguous
    fp32 tensor of that shape."""
    _need_gpu(x, out)
    assert x.dim() == 4 and x.dtype == torch.float32 and x.numel() > 0 and x.shape[0] % t == 0, (x.shape, x.dtype, t)
    x = x.contiguous()
    nt, c, h, w = x.shape
    (kt, kh, kw), (st, sh, sw) = kernel, stride
    shape = (nt // t * same_pad(t, kt, st)[0], c, same_pad(h, kh, sh)[0], same_pad(w, kw, sw)[0])
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    assert out.shape == shape and out.dtype == torch.float32 and out.is_contiguous(), (out.shape, shape)
    _lib.check(_lib.load().ccvs_maxpool3d_same(_p(x), _p(out), nt // t, t, c, h, w, kt, kh, kw, st, sh, sw, int(bool(relu)), _stream()),
               "ccvs_maxpool3d_same")
    return out


def i3d_head(x, t, weight, bias, relu=False, out=None):
    """The I3D head (`ccvs_i3d_head`).  x: [N t, C, 7, 7] fp32, clips of t >= 2 frames; weight [K, C] and bias [K] fp32 -> float64 [N, K]:
    the (2, 7, 7) average pool (stride 1, VALID: t - 1 windows), the logits `weight x + bias` and their mean over the windows, float64
    inside, the same bits on every run.  relu=True averages max(x, 0).  out: optional float64 [N, K] to write into."""
    _need_gpu(x, weight, bias, out)
    assert x.dim() == 4 and x.dtype == torch.float32 and x.numel() > 0 and x.shape[0] % t == 0, (x.shape, x.dtype, t)
    if x.shape[2:] != (7, 7):
        raise ValueError(f"i3d_head: the map in front of the (2, 7, 7) average pool is {tuple(x.shape[2:])}, not 7 x 7 (the squeeze needs 1 x 1 behind it)")
    x = x.contiguous()
    nt, c = x.shape[:2]
    weight = weight.reshape(weight.shape[0], -1).contiguous()
    bias = bias.reshape(-1).contiguous()
    k = weight.shape[0]
    assert weight.dtype == torch.float32 and bias.dtype == torch.float32 and weight.shape == (k, c) and bias.shape == (k,), (weight.shape, bias.shape, c)
    if out is None:
        out = torch.empty(nt // t, k, dtype=torch.float64, device=x.device)
    assert out.shape == (nt // t, k) and out.dtype == torch.float64 and out.is_contiguous(), (out.shape, out.dtype)
    _lib.check(_lib.load().ccvs_i3d_head(_p(x), _p(weight), _p(bias), _p(out), nt // t, t, c, 49, k, int(bool(relu)), _stream()), "ccvs_i3d_head")
    return out


def pack_u8(vid, lo=-1.0, hi=1.0, out=None):
    """[..., 3, H, W] fp32 -> [..., H, W, 3] uint8 (helpers/generator.py:306-309).  out: optional contiguous uint8 [..., H, W, 3]
    tensor to write into (default: a new one)."""
    _need_gpu(vid, out)
    vid = vid.contiguous()
    lead = vid.shape[:-3]
    h, w = vid.shape[-2:]
    n = int(math.prod(lead)) if len(lead) else 1
    if out is None:
        out = torch.empty(*lead, h, w, 3, dtype=torch.uint8, device=vid.device)
    assert out.shape == (*lead, h, w, 3) and out.is_contiguous() and out.dtype == torch.uint8
    L = _lib.load()
    _lib.check(L.ccvs_pack_u8(_p(vid), _p(out), n, h, w, lo, hi, _stream()), "ccvs_pack_u8")
    return out


# ------------------------------------------------------------------ motion export (include/ccvs_hip_flowviz.h)
_FLOW_LUTS = {}


def _motion_strides(motion):
    """[B, T, 3, H, W] fp32 whose three planes per frame are dense: (B, T, H, W, batch stride, frame stride)."""
    _need_gpu(motion)
    assert motion.dim() == 5 and motion.shape[2] == 3 and motion.dtype == torch.float32, tuple(motion.shape)
    b, t, _, h, w = motion.shape
    assert motion.stride(4) == 1 and motion.stride(3) == w and motion.stride(2) == h * w, "motion: the planes of a frame must be dense"
    return b, t, h, w, motion.stride(0), motion.stride(1)


def flow_export(fo, k, flow_mult, out, t):
    """The last InterBlock's rows of one new frame into slot t of the clip's motion buffer (`ccvs_flow_export`).  fo: [B * k, 3, H, W]
    (flow | occ), usually the channel-slice view `InterBlock.forward_fused` returns -- read in place, any batch stride; out: the
    [B, T, 3, H, W] fp32 buffer.  out[:, t, 0:2] = fo[b * k, 0:2] * flow_mult (context 0 of every clip), out[:, t, 2] = the mask the
    blend used: sigmoid of the confidence-weighted mean of the k occlusion logits."""
    _need_gpu(fo, out)
    assert fo.dim() == 4 and fo.shape[1] == 3 and fo.dtype == torch.float32 and _planes_dense(fo), (tuple(fo.shape), fo.stride())
    b, nt, h, w, s_b, s_t = _motion_strides(out)
    assert fo.shape == (b * k, 3, h, w) and 0 <= t < nt, (tuple(fo.shape), k, tuple(out.shape), t)
    fo_sn = fo.stride(0) if fo.shape[0] > 1 else 3 * h * w
    L = _lib.load()
    _lib.check(L.ccvs_flow_export(_p(fo), fo_sn, b, int(k), h, w, float(flow_mult), C.c_void_p(out.data_ptr() + 4 * t * s_t),
                                  s_b if b > 1 else 3 * h * w, _stream()), "ccvs_flow_export")
    return out


def flow_max(motion):
    """Per-clip largest flow magnitude sqrt(fx^2 + fy^2) of a motion buffer [B, T, 3, H, W] over its finite pixels: [B] fp32, 0 for a
    clip without one (`ccvs_flow_max`; an integer maximum on the bit pattern, the same bits on every run)."""
    b, t, h, w, s_b, s_t = _motion_strides(motion)
    out = torch.empty(b, dtype=torch.float32, device=motion.device)
    L = _lib.load()
    _lib.check(L.ccvs_flow_max(_p(motion), s_b if b > 1 else t * 3 * h * w, s_t if t > 1 else 3 * h * w, b, t, h, w, _p(out), _stream()),
               "ccvs_flow_max")
    return out


def flow_lut(device):
    """`tools.flowviz.HSV128` on `device`, uploaded once."""
    key = torch.device(device)
    if key not in _FLOW_LUTS:
        from ccvs_amd.tools.flowviz import HSV128
        _FLOW_LUTS[key] = torch.from_numpy(HSV128.copy()).to(key)
    return _FLOW_LUTS[key]


def flow_render(motion, max_px, lut=None):
    """A motion buffer [B, T, 3, H, W] as (flow_u8, occ_u8), both uint8 [B, T, H, W, 3] (`ccvs_flow_render`): the reference's
    get_flow_rgb colours saturating at max_px[b] pixels (a [B] fp32 device tensor: `flow_max`'s output or a filled constant; a clip
    with max_px 0 is black, and so is a pixel with a non-finite component), and the mask as grey.  lut: [128, 3] fp32 on the device
    (default: `flow_lut`)."""
    b, t, h, w, s_b, s_t = _motion_strides(motion)
    lut = flow_lut(motion.device) if lut is None else lut
    _need_gpu(max_px, lut)
    assert max_px.shape == (b,) and max_px.dtype == torch.float32 and max_px.is_contiguous()
    assert lut.shape == (128, 3) and lut.dtype == torch.float32 and lut.is_contiguous()
    flow_u8 = torch.empty(b, t, h, w, 3, dtype=torch.uint8, device=motion.device)
    occ_u8 = torch.empty_like(flow_u8)
    L = _lib.load()
    _lib.check(L.ccvs_flow_render(_p(motion), s_b if b > 1 else t * 3 * h * w, s_t if t > 1 else 3 * h * w, b, t, h, w, _p(max_px), _p(lut),
                                  _p(flow_u8), _p(occ_u8), _stream()), "ccvs_flow_render")
    return flow_u8, occ_u8


# ------------------------------------------------------------------ input stage (include/ccvs_hip_input.h)
_RESAMPLE_TABLES = {}
_NORM_TABLES = {}


def resample_tables(in_size, out_size, device=None):
    """The tables of one axis of Pillow's 8-bit bilinear resampler (`ImagingResample`: `precompute_coeffs` + `normalize_coeffs_8bpc`)
    for `in_size` -> `out_size` samples, built on the host in float64: (coef int32 [out, ksize], bounds int32 [out, 2]).  bounds[o] =
    (first tap, number of taps); coef[o][i] = int(w_i * 2^22 + 0.5), w the triangle weights max(0, 1 - |(i + first - center + 0.5) /
    filterscale|) divided by their sum (added in tap order), zero past the last tap.  ksize = 2 * ceil(max(in / out, 1)) + 1.
    Cached per (in, out, device); `device` None: the CPU -- no GPU is needed to build or to check them."""
    in_size, out_size = int(in_size), int(out_size)
    assert in_size > 0 and out_size > 0, (in_size, out_size)
    device = torch.device("cpu" if device is None else device)
    key = (in_size, out_size, str(device))
    if key in _RESAMPLE_TABLES:
        return _RESAMPLE_TABLES[key]
    f64 = torch.float64
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    center = (torch.arange(out_size, dtype=f64) + 0.5) * scale
    xmin = torch.trunc(center - support + 0.5).clamp_(min=0)
    xmax = torch.trunc(center + support + 0.5).clamp_(max=in_size) - xmin
    ss = 1.0 / filterscale
    w = torch.zeros(out_size, ksize, dtype=f64)
    ww = torch.zeros(out_size, dtype=f64)
    for x in range(ksize):
        v = (1.0 - ((x + xmin - center + 0.5) * ss).abs()).clamp_(min=0)
        v = torch.where(x < xmax, v, torch.zeros_like(v))
        w[:, x] = v
        ww += v
    w = torch.where((ww != 0)[:, None], w / ww[:, None], w)
    coef = torch.trunc(w * float(1 << 22) + 0.5).to(torch.int32)
    bounds = torch.stack([xmin, xmax], dim=1).to(torch.int32)
    _RESAMPLE_TABLES[key] = (coef.contiguous().to(device), bounds.contiguous().to(device))
    return _RESAMPLE_TABLES[key]


def norm_table(mean, std, device):
    """float32 [3, 256] on `device`: ToTensor + Normalize of every uint8 value per channel, ((v / 255) - mean[c]) / std[c], computed
    by the framework on the HOST (where the reference's transforms run: a true fp32 division by 255, then tensor - tensor and tensor /
    tensor) and uploaded once per (mean, std, device)."""
    mean, std = tuple(float(m) for m in mean), tuple(float(s) for s in std)
    assert len(mean) == 3 and len(std) == 3, (mean, std)
    key = (mean, std, str(torch.device(device)))
    if key not in _NORM_TABLES:
        v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)[None].repeat(3, 1)
        v = v.sub_(torch.tensor(mean, dtype=torch.float32)[:, None]).div_(torch.tensor(std, dtype=torch.float32)[:, None])
        _NORM_TABLES[key] = v.contiguous().to(device)
    return _NORM_TABLES[key]


def ingest_u8(frames, box=None, size=None, out=None, mean=None, std=None, as_u8=False):
    """One crop + resample stage of the input chain (`ccvs_ingest_u8`): uint8 frames [N, Hs, Ws, 3] (or [Hs, Ws, 3]) on the device, any
    frame stride, `box` = (top, left, h, w) inside the frame (None: all of it), `size` = (Ho, Wo) (None: the box's size).  The
    resample is `PIL.Image.resize((Wo, Ho), BILINEAR)` of the cropped frame, bit for bit; an axis whose size does not change is not
    resampled.
      as_u8=True   -> uint8 [N, Ho, Wo, 3] (`out`: optional contiguous tensor of that shape), the input of a further stage;
      as_u8=False  -> fp32 [N, 3, Ho, Wo] = ((v / 255) - mean) / std per channel (defaults 0.5 / 0.5: ToTensor + Normalize).  `out`:
                      optional fp32 tensor of that shape with dense rows and any frame / channel strides, e.g. `clip[b, t0:t1]` of a
                      [B, T, 3, H, W] clip -- it is written in place and returned.
    Runs on the current stream; nothing is synchronised."""
    _need_gpu(frames, out)
    assert frames.dtype == torch.uint8 and frames.dim() in (3, 4) and frames.shape[-1] == 3, (frames.dtype, frames.shape)
    if frames.dim() == 3:
        frames = frames[None]
    n, hs, ws = frames.shape[:3]
    if frames.stride()[1:] != (3 * ws, 3, 1) or (n > 1 and frames.stride(0) < hs * ws * 3):
        frames = frames.contiguous()
    top, left, hc, wc = (0, 0, hs, ws) if box is None else (int(v) for v in box)
    ho, wo = (hc, wc) if size is None else (int(size[0]), int(size[1]))
    if not (0 <= top and 0 <= left and hc > 0 and wc > 0 and top + hc <= hs and left + wc <= ws):
        raise ValueError(f"ingest_u8: crop box {(top, left, hc, wc)} leaves the {hs} x {ws} frame")
    dev = frames.device
    hcoef, hbounds = resample_tables(wc, wo, dev) if wo != wc else (None, None)
    vcoef, vbounds = resample_tables(hc, ho, dev) if ho != hc else (None, None)
    lut = None
    if as_u8:
        assert mean is None and std is None, "as_u8: the uint8 form is not normalised"
        if out is None:
            out = torch.empty(n, ho, wo, 3, dtype=torch.uint8, device=dev)
        assert out.dtype == torch.uint8 and out.shape == (n, ho, wo, 3) and out.is_contiguous(), (out.dtype, out.shape, out.stride())
        s_n = s_c = 0
    else:
        lut = norm_table((0.5, 0.5, 0.5) if mean is None else mean, (0.5, 0.5, 0.5) if std is None else std, dev)
        if out is None:
            out = torch.empty(n, 3, ho, wo, dtype=torch.float32, device=dev)
        assert out.dtype == torch.float32 and out.shape == (n, 3, ho, wo) and _rows_dense(out), (out.dtype, out.shape, out.stride())
        s_n, s_c = out.stride(0), out.stride(1)
        assert s_c >= ho * wo and (n == 1 or s_n >= 2 * s_c + ho * wo), out.stride()
    _lib.check(_lib.load().ccvs_ingest_u8(_p(frames), frames.stride(0) if n > 1 else hs * ws * 3, n, hs, ws, top, left, hc, wc,
                                          _p(hcoef), _p(hbounds), hcoef.shape[1] if hcoef is not None else 0,
                                          _p(vcoef), _p(vbounds), vcoef.shape[1] if vcoef is not None else 0, ho, wo,
                                          _p(out) if as_u8 else None, None if as_u8 else _p(out), s_n, s_c, _p(lut), _stream()),
               "ccvs_ingest_u8")
    return out


# ------------------------------------------------------------------ input stage of the video-file datasets (include/ccvs_hip_video.h)
INGEST_PRE = {None: 0, "div255": 1, "x2m1": 2}
# the launch form when the caller does not choose: fused up to this many RESIZING stages, staged beyond (DESIGN.md section 4.17 has the
# timings that decide it)
INGEST_F32_FUSED_MAX_RESIZES = 2


def ingest_stages(hs, ws, stages):
    """`stages` = [(box, size), ...] (box (top, left, h, w) or None: the whole input; size (Ho, Wo) or None: the box's size) for an
    hs x ws source as rows (top, left, hc, wc, Ho, Wo); ValueError where a box leaves its stage's input."""
    rows, h, w = [], int(hs), int(ws)
    for k, (box, size) in enumerate(stages):
        top, left, hc, wc = (0, 0, h, w) if box is None else (int(v) for v in box)
        ho, wo = (hc, wc) if size is None else (int(size[0]), int(size[1]))
        if not (0 <= top and 0 <= left and hc > 0 and wc > 0 and top + hc <= h and left + wc <= w and ho > 0 and wo > 0):
            raise ValueError(f"ingest_f32: stage {k}: crop box {(top, left, hc, wc)} leaves its {h} x {w} input, or an empty size {(ho, wo)}")
        rows.append((top, left, hc, wc, ho, wo))
        h, w = ho, wo
    return rows


def ingest_f32(src, stages=(), out=None, pre="div255", mean=None, std=None, fused=None):
    """The reference's TENSOR transform chain (`ccvs_ingest_f32`) on N frames: `src` uint8 [N, Hs, Ws, 3] (any
    frame stride) or fp32 [N, C, Hs, Ws] (C 1 or 3, rows dense) on the device -> `pre` ("div255": v / 255, "x2m1": v * 2 - 1, None) ->
    the `stages` [(box, size), ...] (1 to 3; none: a copy), each a crop and torch's `F.interpolate(size, mode="bilinear",
    align_corners=False)` in fp32 -> (y - mean[c]) / std[c] when `mean` / `std` are given -> fp32 [N, C, Ho, Wo].  `out`: optional
    tensor of that shape with dense rows and any frame / channel strides (`clip[b, t0:t1]`), written in place and returned.
      fused=True   all stages in ONE launch, evaluated per output pixel: no intermediate tensor;
      fused=False  one launch per stage through fp32 intermediates in HBM -- the same bits;
      fused=None   fused when at most INGEST_F32_FUSED_MAX_RESIZES stages change a size, staged otherwise.
    Runs on the current stream; nothing is synchronised."""
    _need_gpu(src, out)
    if pre not in INGEST_PRE:
        raise ValueError(f"ingest_f32: pre-op {pre!r} is none of {list(INGEST_PRE)}")
    if src.dtype == torch.uint8:
        assert src.dim() == 4 and src.shape[-1] == 3, src.shape
        n, hs, ws, c = src.shape[0], src.shape[1], src.shape[2], 3
        if src.stride()[1:] != (3 * ws, 3, 1) or (n > 1 and src.stride(0) < hs * ws * 3):
            src = src.contiguous()
        s_n, s_c = (src.stride(0) if n > 1 else hs * ws * 3), 0
    else:
        assert src.dtype == torch.float32 and src.dim() == 4 and src.shape[1] in (1, 3), (src.dtype, src.shape)
        n, c, hs, ws = src.shape
        if not _rows_dense(src) or (c > 1 and src.stride(1) < hs * ws) or (n > 1 and src.stride(0) < hs * ws):
            src = src.contiguous()
        s_n, s_c = src.stride(0), src.stride(1)
    if (mean is None) != (std is None):
        raise ValueError("ingest_f32: mean and std go together")
    rows = ingest_stages(hs, ws, list(stages) or [(None, None)])
    if len(rows) > 3:
        raise ValueError(f"ingest_f32: {len(rows)} stages, at most 3 are evaluated")
    ho, wo = rows[-1][4:]
    dev = src.device
    if out is None:
        out = torch.empty(n, c, ho, wo, dtype=torch.float32, device=dev)
    assert out.dtype == torch.float32 and tuple(out.shape) == (n, c, ho, wo) and _rows_dense(out), (out.dtype, out.shape, out.stride())
    assert (c == 1 or out.stride(1) >= ho * wo) and (n == 1 or out.stride(0) >= (c - 1) * out.stride(1) + ho * wo), out.stride()
    if fused is None:
        fused = sum(1 for r in rows if r[2:4] != r[4:6]) <= INGEST_F32_FUSED_MAX_RESIZES
    ms = None
    if mean is not None:
        mean, std = [float(v) for v in mean], [float(v) for v in std]
        assert len(mean) == c and len(std) == c, (mean, std, c)
        ms = (C.c_float * (2 * c))(*mean, *std)
    L = _lib.load()

    def launch(x, x_u8, x_sn, x_sc, h, w, pre_op, part, norm, dst):
        flat = (C.c_int32 * (6 * len(part)))(*[v for r in part for v in r])
        _lib.check(L.ccvs_ingest_f32(_p(x), 1 if x_u8 else 0, x_sn, x_sc, n, c, h, w, INGEST_PRE[pre_op], flat, len(part), norm,
                                     _p(dst), dst.stride(0), dst.stride(1), _stream()), "ccvs_ingest_f32")

    if fused or len(rows) == 1:
        launch(src, src.dtype == torch.uint8, s_n, s_c, hs, ws, pre, rows, ms, out)
        return out
    x, x_u8, x_sn, x_sc, h, w = src, src.dtype == torch.uint8, s_n, s_c, hs, ws
    for k, r in enumerate(rows):
        last = k == len(rows) - 1
        dst = out if last else torch.empty(n, c, r[4], r[5], dtype=torch.float32, device=dev)
        launch(x, x_u8, x_sn, x_sc, h, w, pre if k == 0 else None, [r], ms if last else None, dst)
        x, x_u8, x_sn, x_sc, h, w = dst, False, dst.stride(0), dst.stride(1), r[4], r[5]
    return out


# ------------------------------------------------------------------ output stage (include/ccvs_hip_output.h)
def mjpeg_encode(u8, quality=90, restart_mcus=None, capacity=None, out=None, sampling=0):
    """Baseline JPEG scans of uint8 frames [..., H, W, 3] on the device (`ccvs_mjpeg_encode`: libjpeg's bytes, bit for bit): returns
    (stream uint8 [capacity], offsets int64 [n + 1]), both on the device -- frame i's scan is stream[offsets[i]:offsets[i + 1]].
    Leading axes are flattened in order; rows and pixels must be dense, a frame axis of any regular stride is passed on as it is
    (`clip[:, 1::2]` of a contiguous clip is not copied).  sampling: 0 = 4:4:4 (the default), 1 = 4:2:2, 2 = 4:2:0 -- the
    subsampled forms go through `ccvs_mjpeg_encode_sampled` (include/ccvs_hip_output_sampled.h), libjpeg's bytes as well.  restart_mcus:
    the restart interval in MCUs of the sampling's size (8 x 8, 16 x 8, 16 x 16 pixels), 1 .. 32 / 24 / 16 (None: one row of MCUs,
    capped at that limit).  capacity: bytes of `stream` (None: the raw size of the frames); the offsets are complete also when
    offsets[n] > capacity, nothing at or beyond `capacity` is written, and the CALLER runs again with a larger one once it has
    the offsets on the host (`mjpeg_encode_to_host` does).  out: optional uint8 stream to write into (its length is the capacity).
    `ccvs_amd.tools.mjpeg.jpeg_header(h, w, quality, restart_mcus, sampling)` + scan + EOI is a JPEG file.  Runs on the current stream; nothing
    is synchronised."""
    frames, n, h, w, sampling, r, stream, capacity, offsets = _mjpeg_encode_args("mjpeg_encode", u8, restart_mcus, capacity, out, sampling)
    L = _lib.load()
    dev = u8.device
    if sampling == 0:
        work = torch.empty(max(int(L.ccvs_mjpeg_workspace_bytes(n, h, w, r)), 8), dtype=torch.uint8, device=dev)
        _lib.check(L.ccvs_mjpeg_encode(_p(frames), frames.stride(0) if n > 1 else h * w * 3, n, h, w, int(quality), r, _p(stream), int(capacity),
                                       _p(offsets), _p(work), _stream()), "ccvs_mjpeg_encode")
    else:
        work = torch.empty(max(int(L.ccvs_mjpeg_sampled_workspace_bytes(n, h, w, sampling, r)), 8), dtype=torch.uint8, device=dev)
        _lib.check(L.ccvs_mjpeg_encode_sampled(_p(frames), frames.stride(0) if n > 1 else h * w * 3, n, h, w, int(quality), sampling, r, _p(stream),
                                               int(capacity), _p(offsets), _p(work), _stream()), "ccvs_mjpeg_encode_sampled")
    return stream, offsets


def _mjpeg_encode_args(who, u8, restart_mcus, capacity, out, sampling):
    """What the encoders share: the frames as [n, H, W, 3] with dense rows (a view where the strides allow), the sampling and restart
    interval checked / defaulted, the stream (`out`, or `capacity` bytes) and the offsets tensor."""
    _need_gpu(u8, out)
    assert u8.dtype == torch.uint8 and u8.dim() >= 3 and u8.shape[-1] == 3, (u8.dtype, u8.shape)
    h, w = int(u8.shape[-3]), int(u8.shape[-2])
    frames = u8.reshape(1, h, w, 3) if u8.dim() == 3 else u8
    if frames.stride()[-3:] != (3 * w, 3, 1):
        frames = frames.contiguous()
    if frames.dim() > 4:
        try:
            frames = frames.view(-1, h, w, 3)      # leading axes of one regular stride
        except RuntimeError:
            frames = frames.reshape(-1, h, w, 3)
    n = int(frames.shape[0])
    sampling = int(sampling)
    if sampling not in (0, 1, 2):
        raise ValueError(f"{who}: sampling {sampling} is none of 0 (4:4:4), 1 (4:2:2), 2 (4:2:0)")
    mw = 16 if sampling else 8
    r = min((w + mw - 1) // mw, (32, 24, 16)[sampling]) if restart_mcus is None else int(restart_mcus)
    if out is not None:
        assert out.dtype == torch.uint8 and out.dim() == 1 and out.is_contiguous() and capacity in (None, out.numel()), (out.dtype, out.shape)
        capacity = out.numel()
    elif capacity is None:
        capacity = n * h * w * 3
    stream = out if out is not None else torch.empty(int(capacity), dtype=torch.uint8, device=u8.device)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=u8.device)
    return frames, n, h, w, sampling, r, stream, int(capacity), offsets


def mjpeg_encode_optimized(u8, quality=90, restart_mcus=None, capacity=None, out=None, sampling=0):
    """`mjpeg_encode` with per-frame optimised Huffman tables (`ccvs_mjpeg_encode_optimized`, include/ccvs_hip_output_optimized.h: the
    bytes libjpeg writes with optimize_coding, bit for bit): returns (stream, offsets, tables).  stream and
    offsets are what `mjpeg_encode` returns -- the same coefficients, coded with each frame's own tables -- and `tables` (uint8
    [n, 4, 272], on the device) holds every frame's four tables in DHT order as bits[16] + huffval, zero-padded:
    `tools.mjpeg.huffman_from_spec(tables[i].cpu().numpy())` is the `huffman` argument of `tools.mjpeg.jpeg_header` for frame i.  Frames,
    strides, the default restart interval, capacity and `out` are handled as in `mjpeg_encode`.  Runs on the current stream; nothing
    is synchronised."""
    frames, n, h, w, sampling, r, stream, capacity, offsets = _mjpeg_encode_args("mjpeg_encode_optimized", u8, restart_mcus, capacity, out, sampling)
    L = _lib.load()
    tables = torch.empty((n, 4, 272), dtype=torch.uint8, device=u8.device)
    work = torch.empty(max(int(L.ccvs_mjpeg_optimized_workspace_bytes(n, h, w, sampling, r)), 8), dtype=torch.uint8, device=u8.device)
    _lib.check(L.ccvs_mjpeg_encode_optimized(_p(frames), frames.stride(0) if n > 1 else h * w * 3, n, h, w, int(quality), sampling, r, _p(stream),
                                             int(capacity), _p(offsets), _p(tables), _p(work), _stream()), "ccvs_mjpeg_encode_optimized")
    return stream, offsets, tables


def mjpeg_encode_to_host(u8, quality=90, restart_mcus=None, sampling=0, optimize=False):
    """`mjpeg_encode` (sampling: 0 / 1 / 2 = 4:4:4 / 4:2:2 / 4:2:0), then the scans on the host: (bytes of all scans, list of n + 1
    offsets).  The first run's stream has the
    frames' raw size; where the scans are larger than that (noise at quality 100) the offsets say by how much and a second run with
    that capacity is exact.  What crosses to the host is the offsets and the compressed bytes, not the stream's capacity.
    optimize: `mjpeg_encode_optimized` instead, and a third result: the frames' tables (uint8 numpy [n, 4, 272])."""
    encode = mjpeg_encode_optimized if optimize else mjpeg_encode
    res = encode(u8, quality, restart_mcus, sampling=sampling)
    off = res[1].cpu().tolist()
    if off[-1] > res[0].numel():
        res = encode(u8, quality, restart_mcus, capacity=off[-1], sampling=sampling)
    scans = res[0][:off[-1]].cpu().numpy().tobytes()
    return (scans, off, res[2].cpu().numpy()) if optimize else (scans, off)


# ------------------------------------------------------------------ lossless output stage (include/ccvs_hip_output_lossless.h)
def png_encode(u8, filter=-1, band_rows=0, capacity=None, out=None, lz77=False):
    """One zlib stream per frame of uint8 frames [..., H, W, 3] on the device (`ccvs_apng_encode`): PNG's row
    filters, then Huffman-only deflate with dynamic tables -- the payload of a PNG IDAT / APNG fdAT chunk (`ccvs_amd.tools.apng`
    writes the container).  Returns (stream uint8 [capacity], offsets int64 [n + 1]), both on the device -- frame i's stream is
    stream[offsets[i]:offsets[i + 1]].  filter: -1 = per row the type with the smallest sum of |signed byte| (libpng's heuristic),
    0 .. 4 = None, Sub, Up, Average, Paeth for every row.  band_rows: rows per deflate block (0: about 32 KiB of filtered bytes).
    Frames and strides are handled as in `mjpeg_encode`.  capacity: bytes of `stream` (None: 9/8 of the filtered size plus 470 bytes
    per band, which noise does not fill); the offsets are complete also when offsets[n] > capacity, nothing at or beyond `capacity` is
    written, and the CALLER runs again with a larger one (`png_encode_to_host` does; `ccvs_apng_stream_bound` always suffices).
    out: optional uint8 stream to write into (its length is the capacity).  Runs on the current stream; nothing is synchronised.
    lz77: the deflate blocks may hold LZ77 matches (`ccvs_apng_encode_lz`); per block the form with fewer bits
    is written, so no frame's stream is longer than without and the default capacity suffices as before.  Flat and structured frames
    shrink several times; the encode takes longer."""
    _need_gpu(u8, out)
    assert u8.dtype == torch.uint8 and u8.dim() >= 3 and u8.shape[-1] == 3, (u8.dtype, u8.shape)
    h, w = int(u8.shape[-3]), int(u8.shape[-2])
    frames = u8.reshape(1, h, w, 3) if u8.dim() == 3 else u8
    if frames.stride()[-3:] != (3 * w, 3, 1):
        frames = frames.contiguous()
    if frames.dim() > 4:
        try:
            frames = frames.view(-1, h, w, 3)      # leading axes of one regular stride
        except RuntimeError:
            frames = frames.reshape(-1, h, w, 3)
    n, filter, band_rows = int(frames.shape[0]), int(filter), int(band_rows)
    if n > 1 and frames.stride(0) < 3 * w * h:     # (an expanded frame axis)
        frames = frames.contiguous()
    L = _lib.load()
    if out is not None:
        assert out.dtype == torch.uint8 and out.dim() == 1 and out.is_contiguous() and capacity in (None, out.numel()), (out.dtype, out.shape)
        capacity = out.numel()
    elif capacity is None:
        rows = band_rows if band_rows > 0 else max(1, 32768 // (3 * w + 1))
        capacity = n * (6 + h * (3 * w + 1) * 9 // 8 + 470 * ((h + rows - 1) // rows))
    stream = out if out is not None else torch.empty(int(capacity), dtype=torch.uint8, device=u8.device)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=u8.device)
    size, encode, who = ((L.ccvs_apng_lz_workspace_bytes, L.ccvs_apng_encode_lz, "ccvs_apng_encode_lz") if lz77 else
                         (L.ccvs_apng_workspace_bytes, L.ccvs_apng_encode, "ccvs_apng_encode"))
    work = torch.empty(max(int(size(n, h, w, max(band_rows, 0))), 8), dtype=torch.uint8, device=u8.device)
    _lib.check(encode(_p(frames), frames.stride(0) if n > 1 else h * w * 3, n, h, w, filter, band_rows, _p(stream), int(capacity),
                      _p(offsets), _p(work), _stream()), who)
    return stream, offsets


def png_encode_to_host(u8, filter=-1, band_rows=0, lz77=False):
    """`png_encode`, then the streams on the host: (bytes of all frames' zlib streams, list of n + 1 offsets).  Where the first run's
    stream is too small the offsets say by how much and a second run with that capacity is exact.  What crosses to the host is the
    offsets and offsets[n] compressed bytes."""
    stream, offsets = png_encode(u8, filter, band_rows, lz77=lz77)
    off = offsets.cpu().tolist()
    if off[-1] > stream.numel():
        stream, offsets = png_encode(u8, filter, band_rows, capacity=off[-1], lz77=lz77)
    return stream[:off[-1]].cpu().numpy().tobytes(), off


# ------------------------------------------------------------------ GIF output stage (include/ccvs_hip_output_gif.h)
def _gif_clips(who, u8):
    """The clips [B, T, H, W, 3] (or one clip [T, H, W, 3]) as the C calls take them: (clips, b, t, h, w, clip stride, frame stride)."""
    assert u8.dtype == torch.uint8 and u8.dim() in (4, 5) and u8.shape[-1] == 3, (who, u8.dtype, u8.shape)
    clips = u8.unsqueeze(0) if u8.dim() == 4 else u8
    b, t, h, w = (int(v) for v in clips.shape[:4])
    frame = 3 * w * h
    if clips.stride()[-3:] != (3 * w, 3, 1):
        clips = clips.contiguous()
    fs = clips.stride(1) if t > 1 else frame
    cs = clips.stride(0) if b > 1 else (t - 1) * fs + frame
    if fs < frame or cs < (t - 1) * fs + frame:       # (an expanded or interleaved axis)
        clips = clips.contiguous()
        fs, cs = frame, t * frame
    return clips, b, t, h, w, cs, fs


def _gif_palette(L, clips, b, t, h, w, cs, fs, work, max_colours=256):
    dev = clips.device
    palette = torch.empty((b, 256, 3), dtype=torch.uint8, device=dev)
    table = torch.empty((b, 32768), dtype=torch.uint8, device=dev)
    used = torch.empty(b, dtype=torch.int32, device=dev)
    if max_colours == 256:
        _lib.check(L.ccvs_gif_palette(_p(clips), cs, fs, b, t, h, w, _p(palette), _p(table), _p(used), _p(work), _stream()), "ccvs_gif_palette")
    else:
        _lib.check(L.ccvs_gif_palette_n(_p(clips), cs, fs, b, t, h, w, int(max_colours), _p(palette), _p(table), _p(used), _p(work), _stream()),
                   "ccvs_gif_palette_n")
    return palette, table, used


def gif_palette(u8_clips, max_colours=256):
    """The colour tables of uint8 clips [B, T, H, W, 3] on the device (`ccvs_gif_palette`), one per clip from that
    clip's own pixels: (palette uint8 [B, 256, 3], table uint8 [B, 32768], used int32 [B]), all on the device.  The pixels are counted
    in 32768 bins of 5 bits per channel, median cut makes up to 256 boxes of the occupied bins, a box's mean colour is its palette
    entry (`used` of them; the rest are 0) and `table` gives every bin's entry: a pixel's index is table[(R >> 3) << 10 | (G >> 3) << 5 |
    B >> 3].  A [T, H, W, 3] input is one clip.  Views whose rows are dense and whose frame and clip strides hold a frame / a clip are
    read in place.  max_colours (2 .. 256): the median cut stops at so many boxes (`ccvs_gif_palette_n`; 255
    leaves index 255 free for the changed-rectangle frames' transparency).  Runs on the current stream; nothing is synchronised."""
    _need_gpu(u8_clips)
    clips, b, t, h, w, cs, fs = _gif_clips("gif_palette", u8_clips)
    L = _lib.load()
    work = torch.empty(max(int(L.ccvs_gif_workspace_bytes(b, t, h, w, 0)), 8), dtype=torch.uint8, device=clips.device)
    return _gif_palette(L, clips, b, t, h, w, cs, fs, work, max_colours)


def gif_encode(u8_clips, band_rows=0, capacity=None, out=None, delta=False):
    """The GIF image data of uint8 clips [B, T, H, W, 3] on the device (`ccvs_gif_palette`, then `ccvs_gif_encode`, DESIGN.md section
    4.27): every clip's pixels are mapped to its own 256 colours (`gif_palette`) and every frame's indices are LZW-coded on the GPU and
    framed in sub-blocks -- what follows an image descriptor in a GIF file (`ccvs_amd.tools.gif` writes the container).  Returns
    (stream uint8 [capacity], offsets int64 [B T + 1], palette uint8 [B, 256, 3]), all on the device -- frame j of clip i is
    stream[offsets[i T + j]:offsets[i T + j + 1]].  band_rows: rows per independently coded band (0: about 4096 pixels).  Clips and
    strides are handled as in `gif_palette`.  capacity: bytes of `stream` (None: a byte per pixel, which noise overflows); the offsets
    are complete also when offsets[n] > capacity, nothing at or beyond `capacity` is written, and the CALLER runs again with a larger one
    (`gif_encode_to_host` does; `ccvs_gif_stream_bound` always suffices).  out: optional uint8 stream to write into (its length is the
    capacity).  delta: changed-rectangle frames (`ccvs_gif_palette_n` at 255 colours, then `ccvs_gif_encode_delta`, DESIGN.md section
    4.29): a frame after its clip's first is written as the rectangle of what changed against the frame before, index 255 transparent,
    where that is fewer bytes; a fourth result, rects int32 [B T, 4], holds every written frame's x0, y0, width and height.  Runs on the
    current stream; nothing is synchronised."""
    _need_gpu(u8_clips, out)
    clips, b, t, h, w, cs, fs = _gif_clips("gif_encode", u8_clips)
    n, band_rows = b * t, int(band_rows)
    L = _lib.load()
    if out is not None:
        assert out.dtype == torch.uint8 and out.dim() == 1 and out.is_contiguous() and capacity in (None, out.numel()), (out.dtype, out.shape)
        capacity = out.numel()
    elif capacity is None:
        capacity = n * (2 + h * w + (h * w + 254) // 255)
    stream = out if out is not None else torch.empty(int(capacity), dtype=torch.uint8, device=clips.device)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=clips.device)
    if delta:
        work = torch.empty(max(int(L.ccvs_gif_delta_workspace_bytes(b, t, h, w, max(band_rows, 0))), 8), dtype=torch.uint8, device=clips.device)
        palette, table, _ = _gif_palette(L, clips, b, t, h, w, cs, fs, work, 255)
        rects = torch.empty((n, 4), dtype=torch.int32, device=clips.device)
        _lib.check(L.ccvs_gif_encode_delta(_p(clips), cs, fs, b, t, h, w, band_rows, _p(table), _p(stream), int(capacity), _p(offsets),
                                           _p(rects), _p(work), _stream()), "ccvs_gif_encode_delta")
        return stream, offsets, palette, rects
    work = torch.empty(max(int(L.ccvs_gif_workspace_bytes(b, t, h, w, max(band_rows, 0))), 8), dtype=torch.uint8, device=clips.device)
    palette, table, _ = _gif_palette(L, clips, b, t, h, w, cs, fs, work)
    _lib.check(L.ccvs_gif_encode(_p(clips), cs, fs, b, t, h, w, band_rows, _p(table), _p(stream), int(capacity), _p(offsets), _p(work),
                                 _stream()), "ccvs_gif_encode")
    return stream, offsets, palette


def gif_encode_to_host(u8_clips, band_rows=0, delta=False):
    """`gif_encode`, then its results on the host: (bytes of all frames' payloads, list of B T + 1 offsets, palettes uint8 numpy
    [B, 256, 3]).  Where the first run's stream is too small the offsets say by how much and a second run with that capacity is exact.
    What crosses to the host is the offsets, offsets[n] coded bytes and 768 palette bytes per clip.  delta: `gif_encode(delta=True)`;
    a fourth result, the written rectangles as int32 numpy [B T, 4]."""
    if not delta:
        stream, offsets, palette = gif_encode(u8_clips, band_rows)
        off = offsets.cpu().tolist()
        if off[-1] > stream.numel():
            stream, offsets, palette = gif_encode(u8_clips, band_rows, capacity=off[-1])
        return stream[:off[-1]].cpu().numpy().tobytes(), off, palette.cpu().numpy()
    stream, offsets, palette, rects = gif_encode(u8_clips, band_rows, delta=True)
    off = offsets.cpu().tolist()
    if off[-1] > stream.numel():
        stream, offsets, palette, rects = gif_encode(u8_clips, band_rows, capacity=off[-1], delta=True)
    return stream[:off[-1]].cpu().numpy().tobytes(), off, palette.cpu().numpy(), rects.cpu().numpy()


# ------------------------------------------------------------------ the way back (include/ccvs_hip_decode.h)
_MJPEG_STATUS = {1: "its table entry points outside the call's frames, stream, MCUs or tables", 2: "no Huffman code starts so",
                 3: "the MCUs need more bits than the unit has", 4: "a run leads past coefficient 63",
                 5: "bytes are left behind the last MCU, or a 0xFF that no 0x00 follows"}


def mjpeg_decode_pack(plan):
    """A plan of `ccvs_amd.tools.mjpeg.plan_frames` as ONE host blob (uint8 numpy): the unit table, the table records, the frames' record
    indices and the scans, each part at the alignment `ccvs_mjpeg_decode` asks for.  Returns (meta, blob): `meta` with the blob on the
    device under "blob" (a uint8 tensor whose first byte is 8-byte aligned) is what `mjpeg_decode_uploaded` takes -- callers that
    batch several plans into one upload (`ccvs_amd.data.VideoLoader`) place the blobs themselves."""
    import numpy as np
    n, h, w, sampling = (int(plan[k]) for k in ("n", "h", "w", "sampling"))
    units = np.ascontiguousarray(plan["units"], dtype=np.int64).reshape(-1, 5)
    tables = np.ascontiguousarray(plan["tables"], dtype=np.uint8).reshape(-1)
    frame_table = np.ascontiguousarray(plan["frame_table"], dtype=np.int32).reshape(-1)
    scans = np.ascontiguousarray(plan["scans"], dtype=np.uint8).reshape(-1)
    assert frame_table.size == n and tables.size % 4008 == 0, (frame_table.size, n, tables.size)
    o_tab = units.nbytes                                  # (a multiple of 8; 4008 is one too)
    o_ft = o_tab + tables.nbytes
    o_scan = (o_ft + frame_table.nbytes + 7) & ~7
    blob = np.zeros(o_scan + max(scans.size, 1), dtype=np.uint8)
    blob[:o_tab] = units.view(np.uint8).reshape(-1)
    blob[o_tab:o_ft] = tables
    blob[o_ft:o_ft + frame_table.nbytes] = frame_table.view(np.uint8)
    blob[o_scan:o_scan + scans.size] = scans
    return {"n": n, "h": h, "w": w, "sampling": sampling, "units_host": units, "o_tab": o_tab, "o_ft": o_ft,
            "o_scan": o_scan, "scan_bytes": scans.size, "n_tables": tables.size // 4008}, blob


def mjpeg_decode_upload(plan):
    """A plan of `ccvs_amd.tools.mjpeg.plan_frames` on the device: the unit table, the table records, the frames' record indices and
    the scans go up in ONE copy (each part at the alignment `ccvs_mjpeg_decode` asks for).  Returns what `mjpeg_decode_uploaded` takes."""
    meta, blob = mjpeg_decode_pack(plan)
    meta["blob"] = torch.from_numpy(blob).to("cuda")
    return meta


def mjpeg_decode_uploaded(up, out=None, status=None, work=None):
    """`ccvs_mjpeg_decode` on an uploaded plan: (frames uint8 [n, H, W, 3], status int32 [units]), both on the device; status[k] == 0:
    unit k (row k of the plan's unit table) decoded exactly its MCUs within its bytes.  out: optional uint8 [n, H, W, 3] to write into,
    frames dense, any frame stride of at least a frame (a slice of a larger clip); only its own bytes are written.  status / work:
    optional buffers to reuse.  Runs on the current stream; nothing is synchronised."""
    n, h, w, sampling = up["n"], up["h"], up["w"], up["sampling"]
    dev = up["blob"].device
    if out is not None:
        _need_gpu(out)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (n, h, w, 3) and out.stride()[1:] == (3 * w, 3, 1) and (n == 1 or out.stride(0) >= 3 * h * w), \
            (out.dtype, out.shape, out.stride())
    else:
        out = torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev)
    units = up["units_host"]
    L = _lib.load()
    if status is None:
        status = torch.empty(units.shape[0], dtype=torch.int32, device=dev)
    if work is None:
        work = torch.empty(max(int(L.ccvs_mjpeg_decode_workspace_bytes(n, h, w, sampling)), 16), dtype=torch.uint8, device=dev)
    base = up["blob"].data_ptr()
    _lib.check(L.ccvs_mjpeg_decode(C.c_void_p(base + up["o_scan"]), up["scan_bytes"], C.c_void_p(base), units.ctypes.data_as(C.c_void_p), units.shape[0],
                                   C.c_void_p(base + up["o_tab"]), up["n_tables"], C.c_void_p(base + up["o_ft"]), n, h, w, sampling,
                                   _p(out), out.stride(0) if n > 1 else 3 * h * w, _p(status), _p(work), _stream()), "ccvs_mjpeg_decode")
    return out, status


def mjpeg_decode_planned(plan, out=None):
    """Upload and decode a plan of `ccvs_amd.tools.mjpeg.plan_frames`: (frames, status) as `mjpeg_decode_uploaded` returns them."""
    return mjpeg_decode_uploaded(mjpeg_decode_upload(plan), out)


def mjpeg_decode(jpegs, out=None, check=True):
    """uint8 [T, H, W, 3] on the device of T baseline JPEG files (bytes) of one size and sampling -- libjpeg's pixels, bit for bit
    (DESIGN.md section 4.16).  The files are parsed on the host (`ccvs_amd.tools.mjpeg.plan_frames`: ValueError names the frame and what
    is malformed or not decoded), everything else runs on the GPU.  check=True reads the units' status words back -- the call's one
    synchronisation -- and raises ValueError naming the frame and the unit that failed; check=False returns (frames, status) on the
    device for callers that batch (see `mjpeg_decode_uploaded`)."""
    from .tools import mjpeg as _mjpeg
    plan = _mjpeg.plan_frames(jpegs)
    frames, status = mjpeg_decode_planned(plan, out)
    if not check:
        return frames, status
    st = status.cpu().numpy()
    if st.any():
        k = int(st.nonzero()[0][0])
        frame = int(plan["units"][k, 0])
        unit = k - int((plan["units"][:k, 0] < frame).sum())
        raise ValueError(f"mjpeg_decode: frame {frame}, unit {unit} (MCUs {int(plan['units'][k, 3])} .. {int(plan['units'][k, 3] + plan['units'][k, 4]) - 1}) "
                         f"failed with status {int(st[k])}: {_MJPEG_STATUS.get(int(st[k]), 'unknown')}; {int((st != 0).sum())} of {st.size} units failed")
    return frames


def read_avi_clips(paths):
    """uint8 [N, T, H, W, 3] on the device of N Motion-JPEG AVI files of equal size and length (`tools.mjpeg.read_avi`), all frames in
    one decode call."""
    from .tools import mjpeg as _mjpeg
    clips = [_mjpeg.read_avi(p) for p in paths]
    if not clips:
        raise ValueError("read_avi_clips: no files")
    h, w, t = clips[0][1], clips[0][2], len(clips[0][3])
    for p, c in zip(paths, clips):
        if (c[1], c[2], len(c[3])) != (h, w, t) or t == 0:
            raise ValueError(f"read_avi_clips: {p} holds {len(c[3])} frames of {c[1]} x {c[2]}, {paths[0]} {t} of {h} x {w}")
    try:
        frames = mjpeg_decode([f for c in clips for f in c[3]])
    except ValueError as exc:
        raise ValueError(f"read_avi_clips: {exc} (frames count through the files in order, {t} per file; the first is {paths[0]})") from None
    return frames.view(len(paths), t, h, w, 3)


# ------------------------------------------------------------------ the way back from the lossless stage (include/ccvs_hip_decode_lossless.h)
PD_OK, PD_BAD_STREAM, PD_BAD_HEADER, PD_BAD_BLOCK, PD_BAD_TABLE, PD_BAD_CODE, PD_BAD_DISTANCE, PD_OVERRUN, PD_TOO_LONG, PD_TOO_SHORT, PD_BAD_CHECK, PD_BAD_FILTER = range(12)
PD_STATUS = {
    PD_OK: ("OK", "decoded"), PD_BAD_STREAM: ("BAD_STREAM", "the table row points outside the call's buffers"),
    PD_BAD_HEADER: ("BAD_HEADER", "no zlib header of method 8 and a window of up to 32768, or it asks for a dictionary"),
    PD_BAD_BLOCK: ("BAD_BLOCK", "block type 3, or a stored block whose LEN is not ~NLEN"),
    PD_BAD_TABLE: ("BAD_TABLE", "a dynamic block's code lengths are no set zlib accepts"), PD_BAD_CODE: ("BAD_CODE", "no code starts so, or a symbol above the last"),
    PD_BAD_DISTANCE: ("BAD_DISTANCE", "a match reaches before the first byte"), PD_OVERRUN: ("OVERRUN", "the input ended"),
    PD_TOO_LONG: ("TOO_LONG", "more output than expected"), PD_TOO_SHORT: ("TOO_SHORT", "the final block ended before the expected output was there"),
    PD_BAD_CHECK: ("BAD_CHECK", "the Adler-32 is not that of the output"), PD_BAD_FILTER: ("BAD_FILTER", "a row's filter type is above 4"),
}


def _pd_pack(streams, row):
    """The table (int64 [n][len(row(0, 0, 0))]) and the streams as ONE host blob (uint8 numpy): the table first, the streams one behind
    the other.  Returns (the table on the host, the blob, the streams' offset in it, their bytes)."""
    import numpy as np
    streams = [bytes(s) for s in streams]
    rows, pos = [], 0
    for i, s in enumerate(streams):
        rows.append(row(i, pos, len(s)))
        pos += len(s)
    table = np.ascontiguousarray(rows, dtype=np.int64)
    blob = np.zeros(table.nbytes + max(pos, 1), dtype=np.uint8)        # (the table's bytes are a multiple of 8)
    blob[:table.nbytes] = table.view(np.uint8).reshape(-1)
    blob[table.nbytes:table.nbytes + pos] = np.frombuffer(b"".join(streams), np.uint8)
    return table, blob, table.nbytes, pos


def _pd_raise(who, st, what, total=None):
    k = int(st.nonzero()[0][0])
    word, why = PD_STATUS.get(int(st[k]), ("?", "unknown"))
    raise ValueError(f"{who}: {what} {k} failed with status {int(st[k])} ({word}: {why}); {int((st != 0).sum())} of {st.size if total is None else total} failed")


def zlib_inflate(streams, sizes, check=True, out=None, offsets=None):
    """n zlib streams (bytes each) inflated on the GPU (`ccvs_zlib_inflate`): a complete RFC 1950 / 1951 inflate
    under zlib's acceptance rules.  sizes[i]: the bytes stream i is to hold.  Returns a uint8 tensor on the device with stream i's
    bytes at offsets[i] (default: one behind the other); out: optional uint8 tensor to write into -- only the streams' own ranges are
    written.  The table and the streams go up in ONE copy.  check=True reads the status words back -- the call's one synchronisation --
    and raises ValueError naming the first failed stream and its status word; check=False returns (out, status int32 [n]) on the
    device.  Runs on the current stream."""
    sizes = [int(v) for v in sizes]
    streams = list(streams)
    if not streams or len(sizes) != len(streams) or min(sizes) < 0:
        raise ValueError(f"zlib_inflate: {len(streams)} streams, {len(sizes)} sizes (none may be negative)")
    if offsets is None:
        offsets, pos = [], 0
        for v in sizes:
            offsets.append(pos)
            pos += v
    table, blob, o_data, data_bytes = _pd_pack(streams, lambda i, pos, n: (pos, n, int(offsets[i]), sizes[i]))
    if not torch.cuda.is_available():
        raise _lib.CcvsError("zlib_inflate needs a GPU: there is no CPU fallback")
    up = torch.from_numpy(blob).to("cuda")
    if out is None:
        out = torch.empty(max(max(o + v for o, v in zip(offsets, sizes)), 1), dtype=torch.uint8, device=up.device)
    _need_gpu(out)
    assert out.dtype == torch.uint8 and out.is_contiguous(), (out.dtype, out.stride())
    status = torch.empty(len(streams), dtype=torch.int32, device=up.device)
    base = up.data_ptr()
    _lib.check(_lib.load().ccvs_zlib_inflate(C.c_void_p(base + o_data), data_bytes, C.c_void_p(base), table.ctypes.data_as(C.c_void_p), len(streams),
                                             _p(out), out.numel(), _p(status), _stream()), "ccvs_zlib_inflate")
    if not check:
        return out, status
    st = status.cpu().numpy()
    if st.any():
        _pd_raise("zlib_inflate", st, "stream")
    return out


def png_decode_pack(streams, h, w):
    """The zlib streams of n 8-bit RGB PNG images of h x w as ONE host blob (uint8 numpy): the table of (offset, bytes) rows, then
    the streams.  Returns (meta, blob): `meta` with the blob on the device under "blob" (a uint8 tensor whose first byte is 8-byte
    aligned) is what `png_decode_uploaded` takes -- callers that batch (`ccvs_amd.data.FrameLoader`) upload the blob themselves."""
    streams = list(streams)
    if not streams or not (1 <= int(h) <= 65535 and 1 <= int(w) <= 65535):
        raise ValueError(f"png_decode: {len(streams)} streams of {h} x {w} (sizes are 1 .. 65535)")
    table, blob, o_data, data_bytes = _pd_pack(streams, lambda i, pos, n: (pos, n))
    return {"n": len(streams), "h": int(h), "w": int(w), "rows_host": table, "o_data": o_data, "data_bytes": data_bytes}, blob


def png_decode_uploaded(up, out=None, status=None, work=None):
    """`ccvs_png_decode` on an uploaded pack: (frames uint8 [n, H, W, 3], status int32 [n]), both on the device; status[i] == 0: frame i
    inflated to exactly its h (3 w + 1) filtered bytes with the right Adler-32 and every row's filter type was 0 .. 4.  out: optional
    uint8 [n, H, W, 3] to write into, frames dense, any frame stride of at least a frame; only its own bytes are written.  status /
    work: optional buffers to reuse.  Runs on the current stream; nothing is synchronised."""
    n, h, w = up["n"], up["h"], up["w"]
    dev = up["blob"].device
    if out is not None:
        _need_gpu(out)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (n, h, w, 3) and out.stride()[1:] == (3 * w, 3, 1) and (n == 1 or out.stride(0) >= 3 * h * w), \
            (out.dtype, out.shape, out.stride())
    else:
        out = torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev)
    L = _lib.load()
    if status is None:
        status = torch.empty(n, dtype=torch.int32, device=dev)
    if work is None:
        work = torch.empty(max(int(L.ccvs_png_decode_workspace_bytes(n, h, w)), 16), dtype=torch.uint8, device=dev)
    base = up["blob"].data_ptr()
    _lib.check(L.ccvs_png_decode(C.c_void_p(base + up["o_data"]), up["data_bytes"], C.c_void_p(base), up["rows_host"].ctypes.data_as(C.c_void_p), n, h, w,
                                 _p(out), out.stride(0) if n > 1 else 3 * h * w, _p(status), _p(work), _stream()), "ccvs_png_decode")
    return out, status


def png_decode(streams, h, w, out=None, check=True):
    """uint8 [n, H, W, 3] on the device of the zlib streams (bytes each: a PNG's concatenated IDAT payload, `tools.apng.apng_streams`) of n
    8-bit RGB images of h x w -- inflated and un-filtered on the GPU, the bytes `tools.apng.read_apng` gives.
    One upload.  check=True reads the status words back -- the call's one synchronisation -- and raises ValueError naming the frame,
    the status word and how many failed; check=False returns (frames, status) on the device (see `png_decode_uploaded`)."""
    meta, blob = png_decode_pack(streams, h, w)
    if not torch.cuda.is_available():
        raise _lib.CcvsError("png_decode needs a GPU: there is no CPU fallback")
    meta["blob"] = torch.from_numpy(blob).to("cuda")
    frames, status = png_decode_uploaded(meta, out)
    if not check:
        return frames, status
    st = status.cpu().numpy()
    if st.any():
        _pd_raise("png_decode", st, "frame")
    return frames


def read_apng_clips(paths):
    """uint8 [N, T, H, W, 3] on the device of N PNG / APNG files of equal size and length (`tools.apng.apng_streams`), all frames of all
    files in one decode call: only the compressed bytes cross to the device."""
    from .tools import apng as _apng
    clips = [_apng.apng_streams(p) for p in paths]
    if not clips:
        raise ValueError("read_apng_clips: no files")
    h, w, t = clips[0][0], clips[0][1], len(clips[0][2])
    for p, c in zip(paths, clips):
        if (c[0], c[1], len(c[2])) != (h, w, t) or t == 0:
            raise ValueError(f"read_apng_clips: {p} holds {len(c[2])} frames of {c[0]} x {c[1]}, {paths[0]} {t} of {h} x {w}")
    try:
        frames = png_decode([z for c in clips for z in c[2]], h, w)
    except ValueError as exc:
        raise ValueError(f"read_apng_clips: {exc} (frames count through the files in order, {t} per file; the first is {paths[0]})") from None
    return frames.view(len(paths), t, h, w, 3)

"""Float64 mirror of the flow decoder's gather kernels (`backwarp_kernel`, `backwarp_p8_kernel`, `warp_proj_kernel`,
`warp_proj4_kernel`, `warp_fuse_blend_kernel`, `warp_fuse_blend4_kernel`; ccvs_amd/csrc/flow.hip) with a derived per-element
error bound, the wrong readings of the reference that the bound has to tell from the right one, and the case table that the
host test (test_warp_ref_host.py) and the GPU test (test_warp_forms_gpu.py) share.  Plain torch, runs anywhere.

The operations (skip_autoencoder.py:120-128, 186-190, 254-264), F = flow * mult, per axis of size W (H likewise):

    g   = linspace(-1 + 1/W, 1 - 1/W, W)[x] + F / ((W - 1) / 2)          the reference's grid, = (2x + 1)/W - 1 + 2F/(W - 1)
    ix  = ((g + 1) W - 1) / 2                                            grid_sample, align_corners=False
        = x + F W / (W - 1)                                              `positions`: the two lines above in float64
    v   = ((x00 w00 + x01 w01) + x10 w10) + x11 w11                      corners outside the image count as 0
    y   = lrelu(b + sum_c W_oc v_c / sqrt(Cin))                          warp + projection
    conf_j = (1 - sigmoid(o_j)) + 1e-6,  S = sum_j conf_j,  p_j = conf_j / S          (k > 1;  k == 1: p = 1, occ = o)
    wi  = sum_j p_j v_j,   occ = sum_j p_j o_j,   m = sigmoid(occ),   out = m dec + (1 - m) wi

The bound.  eps = 2**-24 (unit roundoff of fp32), gamma_n = n eps / (1 - n eps).  Every term comes from counting the fp32
roundings of the reference's chain (torch on a CPU) and of the kernels' (`bilin_pos` and the bodies); nothing is fitted to a result.

 1. Coordinate, in units of g (every magnitude below is <= 1 unless stated), u = 2F/(W - 1):
      linspace: start = fl(-1 + 1/W) 1;  step = fl(fl(end - start) / (W - 1)): the two end points and the difference (~2) cost
      (1 + 1 + 2)/(W - 1), the quotient 2/(W - 1), times an index <= W/2: 3 W/(W - 1);  base = fl(start + fl(step i)) 2;  the
      vector lane fl(base + fl(step l)) 2:  5 + 3 W/(W - 1).  The kernel's fl(fl((2x + 1)/W) - 1) is 2 roundings of <= 2, within it.
      u: fl(f mult) and the quotient by the exact (W - 1)/2:  2 |u|.        g = fl(lin + u):  1 + |u|.
      |dg| <= eps (6 + 3 W/(W - 1) + 3 |u|);  each unit of g is worth W/2 pixels.
    Un-normalisation, in pixels: fl(g + 1) and fl(. W) (or . W/2) each eps |ix + 1/2|, fl(. - 1) (or - 1/2) eps (|ix| + 1/2),
      the halving exact, and tx = fl(ix - floor(ix)) at most eps:  eps (3 |ix| + 2.5), with |ix| <= W - 1 + |F| W/(W - 1).
      delta_pos(W, |F|) = eps (6 W - 1/2 + 3 W^2 / (2 (W - 1)) + 6 |F| W / (W - 1))        pixels, reference and kernel alike
    The bilinear interpolant with zero padding is continuous and, inside a cell, changes by at most G = max(|x01 - x00|,
    |x11 - x10|, |x10 - x00|, |x11 - x01|) per pixel along either axis.  A position that is off by (dx, dy) = (delta_pos(W, |Fx|),
    delta_pos(H, |Fy|)) stays in the cells of the nine points (ix + {-dx, 0, dx}, iy + {-dy, 0, dy}) (delta_pos < 1/2 is asserted):
      coordinate part = (dx + dy) G9         G9, A9: the largest G, A over those nine points       (= 2 delta_pos G for a square image)
 2. Weights and sum: 1 - tx, 1 - ty and their product 3 roundings per weight, the product with the corner 1, the three additions 3:
      weight and sum part = gamma_7 A9,      A = sum_i |w_i| |x_i|,   n = 7
    A position more than 1 + delta_pos outside [0, W-1] (or [0, H-1]) has all four corners outside in fp32 too: the result is
    exactly 0 (`far`; tol = 0 there).  Flows must be finite and H, W >= 2: the reference divides by (W - 1)/2 and casts a
    non-finite coordinate to an integer, so its result there is not defined and nothing here speaks about it.
 3. Projection: w = fl(fl(1/sqrt(Cin)) W_oc) 2, product 1, Cin - 1 additions in any order, the bias 1, the slope 0.1f and its
    product 2:      tol_y = sum_c |w_oc| tol_v_c + gamma_{Cin+5} (|b_o| + sum_c |w_oc| A9_c)
 4. Fusion and blend.  sigmoid as 1 / (1 + exp(-o)) (torch's CPU kernel and the HIP kernels alike), exp to 2 ulp = 4 eps (both
    libraries document 1 ulp), e = exp(-o), s = 1 + e; a rounding to nearest errs by no more than the distance to ANY representable
    number, 1 in particular:
      d_s = 4 eps e + min(eps s, e)         d_sig(o) = d_s / s^2 + min(eps sig, 1 - sig) + 1e-37   (1e-37: exp overflow / denormals)
      d_conf = d_sig + [sig < 1/2] eps (1 - sig) + eps 1e-6 + eps conf         (1 - sig is exact for sig >= 1/2; fl(1e-6); the sum)
      d_S = sum_j d_conf_j + gamma_{k-1} S          d_p_j = (d_conf_j + p_j d_S) / (S - d_S)          (d_S < S is asserted)
    occ and wi are weighted means, so a change of the weights moves them by the spread of what is averaged, not by its size:
      d_occ = sum_j d_p_j |o_j - occ| + gamma_{k+1} sum_j (p_j + d_p_j) |o_j|               (product, k - 1 additions, quotient)
      d_m   = max(sig(occ + d_occ) - m, m - sig(occ - d_occ)) + max d_sig(occ, occ +- d_occ)            (sigmoid is monotone)
      d_wi  = sum_j d_p_j |v_j - wi| + sum_j (p_j + d_p_j) (tol_v_j + gamma_{k+1} A9_j)
      tol_out = d_m (|dec - wi| + d_wi) + (1 - m) d_wi + eps (1 - m) |wi| + gamma_3 (m |dec| + (1 - m) |wi|)
    k == 1: p = 1, d_p = 0, d_occ = 0, d_wi = tol_v.  Where every o_j >= 30, 1 - m < 1e-13 and tol_out is a few ulp of dec.
 All of it is first order; the total is multiplied by 1 + 2**-10 for the products of two error terms.

This is a derivation, not a measurement."""
import functools
import math
import re
import zlib
from collections import namedtuple

import torch

EPS32 = 2.0 ** -24
SECOND_ORDER = 1.0 + 2.0 ** -10
N_SUM = 7                     # n of gamma_n in the weight and sum part
LRELU_SLOPE = 0.1


def gamma(n):
    return n * EPS32 / (1.0 - n * EPS32)


def delta_pos(size, fabs):
    """Upper bound, in pixels, of |fp32 sample coordinate - positions()| along an axis of `size` pixels for |flow * mult| = fabs
    (a number or a float64 tensor), for the reference's chain and for `bilin_pos`."""
    r = size / (size - 1.0)
    return EPS32 * (6.0 * size - 0.5 + 1.5 * size * r + 6.0 * fabs * r)


# ---------------------------------------------------------------- the mirror
def _axis(lin, f, size, norm):
    """The reference's own expressions, operation by operation, in float64 (x + F W/(W - 1) to 1e-14 of a pixel)."""
    if norm == "half_size":                # flow normalised by W / 2
        g = lin + f / (size / 2.0)
    else:
        g = lin + f / ((size - 1.0) / 2.0)
    if norm == "align_corners":
        return (g + 1) / 2 * (size - 1)
    return ((g + 1) * size - 1) / 2


def positions(flow, mult, H, W, norm="ref", swap=False):
    """flow [N,2,H,W] -> float64 sample positions (ix, iy), each [N,H,W], of the reference's backwarp (skip_autoencoder.py:120-128)
    followed by the un-normalisation of grid_sample(align_corners=False)."""
    f = flow.double() * mult
    fx, fy = (f[:, 1], f[:, 0]) if swap else (f[:, 0], f[:, 1])
    hor = torch.linspace(-1.0 + (1.0 / W), 1.0 - (1.0 / W), W, dtype=torch.float64).view(1, 1, W)
    ver = torch.linspace(-1.0 + (1.0 / H), 1.0 - (1.0 / H), H, dtype=torch.float64).view(1, H, 1)
    return _axis(hor, fx, W, norm), _axis(ver, fy, H, norm)


def _sample_at(x, ix, iy, padding="zeros"):
    """Bilinear sample of x [N,C,H,W] float64 at (ix, iy) [N,H,W]: (value, A, G), each [N,C,H,W]."""
    n, c, h, w = x.shape
    if padding == "border":
        ix, iy = ix.clamp(0, w - 1), iy.clamp(0, h - 1)
    x0f, y0f = torch.floor(ix), torch.floor(iy)
    tx, ty = (ix - x0f).unsqueeze(1), (iy - y0f).unsqueeze(1)
    x0, y0 = x0f.clamp(-2, w + 1).long(), y0f.clamp(-2, h + 1).long()
    flat = x.reshape(n, c, h * w)

    def corner(yy, xx):
        ok = ((xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)).unsqueeze(1)
        idx = (yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)).reshape(n, 1, h * w).expand(n, c, h * w)
        return torch.gather(flat, 2, idx).reshape(n, c, h, w) * ok
    v00, v01, v10, v11 = corner(y0, x0), corner(y0, x0 + 1), corner(y0 + 1, x0), corner(y0 + 1, x0 + 1)
    w00, w01, w10, w11 = (1 - tx) * (1 - ty), tx * (1 - ty), (1 - tx) * ty, tx * ty
    val = ((v00 * w00 + v01 * w01) + v10 * w10) + v11 * w11
    a = ((v00.abs() * w00 + v01.abs() * w01) + v10.abs() * w10) + v11.abs() * w11
    g = torch.maximum(torch.maximum((v01 - v00).abs(), (v11 - v10).abs()), torch.maximum((v10 - v00).abs(), (v11 - v01).abs()))
    return val, a, g


def stack(ctxs):
    """k contexts [nf,C,H,W] -> [nf * k, C, H, W] in (frame, context) order, what the kernels' context list stands for."""
    return torch.stack(list(ctxs), dim=1).reshape(-1, *ctxs[0].shape[1:])


def backwarp(x, flow, mult, norm="ref", swap=False, padding="zeros"):
    """x [N,C,H,W], flow [N,2,H,W] -> (y, A, G) in float64: bilinear, zeros outside, at `positions`."""
    x = x.double()
    ix, iy = positions(flow, mult, x.shape[2], x.shape[3], norm, swap)
    return _sample_at(x, ix, iy, padding)


def sigmoid(o):
    return 1.0 / (1.0 + torch.exp(-o))


def _fuse_parts(dec, x, flows, occs, mult, k, conf="ref", occ_fuse="weighted", blend="ref", k1="shortcut", **warp):
    dec, o = dec.double(), occs.double()
    n, c, h, w = dec.shape
    v = backwarp(x, flows, mult, **warp)[0].view(n, k, c, h, w)
    o = o.view(n, k, 1, h, w)
    if k > 1 or k1 == "formula":
        if conf == "ref":
            cf = (1 - sigmoid(o)) + 1e-6
        elif conf == "sigmoid":
            cf = sigmoid(o) + 1e-6
        else:
            cf = 1 - sigmoid(o)
        s = cf.sum(1)
        wi = (v * cf).sum(1) / s
        occ = o.mean(1) if occ_fuse == "mean" else (o * cf).sum(1) / s
    else:
        cf = torch.ones_like(o)
        wi, occ = v[:, 0], o[:, 0]
    m = sigmoid(occ)
    out = (1 - m) * dec + m * wi if blend == "swapped" else m * dec + (1 - m) * wi
    return dict(out=out, v=v, o=o, conf=cf, wi=wi, occ=occ, m=m, dec=dec)


def fuse_blend(dec, ctxs, flows, occs, mult, k, **mut):
    """The InterBlock tail in float64.  dec [n,C,H,W]; ctxs [n*k,C,H,W] in (frame, context) order; flows [n*k,2,H,W]; occs [n*k,1,H,W]."""
    return _fuse_parts(dec, ctxs, flows, occs, mult, k, **mut)["out"]


def warp_proj(ctxs, flow, mult, weight, bias, act=True, **warp):
    """lrelu(bias + W / sqrt(Cin) . backwarp(ctxs, flow * mult)) in float64; weight [Cout,Cin,1,1]."""
    v = backwarp(ctxs, flow, mult, **warp)[0]
    cout, cin = weight.shape[:2]
    y = torch.einsum("oc,nchw->nohw", weight.double().view(cout, cin) / math.sqrt(cin), v) + bias.double().view(1, -1, 1, 1)
    return torch.where(y > 0, y, LRELU_SLOPE * y) if act else y


# ---------------------------------------------------------------- the bound
def far_mask(flow, mult, H, W):
    """[N,H,W] bool: the float64 position lies more than 1 + delta_pos outside the image along an axis: an exact 0 is due."""
    f = flow.double() * mult
    ix, iy = positions(flow, mult, H, W)
    dx, dy = delta_pos(W, f[:, 0].abs()), delta_pos(H, f[:, 1].abs())
    return (ix < -1 - dx) | (ix > W + dx) | (iy < -1 - dy) | (iy > H + dy)


def bound_backwarp(x, flow, mult):
    """(tol, A9, far): tol [N,C,H,W] for `backwarp`; tol is 0 where `far`."""
    x = x.double()
    h, w = x.shape[2:]
    f = flow.double() * mult
    assert torch.isfinite(f).all() and h >= 2 and w >= 2
    ix, iy = positions(flow, mult, h, w)
    far = far_mask(flow, mult, h, w)
    dx = torch.where(far, torch.zeros_like(ix), delta_pos(w, f[:, 0].abs()))
    dy = torch.where(far, torch.zeros_like(iy), delta_pos(h, f[:, 1].abs()))
    assert float(dx.max()) < 0.5 and float(dy.max()) < 0.5, "delta_pos must stay below half a pixel where a value is due"
    a9 = g9 = None
    for sx in (-1, 0, 1):
        for sy in (-1, 0, 1):
            _, a, g = _sample_at(x, ix + sx * dx, iy + sy * dy)
            a9 = a if a9 is None else torch.maximum(a9, a)
            g9 = g if g9 is None else torch.maximum(g9, g)
    keep = (~far).unsqueeze(1)
    a9 = a9 * keep
    tol = ((dx + dy).unsqueeze(1) * g9 + gamma(N_SUM) * a9) * keep * SECOND_ORDER
    return tol, a9, far


def bound_warp_proj(ctxs, flow, mult, weight, bias):
    """(tol [N,Cout,H,W], far)."""
    tol_v, a9, far = bound_backwarp(ctxs, flow, mult)
    cout, cin = weight.shape[:2]
    wa = weight.double().view(cout, cin).abs() / math.sqrt(cin)
    mag = torch.einsum("oc,nchw->nohw", wa, a9) + bias.double().abs().view(1, -1, 1, 1)
    tol = torch.einsum("oc,nchw->nohw", wa, tol_v) + gamma(cin + 5) * mag * SECOND_ORDER
    return tol, far


def sigmoid_err(o):
    """|fp32 sigmoid(o) - sigmoid(o)| for 1 / (1 + exp(-o)) with exp good to 2 ulp."""
    e = torch.exp(-o)
    s = 1.0 + e
    sig = 1.0 / s
    d_s = 4 * EPS32 * e + torch.minimum(EPS32 * s, e)
    return d_s / (s * s) + torch.minimum(EPS32 * sig, 1 - sig) + 1e-37


def bound_fuse_blend(dec, ctxs, flows, occs, mult, k):
    """tol [n,C,H,W] for `fuse_blend`."""
    p = _fuse_parts(dec, ctxs, flows, occs, mult, k)
    n, c, h, w = p["dec"].shape
    tol_v, a9, _ = bound_backwarp(ctxs, flows, mult)
    tol_v, a9 = tol_v.view(n, k, c, h, w), a9.view(n, k, c, h, w)
    o, v, wi, occ, m, d = p["o"], p["v"], p["wi"], p["occ"], p["m"], p["dec"]
    if k > 1:
        sig = sigmoid(o)
        cf = p["conf"]
        d_cf = sigmoid_err(o) + (sig < 0.5) * EPS32 * (1 - sig) + EPS32 * 1e-6 + EPS32 * cf
        s = cf.sum(1, keepdim=True)
        d_s = d_cf.sum(1, keepdim=True) + gamma(k - 1) * s
        assert bool((d_s < s).all())
        pj = cf / s
        d_p = (d_cf + pj * d_s) / (s - d_s)
        d_occ = (d_p * (o - occ.unsqueeze(1)).abs()).sum(1) + gamma(k + 1) * ((pj + d_p) * o.abs()).sum(1)
        d_wi = (d_p * (v - wi.unsqueeze(1)).abs()).sum(1) + ((pj + d_p) * (tol_v + gamma(k + 1) * a9)).sum(1)
    else:
        d_occ = torch.zeros_like(occ)
        d_wi = tol_v[:, 0]
    hi, lo = occ + d_occ, occ - d_occ
    d_m = torch.maximum(sigmoid(hi) - m, m - sigmoid(lo)) + torch.maximum(sigmoid_err(occ), torch.maximum(sigmoid_err(hi), sigmoid_err(lo)))
    tol = (d_m * ((d - wi).abs() + d_wi) + (1 - m) * d_wi + EPS32 * (1 - m) * wi.abs()
           + gamma(3) * (m * d.abs() + (1 - m) * wi.abs()))
    return tol * SECOND_ORDER


# ---------------------------------------------------------------- wrong readings of the reference (float64), one function each
# Each takes (op, inp) with op in OPS and inp the dict of `make_inputs`, and returns what `mirror(op, inp)` would if the
# reference were read that way.
def mirror(op, inp, **mut):
    x = stack(inp["ctxs"])
    if op == "backwarp":
        return backwarp(x, inp["flow"], inp["mult"], **mut)[0]
    if op == "warp_proj":
        return warp_proj(x, inp["flow"], inp["mult"], inp["weight"], inp["bias"], True, **mut)
    if op == "fuse_blend":
        return fuse_blend(inp["dec"], x, inp["flow"], inp["occ"], inp["mult"], inp["k"], **mut)
    raise ValueError(op)


def mut_align_corners(op, inp):
    """grid_sample(align_corners=True)."""
    return mirror(op, inp, norm="align_corners")


def mut_flow_by_half_size(op, inp):
    """Flow normalised by W / 2, H / 2 instead of (W - 1) / 2, (H - 1) / 2."""
    return mirror(op, inp, norm="half_size")


def mut_flow_xy_swapped(op, inp):
    """Flow channel 0 moves rows, channel 1 columns."""
    return mirror(op, inp, swap=True)


def mut_border_padding(op, inp):
    """padding_mode='border' instead of 'zeros'."""
    return mirror(op, inp, padding="border")


def mut_mult_dropped(op, inp):
    """The flow is used as stored, without flow_mult."""
    return mirror(op, dict(inp, mult=1.0))


def mut_conf_is_sigmoid(op, inp):
    """conf = sigmoid(occ) + 1e-6."""
    return mirror(op, inp, conf="sigmoid")


def mut_conf_without_eps(op, inp):
    """conf = 1 - sigmoid(occ): 0 / 0 where every context is occluded."""
    return mirror(op, inp, conf="no_eps")


def mut_occ_plain_mean(op, inp):
    """The fused occlusion is the plain mean of the k logits."""
    return mirror(op, inp, occ_fuse="mean")


def mut_mask_exchanged(op, inp):
    """out = (1 - m) dec + m wi."""
    return mirror(op, inp, blend="swapped")


def mut_k1_through_formula(op, inp):
    """k == 1 run through the k > 1 expressions: conf v / conf and occ conf / conf.  Since conf >= 1e-6 > 0 this is the SAME function
    of the inputs (it differs by float64 roundings only), so no bound can or should tell it apart; the host test asserts exactly that."""
    return mirror(op, inp, k1="formula")


WARP_OPS = ("backwarp", "warp_proj", "fuse_blend")
MUTATIONS = {
    "align_corners": (mut_align_corners, WARP_OPS),
    "flow_by_half_size": (mut_flow_by_half_size, WARP_OPS),
    "flow_xy_swapped": (mut_flow_xy_swapped, WARP_OPS),
    "border_padding": (mut_border_padding, WARP_OPS),
    "mult_dropped": (mut_mult_dropped, WARP_OPS),
    "conf_is_sigmoid": (mut_conf_is_sigmoid, ("fuse_blend",)),
    "conf_without_eps": (mut_conf_without_eps, ("fuse_blend",)),
    "occ_plain_mean": (mut_occ_plain_mean, ("fuse_blend",)),
    "mask_exchanged": (mut_mask_exchanged, ("fuse_blend",)),
}
EQUIVALENT_MUTATIONS = {"k1_through_formula": (mut_k1_through_formula, ("fuse_blend",))}
CONF_MUTATIONS = ("conf_is_sigmoid", "conf_without_eps")


# ---------------------------------------------------------------- launch forms (the guards mirror flow.hip's launchers)
FORMS = {"one": (9, 13), "quad": (12, 20), "tiled": (16, 64)}
WARP_CCH = {1: 16, 4: 8}          # warp_cch(px)


def max_ctx():
    """CCVS_MAX_CTX of include/ccvs_hip.h."""
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ccvs_hip.h")
    with open(path) as fh:
        return int(re.search(r"#define\s+CCVS_MAX_CTX\s+(\d+)", fh.read()).group(1))


def warp_tiled(H, W, env=None):
    """`warp_tiled` of flow.hip: threads along a tile row, 0 for the plain order."""
    import os
    t = int((os.environ if env is None else env).get("CCVS_WARP_TILED", "16"))
    if t not in (8, 16, 32, 64):
        return 0
    return t if (W % (4 * t) == 0 and H % (256 // t) == 0) else 0


def _order(H, W):
    return "tiled" if warp_tiled(H, W) else "plain"


def launched(op, H, W, cout=None):
    """The kernel instantiation that the launcher of `op` picks, as `name<args>[pixel order]`."""
    if op == "backwarp":
        return f"backwarp_kernel<4>[{_order(H, W)}]" if W % 4 == 0 else "backwarp_kernel<1>"
    if op == "backwarp_p8":
        assert W % 4 == 0
        return "backwarp_p8_kernel"
    if op == "fuse_blend":
        return f"warp_fuse_blend4_kernel[{_order(H, W)}]" if W % 4 == 0 else "warp_fuse_blend_kernel"
    if op == "warp_proj":
        pad = [p for p in (16, 24, 48, 96) if p >= cout][0]
        if W % 4 == 0 and pad <= 24:
            return f"warp_proj4_kernel<{pad}>[{_order(H, W)}]"
        return f"warp_proj_kernel<{pad}>"
    raise ValueError(op)


ALL_INSTANTIATIONS = frozenset(
    ["backwarp_kernel<1>", "backwarp_kernel<4>[plain]", "backwarp_kernel<4>[tiled]", "backwarp_p8_kernel",
     "warp_proj_kernel<16>", "warp_proj_kernel<24>", "warp_proj_kernel<48>", "warp_proj_kernel<96>",
     "warp_proj4_kernel<16>[plain]", "warp_proj4_kernel<16>[tiled]", "warp_proj4_kernel<24>[plain]", "warp_proj4_kernel<24>[tiled]",
     "warp_fuse_blend_kernel", "warp_fuse_blend4_kernel[plain]", "warp_fuse_blend4_kernel[tiled]"])


# ---------------------------------------------------------------- the case table
Case = namedtuple("Case", "op form regime var")      # var: k (fuse_blend), Cout (warp_proj), C (backwarp, backwarp_p8)

NF = 2                      # frames; the batch is NF * k (frame, context) pairs
C_WARP = 10                 # a ragged channel chunk for both warp_cch values
C_PROJ_IN = 40
REGIMES = ("noise", "lattice", "lattice_half", "far", "large")
MULT = {"noise": 0.5, "lattice": 1.0, "lattice_half": 0.5, "far": 1.0, "large": 2.0, "saturated": 0.5}
ZERO_REGIMES = ("lattice", "lattice_half", "far")
SAT_VALUES = (-100.0, -30.0, -12.0, 12.0, 30.0, 100.0)


def lattice_points(n):
    """Sample positions along an axis of n pixels: the edges of the zero-padding window, and one point beyond each (an exact 0)."""
    return [-2.5, -1.0, -1.0 + 2.0 ** -10, -0.5, 0.0, 2.0, 2.25, n - 1.0, n - 0.5, n - 2.0 ** -10, float(n), n + 1.5]


def k_values():
    return (1, 2, max_ctx())


def cases():
    out = []
    for form in FORMS:
        for regime in REGIMES:
            out.append(Case("backwarp", form, regime, C_WARP))
            for cout in ((10, 24, 48, 96) if form != "tiled" else (10, 24)):
                out.append(Case("warp_proj", form, regime, cout))
            if form != "one":
                for c in (8, 24):
                    out.append(Case("backwarp_p8", form, regime, c))
        for regime in REGIMES + ("saturated",):
            for k in k_values():
                out.append(Case("fuse_blend", form, regime, k))
    return out


def _gen(case):
    return torch.Generator().manual_seed(zlib.crc32(repr(tuple(case)).encode()))


def _flows(regime, n, H, W, mult, g):
    if regime in ("noise", "saturated"):
        return torch.randn(n, 2, H, W, generator=g) * 4
    if regime in ("lattice", "lattice_half"):
        px, py = lattice_points(W), lattice_points(H)
        pix = torch.arange(H * W).view(1, H * W) + 41 * torch.arange(n).view(n, 1)
        pair = pix % (len(px) * len(py))
        tx = torch.tensor(px, dtype=torch.float64)[pair % len(px)].view(n, H, W)
        ty = torch.tensor(py, dtype=torch.float64)[pair // len(px)].view(n, H, W)
        xs = torch.arange(W, dtype=torch.float64).view(1, 1, W)
        ys = torch.arange(H, dtype=torch.float64).view(1, H, 1)
        fx = (tx - xs) * ((W - 1.0) / W) / mult
        fy = (ty - ys) * ((H - 1.0) / H) / mult
        return torch.stack([fx, fy], dim=1).float()          # the nearest fp32 flow: the position is the lattice point to 2^-24 |f|
    if regime == "far":
        vals = [W + 5.0, -(W + 5.0), 300.0, -300.0, 1e4, -1e4, 1e9, -1e9]
        f = torch.randn(n, 2, H, W, generator=g) * 1.5
        for i in range(n):
            for r in range(0, H, 3):
                v, which = vals[(r // 3 + 3 * i) % 8], (r // 3 + i) % 3
                if which != 1:
                    f[i, 0, r, :] = v
                if which != 0:
                    f[i, 1, r, :] = v
            f[i, :, H - 2:, :4] = vals[(i + 4) % 8]
        return f
    if regime == "large":
        xs = torch.arange(W, dtype=torch.float64).view(1, 1, W)
        ys = torch.arange(H, dtype=torch.float64).view(1, H, 1)
        amp = 0.7 + 0.3 * torch.rand(n, 2, 1, 1, generator=g).double()
        fx = 0.4 * W * torch.cos(math.pi * xs / (W - 1)) * amp[:, 0] * (0.8 + 0.2 * torch.cos(math.pi * ys / (H - 1)))
        fy = 0.4 * H * torch.cos(math.pi * ys / (H - 1)) * amp[:, 1] * (0.8 + 0.2 * torch.cos(math.pi * xs / (W - 1)))
        return (torch.stack([fx, fy], dim=1) / mult).float()
    raise ValueError(regime)


def _saturated_occ(n, k, H, W, g):
    """[n*k,1,H,W]: pixel class = index % 6: every context +100; +30; one context -30 among +30s; the six values and randn mixed;
    every context -100; +12 and -12 alternating."""
    occ = torch.randn(n, k, H * W, generator=g)
    pix = torch.arange(H * W)
    ctx = torch.arange(k).view(k, 1)
    cls = pix % 6
    vals = torch.tensor(SAT_VALUES)
    occ[:, :, cls == 0] = 100.0
    occ[:, :, cls == 1] = 30.0
    one = torch.where(ctx == (pix // 6) % k, torch.tensor(-30.0), torch.tensor(30.0))          # [k, HW]
    occ[:, :, cls == 2] = one[:, cls == 2]
    mixed = vals[(pix.view(1, -1) + ctx) % 6]
    sel = (cls == 3).view(1, -1) & (ctx % 2 == 0)
    occ = torch.where(sel.unsqueeze(0), mixed.unsqueeze(0).expand(n, k, H * W), occ)
    occ[:, :, cls == 4] = -100.0
    alt = torch.where((ctx + pix.view(1, -1)) % 2 == 0, torch.tensor(12.0), torch.tensor(-12.0))
    occ[:, :, cls == 5] = alt[:, cls == 5]
    return occ.reshape(n * k, 1, H, W).contiguous()


def make_inputs(case):
    """fp32 tensors of a case (CPU): ctxs (k tensors [NF,C,H,W]), flow [NF*k,2,H,W], mult, and per op occ / dec / weight / bias."""
    g = _gen(case)
    H, W = FORMS[case.form]
    mult = MULT[case.regime]
    k = case.var if case.op == "fuse_blend" else 2
    c = C_PROJ_IN if case.op == "warp_proj" else (C_WARP if case.op == "fuse_blend" else case.var)
    shift, scale = (2.0, 1.0) if case.regime in ZERO_REGIMES else ((0.0, 50.0) if case.regime == "large" else (0.0, 1.0))
    inp = dict(k=k, mult=mult, H=H, W=W)
    inp["ctxs"] = [(torch.randn(NF, c, H, W, generator=g) + shift) * scale for _ in range(k)]
    inp["flow"] = _flows(case.regime, NF * k, H, W, mult, g)
    if case.op in ("fuse_blend", "backwarp_p8"):
        inp["occ"] = _saturated_occ(NF, k, H, W, g) if case.regime == "saturated" else torch.randn(NF * k, 1, H, W, generator=g)
    if case.op == "fuse_blend":
        inp["dec"] = torch.randn(NF, c, H, W, generator=g) * scale
    if case.op == "warp_proj":
        inp["weight"] = torch.randn(case.var, c, 1, 1, generator=g)
        inp["bias"] = torch.randn(case.var, generator=g)
    return inp


@functools.lru_cache(maxsize=None)
def reference(case):
    """dict(inp, want, tol, far) of a case, computed once and shared; nothing in it may be modified.  For backwarp_p8 the
    reference is that of the back-warp of the same inputs."""
    inp = make_inputs(case)
    x = stack(inp["ctxs"])
    op = "backwarp" if case.op == "backwarp_p8" else case.op
    want = mirror(op, inp)
    far = far_mask(inp["flow"], inp["mult"], inp["H"], inp["W"])
    if op == "backwarp":
        tol = bound_backwarp(x, inp["flow"], inp["mult"])[0]
    elif op == "warp_proj":
        tol = bound_warp_proj(x, inp["flow"], inp["mult"], inp["weight"], inp["bias"])[0]
    else:
        tol = bound_fuse_blend(inp["dec"], x, inp["flow"], inp["occ"], inp["mult"], inp["k"])
    return dict(inp=inp, want=want, tol=tol, far=far)


def worst_ratio(got, want, tol):
    """Largest |got - want| / tol; an error where tol == 0 counts as inf, a non-finite `got` as inf."""
    err = (got.double() - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    ratio = torch.where(torch.isfinite(got.double()), ratio, torch.full_like(ratio, float("inf")))
    return float(ratio.max())

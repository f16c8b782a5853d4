"""-m gpu: the flow-decoder variants of Matching on the MI355X.  The deformable convolution kernel against the CPU restatement in
fp64 (ctx-list views, k = 1 / 2 / 3 / 5, 16 ... 256 channels, padded output channels, sample points on the window edges, both
precisions, fused epilogue), the grouped x2 transposed convolution
and the masked-flow / trade-off epilogue against torch on CPU, every variant's full-frame decoder against the reference's run
(tests/golden/tiny_variants.npz), the step decoder against the full-frame decoder, and generate_vid's streamed schedule against
the serial one on a variant model."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import deform_ref  # noqa: E402
import ref_harness as rh  # noqa: E402

pytestmark = pytest.mark.gpu

META = json.load(open(os.path.join(HERE, "golden", "tiny_variants.json")))
PIX_TOL = 1e-3


def maxdiff(a, b):
    return (a.detach().double().cpu() - b.detach().double().cpu()).abs().max().item()


def _cpu_deform(ctxs, flow, mult, w, b, occ=None, toff=None, act=False):
    """Matching's deform step on CPU in fp64: offsets built as the reference builds them (flow.unsqueeze(1).repeat_interleave(9, 1))."""
    x = torch.stack([c.double().cpu() for c in ctxs], dim=1).flatten(0, 1)
    fl = flow.double().cpu() * mult
    n, _, h, wd = fl.shape
    off = fl.unsqueeze(1).repeat_interleave(9, dim=1).view(n, 18, h, wd)
    y = deform_ref.deform_conv2d(x, off, w.double().cpu(), b.double().cpu(), padding=1)
    if occ is not None:
        y = y * (1 - torch.sigmoid(occ.double().cpu()))
    if toff is not None:
        y = y + toff.double().cpu()
    return F.leaky_relu(y, 0.1) if act else y


# The added cases: C = 128 / 256 (CoutPad / 32 = 4: deform_conv3x3_kernel<4, ...>, two weight units per thread -- in split-bf16 the
# only MB = 4 form), C = 16 / 48 / 80 (CoutPad above C in split-bf16: 32 / 64 / 96), H*W = 63 (< one 256-pixel tile), 256 (exactly
# one) and 768 (three), k = 5 contexts whose views have different batch strides.  Matching's deform runs at feat_size =
# necf * necf_mult[i] (skip_autoencoder.py: Matching.deform), so every one of these channel counts is reachable from the options.
@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("k,c,hw", [(1, 32, (17, 23)), (3, 96, (16, 16)), (3, 192, (9, 40)), (1, 64, (33, 8)),
                                    (1, 128, (16, 16)), (2, 256, (7, 9)), (1, 16, (7, 9)), (3, 48, (32, 24)), (2, 80, (16, 16)),
                                    (5, 32, (7, 9)), (5, 16, (32, 24))])
def test_deform_conv3x3_op(prec, k, c, hw):
    from ccvs_amd import ops
    g = torch.Generator().manual_seed(c + k)
    nf, (h, w) = 2, hw
    extra = [8] * k if k <= 3 else [8 * (j + 1) for j in range(k)]   # k = 5: a different batch stride per context
    bases = [torch.randn(nf, c + extra[j], h, w, generator=g) for j in range(k)]
    ctxs = [t.cuda()[:, 3:3 + c] for t in bases]                      # channel-slice views: batch stride (c + extra) h w
    fo = torch.zeros(nf * k, 5, h, w)
    fo[:, 0] = torch.randn(nf * k, h, w, generator=g) * 2.5 + 1.0    # flow x and y clearly different, some samples outside
    fo[:, 1] = torch.randn(nf * k, h, w, generator=g) * 1.5 - 2.0
    fo[:, 2] = torch.randn(nf * k, h, w, generator=g)
    fo = fo.cuda()
    wt = torch.randn(c, c, 3, 3, generator=g) / (3 * c ** 0.5)
    bias = torch.randn(c, generator=g) * 0.1
    toff = torch.randn(nf * k, c, h, w, generator=g) * 0.3
    wp = ops.pack_deform_weight(wt.cuda(), precision=prec)
    tol = 2e-4 if prec == "bf16x3" else 2e-5
    for mult, occ, tf, act in ((2.0, None, None, False), (0.75, fo[:, 2:3], toff.cuda(), True)):
        got = ops.deform_conv3x3(ctxs, fo[:, :2], mult, wp, bias.cuda(), occ=occ, toff=tf, act=act)
        want = _cpu_deform(ctxs, fo[:, :2], mult, wt, bias, occ=occ, toff=tf, act=act)
        assert maxdiff(got, want) < tol * max(1.0, want.abs().max().item()), (maxdiff(got, want), prec)
    # the offset axes are torchvision's (row, column) = (flow x, flow y): the swapped reading is far off
    swapped = _cpu_deform(ctxs, fo[:, [1, 0]], 2.0, wt, bias)
    got = ops.deform_conv3x3(ctxs, fo[:, :2], 2.0, wp, bias.cuda())
    assert maxdiff(got, swapped) > 100 * tol


def _deform_into(ctxs, flow, mult, wp, bias, pad):
    """ccvs_deform_conv3x3_ctx through the C ABI into channels [0, C) of a NaN-filled [N, C + pad, H, W] buffer (ops.deform_conv3x3
    allocates its own output, so a stray write to a padded channel would land in the next image or past the tensor)."""
    import ctypes
    from ccvs_amd import lib, ops
    cl, keep = ops._ctx_list(ctxs)
    nf, c, h, w = keep[0].shape
    n = nf * cl.k
    big = torch.full((n, c + pad, h, w), float("nan"), device="cuda")
    out = big[:, :c]
    prec = {"f32": 0, "bf16x3": 1}[wp.kind]
    lib.check(lib.load().ccvs_deform_conv3x3_ctx(ctypes.byref(cl), h * w, ops._p(flow), flow.stride(0), float(mult), ops._p(wp.data),
                                                 wp.cout_pad, prec, ops._p(bias), ops._p(None), 0, ops._p(None), 0, 0, ops._p(out),
                                                 out.stride(0), out.stride(1), n, c, h, w, ops.ACT_NONE, ops._stream()), "deform")
    return big


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("c", [16, 48, 80, 128])
def test_deform_conv3x3_padded_channels_stay_untouched(prec, c):
    """Output channels C .. CoutPad - 1 of the packed weights (zero columns; split-bf16 pads C to a multiple of 32, f32 to 32 or
    a multiple of 64) are never written (the epilogue's `co < C`), channels [0, C) equal ops.deform_conv3x3 bit for bit and the
    float64 reference within the op test's tolerance."""
    from ccvs_amd import ops
    g = torch.Generator().manual_seed(3 * c)
    nf, k, h, w = 2, 2, 7, 9
    ctxs = [torch.randn(nf, c, h, w, generator=g).cuda() for _ in range(k)]
    flow = (torch.randn(nf * k, 2, h, w, generator=g) * 2).cuda()
    wt = torch.randn(c, c, 3, 3, generator=g) / (3 * c ** 0.5)
    bias = torch.randn(c, generator=g) * 0.1
    wp = ops.pack_deform_weight(wt.cuda(), precision=prec)
    assert wp.cout_pad > c or c == 128
    big = _deform_into(ctxs, flow, 1.5, wp, bias.cuda(), wp.cout_pad - c + 16)
    assert torch.isnan(big[:, c:]).all(), "a padded output channel was written"
    got = ops.deform_conv3x3(ctxs, flow, 1.5, wp, bias.cuda())
    assert torch.equal(big[:, :c], got)
    want = _cpu_deform(ctxs, flow, 1.5, wt, bias)
    tol = 2e-4 if prec == "bf16x3" else 2e-5
    assert maxdiff(got, want) < tol * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
def test_deform_conv3x3_border_samples(prec):
    """Sample points exactly on the edges of torchvision's validity window.  Reading (torchvision deform_conv2d's
    bilinear_interpolate, restated in tests/golden/deform_ref.py:bilinear_zero): a point with h <= -1 or h >= H (w likewise) is 0;
    otherwise each of the 4 corners outside [0, H-1] x [0, W-1] adds 0.  Positions (rows and columns independently): -1, -1 + 2^-10,
    -0.5, 0, 2 (integer, lh == 0), 2.25, H - 1, H - 1 + 0.5, H - 2^-10, H -- every pixel gets one (row, column) pair, with the
    flow multiplier 1 so that the point is exact.  Only one tap has non-zero weights and the bias is 0, so wherever the reference
    is 0 the kernel's output must be exactly 0: no weight on a clamped corner."""
    from ccvs_amd import ops
    c, nf, h, w = 32, 1, 12, 20
    g = torch.Generator().manual_seed(77)
    ctx = torch.randn(nf, c, h, w, generator=g) + 2.0                  # no accidental zeros
    pos = lambda n: [-1.0, -1.0 + 2 ** -10, -0.5, 0.0, 2.0, 2.25, n - 1.0, n - 0.5, n - 2 ** -10, float(n)]
    ph, pw = pos(h), pos(w)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    pix = torch.arange(h * w).view(h, w)
    for ti, tj in ((1, 1), (0, 2), (2, 0)):
        th = torch.tensor(ph)[pix % len(ph)] - (ti - 1)                 # this tap then samples at ph[...] exactly
        tw = torch.tensor(pw)[(pix // len(ph)) % len(pw)] - (tj - 1)
        flow = torch.stack([th - ys, tw - xs]).unsqueeze(0)            # [1, 2, H, W]: (row, column) offsets
        assert torch.equal(ys + (ti - 1) + flow[0, 0], th + (ti - 1))
        wt = torch.zeros(c, c, 3, 3)
        wt[:, :, ti, tj] = torch.randn(c, c, generator=g) / c ** 0.5
        bias = torch.zeros(c)
        wp = ops.pack_deform_weight(wt.cuda(), precision=prec)
        got = ops.deform_conv3x3([ctx.cuda()], flow.cuda(), 1.0, wp, bias.cuda()).double().cpu()
        want = _cpu_deform([ctx], flow, 1.0, wt, bias)
        zero = (want == 0).all(dim=1, keepdim=True).expand_as(want)
        assert 0.2 < zero.float().mean().item() < 0.8                    # both kinds of points present
        assert (got[zero] == 0).all(), f"tap {(ti, tj)}: {int((got[zero] != 0).sum())} outputs leak from outside the window"
        tol = 2e-4 if prec == "bf16x3" else 2e-5
        assert maxdiff(got, want) < tol * max(1.0, want.abs().max().item()), (ti, tj, maxdiff(got, want))


@pytest.mark.parametrize("mult,hw", [(1, (8, 8)), (2, (16, 12)), (3, (5, 7))])
def test_gconvT4x4s2_op(mult, hw):
    from ccvs_amd import ops
    g = torch.Generator().manual_seed(mult)
    x = torch.randn(3, 32, *hw, generator=g)
    w = torch.randn(32, mult, 4, 4, generator=g)
    want = F.conv_transpose2d(x.double(), w.double(), stride=2, padding=1, groups=32)
    got = ops.gconvT4x4s2(x.cuda(), w.cuda())
    assert got.shape == want.shape and maxdiff(got, want) < 1e-5


def test_flow_mask_toff_op():
    from ccvs_amd import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 24, 9, 11, generator=g)
    occ, toff = torch.randn(4, 1, 9, 11, generator=g), torch.randn(4, 24, 9, 11, generator=g)
    for o, t, act in ((occ, None, False), (None, toff, True), (occ, toff, True)):
        want = x.double()
        if o is not None:
            want = want * (1 - torch.sigmoid(o.double()))
        if t is not None:
            want = want + t.double()
        want = F.leaky_relu(want, 0.1) if act else want
        got = ops.flow_mask_toff_(x.cuda(), o.cuda() if o is not None else None, t.cuda() if t is not None else None, act=act)
        assert maxdiff(got, want) < 1e-5


def _variant_decoder(name):
    from ccvs_amd.tools.options import Options
    from ccvs_amd.models.skip_vid_generator.models.skip_autoencoder import SkipGANDecoder
    opt = Options().parse(load_qvid_generator=True, load_transformer=True, argv=META["argv"] + META["configs"][name]["flags"])
    dec = SkipGANDecoder(opt["qvid_generator"])
    sd = rh.seeded_weights(META["configs"][name]["weight_spec"], META["weight_seed"])
    sd.update({k: v for k, v in dec.state_dict().items() if k.endswith(".kernel")})
    dec.load_state_dict(sd, strict=True)
    return dec.cuda().eval(), opt


def _inputs():
    spec = META["variant_inputs"]
    g = torch.Generator().manual_seed(spec["z"][1])
    z = torch.randn(spec["z"][0], generator=g)
    ctx = []
    for j in range(spec["k"]):
        g = torch.Generator().manual_seed(spec["ctx"][1] + j)
        ctx.append([torch.randn(s, generator=g).cuda() for s in spec["ctx"][0]])
    return z.cuda(), ctx


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("name", sorted(META["configs"]))
def test_variant_decoder_golden(name, prec, golden_dir, monkeypatch):
    from ccvs_amd import ops
    monkeypatch.setattr(ops, "CONV_PRECISION", prec)
    gold = np.load(os.path.join(golden_dir, "tiny_variants.npz"))
    dec, _ = _variant_decoder(name)
    z, ctx = _inputs()
    rgb, _, flows, occs, _ = dec(z, ctx, return_all=True)
    assert maxdiff(rgb, torch.from_numpy(gold[f"{name}/rgb"])) < PIX_TOL
    for i in range(len(flows)):
        assert maxdiff(flows[i], torch.from_numpy(gold[f"{name}/flow{i}"])) < PIX_TOL, (name, i)
        assert maxdiff(occs[i], torch.from_numpy(gold[f"{name}/occ{i}"])) < PIX_TOL, (name, i)


def test_variant_interblock_forward_threads_toff():
    """InterBlock.forward (the reference's per-level signature) returns the Subpixel feature and takes it back at the next level."""
    dec, _ = _variant_decoder("all")
    z, ctx = _inputs()
    want = dec(z, ctx)[0]
    x = dec.blocks[0](z.flatten(0, 1))
    flows = occs = toffs = None
    for i, blk in enumerate(dec.inter_blocks):
        if i > 0:
            x = dec.blocks[i](x)
        s = dec.inter_sizes[i]
        out, flows, occs, toffs = blk(x[:, :s], [c[-1 - i].flatten(0, 1) for c in ctx], flows, occs, toffs)
        assert toffs is not None and toffs.shape[1] == 32
        x = torch.cat([out, x[:, s:]], dim=1)
    assert maxdiff(dec.blocks[-1](x).view_as(want), want) < 1e-5


@pytest.fixture(scope="module")
def variant_gen():
    from ccvs_amd.tools.options import Options
    from ccvs_amd.helpers.generator import Generator
    torch.manual_seed(0)
    opt = Options().parse(load_qvid_generator=True, load_transformer=True, argv=META["argv"] + META["configs"]["all"]["flags"])
    gen = Generator(opt).build_models()
    with torch.no_grad():
        z_e, _ = gen.vid_model.net_e(gen.synthetic_batch(2)["vid"].cuda())
        cb = gen.vid_model.net_q.embedding.weight
        cb.copy_(torch.randn(cb.shape, generator=torch.Generator().manual_seed(4)).cuda() * z_e.std())
        gen.transformer_model.net_t.s_emb.normal_(0, 0.02)
        gen.transformer_model.net_t.t_emb.normal_(0, 0.02)
        for blk in gen.vid_model.net_g.inter_blocks:     # clearly non-zero flows at every level
            blk.matching.flow_head.conv.bias.normal_(0, 1.0)
    return gen, opt


def test_variant_step_decoder_equals_full_frame(variant_gen):
    gen, _ = variant_gen
    qv = gen.vid_model
    enc = qv({"vid": gen.synthetic_batch(2, seed=9)["vid"]}, mode="vid_encoder")
    inter = [f[:, :1].contiguous() for f in enc["inter"]]
    code = enc["code"][:, 64:128].contiguous()
    step = qv({"code": code, "inter": inter}, mode="vid_step_decoder")
    full = qv.net_g(qv._embed(code, 1), [[f[:, [-1]] for f in inter]])[0]
    assert maxdiff(step["vid"], full) < 1e-6


def test_variant_generate_vid_stream_equals_serial(variant_gen):
    gen, opt = variant_gen
    xopt = opt["transformer"]
    xopt.sample, xopt.top_k = False, 10
    data = gen.synthetic_batch(2, seed=31)["vid"]
    want = gen.generate_vid({"vid": data.clone()}, schedule="serial")
    got = gen.generate_vid({"vid": data.clone()}, schedule="stream")
    torch.cuda.synchronize()
    assert torch.equal(got["fake"]["code"], want["fake"]["code"])
    assert maxdiff(got["fake"]["vid"], want["fake"]["vid"]) < PIX_TOL
    assert torch.isfinite(got["fake"]["vid"]).all()

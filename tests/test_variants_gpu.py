"""-m gpu: the flow-decoder variants of Matching on the MI355X.  The deformable convolution kernel against the CPU restatement in
fp64 (ctx-list views, k = 1 / 3, 32 / 96 / 192 channels, both precisions, fused epilogue), the grouped x2 transposed convolution
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


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("k,c,hw", [(1, 32, (17, 23)), (3, 96, (16, 16)), (3, 192, (9, 40)), (1, 64, (33, 8))])
def test_deform_conv3x3_op(prec, k, c, hw):
    from ccvs_amd import ops
    g = torch.Generator().manual_seed(c + k)
    nf, (h, w) = 2, hw
    bases = [torch.randn(nf, c + 8, h, w, generator=g) for _ in range(k)]
    ctxs = [t.cuda()[:, 3:3 + c] for t in bases]                      # channel-slice views: batch stride (c + 8) h w
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

"""-m gpu: the decoder's motion export against its mirror (tests/flow_ref.py).
  1. the three ops through the C ABI, at ragged sizes (1x1, 3x5, 16x16, 17x33 against 16-byte lanes), B in {1, 3}, T in {1, 4}, k in
     {1, 2, 3}: inputs are views inside NaN-filled tensors, outputs slots of NaN-filled tensors whose other slots must stay NaN;
  2. the model and the generator on the tiny flow-guided configuration of tests/test_e2e_gpu.py (three skip contexts; point to point):
     the clips do not move, flow / occ are what `net_g(..., return_all=True)` returned, warp is the back-warp of the clip's own frame;
  3. the files `run()` writes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_ref as FR  # noqa: E402
from oracle import ccvs_oracle as O  # noqa: E402
from test_e2e_gpu import TINY_ARGV, _load, _sd  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 5), (16, 16), (17, 33)]
BTS = [(1, 1), (1, 4), (3, 1), (3, 4)]


def lut():
    from ccvs_amd.tools.flowviz import HSV128
    return torch.from_numpy(HSV128.copy())


def nan_view(t, dim, before, after):
    """`t` on the GPU as a slice along `dim` of a larger NaN-filled tensor"""
    shape = list(t.shape)
    shape[dim] += before + after
    big = torch.full(shape, float("nan"), device="cuda")
    view = big.narrow(dim, before, t.shape[dim])
    view.copy_(t)
    return view


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("h,w", SIZES)
def test_flow_export_slot(h, w):
    """Flow bit-equal to fo * flow_mult; the mask within 4 x the error torch's fp32 makes with the same formula on these inputs
    (floor 1e-6: the kernel has its own expf and summation order, not another algorithm), against the float64 mirror."""
    from ccvs_amd import ops
    s, mult = 5, 4.0
    for b, t in BTS:
        for k in (1, 2, 3):
            g = torch.Generator().manual_seed(h * 1000 + w * 10 + b * 3 + t + k)
            fo = torch.randn(b * k, 3, h, w, generator=g) * torch.tensor([3.0, 3.0, 4.0]).view(1, 3, 1, 1)
            fo[0, 2, 0, 0], fo[-1, 2, -1, -1] = 40.0, -40.0              # saturated logits
            dev = nan_view(fo, 1, s, 0)                                   # channels s .. s + 2 of [N * k, s + 3, H, W], the rest NaN
            assert dev.stride(0) == (s + 3) * h * w and dev.data_ptr() % 16 == (4 * s * h * w) % 16
            out = torch.full((b, t, 3, h, w), float("nan"), device="cuda")
            slot = t - 1 if t > 1 else 0
            ops.flow_export(dev, k, mult, out, slot)
            got = out.cpu()
            for other in range(t):
                if other != slot:
                    assert got[:, other].isnan().all(), (b, t, k, other)
            assert torch.equal(got[:, slot, :2], fo[0::k, :2] * mult), (b, t, k)
            want = FR.export(fo, k, mult)[:, 2]
            err32 = (FR.export(fo, k, mult, dtype=torch.float32)[:, 2].double() - want).abs().max().item()
            err = (got[:, slot, 2].double() - want).abs().max().item()
            print(f"flow_export mask {h}x{w} B={b} T={t} k={k}: kernel {err:.3e}, torch fp32 {err32:.3e}")
            assert err <= max(4 * err32, 1e-6), (b, t, k, err, err32)


@pytest.mark.parametrize("h,w", SIZES)
def test_flow_max_bits(h, w):
    """The fp32 mirror's bits, NaN and inf planted; the same bits twice, through a strided view, and under a CU budget."""
    from ccvs_amd import ops
    for b, t in BTS:
        g = torch.Generator().manual_seed(h * 100 + w + b + t)
        m = torch.randn(b, t, 3, h, w, generator=g) * 7
        m[0, 0, 0, 0, 0] = float("nan")
        m[-1, -1, 1, -1, -1] = float("inf")
        if h * w > 1:
            m[0, 0, 0, -1, -1], m[0, 0, 1, -1, -1] = 2e19, 2e19           # finite components, an infinite fp32 magnitude
        want = FR.clip_max(m)
        dev = nan_view(m, 1, 1, 2)
        got = ops.flow_max(dev)
        assert got.shape == (b,) and got.dtype == torch.float32
        assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)), (b, t, got.cpu(), want)
        assert torch.equal(ops.flow_max(dev), got) and torch.equal(ops.flow_max(m.cuda()), got)
        st = torch.cuda.current_stream()
        ops.stream_cu_limit(st, 2)
        try:
            assert torch.equal(ops.flow_max(dev), got)
        finally:
            ops.stream_cu_limit(st, 0)
    still = torch.zeros(2, 2, 3, h, w)
    still[1, :, :2] = float("nan")
    assert ops.flow_max(still.cuda()).tolist() == [0.0, 0.0]


def test_flow_max_several_workgroups_per_clip():
    """More than the 8192 pixels one workgroup takes per clip, the largest flow in the last one's ragged tail; a frame-strided view."""
    from ccvs_amd import ops
    m = torch.randn(2, 9, 3, 33, 31, generator=torch.Generator().manual_seed(8))         # 9207 pixels per clip: two workgroups
    m[1, 8, :2, 32, 30] = torch.tensor([-30.0, 40.0])
    m[0, 4, 0, 3, 3] = float("nan")
    got = ops.flow_max(nan_view(m, 1, 0, 1))
    assert torch.equal(got.cpu().view(torch.int32), FR.clip_max(m).view(torch.int32)) and got[1].item() == 50.0
    assert torch.equal(ops.flow_max(m.cuda()), got)


def _check_render(motion, max_px, got_flow, got_occ, max_share=0.02):
    """Every byte equals the fp32 mirror's outside `edge_sensitive`; inside it the bin may be a neighbour and each byte may differ by
    1; at most `max_share` of the pixels are inside."""
    table = lut()
    want_flow, want_occ, idx = FR.render(motion, max_px, table)
    edge = FR.edge_sensitive(motion, max_px, table)
    share = edge.float().mean().item()
    assert share <= max_share, share
    got_flow, got_occ = got_flow.cpu(), got_occ.cpu()
    assert got_flow.shape == want_flow.shape and got_flow.dtype == torch.uint8 and got_occ.shape == want_occ.shape
    assert torch.equal(got_flow[~edge], want_flow[~edge]) and torch.equal(got_occ[~edge], want_occ[~edge])
    if edge.any():
        assert (got_occ[edge].int() - want_occ[edge].int()).abs().max() <= 1
        r = FR.colours(motion, max_px, torch.ones(128, 3))[0][..., :1]       # (a table of ones: the radius itself)
        near = torch.zeros(int(edge.sum()), dtype=torch.bool)
        for d in (-1, 0, 1):
            cand = ((r * table[(idx + d).clamp(0, 127)]).clamp(0, 1) * 255).to(torch.uint8)
            near |= ((got_flow[edge].int() - cand[edge].int()).abs().amax(dim=-1) <= 1)
        assert near.all()
    return share


@pytest.mark.parametrize("h,w", SIZES)
def test_flow_render_bytes(h, w):
    from ccvs_amd import ops
    for b, t in BTS:
        motion = FR.make_motion(b, t, h, w, seed=h * 64 + w + 5 * b + t, lut=lut(), max_px=8.0)
        max_px = torch.full((b,), 8.0)
        flow_u8, occ_u8 = ops.flow_render(nan_view(motion, 1, 2, 1), max_px.cuda())
        assert flow_u8.is_contiguous() and occ_u8.is_contiguous()
        assert _check_render(motion, max_px, flow_u8, occ_u8) == 0.0      # (a clean draw: every byte is the mirror's)


def test_flow_render_edges_and_special_values():
    """Raw random flows (their edge pixels included), a fixed against each clip's own radius, max_px = 0, non-finite pixels, r = 1."""
    from ccvs_amd import ops
    table = lut()
    motion = FR.make_motion(3, 4, 17, 33, seed=3, lut=table, max_px=8.0, clean=False)
    motion[0, 1, 0, 2, 3] = float("nan")
    motion[0, 2, 1, 4, 5] = float("-inf")
    motion[1, 0, 2, 0, 0] = float("nan")
    motion[1, 0, 2, 0, 1], motion[1, 0, 2, 0, 2] = -3.0, 7.0
    motion[2, 3, :2, 16, 32] = torch.tensor([600.0, -800.0])             # clip 2's largest: |f| = 1000 exactly
    dev = motion.cuda()
    fixed = torch.full((3,), 8.0)
    share = _check_render(motion, fixed, *ops.flow_render(dev, fixed.cuda()))
    print(f"flow_render: edge-sensitive share {share:.4%} at a fixed radius")
    own = ops.flow_max(dev)
    assert torch.equal(own.cpu(), FR.clip_max(motion)) and own[2].item() == 1000.0
    flow_own, occ_own = ops.flow_render(dev, own)
    _check_render(motion, own.cpu(), flow_own, occ_own)
    flow_own, occ_own = flow_own.cpu(), occ_own.cpu()
    idx = FR.render(motion, own.cpu(), table)[2]
    assert flow_own[2, 3, 16, 32].tolist() == (table[idx[2, 3, 16, 32]] * 255).to(torch.uint8).tolist()     # r exactly 1: the table's colour
    assert flow_own[0, 1, 2, 3].eq(0).all() and flow_own[0, 2, 4, 5].eq(0).all()                             # a non-finite component: black
    assert occ_own[1, 0, 0, :3].tolist() == [[0] * 3, [0] * 3, [255] * 3]                                    # NaN, below 0, above 1
    zero = torch.tensor([0.0, 8.0, 0.0])
    flow_zero, occ_zero = ops.flow_render(dev, zero.cuda())
    assert flow_zero[0].eq(0).all() and flow_zero[2].eq(0).all() and torch.equal(occ_zero.cpu(), occ_own)
    assert torch.equal(flow_zero[1].cpu(), ops.flow_render(dev, fixed.cuda())[0][1].cpu())


# ------------------------------------------------------------------ 2
@pytest.fixture(scope="module")
def nets(golden_dir):
    from ccvs_amd.tools.options import Options
    from ccvs_amd.models.skip_vid_generator.models.quantized_video_model import QVidModel
    from ccvs_amd.models.skip_vid_generator.models.transformer_model import Transformer
    gold = np.load(os.path.join(golden_dir, "tiny_e2e.npz"))
    opt = Options().parse(load_qvid_generator=True, load_transformer=True, argv=TINY_ARGV)
    opt["transformer"].sample, opt["transformer"].top_k = False, 10
    qv = QVidModel(opt["qvid_generator"], is_train=False, is_main=True).eval()
    tr = Transformer(opt["transformer"], is_train=False, is_main=True).eval()
    for net, key in ((qv.net_e, "e"), (qv.net_q, "q"), (qv.net_g, "g"), (tr.net_t, "t")):
        _load(net, _sd(gold, key))
    yield opt, qv, tr
    opt["transformer"].p2p, opt["transformer"].save_flow = False, False


def make_gen(nets, save_flow, p2p):
    """A Generator on the shared networks and their option objects (the models read them while they run, as in tests/test_e2e_gpu.py);
    --save_flow is read when the Generator is made, --x_p2p while it runs: the generators of one test share one p2p setting."""
    from ccvs_amd.helpers.generator import Generator
    opt, qv, tr = nets
    opt["transformer"].save_flow, opt["transformer"].p2p = save_flow, p2p
    gen = Generator(opt)
    gen.vid_model, gen.transformer_model = qv, tr
    return gen


MOTION_KEYS = ("flow", "occ", "warp", "motion")


@pytest.mark.parametrize("p2p", [False, True])
def test_clips_do_not_move_and_schedules_agree(nets, p2p):
    plain, flow = make_gen(nets, False, p2p), make_gen(nets, True, p2p)
    data = plain.synthetic_batch(2, seed=21)
    outs = {}
    for schedule in ("serial", "stream"):
        a = plain.generate_vid({"vid": data["vid"].clone()}, schedule=schedule)
        b = flow.generate_vid({"vid": data["vid"].clone()}, schedule=schedule)
        torch.cuda.synchronize()
        for side in ("fake", "rec"):
            assert torch.equal(a[side]["vid"], b[side]["vid"]), (schedule, side)
            assert not any(k in a[side] for k in MOTION_KEYS + ("flow_dt",))
            d = b[side]
            assert d["flow"].shape == (2, 4, 2, 32, 32) and d["occ"].shape == (2, 4, 1, 32, 32) and d["warp"].shape == d["vid"].shape
            assert d["motion"].dtype == d["warp"].dtype == torch.float32
            assert d["flow_dt"] == ([0, 1, 1, 0] if p2p else [0, 1, 1, 1])
        outs[schedule] = b
    piped = flow.run_pipelined([{"vid": data["vid"].clone()}], rec_pass=True)[0]
    torch.cuda.synchronize()
    for other in (outs["stream"], piped):
        for side in ("fake", "rec"):
            assert torch.equal(other[side]["vid"], outs["serial"][side]["vid"])
            assert other[side]["flow_dt"] == outs["serial"][side]["flow_dt"]
            for k in MOTION_KEYS:
                assert torch.equal(other[side][k], outs["serial"][side][k]), (side, k)


@pytest.mark.parametrize("p2p", [False, True])
def test_flow_occ_are_the_decoders_and_warp_is_the_backwarp(nets, p2p, monkeypatch):
    from ccvs_amd import ops
    qv = nets[1]
    gen = make_gen(nets, True, p2p)
    data = gen.synthetic_batch(2, seed=22)
    seen = []
    forward = qv.net_g.forward

    def recording(*args, **kwargs):
        res = forward(*args, **kwargs)
        if kwargs.get("return_all"):
            seen.append((len(args[1]), [f.clone() for f in res[2]], [o.clone() for o in res[3]]))
        return res

    monkeypatch.setattr(qv.net_g, "forward", recording)
    out = gen.generate_vid({"vid": data["vid"].clone()}, schedule="serial")
    monkeypatch.undo()
    torch.cuda.synchronize()
    new = 2 if p2p else 3                                     # new frames per decode; the fake decode ran first, then the rec decode
    assert len(seen) == 2 * new
    mult = float(qv.net_g.last_flow_mult)
    assert mult == 4.0
    for side, calls in (("fake", seen[:new]), ("rec", seen[new:])):
        d = out[side]
        vid, flow, occ, warp = d["vid"], d["flow"], d["occ"], d["warp"]
        assert d["flow_dt"] == ([0, 1, 1, 0] if p2p else [0, 1, 1, 1])
        for t, dt in enumerate(d["flow_dt"]):
            if dt == 0:
                assert flow[:, t].eq(0).all() and occ[:, t].eq(0).all() and torch.equal(warp[:, t], vid[:, t])
                continue
            k, flows, occs = calls[t - 1]
            assert k == min(t, 3) + (1 if p2p else 0) and flows[-1].shape == (2 * k, 2, 32, 32)
            assert torch.equal(flow[:, t], flows[-1][0::k] * mult)
            fo = torch.cat([flows[-1], occs[-1]], dim=1).cpu()
            want = FR.export(fo, k, mult)[:, 2]
            err32 = (FR.export(fo, k, mult, dtype=torch.float32)[:, 2].double() - want).abs().max().item()
            assert (occ[:, t, 0].cpu().double() - want).abs().max().item() <= max(4 * err32, 1e-6)
            assert torch.equal(warp[:, t], ops.backwarp(vid[:, t - dt].contiguous(), flow[:, t].contiguous(), 1.0))
            ref = O.backwarp(vid[:, t - dt].cpu(), flow[:, t].cpu(), O.backwarp_grid(32, 32))
            assert (warp[:, t].cpu() - ref).abs().max().item() <= 1e-4          # the tolerance of test_backwarp_oracle
        assert flow[:, 1:3].abs().max() > 0 and 0 < occ[:, 1].min() and occ[:, 1].max() < 1


# ------------------------------------------------------------------ 3
def _run(root, extra, capture=None):
    from ccvs_amd.tools.options import Options
    from ccvs_amd.helpers.generator import Generator
    torch.manual_seed(0)
    argv = TINY_ARGV + ["--n_iter", "2", "--x_top_k", "10", "--x_sample", "--save_path", str(root)] + extra
    opt = Options().parse(load_qvid_generator=True, load_transformer=True, argv=argv)
    gen = Generator(opt)
    if capture is not None:
        save = gen.save_results

        def keeping(out, global_iter):
            capture[global_iter] = {side: out[side]["motion"].cpu() for side in ("fake", "rec")}
            return save(out, global_iter)

        gen.save_results = keeping
    torch.manual_seed(9)
    gen.run()
    top = opt["transformer"].result_path
    return top, {kind: sorted(os.listdir(os.path.join(top, kind))) for kind in sorted(os.listdir(top))}


def test_run_writes_the_motion_clips(tmp_path):
    from ccvs_amd import ops
    from ccvs_amd.tools import apng, mjpeg
    kept = {}
    top, tree = _run(tmp_path / "apng", ["--save_flow", "--save_flow_raw", "--video_format", "apng"], capture=kept)
    names = [f"vid_{i:05d}" for i in range(4)]
    clips = ["real", "fake", "rec"] + [f"{side}_{kind}" for side in ("fake", "rec") for kind in ("flow", "occ", "warp")]
    assert tree == {**{kind: [n + ".png" for n in names] for kind in clips}, "fake_motion": [n + ".npy" for n in names], "rec_motion": [n + ".npy" for n in names]}
    assert sorted(kept) == [0, 1]
    for side in ("fake", "rec"):
        for it in (0, 1):
            motion = kept[it][side]
            assert motion.shape == (2, 4, 3, 32, 32) and motion[:, 1:, :2].abs().max() > 0
            flow_u8, occ_u8 = ops.flow_render(motion.cuda(), ops.flow_max(motion.cuda()))
            for i in range(2):
                name = names[2 * it + i]
                assert np.array_equal(np.load(os.path.join(top, side + "_motion", name + ".npy")), motion[i].numpy())
                assert np.array_equal(apng.read_apng(os.path.join(top, side + "_flow", name + ".png")), flow_u8[i].cpu().numpy())
                assert np.array_equal(apng.read_apng(os.path.join(top, side + "_occ", name + ".png")), occ_u8[i].cpu().numpy())
                assert apng.read_apng(os.path.join(top, side + "_warp", name + ".png")).shape == (4, 32, 32, 3)
    top, tree = _run(tmp_path / "avi", ["--save_flow", "--flow_max_px", "3", "--video_format", "avi"])
    assert sorted(tree) == sorted(clips) and all(v == [n + ".avi" for n in names] for v in tree.values())
    for kind in ("fake_flow", "rec_occ", "fake_warp"):
        fps, h, w, frames = mjpeg.read_avi(os.path.join(top, kind, names[3] + ".avi"))
        assert (h, w) == (32, 32) and len(frames) == 4
    top, tree = _run(tmp_path / "plain", ["--video_format", "apng"])
    assert tree == {kind: [n + ".png" for n in names] for kind in ("fake", "real", "rec")}

"""Not gpu: the motion export's host side.
  1. `tools.flowviz.HSV128` is matplotlib's `hsv` colormap resampled to 128 entries, to fp32 (where matplotlib imports);
  2. the mirror's colours (tests/flow_ref.py) against a restatement of the reference's `Logger.get_flow_rgb` (tools/logger.py:95-103)
     with boost = sqrt(2) / max_px: the same bin bit for bit, the colour within 1e-6 -- random flows, the axis cases, saturated radii;
  3. the mirror's special cases: k = 1 and k = 3 masks, `clip_max` without NaN / inf, a clip without flow is black;
  4. the edge-sensitive share of random flows stays under 2 % (the bar tests/test_flowviz_gpu.py asserts per case);
  5. options and glue: the flags parse, the refusals raise by name, the three symbols are declared in their header and named in
     lib.py, the built library exports them, and `save_results` sends the six folders to the writers."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_ref as FR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TINY_ARGV = ["--name", "tiny", "--dataset", "bairhd", "--max_dim", "32", "--vid_len", "4", "--q_z_num", "32", "--q_z_size", "16",
             "--q_z_shape", "8", "8", "--q_use_enc", "--q_use_dec", "--q_necf", "8", "--q_necf_mult", "1", "2", "2",
             "--q_enc_model", "skipgan", "--q_dec_model", "skipgan", "--q_use_inter", "--q_inter_p", "0.75",
             "--q_skip_context", "1", "2", "3", "--q_skip_memory", "3", "--x_z_num", "32", "--x_z_len", "256", "--x_n_layer", "2",
             "--x_n_head", "2", "--x_n_embd", "32", "--x_z_chunk", "64", "--x_cond_len", "64", "--x_emb_mode", "temporal",
             "--x_num_blocks", "4", "--batch_size_vid", "2"]


def lut():
    from ccvs_amd.tools.flowviz import HSV128
    return torch.from_numpy(HSV128.copy())


# ------------------------------------------------------------------ 1
def test_table_is_matplotlibs_hsv_resampled_to_128():
    matplotlib = pytest.importorskip("matplotlib")
    from ccvs_amd.tools.flowviz import HSV128
    want = matplotlib.colormaps["hsv"].resampled(128)(np.arange(128))[:, :3].astype(np.float32)
    assert HSV128.dtype == np.float32 and HSV128.shape == (128, 3) and not HSV128.flags.writeable
    assert np.array_equal(HSV128, want)


def test_product_code_does_not_import_matplotlib():
    for base, _, files in os.walk(os.path.join(ROOT, "ccvs_amd")):
        for f in files:
            if f.endswith(".py"):
                assert not re.search(r"^\s*(from|import)\s+matplotlib", open(os.path.join(base, f)).read(), re.M), f


# ------------------------------------------------------------------ 2
def reference_colours(flow, boost):
    """The reference's flow picture restated: flow [..., 2] (x, y) fp32 -> (rgb [..., 3] fp32, bin [...]), the colormap called on theta."""
    matplotlib = pytest.importorskip("matplotlib")
    radius = (flow ** 2).sum(-1).sqrt() / np.sqrt(2) * boost
    radius[radius > 1] = 1.
    theta = (1 + torch.atan2(flow.select(-1, -1), flow.select(-1, 0)) / np.pi) / 2
    rgba = matplotlib.colormaps["hsv"].resampled(128)(theta.numpy())
    rgb = radius.unsqueeze(-1) * torch.tensor(rgba[..., :3]).float()
    return rgb, np.minimum((theta.numpy() * 128).astype(np.int64), 127), theta


def _as_motion(flow):
    """[N, 2] flows -> a motion buffer [1, 1, 3, 1, N] with mask 0.5"""
    n = flow.shape[0]
    return torch.cat([flow.t().reshape(2, 1, n), torch.full((1, 1, n), 0.5)]).view(1, 1, 3, 1, n)


@pytest.mark.parametrize("max_px", [1.0, 3.5, 20.0])
def test_mirror_colours_are_the_references(max_px):
    g = torch.Generator().manual_seed(int(max_px * 10))
    rnd = torch.randn(4096, 2, generator=g) * torch.exp(torch.empty(4096, 1).uniform_(-3, 3, generator=g))
    axis = torch.tensor([[0.0, 0.0], [-1.0, 0.0], [-1.0, -0.0], [1.0, 0.0], [0.0, 1.0], [0.0, -1.0]])
    saturated = torch.tensor([[max_px, 0.0], [0.0, -max_px], [2 * max_px, 2 * max_px], [-1e6, 3.0], [max_px * 0.6, max_px * 0.8]])
    flow = torch.cat([rnd, axis, saturated])
    want_rgb, want_bin, theta = reference_colours(flow.clone(), float(np.sqrt(2) / max_px))
    assert theta[4096:4102].tolist() == [0.5, 1.0, 0.0, 0.5, 0.75, 0.25]
    rgb, idx = FR.colours(_as_motion(flow), torch.tensor([max_px]), lut())
    assert np.array_equal(idx.view(-1).numpy(), want_bin)
    assert (rgb.view(-1, 3) - want_rgb).abs().max().item() <= 1e-6
    assert idx.view(-1)[4096:4102].tolist() == [64, 127, 0, 64, 96, 32]
    sat = rgb.view(-1, 3)[4102:4106]
    assert torch.equal(sat, lut()[idx.view(-1)[4102:4106]])        # radius exactly 1: the table's own colour


# ------------------------------------------------------------------ 3
def test_export_mirror_masks():
    g = torch.Generator().manual_seed(1)
    fo = torch.randn(6, 3, 5, 7, generator=g) * 3
    one = FR.export(fo, 1, 4.0)
    assert torch.equal(one[:, :2], fo[:, :2].double() * 4) and torch.equal(one[:, 2], torch.sigmoid(fo[:, 2].double()))
    # k = 3: the reference's lines (skip_autoencoder.py:255-263) evaluated in float64
    occs = fo[:, 2:3].double()
    confs = (1 - torch.sigmoid(occs)).view(-1, 3, *occs.shape[1:]) + 1e-6
    occ = (occs.view(-1, 3, *occs.shape[1:]) * confs).sum(dim=1) / confs.sum(dim=1)
    three = FR.export(fo, 3, 4.0)
    assert three.shape == (2, 3, 5, 7)
    assert torch.equal(three[:, 2:3], torch.sigmoid(occ)) and torch.equal(three[:, :2], fo[0::3, :2].double() * 4)
    f32 = FR.export(fo, 3, 4.0, dtype=torch.float32)
    assert f32.dtype == torch.float32 and torch.equal(f32[:, :2], fo[0::3, :2] * 4) and (f32[:, 2].double() - three[:, 2]).abs().max() < 1e-6


def test_clip_max_ignores_non_finite_and_a_still_clip_is_black():
    m = torch.zeros(3, 2, 3, 4, 5)
    m[0, 1, 0, 2, 3], m[0, 1, 1, 2, 3] = 3.0, -4.0
    m[0, 0, 0, 0, 0] = float("nan")
    m[0, 0, 1, 1, 1] = float("inf")
    m[0, 1, 0, 0, 0] = 3e38            # finite components, infinite fp32 magnitude: not a finite pixel
    m[1, 0, 0, 0, 0], m[1, 0, 1, 0, 1] = float("-inf"), float("nan")
    assert FR.clip_max(m).tolist() == [5.0, 0.0, 0.0]
    m[:, :, 2] = 0.5
    flow_u8, occ_u8, _ = FR.render(m, FR.clip_max(m), lut())
    assert flow_u8[1:].eq(0).all() and occ_u8.eq(127).all()
    assert flow_u8[0, 0, 0, 0].eq(0).all() and flow_u8[0, 0, 1, 1].eq(0).all()      # NaN / inf pixels are black
    assert flow_u8[0, 1, 2, 3].tolist() == (lut()[FR.render(m, FR.clip_max(m), lut())[2][0, 1, 2, 3]] * 255).to(torch.uint8).tolist()
    assert not FR.edge_sensitive(m, torch.zeros(3), lut()).any()                    # black pixels and a mask of 0.5: no edges
    zero =FR.render(m, torch.zeros(3), lut())[0]
    assert zero.eq(0).all()                                                         # max_px = 0: black, no division


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("max_px", [1.0, 8.0, 32.0])
def test_edge_sensitive_share_of_random_flows(max_px):
    """Random flows of 0.05 - 20 px: the flagged share -- bin edges, value edges per channel, the mask's -- is under 2 %."""
    motion = FR.make_motion(3, 4, 64, 64, seed=11, lut=lut(), max_px=max_px, clean=False)
    share = FR.edge_sensitive(motion, torch.full((3,), max_px), lut()).float().mean().item()
    print(f"edge-sensitive share at max_px {max_px}: {share:.4%}")
    assert 0 < share <= 0.02
    clean = FR.make_motion(3, 4, 17, 33, seed=12, lut=lut(), max_px=max_px)
    assert not FR.edge_sensitive(clean, torch.full((3,), max_px), lut()).any()


# ------------------------------------------------------------------ 5
def test_flags_parse_and_refusals_name_the_reason():
    from ccvs_amd.tools.options import Options
    from ccvs_amd.helpers.generator import Generator
    x = Options().parse(True, True, argv=TINY_ARGV)["transformer"]
    assert x.save_flow is False and x.save_flow_raw is False and x.flow_max_px == 0.0
    x = Options().parse(True, True, argv=TINY_ARGV + ["--save_flow", "--flow_max_px", "2.5", "--save_flow_raw"])["transformer"]
    assert x.save_flow is True and x.save_flow_raw is True and x.flow_max_px == 2.5
    gen = Generator(Options().parse(True, True, argv=TINY_ARGV + ["--save_flow"]))
    assert gen.save_flow and gen.flow_max_px == 0.0 and not gen.save_flow_raw
    assert gen.motion_bytes_per_clip_pixel(False) == 24.0 * 4 and gen.motion_bytes_per_clip_pixel(True) == 48.0 * 4
    assert Generator(Options().parse(True, True, argv=TINY_ARGV)).motion_bytes_per_clip_pixel(True) == 0.0
    no_inter = [a for a in TINY_ARGV if a != "--q_use_inter"]
    for argv, exc, word in ((no_inter + ["--save_flow"], ValueError, "--q_use_inter"),
                            (TINY_ARGV + ["--save_flow", "--step_by_step"], NotImplementedError, "--step_by_step"),
                            (TINY_ARGV + ["--save_flow", "--flow_max_px", "-1"], ValueError, "negative"),
                            (TINY_ARGV + ["--save_flow_raw"], ValueError, "--save_flow")):
        with pytest.raises(exc, match=word):
            Generator(Options().parse(True, True, argv=argv))


def test_flowviz_symbols_declared_named_and_exported(tmp_path):
    from ccvs_amd import lib
    header = open(os.path.join(ROOT, "include", "ccvs_hip_flowviz.h")).read()
    main = open(os.path.join(ROOT, "include", "ccvs_hip.h")).read()
    assert re.search(r'^#include "ccvs_hip_flowviz.h"', main, re.M)
    declared = sorted(set(re.findall(r"^\w[\w \*]*?\b(ccvs_\w+)\(", header, re.M)))
    assert declared == sorted(lib.FLOWVIZ_SYMBOLS) == ["ccvs_flow_export", "ccvs_flow_max", "ccvs_flow_render"]
    others = [getattr(lib, n) for n in dir(lib) if n.endswith("EXPORTS")]
    assert not any(set(lib.FLOWVIZ_SYMBOLS) & set(o) for o in others)
    handle = ctypes.CDLL(lib.LIB_PATH)
    for sym in lib.FLOWVIZ_SYMBOLS:
        assert hasattr(handle, sym), sym
    L = lib.load()
    assert L.ccvs_abi_version() == 6
    assert open(os.path.join(ROOT, "ccvs_amd", "csrc", "Makefile")).read().count("ccvs_hip_flowviz.h") == 1
    c = tmp_path / "p.c"
    c.write_text('#include "ccvs_hip.h"\nvoid* p[] = {' + ", ".join("(void*)" + s for s in lib.FLOWVIZ_SYMBOLS) + "};\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "p.o")], check=True)
    # refused by name before any launch (no GPU needed): null pointers, bad shapes, too many contexts, short strides, a misaligned output
    one = ctypes.c_void_p(16)
    assert L.ccvs_flow_export(None, 48, 1, 1, 4, 4, 1.0, one, 48, None) != 0 and b"null" in L.ccvs_last_error()
    assert L.ccvs_flow_export(one, 48, 1, 17, 4, 4, 1.0, one, 48, None) != 0 and b"contexts" in L.ccvs_last_error()
    assert L.ccvs_flow_export(one, 47, 1, 1, 4, 4, 1.0, one, 48, None) != 0 and b"stride" in L.ccvs_last_error()
    assert L.ccvs_flow_max(one, 48, 48, 1, 1, 0, 4, one, None) != 0 and b"shape" in L.ccvs_last_error()
    assert L.ccvs_flow_render(one, 48, 48, 1, 1, 4, 4, one, one, ctypes.c_void_p(18), one, None) != 0 and b"4-byte" in L.ccvs_last_error()
    from ccvs_amd import ops
    with pytest.raises(lib.CcvsError):
        ops.flow_max(torch.zeros(1, 1, 3, 2, 2))           # no CPU fallback


def test_save_results_writes_the_six_folders(tmp_path, monkeypatch):
    from ccvs_amd.tools.options import Options
    from ccvs_amd.helpers import generator as G
    gen = G.Generator(Options().parse(True, True, argv=TINY_ARGV + ["--save_flow", "--save_flow_raw", "--flow_max_px", "4", "--video_format", "npy"]))
    gen.opt.result_path = str(tmp_path)
    seen, rendered = [], []

    def fake_render(motion, max_px):
        rendered.append(max_px.tolist())
        z = torch.zeros(*motion.shape[:2], *motion.shape[3:], 3, dtype=torch.uint8)
        return z, z + 1

    monkeypatch.setattr(G.ops, "flow_render", fake_render)
    monkeypatch.setattr(G, "save_video_batch", lambda vid, bs, it, path, *a, **k: seen.append(("clip", os.path.basename(path), tuple(vid.shape))))
    monkeypatch.setattr(G, "write_u8_clips", lambda u8, dev, device, bs, it, path, fps, fmt, **k: seen.append(("u8", os.path.basename(path), int(u8.max()), fmt)))

    def clip(with_motion):
        d = {"vid": torch.zeros(2, 4, 3, 8, 8)}
        if with_motion:
            d.update(motion=torch.arange(2 * 4 * 3 * 8 * 8, dtype=torch.float32).view(2, 4, 3, 8, 8), warp=torch.ones(2, 4, 3, 8, 8), flow_dt=[0, 1, 1, 1])
        return d

    gen.save_results({"real": torch.zeros(2, 4, 3, 8, 8), "fake": clip(True), "rec": clip(True), "blur": None}, 3)
    assert [s[1] for s in seen] == ["real", "fake", "fake_flow", "fake_occ", "fake_warp", "rec", "rec_flow", "rec_occ", "rec_warp"]
    assert [s for s in seen if s[0] == "u8"] == [("u8", "fake_flow", 0, "npy"), ("u8", "fake_occ", 1, "npy"), ("u8", "rec_flow", 0, "npy"), ("u8", "rec_occ", 1, "npy")]
    assert rendered == [[4.0, 4.0], [4.0, 4.0]]
    for name in ("fake_motion", "rec_motion"):
        files = sorted(os.listdir(tmp_path / name))
        assert files == ["vid_00006.npy", "vid_00007.npy"]
        arr = np.load(tmp_path / name / files[1])
        assert arr.dtype == np.float32 and np.array_equal(arr, clip(True)["motion"][1].numpy())
    # a clip decoded by one decoder call carries no motion: nothing is written for it, and nothing without the flag
    seen.clear()
    gen.save_results({"real": torch.zeros(2, 4, 3, 8, 8), "fake": clip(False), "rec": None, "blur": None}, 0)
    assert [s[1] for s in seen] == ["real", "fake"]
    plain = G.Generator(Options().parse(True, True, argv=TINY_ARGV + ["--video_format", "npy"]))
    plain.opt.result_path = str(tmp_path / "plain")
    plain.save_results({"real": torch.zeros(2, 4, 3, 8, 8), "fake": clip(True), "rec": None, "blur": None}, 0)
    assert [s[1] for s in seen] == ["real", "fake", "real", "fake"]

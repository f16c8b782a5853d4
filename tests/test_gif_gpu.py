"""gpu: the GIF output stage (`ccvs_gif_palette`, `ccvs_gif_encode`, csrc/gif.hip) against the spec mirror
tests/gif_ref.py, which tests/test_gif_host.py holds against Pillow's decoder.  Every comparison is bit for bit.

  1. `ops.gif_palette` gives the mirror's palette, table and count: the clip table, the hand-made histograms, 200 colours, a strided
     view, and a batch of three different clips (every clip its own palette);
  2. `ops.gif_encode` gives the mirror's stream and offsets: the clip table at band_rows 0, 1, 3 and h; `ccvs_gif_encode` on chosen
     indices: the band-length sweep, the clear in mid-band, the sub-block edges; five frames in one launch equal their single launches,
     also under a CU budget, twice the same bytes; frame and clip strides with garbage between;
  3. capacity exact, one byte short and zero: complete offsets, the bytes beyond untouched, `gif_encode_to_host` recovers;
  4. files: `save_video_batch`, `write_u8_clips` and `Generator.run()` serial and pipelined write the same `.gif` files, which are the
     mirror's files of the clips the `npy` format writes and which Pillow decodes to palette[indices]; with `--save_flow` the motion
     folders hold `.gif` files, and a rendered flow clip of few colours comes back exactly; the other formats never reach the GIF calls.
"""
import ctypes
import io
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gif_ref as G  # noqa: E402
from tests.test_e2e_gpu import TINY_ARGV  # noqa: E402
from tests.test_mjpeg_opt_gpu import budgeted  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0xA5


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def encode_indices(idx, band_rows, capacity=None, extra=16, t=None):
    """`ccvs_gif_encode` on frames of chosen indices [n, H, W] (as b clips of t frames: one clip unless t is given) through the table of
    `G.direct_colours`, into a stream of `capacity` bytes with `extra` more behind it, all pre-filled with FILL; the workspace holds
    garbage.  (the whole stream on the host, the offsets)."""
    from ccvs_amd import lib
    L = lib.load()
    colours, table = G.direct_colours()
    idx = np.asarray(idx)
    n, h, w = idx.shape
    t = n if t is None else t
    b = n // t
    clips = torch.from_numpy(colours[idx]).cuda()
    tables = torch.from_numpy(np.tile(table, (b, 1))).cuda()
    if capacity is None:
        capacity = int(L.ccvs_gif_stream_bound(n, h, w, band_rows))
    out = torch.full((capacity + extra,), FILL, dtype=torch.uint8, device="cuda")
    offsets = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    work = torch.randint(0, 256, (L.ccvs_gif_workspace_bytes(b, t, h, w, band_rows),), dtype=torch.uint8, device="cuda",
                         generator=torch.Generator("cuda").manual_seed(n * h + w))
    rc = L.ccvs_gif_encode(_p(clips), t * h * w * 3, h * w * 3, b, t, h, w, band_rows, _p(tables), _p(out), capacity, _p(offsets), _p(work),
                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.ccvs_last_error().decode()
    return out.cpu().numpy(), offsets.cpu().tolist()


def same_as_mirror(idx, band_rows, tag, **kw):
    want, off_w = G.encode_indices(idx, band_rows)
    got, off = encode_indices(idx, band_rows, **kw)
    assert off == [int(v) for v in off_w], (tag, off[-1], int(off_w[-1]))
    diff = np.flatnonzero(got[:len(want)] != np.frombuffer(want, np.uint8))
    assert diff.size == 0, (tag, "first differing byte", int(diff[0]), "of", len(want))
    assert (got[len(want):] == FILL).all(), tag


# ------------------------------------------------------------------ 1
def _palette_equals(clips, tag):
    from ccvs_amd import ops
    pal, table, used = ops.gif_palette(clips)
    host = clips.cpu().numpy()
    host = host[None] if host.ndim == 4 else host
    assert pal.shape == (len(host), 256, 3) and table.shape == (len(host), 32768) and used.dtype == torch.int32
    for i, clip in enumerate(host):
        want_pal, want_table, want_used = G.palette(clip)
        assert int(used[i]) == want_used, (tag, i, int(used[i]), want_used)
        assert np.array_equal(pal[i].cpu().numpy(), want_pal), (tag, i)
        assert np.array_equal(table[i].cpu().numpy(), want_table), (tag, i)


def test_palette_equals_the_mirror():
    for name, clip in G.clips().items():
        _palette_equals(torch.from_numpy(clip.copy()).cuda()[None], name)
    _palette_equals(torch.from_numpy(G.colours_200()).cuda(), "200 colours")                 # [T, H, W, 3]: one clip
    hand = ([(0, 2, 0, 1), (2, 0, 0, 1), (1, 1, 0, 2)], [(0, 0, 2, 1), (2, 0, 0, 1), (1, 0, 1, 2)], [(0, 0, 0, 1), (1, 0, 0, 1), (10, 0, 0, 1), (11, 0, 0, 1)],
            [(0, 0, 0, 1), (1, 0, 0, 1), (10, 0, 0, 1), (12, 0, 0, 1)], [(0, 0, 0, 2), (2, 0, 0, 2), (4, 0, 0, 4)], [(0, 0, 0, 2), (2, 0, 0, 1), (4, 0, 0, 4)],
            [(0, 5, 0, 1), (0, 9, 0, 10)], [(r, (3 * r) % 32, (7 * r) % 32, 1 + r % 3) for r in range(20)], [(31, 31, 31, 5)])
    for k, bins in enumerate(hand):
        _palette_equals(torch.from_numpy(G.clip_of_bins(bins)).cuda(), ("hand", k))


def _three():
    rng = np.random.default_rng(5)
    smooth = G.clips()["smooth_3x23x17"]
    noise = rng.integers(0, 256, smooth.shape).astype(np.uint8)
    dark = (rng.integers(0, 256, smooth.shape) // 9 * np.array([1, 0, 2])).astype(np.uint8)
    return np.stack([smooth, noise, dark])


def test_palette_per_clip_and_through_strided_views():
    batch = _three()
    _palette_equals(torch.from_numpy(batch).cuda(), "three clips")
    # frames at odd addresses with garbage between them, clips further apart than their frames need
    t, h, w = batch.shape[1:4]
    raw = h * w * 3
    fs, cs = raw + 61, 3 * (raw + 61) + 1000
    buf = torch.randint(0, 256, (3 * cs,), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    view = buf.as_strided((3, t, h, w, 3), (cs, fs, 3 * w, 3, 1))
    view.copy_(torch.from_numpy(batch).cuda())
    assert view.stride()[:2] == (cs, fs) and not view.is_contiguous()
    _palette_equals(view, "strided")
    _palette_equals(torch.from_numpy(batch).cuda()[:, ::2], "every other frame")


# ------------------------------------------------------------------ 2
def test_encode_equals_the_mirror_on_the_clip_table():
    from ccvs_amd import ops
    dev = {name: torch.from_numpy(clip.copy()).cuda()[None] for name, clip in G.clips().items()}
    for name, r in G.rows():
        m = G.mirrored(name, r)
        stream, offsets, pal = ops.gif_encode(dev[name], r, capacity=m["off"][-1] + 9)
        assert offsets.tolist() == m["off"], (name, r)
        assert stream[:m["off"][-1]].cpu().numpy().tobytes() == m["stream"], (name, r)
        assert np.array_equal(pal[0].cpu().numpy(), m["pal"]), (name, r)
    print("rows", len(G.rows()))


def test_band_length_sweep_equals_the_mirror():
    for L in G.BAND_SWEEP:
        for kind in ("noise", "flat", "two"):
            same_as_mirror(G.sweep_indices(L, kind)[None], L, (L, kind))


def test_clear_in_mid_band_and_sub_block_edges():
    rng = np.random.default_rng(11)
    for shape, r in (((1, 1, 5000), 0), ((1, 1, 5000), 1), ((2, 50, 100), 50), ((1, 3, 4100), 3), ((1, 2, 9001), 1)):
        same_as_mirror(rng.integers(0, 256, shape).astype(np.uint8), r, (shape, r))
    for target in (254, 255, 256, 510):
        same_as_mirror(G.edge_frame(target)[None], 0, ("edge", target))


def test_five_frames_in_one_launch_equal_their_single_launches():
    rng = np.random.default_rng(6)
    idx = np.stack([rng.integers(0, 256, (33, 65)), np.full((33, 65), 9), rng.integers(0, 2, (33, 65)) * 255,
                    (np.arange(33)[:, None] + np.arange(65)[None]) % 256, rng.integers(0, 16, (33, 65))]).astype(np.uint8)
    for r in (0, 5, 1, 33):                                             # 1, 7, 33 and 1 bands per frame
        singles = [G.encode_indices(idx[i:i + 1], r)[0] for i in range(5)]
        for i in (0, 3):
            got, off = encode_indices(idx[i:i + 1], r, capacity=len(singles[i]), extra=0)
            assert off == [0, len(singles[i])] and got.tobytes() == singles[i], (r, i)
        want = b"".join(singles)
        for lim in (0, 1):                                              # 1: a few workgroups walk over all bands and frames
            runs = [budgeted(lim, lambda: encode_indices(idx, r, capacity=len(want) + 5, extra=0)) for _ in range(2)]
            got, off = runs[0]
            assert off == list(np.cumsum([0] + [len(x) for x in singles])), (r, lim)
            assert got[:len(want)].tobytes() == want and (got[len(want):] == FILL).all(), (r, lim)
            assert runs[1][1] == off and np.array_equal(runs[1][0], got)             # the same bytes on every run
        got, off = encode_indices(idx[:4], r, t=2)                                   # two clips of two frames: the frames in the clips' order
        assert off == list(np.cumsum([0] + [len(x) for x in singles[:4]])) and got[:off[-1]].tobytes() == b"".join(singles[:4]), r


def test_strides_with_garbage_between_the_frames():
    from ccvs_amd import ops
    batch = _three()
    t, h, w = batch.shape[1:4]
    raw = h * w * 3
    fs, cs = raw + 61, 3 * (raw + 61) + 1000
    buf = torch.randint(0, 256, (3 * cs,), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    view = buf.as_strided((3, t, h, w, 3), (cs, fs, 3 * w, 3, 1))
    view.copy_(torch.from_numpy(batch).cuda())
    wants = [G.encode(clip, 4) for clip in batch]
    want = b"".join(x[0] for x in wants)
    stream, offsets, pal = ops.gif_encode(view, 4, capacity=len(want) + 7)      # (the noise clip needs more than the default byte per pixel)
    assert offsets.tolist() == list(np.cumsum([0] + [int(b - a) for x in wants for a, b in zip(x[1][:-1], x[1][1:])]))
    assert stream[:len(want)].cpu().numpy().tobytes() == want and np.array_equal(pal.cpu().numpy(), np.stack([x[2] for x in wants]))
    data, off, pals = ops.gif_encode_to_host(torch.from_numpy(batch).cuda()[:, ::2], 0)  # a time-strided view
    wants = [G.encode(clip[::2], 0) for clip in batch]
    assert data == b"".join(x[0] for x in wants) and np.array_equal(pals, np.stack([x[2] for x in wants])) and len(off) == 7


# ------------------------------------------------------------------ 3
def test_capacity_keeps_offsets_and_writes_nothing_beyond():
    from ccvs_amd import lib, ops
    rng = np.random.default_rng(8)
    idx = np.stack([rng.integers(0, 256, (33, 65)), (np.arange(33)[:, None] * 3 + np.arange(65)[None]) % 256]).astype(np.uint8)
    want, off_w = G.encode_indices(idx, 8)                              # 5 bands per frame
    off_w = [int(v) for v in off_w]
    want = np.frombuffer(want, np.uint8)
    for capacity in (len(want), len(want) - 1, 0, 1, off_w[1] + 3):     # exact, one byte short, zero, and two more
        got, off = encode_indices(idx, 8, capacity=capacity, extra=64)
        assert off == off_w, capacity
        assert (got[capacity:] == FILL).all(), capacity
        assert np.array_equal(got[:capacity], want[:capacity]), capacity
    # a null stream goes with capacity 0
    L = lib.load()
    colours, table = G.direct_colours()
    clips, tables = torch.from_numpy(colours[idx]).cuda(), torch.from_numpy(table).cuda()
    offsets = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    work = torch.empty(L.ccvs_gif_workspace_bytes(1, 2, 33, 65, 8), dtype=torch.uint8, device="cuda")
    assert L.ccvs_gif_encode(_p(clips), 2 * 33 * 65 * 3, 33 * 65 * 3, 1, 2, 33, 65, 8, _p(tables), None, 0, _p(offsets), _p(work), None) == 0
    torch.cuda.synchronize()
    assert offsets.tolist() == off_w
    # through ops, on a noise clip, whose frames need more than the default byte per pixel: the offsets say so, the host form runs again
    clip = G.clips()["noise_2x33x65"]
    dev = torch.from_numpy(clip.copy()).cuda()[None]
    m = G.mirrored("noise_2x33x65", 8)
    stream, offsets, _ = ops.gif_encode(dev, 8)
    assert offsets.tolist() == m["off"] and m["off"][-1] > stream.numel()
    assert stream.cpu().numpy().tobytes() == m["stream"][:stream.numel()]
    out = torch.full((100,), FILL, dtype=torch.uint8, device="cuda")
    stream, offsets, _ = ops.gif_encode(dev, 8, out=out)
    assert stream is out and offsets.tolist() == m["off"] and out.cpu().numpy().tobytes() == m["stream"][:100]
    data, off, pals = ops.gif_encode_to_host(dev, 8)
    assert off == m["off"] and data == m["stream"] and np.array_equal(pals[0], m["pal"])


# ------------------------------------------------------------------ 4
def _pil_frames(path):
    from PIL import Image
    with Image.open(path) as im:
        out = []
        for t in range(getattr(im, "n_frames", 1)):
            im.seek(t)
            out.append(np.asarray(im.convert("RGB")).copy())
        return np.stack(out), im.info.get("duration"), im.info.get("loop")


def _mirror_file(clip, fps):
    """(the mirror's file of a uint8 clip [T, H, W, 3], palette[indices])."""
    stream, off, pal, table, _ = G.encode(clip, 0)
    t, h, w = clip.shape[:3]
    return G.gif_file([stream[off[i]:off[i + 1]] for i in range(t)], pal, fps, h, w), pal[G.indices(clip, table)]


def test_save_video_batch_gif(tmp_path):
    pytest.importorskip("PIL")
    from ccvs_amd.helpers.generator import save_video_batch, write_u8_clips
    from ccvs_amd.tools import gif
    vid = torch.rand(2, 3, 3, 24, 40, generator=torch.Generator().manual_seed(5)) * 2.4 - 1.2
    vid[1, 2] = 0.25                                                    # a flat frame among them
    state = torch.tensor([[[0.1, 0.2], [0.5, 0.5], [0.99, 0.0]], [[0.3, 0.9], [0.0, 0.0], [0.7, 0.4]]])
    cases = {"span": dict(imagenet_norm=False), "imagenet": dict(imagenet_norm=True), "state": dict(imagenet_norm=False, state=state),
             "named": dict(imagenet_norm=False, cat=["a", "b"], idx=[7, 8])}
    for tag, kw in cases.items():
        norm = kw.pop("imagenet_norm")
        d = tmp_path / tag
        dataset = "bair" if tag == "state" else "kinetics600"
        u8 = save_video_batch(vid.cuda(), 2, 3, str(d), 4, True, norm, [-1, 1], dataset, video_format="gif", quality=10, subsampling="420", optimize=True,
                              lz77=True, **kw)
        assert u8.shape == (2, 3, 24, 40, 3) and u8.dtype == torch.uint8 and not u8.is_cuda
        names = [f"vid_{6 + i:05d}" + (f"_{'ab'[i]}_{7 + i}" if tag == "named" else "") + ".gif" for i in range(2)]
        assert sorted(os.listdir(d)) == names
        for i, n in enumerate(names):
            data, shown = _mirror_file(u8[i].numpy(), 4)
            assert (d / n).read_bytes() == data, (tag, i)
            frames, duration, loop = _pil_frames(str(d / n))
            assert duration == 250 and loop == 0 and np.array_equal(frames, shown), (tag, i)
            assert np.array_equal(gif.read_gif(str(d / n)), shown), (tag, i)
        e = tmp_path / (tag + "_nc")                                    # return_clip=False (what `save_results` asks for): the same files, no clip
        assert save_video_batch(vid.cuda(), 2, 3, str(e), 4, True, norm, [-1, 1], dataset, video_format="gif", return_clip=False, **kw) is None or tag == "state"
        assert all((e / n).read_bytes() == (d / n).read_bytes() for n in names)
    # the largest shape of this module: one clip of two 256 x 256 frames, through `write_u8_clips` on the device
    big = (torch.rand(1, 2, 256, 256, 3, generator=torch.Generator().manual_seed(7)) * 255).to(torch.uint8)
    big[0, 1, 64:192] = big[0, 0, 64:192] // 32 * 32
    write_u8_clips(big.cuda(), big.cuda(), "cuda", 1, 0, str(tmp_path / "big"), 25, "gif")
    data, shown = _mirror_file(big[0].numpy(), 25)
    assert (tmp_path / "big" / "vid_00000.gif").read_bytes() == data
    frames, duration, _ = _pil_frames(str(tmp_path / "big" / "vid_00000.gif"))
    assert duration == 40 and np.array_equal(frames, shown)


def test_other_formats_never_reach_the_gif_calls(tmp_path, monkeypatch):
    """A call without the format launches and allocates what it did: the GIF stage is reached through `write_u8_clips(video_format="gif")`
    alone -- with its three entry points and the two C calls poisoned, every other format writes its files."""
    from ccvs_amd import lib, ops
    from ccvs_amd.helpers.generator import save_video_batch

    def poisoned(*a, **k):
        raise AssertionError("the GIF stage was reached")
    for name in ("gif_palette", "gif_encode", "gif_encode_to_host", "_gif_palette"):
        monkeypatch.setattr(ops, name, poisoned)
    L = lib.load()
    kept = L.ccvs_gif_palette, L.ccvs_gif_encode
    L.ccvs_gif_palette = L.ccvs_gif_encode = poisoned
    try:
        vid = torch.rand(2, 3, 3, 24, 40, generator=torch.Generator().manual_seed(6)) * 2 - 1
        for fmt, ext in ((None, None), ("npy", ".npy"), ("avi", ".avi"), ("apng", ".png")):
            d = tmp_path / str(fmt)
            save_video_batch(vid.cuda(), 2, 0, str(d), 4, True, False, [-1, 1], "kinetics600", video_format=fmt)
            assert len(os.listdir(d)) == 2 and (ext is None or all(n.endswith(ext) for n in os.listdir(d)))
        with pytest.raises(AssertionError, match="GIF stage"):
            save_video_batch(vid.cuda(), 2, 0, str(tmp_path / "gif"), 4, True, False, [-1, 1], "kinetics600", video_format="gif")
    finally:
        L.ccvs_gif_palette, L.ccvs_gif_encode = kept


def _run(root, mode, extra):
    """`Generator(opt).run()` at the tiny geometry, 2 batches of 2 clips: (the results' folder, {(folder, file): bytes})."""
    from ccvs_amd.tools.options import Options
    from ccvs_amd.helpers.generator import Generator
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("CCVS_RUN_SCHEDULE", mode)
        torch.manual_seed(0)
        argv = TINY_ARGV + ["--n_iter", "2", "--x_top_k", "10", "--x_sample", "--save_path", str(root)] + extra
        opt = Options().parse(load_qvid_generator=True, load_transformer=True, argv=argv)
        gen = Generator(opt)
        torch.manual_seed(9)
        gen.run()
    top, files = opt["transformer"].result_path, {}
    for kind in sorted(os.listdir(top)):
        for n in sorted(os.listdir(os.path.join(top, kind))):
            files[kind, n] = open(os.path.join(top, kind, n), "rb").read()
    return top, files


def test_run_writes_gif_files_pipelined_equals_serial(tmp_path):
    pytest.importorskip("PIL")
    from ccvs_amd.helpers.generator import write_u8_clips
    runs = {tag: _run(tmp_path / tag, mode, extra) for tag, mode, extra in (
        ("gif", "pipelined", ["--video_format", "gif", "--video_quality", "5", "--video_subsampling", "420", "--video_optimize", "--video_lz77"]),
        ("serial", "serial", ["--video_format", "gif"]), ("npy", "pipelined", ["--video_format", "npy"]))}
    files = runs["gif"][1]
    assert files == runs["serial"][1]                                   # (and the other formats' flags beside gif moved nothing)
    assert sorted(files) == sorted((kind, f"vid_{i:05d}.gif") for kind in ("real", "fake", "rec") for i in range(4))
    fps = None
    for (kind, name), data in files.items():
        clip = np.load(os.path.join(runs["npy"][0], kind, name[:-4] + ".npy"))
        frames, duration, loop = _pil_frames(os.path.join(runs["gif"][0], kind, name))
        fps = fps or round(1000 / duration)
        want, shown = _mirror_file(clip, fps)
        assert frames.shape == (4, 32, 32, 3) and loop == 0 and np.array_equal(frames, shown), (kind, name)
        assert data == want, (kind, name)
    # `write_u8_clips` on the clips of the .npy files: the run's files
    for kind in ("real", "fake"):
        clips = torch.from_numpy(np.stack([np.load(os.path.join(runs["npy"][0], kind, f"vid_{i:05d}.npy")) for i in (2, 3)]))
        write_u8_clips(clips.cuda(), clips.cuda(), "cuda", 2, 1, str(tmp_path / "again" / kind), fps, "gif")
        for i in (2, 3):
            assert (tmp_path / "again" / kind / f"vid_{i:05d}.gif").read_bytes() == files[kind, f"vid_{i:05d}.gif"], (kind, i)


def test_save_flow_folders_and_a_flow_clip_of_few_colours(tmp_path):
    pytest.importorskip("PIL")
    from ccvs_amd import ops
    from ccvs_amd.helpers.generator import write_u8_clips
    top, files = _run(tmp_path / "flow", "pipelined", ["--save_flow", "--video_format", "gif"])
    names = [f"vid_{i:05d}.gif" for i in range(4)]
    kinds = ["real", "fake", "rec"] + [f"{side}_{kind}" for side in ("fake", "rec") for kind in ("flow", "occ", "warp")]
    assert sorted(files) == sorted((kind, n) for kind in kinds for n in names)
    for kind in ("fake_flow", "fake_occ", "rec_flow"):
        frames, _, loop = _pil_frames(os.path.join(top, kind, names[1]))
        assert frames.shape == (4, 32, 32, 3) and loop == 0
    # a flow field that is constant on 8 x 8 blocks renders to few colours, far apart: the file holds the rendered clip exactly
    rng = np.random.default_rng(12)
    order = rng.permutation(48).reshape(1, 3, 4, 4)                     # 16 directions x 3 magnitudes, each on one block
    ang, mag = (order % 16 + 0.5) * (2 * np.pi / 16), np.array([1.0, 2.5, 4.0])[order // 16]
    coarse = np.stack([mag * np.cos(ang), mag * np.sin(ang), rng.choice([0.0, 0.5, 1.0], (1, 3, 4, 4))], 2)         # [1, 3, 3, 4, 4]
    motion = torch.from_numpy(np.kron(coarse, np.ones((8, 8)))).float().cuda()
    for k, u8 in enumerate(ops.flow_render(motion, torch.full((1,), 4.0, device="cuda"))):
        clip = u8[0].cpu().numpy()
        cnt, _ = G.histogram(clip)
        colours = np.unique(clip.reshape(-1, 3), axis=0)
        assert len(colours) <= 256 and len(colours) == np.count_nonzero(cnt), (k, len(colours), np.count_nonzero(cnt))    # each in a bin of its own
        write_u8_clips(u8, u8, u8.device, 1, k, str(tmp_path / "few"), 10, "gif")
        frames, _, _ = _pil_frames(str(tmp_path / "few" / f"vid_{k:05d}.gif"))
        assert np.array_equal(frames, clip), k

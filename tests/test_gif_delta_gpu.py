"""gpu: the changed-rectangle GIF frames (`ccvs_gif_palette_n`, `ccvs_gif_encode_delta`, csrc/gif.hip) against the
spec mirror tests/gif_delta_ref.py, which tests/test_gif_delta_host.py holds against Pillow's decoder.  Every comparison is bit for bit,
and `stream`, `offsets` and `rects` are poisoned before every call.

  1. `ops.gif_palette(max_colours=...)` gives the mirror's palette, table and count at 2, 16, 255 and 256; `ccvs_gif_palette_n` called
     directly with 256, on poisoned outputs, gives `ccvs_gif_palette`'s bytes and the mirror's;
  2. `ccvs_gif_encode_delta` on chosen indices gives the mirror's stream, offsets and rectangles: identical frames, corners, edges, thin
     rectangles, a tie, a larger rectangle, two clips whose boundary frames match, a 7 x 150 rectangle (1050 indices in one band, across
     the 1024-index chunk), a 64 x 64 rectangle in a frame 100 wide (a band of 4096 indices, more than any full-frame band);
     `ops.gif_encode(delta=True)` on the clip table at band_rows 0, 1, 3 and h, 255 colours, many bins;
  3. two and three clips per launch equal their single launches, also under a CU budget, twice the same bytes; frame and clip strides;
  4. capacity exact, one byte short and zero: complete offsets and rectangles, the bytes beyond untouched, `gif_encode_to_host` recovers;
  5. files: `save_video_batch`, `write_u8_clips` and `Generator.run()` serial and pipelined write the mirror's files, which Pillow decodes
     to palette[indices]; a rendered `--save_flow` clip of few colours comes back exactly; without the flag the new entries are never
     reached and the files are the full-frame ones.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gif_delta_ref as D  # noqa: E402
import gif_ref as G  # noqa: E402
from tests.test_e2e_gpu import TINY_ARGV  # noqa: E402
from tests.test_mjpeg_opt_gpu import budgeted  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0xA5


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def encode_indices(idx, band_rows, t=None, capacity=None, extra=16):
    """`ccvs_gif_encode_delta` on frames of chosen indices [n, H, W] below 255 (clips of t frames: one clip unless t is given) through
    the table of `D.direct_colours`, into a stream of `capacity` bytes with `extra` more behind it, pre-filled with FILL; offsets and
    rects are pre-filled too, the workspace holds garbage.  (the whole stream on the host, the offsets, the rects)."""
    from ccvs_amd import lib
    L = lib.load()
    colours, table = D.direct_colours()
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
    rects = torch.full((n + 1, 4), -7, dtype=torch.int32, device="cuda")            # (a row more than the call may write)
    work = torch.randint(0, 256, (L.ccvs_gif_delta_workspace_bytes(b, t, h, w, band_rows),), dtype=torch.uint8, device="cuda",
                         generator=torch.Generator("cuda").manual_seed(n * h + w))
    rc = L.ccvs_gif_encode_delta(_p(clips), t * h * w * 3, h * w * 3, b, t, h, w, band_rows, _p(tables), _p(out), capacity, _p(offsets),
                                 _p(rects), _p(work), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.ccvs_last_error().decode()
    rects = rects.cpu().numpy()
    assert (rects[n] == -7).all()
    return out.cpu().numpy(), offsets.cpu().tolist(), rects[:n]


def same_as_mirror(name, band_rows, **kw):
    m = D.mirrored_indices(name, band_rows)
    got, off, rects = encode_indices(m["idx"], band_rows, t=m["t"], **kw)
    assert np.array_equal(rects, m["rects"]), (name, band_rows, rects.tolist(), m["rects"].tolist())
    assert off == m["off"], (name, band_rows, off, m["off"])
    want = np.frombuffer(m["stream"], np.uint8)
    diff = np.flatnonzero(got[:len(want)] != want)
    assert diff.size == 0, (name, band_rows, "first differing byte", int(diff[0]), "of", len(want))
    assert (got[len(want):] == FILL).all(), (name, band_rows)


# ------------------------------------------------------------------ 1
def palette_n_direct(dev, max_colours):
    """`ccvs_gif_palette_n` through ctypes on one clip [T, H, W, 3] (or [1, T, H, W, 3]) on the device: palette, table and used pre-filled
    with poison, the workspace with garbage."""
    from ccvs_amd import lib
    L = lib.load()
    clip = dev if dev.dim() == 5 else dev[None]
    assert clip.is_contiguous()
    b, t, h, w = (int(v) for v in clip.shape[:4])
    palette = torch.full((b, 256, 3), FILL, dtype=torch.uint8, device="cuda")
    table = torch.full((b, 32768), FILL, dtype=torch.uint8, device="cuda")
    used = torch.full((b,), -7, dtype=torch.int32, device="cuda")
    work = torch.randint(0, 256, (L.ccvs_gif_delta_workspace_bytes(b, t, h, w, 0),), dtype=torch.uint8, device="cuda",
                         generator=torch.Generator("cuda").manual_seed(t * h + w))
    rc = L.ccvs_gif_palette_n(_p(clip), t * h * w * 3, h * w * 3, b, t, h, w, max_colours, _p(palette), _p(table), _p(used), _p(work),
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.ccvs_last_error().decode()
    return palette, table, used


def test_palette_n_equals_the_mirror():
    from ccvs_amd import ops
    clips = [G.clip_of_bins(bins) for bins in D.HAND] + [G.clips()[n][None] for n in ("noise_2x33x65", "smooth_5x64x96", "two_4x40x31")]
    clips += [D.colours_255()[None], D.many_bins_clip()[None]]
    for k, clip in enumerate(clips):
        dev = torch.from_numpy(np.ascontiguousarray(clip)).cuda()
        for cap in (2, 16, 255, 256):
            pal, table, used = ops.gif_palette(dev, cap)
            want_pal, want_table, want_used = D.palette_n(clip[0], cap)
            assert int(used[0]) == want_used, (k, cap, int(used[0]), want_used)
            assert np.array_equal(pal[0].cpu().numpy(), want_pal) and np.array_equal(table[0].cpu().numpy(), want_table), (k, cap)
        # `ccvs_gif_palette_n` itself at 256 (`ops.gif_palette` hands 256 to `ccvs_gif_palette`): that entry's bytes and the mirror's
        plain = ops.gif_palette(dev)
        for cap in (256, 255):
            got = palette_n_direct(dev, cap)
            want = plain if cap == 256 else ops.gif_palette(dev, 255)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (k, cap)
            mirror = D.palette_n(clip[0], cap)
            assert int(got[2][0]) == mirror[2] and np.array_equal(got[0][0].cpu().numpy(), mirror[0]), (k, cap)
            assert np.array_equal(got[1][0].cpu().numpy(), mirror[1]), (k, cap)
    batch = torch.from_numpy(np.stack([G.clips()["smooth_3x23x17"], D.many_bins_clip()[:3, :23, :17]])).cuda()       # every clip its own
    pal, table, used = ops.gif_palette(batch, 255)
    for i in range(2):
        want = D.palette_n(batch[i].cpu().numpy(), 255)
        assert int(used[i]) == want[2] and np.array_equal(pal[i].cpu().numpy(), want[0]) and np.array_equal(table[i].cpu().numpy(), want[1]), i


# ------------------------------------------------------------------ 2
def test_index_cases_equal_the_mirror():
    for name, r in D.index_rows():
        same_as_mirror(name, r)
    print("rows", len(D.index_rows()))


def test_identical_frames_are_seven_bytes_each():
    idx, t = D.index_cases()["identical_5x40x56"]
    got, off, rects = encode_indices(idx, 0)
    for f in range(1, 5):
        assert got[off[f]:off[f + 1]].tobytes() == D.NOTHING and rects[f].tolist() == [0, 0, 1, 1], f


def test_a_band_across_the_chunk_and_a_band_larger_than_the_full_frames():
    m = D.mirrored_indices("chunk_2x160x9", 0)
    assert m["rects"][1].tolist() == [1, 5, 7, 150] and m["dsize"][1] < m["fsize"][1]
    same_as_mirror("chunk_2x160x9", 0)
    m = D.mirrored_indices("big_band_2x64x100", 0)
    assert m["rects"][1].tolist() == [18, 0, 64, 64] and m["dsize"][1] < m["fsize"][1]
    same_as_mirror("big_band_2x64x100", 0)


def test_encode_equals_the_mirror_on_the_clip_table():
    from ccvs_amd import ops
    dev = {name: torch.from_numpy(clip.copy()).cuda()[None] for name, clip in G.clips().items()}
    for name, r in G.rows():
        m = D.mirrored(name, r)
        out = torch.full((m["off"][-1] + 9,), FILL, dtype=torch.uint8, device="cuda")
        stream, offsets, pal, rects = ops.gif_encode(dev[name], r, out=out, delta=True)
        assert offsets.tolist() == m["off"] and np.array_equal(rects.cpu().numpy(), m["rects"]), (name, r)
        assert stream[:m["off"][-1]].cpu().numpy().tobytes() == m["stream"] and (stream[m["off"][-1]:] == FILL).all(), (name, r)
        assert np.array_equal(pal[0].cpu().numpy(), m["pal"]), (name, r)
    for tag, clip in (("255 colours", D.colours_255()), ("many bins", D.many_bins_clip())):
        want = D.encode(clip, 0)
        data, off, pals, rects = ops.gif_encode_to_host(torch.from_numpy(clip).cuda(), 0, delta=True)
        assert data == want[0] and off == [int(v) for v in want[1]] and np.array_equal(pals[0], want[2]) and np.array_equal(rects, want[5]), tag
        assert any(tuple(r) != (0, 0, clip.shape[2], clip.shape[1]) for r in rects[1:]), tag
    print("rows", len(G.rows()))


# ------------------------------------------------------------------ 3
def _clips_of_indices():
    """Three clips of three 33 x 65 index frames: a moving block on noise, identical frames, two-valued noise."""
    rng = np.random.default_rng(6)
    a = np.stack([rng.integers(0, 255, (33, 65))] * 3)
    a[1, 4:20, 10:50] = rng.integers(0, 255, (16, 40))
    a[2] = a[1]
    a[2, 30:33, 60:65] = (a[2, 30:33, 60:65] + 9) % 255
    b = np.stack([rng.integers(0, 16, (33, 65))] * 3)
    c = rng.integers(0, 2, (3, 33, 65)) * 254
    return np.concatenate([a, b, c]).astype(np.uint8)


def test_two_and_three_clips_per_launch_equal_their_single_launches():
    idx = _clips_of_indices()
    for r in (0, 5, 1, 33):
        singles = [D.encode_indices(idx[3 * i:3 * i + 3], r) for i in range(3)]
        for i in range(3):
            got, off, rects = encode_indices(idx[3 * i:3 * i + 3], r, capacity=len(singles[i][0]), extra=0)
            assert off == [int(v) for v in singles[i][1]] and got.tobytes() == singles[i][0] and np.array_equal(rects, singles[i][2]), (r, i)
        for k in (2, 3):
            want = b"".join(s[0] for s in singles[:k])
            want_off = list(np.cumsum([0] + [int(b - a) for s in singles[:k] for a, b in zip(s[1][:-1], s[1][1:])]))
            want_rects = np.concatenate([s[2] for s in singles[:k]])
            for lim in (0, 1):                                          # 1: a few workgroups walk over all frames, bands and candidates
                runs = [budgeted(lim, lambda: encode_indices(idx[:3 * k], r, t=3, capacity=len(want) + 5, extra=0)) for _ in range(2)]
                got, off, rects = runs[0]
                assert off == want_off and np.array_equal(rects, want_rects), (r, k, lim)
                assert got[:len(want)].tobytes() == want and (got[len(want):] == FILL).all(), (r, k, lim)
                assert runs[1][1] == off and np.array_equal(runs[1][0], got) and np.array_equal(runs[1][2], rects)   # the same bytes on every run
        assert [tuple(r) for r in singles[1][2][1:]] == [(0, 0, 1, 1)] * 2 and tuple(singles[0][2][1]) == (10, 4, 40, 16)


def test_strides_with_garbage_between_the_frames():
    from ccvs_amd import ops
    batch = np.stack([D.many_bins_clip()[:3, :23, :17], G.clips()["smooth_3x23x17"], D.colours_255()[:, :23, :17]])
    t, h, w = batch.shape[1:4]
    raw = h * w * 3
    fs, cs = raw + 61, 3 * (raw + 61) + 1000
    buf = torch.randint(0, 256, (3 * cs,), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    view = buf.as_strided((3, t, h, w, 3), (cs, fs, 3 * w, 3, 1))
    view.copy_(torch.from_numpy(batch).cuda())
    assert view.stride()[:2] == (cs, fs) and not view.is_contiguous()
    wants = [D.encode(clip, 4) for clip in batch]
    want = b"".join(x[0] for x in wants)
    out = torch.full((len(want) + 7,), FILL, dtype=torch.uint8, device="cuda")
    stream, offsets, pal, rects = ops.gif_encode(view, 4, out=out, delta=True)
    assert offsets.tolist() == list(np.cumsum([0] + [int(b - a) for x in wants for a, b in zip(x[1][:-1], x[1][1:])]))
    assert stream[:len(want)].cpu().numpy().tobytes() == want and (stream[len(want):] == FILL).all()
    assert np.array_equal(pal.cpu().numpy(), np.stack([x[2] for x in wants])) and np.array_equal(rects.cpu().numpy(), np.concatenate([x[5] for x in wants]))
    data, off, pals, rects = ops.gif_encode_to_host(torch.from_numpy(batch).cuda()[:, ::2], 0, delta=True)           # a time-strided view
    wants = [D.encode(clip[::2], 0) for clip in batch]
    assert data == b"".join(x[0] for x in wants) and np.array_equal(pals, np.stack([x[2] for x in wants])) and len(off) == 7
    assert np.array_equal(rects, np.concatenate([x[5] for x in wants]))


# ------------------------------------------------------------------ 4
def test_capacity_keeps_offsets_and_rects_and_writes_nothing_beyond():
    from ccvs_amd import lib, ops
    idx = _clips_of_indices()[:6]
    want, off_w, rects_w, _, _ = D.encode_indices(idx, 8, 3)            # 5 band slots per candidate
    off_w = [int(v) for v in off_w]
    want = np.frombuffer(want, np.uint8)
    for capacity in (len(want), len(want) - 1, 0, 1, off_w[1] + 3):     # exact, one byte short, zero, and two more
        got, off, rects = encode_indices(idx, 8, t=3, capacity=capacity, extra=64)
        assert off == off_w and np.array_equal(rects, rects_w), capacity
        assert (got[capacity:] == FILL).all(), capacity
        assert np.array_equal(got[:capacity], want[:capacity]), capacity
    # a null stream goes with capacity 0
    L = lib.load()
    colours, table = D.direct_colours()
    clips, tables = torch.from_numpy(colours[idx]).cuda(), torch.from_numpy(np.tile(table, (2, 1))).cuda()
    offsets = torch.full((7,), -1, dtype=torch.int64, device="cuda")
    rects = torch.full((6, 4), -7, dtype=torch.int32, device="cuda")
    work = torch.empty(L.ccvs_gif_delta_workspace_bytes(2, 3, 33, 65, 8), dtype=torch.uint8, device="cuda")
    assert L.ccvs_gif_encode_delta(_p(clips), 3 * 33 * 65 * 3, 33 * 65 * 3, 2, 3, 33, 65, 8, _p(tables), None, 0, _p(offsets), _p(rects), _p(work), None) == 0
    torch.cuda.synchronize()
    assert offsets.tolist() == off_w and np.array_equal(rects.cpu().numpy(), rects_w)
    # through ops, on a noise clip, whose frames need more than the default byte per pixel: the offsets say so, the host form runs again
    clip = G.clips()["noise_2x33x65"]
    dev = torch.from_numpy(clip.copy()).cuda()[None]
    m = D.mirrored("noise_2x33x65", 8)
    stream, offsets, _, rects = ops.gif_encode(dev, 8, delta=True)
    assert offsets.tolist() == m["off"] and m["off"][-1] > stream.numel() and np.array_equal(rects.cpu().numpy(), m["rects"])
    assert stream.cpu().numpy().tobytes() == m["stream"][:stream.numel()]
    data, off, pals, rects = ops.gif_encode_to_host(dev, 8, delta=True)
    assert off == m["off"] and data == m["stream"] and np.array_equal(pals[0], m["pal"]) and np.array_equal(rects, m["rects"])


# ------------------------------------------------------------------ 5
def _pil_frames(path):
    from PIL import Image
    with Image.open(path) as im:
        out = []
        for t in range(getattr(im, "n_frames", 1)):
            im.seek(t)
            out.append(np.asarray(im.convert("RGB")).copy())
        return np.stack(out), im.info.get("duration"), im.info.get("loop")


def test_save_video_batch_and_write_u8_clips_delta(tmp_path):
    pytest.importorskip("PIL")
    from ccvs_amd.helpers.generator import save_video_batch, write_u8_clips
    from ccvs_amd.tools import gif
    vid = torch.rand(2, 1, 3, 24, 40, generator=torch.Generator().manual_seed(5)).repeat(1, 3, 1, 1, 1) * 2.4 - 1.2      # a static background
    vid[0, 1, :, 4:12, 6:30] = 0.5                                      # a patch appears, then moves
    vid[0, 2, :, 8:16, 10:34] = 0.5
    vid[1, 2, :, 20, 3] = -0.9                                          # clip 1: an identical frame, then one pixel
    d = tmp_path / "d"
    u8 = save_video_batch(vid.cuda(), 2, 3, str(d), 4, True, False, [-1, 1], "kinetics600", video_format="gif", delta=True)
    assert u8.shape == (2, 3, 24, 40, 3) and not u8.is_cuda
    names = [f"vid_{6 + i:05d}.gif" for i in range(2)]
    assert sorted(os.listdir(d)) == names
    for i, n in enumerate(names):
        data, shown, rects = D.clip_file(u8[i].numpy(), 4)
        assert (d / n).read_bytes() == data, i
        frames, duration, loop = _pil_frames(str(d / n))
        assert duration == 250 and loop == 0 and np.array_equal(frames, shown), i
        mine, info = gif.read_gif(str(d / n), with_info=True, delta=True)
        assert np.array_equal(mine, shown) and info["rects"] == [tuple(int(v) for v in r) for r in rects], i
        assert all(r != (0, 0, 40, 24) for r in info["rects"][1:]), (i, info["rects"])
        with pytest.raises(ValueError, match="transparency"):
            gif.read_gif(str(d / n))
    e = tmp_path / "e"                                                  # return_clip=False (what `save_results` asks for): the same files
    assert save_video_batch(vid.cuda(), 2, 3, str(e), 4, True, False, [-1, 1], "kinetics600", video_format="gif", return_clip=False, delta=True) is None
    assert all((e / n).read_bytes() == (d / n).read_bytes() for n in names)
    write_u8_clips(u8.cuda(), u8.cuda(), "cuda", 2, 3, str(tmp_path / "w"), 4, "gif", delta=True)
    assert all((tmp_path / "w" / n).read_bytes() == (d / n).read_bytes() for n in names)
    # without the flag: the full-frame files, as before
    save_video_batch(vid.cuda(), 2, 3, str(tmp_path / "f"), 4, True, False, [-1, 1], "kinetics600", video_format="gif")
    for i, n in enumerate(names):
        stream, off, pal, _, _ = G.encode(u8[i].numpy(), 0)
        assert (tmp_path / "f" / n).read_bytes() == G.gif_file([stream[off[k]:off[k + 1]] for k in range(3)], pal, 4, 24, 40), i
        assert len((d / n).read_bytes()) < len((tmp_path / "f" / n).read_bytes()), i


def test_without_the_flag_the_new_entries_are_never_reached(tmp_path, monkeypatch):
    """A call without `delta` launches and allocates what it did: with the three new C entries poisoned every format, gif among them,
    writes its files; with the flag the poison is met."""
    from ccvs_amd import lib
    from ccvs_amd.helpers.generator import save_video_batch

    def poisoned(*a, **k):
        raise AssertionError("the changed-rectangle stage was reached")
    L = lib.load()
    kept = L.ccvs_gif_palette_n, L.ccvs_gif_encode_delta, L.ccvs_gif_delta_workspace_bytes
    L.ccvs_gif_palette_n = L.ccvs_gif_encode_delta = L.ccvs_gif_delta_workspace_bytes = poisoned
    try:
        vid = torch.rand(2, 3, 3, 24, 40, generator=torch.Generator().manual_seed(6)) * 2 - 1
        for fmt, ext in ((None, None), ("npy", ".npy"), ("avi", ".avi"), ("apng", ".png"), ("gif", ".gif")):
            d = tmp_path / str(fmt)
            save_video_batch(vid.cuda(), 2, 0, str(d), 4, True, False, [-1, 1], "kinetics600", video_format=fmt)
            assert len(os.listdir(d)) == 2 and (ext is None or all(n.endswith(ext) for n in os.listdir(d)))
        for fmt in ("npy", "avi", "apng"):                              # the other formats do not look at the flag
            save_video_batch(vid.cuda(), 2, 0, str(tmp_path / ("d" + fmt)), 4, True, False, [-1, 1], "kinetics600", video_format=fmt, delta=True)
            for n in os.listdir(tmp_path / fmt):
                assert (tmp_path / ("d" + fmt) / n).read_bytes() == (tmp_path / fmt / n).read_bytes(), (fmt, n)
        with pytest.raises(AssertionError, match="changed-rectangle stage"):
            save_video_batch(vid.cuda(), 2, 0, str(tmp_path / "dgif"), 4, True, False, [-1, 1], "kinetics600", video_format="gif", delta=True)
    finally:
        L.ccvs_gif_palette_n, L.ccvs_gif_encode_delta, L.ccvs_gif_delta_workspace_bytes = kept


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


def test_run_writes_delta_files_pipelined_equals_serial_and_a_flow_clip_comes_back(tmp_path):
    pytest.importorskip("PIL")
    from ccvs_amd import ops
    from ccvs_amd.helpers.generator import write_u8_clips
    flags = ["--save_flow", "--video_format", "gif", "--video_delta"]
    runs = {tag: _run(tmp_path / tag, mode, extra) for tag, mode, extra in (
        ("delta", "pipelined", flags), ("serial", "serial", flags), ("npy", "pipelined", ["--video_format", "npy"]))}
    files = runs["delta"][1]
    assert files == runs["serial"][1]
    names = [f"vid_{i:05d}.gif" for i in range(4)]
    kinds = ["real", "fake", "rec"] + [f"{side}_{kind}" for side in ("fake", "rec") for kind in ("flow", "occ", "warp")]
    assert sorted(files) == sorted((kind, n) for kind in kinds for n in names)
    fps = None
    for kind in ("real", "fake", "rec"):                                # the mirror's files of the clips the `npy` format writes
        for name in names:
            clip = np.load(os.path.join(runs["npy"][0], kind, name[:-4] + ".npy"))
            frames, duration, loop = _pil_frames(os.path.join(runs["delta"][0], kind, name))
            fps = fps or round(1000 / duration)
            want, shown, _ = D.clip_file(clip, fps)
            assert frames.shape == (4, 32, 32, 3) and loop == 0 and np.array_equal(frames, shown), (kind, name)
            assert files[kind, name] == want, (kind, name)
    for kind in ("fake_flow", "fake_occ", "rec_warp"):
        frames, _, loop = _pil_frames(os.path.join(runs["delta"][0], kind, names[1]))
        assert frames.shape == (4, 32, 32, 3) and loop == 0
    # a flow field that is constant on 8 x 8 blocks and changes in one block per frame renders to few colours: the file holds the
    # rendered clip exactly, its later frames as rectangles
    rng = np.random.default_rng(12)
    order = np.tile(rng.permutation(48)[:16].reshape(1, 1, 4, 4), (1, 3, 1, 1))
    order[0, 1, 1, 2], order[0, 2, 3, 0] = 47 - order[0, 0, 1, 2], 47 - order[0, 0, 3, 0]
    order[0, 2, 1, 2] = order[0, 1, 1, 2]
    ang, mag = (order % 16 + 0.5) * (2 * np.pi / 16), np.array([1.0, 2.5, 4.0])[order // 16]
    coarse = np.stack([mag * np.cos(ang), mag * np.sin(ang), np.tile(rng.choice([0.0, 0.5, 1.0], (1, 1, 4, 4)), (1, 3, 1, 1))], 2)
    motion = torch.from_numpy(np.kron(coarse, np.ones((8, 8)))).float().cuda()
    for k, u8 in enumerate(ops.flow_render(motion, torch.full((1,), 4.0, device="cuda"))):
        clip = u8[0].cpu().numpy()
        cnt, _ = G.histogram(clip)
        colours = np.unique(clip.reshape(-1, 3), axis=0)
        assert len(colours) <= 255 and len(colours) == np.count_nonzero(cnt), (k, len(colours), np.count_nonzero(cnt))
        write_u8_clips(u8, u8, u8.device, 1, k, str(tmp_path / "few"), 10, "gif", delta=True)
        path = str(tmp_path / "few" / f"vid_{k:05d}.gif")
        frames, _, _ = _pil_frames(path)
        assert np.array_equal(frames, clip), k
        assert open(path, "rb").read() == D.clip_file(clip, 10)[0], k

"""not gpu: the changed-rectangle GIF frames' specification (tests/gif_delta_ref.py) against independent decoders,
and the host side of the feature.

  1. every file the mirror writes is decoded by Pillow to exactly palette[indices], frame by frame, with the frame count, size, loop flag
     and delays; `tools.gif.read_gif(delta=True)` agrees, `read_gif()` still refuses the file, and `write_gif(rects=...)` writes the
     mirror's bytes.  Cases: the clip table of `gif_ref.clips()` at band_rows 0, 1, 3 and h; five identical frames (every later payload
     the 7 bytes 08 04 00 ff 05 04 00); one changed pixel at each corner; changes in the first / last row / column alone; a rectangle
     1 pixel wide and one 1 pixel high; every pixel changed (D ties with F: F is written); noise with scattered unchanged pixels (D is
     the larger: F is written); two clips in one batch whose boundary frames match (clip 1's frame 0 stays full); a 7 x 150 rectangle
     (1050 indices in a band, across the coder's 1024-index chunk); a 64 x 64 rectangle in a frame 100 wide (a band of 4096 indices,
     more than any full-frame band); 255 distinct-bin colours stored exactly; more than 300 occupied bins (used == 255, index 255
     only ever transparent);
  2. per frame the written payload has min(len(F), len(D)) bytes and never more than `ccvs_gif_stream_bound` allows;
  3. the container field by field;
  4. `max_colours` 2, 16, 255 and 256 on the hand-made histograms of the palette tests; 256 is `gif_ref.palette`;
  5. the symbols are declared, listed, in the library and compile as C; sizes and refusals before any launch;
  6. `--video_delta` parses and moves no default; `save_results` passes it on; CPU tensors are refused; other formats ignore it;
  7. ccvs_amd/csrc/gif_core.h on the host, outside python: tests/gif_delta_core_check.cpp, a program of its own, built with
     -fsanitize=address,undefined and run as a child process, gives the mirror's bytes and rectangles in buffers of the library's sizes;
  8. recorded, no bar: whole-file size, delta over full, on a static-background clip without and with pixel noise, on uniform noise and
     on identical frames.
"""
import ctypes
import io
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import gif_delta_ref as D  # noqa: E402
import gif_ref as G  # noqa: E402
from tests.test_mjpeg_host import TINY  # noqa: E402


def pil_decode(data):
    Image = pytest.importorskip("PIL.Image")                            # (only the tests that decode with Pillow skip without it)
    with Image.open(io.BytesIO(data)) as im:
        frames, delays = [], []
        for t in range(getattr(im, "n_frames", 1)):
            im.seek(t)
            frames.append(np.asarray(im.convert("RGB")).copy())
            delays.append(im.info.get("duration"))
        return np.stack(frames), delays, im.info.get("loop"), im.size


def check_clip(idx, pal, stream, off, rects, tmp_path, tag, fps=10):
    """One clip's mirror file (index frames [t, H, W], its part of the stream) through Pillow, `read_gif(delta=True)` and `write_gif`."""
    from ccvs_amd.tools import gif
    t, h, w = idx.shape
    payloads = [stream[off[i]:off[i + 1]] for i in range(t)]
    data = D.gif_file(payloads, rects, pal, fps, h, w)
    want = np.asarray(pal)[idx]
    frames, delays, loop, size = pil_decode(data)
    assert frames.shape == want.shape and size == (w, h) and loop == 0, tag
    assert delays == [10 * G.delay_cs(fps)] * t, (tag, delays)
    assert np.array_equal(frames, want), tag
    path = tmp_path / "f.gif"
    gif.write_gif(str(path), payloads, pal, fps, h, w, rects=rects)
    assert path.read_bytes() == data, tag
    mine, info = gif.read_gif(str(path), with_info=True, delta=True)
    assert np.array_equal(mine, want) and info["loop"] == 0 and info["delays"] == [G.delay_cs(fps)] * t, tag
    assert info["rects"] == [tuple(int(v) for v in r) for r in rects] and info["disposals"] == [1] * t, tag
    assert info["transparent"] == [None] + [255] * (t - 1), tag
    if t > 1:                                                           # the plain reader still refuses such files
        with pytest.raises(ValueError, match="transparency"):
            gif.read_gif(str(path))
    return data


def check_index_case(name, band_rows, tmp_path):
    colours, _ = D.direct_colours()
    pal = np.concatenate([colours, np.zeros((1, 3), np.uint8)])
    m = D.mirrored_indices(name, band_rows)
    idx, t = m["idx"], m["t"]
    n, h, w = idx.shape
    assert m["off"][-1] <= G.stream_bound(n, h, w, band_rows), name
    for f in range(n):                                                   # 2: the shorter candidate, the full frame where they tie
        size = m["off"][f + 1] - m["off"][f]
        assert size == (m["fsize"][f] if m["dsize"][f] is None else min(m["fsize"][f], m["dsize"][f])), (name, f)
        is_d = m["dsize"][f] is not None and m["dsize"][f] < m["fsize"][f]
        assert is_d or tuple(m["rects"][f]) == (0, 0, w, h), (name, f)
        assert size <= G.stream_bound(1, h, w, band_rows), (name, f)
    for c in range(n // t):
        off = [v - m["off"][c * t] for v in m["off"][c * t:(c + 1) * t + 1]]
        check_clip(idx[c * t:(c + 1) * t], pal, m["stream"][m["off"][c * t]:m["off"][(c + 1) * t]], off, m["rects"][c * t:(c + 1) * t], tmp_path,
                   (name, band_rows, c))
    return m


# ------------------------------------------------------------------ 1, 2
def test_clip_table_decodes_to_palette_of_indices(tmp_path):
    for name, r in G.rows():
        m = D.mirrored(name, r)
        assert m["used"] <= 255 and m["idx"].max() < 255 and not m["pal"][255].any(), name
        check_clip(m["idx"], m["pal"], m["stream"], m["off"], m["rects"], tmp_path, (name, r), fps=4)
    print("rows", len(G.rows()))


def test_index_cases_decode_and_take_the_shorter_candidate(tmp_path):
    for name, r in D.index_rows():
        check_index_case(name, r, tmp_path)
    print("rows", len(D.index_rows()))


def test_identical_frames_are_seven_bytes_each():
    for r in (0, 1, 3, 40):
        m = D.mirrored_indices("identical_5x40x56", r)
        for f in range(1, 5):
            assert m["stream"][m["off"][f]:m["off"][f + 1]] == D.NOTHING == bytes.fromhex("080400ff050400"), (r, f)
            assert tuple(m["rects"][f]) == (0, 0, 1, 1), (r, f)
        assert tuple(m["rects"][0]) == (0, 0, 56, 40)


def test_rectangles_of_the_edge_cases():
    rects = lambda name: [tuple(int(v) for v in r) for r in D.mirrored_indices(name, 0)["rects"]]
    assert rects("corners_5x24x40") == [(0, 0, 40, 24), (0, 0, 1, 1), (39, 0, 1, 1), (0, 23, 1, 1), (39, 23, 1, 1)]
    assert rects("edges_5x24x40") == [(0, 0, 40, 24), (0, 0, 40, 1), (0, 23, 40, 1), (0, 0, 1, 24), (39, 0, 1, 24)]
    assert rects("thin_3x24x40") == [(0, 0, 40, 24), (17, 3, 1, 17), (5, 11, 28, 1)]
    assert rects("chunk_2x160x9") == [(0, 0, 9, 160), (1, 5, 7, 150)] and G.bands(150, 7, 0) == 1 and 7 * 150 > 1024 and 1024 % 7
    assert rects("big_band_2x64x100") == [(0, 0, 100, 64), (18, 0, 64, 64)] and G.bands(64, 64, 0) == 1 and G.band_rows_of(100, 0) * 100 == 4000
    m = D.mirrored_indices("all_changed_3x17x23", 0)                   # the whole frame changed: D is F's bytes, a tie, F is written
    assert m["dsize"][1:] == m["fsize"][1:] and rects("all_changed_3x17x23") == [(0, 0, 23, 17)] * 3
    m = D.mirrored_indices("noise_kept_3x33x65", 0)                    # D is the larger
    assert all(d > f for d, f in zip(m["dsize"][1:], m["fsize"][1:])) and rects("noise_kept_3x33x65") == [(0, 0, 65, 33)] * 3
    m = D.mirrored_indices("two_clips_6x20x30", 0)                     # clip 1's frame 0 equals clip 0's last: still full
    assert np.array_equal(m["idx"][3], m["idx"][2]) and tuple(m["rects"][3]) == (0, 0, 30, 20) and m["dsize"][3] is None
    assert all(tuple(m["rects"][f]) != (0, 0, 30, 20) for f in (1, 2, 4, 5))
    # a rectangle's bands are never more than its frame's
    for w in (1, 7, 63, 64, 100, 4095, 4096, 4097, 5000):
        for rw in {1, 2, w // 3 + 1, w - 1 or 1, w}:
            for h in (1, 5, 64, 700):
                assert G.bands(h, rw, 0) <= G.bands(h, w, 0), (h, w, rw)


def test_255_colours_are_stored_exactly_and_256_are_not(tmp_path):
    clip = D.colours_255()
    pal, table, used = D.palette_n(clip)
    assert used == 255 and np.array_equal(pal[G.indices(clip, table)], clip) and not pal[255].any() and table.max() == 254
    data, shown, rects = D.clip_file(clip, 8)
    frames, _, _, _ = pil_decode(data)
    assert np.array_equal(frames, clip) and np.array_equal(shown, clip)
    assert [tuple(int(v) for v in r) for r in rects] == [(0, 0, 40, 24), (8, 5, 22, 7), (3, 20, 1, 1)]
    colours, _ = G.direct_colours()                                    # 256 colours in 256 bins: exact at 256, no longer at 255
    clip = colours[np.arange(512).reshape(1, 16, 32) % 256]
    pal, table, used = D.palette_n(clip, 256)
    assert used == 256 and np.array_equal(pal[G.indices(clip, table)], clip)
    pal, table, used = D.palette_n(clip, 255)
    assert used == 255 and not np.array_equal(pal[G.indices(clip, table)], clip)


def test_many_bins_use_255_entries_and_255_is_only_ever_transparent(tmp_path):
    clip = D.many_bins_clip()
    cnt, _ = G.histogram(clip)
    assert np.count_nonzero(cnt) >= 300
    stream, off, pal, table, used, rects = D.encode(clip, 0)
    idx = G.indices(clip, table)
    assert used == 255 and idx.max() == 254 and table.max() == 254 and not pal[255].any()
    check_clip(idx, pal, stream, [int(v) for v in off], rects, tmp_path, "many bins")
    assert all(tuple(r) != (0, 0, 48, 32) for r in rects[1:])        # the moving patch alone is written
    from ccvs_amd.tools import gif                                     # ... and decoded: index 255 inside the rectangles, nowhere in frame 0
    seen = 0
    for f in range(4):
        body, _ = gif._sub_blocks(stream[off[f]:off[f + 1]], 1, "frame")
        part = gif.lzw_decode(body, 8, int(rects[f][2]) * int(rects[f][3]))
        seen += int((part == 255).sum())
        assert f or not (part == 255).any()
    assert seen > 0


# ------------------------------------------------------------------ 3
def test_container_field_by_field(tmp_path):
    from ccvs_amd.tools import gif
    m = D.mirrored_indices("two_clips_6x20x30", 3)
    colours, _ = D.direct_colours()
    pal = np.concatenate([colours, np.zeros((1, 3), np.uint8)])
    payloads = [m["stream"][m["off"][i]:m["off"][i + 1]] for i in range(3)]
    rects = m["rects"][:3]
    for fps, delay in ((1, 100), (4, 25), (50, 2), (100, 2)):
        path = tmp_path / f"{fps}.gif"
        gif.write_gif(str(path), payloads, pal, fps, 20, 30, rects=rects)
        data = path.read_bytes()
        assert data == D.gif_file(payloads, rects, pal, fps, 20, 30)
        assert data[:6] == b"GIF89a" and struct.unpack("<HH", data[6:10]) == (30, 20) and data[10] == 0xF7 and data[11:13] == b"\x00\x00"
        assert data[13:781] == pal.tobytes() and data[778:781] == b"\x00\x00\x00"
        assert data[781:800] == b"\x21\xFF\x0BNETSCAPE2.0\x03\x01\x00\x00\x00"
        pos = 800
        for k, (p, r) in enumerate(zip(payloads, rects)):
            packed = 0x05 if k else 0x04                                 # disposal 1; the transparent-colour flag behind frame 0
            assert data[pos:pos + 8] == b"\x21\xF9\x04" + bytes([packed]) + struct.pack("<H", delay) + b"\xFF\x00", k
            assert data[pos + 8:pos + 18] == b"\x2C" + struct.pack("<HHHHB", *(int(v) for v in r), 0), k
            assert data[pos + 18:pos + 18 + len(p)] == p and p[0] == 8 and p[-1] == 0
            pos += 18 + len(p)
        assert data[pos:] == b"\x3B"
    # without rects the bytes are the full-frame writer's
    full, off = G.encode_indices(m["idx"][:3], 3)
    gif.write_gif(str(tmp_path / "n.gif"), [full[off[i]:off[i + 1]] for i in range(3)], pal, 4, 20, 30)
    gif.write_gif(str(tmp_path / "m.gif"), [full[off[i]:off[i + 1]] for i in range(3)], pal, 4, 20, 30, rects=None)
    assert (tmp_path / "n.gif").read_bytes() == (tmp_path / "m.gif").read_bytes() == G.gif_file([full[off[i]:off[i + 1]] for i in range(3)], pal, 4, 20, 30)
    for bad in ([(0, 0, 30, 20)] * 2, [(0, 0, 30, 19)] + [(0, 0, 1, 1)] * 2, [(0, 0, 30, 20), (29, 0, 2, 1), (0, 0, 1, 1)], [(0, 0, 30, 20), (0, 0, 0, 1), (0, 0, 1, 1)]):
        with pytest.raises(ValueError, match="write_gif"):
            gif.write_gif(str(tmp_path / "bad.gif"), payloads, pal, 4, 20, 30, rects=bad)
    # the reader: disposal 2 and 3 are refused, a partial first frame too; the default refuses transparency and partial frames
    good = (tmp_path / "4.gif").read_bytes()
    second = 800 + 18 + len(payloads[0])
    assert good[second + 3] == 0x05
    for data, word, delta in ((good[:second + 3] + b"\x09" + good[second + 4:], "disposal", True), (good[:second + 3] + b"\x0D" + good[second + 4:], "disposal", True),
                              (good[:813] + b"\x13" + good[814:], "partial frame", True), (good, "transparency", False),
                              (good[:second + 3] + b"\x04" + good[second + 4:], "partial frame", False)):
        (tmp_path / "r.gif").write_bytes(data)
        with pytest.raises(ValueError, match=word):
            gif.read_gif(str(tmp_path / "r.gif"), delta=delta)


# ------------------------------------------------------------------ 4
def test_max_colours_on_hand_made_histograms():
    for k, bins in enumerate(D.HAND):
        clip = G.clip_of_bins(bins)
        full = G.palette(clip)
        for cap in (2, 16, 255, 256):
            pal, table, used = D.palette_n(clip, cap)
            assert used == min(cap, len(bins)) and not pal[used:].any() and table.max() < used, (k, cap)
            if cap == 256 or len(bins) <= cap:                           # the cap is not reached: `gif_ref.palette`
                assert used == full[2] and np.array_equal(pal, full[0]) and np.array_equal(table, full[1]), (k, cap)
    # the boxes made before the cap are the uncapped run's first ones: 4 bins, cap 2 -> the first split alone
    occ, box, n = D.median_cut_n(G.histogram(G.clip_of_bins(D.HAND[2]))[0], 2)
    assert n == 2 and box.tolist() == [0, 0, 1, 1]
    for name in ("noise_2x33x65", "smooth_5x64x96"):
        clip = G.clips()[name]
        want = G.clip_palette(name)
        got = D.palette_n(clip, 256)
        assert got[2] == want[2] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
        pal, table, used = D.palette_n(clip, 255)
        assert used == 255 and table.max() == 254 and not pal[255].any(), name


# ------------------------------------------------------------------ 5
def test_delta_symbols_declared_and_exported(tmp_path):
    from ccvs_amd import lib
    header = open(os.path.join(ROOT, "include", "ccvs_hip_output_gif_delta.h")).read()
    assert re.search(r'^#include "ccvs_hip_output_gif_delta.h"', open(os.path.join(ROOT, "include", "ccvs_hip.h")).read(), re.M)
    declared = sorted(set(re.findall(r"^\w[\w \*]*?\b(ccvs_\w+)\(", header, re.M)))
    assert declared == sorted(lib.GIF_DELTA_SYMBOLS) == ["ccvs_gif_delta_workspace_bytes", "ccvs_gif_encode_delta", "ccvs_gif_palette_n"]
    others = [getattr(lib, n) for n in dir(lib) if n.endswith("EXPORTS") or (n.endswith("SYMBOLS") and n != "GIF_DELTA_SYMBOLS")]
    assert not any(set(lib.GIF_DELTA_SYMBOLS) & set(o) for o in others) and len(lib.EXPORTS) == 51
    handle = ctypes.CDLL(lib.LIB_PATH)
    for sym in lib.GIF_DELTA_SYMBOLS:
        assert hasattr(handle, sym), sym
    c = tmp_path / "p.c"
    c.write_text('#include "ccvs_hip.h"\nvoid* p[] = {' + ", ".join("(void*)" + s for s in lib.GIF_DELTA_SYMBOLS) + "};\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "p.o")], check=True)
    assert lib.load().ccvs_abi_version() == 6


def test_sizes_and_refusals_before_any_launch():
    from ccvs_amd import lib
    L = lib.load()
    ws, full_ws = L.ccvs_gif_delta_workspace_bytes, L.ccvs_gif_workspace_bytes
    for h, w in ((33, 65), (1, 5000), (64, 96), (7, 1), (1, 1), (64, 100), (160, 9)):
        for r in sorted({0, 1, 3, h}):
            nb = G.bands(h, w, r)
            # the bins, both candidates' band positions, and both candidates' words at the largest band a rectangle can have
            biggest = min(r, h) * w if r else (w if w > 4096 else min(4096, h * w))
            words = (12 * (biggest + biggest // 3838 + 2) + 31) // 32 + 1
            assert ws(2, 3, h, w, r) >= 2 * (1 << 20) + 6 * 2 * 8 * (nb + 1) + 6 * 2 * nb * words * 4, (h, w, r)
            assert ws(2, 3, h, w, r) > full_ws(2, 3, h, w, r), (h, w, r)
    for args in ((0, 8, 8, 0), (1, 0, 8, 0), (1, 8, 0, 0), (1, 65536, 8, 0), (1, 8, 65536, 0), (1, 8, 8, -1), (1, 65535, 65535, 65535), (1 << 24, 8, 8, 0)):
        assert ws(1, *args) == 0, args
    assert ws(0, 1, 8, 8, 0) == 0 and ws(1, 0, 8, 8, 0) == 0
    one = ctypes.c_void_p(16)

    def encode(b=1, t=2, h=8, w=8, r=0, cap=64, cs=384, fs=192):
        return L.ccvs_gif_encode_delta(one, cs, fs, b, t, h, w, r, one, one, cap, one, one, one, None)

    def palette(b=1, t=2, h=8, w=8, cs=384, fs=192, cap=255):
        return L.ccvs_gif_palette_n(one, cs, fs, b, t, h, w, cap, one, one, one, one, None)

    for kw, word in ((dict(b=0), "clips"), (dict(t=0), "clips"), (dict(b=1 << 12, t=1 << 12), "clips"), (dict(h=0), "size"), (dict(w=65536), "size"),
                     (dict(fs=191), "frame stride"), (dict(cs=383), "clip stride"), (dict(fs=-192), "frame stride")):
        for call, who in ((encode, "ccvs_gif_encode_delta"), (palette, "ccvs_gif_palette_n")):
            assert call(**kw) != 0, kw
            msg = L.ccvs_last_error().decode()
            assert word in msg and who in msg, (kw, msg)
    for kw, word in ((dict(r=-1), "band_rows"), (dict(cap=-1), "capacity"), (dict(h=65535, w=65535, r=65535, fs=1 << 40, cs=1 << 42), "band_rows")):
        assert encode(**kw) != 0 and word in L.ccvs_last_error().decode(), kw
    for cap in (1, 0, -3, 257):
        assert palette(cap=cap) != 0 and "max_colours" in L.ccvs_last_error().decode(), cap
    for k in (0, 8, 9, 11, 12, 13):                                     # clips, table, stream (with a capacity), offsets, rects, workspace
        argv = [one, 384, 192, 1, 2, 8, 8, 0, one, one, 64, one, one, one, None]
        argv[k] = None
        assert L.ccvs_gif_encode_delta(*argv) != 0 and "null" in L.ccvs_last_error().decode(), k
    for k in (0, 8, 9, 10, 11):
        argv = [one, 384, 192, 1, 2, 8, 8, 255, one, one, one, one, None]
        argv[k] = None
        assert L.ccvs_gif_palette_n(*argv) != 0 and "null" in L.ccvs_last_error().decode(), k


# ------------------------------------------------------------------ 6
def test_option_parses_and_moves_no_default():
    from ccvs_amd.tools.options import Options
    plain = Options().parse(True, True, argv=TINY)
    assert plain["transformer"].video_delta is False and plain["base"].video_delta is False
    for argv, want in ((["--video_delta"], True), (["--video_delta", "true"], True), (["--video_delta", "false"], False)):
        on = Options().parse(True, True, argv=TINY + ["--video_format", "gif"] + argv)
        assert on["transformer"].video_delta is want and on["base"].video_delta is want and on["transformer"].video_format == "gif"
    for fmt in ("auto", "npy", "avi", "apng"):
        assert Options().parse(True, True, argv=TINY + ["--video_format", fmt, "--video_delta"])["base"].video_format == fmt
    on = Options().parse(True, True, argv=TINY + ["--video_delta"])
    for key in ("transformer", "qvid_generator"):
        a, b = vars(plain[key]), vars(on[key])
        skip = lambda k: k in ("video_delta", "signature") or k.endswith("_path")
        assert {k: v for k, v in a.items() if not skip(k)} == {k: v for k, v in b.items() if not skip(k)}, key


def test_save_results_passes_delta_through(tmp_path, monkeypatch):
    import types
    from ccvs_amd.helpers import generator as Gn
    seen = []
    monkeypatch.setattr(Gn, "save_video_batch", lambda *a, **k: seen.append((os.path.basename(a[3]), k["video_format"], k.get("delta", False))))
    opt = types.SimpleNamespace(video_format="gif", video_quality=80, video_subsampling="420", video_optimize=False, video_lz77=False, video_delta=True,
                                result_path=str(tmp_path), fps=4, imagenet_norm=False, dataset="bairhd", state=True)
    me = types.SimpleNamespace(opt=opt, decode_stft=False)
    vid = torch.zeros(2, 2, 3, 8, 8)
    out = {"real": vid, "fake": {"vid": vid, "state": torch.zeros(2, 2, 2)}, "rec": {"vid": vid}, "blur": vid}
    Gn.Generator.save_results(me, out, 0)
    assert seen == [(k, "gif", True) for k in ("real", "fake", "fake_state", "rec", "blur")]
    for change in (lambda: setattr(opt, "video_delta", False), lambda: delattr(opt, "video_delta")):     # off; an options object from before the flag
        change()
        seen.clear()
        Gn.Generator.save_results(me, out, 0)
        assert seen == [(k, "gif", False) for k in ("real", "fake", "fake_state", "rec", "blur")]


def test_cpu_tensors_are_refused_and_other_formats_ignore_the_flag(tmp_path):
    from ccvs_amd import lib, ops
    from ccvs_amd.helpers.generator import save_video_batch
    clips = torch.zeros(1, 2, 8, 8, 3, dtype=torch.uint8)
    for fn in (lambda: ops.gif_palette(clips, 255), lambda: ops.gif_encode(clips, delta=True), lambda: ops.gif_encode_to_host(clips, delta=True)):
        with pytest.raises(lib.CcvsError):
            fn()
    with pytest.raises(lib.CcvsError):
        save_video_batch(torch.zeros(1, 2, 3, 8, 8), 1, 0, str(tmp_path / "a"), 4, True, False, [-1, 1], "bairhd", video_format="gif", delta=True)
    vid = torch.rand(1, 2, 3, 8, 8, generator=torch.Generator().manual_seed(1))
    a = save_video_batch(vid, 1, 0, str(tmp_path / "n"), 4, False, False, [-1, 1], "bairhd", video_format="npy", delta=True)
    b = save_video_batch(vid, 1, 0, str(tmp_path / "m"), 4, False, False, [-1, 1], "bairhd", video_format="npy")
    assert torch.equal(a, b) and (tmp_path / "n" / "vid_00000.npy").read_bytes() == (tmp_path / "m" / "vid_00000.npy").read_bytes()


# ------------------------------------------------------------------ 7
def _case(idx, t, band_rows, chunk):
    idx = np.ascontiguousarray(idx, np.uint8)
    stream, off, rects, _, _ = D.encode_indices(idx, band_rows, t)
    n, h, w = idx.shape
    return np.array([n, t, h, w, band_rows, chunk, len(stream)], np.int64).tobytes() + idx.tobytes() + np.ascontiguousarray(rects, np.int32).tobytes() + stream


def test_core_on_the_host_under_sanitizers(tmp_path):
    cases = []
    for name, r in D.index_rows():
        idx, t = D.index_cases()[name]
        cases.append(_case(idx, t, r, 1024))
    for name, chunk in (("chunk_2x160x9", 7), ("chunk_2x160x9", 1000), ("big_band_2x64x100", 4096), ("thin_3x24x40", 1), ("two_clips_6x20x30", 5)):
        idx, t = D.index_cases()[name]
        cases.append(_case(idx, t, 0, chunk))
    for name, r in G.rows():
        cases.append(_case(D.mirrored(name, r)["idx"], len(G.clips()[name]), r, 1024))
    cases.append(_case(G.indices(D.many_bins_clip(), D.palette_n(D.many_bins_clip())[1]), 4, 0, 1024))
    rng = np.random.default_rng(13)
    wide = rng.integers(0, 255, (2, 2, 5000)).astype(np.uint8)         # a frame wider than 4096: bands of one row; a rectangle of two rows in one band
    wide[1, :, 900:] = wide[0, :, 900:]
    cases.append(_case(wide, 2, 0, 1024))
    exe = str(tmp_path / "gif_delta_core_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-I", os.path.join(ROOT, "ccvs_amd", "csrc"), os.path.join(HERE, "gif_delta_core_check.cpp"), "-o", exe], check=True)
    (tmp_path / "cases.bin").write_bytes(b"".join(cases))
    run = subprocess.run([exe, str(tmp_path / "cases.bin")], capture_output=True, text=True)
    print(run.stdout, run.stderr[-4000:])
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    assert run.stdout.split() == ["cases", str(len(cases)), "wrong", "0"]


# ------------------------------------------------------------------ 8
def _file_sizes(clip):
    t, h, w = clip.shape[:3]
    full = G.encode(clip, 0)
    delta = D.encode(clip, 0)
    a = len(G.gif_file([full[0][full[1][i]:full[1][i + 1]] for i in range(t)], full[2], 10, h, w))
    b = len(D.gif_file([delta[0][delta[1][i]:delta[1][i + 1]] for i in range(t)], delta[5], delta[2], 10, h, w))
    written = sum(tuple(r) != (0, 0, w, h) for r in delta[5][1:])
    return a, b, written


def test_recorded_file_sizes():
    """Recorded, no bar: the whole file with changed rectangles over the full-frame file of the same clip (each with its own palette: 255
    and 256 colours), and how many of the later frames are written as rectangles."""
    rng = np.random.default_rng(3)
    base = G.clips()["smooth_3x23x17"]
    clips = {"static background, moving patch 8x64x96": D.prototype_clip(), "the same, pixel noise sigma 1": D.prototype_clip(1.0),
             "the same, pixel noise sigma 4": D.prototype_clip(4.0), "uniform noise 3x33x65": rng.integers(0, 256, (3, 33, 65, 3)).astype(np.uint8),
             "5 identical frames 40x56": np.stack([np.resize(base[0], (40, 56, 3))] * 5)}
    for name, clip in clips.items():
        full, delta, written = _file_sizes(clip)
        print(f"{name}: delta / full = {delta / full:.2f} ({delta} / {full} bytes), {written} of {len(clip) - 1} later frames as rectangles")
        assert 0 < delta < 2 * full                                     # (a sanity bracket, not a bar)

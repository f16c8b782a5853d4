"""not gpu: the GIF output stage's specification (tests/gif_ref.py) against independent decoders, and the host
side of the feature.

  1. every file the mirror writes is decoded by Pillow to exactly palette[indices], frame by frame, with the frame count, size, loop flag
     and delay; `tools.gif.read_gif` agrees with Pillow.  Cases: the clip table (1 .. 5 frames, 1 x 1 .. 96 x 64; smooth, noise, flat,
     two-colour) at band_rows 0, 1, 3 and h; 1-pixel-wide frames whose first band takes every length in 250 .. 262, 506 .. 519,
     760 .. 774, 1784 .. 1797 and 3830 .. 3847 (band ends at every change of the code width and at the full table) on noise, flat and
     two-valued indices with a band behind it; one band of more than 4096 noise indices (the clear in mid-band); frames whose data is
     exactly 254, 255, 256 and 510 bytes (the sub-block edges);
  2. the palette rules on hand-made histograms: ties in box choice, axis and cut, a median that falls on hi, fewer than 256 occupied
     bins, a single colour; a clip of 200 colours in distinct bins is stored exactly;
  3. the container field by field at 1, 4, 25, 50 and 100 frames per second (the last two: the max(2, ...) rule);
  4. `ccvs_gif_stream_bound` equals the mirror's and covers the mirror's streams of all-noise frames at each band setting; sizes and
     refusals before any launch; the exports are declared, listed and in the library;
  5. `ops.gif_*` and `save_video_batch(video_format="gif")` refuse CPU tensors, "mp4" still raises ValueError; the option parses and
     every other default is unchanged;
  6. ccvs_amd/csrc/gif_core.h on the host, outside python: tests/gif_core_check.cpp, a program of its own, built with
     -fsanitize=address,undefined and run as a child process, gives the mirror's bytes on the band cases;
  7. recorded, no bar: file size against Pillow's own GIF of the same index frames and palette, quantisation PSNR beside Pillow's.
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
import gif_ref as G  # noqa: E402
from tests.test_mjpeg_host import TINY  # noqa: E402

Image = pytest.importorskip("PIL.Image")


def pil_decode(data):
    with Image.open(io.BytesIO(data)) as im:
        frames, delays = [], []
        for t in range(getattr(im, "n_frames", 1)):
            im.seek(t)
            frames.append(np.asarray(im.convert("RGB")).copy())
            delays.append(im.info.get("duration"))
        return np.stack(frames), delays, im.info.get("loop"), im.size


def check_file(idx, pal, band_rows, tmp_path, tag, fps=10):
    """The mirror's file of index frames [n, H, W] through Pillow and `read_gif`: both give pal[idx]."""
    from ccvs_amd.tools import gif
    idx = np.asarray(idx)
    n, h, w = idx.shape
    stream, off = G.encode_indices(idx, band_rows)
    assert off[-1] <= G.stream_bound(n, h, w, band_rows), tag
    data = G.gif_file([stream[off[i]:off[i + 1]] for i in range(n)], pal, fps, h, w)
    want = np.asarray(pal)[idx]
    frames, delays, loop, size = pil_decode(data)
    assert frames.shape == want.shape and size == (w, h) and loop == 0, tag
    assert delays == [10 * G.delay_cs(fps)] * n, (tag, delays)
    assert np.array_equal(frames, want), tag
    path = tmp_path / "f.gif"
    path.write_bytes(data)
    mine, info = gif.read_gif(str(path), with_info=True)
    assert np.array_equal(mine, want) and info["loop"] == 0 and info["delays"] == [G.delay_cs(fps)] * n, tag
    return data


def noise_palette():
    pal = np.random.default_rng(3).permutation(1 << 24)[:256]
    return np.stack([pal >> 16, (pal >> 8) & 255, pal & 255], 1).astype(np.uint8)         # 256 different colours


# ------------------------------------------------------------------ 1
def test_clip_table_decodes_to_palette_of_indices(tmp_path):
    from ccvs_amd.tools import gif
    for name, r in G.rows():
        m = G.mirrored(name, r)
        clip = G.clips()[name]
        t, h, w = clip.shape[:3]
        data = check_file(m["idx"], m["pal"], r, tmp_path, (name, r), fps=4)
        path = tmp_path / "w.gif"                                       # the writer gives the mirror's file
        gif.write_gif(str(path), [m["stream"][m["off"][i]:m["off"][i + 1]] for i in range(t)], m["pal"], 4, h, w)
        assert path.read_bytes() == data, (name, r)
    print("rows", len(G.rows()))


def test_band_ends_at_every_width_change_and_the_full_table(tmp_path):
    pal = noise_palette()
    assert len(G.BAND_SWEEP) == 74
    for L in G.BAND_SWEEP:
        for kind in ("noise", "flat", "two"):
            idx = G.sweep_indices(L, kind)
            assert G.bands(idx.shape[0], 1, L) == 2
            check_file(idx[None], pal, L, tmp_path, (L, kind))
    # the widths the noise bands end with cover 10, 11 and 12 bits, and the longest ones reset the dictionary
    ends = {L: G.lzw_band(G.sweep_indices(L, "noise")[:L], True, False) for L in G.BAND_SWEEP}
    assert {p[-1][1] for p in ends.values()} >= {9, 10, 11, 12}
    assert any(sum(c == G.CLEAR for c, _ in p) == 3 for p in ends.values())      # leading, table full, band end


def test_clear_in_mid_band_and_sub_block_edges(tmp_path):
    pal = noise_palette()
    rng = np.random.default_rng(11)
    for shape, r in (((1, 1, 5000), 0), ((1, 1, 5000), 1), ((2, 50, 100), 50), ((1, 3, 4100), 3)):
        idx = rng.integers(0, 256, shape).astype(np.uint8)
        pairs = G.frame_pairs(idx[0], r)
        assert sum(c == G.CLEAR for c, _ in pairs) >= 2, shape           # the leading one and the full table's
        check_file(idx, pal, r, tmp_path, (shape, r))
    for target in (254, 255, 256, 510):
        idx = G.edge_frame(target)
        data = G.frame_data(idx, 0)
        assert len(data) == target and len(G.payload(data)) == 2 + target + -(-target // 255)
        check_file(idx[None], pal, 0, tmp_path, ("edge", target))


# ------------------------------------------------------------------ 2
def _boxes(bins):
    cnt, _ = G.histogram(G.clip_of_bins(bins))
    occ, box, nbox = G.median_cut(cnt)
    return {(int(b) >> 10, (int(b) >> 5) & 31, int(b) & 31): int(k) for b, k in zip(occ, box)}, nbox


def test_palette_rules_on_hand_made_histograms():
    # the axis: R and G tie -> G; R and B tie -> R
    boxes, n = _boxes([(0, 2, 0, 1), (2, 0, 0, 1), (1, 1, 0, 2)])
    assert n == 3 and boxes[0, 2, 0] == 1 and boxes[2, 0, 0] == 0       # first split along G: g <= 1 stays
    boxes, n = _boxes([(0, 0, 2, 1), (2, 0, 0, 1), (1, 0, 1, 2)])
    assert n == 3 and boxes[2, 0, 0] == 1 and boxes[0, 0, 2] == 0       # first split along R: r <= 1 stays
    # the box: two boxes of the same score -> the lower one is split first
    boxes, n = _boxes([(0, 0, 0, 1), (1, 0, 0, 1), (10, 0, 0, 1), (11, 0, 0, 1)])
    assert n == 4 and boxes == {(0, 0, 0): 0, (1, 0, 0): 2, (10, 0, 0): 1, (11, 0, 0): 3}
    # ... and the larger population x extent first
    boxes, n = _boxes([(0, 0, 0, 1), (1, 0, 0, 1), (10, 0, 0, 1), (12, 0, 0, 1)])
    assert boxes == {(0, 0, 0): 0, (1, 0, 0): 3, (10, 0, 0): 1, (12, 0, 0): 2}
    # the cut: the smallest c with P(c) >= ceil(total / 2)
    boxes, n = _boxes([(0, 0, 0, 2), (2, 0, 0, 2), (4, 0, 0, 4)])
    assert boxes[4, 0, 0] == 1 and boxes[2, 0, 0] != 1
    boxes, n = _boxes([(0, 0, 0, 2), (2, 0, 0, 1), (4, 0, 0, 4)])           # total 7, half 4: P(2) = 3 < 4, so the median falls on hi
    assert boxes[4, 0, 0] == 1 and boxes[2, 0, 0] != 1
    # a median that falls on hi: the cut is hi - 1, the box still splits
    boxes, n = _boxes([(0, 5, 0, 1), (0, 9, 0, 10)])
    assert n == 2 and boxes == {(0, 5, 0): 0, (0, 9, 0): 1}
    # a single colour; fewer than 256 occupied bins: every bin its own entry, the rest 0
    pal, table, used = G.palette(np.full((2, 3, 4, 3), 77, np.uint8))
    assert used == 1 and pal[0].tolist() == [77, 77, 77] and not pal[1:].any() and table[G.bins_of(np.array([77, 77, 77], np.uint8))] == 0
    clip = G.clip_of_bins([(r, (3 * r) % 32, (7 * r) % 32, 1 + r % 3) for r in range(20)])
    pal, table, used = G.palette(clip)
    assert used == 20 and not pal[20:].any() and np.array_equal(pal[G.indices(clip, table)], clip)
    # the rounding: floor((2 sum + n) / (2 n)) -- 1, 2 -> 2 (1.5 rounds up); 1, 1, 2 -> 1
    pal, _, _ = G.palette(np.array([[1, 1, 2], [2, 1, 1]], np.uint8).reshape(1, 1, 2, 3))
    assert pal[0].tolist() == [2, 1, 2]
    pal, _, _ = G.palette(np.array([[1, 0, 0], [1, 0, 0], [2, 0, 0]], np.uint8).reshape(1, 1, 3, 3))
    assert pal[0].tolist() == [1, 0, 0]
    # the table's ties go to the lowest entry, and a full palette of noise has 256 boxes
    pal, table, used = G.clip_palette("noise_2x33x65")
    assert used == 256
    cnt, sums = G.histogram(G.clips()["noise_2x33x65"])
    for b in np.nonzero(cnt)[0][::97]:
        own = (2 * sums[b] + cnt[b]) // (2 * cnt[b])
        d = ((pal.astype(np.int64) - own) ** 2).sum(1)
        assert table[b] == int(np.flatnonzero(d == d.min())[0])


def test_two_hundred_colours_are_stored_exactly(tmp_path):
    clip = G.colours_200()
    pal, table, used = G.palette(clip)
    assert used == 200 and np.array_equal(pal[G.indices(clip, table)], clip)
    stream, off, pal, table, used = G.encode(clip, 0)
    frames, _, _, _ = pil_decode(G.gif_file([stream[off[i]:off[i + 1]] for i in range(3)], pal, 8, 24, 40))
    assert np.array_equal(frames, clip)


# ------------------------------------------------------------------ 3
def test_container_field_by_field(tmp_path):
    from ccvs_amd.tools import gif
    m = G.mirrored("two_4x40x31", 3)
    payloads = [m["stream"][m["off"][i]:m["off"][i + 1]] for i in range(4)]
    for fps, delay in ((1, 100), (4, 25), (25, 4), (50, 2), (100, 2)):
        path = tmp_path / f"{fps}.gif"
        gif.write_gif(str(path), payloads, m["pal"], fps, 40, 31)
        data = path.read_bytes()
        assert data == G.gif_file(payloads, m["pal"], fps, 40, 31) and gif.delay_cs(fps) == delay
        assert data[:6] == b"GIF89a" and struct.unpack("<HH", data[6:10]) == (31, 40)
        assert data[10] == 0xF7 and data[11:13] == b"\x00\x00"          # a global table of 2^(7 + 1) entries, 8 bits per primary; no background, no aspect
        assert data[13:781] == m["pal"].tobytes()
        assert data[781:800] == b"\x21\xFF\x0BNETSCAPE2.0\x03\x01\x00\x00\x00"
        pos = 800
        for p in payloads:
            assert data[pos:pos + 8] == b"\x21\xF9\x04\x00" + struct.pack("<H", delay) + b"\x00\x00"
            assert data[pos + 8:pos + 18] == b"\x2C" + struct.pack("<HHHHB", 0, 0, 31, 40, 0)
            assert data[pos + 18:pos + 18 + len(p)] == p and p[0] == 8 and p[-1] == 0
            pos += 18 + len(p)
        assert data[pos:] == b"\x3B"
        frames, delays, loop, size = pil_decode(data)
        assert delays == [10 * delay] * 4 and loop == 0 and size == (31, 40) and len(frames) == 4
    assert "below 2" in gif.write_gif.__doc__ and "below 2" in gif.delay_cs.__doc__
    for bad in (dict(payloads=[]), dict(h=0), dict(w=65536), dict(fps=0), dict(palette=b"\x00" * 767)):
        kw = dict(payloads=payloads, palette=m["pal"], fps=4, h=40, w=31)
        kw.update(bad)
        with pytest.raises(ValueError, match="write_gif"):
            gif.write_gif(str(tmp_path / "bad.gif"), **kw)
    # the reader refuses what it does not read
    good = (tmp_path / "4.gif").read_bytes()
    for data, word in ((b"GIF00a" + good[6:], "signature"), (good[:-1], "trailer"), (good[:10] + b"\x77" + good[11:], "global colour table"),
                       (good[:803] + b"\x01" + good[804:], "transparency"), (good[:900], "past the end")):
        (tmp_path / "r.gif").write_bytes(data)
        with pytest.raises(ValueError, match=word):
            gif.read_gif(str(tmp_path / "r.gif"))


# ------------------------------------------------------------------ 4
def test_gif_symbols_declared_and_exported(tmp_path):
    from ccvs_amd import lib
    header = open(os.path.join(ROOT, "include", "ccvs_hip_output_gif.h")).read()
    assert re.search(r'^#include "ccvs_hip_output_gif.h"', open(os.path.join(ROOT, "include", "ccvs_hip.h")).read(), re.M)
    declared = sorted(set(re.findall(r"^\w[\w \*]*?\b(ccvs_\w+)\(", header, re.M)))
    assert declared == sorted(lib.GIF_SYMBOLS) == ["ccvs_gif_encode", "ccvs_gif_palette", "ccvs_gif_stream_bound", "ccvs_gif_workspace_bytes"]
    others = [getattr(lib, n) for n in dir(lib) if n.endswith("EXPORTS") or (n.endswith("SYMBOLS") and n != "GIF_SYMBOLS")]
    assert not any(set(lib.GIF_SYMBOLS) & set(o) for o in others) and len(lib.EXPORTS) == 51
    handle = ctypes.CDLL(lib.LIB_PATH)
    for sym in lib.GIF_SYMBOLS:
        assert hasattr(handle, sym), sym
    c = tmp_path / "p.c"
    c.write_text('#include "ccvs_hip.h"\nvoid* p[] = {' + ", ".join("(void*)" + s for s in lib.GIF_SYMBOLS) + "};\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "p.o")], check=True)
    assert lib.load().ccvs_abi_version() == 6


def test_stream_bound_sizes_and_refusals_before_any_launch():
    from ccvs_amd import lib
    L = lib.load()
    ws, bound = L.ccvs_gif_workspace_bytes, L.ccvs_gif_stream_bound
    rng = np.random.default_rng(4)
    for h, w in ((33, 65), (1, 5000), (64, 96), (7, 1), (1, 1), (3, 4100)):
        for r in sorted({0, 1, 3, h}):
            assert bound(1, h, w, r) == G.stream_bound(1, h, w, r) and bound(5, h, w, r) == 5 * bound(1, h, w, r), (h, w, r)
            stream, off = G.encode_indices(rng.integers(0, 256, (2, h, w)).astype(np.uint8), r)
            assert len(stream) <= bound(2, h, w, r), (h, w, r)
            assert ws(2, 3, h, w, r) >= 2 * (1 << 20) + 6 * 8 * (G.bands(h, w, r) + 2), (h, w, r)
    for args in ((0, 8, 8, 0), (1, 0, 8, 0), (1, 8, 0, 0), (1, 65536, 8, 0), (1, 8, 65536, 0), (1, 8, 8, -1), (1, 65535, 65535, 65535), (1 << 24, 8, 8, 0)):
        assert bound(*args) == 0 and ws(1, *args) == 0, args
    assert ws(0, 1, 8, 8, 0) == 0 and ws(1, 0, 8, 8, 0) == 0
    one = ctypes.c_void_p(16)

    def encode(b=1, t=2, h=8, w=8, r=0, cap=64, cs=384, fs=192):
        return L.ccvs_gif_encode(one, cs, fs, b, t, h, w, r, one, one, cap, one, one, None)

    def palette(b=1, t=2, h=8, w=8, cs=384, fs=192):
        return L.ccvs_gif_palette(one, cs, fs, b, t, h, w, one, one, one, one, None)

    for kw, word in ((dict(b=0), "clips"), (dict(t=0), "clips"), (dict(b=1 << 12, t=1 << 12), "clips"), (dict(h=0), "size"), (dict(w=65536), "size"),
                     (dict(fs=191), "frame stride"), (dict(cs=383), "clip stride"), (dict(fs=-192), "frame stride")):
        for call, who in ((encode, "ccvs_gif_encode"), (palette, "ccvs_gif_palette")):
            assert call(**kw) != 0, kw
            msg = L.ccvs_last_error().decode()
            assert word in msg and who in msg, (kw, msg)
    for kw, word in ((dict(r=-1), "band_rows"), (dict(cap=-1), "capacity"), (dict(h=65535, w=65535, r=65535, fs=1 << 40, cs=1 << 42), "band_rows")):
        assert encode(**kw) != 0 and word in L.ccvs_last_error().decode(), kw
    for k in (0, 8, 9, 11, 12):                                         # clips, table, stream (with a capacity), offsets, workspace
        argv = [one, 384, 192, 1, 2, 8, 8, 0, one, one, 64, one, one, None]
        argv[k] = None
        assert L.ccvs_gif_encode(*argv) != 0 and "null" in L.ccvs_last_error().decode(), k
    for k in (0, 7, 8, 9, 10):
        argv = [one, 384, 192, 1, 2, 8, 8, one, one, one, one, None]
        argv[k] = None
        assert L.ccvs_gif_palette(*argv) != 0 and "null" in L.ccvs_last_error().decode(), k


# ------------------------------------------------------------------ 5
def test_cpu_tensors_are_refused(tmp_path):
    from ccvs_amd import lib, ops
    from ccvs_amd.helpers.generator import save_video_batch, write_u8_clips
    clips = torch.zeros(1, 2, 8, 8, 3, dtype=torch.uint8)
    for fn in (ops.gif_palette, ops.gif_encode, ops.gif_encode_to_host):
        with pytest.raises(lib.CcvsError):
            fn(clips)
    with pytest.raises(lib.CcvsError):
        save_video_batch(torch.zeros(1, 2, 3, 8, 8), 1, 0, str(tmp_path / "a"), 4, True, False, [-1, 1], "bairhd", video_format="gif")
    with pytest.raises(ValueError, match="video_format"):
        save_video_batch(torch.zeros(1, 2, 3, 8, 8), 1, 0, str(tmp_path / "a"), 4, True, False, [-1, 1], "bairhd", video_format="mp4")
    with pytest.raises(ValueError, match="video_format"):
        write_u8_clips(clips, None, "cpu", 1, 0, str(tmp_path / "b"), 4, "mp4")


def test_option_parses_and_moves_no_default():
    from ccvs_amd.tools.options import Options
    plain = Options().parse(True, True, argv=TINY)
    on = Options().parse(True, True, argv=TINY + ["--video_format", "gif", "--video_quality", "50", "--video_subsampling", "420", "--video_optimize", "--video_lz77"])
    assert plain["transformer"].video_format == "auto" and on["transformer"].video_format == "gif" and on["base"].video_format == "gif"
    with pytest.raises(SystemExit):
        Options().parse(True, True, argv=TINY + ["--video_format", "mp4"])
    on = Options().parse(True, True, argv=TINY + ["--video_format", "gif"])
    for key in ("transformer", "qvid_generator"):
        a, b = vars(plain[key]), vars(on[key])
        skip = lambda k: k in ("video_format", "signature") or k.endswith("_path")
        assert {k: v for k, v in a.items() if not skip(k)} == {k: v for k, v in b.items() if not skip(k)}, key


def test_save_results_passes_gif_through(tmp_path, monkeypatch):
    import types
    from ccvs_amd.helpers import generator as Gn
    seen = []
    monkeypatch.setattr(Gn, "save_video_batch", lambda *a, **k: seen.append((os.path.basename(a[3]), k["video_format"], k["return_clip"])))
    opt = types.SimpleNamespace(video_format="gif", video_quality=80, video_subsampling="420", video_optimize=True, video_lz77=True, result_path=str(tmp_path),
                                fps=4, imagenet_norm=False, dataset="bairhd", state=True)
    me = types.SimpleNamespace(opt=opt, decode_stft=False)
    vid = torch.zeros(2, 2, 3, 8, 8)
    Gn.Generator.save_results(me, {"real": vid, "fake": {"vid": vid, "state": torch.zeros(2, 2, 2)}, "rec": {"vid": vid}, "blur": vid}, 0)
    assert seen == [(k, "gif", False) for k in ("real", "fake", "fake_state", "rec", "blur")]


# ------------------------------------------------------------------ 6
def _case(idx, band_rows, chunk):
    idx = np.ascontiguousarray(idx, np.uint8)
    want = G.payload(G.frame_data(idx, band_rows))
    return np.array([idx.shape[0], idx.shape[1], band_rows, chunk, len(want)], np.int64).tobytes() + idx.tobytes() + want


def test_core_on_the_host_under_sanitizers(tmp_path):
    cases = []
    for L in G.BAND_SWEEP:
        for kind in ("noise", "flat", "two"):
            cases.append(_case(G.sweep_indices(L, kind), L, 1024))
    for name, r in G.rows():
        for f in G.mirrored(name, r)["idx"][:2]:
            cases.append(_case(f, r, 1024))
    rng = np.random.default_rng(11)
    for shape, r, chunk in (((1, 5000), 0, 1024), ((1, 5000), 0, 7), ((3, 4100), 3, 4096), ((50, 100), 50, 1), ((1, 9000), 1, 1000)):
        cases.append(_case(rng.integers(0, 256, shape), r, chunk))
    for target in (254, 255, 256, 510):
        cases.append(_case(G.edge_frame(target), 0, 1024))
    exe = str(tmp_path / "gif_core_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-I", os.path.join(ROOT, "ccvs_amd", "csrc"), os.path.join(HERE, "gif_core_check.cpp"), "-o", exe], check=True)
    (tmp_path / "cases.bin").write_bytes(b"".join(cases))
    run = subprocess.run([exe, str(tmp_path / "cases.bin")], capture_output=True, text=True)
    print(run.stdout, run.stderr[-4000:])
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    assert run.stdout.split() == ["cases", str(len(cases)), "wrong", "0"]


# ------------------------------------------------------------------ 7
def _psnr(a, b):
    mse = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def test_recorded_file_size_and_quantisation_psnr():
    """Recorded, no bar: the banded stream's size over Pillow's own GIF of the same index frames and palette (save_all, optimize=False), and
    the PSNR of palette[indices] against the uint8 source beside Pillow's per-frame quantize(256, MEDIANCUT, dither=NONE)."""
    for name in ("smooth_5x64x96", "noise_2x33x65", "two_4x40x31", "smooth_3x23x17"):
        clip = G.clips()[name]
        t, h, w = clip.shape[:3]
        pal, _, _ = G.clip_palette(name)
        ratios = {}
        for r in (0, h):
            m = G.mirrored(name, r)
            ours = len(G.gif_file([m["stream"][m["off"][i]:m["off"][i + 1]] for i in range(t)], pal, 10, h, w))
            ims = []
            for f in m["idx"]:
                im = Image.fromarray(f, "P")
                im.putpalette(pal.tobytes())
                ims.append(im)
            buf = io.BytesIO()
            ims[0].save(buf, "GIF", save_all=True, append_images=ims[1:], optimize=False, duration=100, loop=0)
            ratios[r] = ours / len(buf.getvalue())
        ours = _psnr(pal[G.mirrored(name, 0)["idx"]], clip)
        pil = _psnr(np.stack([np.asarray(Image.fromarray(f).quantize(256, Image.Quantize.MEDIANCUT, dither=Image.Dither.NONE).convert("RGB")) for f in clip]), clip)
        print(f"{name}: size / Pillow's band_rows 0: {ratios[0]:.3f}, h: {ratios[h]:.3f}; PSNR {ours:.2f} dB, Pillow per frame {pil:.2f} dB")
        assert all(0 < v < 4 for v in ratios.values())                 # (a sanity bracket, not a bar)

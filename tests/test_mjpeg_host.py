"""not gpu: the host side of the Motion-JPEG output stage.

  1. the spec mirror tests/jpeg_ref.py gives, byte for byte, the scan of every file of tests/golden/mjpeg_cases.npz (written by Pillow =
     libjpeg), and of a live Pillow encode where Pillow imports;
  2. the mirror's counts over the case table: stuffed bytes, ZRL, blocks without EOB, DC category 11, AC category 10, the RST counter
     wrapping from 7 to 0, a partial last interval -- so that the table cannot quietly lose them;
  3. `jpeg_header(...) + scan + EOI` is a well-formed file (a marker walk), holds the tables the mirror coded with and Pillow wrote,
     and decodes to the pixels Pillow's own file decodes to;
  4. `write_avi` -> `read_avi`: frames byte for byte (an odd-length one among them), fps and size, every RIFF / LIST size against the
     file's length, every idx1 entry against its chunk;
  5. `lib.OUTPUT_EXPORTS` equals what include/ccvs_hip_output.h declares, the built library exports it, bad arguments are refused;
  6. the options, and `save_video_batch(video_format=None)` still taking the branch it took before.
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
import jpeg_ref as R  # noqa: E402

TINY = ["--name", "tiny", "--dataset", "bairhd", "--max_dim", "32", "--vid_len", "4", "--q_z_num", "32", "--q_z_size", "16",
        "--q_z_shape", "8", "8", "--q_use_enc", "--q_use_dec", "--q_necf", "8", "--q_necf_mult", "1", "2", "2",
        "--q_enc_model", "skipgan", "--q_dec_model", "skipgan", "--q_use_inter", "--q_inter_p", "0.75",
        "--q_skip_context", "1", "2", "3", "--q_skip_memory", "3", "--x_z_num", "32", "--x_z_len", "256", "--x_n_layer", "2",
        "--x_n_head", "2", "--x_n_embd", "32", "--x_z_chunk", "64", "--x_cond_len", "64", "--x_emb_mode", "temporal",
        "--x_num_blocks", "4", "--batch_size_vid", "2"]


@pytest.fixture(scope="module")
def gold(golden_dir):
    path = os.path.join(golden_dir, "mjpeg_cases.npz")
    assert os.path.getsize(path) < 512 << 10
    return np.load(path)


@pytest.fixture(scope="module")
def mirror(gold):
    """{row key: the mirror's scan} and the counts over the whole table, computed once."""
    stats = R.new_stats()
    return {key: R.encode_scan(gold[name + "/in"], q, r, stats) for key, name, q, r in R.rows()}, stats


# ------------------------------------------------------------------ 1, 2: the mirror
def test_fixture_holds_the_case_table(gold):
    assert str(gold["pillow_version"])
    for name, (make, _, _) in R.CASES.items():
        assert np.array_equal(gold[name + "/in"], make()), name
    assert sorted(k for k in gold.files if "/q" in k) == sorted(key for key, _, _, _ in R.rows())
    for case in ("constant_8x8", "noise_8x8", "noise_24x40", "noise_13x21", "checker_16x16", "smooth_64x64", "sparse_32x32", "noise_72x8",
                 "noise_16x40_r3", "noise_8x520"):
        assert R.CASES[case][1] == (100, 90, 75, 30, 5), case
    assert R.CASES["smooth_256x256"][1] and R.CASES["noise_16x40_r3"][2] == 3
    # the overflow case: the scan is larger than the raw frame
    assert len(R.scan_of(gold["noise_24x40/q100"].tobytes())) > gold["noise_24x40/in"].size


def test_mirror_equals_the_fixture_scans(gold, mirror):
    scans, _ = mirror
    for key, name, q, r in R.rows():
        want = R.scan_of(gold[key].tobytes())
        assert scans[key] == want, (key, len(scans[key]), len(want))


def test_mirror_equals_a_live_pillow_encode(gold, mirror):
    PIL = pytest.importorskip("PIL")
    from PIL import Image
    print("Pillow", PIL.__version__, "; fixture made with", str(gold["pillow_version"]))
    scans, _ = mirror
    for key, name, q, r in R.rows():
        buf = io.BytesIO()
        Image.fromarray(gold[name + "/in"], "RGB").save(buf, format="JPEG", quality=q, subsampling=0, restart_marker_blocks=r)
        assert R.scan_of(buf.getvalue()) == scans[key], key


def test_case_table_statistics(mirror):
    _, stats = mirror
    print(stats)
    assert stats["stuffed"] >= 1 and stats["zrl"] >= 1 and stats["no_eob"] >= 1
    assert stats["max_dc_cat"] == 11 and stats["max_ac_cat"] == 10
    assert stats["rst_wrap"] >= 1 and stats["partial_last"] >= 1
    # the intervals of the 8 x 520 row: 32 / 32 / 1 MCUs; of the 72 x 8 one: nine
    one = R.new_stats()
    R.encode_scan(R.CASES["noise_8x520"][0](), 30, None, one)
    assert one["intervals"] == 3 and one["partial_last"] == 1
    nine = R.new_stats()
    scan = R.encode_scan(R.CASES["noise_72x8"][0](), 30, None, nine)
    assert nine["intervals"] == 9 and scan.count(b"\xff\xd7") >= 1


# ------------------------------------------------------------------ 3: the header
def walk(data):
    """The marker walk of a whole baseline file: {marker: [payloads]}, the scan."""
    segs, start = R.segments(data)
    assert data[-2:] == b"\xff\xd9"
    scan = data[start:-2]
    i = 0
    while True:                       # inside the scan 0xFF is followed by 0x00 or by RSTn only
        i = scan.find(b"\xff", i)
        if i < 0:
            break
        assert i + 1 < len(scan) and (scan[i + 1] == 0 or 0xD0 <= scan[i + 1] <= 0xD7), (i, scan[i:i + 2])
        i += 2
    by = {}
    for marker, payload in segs:
        by.setdefault(marker, []).append(payload)
    return by, scan


def test_header_is_well_formed_and_holds_the_tables(gold, mirror):
    from ccvs_amd.tools import mjpeg
    scans, _ = mirror
    for key, name, q, r in R.rows():
        h, w = gold[name + "/in"].shape[:2]
        by, scan = walk(mjpeg.jpeg_header(h, w, q, r) + scans[key] + mjpeg.EOI)
        assert scan == scans[key]
        assert set(by) == {0xDB, 0xC0, 0xC4, 0xDD, 0xDA}, key                     # no APP0 needed, nothing else
        (sof,) = by[0xC0]
        assert struct.unpack(">BHHB", sof[:6]) == (8, h, w, 3) and sof[6:] == bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
        assert len(by[0xC4]) == 4 and R.dht_tables([(0xC4, p) for p in by[0xC4]]) == {k: (list(b), list(v)) for k, (b, v) in R.HUFF.items()}
        assert by[0xDD] == [struct.pack(">H", r)] and by[0xDA] == [bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])]
        tables = R.quant_tables(q)
        assert [p[0] for p in by[0xDB]] == [0, 1]
        for t, p in enumerate(by[0xDB]):
            assert list(p[1:]) == [int(tables[t][R.ZIGZAG[k]]) for k in range(64)], (key, t)
        # ... and they are the tables of Pillow's own file
        theirs, _ = walk(gold[key].tobytes())
        assert sorted(theirs[0xDB]) == sorted(by[0xDB]) and theirs[0xDD] == by[0xDD] and theirs[0xC0] == by[0xC0]
        assert R.dht_tables([(0xC4, p) for p in theirs[0xC4]]) == R.dht_tables([(0xC4, p) for p in by[0xC4]])
    assert mjpeg.jpeg_header(24, 40, 90) == mjpeg.jpeg_header(24, 40, 90, 5)      # the default interval: a row of MCUs
    assert mjpeg.default_restart(256) == 32 and mjpeg.default_restart(520) == 32 and mjpeg.default_restart(21) == 3
    for bad in ((0, 8, 90, 1), (8, 65536, 90, 1), (8, 8, 90, 33), (8, 8, 90, 0)):
        with pytest.raises(ValueError):
            mjpeg.jpeg_header(*bad)
    for q in (0, 101):
        with pytest.raises(ValueError):
            mjpeg.jpeg_header(8, 8, q)


def test_header_and_scan_decode_to_pillows_pixels(gold, mirror):
    pytest.importorskip("PIL")
    from ccvs_amd.tools import mjpeg
    scans, _ = mirror
    for key, name, q, r in R.rows():
        h, w = gold[name + "/in"].shape[:2]
        ours = mjpeg.decode_frames([mjpeg.jpeg_header(h, w, q, r) + scans[key] + mjpeg.EOI])
        theirs = mjpeg.decode_frames([gold[key].tobytes()])
        assert ours.shape == (1, h, w, 3) and ours.dtype == np.uint8 and np.array_equal(ours, theirs), key


def test_decode_frames_names_pillow_when_it_is_missing(monkeypatch):
    from ccvs_amd.tools import mjpeg
    monkeypatch.setitem(sys.modules, "PIL", None)
    with pytest.raises(ImportError, match="Pillow"):
        mjpeg.decode_frames([b""])


# ------------------------------------------------------------------ 4: the container
def riff_tree(data, start, end, depth=0):
    """Walks RIFF chunks, asserting that every size stays inside its container and that every LIST is filled exactly."""
    out, pos = [], start
    while pos < end:
        assert pos + 8 <= end
        tag, size = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
        assert pos + 8 + size + (size & 1) <= end, (tag, pos, size)
        if tag in (b"RIFF", b"LIST"):
            out.append((tag + data[pos + 8:pos + 12], pos, size, riff_tree(data, pos + 12, pos + 8 + size, depth + 1)))
        else:
            out.append((tag, pos, size, None))
        pos += 8 + size + (size & 1)
    assert pos == end
    return out


def test_avi_round_trip(tmp_path, gold, mirror):
    from ccvs_amd.tools import mjpeg
    scans, _ = mirror
    frames = [mjpeg.jpeg_header(24, 40, q, 5) + scans[f"noise_24x40/q{q}"] + mjpeg.EOI for q in (100, 90, 75, 30, 5)]
    assert any(len(f) & 1 for f in frames) and any(not len(f) & 1 for f in frames)
    path = str(tmp_path / "v.avi")
    mjpeg.write_avi(path, frames, 4, 24, 40)
    fps, h, w, back = mjpeg.read_avi(path)
    assert (fps, h, w) == (4, 24, 40) and back == frames
    data = open(path, "rb").read()
    (riff,) = riff_tree(data, 0, len(data))
    assert riff[0] == b"RIFFAVI " and riff[2] + 8 == len(data)
    kinds = [c[0] for c in riff[3]]
    assert kinds == [b"LISThdrl", b"LISTmovi", b"idx1"]
    hdrl, movi, idx1 = riff[3]
    assert [c[0] for c in hdrl[3]] == [b"avih", b"LISTstrl"] and [c[0] for c in hdrl[3][1][3]] == [b"strh", b"strf"]
    avih = struct.unpack_from("<14I", data, hdrl[3][0][1] + 8)
    assert avih[0] == 250000 and avih[4] == 5 and avih[6] == 1 and avih[8:10] == (40, 24) and avih[3] & 0x10
    strh, strf = hdrl[3][1][3]
    assert data[strh[1] + 8:strh[1] + 16] == b"vidsMJPG" and strh[2] == 56
    assert struct.unpack_from("<II", data, strh[1] + 8 + 20) == (1, 4) and struct.unpack_from("<I", data, strh[1] + 8 + 32)[0] == 5
    bi = struct.unpack_from("<IiiHH4s", data, strf[1] + 8)
    assert strf[2] == 40 and bi == (40, 40, 24, 1, 24, b"MJPG")
    assert [c[0] for c in movi[3]] == [b"00dc"] * 5 and [c[2] for c in movi[3]] == [len(f) for f in frames]
    # idx1: offsets from the 'movi' tag to the chunk header, sizes of the payloads
    assert idx1[2] == 16 * 5
    movi_tag = movi[1] + 8
    for k, f in enumerate(frames):
        tag, flags, off, size = struct.unpack_from("<4sIII", data, idx1[1] + 8 + 16 * k)
        assert tag == b"00dc" and flags & 0x10 and size == len(f)
        assert data[movi_tag + off:movi_tag + off + 4] == b"00dc" and struct.unpack_from("<I", data, movi_tag + off + 4)[0] == size
        assert data[movi_tag + off + 8:movi_tag + off + 8 + size] == f
    with pytest.raises(ValueError):
        mjpeg.write_avi(path, [], 4, 24, 40)
    open(path, "wb").write(data[:-3])
    with pytest.raises(ValueError, match="stated length"):
        mjpeg.read_avi(path)


def test_avi_frames_decode(tmp_path, gold):
    pytest.importorskip("PIL")
    from ccvs_amd.tools import mjpeg
    frames = [gold[f"noise_13x21/q{q}"].tobytes() for q in (100, 5)]
    mjpeg.write_avi(str(tmp_path / "p.avi"), frames, 10, 13, 21)
    fps, h, w, back = mjpeg.read_avi(str(tmp_path / "p.avi"))
    clip = mjpeg.decode_frames(back)
    assert fps == 10 and clip.shape == (2, 13, 21, 3)
    assert int(np.abs(clip[0].astype(int) - gold["noise_13x21/in"].astype(int)).max()) <= 4      # quality 100 is near lossless


# ------------------------------------------------------------------ 5: the C ABI
def test_output_symbols_declared_and_exported(tmp_path):
    from ccvs_amd import lib
    header = open(os.path.join(ROOT, "include", "ccvs_hip_output.h")).read()
    assert re.search(r'^#include "ccvs_hip_output.h"', open(os.path.join(ROOT, "include", "ccvs_hip.h")).read(), re.M)
    assert sorted(set(re.findall(r"\b(ccvs_[a-zA-Z0-9_]+)\s*\(", header))) == sorted(lib.OUTPUT_EXPORTS) == ["ccvs_mjpeg_encode", "ccvs_mjpeg_workspace_bytes"]
    others = set(lib.EXPORTS) | set(lib.EVAL_EXPORTS) | set(lib.INPUT_EXPORTS) | set(lib.GEMM_EXPORTS)
    assert not set(lib.OUTPUT_EXPORTS) & others and len(lib.EXPORTS) == 51
    handle = ctypes.CDLL(lib.LIB_PATH)
    for sym in lib.OUTPUT_EXPORTS:
        assert hasattr(handle, sym), sym
    c = tmp_path / "p.c"
    c.write_text('#include "ccvs_hip.h"\nvoid* p[] = {' + ", ".join("(void*)" + s for s in lib.OUTPUT_EXPORTS) + "};\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "p.o")], check=True)
    L = lib.load()
    assert L.ccvs_abi_version() == 6
    # 12 bytes per interval: 768 frames of 256 x 256 at 32 MCUs = 768 x 32 intervals
    assert L.ccvs_mjpeg_workspace_bytes(768, 256, 256, 32) == 12 * 768 * 32
    assert L.ccvs_mjpeg_workspace_bytes(1, 8, 8, 1) == 16 and L.ccvs_mjpeg_workspace_bytes(1, 8, 8, 33) == 0
    # refused before any GPU call
    one = ctypes.c_void_p(16)
    call = lambda n, h, w, q, r, cap=64, stride=192: L.ccvs_mjpeg_encode(one, stride, n, h, w, q, r, one, cap, one, one, None)
    for args, word in (((1, 8, 8, 0, 1), "quality"), ((1, 8, 8, 101, 1), "quality"), ((1, 8, 8, 90, 0), "restart"), ((1, 8, 8, 90, 33), "restart"),
                       ((1, 0, 8, 90, 1), "size"), ((1, 8, 65536, 90, 1), "size"), ((0, 8, 8, 90, 1), "frames"), ((1, 8, 8, 90, 1, -1), "capacity"),
                       ((2, 8, 8, 90, 1, 64, -192), "stride")):
        assert call(*args) != 0, args
        assert word in L.ccvs_last_error().decode(), (args, L.ccvs_last_error())
    assert L.ccvs_mjpeg_encode(None, 192, 1, 8, 8, 90, 1, one, 64, one, one, None) != 0 and "null" in L.ccvs_last_error().decode()


def test_ops_refuse_host_tensors():
    from ccvs_amd import lib, ops
    with pytest.raises(lib.CcvsError):
        ops.mjpeg_encode(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))


# ------------------------------------------------------------------ 6: options and the untouched default
def test_options():
    from ccvs_amd.tools.options import Options
    b = Options().parse(True, True, argv=TINY)["transformer"]
    assert b.video_format == "auto" and b.video_quality == 90
    a = Options().parse(True, True, argv=TINY + ["--video_format", "avi", "--video_quality", "75"])["base"]
    assert a.video_format == "avi" and a.video_quality == 75
    for bad in (["--video_quality", "0"], ["--video_quality", "101"], ["--video_format", "mp4"]):
        with pytest.raises(SystemExit):
            Options().parse(True, True, argv=TINY + bad)


def test_default_format_takes_the_branch_it_took(tmp_path, monkeypatch):
    """No GPU: `ops.pack_u8` is replaced by the same arithmetic in torch, the encoder by a function that fails the test."""
    from ccvs_amd.helpers import generator as G
    monkeypatch.setattr(G.ops, "pack_u8", lambda vid, lo, hi: ((vid.clamp(lo, hi) - lo) / (hi - lo) * 255).permute(0, 1, 3, 4, 2).to(torch.uint8))
    monkeypatch.setattr(G.ops, "mjpeg_encode_to_host", lambda *a, **k: pytest.fail("the default format must not encode"))
    monkeypatch.setitem(sys.modules, "torchvision.io", None)        # as on a machine without torchvision: the .npy branch
    vid = torch.rand(2, 3, 3, 8, 8, generator=torch.Generator().manual_seed(0)) * 2 - 1
    for k, extra in enumerate(({}, {"video_format": None}, {"video_format": "npy"})):
        d = tmp_path / str(k)
        u8 = G.save_video_batch(vid, 2, 1, str(d), 4, True, False, [-1, 1], "bairhd", **extra)
        assert sorted(os.listdir(d)) == ["vid_00002.npy", "vid_00003.npy"]
        assert u8.dtype == torch.uint8 and u8.shape == (2, 3, 8, 8, 3) and np.array_equal(np.load(d / "vid_00003.npy"), u8[1].numpy())
    # where torchvision imports, None still hands the clip to write_video and "npy" does not
    import types
    seen = []
    monkeypatch.setitem(sys.modules, "torchvision.io", types.SimpleNamespace(write_video=lambda fn, v, fps: seen.append((os.path.basename(fn), tuple(v.shape), fps))))
    G.save_video_batch(vid, 2, 0, str(tmp_path / "m"), 4, True, False, [-1, 1], "bairhd")
    assert seen == [("vid_00000.mp4", (3, 8, 8, 3), 4), ("vid_00001.mp4", (3, 8, 8, 3), 4)] and os.listdir(tmp_path / "m") == []
    G.save_video_batch(vid, 2, 0, str(tmp_path / "n"), 4, True, False, [-1, 1], "bairhd", video_format="npy")
    assert len(seen) == 2 and sorted(os.listdir(tmp_path / "n")) == ["vid_00000.npy", "vid_00001.npy"]
    with pytest.raises(ValueError, match="video_format"):
        G.save_video_batch(vid, 2, 0, str(tmp_path / "x"), 4, True, False, [-1, 1], "bairhd", video_format="mp4")

"""not gpu: the host side of the subsampled Motion-JPEG output (4:2:2 and 4:2:0).

  1. the spec mirror tests/jpeg_sub_ref.py gives, byte for byte, the scan of every file of tests/golden/mjpeg_sub_cases.npz (written by
     Pillow = libjpeg), and of a live Pillow encode where Pillow imports; its counts over the case table -- dummy blocks on the right, at
     the bottom and both in one MCU, stuffed bytes, ZRL, blocks without EOB, a DC category of 10 or more, the RST counter wrapping, a
     partial last interval -- so that the table cannot quietly lose them;
  2. `jpeg_header(..., sampling=s)` walked marker by marker: SOF factors, DRI and the tables are those of Pillow's header for the row;
  3. header + mirror scan + EOI decodes, with Pillow and with tests/jpeg_decode_ref.py, to the pixels Pillow decodes from its own file;
  4. `sampling=0` gives the bytes there were: `jpeg_header`, `default_restart`, and the mirror against `jpeg_ref.encode_scan`;
  5. `lib.OUTPUT_SAMPLED_EXPORTS` equals what include/ccvs_hip_output_sampled.h declares, the built library exports it, ccvs_hip.h alone
     serves a C translation unit, every refused argument is named in `ccvs_last_error()` -- before any launch, so without a GPU;
  6. `--video_subsampling` and `save_video_batch(subsampling=...)`.
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
import jpeg_decode_ref as D  # noqa: E402
import jpeg_ref as R  # noqa: E402
import jpeg_sub_ref as S  # noqa: E402
from tests.test_mjpeg_host import TINY, walk  # noqa: E402


@pytest.fixture(scope="module")
def gold(golden_dir):
    path = os.path.join(golden_dir, "mjpeg_sub_cases.npz")
    assert os.path.getsize(path) < 512 << 10
    return np.load(path)


@pytest.fixture(scope="module")
def mirror(gold):
    """{row key: the mirror's scan} and the counts over the whole table, computed once."""
    stats = S.new_stats()
    return {key: S.encode_scan_sub(gold[name + "/in"], q, s, r, stats) for key, name, s, q, r in S.rows()}, stats


# ------------------------------------------------------------------ 1: the mirror
def test_fixture_holds_the_case_table(gold):
    assert str(gold["pillow_version"])
    for name, (make, _, _) in S.CASES.items():
        assert np.array_equal(gold[name + "/in"], make()), name
    assert sorted(k for k in gold.files if "/q" in k) == sorted(row[0] for row in S.rows())
    sizes = {gold[name + "/in"].shape[:2] for name in S.CASES}
    assert sizes >= {(8, 8), (1, 1), (16, 16), (24, 40), (40, 24), (24, 24), (13, 21), (17, 33), (9, 9), (33, 7), (7, 33), (25, 72), (16, 520), (256, 256)}
    assert any(name.startswith("smooth") for name in S.CASES) and S.CASES["noise_56x72_r3"][2] == 3 and S.CASES["smooth_256x256"][1] == (90,)
    assert all(set(qs) <= set(R.ALL_Q) for _, qs, _ in S.CASES.values())
    assert {s for _, _, s, _, _ in S.rows()} == {1, 2}
    # the default interval of the workload's frame in 4:2:0 is exactly the 96 blocks an interval may hold
    assert [r for key, _, _, _, r in S.rows() if key == "smooth_256x256/s2/q90"] == [16]


def test_mirror_equals_the_fixture_scans(gold, mirror):
    scans, _ = mirror
    for key, name, s, q, r in S.rows():
        want = R.scan_of(gold[key].tobytes())
        assert scans[key] == want, (key, len(scans[key]), len(want))


def test_mirror_equals_a_live_pillow_encode(gold, mirror):
    PIL = pytest.importorskip("PIL")
    from PIL import Image
    print("Pillow", PIL.__version__, "; fixture made with", str(gold["pillow_version"]))
    scans, _ = mirror
    for key, name, s, q, r in S.rows():
        buf = io.BytesIO()
        Image.fromarray(gold[name + "/in"], "RGB").save(buf, format="JPEG", quality=q, subsampling=s, restart_marker_blocks=r)
        assert R.scan_of(buf.getvalue()) == scans[key], key


def test_case_table_statistics(mirror):
    _, stats = mirror
    print(stats)
    assert stats["dummy_right"] >= 1 and stats["dummy_bottom"] >= 1 and stats["mcu_with_both"] >= 1
    assert stats["stuffed"] >= 1 and stats["zrl"] >= 1 and stats["no_eob"] >= 1
    assert stats["max_dc_cat"] >= 10
    assert stats["rst_wrap"] >= 1 and stats["partial_last"] >= 1
    # the intervals of the 16 x 520 row: 33 MCUs as 16 / 16 / 1 in 4:2:0; two rows of 33 as 24 / 24 / 18 in 4:2:2, the middle one
    # straddling the rows; the tall one wraps the RST counter twice
    for s, n in ((2, 3), (1, 3)):
        one = S.new_stats()
        S.encode_scan_sub(S.CASES["noise_16x520"][0](), 30, s, None, one)
        assert one["intervals"] == n and one["partial_last"] == 1, s
        tall = S.new_stats()
        S.encode_scan_sub(S.CASES["noise_280x8"][0](), 30, s, None, tall)
        assert tall["intervals"] > 16 and tall["rst_wrap"] >= 2, s
    r3 = S.new_stats()
    S.encode_scan_sub(S.CASES["noise_56x72_r3"][0](), 5, 2, 3, r3)
    assert r3["intervals"] == 7 and r3["partial_last"] == 1 and r3["mcu_with_both"] == 1
    # where the issue's padding rule bites: h mod 16 in 1 .. 8 in 4:2:0 has a bottom row of dummies, 4:2:2 has none
    for s, bottom in ((2, True), (1, False)):
        one = S.new_stats()
        S.encode_scan_sub(S.CASES["noise_24x40"][0](), 90, s, None, one)
        assert (one["dummy_bottom"] > 0) == bottom and one["dummy_right"] > 0, s


# ------------------------------------------------------------------ 2, 3: the header
def test_header_is_well_formed_and_equals_pillows(gold, mirror):
    from ccvs_amd.tools import mjpeg
    scans, _ = mirror
    for key, name, s, q, r in S.rows():
        h, w = gold[name + "/in"].shape[:2]
        by, scan = walk(mjpeg.jpeg_header(h, w, q, r, s) + scans[key] + mjpeg.EOI)
        assert scan == scans[key]
        assert set(by) == {0xDB, 0xC0, 0xC4, 0xDD, 0xDA}, key
        (sof,) = by[0xC0]
        assert struct.unpack(">BHHB", sof[:6]) == (8, h, w, 3) and sof[6:] == bytes([1, (0x21, 0x22)[s - 1], 0, 2, 0x11, 1, 3, 0x11, 1])
        assert by[0xDD] == [struct.pack(">H", r)] and by[0xDA] == [bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])]
        theirs, _ = walk(gold[key].tobytes())
        assert sorted(theirs[0xDB]) == sorted(by[0xDB]) and theirs[0xDD] == by[0xDD] and theirs[0xC0] == by[0xC0], key
        assert R.dht_tables([(0xC4, p) for p in theirs[0xC4]]) == R.dht_tables([(0xC4, p) for p in by[0xC4]])
        parsed = mjpeg.parse_jpeg(gold[key].tobytes()) if w > 4 else None
        assert parsed is None or (parsed["sampling"], parsed["restart_interval"]) == (s, r)
    # the default interval: a row of the sampling's MCUs, capped at its limit
    assert mjpeg.jpeg_header(24, 40, 90, sampling=2) == mjpeg.jpeg_header(24, 40, 90, 3, 2) != mjpeg.jpeg_header(24, 40, 90, 3, 1)
    assert [mjpeg.default_restart(256, s) for s in (0, 1, 2)] == [32, 16, 16]
    assert [mjpeg.default_restart(520, s) for s in (0, 1, 2)] == [32, 24, 16] and mjpeg.default_restart(21, 2) == 2
    for bad in ((8, 8, 90, 1, 3), (8, 8, 90, 1, -1), (8, 8, 90, 1, "420"), (8, 8, 90, 25, 1), (8, 8, 90, 17, 2), (8, 8, 90, 0, 2), (0, 8, 90, 1, 2)):
        with pytest.raises(ValueError):
            mjpeg.jpeg_header(*bad)
    with pytest.raises(ValueError):
        mjpeg.default_restart(8, 3)
    mjpeg.jpeg_header(8, 8, 90, 24, 1), mjpeg.jpeg_header(8, 8, 90, 16, 2)                      # the limits themselves are taken


def test_header_and_scan_decode_to_pillows_pixels(gold, mirror):
    pytest.importorskip("PIL")
    from ccvs_amd.tools import mjpeg
    scans, _ = mirror
    for key, name, s, q, r in S.rows():
        h, w = gold[name + "/in"].shape[:2]
        ours = mjpeg.jpeg_header(h, w, q, r, s) + scans[key] + mjpeg.EOI
        theirs = mjpeg.decode_frames([gold[key].tobytes()])
        assert np.array_equal(mjpeg.decode_frames([ours]), theirs) and theirs.shape == (1, h, w, 3), key
        # the decoder mirror does not reproduce libjpeg's path for subsampled frames at most 4 pixels wide (it says so itself)
        if w > 4 and h * w <= 72 * 72:
            assert np.array_equal(D.decode(ours), theirs[0]), key
    key = "smooth_256x256/s2/q90"
    assert np.array_equal(D.decode(mjpeg.jpeg_header(256, 256, 90, 16, 2) + scans[key] + mjpeg.EOI), mjpeg.decode_frames([gold[key].tobytes()])[0])


# ------------------------------------------------------------------ 4: sampling 0 is what there was
def test_sampling_0_gives_the_bytes_there_were(golden_dir):
    from ccvs_amd.tools import mjpeg
    old = np.load(os.path.join(golden_dir, "mjpeg_cases.npz"))
    for key, name, q, r in R.rows():
        h, w = old[name + "/in"].shape[:2]
        head = mjpeg.jpeg_header(h, w, q, r)
        assert mjpeg.jpeg_header(h, w, q, r, 0) == mjpeg.jpeg_header(h, w, q, r, sampling=0) == head
        assert old[key].tobytes().endswith(R.scan_of(old[key].tobytes()) + mjpeg.EOI) and walk(head + mjpeg.EOI)[0][0xC0] == walk(old[key].tobytes())[0][0xC0]
        if h * w <= 64 * 64:
            assert S.encode_scan_sub(old[name + "/in"], q, 0, r) == R.encode_scan(old[name + "/in"], q, r) == R.scan_of(old[key].tobytes()), key
    for w in (1, 8, 9, 21, 255, 256, 257, 520, 65535):
        assert mjpeg.default_restart(w) == mjpeg.default_restart(w, 0) == S.default_restart(w) == R.default_restart(w) == min((w + 7) // 8, 32)
    assert mjpeg.jpeg_header(13, 21, 75) == mjpeg.jpeg_header(13, 21, 75, None, 0) == mjpeg.jpeg_header(13, 21, 75, 3)


# ------------------------------------------------------------------ 5: the C ABI
def test_sampled_symbols_declared_and_exported(tmp_path):
    from ccvs_amd import lib
    header = open(os.path.join(ROOT, "include", "ccvs_hip_output_sampled.h")).read()
    assert re.search(r'^#include "ccvs_hip_output_sampled.h"', open(os.path.join(ROOT, "include", "ccvs_hip.h")).read(), re.M)
    declared = sorted(set(re.findall(r"^(?:size_t|int) (ccvs_[a-zA-Z0-9_]+)\s*\(", header, re.M)))
    assert declared == sorted(lib.OUTPUT_SAMPLED_EXPORTS) == ["ccvs_mjpeg_encode_sampled", "ccvs_mjpeg_sampled_workspace_bytes"]
    others = (set(lib.EXPORTS) | set(lib.EVAL_EXPORTS) | set(lib.INPUT_EXPORTS) | set(lib.GEMM_EXPORTS) | set(lib.OUTPUT_EXPORTS) | set(lib.DECODE_EXPORTS)
              | set(lib.VIDEO_EXPORTS))
    assert not set(lib.OUTPUT_SAMPLED_EXPORTS) & others and len(lib.EXPORTS) == 51
    assert lib.OUTPUT_EXPORTS == ["ccvs_mjpeg_workspace_bytes", "ccvs_mjpeg_encode"]
    handle = ctypes.CDLL(lib.LIB_PATH)
    for sym in lib.OUTPUT_SAMPLED_EXPORTS:
        assert hasattr(handle, sym), sym
    c = tmp_path / "p.c"
    c.write_text('#include "ccvs_hip.h"\nvoid* p[] = {' + ", ".join("(void*)" + s for s in lib.OUTPUT_SAMPLED_EXPORTS) + "};\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "p.o")], check=True)
    L = lib.load()
    assert L.ccvs_abi_version() == 6
    ws = L.ccvs_mjpeg_sampled_workspace_bytes
    # 12 bytes per interval: 768 frames of 256 x 256 are 768 x 16 intervals of 16 MCUs in 4:2:0, 768 x 32 in 4:2:2 and 4:4:4
    assert ws(768, 256, 256, 2, 16) == 12 * 768 * 16 and ws(768, 256, 256, 1, 16) == 12 * 768 * 32
    assert ws(768, 256, 256, 0, 32) == L.ccvs_mjpeg_workspace_bytes(768, 256, 256, 32) == 12 * 768 * 32
    assert ws(1, 24, 40, 2, 1) == 12 * 6 and ws(1, 24, 40, 1, 1) == 12 * 9 + 4 and ws(1, 8, 8, 2, 1) == 16
    assert ws(1, 8, 8, 3, 1) == 0 and ws(1, 8, 8, -1, 1) == 0 and ws(1, 8, 8, 2, 17) == 0 and ws(1, 8, 8, 1, 25) == 0 and ws(1, 8, 8, 0, 33) == 0
    assert ws(1, 8, 8, 2, 16) and ws(1, 8, 8, 1, 24) and ws(1, 8, 8, 0, 32) and ws(0, 8, 8, 2, 1) == 0
    # refused before any GPU call
    one = ctypes.c_void_p(16)
    call = lambda n, h, w, q, s, r, cap=64, stride=192: L.ccvs_mjpeg_encode_sampled(one, stride, n, h, w, q, s, r, one, cap, one, one, None)
    for args, word in (((1, 8, 8, 90, 3, 1), "sampling"), ((1, 8, 8, 90, -1, 1), "sampling"),
                       ((1, 8, 8, 90, 0, 33), "restart"), ((1, 8, 8, 90, 1, 25), "restart"), ((1, 8, 8, 90, 2, 17), "restart"), ((1, 8, 8, 90, 2, 0), "restart"),
                       ((1, 8, 8, 0, 2, 1), "quality"), ((1, 8, 8, 101, 1, 1), "quality"), ((1, 0, 8, 90, 2, 1), "size"), ((1, 8, 65536, 90, 1, 1), "size"),
                       ((0, 8, 8, 90, 2, 1), "frames"), ((1, 8, 8, 90, 2, 1, -1), "capacity"), ((2, 8, 8, 90, 1, 1, 64, -192), "stride")):
        assert call(*args) != 0, args
        msg = L.ccvs_last_error().decode()
        assert word in msg and "ccvs_mjpeg_encode_sampled" in msg, (args, msg)
    assert L.ccvs_mjpeg_encode_sampled(None, 192, 1, 8, 8, 90, 2, 1, one, 64, one, one, None) != 0 and "null" in L.ccvs_last_error().decode()
    assert L.ccvs_mjpeg_encode_sampled(one, 192, 1, 8, 8, 90, 2, 1, one, 64, None, one, None) != 0 and "null" in L.ccvs_last_error().decode()


def test_ops_refuse_before_the_gpu():
    from ccvs_amd import lib, ops
    with pytest.raises(lib.CcvsError):
        ops.mjpeg_encode(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), sampling=2)
    with pytest.raises(lib.CcvsError):
        ops.mjpeg_encode_to_host(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 90, None, sampling=1)


# ------------------------------------------------------------------ 6: the options
def test_options():
    from ccvs_amd.tools.options import Options
    b = Options().parse(True, True, argv=TINY)["transformer"]
    assert b.video_subsampling == "444" and b.video_format == "auto"
    for value in ("444", "422", "420"):
        a = Options().parse(True, True, argv=TINY + ["--video_format", "avi", "--video_subsampling", value])["base"]
        assert a.video_subsampling == value and a.video_format == "avi"
    assert Options().parse(True, True, argv=TINY + ["--video_subsampling", "420"])["base"].video_format == "auto"      # ignored there, not refused
    for bad in ("411", "440", "2", ""):
        with pytest.raises(SystemExit):
            Options().parse(True, True, argv=TINY + ["--video_subsampling", bad])


def test_save_video_batch_validates_subsampling_before_the_device(tmp_path, monkeypatch):
    from ccvs_amd.helpers import generator as G
    for name in ("pack_u8", "pack_u8_norm", "mjpeg_encode_to_host"):
        monkeypatch.setattr(G.ops, name, lambda *a, **k: pytest.fail("refusal comes before any device work"))
    vid = torch.zeros(1, 2, 3, 8, 8)
    for bad in ("411", 2, None, "4:2:0"):
        with pytest.raises(ValueError, match="subsampling"):
            G.save_video_batch(vid, 1, 0, str(tmp_path / "x"), 4, True, False, [-1, 1], "bairhd", video_format="avi", subsampling=bad)
    assert not (tmp_path / "x").exists()
    # the other formats do not look at a valid value: the .npy branch writes what it wrote
    monkeypatch.setattr(G.ops, "pack_u8", lambda v, lo, hi: ((v.clamp(lo, hi) - lo) / (hi - lo) * 255).permute(0, 1, 3, 4, 2).to(torch.uint8))
    a = G.save_video_batch(vid, 1, 0, str(tmp_path / "a"), 4, True, False, [-1, 1], "bairhd", video_format="npy", subsampling="420")
    b = G.save_video_batch(vid, 1, 0, str(tmp_path / "b"), 4, True, False, [-1, 1], "bairhd", video_format="npy")
    assert torch.equal(a, b) and open(tmp_path / "a" / "vid_00000.npy", "rb").read() == open(tmp_path / "b" / "vid_00000.npy", "rb").read()


def test_save_results_passes_the_option_through(tmp_path, monkeypatch):
    """`Generator.save_results` hands --video_subsampling to every `save_video_batch` call (no GPU: the call is recorded, not made)."""
    import types
    from ccvs_amd.helpers import generator as G
    seen = []
    monkeypatch.setattr(G, "save_video_batch", lambda *a, **k: seen.append((os.path.basename(a[3]), k.get("state") is not None, k["video_format"], k["subsampling"])))
    opt = types.SimpleNamespace(video_format="avi", video_quality=80, video_subsampling="420", result_path=str(tmp_path), fps=4, imagenet_norm=False,
                                dataset="bairhd", state=True)
    me = types.SimpleNamespace(opt=opt, decode_stft=False)
    vid = torch.zeros(2, 2, 3, 8, 8)
    G.Generator.save_results(me, {"real": vid, "fake": {"vid": vid, "state": torch.zeros(2, 2, 2)}, "rec": {"vid": vid}}, 0)
    assert seen == [("real", False, "avi", "420"), ("fake", False, "avi", "420"), ("fake_state", True, "avi", "420"), ("rec", False, "avi", "420")]
    seen.clear()
    del opt.video_subsampling                                       # an options object from before the flag: full chrominance
    G.Generator.save_results(me, {"real": vid}, 0)
    assert seen == [("real", False, "avi", "444")]

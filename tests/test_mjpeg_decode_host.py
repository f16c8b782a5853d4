"""not gpu: the host side of the JPEG decoder.

  1. the spec mirror tests/jpeg_decode_ref.py decodes every file of tests/golden/mjpeg_decode_cases.npz to the pixels Pillow
     (libjpeg-turbo) decoded from it, and to a live Pillow decode where Pillow imports; the fixture holds the case table and what the
     entropy decoder must meet;
  2. `parse_jpeg` gives back the fields `jpeg_header` wrote, and the fixture files' fields as the mirror's own marker walk reads them;
  3. `find_units` equals the mirror's byte-by-byte split; `huffman_table` / `decode_tables` decode every code of every fixture table;
  4. ValueError, with the reason, for what is malformed or not decoded;
  5. `lib.DECODE_EXPORTS` equals what include/ccvs_hip_decode.h declares, the built library exports it, bad arguments are refused;
  6. `get_video_files`, `get_folders`, `print_scores` on a temporary tree; `metrics_from_files` still refuses mp4 and any resize.
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

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import jpeg_decode_ref as D  # noqa: E402
import jpeg_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def fixture(golden_dir):
    path = os.path.join(golden_dir, "mjpeg_decode_cases.npz")
    assert os.path.getsize(path) < 512 << 10
    return D.load_fixture(path)


@pytest.fixture(scope="module")
def mirror(fixture):
    """{row key: the mirror's pixels} and the counts over the whole table, computed once."""
    stats = D.new_stats()
    rows_with = {k: 0 for k in stats}
    out = {}
    for key, (data, _) in fixture[0].items():
        one = D.new_stats()
        out[key] = D.decode(data, one)
        for k, v in one.items():
            stats[k] = max(stats[k], v) if k == "max_dc_cat" else stats[k] + v
            rows_with[k] += v > 0
    return out, stats, rows_with


# ------------------------------------------------------------------ 1: the mirror and the fixture
def test_mirror_equals_pillows_pixels_on_every_row(fixture, mirror):
    for key, (_, rgb) in fixture[0].items():
        assert mirror[0][key].shape == rgb.shape and np.array_equal(mirror[0][key], rgb), key


def test_mirror_equals_a_live_pillow_decode(fixture, mirror):
    PIL = pytest.importorskip("PIL")
    from PIL import Image
    print("Pillow", PIL.__version__, "; fixture made with", fixture[1])
    for key, (data, _) in fixture[0].items():
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), mirror[0][key]), key


def test_fixture_holds_the_case_table(fixture, mirror):
    rows = D.rows()
    assert list(fixture[0]) == [r[0] for r in rows] and fixture[1]
    imgs = D.images()
    assert {r[1] for r in rows} == set(imgs) == set(R.CASES) | {"noise_17x35", "noise_1x1", "smooth_31x50"}
    assert imgs["noise_1x1"].shape == (1, 1, 3) and imgs["noise_17x35"].shape == (17, 35, 3) and imgs["smooth_31x50"].shape == (31, 50, 3)
    for name in imgs:
        mine = [r for r in rows if r[1] == name and not r[5] and not r[0].startswith("project/")]
        if name == "smooth_256x256":
            assert [r[2:5] for r in mine] == [(90, 0, 32)]
            continue
        subs = (0,) if imgs[name].shape[1] <= 4 else (0, 1, 2)                      # no subsampled rows 4 pixels wide or less
        assert {r[2] for r in mine} == set(D.THIN.get(name, D.ALL_Q)) and {(r[3], r[4]) for r in mine} == {(s, r) for s in subs for r in (0, 3)}, name
    assert {q for r in rows for q in [r[2]]} == {100, 90, 30, 5} and sum(r[5] for r in rows) == 3
    # the project's own header without its DHT segments: the frame relies on the Annex K tables
    data = fixture[0]["project/noise_24x40/q90/nodht"][0]
    assert 0xC4 not in [m for m, _ in R.segments(data)[0]] and D.parse(data)["ri"] == 5
    # what the entropy decoder must meet, counted by the mirror: rows with stuffed bytes, ZRL, blocks without EOB, codes longer than 8
    # bits, restart numbering past RST7, a partial last interval, partial MCUs on both edges at 4:2:0; DC category 11; no inverse DCT
    # value outside -512 .. 511 (there libjpeg's C and SIMD code differ and the bit-exact claim ends)
    _, stats, rows_with = mirror
    print(rows_with, stats)
    for k in ("stuffed", "zrl", "no_eob", "long_code", "rst_wrap", "partial_last", "partial_mcu_420"):
        assert rows_with[k] > 0, k
    assert stats["max_dc_cat"] == 11 and stats["idct_out_of_range"] == 0
    assert D.parse(fixture[0]["noise_17x35/q30/s2/r3"][0])["sampling"] == 2


# ------------------------------------------------------------------ 2, 3: parse_jpeg, find_units, the tables
def test_parse_jpeg_round_trips_jpeg_header():
    from ccvs_amd.tools import mjpeg
    for h, w, q, r in ((24, 40, 90, None), (13, 21, 5, 3), (256, 256, 100, 32), (1, 1, 75, 1)):
        head = mjpeg.jpeg_header(h, w, q, r)
        scan = R.encode_scan(np.zeros((h, w, 3), np.uint8), q, mjpeg.default_restart(w) if r is None else r)
        p = mjpeg.parse_jpeg(head + scan + mjpeg.EOI)
        assert (p["h"], p["w"], p["sampling"]) == (h, w, 0) and p["restart_interval"] == (mjpeg.default_restart(w) if r is None else r)
        tables = mjpeg.quant_tables(q)
        assert p["quant"] == (tables[0], tables[1], tables[1])
        assert p["huffman"] == mjpeg.HUFF and p["dc_tables"] == (0, 1, 1) and p["ac_tables"] == (0, 1, 1)
        assert (p["scan_offset"], p["scan_length"]) == (len(head), len(scan))


def test_parse_jpeg_and_find_units_equal_the_mirror(fixture):
    from ccvs_amd.tools import mjpeg
    for key, (data, _) in fixture[0].items():
        p, m = mjpeg.parse_jpeg(data), D.parse(data)
        assert (p["h"], p["w"], p["sampling"], p["restart_interval"]) == (m["h"], m["w"], m["sampling"], m["ri"]), key
        assert [list(q) for q in p["quant"]] == m["q"] and list(p["dc_tables"]) == m["dc"] and list(p["ac_tables"]) == m["ac"], key
        assert {k: (list(b), list(v)) for k, (b, v) in p["huffman"].items()} == m["huff"], key
        assert data[p["scan_offset"]:p["scan_offset"] + p["scan_length"]] == m["scan"], key
        mx, my = mjpeg.mcu_grid(p["h"], p["w"], p["sampling"])
        assert (mx, my) == D.geometry(m["h"], m["w"], m["sampling"])[2:]
        units = mjpeg.find_units(m["scan"], [0, len(m["scan"])], [m["ri"]], mx * my)
        assert units.dtype == np.int64 and units.tolist() == [[0, o, n, f, c] for o, n, f, c in D.split_units(m["scan"], m["ri"], mx * my)], key


def test_decode_tables_decode_every_code(fixture):
    """The record's lookup and maxcode / valoff / vals give every symbol of every fixture table back from its code."""
    from ccvs_amd.tools import mjpeg
    seen = set()
    for key, (data, _) in fixture[0].items():
        p = mjpeg.parse_jpeg(data)
        rec = mjpeg.decode_tables(p)
        if rec in seen:
            continue
        seen.add(rec)
        assert len(rec) == mjpeg.TABLE_BYTES == 4008
        assert np.frombuffer(rec, "<u2", 192).reshape(3, 64).tolist() == [list(q) for q in p["quant"]]
        assert list(rec[384:390]) == list(p["dc_tables"]) + list(p["ac_tables"])
        for slot, tkey in enumerate((0x00, 0x01, 0x10, 0x11)):
            base = 392 + 904 * slot
            look = np.frombuffer(rec, "<u2", 256, base)
            maxcode, valoff = np.frombuffer(rec, "<i4", 17, base + 512), np.frombuffer(rec, "<i4", 17, base + 580)
            vals = rec[base + 648:base + 904]
            for sym, (code, length) in R.huff_codes(*p["huffman"][tkey]).items():
                if length <= 8:
                    for fill in (0, (1 << (8 - length)) - 1):
                        assert look[(code << (8 - length)) | fill] == (length << 8) | sym
                else:
                    assert look[code >> (length - 8)] == 0 and all(code >> (length - n) > maxcode[n] for n in range(9, length))
                    assert code <= maxcode[length] and vals[valoff[length] + code] == sym
    assert len(seen) == 4 + 3    # a record per quality, and the three optimised files' own
    with pytest.raises(ValueError, match="prefix"):
        mjpeg.huffman_table([3] + [0] * 15, [0, 1, 2])


# ------------------------------------------------------------------ 4: what is refused
def _segment(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


def test_parse_jpeg_says_what_is_wrong(fixture):
    from ccvs_amd.tools import mjpeg
    good = fixture[0]["noise_13x21/q90/s0/r3"][0]
    mjpeg.parse_jpeg(good)
    sof = good.index(b"\xff\xc0")
    sos = good.index(b"\xff\xda")

    def sof_with(**kw):
        p = bytearray(good)
        for off, v in kw.values():
            p[sof + off] = v
        return bytes(p)

    cases = [
        (good[2:], "SOI"),
        (good[:-2], "EOI"),
        (good[:sos + 6] + mjpeg.EOI, "truncated"),                                               # the SOS segment runs past the end
        (good[:sof] + mjpeg.EOI, "truncated"),                                                   # no SOS at all
        (good[:sof + 1] + b"\xc2" + good[sof + 2:], "progressive"),
        (good[:sof + 1] + b"\xc9" + good[sof + 2:], "arithmetic"),
        (sof_with(a=(4, 12)), "12-bit"),
        (good[:sof] + _segment(0xC0, struct.pack(">BHHB", 8, 13, 21, 1) + bytes([1, 0x11, 0])) + good[sos:], "greyscale"),
        (good[:sof] + _segment(0xC0, struct.pack(">BHHB", 8, 13, 21, 4) + bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1, 4, 0x11, 0])) + good[sos:], "CMYK"),
        (sof_with(a=(11, 0x22), b=(14, 0x22)), "sampling"),                                      # 2 x 2 chrominance
        (sof_with(a=(11, 0x41)), "sampling"),                                                    # 4 x 1 luminance
        (sof_with(a=(11, 0x22), b=(7, 0), c=(8, 4)), "chrominance columns"),                     # 4:2:0 at w = 4
        (good[:sos + 4] + b"\x01" + good[sos + 5:], "interleaved"),
    ]
    for data, word in cases:
        with pytest.raises(ValueError, match=word):
            mjpeg.parse_jpeg(data)
    # through plan_frames the message names the frame; frames of another size are refused
    with pytest.raises(ValueError, match="frame 1: .*EOI"):
        mjpeg.plan_frames([good, good[:-2]])
    with pytest.raises(ValueError, match="frame 1: size"):
        mjpeg.plan_frames([good, fixture[0]["noise_17x35/q30/s0/r3"][0]])
    with pytest.raises(ValueError, match="frame 1: size"):
        mjpeg.plan_frames([good, fixture[0]["noise_13x21/q90/s2/r3"][0]])
    with pytest.raises(ValueError):
        mjpeg.plan_frames([])


def test_find_units_checks_markers_and_counts(fixture):
    from ccvs_amd.tools import mjpeg
    m = D.parse(fixture[0]["noise_72x8/q30/s0/r3"][0])                                          # 9 MCUs, interval 3: RST0, RST1
    scan = m["scan"]
    one = lambda sc, ri, n_mcu: mjpeg.find_units(sc, [0, len(sc)], [ri], n_mcu)  # noqa: E731
    assert one(scan, 3, 9).shape == (3, 5)
    at = scan.index(b"\xff\xd1")
    with pytest.raises(ValueError, match="frame 0: .*RST5.*RST1 expected"):
        one(scan[:at] + b"\xff\xd5" + scan[at + 2:], 3, 9)
    with pytest.raises(ValueError, match="3 unit.*5 expected"):
        one(scan, 2, 9)
    with pytest.raises(ValueError, match="3 unit.*1 expected"):
        one(scan, 0, 9)
    with pytest.raises(ValueError, match="marker 0xffc4"):
        one(scan[:at] + b"\xff\xc4" + scan[at + 2:], 3, 9)
    with pytest.raises(ValueError, match="ends in 0xFF"):
        one(scan + b"\xff", 3, 9)
    # several frames in one pass, with and without DRI: the table of each, offsets shifted; an error names its frame
    plain = D.parse(fixture[0]["noise_72x8/q30/s0/r0"][0])["scan"]
    both = mjpeg.find_units(scan + plain + scan, [0, len(scan), len(scan) + len(plain), 2 * len(scan) + len(plain)], [3, 0, 3], 9)
    assert both[:, 0].tolist() == [0, 0, 0, 1, 2, 2, 2] and both[3].tolist() == [1, len(scan), len(plain), 0, 9]
    assert (both[4:, 1:] - both[:3, 1:]).tolist() == [[len(scan) + len(plain), 0, 0, 0]] * 3 and both[:3].tolist() == one(scan, 3, 9).tolist()
    with pytest.raises(ValueError, match="frame 2: .*RST5.*RST1 expected"):
        mjpeg.find_units(scan + plain + scan[:at] + b"\xff\xd5" + scan[at + 2:], [0, len(scan), len(scan) + len(plain), 2 * len(scan) + len(plain)], [3, 0, 3], 9)
    with pytest.raises(ValueError, match="frame 1: the scan ends in 0xFF"):
        mjpeg.find_units(scan + plain + b"\xff" + scan, [0, len(scan), len(scan) + len(plain) + 1, 2 * len(scan) + len(plain) + 1], [3, 0, 3], 9)
    # rows past RST7, and a whole scan as one unit
    m = D.parse(fixture[0]["noise_88x8/q30/s0/r3"][0])
    units = one(m["scan"], 3, 11)
    assert units.shape == (4, 5) and units[:, 4].tolist() == [3, 3, 3, 2]
    m = D.parse(fixture[0]["noise_72x8/q100/s0/r3"][0])
    assert len(D.split_units(m["scan"], 3, 9)) == 3
    m = D.parse(fixture[0]["noise_13x21/q90/s0/r0"][0])
    assert one(m["scan"], 0, 6).tolist() == [[0, 0, len(m["scan"]), 0, 6]]
    long = D.parse(fixture[0]["smooth_256x256/q90/s0/r32"][0])
    units = one(long["scan"], 32, 1024)
    assert units.shape == (32, 5) and bytes(long["scan"][units[9, 1] - 2:units[9, 1]]) == b"\xff\xd0"      # the ninth marker is RST0 again


def test_plan_frames_shares_table_records(fixture):
    from ccvs_amd.tools import mjpeg
    files = [fixture[0][k][0] for k in ("noise_13x21/q90/s2/r3", "noise_13x21/q90/s2/opt", "noise_13x21/q90/s2/r0", "noise_13x21/q30/s2/r0")]
    plan = mjpeg.plan_frames(files)
    assert (plan["n"], plan["h"], plan["w"], plan["sampling"]) == (4, 13, 21, 2)
    assert plan["frame_table"].tolist() == [0, 1, 0, 2] and plan["tables"].size == 3 * 4008
    assert plan["units"][:, 0].tolist() == [0, 1, 2, 3] and plan["units"][:, 1].tolist() == list(np.cumsum([0] + [int(n) for n in plan["units"][:-1, 2]]))
    assert plan["scans"].size == int(plan["units"][:, 2].sum())


def test_mjpeg_module_stays_host_only():
    code = "import sys; import ccvs_amd.tools.mjpeg as m; m.parse_jpeg; assert 'torch' not in sys.modules and 'numpy' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


# ------------------------------------------------------------------ 5: the C ABI
def test_decode_symbols_declared_and_exported(tmp_path):
    from ccvs_amd import lib
    header = open(os.path.join(ROOT, "include", "ccvs_hip_decode.h")).read()
    assert re.search(r'^#include "ccvs_hip_decode.h"', open(os.path.join(ROOT, "include", "ccvs_hip.h")).read(), re.M)
    assert sorted(set(re.findall(r"^(?:size_t|int) (ccvs_[a-zA-Z0-9_]+)\s*\(", header, re.M))) == sorted(lib.DECODE_EXPORTS) == ["ccvs_mjpeg_decode", "ccvs_mjpeg_decode_workspace_bytes"]
    others = set(lib.EXPORTS) | set(lib.EVAL_EXPORTS) | set(lib.INPUT_EXPORTS) | set(lib.GEMM_EXPORTS) | set(lib.OUTPUT_EXPORTS)
    assert not set(lib.DECODE_EXPORTS) & others and len(lib.EXPORTS) == 51
    handle = ctypes.CDLL(lib.LIB_PATH)
    for sym in lib.DECODE_EXPORTS:
        assert hasattr(handle, sym), sym
    c = tmp_path / "p.c"
    c.write_text('#include "ccvs_hip.h"\nvoid* p[] = {' + ", ".join("(void*)" + s for s in lib.DECODE_EXPORTS) + "};\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "p.o")], check=True)
    L = lib.load()
    assert L.ccvs_abi_version() == 6
    # 128 bytes of coefficients per block and the planes: 256 x 256 at 4:4:4 is 3 x 1024 blocks and 3 x 65536 bytes a frame
    assert L.ccvs_mjpeg_decode_workspace_bytes(16, 256, 256, 0) == 16 * (3 * 1024 * 128 + 3 * 65536)
    # 13 x 21 at 4:2:0: 2 x 1 MCUs of 6 blocks; planes 32 x 16 and 2 x 16 x 8; both parts rounded up to 256 bytes
    assert L.ccvs_mjpeg_decode_workspace_bytes(1, 13, 21, 2) == 12 * 128 + 768
    assert L.ccvs_mjpeg_decode_workspace_bytes(1, 8, 8, 3) == 0 and L.ccvs_mjpeg_decode_workspace_bytes(1, 8, 4, 1) == 0 and L.ccvs_mjpeg_decode_workspace_bytes(0, 8, 8, 0) == 0
    # refused before any GPU call
    one = ctypes.c_void_p(16)
    units = np.array([[0, 0, 10, 0, 1]], dtype=np.int64)

    def call(scan_bytes=10, n_units=1, n=1, h=8, w=8, s=0, stride=192, n_tables=1, dev=one, host=True, rgb=one):
        rc = L.ccvs_mjpeg_decode(one, scan_bytes, dev, units.ctypes.data_as(ctypes.c_void_p) if host else None, n_units, one, n_tables, one, n, h, w, s,
                                 rgb, stride, one, one, None)
        return rc, L.ccvs_last_error().decode()

    for kw, word in (({"s": 3}, "sampling"), ({"s": -1}, "sampling"), ({"h": 0}, "size"), ({"w": 65536}, "size"), ({"w": 4, "s": 2, "stride": 96}, "chrominance"),
                     ({"n": 0}, "no frames"), ({"n_units": 0}, "no units"), ({"n_tables": 0}, "no tables"), ({"scan_bytes": -1}, "negative"),
                     ({"stride": 191}, "stride"), ({"host": False}, "null"), ({"rgb": None}, "null"), ({"dev": ctypes.c_void_p(20)}, "misaligned"),
                     ({"scan_bytes": 9}, "outside the stream")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, rc, msg)
    for row, word in (([1, 0, 10, 0, 1], "frame"), ([0, 11, 0, 0, 1], "outside the stream"), ([0, -1, 5, 0, 1], "outside the stream"),
                      ([0, 0, 10, 1, 1], "MCUs"), ([0, 0, 10, 0, 2], "MCUs"), ([0, 0, 10, -1, 1], "MCUs"), ([0, 2 ** 62, 2 ** 62, 0, 1], "outside the stream")):
        units[0] = row
        rc, msg = call()
        assert rc != 0 and word in msg, (row, rc, msg)


def test_ops_refuse_before_the_gpu(fixture):
    """What `ops.mjpeg_decode` refuses on the host: files that do not parse, with the frame named."""
    from ccvs_amd import ops
    good = fixture[0]["noise_13x21/q90/s0/r3"][0]
    with pytest.raises(ValueError, match="frame 1: .*SOI"):
        ops.mjpeg_decode([good, good[2:]])
    scan_at = D.parse(good)["scan_offset"]
    at = good.index(b"\xff\xd0", scan_at)
    with pytest.raises(ValueError, match="frame 0.*RST3"):
        ops.mjpeg_decode([good[:at] + b"\xff\xd3" + good[at + 2:]])


# ------------------------------------------------------------------ 6: the folder glue of the metrics
def test_metrics_folder_glue(tmp_path, monkeypatch, capsys):
    import torch
    from ccvs_amd.tools.pytorch_metrics import metrics as M
    root = tmp_path / "results"
    for tag in ("0001_run_0", "0002_run_1", "0003_other"):
        for kind in ("real", "fake"):
            os.makedirs(root / tag / kind)
    for name in ("vid_00001.avi", "vid_00000.avi", "vid_00002.npy"):
        (root / "0003_other" / "real" / name).write_bytes(b"")
    for name in ("vid_00001.npy", "vid_00000.npy"):
        (root / "0003_other" / "fake" / name).write_bytes(b"")
    (root / "0001_run_0" / "real" / "b.mp4").write_bytes(b"")
    (root / "0001_run_0" / "real" / "a.avi").write_bytes(b"")
    monkeypatch.chdir(tmp_path)
    assert M.get_folder("other") == os.path.join("results", "0003_other") and M.get_folders("other", None) == [os.path.join("results", "0003_other")]
    assert M.get_folders("run", 2) == [os.path.join("results", "0001_run_0"), os.path.join("results", "0002_run_1")]
    with pytest.raises(AssertionError, match="Too many possibilities"):
        M.get_folder("run")
    with pytest.raises(AssertionError):
        M.get_folder("absent")
    # one kind per folder: mp4 before avi before npy, sorted
    assert [os.path.basename(f) for f in M.get_video_files("results/0003_other/real")] == ["vid_00000.avi", "vid_00001.avi"]
    assert [os.path.basename(f) for f in M.get_video_files("results/0003_other/fake")] == ["vid_00000.npy", "vid_00001.npy"]
    assert [os.path.basename(f) for f in M.get_video_files("results/0001_run_0/real")] == ["b.mp4"]
    assert M.get_video_files("results/0002_run_1/real") == []
    M.print_scores([torch.tensor(1.0), torch.tensor(3.0)], "SSIM")
    M.print_scores([None], "LPIPS")
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "Individual SSIM scores" and out[2] == "Mean/std of SSIM across 2 runs" and out[3] == "2.0 1.0"
    assert out[4] == "LPIPS scores: not available (needs pretrained weights)"
    args = M.parse_args(["--exp_tag", "x", "--idx", "0", "2", "--print_256"])
    assert (args.exp_tag, args.real_tag, args.real_folder, args.fake_folder, args.num_folds, args.idx, args.num_workers, args.print_256, args.resize) == \
        ("x", None, "real", "fake", None, [0, 2], 8, True, None)
    # what stays refused: mp4 names without a loader (the message an earlier test pins), any resize, a batch of mixed kinds
    with pytest.raises(RuntimeError, match="no mp4 decoder"):
        M.metrics_from_files(["a.mp4"] * 16, ["b.avi"] * 16, None, 1, False, [])
    with pytest.raises(NotImplementedError, match="INTER_AREA"):
        M.load_videos(["a.avi"], (64, 64), 1)
    with pytest.raises(RuntimeError, match="all .avi or all .npy"):
        M.load_videos(["a.avi", "b.npy"], None, 1)

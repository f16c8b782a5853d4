"""The optimised-Huffman mode of the output stage, host side -- no GPU.

  1. the spec mirror tests/jpeg_opt_ref.py (symbol counts, libjpeg's jpeg_gen_optimal_table, the scan coded with the frame's tables)
     against the fixture tests/golden/mjpeg_opt_cases.npz -- the files Pillow (libjpeg) wrote with optimize=True: the four DHT payloads
     and the scan of every row, byte for byte; where Pillow imports, a live encode equals the fixture;
  2. the 256 x 256 row whose chrominance AC tree is 17 deep before limiting: Pillow's longest code is 16 and the mirror's tables and
     scan are Pillow's;
  3. `optimal_table` on synthetic counts (a Fibonacci vector of 40 symbols, one symbol, all 256, ties): lengths, the Kraft sum with
     the pseudo-symbol's slot left free, the order inside a length, exactly the counted symbols;
  4. the optimised scan is never longer in bits than the standard one on the rows;
  5. `tools.mjpeg.jpeg_header(huffman=...)`: the DHT segments are Pillow's, header + scan + EOI opens in Pillow with the pixels of the
     standard-table file; `huffman=None` gives the bytes there were; `huffman_from_spec`; what is refused;
  6. `lib.OUTPUT_OPTIMIZED_EXPORTS` equals what include/ccvs_hip_output_optimized.h declares, the built library exports it, EXPORTS
     and the ABI version did not move, every refused argument is named in `ccvs_last_error()` before any launch;
  7. `--video_optimize`, `save_results` passing it on, the reference's launch lines.
"""
import ctypes
import hashlib
import io
import json
import os
import re
import subprocess
import sys
import types
from fractions import Fraction

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import jpeg_opt_ref as O  # noqa: E402
import ref_harness as rh  # noqa: E402
from tests.test_mjpeg_host import TINY  # noqa: E402


@pytest.fixture(scope="module")
def gold(golden_dir):
    path = os.path.join(golden_dir, "mjpeg_opt_cases.npz")
    assert os.path.getsize(path) < 512 << 10
    return np.load(path)


@pytest.fixture(scope="module")
def mirror(gold):
    """{row key: (symbols per interval, scan, tables, depths before limiting)}, computed once."""
    out = {}
    for key, name, s, q, r in O.rows():
        symbols = O.scan_symbols(gold[name + "/in"], q, s, r)
        tables, depths = O.frame_tables(O.symbol_counts(None, 0, symbols=symbols))
        out[key] = (symbols, O.code_symbols(symbols, tables), tables, depths)
    return out


def _same_tables(a, b):
    return all((list(a[k][0]), list(a[k][1])) == (list(b[k][0]), list(b[k][1])) for k in O.TABLE_KEYS) and sorted(a) == sorted(b)


# ------------------------------------------------------------------ 1
def test_fixture_holds_the_case_table(gold):
    assert str(gold["pillow_version"])
    rows = O.rows()
    assert len({row[0] for row in rows}) == len(rows) >= 400
    for name in O.images():
        assert np.array_equal(gold[name + "/in"], O.image(name)), name
    # what the table is there to cover
    assert {gold[n + "/in"].shape[:2] for n in O.images()} == {(8, 8), (16, 16), (21, 33), (40, 24), (64, 64)}
    assert {(row[2], row[3]) for row in rows} == {(s, q) for s in (0, 1, 2) for q in (10, 50, 90, 100)}
    for s in (0, 1, 2):
        mine = [row for row in rows if row[2] == s]
        assert {1, 3, O.MAX_RESTART[s]} <= {row[4] for row in mine}
        n_int = lambda row: -(-np.prod(O.mcu_grid(*gold[row[1] + "/in"].shape[:2], s)) // row[4])
        assert any(n_int(row) > 8 for row in mine) and any(n_int(row) == 1 and row[4] > 1 for row in mine)      # RSTn wraps; interval > frame
        assert any(np.prod(O.mcu_grid(*gold[row[1] + "/in"].shape[:2], s)) == row[4] for row in mine) or s == 0  # exactly one MCU row


def test_mirror_equals_the_fixture(gold, mirror):
    for key, name, s, q, r in O.rows():
        data = gold[key].tobytes()
        segs, start = O.segments(data)
        assert [p[0] for m, p in segs if m == 0xC4] == list(O.TABLE_KEYS), key              # one table per DHT segment, libjpeg's order
        _, scan, tables, _ = mirror[key]
        assert _same_tables(tables, O.dht_tables(segs)), key
        assert scan == data[start:-2], key


def test_flat_frames_have_one_symbol_tables(gold, mirror):
    one, two = 0, 0
    for key, name, s, q, r in O.rows():
        if name.startswith("flat"):
            tables = mirror[key][2]
            assert all(len(tables[k][1]) == 1 and list(tables[k][0]) == [1] + [0] * 15 for k in (0x10, 0x11)), key   # EOB alone: one code of length 1
            one += len(tables[0x00][1]) == 1
            two += len(tables[0x00][1]) == 2
    assert one >= 3 and two >= 3          # every difference the same (interval 1), and a first difference beside zeros (interval 3)


def test_mirror_equals_a_live_pillow_encode(gold):
    PIL = pytest.importorskip("PIL")
    from PIL import Image
    print("Pillow", PIL.__version__, "; fixture made with", str(gold["pillow_version"]))
    for key, name, s, q, r in O.rows():
        buf = io.BytesIO()
        Image.fromarray(gold[name + "/in"], "RGB").save(buf, format="JPEG", quality=q, subsampling=s, restart_marker_blocks=r, optimize=True)
        assert buf.getvalue() == gold[key].tobytes(), key


# ------------------------------------------------------------------ 2
@pytest.fixture(scope="module")
def limiter():
    key, name, s, q, r = O.LIMITER_ROW
    return O.encode_scan_optimized(O.image(name), q, s, r)


def test_limiter_row(gold, limiter):
    key = O.LIMITER_ROW[0]
    scan, tables, depths = limiter
    print("depths before limiting", depths)
    assert max(depths) >= 17                                                               # the row is there for the K.2 adjustment
    assert max(len(b) for b, _ in tables.values()) == 16 and any(tables[k][0][15] for k in O.TABLE_KEYS)        # a 16-bit code exists
    assert np.array_equal(O.spec_bytes(tables), gold[key + "/dht"])
    assert len(scan) == int(gold[key + "/scan_len"]) and hashlib.sha256(scan).hexdigest() == str(gold[key + "/scan_sha256"])


def test_limiter_row_live(gold):
    pytest.importorskip("PIL")
    from PIL import Image
    key, name, s, q, r = O.LIMITER_ROW
    buf = io.BytesIO()
    Image.fromarray(O.image(name), "RGB").save(buf, format="JPEG", quality=q, subsampling=s, restart_marker_blocks=r, optimize=True)
    data = buf.getvalue()
    segs, start = O.segments(data)
    assert np.array_equal(O.spec_bytes(O.dht_tables(segs)), gold[key + "/dht"])
    assert hashlib.sha256(data[start:-2]).hexdigest() == str(gold[key + "/scan_sha256"])


# ------------------------------------------------------------------ 3
def _check_table(counts):
    bits, vals, depth = O.optimal_table(counts)
    used = [i for i, c in enumerate(counts[:256]) if c]
    assert len(bits) == 16 and sum(bits) == len(vals) and sorted(vals) == used              # every counted symbol, no other
    # Kraft with one slot of the longest length left free (the pseudo-symbol's all-ones code)
    longest = max(i + 1 for i, b in enumerate(bits) if b)
    assert sum(Fraction(b, 1 << (i + 1)) for i, b in enumerate(bits)) + Fraction(1, 1 << longest) <= 1
    codes = O.huff_codes(bits, vals)
    assert all(code < (1 << length) - 1 or length < longest for code, length in codes.values())
    assert all(code != (1 << length) - 1 for code, length in codes.values())               # no code is all ones
    if depth <= 16:                                                                         # unlimited: ascending symbols within a length
        k = 0
        for b in bits:
            assert vals[k:k + b] == sorted(vals[k:k + b])
            k += b
    return bits, vals, depth


def test_optimal_table_on_synthetic_counts():
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    counts = [0] * 257
    for i, f in enumerate(fib):
        counts[3 * i + 1] = f
    bits, vals, depth = _check_table(counts)
    assert depth >= 17 and max(i + 1 for i, b in enumerate(bits) if b) == 16               # 40 Fibonacci counts: a 40-deep chain
    assert counts[vals[0]] >= fib[-2] and counts[vals[-1]] == 1                             # the shortest code for one of the two commonest
    # one symbol: one code of length 1
    for sym in (0, 5, 255):
        counts = [0] * 257
        counts[sym] = 7
        assert _check_table(counts)[:2] == ([1] + [0] * 15, [sym])
    # two symbols: 1 + 2 bits; ties go to the larger symbol, so of two equals the SMALLER symbol gets the shorter code
    counts = [0] * 257
    counts[4] = counts[9] = 5
    bits, vals, _ = _check_table(counts)
    assert bits[:2] == [1, 1] and vals == [4, 9]
    # all 256 symbols equal: 9 bits would be needed for 257 leaves
    bits, vals, depth = _check_table([3] * 256)
    assert depth == 9 and sum(bits) == 256 and vals[:bits[7]] == sorted(vals[:bits[7]])
    # geometric counts in 256 symbols: deeper than 16 before limiting, 16 after
    bits, vals, depth = _check_table([1 << min(i, 28) for i in range(30)] + [1] * 226)
    assert depth > 16 and bits[15] > 0
    # slot 256 of a counts row is ignored
    assert O.optimal_table([2, 3] + [0] * 254 + [99])[:2] == O.optimal_table([2, 3] + [0] * 254)[:2]


# ------------------------------------------------------------------ 4
def test_optimised_scan_is_not_longer_on_the_rows(mirror):
    standard = {key: O.HUFF[key] for key in O.TABLE_KEYS}
    worse, total = 0, [0, 0]
    for key, (symbols, scan, tables, _) in mirror.items():
        a, b = O.scan_bits(symbols, tables), O.scan_bits(symbols, standard)
        worse += a > b
        total[0] += a
        total[1] += b
    print("bits optimised / standard over the rows:", total)
    assert worse == 0 and total[0] < total[1]


# ------------------------------------------------------------------ 5
def _huffman_arg(tables):
    return tuple((bytes(tables[k][0]), bytes(tables[k][1])) for k in O.TABLE_KEYS)


def test_header_with_tables_equals_pillows_segments(gold, mirror):
    from ccvs_amd.tools import mjpeg
    for key, name, s, q, r in O.rows():
        h, w = gold[name + "/in"].shape[:2]
        tables = mirror[key][2]
        head = mjpeg.jpeg_header(h, w, q, r, s, huffman=_huffman_arg(tables))
        assert head == mjpeg.jpeg_header(h, w, q, r, s, huffman=mjpeg.huffman_from_spec(O.spec_bytes(tables))), key
        ours, pil = O.segments(head + b"\xff\xd9")[0], O.segments(gold[key].tobytes())[0]
        assert pil[0][0] == 0xE0 and ours == pil[1:], key                                   # Pillow's file has a JFIF APP0 in front, nothing else differs
        # None: the standard tables, where they stood
        std = mjpeg.jpeg_header(h, w, q, r, s)
        assert std == mjpeg.jpeg_header(h, w, q, r, s, None) and [m for m, _ in O.segments(std + b"\xff\xd9")[0]] == [m for m, _ in ours]


def test_header_without_tables_gives_the_bytes_there_were(golden_dir):
    from ccvs_amd.tools import mjpeg
    import jpeg_ref as R
    import jpeg_sub_ref as S
    old = np.load(os.path.join(golden_dir, "mjpeg_cases.npz"))
    for key, name, q, r in R.rows():
        h, w = old[name + "/in"].shape[:2]
        pil = old[key].tobytes()
        assert pil[:2] + pil[20:O.segments(pil)[1]] == mjpeg.jpeg_header(h, w, q, r, huffman=None), key      # (SOI, then past the 18-byte APP0)
    sub = np.load(os.path.join(golden_dir, "mjpeg_sub_cases.npz"))
    for key, name, s, q, r in S.rows():
        h, w = sub[name + "/in"].shape[:2]
        pil = sub[key].tobytes()
        assert pil[:2] + pil[20:O.segments(pil)[1]] == mjpeg.jpeg_header(h, w, q, r, s, huffman=None), key


def test_files_open_in_pillow_with_the_standard_files_pixels(gold, mirror):
    pytest.importorskip("PIL")
    from ccvs_amd.tools import mjpeg
    import jpeg_sub_ref as S
    for key, name, s, q, r in O.rows()[::3]:
        img = gold[name + "/in"]
        h, w = img.shape[:2]
        _, scan, tables, _ = mirror[key]
        opt = mjpeg.jpeg_header(h, w, q, r, s, huffman=_huffman_arg(tables)) + scan + mjpeg.EOI
        std = mjpeg.jpeg_header(h, w, q, r, s) + S.encode_scan_sub(img, q, s, r) + mjpeg.EOI
        a, b = mjpeg.decode_frames([opt, std])
        assert np.array_equal(a, b), key
        parsed = mjpeg.parse_jpeg(opt)                                                      # and our own parser reads the tables back
        assert _same_tables({k: parsed["huffman"][k] for k in O.TABLE_KEYS}, tables), key


def test_header_refuses_malformed_tables():
    from ccvs_amd.tools import mjpeg
    good = tuple(mjpeg.HUFF[k] for k in (0x00, 0x10, 0x01, 0x11))
    assert mjpeg.jpeg_header(8, 8, 90, huffman=good) == mjpeg.jpeg_header(8, 8, 90)       # the Annex K tables in DHT order: the same bytes
    for bad in (good[:3], good + good[:1], ((good[0][0], good[0][1][:-1]),) + good[1:], ((good[0][0][:15], good[0][1]),) + good[1:]):
        with pytest.raises(ValueError, match="huffman"):
            mjpeg.jpeg_header(8, 8, 90, huffman=bad)
    with pytest.raises(ValueError, match="huffman_from_spec"):
        mjpeg.huffman_from_spec(np.zeros((3, 272), np.uint8))
    with pytest.raises(ValueError, match="huffman_from_spec"):
        mjpeg.huffman_from_spec(np.zeros((4, 271), np.uint8))


# ------------------------------------------------------------------ 6
def test_optimized_symbols_declared_and_exported(tmp_path):
    from ccvs_amd import lib
    header = open(os.path.join(ROOT, "include", "ccvs_hip_output_optimized.h")).read()
    assert re.search(r'^#include "ccvs_hip_output_optimized.h"', open(os.path.join(ROOT, "include", "ccvs_hip.h")).read(), re.M)
    declared = sorted(set(re.findall(r"^\w[\w \*]*?\b(ccvs_\w+)\(", header, re.M)))
    assert declared == sorted(lib.OUTPUT_OPTIMIZED_EXPORTS) == ["ccvs_mjpeg_encode_optimized", "ccvs_mjpeg_optimized_workspace_bytes"]
    others = (set(lib.EXPORTS) | set(lib.EVAL_EXPORTS) | set(lib.INPUT_EXPORTS) | set(lib.GEMM_EXPORTS) | set(lib.OUTPUT_EXPORTS) | set(lib.DECODE_EXPORTS)
              | set(lib.VIDEO_EXPORTS) | set(lib.OUTPUT_SAMPLED_EXPORTS) | set(lib.LPIPS_EXPORTS) | set(lib.FVD_EXPORTS))
    assert not set(lib.OUTPUT_OPTIMIZED_EXPORTS) & others and len(lib.EXPORTS) == 51
    assert lib.OUTPUT_SAMPLED_EXPORTS == ["ccvs_mjpeg_sampled_workspace_bytes", "ccvs_mjpeg_encode_sampled"]
    handle = ctypes.CDLL(lib.LIB_PATH)
    for sym in lib.OUTPUT_OPTIMIZED_EXPORTS:
        assert hasattr(handle, sym), sym
    c = tmp_path / "p.c"
    c.write_text('#include "ccvs_hip.h"\nvoid* p[] = {' + ", ".join("(void*)" + s for s in lib.OUTPUT_OPTIMIZED_EXPORTS) + "};\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "p.o")], check=True)
    L = lib.load()
    assert L.ccvs_abi_version() == 6
    ws, base = L.ccvs_mjpeg_optimized_workspace_bytes, L.ccvs_mjpeg_sampled_workspace_bytes
    # the standard encoder's workspace plus, per frame, 4 x 257 counts and 4 x 256 codes of 4 bytes
    for args in ((768, 256, 256, 2, 16), (16, 256, 256, 0, 32), (1, 24, 40, 1, 1), (3, 8, 8, 2, 1)):
        assert ws(*args) == base(*args) + args[0] * 8208, args
    assert ws(1, 8, 8, 3, 1) == 0 and ws(1, 8, 8, 2, 17) == 0 and ws(1, 8, 8, 0, 33) == 0 and ws(0, 8, 8, 2, 1) == 0
    # refused before any GPU call
    one = ctypes.c_void_p(16)
    call = lambda n, h, w, q, s, r, cap=64, stride=192: L.ccvs_mjpeg_encode_optimized(one, stride, n, h, w, q, s, r, one, cap, one, one, one, None)
    for args, word in (((1, 8, 8, 90, 3, 1), "sampling"), ((1, 8, 8, 90, -1, 1), "sampling"),
                       ((1, 8, 8, 90, 0, 33), "restart"), ((1, 8, 8, 90, 1, 25), "restart"), ((1, 8, 8, 90, 2, 17), "restart"), ((1, 8, 8, 90, 2, 0), "restart"),
                       ((1, 8, 8, 0, 2, 1), "quality"), ((1, 8, 8, 101, 1, 1), "quality"), ((1, 0, 8, 90, 2, 1), "size"), ((1, 8, 65536, 90, 1, 1), "size"),
                       ((1, 32768, 16384, 90, 0, 1), "2^28"),
                       ((0, 8, 8, 90, 2, 1), "frames"), ((1, 8, 8, 90, 2, 1, -1), "capacity"), ((2, 8, 8, 90, 1, 1, 64, -192), "stride")):
        assert call(*args) != 0, args
        msg = L.ccvs_last_error().decode()
        assert word in msg and "ccvs_mjpeg_encode_optimized" in msg, (args, msg)
    assert L.ccvs_mjpeg_encode_optimized(None, 192, 1, 8, 8, 90, 2, 1, one, 64, one, one, one, None) != 0 and "null" in L.ccvs_last_error().decode()
    assert L.ccvs_mjpeg_encode_optimized(one, 192, 1, 8, 8, 90, 2, 1, one, 64, one, None, one, None) != 0 and "null tables" in L.ccvs_last_error().decode()
    assert L.ccvs_mjpeg_encode_optimized(one, 192, 1, 8, 8, 90, 2, 1, one, 64, one, one, None, None) != 0 and "null" in L.ccvs_last_error().decode()


def test_ops_refuse_before_the_gpu():
    from ccvs_amd import lib, ops
    with pytest.raises(lib.CcvsError):
        ops.mjpeg_encode_optimized(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), sampling=2)
    with pytest.raises(lib.CcvsError):
        ops.mjpeg_encode_to_host(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 90, None, sampling=1, optimize=True)


# ------------------------------------------------------------------ 7
def _plain(v):
    return list(v) if isinstance(v, (list, tuple)) else v


def test_options(golden_dir):
    from ccvs_amd.tools.options import Options
    b = Options().parse(True, True, argv=TINY)["transformer"]
    assert b.video_optimize is False and b.video_format == "auto" and b.video_subsampling == "444"
    for argv, want in ((["--video_optimize"], True), (["--video_optimize", "true"], True), (["--video_optimize", "false"], False)):
        a = Options().parse(True, True, argv=TINY + ["--video_format", "avi"] + argv)["base"]
        assert a.video_optimize is want and a.video_format == "avi"
    assert Options().parse(True, True, argv=TINY + ["--video_optimize"])["base"].video_format == "auto"               # ignored there, not refused
    # every launch line of the reference still parses to the values the reference's own parser gives; the flag moves nothing else
    parse = lambda argv: Options().parse(True, True, load_state_estimator=True, load_stft_ae=True, argv=argv)
    with open(os.path.join(golden_dir, "reference_launch_lines.json")) as f:
        lines = json.load(f)
    with open(os.path.join(golden_dir, "reference_checks.json")) as f:
        parsed = json.load(f)["launch_lines"]
    assert len(lines) >= 9
    for script, argv in sorted(lines.items()):
        got, got_on = parse(argv), parse(argv + ["--video_optimize"])
        assert got["transformer"].video_optimize is False and got_on["transformer"].video_optimize is True
        for key in ("transformer", "qvid_generator"):
            for f in rh.LAUNCH_LINE_FIELDS[key]:
                if f in parsed[script][key]:
                    assert _plain(getattr(got[key], f)) == parsed[script][key][f], (script, key, f)
            a, b = vars(got[key]), vars(got_on[key])
            skip = lambda k: k in ("video_optimize", "signature") or k.endswith("_path")
            assert {k: v for k, v in a.items() if not skip(k)} == {k: v for k, v in b.items() if not skip(k)}, (script, key)


def test_save_results_passes_the_option_through(tmp_path, monkeypatch):
    """`Generator.save_results` hands --video_optimize to every `save_video_batch` call (no GPU: the call is recorded, not made)."""
    from ccvs_amd.helpers import generator as G
    seen = []
    monkeypatch.setattr(G, "save_video_batch", lambda *a, **k: seen.append((os.path.basename(a[3]), k["video_format"], k["subsampling"], k["optimize"])))
    opt = types.SimpleNamespace(video_format="avi", video_quality=80, video_subsampling="420", video_optimize=True, result_path=str(tmp_path), fps=4,
                                imagenet_norm=False, dataset="bairhd", state=True)
    me = types.SimpleNamespace(opt=opt, decode_stft=False)
    vid = torch.zeros(2, 2, 3, 8, 8)
    G.Generator.save_results(me, {"real": vid, "fake": {"vid": vid, "state": torch.zeros(2, 2, 2)}, "rec": {"vid": vid}}, 0)
    assert seen == [("real", "avi", "420", True), ("fake", "avi", "420", True), ("fake_state", "avi", "420", True), ("rec", "avi", "420", True)]
    seen.clear()
    del opt.video_optimize                                          # an options object from before the flag: standard tables
    G.Generator.save_results(me, {"real": vid}, 0)
    assert seen == [("real", "avi", "420", False)]


def test_other_formats_do_not_look_at_optimize(tmp_path, monkeypatch):
    from ccvs_amd.helpers import generator as G
    monkeypatch.setattr(G.ops, "mjpeg_encode_to_host", lambda *a, **k: pytest.fail("the .npy files need no encoder"))
    monkeypatch.setattr(G.ops, "pack_u8", lambda v, lo, hi: ((v.clamp(lo, hi) - lo) / (hi - lo) * 255).permute(0, 1, 3, 4, 2).to(torch.uint8))
    vid = torch.zeros(1, 2, 3, 8, 8)
    a = G.save_video_batch(vid, 1, 0, str(tmp_path / "a"), 4, True, False, [-1, 1], "bairhd", video_format="npy", optimize=True)
    b = G.save_video_batch(vid, 1, 0, str(tmp_path / "b"), 4, True, False, [-1, 1], "bairhd", video_format="npy")
    assert torch.equal(a, b) and open(tmp_path / "a" / "vid_00000.npy", "rb").read() == open(tmp_path / "b" / "vid_00000.npy", "rb").read()

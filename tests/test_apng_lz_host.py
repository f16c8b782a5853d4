"""The lossless output stage with LZ77 matches, host side -- no GPU.

  1. the spec mirror tests/apng_lz_ref.py against zlib's inflate on every row of its table: each stream inflates completely (zlib checks
     the Adler-32) to the filtered bytes;
  2. `write_apng` + Pillow and `read_apng` give the pixels;
  3. no row's stream is longer than `apng_ref`'s (the literal-only stream of the default writer);
  4. where the mirror chose literal-only for every band the stream IS `apng_ref`'s: the noise rows and `period_32769`;
  5. structure: the tokens of a flat frame, every token list replayed, distances within the window and the frame, no match across a
     band's end, matches at exactly 32768, the length cap, the run cut at a band's end;
  6. strictly smaller than Huffman-only on the frames with runs (the distance-1 candidate finds what zlib's Z_RLE finds);
  7. the size table of DESIGN.md, printed: mirror against zlib Huffman-only, Z_RLE, level 1 and level 6;
  8. the ABI: `lib.OUTPUT_LOSSLESS_LZ_EXPORTS` = what include/ccvs_hip_output_lossless_lz.h declares = exported, disjoint from every
     other list, EXPORTS and the ABI version unmoved, refusals by name before any launch, the workspace size;
  9. `--video_lz77`, the reference's launch lines, `save_results` passing it on, CPU tensors refused.
"""
import ctypes
import json
import os
import re
import subprocess
import sys
import types
import zlib

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import apng_lz_ref as Z  # noqa: E402
import apng_ref as R  # noqa: E402
import ref_harness as rh  # noqa: E402
from tests.test_mjpeg_host import TINY  # noqa: E402

RUNS = ("zeros", "ones", "hramp", "vramp", "mixed")                    # contents whose filtered bytes hold runs


def inflate(stream):
    d = zlib.decompressobj()
    out = d.decompress(stream)
    assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b""
    return out


def plain(key, name, flt, r):
    """`apng_ref`'s stream of a row: what the default writer gives for the same frame, filter and bands."""
    return R.encode_frame(Z.images()[name], flt, r)["stream"]


@pytest.fixture(scope="module")
def table():
    """{key: (mirror, apng_ref's stream)} of every row, computed once."""
    return {key: (Z.mirrored(key), plain(key, name, flt, r)) for key, name, flt, r in Z.rows()}


# ------------------------------------------------------------------ 1, 3, 4
def test_table_is_what_the_tests_need():
    rows = Z.rows()
    keys = [row[0] for row in rows]
    assert len(set(keys)) == len(keys)
    for h, w in Z.TABLE_SIZES:
        for name in ("zeros", "ones", "hramp", "vramp", "dramp", "noise", "smooth", "mixed"):
            for flt in (-1, 0, 4):
                assert {row[3] for row in rows if row[1] == f"{name}_{h}x{w}" and row[2] == flt} == {1, h, 0}
    for key in ("smooth_256x256/f-1/b0", "noise_256x256/f-1/b0", "period_32768/f0/b1", "period_32769/f0/b1", "run_517/f0/b1", "run_to_band_end/f0/b1"):
        assert key in keys
    assert Z.images()["period_32768"].shape == (1, 21846, 3)


def test_mirror_streams_inflate_and_are_no_longer(table):
    smaller = 0
    for key, name, flt, r in Z.rows():
        m, ref = table[key]
        img = Z.images()[name]
        rows, _ = R.filter_rows(img, flt)
        assert m["filtered"] == rows.tobytes(), key
        assert inflate(m["stream"]) == m["filtered"], key
        assert m["stream"][:2] == b"\x78\x01" and len(m["choice"]) == len(m["tokens"]) == m["bands"] == len(R.band_cut(*img.shape[:2], r)), key
        assert len(m["stream"]) <= len(ref), (key, len(m["stream"]), len(ref))
        if all(c == "literal" for c in m["choice"]):
            assert m["stream"] == ref, key
        smaller += len(m["stream"]) < len(ref)
    assert smaller > 100
    for key, name, flt, r in Z.rows():
        if name.startswith("noise") or name == "period_32769":
            m, ref = table[key]
            assert set(m["choice"]) == {"literal"} and m["stream"] == ref, key


# ------------------------------------------------------------------ 2
def test_files_open_in_pillow_and_read_apng(tmp_path, table):
    Image = pytest.importorskip("PIL.Image")
    from ccvs_amd.tools import apng
    for key, name, flt, r in Z.rows():
        img = Z.images()[name]
        h, w = img.shape[:2]
        if (flt, r) != (-1, 0) and h * w > 64 * 64:
            continue
        path = str(tmp_path / "a.png")
        z = table[key][0]["stream"]
        apng.write_apng(path, [z, z], 4, h, w)
        assert np.array_equal(apng.read_apng(path), np.stack([img, img])), key
        with Image.open(path) as im:
            assert im.n_frames == 2
            im.seek(1)
            assert np.array_equal(np.asarray(im.convert("RGB")), img), key


# ------------------------------------------------------------------ 5
def test_flat_frame_tokens():
    m = Z.mirrored("zeros_64x64/f0/b64")
    assert m["choice"] == ["lz"] and m["tokens"] == [[0] + [(258, 1)] * 47 + [(225, 1)]]


def test_tokens_replay_and_stay_in_bounds(table):
    for key, name, flt, r in Z.rows():
        m = table[key][0]
        img = Z.images()[name]
        h, w = img.shape[:2]
        f = m["filtered"]
        for (r0, r1), toks in zip(R.band_cut(h, w, r), m["tokens"]):
            s, e = r0 * (3 * w + 1), r1 * (3 * w + 1)
            assert Z.replay(toks, f[:s]) == f[s:e], key                # (a match across the band's end would overshoot)
            p = s
            for t in toks:
                if isinstance(t, tuple):
                    assert 3 <= t[0] <= 258 and 1 <= t[1] <= min(32768, p) and p + t[0] <= e and (t[0] > 3 or t[1] <= 4096), (key, p, t)
                    p += t[0]
                else:
                    p += 1
            assert p == e, key


def test_constructed_rows():
    far = [t for t in Z.mirrored("period_32768/f0/b1")["tokens"][0] if isinstance(t, tuple)]
    assert far and all(t[1] == 32768 for t in far) and max(t[0] for t in far) == 258
    assert not [t for t in Z.mirrored("period_32769/f0/b1")["tokens"][0] if isinstance(t, tuple)]
    run = Z.mirrored("run_517/f0/b1")["tokens"][0]
    at = run.index((258, 1))
    assert run[at - 1:at + 2] == [77, (258, 1), (258, 1)] and not isinstance(run[at + 2], tuple)
    a, b = Z.mirrored("run_to_band_end/f0/b1")["tokens"]
    assert a[-1] == (29, 1) and a[-2] == 0                             # the run's 30 bytes in the first band: a literal and the match cut at its end
    assert b[0] == (61, 1)                                             # the second band's first token looks back into the first band
    cross = Z.mirrored("mixed_64x64/f0/b1")                            # band_rows 1: the byte above is in the band before
    assert any(isinstance(t, tuple) and t[1] == 193 for toks in cross["tokens"][1:] for t in toks)


# ------------------------------------------------------------------ 6, 7
def test_strictly_smaller_where_there_are_runs(table):
    for key, name, flt, r in Z.rows():
        content, size = name.rsplit("_", 1)
        if content in RUNS and size in ("33x65", "64x64"):
            assert len(table[key][0]["stream"]) < len(table[key][1]), key


def test_size_table(table):
    """Recorded for DESIGN.md section 4.24, not asserted: bytes per frame, adaptive filter, default bands."""
    def z(data, level, strategy):
        c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
        return len(c.compress(data) + c.flush())
    print(f"\n{'frame':<18}{'default':>9}{'lz77':>9}{'huffman':>9}{'rle':>9}{'level 1':>9}{'level 6':>9}")
    names = [f"{c}_64x64" for c in ("zeros", "ones", "hramp", "vramp", "dramp", "mixed", "smooth", "noise")] + ["smooth_256x256", "noise_256x256"]
    for name in names:
        m, ref = table[f"{name}/f-1/b0"]
        d = m["filtered"]
        print(f"{name:<18}{len(ref):>9}{len(m['stream']):>9}{z(d, 6, zlib.Z_HUFFMAN_ONLY):>9}{z(d, 6, zlib.Z_RLE):>9}{z(d, 1, 0):>9}{z(d, 6, 0):>9}")


# ------------------------------------------------------------------ 8
def test_lz_symbols_declared_and_exported(tmp_path):
    from ccvs_amd import lib
    header = open(os.path.join(ROOT, "include", "ccvs_hip_output_lossless_lz.h")).read()
    assert re.search(r'^#include "ccvs_hip_output_lossless_lz.h"', open(os.path.join(ROOT, "include", "ccvs_hip.h")).read(), re.M)
    declared = sorted(set(re.findall(r"^\w[\w \*]*?\b(ccvs_\w+)\(", header, re.M)))
    assert declared == sorted(lib.OUTPUT_LOSSLESS_LZ_EXPORTS) == ["ccvs_apng_encode_lz", "ccvs_apng_lz_workspace_bytes"]
    others = set()
    for name in dir(lib):
        if name.endswith("EXPORTS") and name != "OUTPUT_LOSSLESS_LZ_EXPORTS":
            others |= set(getattr(lib, name))
    assert others >= set(lib.EXPORTS) | set(lib.OUTPUT_LOSSLESS_EXPORTS) | set(lib.DECODE_LOSSLESS_EXPORTS) and not set(lib.OUTPUT_LOSSLESS_LZ_EXPORTS) & others and len(lib.EXPORTS) == 51
    handle = ctypes.CDLL(lib.LIB_PATH)
    for sym in lib.OUTPUT_LOSSLESS_LZ_EXPORTS:
        assert hasattr(handle, sym), sym
    c = tmp_path / "p.c"
    c.write_text('#include "ccvs_hip.h"\nvoid* p[] = {' + ", ".join("(void*)" + s for s in lib.OUTPUT_LOSSLESS_LZ_EXPORTS) + "};\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "p.o")], check=True)
    assert lib.load().ccvs_abi_version() == 6


def test_sizes_and_refusals_before_any_launch(table):
    from ccvs_amd import lib
    L = lib.load()
    ws, ws_plain, bound = L.ccvs_apng_lz_workspace_bytes, L.ccvs_apng_workspace_bytes, L.ccvs_apng_stream_bound
    for n, h, w, r in ((256, 256, 256, 0), (1, 17, 23, 1), (3, 33, 65, 32), (2, 1, 1, 0), (5, 64, 64, 2)):
        rows = r or max(1, 32768 // (3 * w + 1))
        bands = -(-h // rows)
        filt = n * h * (3 * w + 1)
        assert ws(n, h, w, r) == n * bands * 2984 + (4 * n + 7) // 8 * 8 + (filt + 7) // 8 * 8 + 4 * filt >= ws_plain(n, h, w, r), (n, h, w, r)
    for args in ((0, 8, 8, 0), (1, 0, 8, 0), (1, 8, 0, 0), (1, 65536, 8, 0), (1, 8, 65536, 0), (1, 8, 8, -1), (1, 65535, 65535, 65535)):
        assert ws(*args) == 0, args
    one = ctypes.c_void_p(16)
    call = lambda n, h, w, f, r, cap=64, stride=192: L.ccvs_apng_encode_lz(one, stride, n, h, w, f, r, one, cap, one, one, None)
    for args, word in (((0, 8, 8, -1, 0), "frames"), ((-1, 8, 8, -1, 0), "frames"), ((1, 0, 8, -1, 0), "size"), ((1, 8, 65536, -1, 0), "size"),
                       ((1, 65536, 8, 0, 0), "size"), ((1, 8, 8, -2, 0), "filter"), ((1, 8, 8, 5, 0), "filter"), ((1, 8, 8, -1, -1), "band_rows"),
                       ((1, 65535, 65535, -1, 65535, 64, 1 << 40), "band_rows"), ((1, 8, 8, -1, 0, -1), "capacity"), ((1, 8, 8, -1, 0, 64, 191), "stride"),
                       ((2, 8, 8, -1, 0, 64, -192), "stride")):
        assert call(*args) != 0, args
        msg = L.ccvs_last_error().decode()
        assert word in msg and "ccvs_apng_encode_lz" in msg, (args, msg)
    for k in (0, 7, 9, 10):                                            # rgb, stream (with a capacity), offsets, workspace
        argv = [one, 192, 1, 8, 8, -1, 0, one, 64, one, one, None]
        argv[k] = None
        assert L.ccvs_apng_encode_lz(*argv) != 0 and "null" in L.ccvs_last_error().decode(), k
    # `ccvs_apng_stream_bound` remains the bound
    for key, name, flt, r in Z.rows():
        h, w = Z.images()[name].shape[:2]
        assert bound(1, h, w, r) >= len(table[key][1]) >= len(table[key][0]["stream"]), key


# ------------------------------------------------------------------ 9
def _plain(v):
    return list(v) if isinstance(v, (list, tuple)) else v


def test_options(golden_dir):
    from ccvs_amd.tools.options import Options
    b = Options().parse(True, True, argv=TINY)["transformer"]
    assert b.video_lz77 is False and b.video_format == "auto"
    for argv, want in ((["--video_lz77"], True), (["--video_lz77", "true"], True), (["--video_lz77", "false"], False)):
        a = Options().parse(True, True, argv=TINY + ["--video_format", "apng"] + argv)["base"]
        assert a.video_lz77 is want and a.video_format == "apng"
    for fmt in ("auto", "npy", "avi"):                                 # ignored there, not refused
        assert Options().parse(True, True, argv=TINY + ["--video_format", fmt, "--video_lz77"])["base"].video_format == fmt
    parse = lambda argv: Options().parse(True, True, load_state_estimator=True, load_stft_ae=True, argv=argv)
    with open(os.path.join(golden_dir, "reference_launch_lines.json")) as f:
        lines = json.load(f)
    with open(os.path.join(golden_dir, "reference_checks.json")) as f:
        parsed = json.load(f)["launch_lines"]
    assert len(lines) >= 9
    for script, argv in sorted(lines.items()):
        got, got_on = parse(argv), parse(argv + ["--video_lz77"])
        assert got["transformer"].video_lz77 is False and got_on["transformer"].video_lz77 is True
        for key in ("transformer", "qvid_generator"):
            for f in rh.LAUNCH_LINE_FIELDS[key]:
                if f in parsed[script][key]:
                    assert _plain(getattr(got[key], f)) == parsed[script][key][f], (script, key, f)
            a, b = vars(got[key]), vars(got_on[key])
            skip = lambda k: k in ("video_lz77", "signature") or k.endswith("_path")
            assert {k: v for k, v in a.items() if not skip(k)} == {k: v for k, v in b.items() if not skip(k)}, (script, key)


def test_save_results_passes_lz77_through(tmp_path, monkeypatch):
    from ccvs_amd.helpers import generator as G
    seen = []
    monkeypatch.setattr(G, "save_video_batch", lambda *a, **k: seen.append((os.path.basename(a[3]), k["video_format"], k["lz77"])))
    opt = types.SimpleNamespace(video_format="apng", video_quality=80, video_subsampling="444", video_optimize=False, video_lz77=True, result_path=str(tmp_path),
                                fps=4, imagenet_norm=False, dataset="bairhd", state=True)
    me = types.SimpleNamespace(opt=opt, decode_stft=False)
    vid = torch.zeros(2, 2, 3, 8, 8)
    G.Generator.save_results(me, {"real": vid, "fake": {"vid": vid, "state": torch.zeros(2, 2, 2)}, "rec": {"vid": vid}}, 0)
    assert seen == [(k, "apng", True) for k in ("real", "fake", "fake_state", "rec")]
    seen.clear()
    del opt.video_lz77                                                 # an options object from before the flag
    G.Generator.save_results(me, {"real": vid}, 0)
    assert seen == [("real", "apng", False)]


def test_other_formats_do_not_look_at_lz77(tmp_path, monkeypatch):
    from ccvs_amd.helpers import generator as G
    monkeypatch.setattr(G.ops, "png_encode_to_host", lambda *a, **k: pytest.fail("the .npy files need no encoder"))
    monkeypatch.setattr(G.ops, "pack_u8", lambda v, lo, hi: ((v.clamp(lo, hi) - lo) / (hi - lo) * 255).permute(0, 1, 3, 4, 2).to(torch.uint8))
    vid = torch.rand(1, 2, 3, 8, 8) * 2 - 1
    a = G.save_video_batch(vid, 1, 0, str(tmp_path / "a"), 4, True, False, [-1, 1], "bairhd", video_format="npy", lz77=True)
    b = G.save_video_batch(vid, 1, 0, str(tmp_path / "b"), 4, True, False, [-1, 1], "bairhd", video_format="npy")
    assert np.array_equal(a.numpy(), b.numpy())
    assert open(tmp_path / "a" / "vid_00000.npy", "rb").read() == open(tmp_path / "b" / "vid_00000.npy", "rb").read()


def test_cpu_tensors_are_refused(tmp_path):
    from ccvs_amd import lib, ops
    from ccvs_amd.helpers.generator import save_video_batch
    with pytest.raises(lib.CcvsError):
        ops.png_encode(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), lz77=True)
    with pytest.raises(lib.CcvsError):
        ops.png_encode_to_host(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), 0, 1, lz77=True)
    with pytest.raises(lib.CcvsError):
        save_video_batch(torch.zeros(1, 2, 3, 8, 8), 1, 0, str(tmp_path / "a"), 4, True, False, [-1, 1], "bairhd", video_format="apng", lz77=True)

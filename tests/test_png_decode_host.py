"""not gpu: the PNG decoder's host side.

  1. the spec mirror tests/png_decode_ref.py equals `zlib.decompress` on every plain stream: filtered images 1 x 1 .. 65 x 67 (flat,
     tiled, smooth plus noise, noise), row-periodic frames and the planted buffer at levels 0, 1, 6, 9 and with Z_FIXED, Z_RLE and
     Z_HUFFMAN_ONLY; the encoder mirror's streams (adaptive filter, every band_rows); a stored stream of several blocks; wbits = 9;
  2. the planted buffer's level-9 and Z_FIXED streams use all 29 length codes and all 30 distance codes, hundreds of overlapping copies,
     matches of 258 and distances beyond 32,000 -- asserted from the mirror's statistics, so that a zlib that loses it fails loudly;
  3. hand-assembled streams (a match at distance 32768, distance = produced bytes and one more, block type 3, LEN / NLEN, symbols 286 and
     30, over-subscribed, incomplete, a single 1-bit distance code, no end-of-block, a repeat with nothing before it, HLIT = 287, FDICT,
     FCHECK, Adler-32, one byte more or less than expected, garbage behind the Adler-32): the stated status word, zero exactly where
     `zlib.decompress` succeeds with the expected length;
  4. 2000 deterministic mutations: the mirror's status is zero exactly where zlib accepts with the expected length, equal bytes there;
     the histogram is printed and holds at least 5 of OK, BAD_TABLE, BAD_CODE, BAD_DISTANCE, OVERRUN and BAD_CHECK -- by zlib's own
     messages too;
  5. `apng_streams` on `write_apng`'s files and on Pillow's PNG / APNG files: `zlib.decompress` + `unfilter` of its streams equals
     `read_apng`; the header probe on each refused kind;
  6. the ABI: declared = exported = `lib.DECODE_LOSSLESS_EXPORTS`, disjoint from every other list, 51 / ABI 6 unchanged, a C file
     including ccvs_hip.h alone compiles with -Wall -Werror, every refusal by its cause;
  7. `--png_decode` defaults to host and leaves the reference launch lines as they parse; `load_videos(png_decode="gpu")` calls
     `ops.read_apng_clips`; `FrameDataset.decode` falls back per item.
"""
import collections
import ctypes
import io
import json
import os
import re
import struct
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
import apng_ref as R  # noqa: E402
import png_decode_ref as D  # noqa: E402
import ref_harness as rh  # noqa: E402
from tests.test_mjpeg_host import TINY  # noqa: E402


# ------------------------------------------------------------------ 1
def test_mirror_equals_zlib_on_plain_streams():
    plain, judged = D.plain_streams(), D.judged("plain")
    names = [n for n, _, _ in plain]
    assert len(set(names)) == len(names) >= 300
    for cfg, _, _ in D.CONFIGS:
        assert sum(n.endswith("/" + cfg) for n in names) == len(D.filtered_images()) + 1 + (cfg == "l0"), cfg    # (+ the planted buffer; + the stored stream)
    assert {n.rsplit("/", 1)[1] for n in names if n.startswith("apng_ref/noise_64x64")} == {"b1", "b2", "b63", "b64", "b0"}
    for (name, stream, raw), (_, _, expect, status, out) in zip(plain, judged):
        assert zlib.decompress(stream) == raw and expect == len(raw), name
        assert status == D.OK and out == raw, (name, D.NAMES[status])
    st = D.new_stats()
    stored = next(s for n, s, _ in plain if n == "stored_150001/l0")
    assert D.inflate(stored, 150001, st)[0] == D.OK and st["blocks"][0] >= 3 and st["blocks"][1:] == [0, 0]
    assert next(s for n, s, _ in plain if n.endswith("wbits9"))[0] == 0x18                          # CINFO 1: a 512-byte window
    kinds = [0, 0, 0]
    for name, stream, raw in plain:
        if len(stream) < 3000:
            st = D.new_stats()
            D.inflate(stream, len(raw), st)
            kinds = [a + b for a, b in zip(kinds, st["blocks"])]
    print("blocks of the small streams: stored, fixed, dynamic =", kinds)
    assert min(kinds) >= 20


# ------------------------------------------------------------------ 2
def test_planted_buffer_covers_every_code():
    raw = D.planted()
    assert len(raw) == 148785
    for cfg in ("l9", "fixed"):
        stream = next(s for n, s, _ in D.plain_streams() if n == "planted/" + cfg)
        st = D.new_stats()
        status, out = D.inflate(stream, len(raw), st)
        print(cfg, {k: (len(v) if isinstance(v, set) else v) for k, v in st.items()})
        assert status == D.OK and out == raw
        assert st["length_codes"] == set(range(29)) and st["distance_codes"] == set(range(30)), cfg
        assert st["overlapping"] >= 500 and st["longest"] == 258 and st["largest_distance"] >= 32000, cfg
        assert st["blocks"][1 if cfg == "fixed" else 2] >= 1


# ------------------------------------------------------------------ 3
def test_hand_assembled_streams():
    hand = D.hand_streams()
    names = [h[0] for h in hand]
    for must in ("distance_32768", "distance_all_produced", "distance_one_before", "block_type_3", "len_nlen", "symbol_286", "distance_symbol_30", "oversubscribed",
                 "incomplete", "single_distance_code", "no_end_of_block", "repeat_without_previous", "hlit_287", "fdict", "fcheck", "adler", "expected_one_more",
                 "expected_one_less", "garbage_behind"):
        assert must in names, must
    st = D.new_stats()
    far = hand[names.index("distance_32768")]
    assert D.inflate(far[1], far[2], st)[0] == D.OK and st["largest_distance"] == 32768
    for (name, stream, expect, want), (_, _, _, status, out) in zip(hand, D.judged("hand")):
        accepted, info = D.zlib_verdict(stream, expect)
        assert status == want, (name, D.NAMES[status], D.NAMES[want])
        assert (status == D.OK) == accepted, (name, D.NAMES[status], info)
        if accepted:
            assert out == info, name


# ------------------------------------------------------------------ 4
ZLIB_WORDS = {"invalid distance too far back": "BAD_DISTANCE", "incorrect data check": "BAD_CHECK", "incomplete or truncated stream": "OVERRUN",
              "invalid code lengths set": "BAD_TABLE", "invalid bit length repeat": "BAD_TABLE", "too many length or distance symbols": "BAD_TABLE",
              "invalid literal/lengths set": "BAD_TABLE", "invalid distances set": "BAD_TABLE", "invalid code -- missing end-of-block": "BAD_TABLE",
              "invalid literal/length code": "BAD_CODE", "invalid distance code": "BAD_CODE"}


def test_mutations_agree_with_zlib():
    judged = D.judged("mutations")
    assert len(judged) == 2000
    seen, by_zlib = collections.Counter(), collections.Counter()
    for name, stream, expect, status, out in judged:
        accepted, info = D.zlib_verdict(stream, expect)
        assert (status == D.OK) == accepted, (name, D.NAMES[status], info if isinstance(info, str) else len(info))
        if accepted:
            assert out == info, name
        seen[D.NAMES[status]] += 1
        by_zlib["OK" if accepted else ZLIB_WORDS.get(info.split(": ", 1)[-1], "other") if isinstance(info, str) else "wrong size"] += 1
    print("mirror's statuses over the mutations:", dict(seen))
    print("zlib's verdicts over the mutations:", dict(by_zlib))
    for word in ("OK", "BAD_TABLE", "BAD_CODE", "BAD_DISTANCE", "OVERRUN", "BAD_CHECK"):
        assert seen[word] >= 5 and by_zlib[word] >= 5, word


# ------------------------------------------------------------------ 5
def test_container_streams_and_probe(tmp_path):
    from ccvs_amd.tools import apng
    z = [R.mirrored(k)["stream"] for k in ("smooth_8x8/f-1/b0", "noise_8x8/f-1/b1", "mixed_8x8/f-1/b2")]
    path = str(tmp_path / "own.png")
    apng.write_apng(path, z, 4, 8, 8)
    h, w, streams = apng.apng_streams(path)
    assert (h, w) == (8, 8) and streams == [bytes(s) for s in z]
    assert apng.apng_streams(open(path, "rb").read()) == (h, w, streams)
    assert np.array_equal(apng.unfilter([zlib.decompress(s) for s in streams], h, w), apng.read_apng(path))
    assert apng.png_gpu_decodable(path) and not apng.png_gpu_decodable(str(tmp_path / "absent.png"))
    with pytest.raises(ValueError, match="signature"):
        apng.apng_streams(b"not a png")
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(4)
    frames = [np.clip(R.images()["smooth_33x65"].astype(int) + rng.integers(-3, 4, (33, 65, 3)), 0, 255).astype(np.uint8) for _ in range(3)]
    one, anim = str(tmp_path / "pil.png"), str(tmp_path / "pil_anim.png")
    Image.fromarray(frames[0]).save(one)
    Image.fromarray(frames[0]).save(anim, save_all=True, append_images=[Image.fromarray(f) for f in frames[1:]], default_image=False, disposal=0, blend=0)
    for p, want in ((one, frames[:1]), (anim, frames)):                 # (noisy frames: Pillow finds no smaller box to write, every frame is whole)
        clip = apng.read_apng(p)
        h, w, streams = apng.apng_streams(p)
        assert np.array_equal(apng.unfilter([zlib.decompress(s) for s in streams], h, w), clip)
        assert np.array_equal(clip, np.stack(want))
        st = D.new_stats()
        assert all(D.inflate(s, h * (3 * w + 1), st)[0] == D.OK for s in streams) and st["matches"] > 0      # Pillow's streams hold LZ77 matches
        assert apng.png_gpu_decodable(p)
    # the header probe on each kind the GPU path does not take
    for mode in ("RGBA", "P", "L", "I;16"):
        img = Image.fromarray(frames[0]).convert("L").convert(mode) if mode == "I;16" else Image.fromarray(frames[0]).convert(mode)
        img.save(str(tmp_path / "other.png"))
        assert not apng.png_gpu_decodable(str(tmp_path / "other.png")), mode
    head = bytearray(open(one, "rb").read()[:33])
    head[28] = 1                                                        # interlace
    (tmp_path / "interlaced.png").write_bytes(bytes(head))
    (tmp_path / "short.png").write_bytes(bytes(head[:20]))
    np.save(str(tmp_path / "frame.npy"), frames[0])
    for name in ("interlaced.png", "short.png", "frame.npy"):
        assert not apng.png_gpu_decodable(str(tmp_path / name)), name


# ------------------------------------------------------------------ 6
def test_decode_lossless_symbols_declared_and_exported(tmp_path):
    from ccvs_amd import lib
    header = open(os.path.join(ROOT, "include", "ccvs_hip_decode_lossless.h")).read()
    main = open(os.path.join(ROOT, "include", "ccvs_hip.h")).read()
    assert re.search(r'^#include "ccvs_hip_decode_lossless.h"', main, re.M) and not re.search(r"ccvs_(png_decode|zlib_inflate)", main)
    declared = sorted(set(re.findall(r"^\w[\w \*]*?\b(ccvs_\w+)\(", header, re.M)))
    assert declared == sorted(lib.DECODE_LOSSLESS_EXPORTS) == ["ccvs_png_decode", "ccvs_png_decode_workspace_bytes", "ccvs_zlib_inflate"]
    others = (set(lib.EXPORTS) | set(lib.EVAL_EXPORTS) | set(lib.INPUT_EXPORTS) | set(lib.GEMM_EXPORTS) | set(lib.OUTPUT_EXPORTS) | set(lib.DECODE_EXPORTS)
              | set(lib.VIDEO_EXPORTS) | set(lib.OUTPUT_SAMPLED_EXPORTS) | set(lib.OUTPUT_OPTIMIZED_EXPORTS) | set(lib.LPIPS_EXPORTS) | set(lib.FVD_EXPORTS)
              | set(lib.OUTPUT_LOSSLESS_EXPORTS))
    assert not set(lib.DECODE_LOSSLESS_EXPORTS) & others and len(lib.EXPORTS) == 51
    handle = ctypes.CDLL(lib.LIB_PATH)
    for sym in lib.DECODE_LOSSLESS_EXPORTS:
        assert hasattr(handle, sym), sym
    c = tmp_path / "p.c"
    c.write_text('#include "ccvs_hip.h"\nvoid* p[] = {' + ", ".join("(void*)" + s for s in lib.DECODE_LOSSLESS_EXPORTS) + "};\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "p.o")], check=True)
    assert lib.load().ccvs_abi_version() == 6
    assert open(os.path.join(ROOT, "ccvs_amd", "csrc", "Makefile")).read().count("ccvs_hip_decode_lossless.h") == 1
    from ccvs_amd import ops
    core = open(os.path.join(ROOT, "ccvs_amd", "csrc", "png_decode_core.h")).read()
    words = dict((name, int(v)) for name, v in re.findall(r"^#define PD_([A-Z_]+) (\d+)\s", core, re.M) if name in D.NAMES)
    assert words == {n: i for i, n in enumerate(D.NAMES)} == {v[0]: k for k, v in ops.PD_STATUS.items()}
    assert all(getattr(ops, "PD_" + n) == i for i, n in enumerate(D.NAMES))


def test_refusals_before_any_launch():
    from ccvs_amd import lib
    L = lib.load()
    ws = L.ccvs_png_decode_workspace_bytes
    for n, h, w in ((256, 256, 256), (1, 1, 1), (3, 33, 65), (2, 65535, 7)):
        assert ws(n, h, w) == (n * h * (3 * w + 1) + 15) // 16 * 16, (n, h, w)
    for args in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, 65536, 8), (1, 8, 65536)):
        assert ws(*args) == 0, args
    one = ctypes.c_void_p(16)
    table = lambda *rows: np.ascontiguousarray(rows, dtype=np.int64)
    host = lambda t: t.ctypes.data_as(ctypes.c_void_p)
    err = lambda: L.ccvs_last_error().decode()
    # ccvs_zlib_inflate(data, data_bytes, rows, rows_host, n, out, out_bytes, status, stream)
    good = table((0, 10, 0, 20), (10, 6, 20, 12))
    inflate = lambda rows=good, n=2, data_bytes=16, out_bytes=32: L.ccvs_zlib_inflate(one, data_bytes, one, host(rows), n, one, out_bytes, one, None)
    for kw, word in ((dict(n=0), "0 streams"), (dict(n=-3), "-3 streams"), (dict(data_bytes=-1), "negative length"), (dict(out_bytes=-1), "negative length"),
                     (dict(data_bytes=15), "stream 1 (bytes 10 + 6) points outside the data of 15"), (dict(out_bytes=31), "stream 1 (output bytes 20 + 12) points outside the output of 31"),
                     (dict(rows=table((-1, 4, 0, 4), (0, 0, 0, 0))), "stream 0 (bytes -1 + 4)"), (dict(rows=table((0, 4, 0, 4), (0, -4, 0, 0))), "stream 1 (bytes 0 + -4)"),
                     (dict(rows=table((0, 4, -2, 4), (0, 0, 0, 0))), "stream 0 (output bytes -2 + 4)"), (dict(rows=table((0, 4, 0, 4), (0, 4, 0, -1))), "stream 1 (output bytes 0 + -1)"),
                     (dict(rows=table((1 << 62, 1 << 62, 0, 4), (0, 0, 0, 0))), "stream 0 (bytes")):
        assert inflate(**kw) != 0, kw
        assert word in err() and "ccvs_zlib_inflate" in err(), (kw, err())
    for k in (0, 2, 3, 5, 7):                                           # data, table, host table, output, status
        argv = [one, 16, one, host(good), 2, one, 32, one, None]
        argv[k] = None
        assert L.ccvs_zlib_inflate(*argv) != 0 and "null" in err(), k
    for k in (2, 7):
        argv = [one, 16, one, host(good), 2, one, 32, one, None]
        argv[k] = ctypes.c_void_p(18)
        assert L.ccvs_zlib_inflate(*argv) != 0 and "misaligned" in err(), k
    # ccvs_png_decode(data, data_bytes, rows, rows_host, n, h, w, rgb, frame_stride, status, workspace, stream)
    good = table((0, 10), (10, 6))
    decode = lambda rows=good, n=2, h=8, w=8, data_bytes=16, stride=192: L.ccvs_png_decode(one, data_bytes, one, host(rows), n, h, w, one, stride, one, one, None)
    for kw, word in ((dict(n=0), "0 frames"), (dict(h=0), "frame size 0 x 8"), (dict(w=0), "frame size 8 x 0"), (dict(h=65536), "frame size"), (dict(w=65536), "frame size"),
                     (dict(data_bytes=-1), "negative length"), (dict(stride=191), "frame stride"), (dict(stride=-192), "frame stride"),
                     (dict(data_bytes=15), "stream 1 (bytes 10 + 6) points outside the data of 15"), (dict(rows=table((0, 4), (-8, 4))), "stream 1 (bytes -8 + 4)"),
                     (dict(rows=table((0, -1), (0, 4))), "stream 0 (bytes 0 + -1)")):
        assert decode(**kw) != 0, kw
        assert word in err() and "ccvs_png_decode" in err(), (kw, err())
    for k in (0, 2, 3, 7, 9, 10):                                       # data, table, host table, frames, status, workspace
        argv = [one, 16, one, host(good), 2, 8, 8, one, 192, one, one, None]
        argv[k] = None
        assert L.ccvs_png_decode(*argv) != 0 and "null" in err(), k
    for k in (2, 9, 10):
        argv = [one, 16, one, host(good), 2, 8, 8, one, 192, one, one, None]
        argv[k] = ctypes.c_void_p(18)
        assert L.ccvs_png_decode(*argv) != 0 and "misaligned" in err(), k


def test_cpu_tensors_and_bad_arguments_are_refused():
    from ccvs_amd import lib, ops
    z = zlib.compress(b"abc")
    with pytest.raises(ValueError, match="sizes"):
        ops.zlib_inflate([z], [3, 4])
    with pytest.raises(ValueError, match="streams"):
        ops.zlib_inflate([], [])
    with pytest.raises(ValueError, match="1 .. 65535"):
        ops.png_decode_pack([z], 0, 8)
    with pytest.raises(ValueError, match="0 streams"):
        ops.png_decode_pack([], 8, 8)
    meta, blob = ops.png_decode_pack([z, z + z], 8, 9)
    assert meta["rows_host"].tolist() == [[0, len(z)], [len(z), 2 * len(z)]] and meta["o_data"] == 32 and meta["data_bytes"] == 3 * len(z)
    assert blob.dtype == np.uint8 and bytes(blob[32:]) == z * 3 and bytes(blob[:32]) == meta["rows_host"].tobytes()
    meta["blob"] = torch.from_numpy(blob)
    with pytest.raises(lib.CcvsError):
        ops.png_decode_uploaded(meta, out=torch.zeros(2, 8, 9, 3, dtype=torch.uint8))
    if not torch.cuda.is_available():
        with pytest.raises(lib.CcvsError):
            ops.zlib_inflate([z], [3])
        with pytest.raises(lib.CcvsError):
            ops.png_decode([z], 1, 1)


# ------------------------------------------------------------------ 7
def _plain(v):
    return list(v) if isinstance(v, (list, tuple)) else v


def test_options(golden_dir):
    from ccvs_amd.tools.options import Options
    assert Options().parse(True, True, argv=TINY)["transformer"].png_decode == "host"
    assert Options().parse(True, True, argv=TINY + ["--png_decode", "gpu"])["base"].png_decode == "gpu"
    with pytest.raises(SystemExit):
        Options().parse(True, True, argv=TINY + ["--png_decode", "auto"])
    parse = lambda argv: Options().parse(True, True, load_state_estimator=True, load_stft_ae=True, argv=argv)
    with open(os.path.join(golden_dir, "reference_launch_lines.json")) as f:
        lines = json.load(f)
    with open(os.path.join(golden_dir, "reference_checks.json")) as f:
        parsed = json.load(f)["launch_lines"]
    assert len(lines) >= 9
    for script, argv in sorted(lines.items()):
        got, got_on = parse(argv), parse(argv + ["--png_decode", "gpu"])
        assert got["transformer"].png_decode == "host" and got_on["transformer"].png_decode == "gpu"
        for key in ("transformer", "qvid_generator"):
            for both in (got, got_on):
                for f in rh.LAUNCH_LINE_FIELDS[key]:
                    if f in parsed[script][key]:
                        assert _plain(getattr(both[key], f)) == parsed[script][key][f], (script, key, f)
            a, b = vars(got[key]), vars(got_on[key])
            skip = lambda k: k in ("png_decode", "signature") or k.endswith("_path")
            assert {k: v for k, v in a.items() if not skip(k)} == {k: v for k, v in b.items() if not skip(k)}, (script, key)
    from ccvs_amd.tools.pytorch_metrics import metrics as M
    from ccvs_amd.tools.tf_fvd import fvd
    for mod in (M, fvd):
        assert mod.parse_args(["--exp_tag", "t"]).png_decode == "host" and mod.parse_args(["--exp_tag", "t", "--png_decode", "gpu"]).png_decode == "gpu"
        with pytest.raises(SystemExit):
            mod.parse_args(["--exp_tag", "t", "--png_decode", "cpu"])


def test_loader_routing(tmp_path, monkeypatch):
    from ccvs_amd import ops
    from ccvs_amd.tools.pytorch_metrics import metrics as M
    from ccvs_amd.tools.tf_fvd import fvd
    from ccvs_amd.tools import apng
    files = [str(tmp_path / "a.png"), str(tmp_path / "b.png")]
    seen = []
    monkeypatch.setattr(ops, "read_apng_clips", lambda paths: seen.append(("gpu", list(paths))) or torch.zeros(2, 2, 8, 8, 3, dtype=torch.uint8))
    monkeypatch.setattr(apng, "read_apng", lambda p: seen.append(("host", p)) or np.zeros((2, 8, 8, 3), np.uint8))
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    got = M.load_videos(files, None, 1, png_decode="gpu")
    assert seen == [("gpu", files)] and got.shape == (2, 2, 8, 8, 3)
    M.load_videos(files, None, 1)
    assert seen[1:] == [("host", files[0]), ("host", files[1])]
    with pytest.raises(ValueError, match="png_decode"):
        M.load_videos(files, None, 1, png_decode="auto")
    with pytest.raises(RuntimeError, match="all .avi or all .npy"):
        M.load_videos(["a.npy", "b.png"], None, 1, png_decode="gpu")
    del seen[:]
    monkeypatch.setattr(M, "_scores", lambda *a: None)
    monkeypatch.setattr(M, "_aggregate", lambda *a: (None, [], []))
    M.metrics_from_files(files * 8, files * 8, None, 1, False, [], png_decode="gpu")
    assert [s[0] for s in seen] == ["gpu", "gpu"]
    del seen[:]
    monkeypatch.setattr(fvd, "_embed_batches", lambda total, real, fake, order: (real(slice(0, 2)), fake(slice(0, 2))))
    fvd.emb_from_files(files, files, None, 1, png_decode="gpu")
    fvd.emb_from_files(files, files, None, 1)
    assert [s[0] for s in seen] == ["gpu", "gpu", "host", "host", "host", "host"]


def test_frame_dataset_falls_back_per_item(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from ccvs_amd.data import FrameDataset
    from ccvs_amd.data.frame_dataset import PngStreams
    from ccvs_amd.tools import apng
    rng = np.random.RandomState(5)
    frames = rng.randint(0, 256, size=(2, 12, 10, 3)).astype(np.uint8)
    other = rng.randint(0, 256, size=(9, 10, 3)).astype(np.uint8)
    root = tmp_path / "original_frames_256" / "test"
    kinds = {"a_rgb": lambda f, p: Image.fromarray(f).save(p + ".png"), "b_npy": lambda f, p: np.save(p + ".npy", f),
             "c_palette": lambda f, p: Image.fromarray(f).convert("P").save(p + ".png"), "d_grey": lambda f, p: Image.fromarray(f).convert("L").save(p + ".png"),
             "e_alpha": lambda f, p: Image.fromarray(f).convert("RGBA").save(p + ".png"), "f_jpeg": lambda f, p: Image.fromarray(f).save(p + ".jpg")}
    for name, save in kinds.items():
        os.makedirs(root / name)
        for k in range(2):
            save(frames[k], str(root / name / f"{k}"))
    os.makedirs(root / "g_sizes")
    Image.fromarray(frames[0]).save(str(root / "g_sizes" / "0.png"))
    Image.fromarray(other).save(str(root / "g_sizes" / "1.png"))
    opt = types.SimpleNamespace(dataroot=str(tmp_path), dataset="bairhd", png_decode="gpu")
    me = types.SimpleNamespace(opt=opt, plan=lambda h, w, offsets: [("plan", h, w)], read_frame=FrameDataset.read_frame)
    me.compressed = lambda item: FrameDataset.compressed(me, item)
    items = {name: {"paths": sorted(str(p) for p in (root / name).iterdir()), "offsets": None} for name in list(kinds) + ["g_sizes"]}
    got, plan = FrameDataset.decode(me, items["a_rgb"])
    assert isinstance(got, PngStreams) and got.shape == (2, 12, 10, 3) and plan == [("plan", 12, 10)] and got.paths == items["a_rgb"]["paths"]
    assert np.array_equal(apng.unfilter([zlib.decompress(s) for s in got.streams], 12, 10), frames)
    for name in ("b_npy", "c_palette", "d_grey", "e_alpha", "f_jpeg"):
        got, plan = FrameDataset.decode(me, items[name])
        assert isinstance(got, np.ndarray) and got.shape == (2, 12, 10, 3) and got.dtype == np.uint8 and plan == [("plan", 12, 10)], name
    assert np.array_equal(FrameDataset.decode(me, items["b_npy"])[0], frames)
    with pytest.raises(ValueError, match="differ in size"):               # mixed sizes: the host path's own verdict
        FrameDataset.decode(me, items["g_sizes"])
    opt.png_decode = "host"
    got, _ = FrameDataset.decode(me, items["a_rgb"])
    assert isinstance(got, np.ndarray) and np.array_equal(got, frames)
    del opt.png_decode                                                    # an options object from before the flag
    assert isinstance(FrameDataset.decode(me, items["a_rgb"])[0], np.ndarray)

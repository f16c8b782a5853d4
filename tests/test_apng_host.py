"""The lossless output stage, host side -- no GPU.

  1. the spec mirror tests/apng_ref.py against independent decoders, on every row of the image table: zlib inflates each frame's stream
     completely (checking the Adler-32) to the filtered bytes the mirror chose; `write_apng` + Pillow and `read_apng` give the pixels;
     over the table the adaptive filter uses all five types;
  2. `code_lengths` on synthetic counts: Kraft sum exactly 1, the length limit, lengths monotone in the counts, prefix-free codes; a
     row whose tree is 17 deep before the limiter, decoded by zlib;
  3. the container: chunk order, lengths, CRCs, acTL, the sequence numbers, the delay fraction; one frame still opens;
  4. `read_apng` on files Pillow wrote (PNG and APNG, every filter type, LZ77-compressed) and each refusal by its message;
  5. `lib.OUTPUT_LOSSLESS_EXPORTS` equals what include/ccvs_hip_output_lossless.h declares, the built library exports it, EXPORTS and
     the ABI version did not move, every refused argument is named in `ccvs_last_error()` before any launch, the stream bound;
  6. `--video_format apng`, the reference's launch lines, CPU tensors refused, `get_video_files` / `load_videos` routing;
  7. sizes: the mirror against zlib's Huffman-only stream of the same filtered bytes, and the 9/8 bound on noise.
"""
import ctypes
import io
import json
import os
import re
import struct
import subprocess
import sys
import zlib
from fractions import Fraction

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import apng_ref as R  # noqa: E402
import ref_harness as rh  # noqa: E402
from tests.test_mjpeg_host import TINY  # noqa: E402


def inflate(stream):
    """The bytes zlib makes of one complete stream: it must end exactly where the stream ends (zlib checks the Adler-32 itself)."""
    d = zlib.decompressobj()
    out = d.decompress(stream)
    assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b""
    return out


# ------------------------------------------------------------------ 1
def test_table_covers_what_it_is_there_for():
    rows = R.rows()
    assert len({row[0] for row in rows}) == len(rows) >= 1000
    shapes = {img.shape[:2] for img in R.images().values()}
    assert shapes == set(R.SIZES) | {(256, 256)}
    assert (3 * 23 + 1) % 4 == 2 and (3 * 65) % 4 == 3                  # filtered rows of 70 bytes; raw rows of 195 (filtered: 196)
    assert {row[2] for row in rows} == set(R.FILTERS)
    for name, img in R.images().items():
        h = img.shape[0]
        assert {row[3] for row in rows if row[1] == name} == {r for r in (1, 2, h - 1, h, 0) if r == 0 or 1 <= r <= h}, name
    # flat frames: one literal and end-of-block, so 1-bit codes; noise: every literal used
    for flat in ("zeros_8x8", "ones_8x8"):
        assert np.count_nonzero(np.bincount(np.frombuffer(R.mirrored(flat + "/f0/b0")["filtered"], np.uint8), minlength=256)) <= 2
    assert np.count_nonzero(np.bincount(np.frombuffer(R.mirrored("noise_64x64/f0/b0")["filtered"], np.uint8), minlength=256)) == 256


def test_mirror_streams_inflate_to_the_filtered_bytes():
    used = set()
    for key, name, flt, r in R.rows():
        m = R.mirrored(key)
        img = R.images()[name]
        h, w = img.shape[:2]
        rows, types = R.filter_rows(img, flt)
        assert m["filtered"] == rows.tobytes() and len(m["filtered"]) == h * (3 * w + 1), key
        assert inflate(m["stream"]) == m["filtered"], key
        assert m["stream"][:2] == b"\x78\x01" and m["bands"] == len(R.band_cut(h, w, r)), key
        if flt == -1:
            used |= {int(t) for t in types}
        else:
            assert set(types) == {flt}
    assert used == {0, 1, 2, 3, 4}                                      # the adaptive choice takes every type somewhere


def test_adaptive_choice_is_the_smallest_sum_ties_low():
    img = R.images()["mixed_33x65"]
    cand = R.filter_candidates(img).astype(int)
    _, types = R.filter_rows(img, -1)
    for y in range(img.shape[0]):
        score = [int(np.where(c[y] < 128, c[y], 256 - c[y]).sum()) for c in cand]
        assert types[y] == score.index(min(score)), y
    assert len(set(types)) == 5                                         # this frame's rows each favour another filter
    # a frame of zeros: all five filters give zeros, the lowest type wins
    assert set(R.filter_rows(np.zeros((4, 5, 3), np.uint8), -1)[1]) == {0}


def test_files_open_in_pillow_and_read_apng(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from ccvs_amd.tools import apng
    for fps, (name, img) in zip((4, 25) * 100, R.images().items()):
        keys = [row[0] for row in R.rows() if row[1] == name]
        if img.shape[0] == 256:
            keys = keys[::3]
        h, w = img.shape[:2]
        path = str(tmp_path / (name + ".png"))
        apng.write_apng(path, [R.mirrored(k)["stream"] for k in keys], fps, h, w)
        with Image.open(path) as im:
            assert im.n_frames == len(keys) and im.size == (w, h) and im.info["duration"] == 1000 / fps, name
            for t in range(im.n_frames):
                im.seek(t)
                assert np.array_equal(np.asarray(im.convert("RGB")), img), (name, keys[t])
        back = apng.read_apng(path)
        assert back.shape == (len(keys), h, w, 3) and back.dtype == np.uint8 and (back == img[None]).all(), name


# ------------------------------------------------------------------ 2
def _fib(n):
    out = [1, 1]
    while len(out) < n:
        out.append(out[-1] + out[-2])
    return out[:n]


SYNTHETIC = {
    "two": [0] * 65 + [7] + [0] * 190 + [1],
    "equal": [5] * 257,
    "fibonacci": _fib(40) + [0] * 216 + [1],
    "one_huge": [1] * 100 + [10 ** 9] + [1] * 156,
    "one_symbol": [0] * 256 + [1],
    "none": [0] * 257,
}


@pytest.mark.parametrize("case", sorted(SYNTHETIC))
@pytest.mark.parametrize("maxlen", [15, 7])
def test_code_lengths_on_synthetic_counts(case, maxlen):
    counts = SYNTHETIC[case] if maxlen == 15 else SYNTHETIC[case][:10] + SYNTHETIC[case][-9:]      # 19 symbols for the code-length code
    lengths = R.code_lengths(counts, maxlen)
    used = [i for i, l in enumerate(lengths) if l]
    assert len(used) >= 2 and all(lengths[i] for i, c in enumerate(counts) if c)
    if sum(c > 0 for c in counts) >= 2:
        assert used == [i for i, c in enumerate(counts) if c]           # exactly the counted symbols
    assert sum(Fraction(1, 2 ** lengths[i]) for i in used) == 1         # complete, not over-subscribed
    assert max(lengths) <= maxlen
    for i in used:
        for j in used:
            if counts[i] > counts[j]:
                assert lengths[i] <= lengths[j], (i, j)
    codes = R.canonical(lengths)
    words = sorted(format(codes[i], f"0{lengths[i]}b") for i in used)
    assert all(not b.startswith(a) for a, b in zip(words, words[1:]))   # prefix-free (sorted: a prefix would stand right before)
    if case == "fibonacci" and maxlen == 15:
        assert max(R.code_lengths(counts, 64)) == 21 and max(lengths) == 15       # 21 deep before the limiter (equal sums make two chains)
        assert lengths[39] == min(l for l in lengths if l)
    if case == "equal" and maxlen == 15:
        assert sorted(set(lengths)) == [8, 9] and lengths.count(9) == 2


def test_deep_row_through_the_limiter():
    img = R.deep_row()
    m = R.encode_frame(img, 0, 0)
    assert m["bands"] == 1 and inflate(m["stream"]) == b"\x00" + img.tobytes()
    filtered = np.frombuffer(m["filtered"], np.uint8)
    _, lengths = R.band_block(filtered, True)
    free = R.code_lengths(np.bincount(filtered, minlength=257) + np.eye(257, dtype=np.int64)[256], 64)
    assert max(free) == 17 and max(lengths) == 15 and sum(Fraction(1, 2 ** l) for l in lengths if l) == 1


def test_run_lengths_cover_their_sequence():
    for seq in ([8] * 257 + [1, 1], [1] + [0] * 255 + [1, 1, 1], [0] * 140 + [3] * 9 + [0] * 2 + [5, 5, 5, 5] + [0] * 11, [4, 4, 4, 0, 0, 0]):
        out, prev = [], None
        for s, extra, nbits in R.run_lengths(seq):
            assert (s < 16 and nbits == 0) or (s, nbits) in ((16, 2), (17, 3), (18, 7))
            assert 0 <= extra < (1 << nbits) or nbits == 0
            if s < 16:
                out.append(s)
            elif s == 16:
                out += [out[-1]] * (3 + extra)
            else:
                out += [0] * ((3 if s == 17 else 11) + extra)
        assert out == seq


# ------------------------------------------------------------------ 3
def _walk(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, out = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        payload = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + payload), tag
        out.append((tag, payload))
        pos += 12 + n
    assert pos == len(data)
    return out


@pytest.mark.parametrize("fps,frac", [(4, (1, 4)), (25, (1, 25))])
def test_container_chunks(tmp_path, fps, frac):
    from ccvs_amd.tools import apng
    img = R.images()["smooth_17x23"]
    zs = [R.mirrored(f"smooth_17x23/f{f}/b0")["stream"] for f in (-1, 0, 4)]
    path = str(tmp_path / "a.png")
    apng.write_apng(path, zs, fps, 17, 23)
    cs = _walk(open(path, "rb").read())
    assert [t for t, _ in cs] == [b"IHDR", b"acTL", b"fcTL", b"IDAT", b"fcTL", b"fdAT", b"fcTL", b"fdAT", b"IEND"]
    assert cs[0][1] == struct.pack(">IIBBBBB", 23, 17, 8, 2, 0, 0, 0) and cs[1][1] == struct.pack(">II", 3, 0) and cs[-1][1] == b""
    seq = []
    for tag, p in cs:
        if tag == b"fcTL":
            assert len(p) == 26 and struct.unpack(">IIIIHHBB", p[4:]) == (23, 17, 0, 0) + frac + (0, 0)
            seq.append(struct.unpack(">I", p[:4])[0])
        elif tag == b"fdAT":
            seq.append(struct.unpack(">I", p[:4])[0])
    assert seq == [0, 1, 2, 3, 4]
    assert cs[3][1] == zs[0] and cs[5][1][4:] == zs[1] and cs[7][1][4:] == zs[2]
    assert (apng.read_apng(path) == img[None]).all()
    assert apng.delay_fraction(fps) == frac and apng.delay_fraction(29.97) == (100, 2997)


def test_one_frame_still_opens(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from ccvs_amd.tools import apng
    img = R.images()["dramp_8x8"]
    path = str(tmp_path / "one.png")
    apng.write_apng(path, [R.mirrored("dramp_8x8/f-1/b0")["stream"]], 4, 8, 8)
    assert [t for t, _ in _walk(open(path, "rb").read())] == [b"IHDR", b"acTL", b"fcTL", b"IDAT", b"IEND"]
    with Image.open(path) as im:
        assert getattr(im, "n_frames", 1) == 1 and np.array_equal(np.asarray(im.convert("RGB")), img)
    assert np.array_equal(apng.read_apng(path), img[None])
    with pytest.raises(ValueError, match="no frames"):
        apng.write_apng(path, [], 4, 8, 8)


# ------------------------------------------------------------------ 4
def test_read_apng_on_pillows_files(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from ccvs_amd.tools import apng
    seen = set()
    for k, (name, level) in enumerate((("mixed_33x65", 1), ("smooth_64x64", 6), ("noise_17x23", 9), ("hramp_8x8", 6), ("mixed_64x64", 9), ("smooth_256x256", 6))):
        img = R.images()[name]
        path = str(tmp_path / f"p{k}.png")
        Image.fromarray(img).save(path, compress_level=level)
        got = apng.read_apng(path)
        with Image.open(path) as im:
            assert np.array_equal(got[0], np.asarray(im)) and got.shape == (1,) + img.shape and np.array_equal(got[0], img)
        raw = zlib.decompress(b"".join(p for t, p in _walk(open(path, "rb").read()) if t == b"IDAT"))
        seen |= set(np.frombuffer(raw, np.uint8).reshape(img.shape[0], -1)[:, 0].tolist())
        # an APNG of three frames that differ everywhere, so that Pillow writes full frames
        frames = [img, 255 - img, np.roll(img, 1, axis=0) ^ 0x55]
        path = str(tmp_path / f"a{k}.png")
        Image.fromarray(frames[0]).save(path, save_all=True, append_images=[Image.fromarray(f) for f in frames[1:]], duration=40, compress_level=level)
        got = apng.read_apng(path)
        with Image.open(path) as im:
            assert im.n_frames == 3
            for t in range(3):
                im.seek(t)
                assert np.array_equal(got[t], np.asarray(im.convert("RGB"))) and np.array_equal(got[t], frames[t]), (name, t)
    # Pillow's libpng chooses among None, Sub, Up and Paeth; Average rows are read from the mirror's files (test 1: filter = 3)
    assert seen >= {0, 1, 2, 4}


def _png(chunks):
    from ccvs_amd.tools import apng
    return apng.SIGNATURE + b"".join(apng._chunk(t, p) for t, p in chunks)


def test_read_apng_refusals(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from ccvs_amd.tools import apng
    img = R.images()["smooth_8x8"]
    z = R.mirrored("smooth_8x8/f-1/b0")["stream"]
    path = str(tmp_path / "x.png")

    def refused(data, word):
        open(path, "wb").write(data)
        with pytest.raises(ValueError, match=word):
            apng.read_apng(path)

    ihdr = lambda depth=8, colour=2, interlace=0: (b"IHDR", struct.pack(">IIBBBBB", 8, 8, depth, colour, 0, 0, interlace))
    fctl = lambda seq, w=8, h=8, x=0, y=0, dispose=0, blend=0: (b"fcTL", struct.pack(">IIIIIHHBB", seq, w, h, x, y, 1, 4, dispose, blend))
    good = [ihdr(), (b"acTL", struct.pack(">II", 2, 0)), fctl(0), (b"IDAT", z), fctl(1), (b"fdAT", struct.pack(">I", 2) + z), (b"IEND", b"")]
    open(path, "wb").write(_png(good))
    assert (apng.read_apng(path) == img[None]).all() and apng.read_apng(path).shape[0] == 2
    refused(b"JUNK" + _png(good), "signature")
    refused(_png(good)[:-3], "past the end")
    bad = bytearray(_png(good))
    bad[40] ^= 1
    refused(bytes(bad), "CRC")
    refused(_png([ihdr(colour=6)] + good[1:]), "colour type 6")
    refused(_png([ihdr(colour=0)] + good[1:]), "colour type 0")
    refused(_png([ihdr(depth=16)] + good[1:]), "bit depth 16")
    refused(_png([ihdr(interlace=1)] + good[1:]), "interlace")
    refused(_png(good[:4] + [fctl(1, w=4)] + good[5:]), "partial frame")
    refused(_png(good[:4] + [fctl(1, x=1, w=7)] + good[5:]), "partial frame")
    refused(_png(good[:4] + [fctl(1, blend=1)] + good[5:]), "blend 1")
    refused(_png(good[:4] + [fctl(1, dispose=2)] + good[5:]), "dispose 2")
    refused(_png(good[:5] + [(b"fdAT", struct.pack(">I", 3) + z)] + good[6:]), "sequence number")
    refused(_png(good[:1] + [(b"acTL", struct.pack(">II", 3, 0))] + good[2:]), "acTL says 3")
    refused(_png(good[:3] + [(b"IDAT", z[:-1])] + good[4:]), "inflate")
    refused(_png([(b"IHDR", struct.pack(">IIBBBBB", 8, 9, 8, 2, 0, 0, 0))] + good[1:2] + [fctl(0, h=9), good[3], fctl(1, h=9)] + good[5:]), "rows")
    # Pillow's own RGBA, palette and greyscale files are refused by their colour type
    for mode, colour in (("RGBA", 6), ("P", 3), ("L", 0)):
        Image.fromarray(img).convert(mode).save(path)
        with pytest.raises(ValueError, match=f"colour type {colour}"):
            apng.read_apng(path)


# ------------------------------------------------------------------ 5
def test_lossless_symbols_declared_and_exported(tmp_path):
    from ccvs_amd import lib
    header = open(os.path.join(ROOT, "include", "ccvs_hip_output_lossless.h")).read()
    assert re.search(r'^#include "ccvs_hip_output_lossless.h"', open(os.path.join(ROOT, "include", "ccvs_hip.h")).read(), re.M)
    declared = sorted(set(re.findall(r"^\w[\w \*]*?\b(ccvs_\w+)\(", header, re.M)))
    assert declared == sorted(lib.OUTPUT_LOSSLESS_EXPORTS) == ["ccvs_apng_encode", "ccvs_apng_stream_bound", "ccvs_apng_workspace_bytes"]
    others = (set(lib.EXPORTS) | set(lib.EVAL_EXPORTS) | set(lib.INPUT_EXPORTS) | set(lib.GEMM_EXPORTS) | set(lib.OUTPUT_EXPORTS) | set(lib.DECODE_EXPORTS)
              | set(lib.VIDEO_EXPORTS) | set(lib.OUTPUT_SAMPLED_EXPORTS) | set(lib.OUTPUT_OPTIMIZED_EXPORTS) | set(lib.LPIPS_EXPORTS) | set(lib.FVD_EXPORTS))
    assert not set(lib.OUTPUT_LOSSLESS_EXPORTS) & others and len(lib.EXPORTS) == 51
    handle = ctypes.CDLL(lib.LIB_PATH)
    for sym in lib.OUTPUT_LOSSLESS_EXPORTS:
        assert hasattr(handle, sym), sym
    c = tmp_path / "p.c"
    c.write_text('#include "ccvs_hip.h"\nvoid* p[] = {' + ", ".join("(void*)" + s for s in lib.OUTPUT_LOSSLESS_EXPORTS) + "};\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "p.o")], check=True)
    assert lib.load().ccvs_abi_version() == 6


def test_sizes_and_refusals_before_any_launch():
    from ccvs_amd import lib
    L = lib.load()
    ws, bound = L.ccvs_apng_workspace_bytes, L.ccvs_apng_stream_bound
    # the filtered bytes (rounded up to 8), 4 bytes per frame (rounded up to 8) and 1576 bytes per band
    for n, h, w, r in ((256, 256, 256, 0), (1, 17, 23, 1), (3, 33, 65, 32), (2, 1, 1, 0), (5, 64, 64, 2)):
        rows = r or max(1, 32768 // (3 * w + 1))
        bands = -(-h // rows)
        assert ws(n, h, w, r) == n * bands * 1576 + (4 * n + 7) // 8 * 8 + (n * h * (3 * w + 1) + 7) // 8 * 8, (n, h, w, r)
        assert bound(n, h, w, r) >= n * (6 + h * (3 * w + 1) * 15 // 8 + bands * 467), (n, h, w, r)
    for args in ((0, 8, 8, 0), (1, 0, 8, 0), (1, 8, 0, 0), (1, 65536, 8, 0), (1, 8, 65536, 0), (1, 8, 8, -1), (1, 65535, 65535, 65535)):
        assert ws(*args) == 0 and bound(*args) == 0, args
    one = ctypes.c_void_p(16)
    call = lambda n, h, w, f, r, cap=64, stride=192: L.ccvs_apng_encode(one, stride, n, h, w, f, r, one, cap, one, one, None)
    for args, word in (((0, 8, 8, -1, 0), "frames"), ((-1, 8, 8, -1, 0), "frames"), ((1, 0, 8, -1, 0), "size"), ((1, 8, 65536, -1, 0), "size"),
                       ((1, 65536, 8, 0, 0), "size"), ((1, 8, 8, -2, 0), "filter"), ((1, 8, 8, 5, 0), "filter"), ((1, 8, 8, -1, -1), "band_rows"),
                       ((1, 65535, 65535, -1, 65535, 64, 1 << 40), "band_rows"), ((1, 8, 8, -1, 0, -1), "capacity"), ((1, 8, 8, -1, 0, 64, 191), "stride"),
                       ((2, 8, 8, -1, 0, 64, -192), "stride")):
        assert call(*args) != 0, args
        msg = L.ccvs_last_error().decode()
        assert word in msg and "ccvs_apng_encode" in msg, (args, msg)
    for k in (0, 7, 9, 10):                                            # rgb, stream (with a capacity), offsets, workspace
        argv = [one, 192, 1, 8, 8, -1, 0, one, 64, one, one, None]
        argv[k] = None
        assert L.ccvs_apng_encode(*argv) != 0 and "null" in L.ccvs_last_error().decode(), k
    # the bound covers the mirror on the noise rows (and on every other row of the small frames)
    for key, name, flt, r in R.rows():
        if name.startswith("noise") or name.endswith("8x8"):
            h, w = R.images()[name].shape[:2]
            assert bound(1, h, w, r) >= len(R.mirrored(key)["stream"]), key


# ------------------------------------------------------------------ 6
def _plain(v):
    return list(v) if isinstance(v, (list, tuple)) else v


def test_options(golden_dir):
    from ccvs_amd.tools.options import Options
    assert Options().parse(True, True, argv=TINY)["transformer"].video_format == "auto"
    a = Options().parse(True, True, argv=TINY + ["--video_format", "apng", "--video_quality", "50", "--video_subsampling", "420", "--video_optimize"])["base"]
    assert a.video_format == "apng"                                    # the avi flags are ignored there, not refused
    with pytest.raises(SystemExit):
        Options().parse(True, True, argv=TINY + ["--video_format", "mp4"])
    parse = lambda argv: Options().parse(True, True, load_state_estimator=True, load_stft_ae=True, argv=argv)
    with open(os.path.join(golden_dir, "reference_launch_lines.json")) as f:
        lines = json.load(f)
    with open(os.path.join(golden_dir, "reference_checks.json")) as f:
        parsed = json.load(f)["launch_lines"]
    assert len(lines) >= 9
    for script, argv in sorted(lines.items()):
        got, got_on = parse(argv), parse(argv + ["--video_format", "apng"])
        assert got["transformer"].video_format == "auto" and got_on["transformer"].video_format == "apng"
        for key in ("transformer", "qvid_generator"):
            for both in (got, got_on):
                for f in rh.LAUNCH_LINE_FIELDS[key]:
                    if f in parsed[script][key]:
                        assert _plain(getattr(both[key], f)) == parsed[script][key][f], (script, key, f)
            a, b = vars(got[key]), vars(got_on[key])
            skip = lambda k: k in ("video_format", "signature") or k.endswith("_path")
            assert {k: v for k, v in a.items() if not skip(k)} == {k: v for k, v in b.items() if not skip(k)}, (script, key)


def test_cpu_tensors_are_refused(tmp_path):
    from ccvs_amd import lib, ops
    from ccvs_amd.helpers.generator import save_video_batch
    with pytest.raises(lib.CcvsError):
        ops.png_encode(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(lib.CcvsError):
        ops.png_encode_to_host(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), 0, 1)
    with pytest.raises(lib.CcvsError):
        save_video_batch(torch.zeros(1, 2, 3, 8, 8), 1, 0, str(tmp_path / "a"), 4, True, False, [-1, 1], "bairhd", video_format="apng")
    with pytest.raises(ValueError, match="video_format"):
        save_video_batch(torch.zeros(1, 2, 3, 8, 8), 1, 0, str(tmp_path / "a"), 4, True, False, [-1, 1], "bairhd", video_format="mp4")


def test_save_results_passes_apng_through(tmp_path, monkeypatch):
    import types
    from ccvs_amd.helpers import generator as G
    seen = []
    monkeypatch.setattr(G, "save_video_batch", lambda *a, **k: seen.append((os.path.basename(a[3]), k["video_format"], k["return_clip"])))
    opt = types.SimpleNamespace(video_format="apng", video_quality=80, video_subsampling="420", video_optimize=True, result_path=str(tmp_path), fps=4,
                                imagenet_norm=False, dataset="bairhd", state=True)
    me = types.SimpleNamespace(opt=opt, decode_stft=False)
    vid = torch.zeros(2, 2, 3, 8, 8)
    G.Generator.save_results(me, {"real": vid, "fake": {"vid": vid, "state": torch.zeros(2, 2, 2)}, "rec": {"vid": vid}, "blur": vid}, 0)
    assert seen == [(k, "apng", False) for k in ("real", "fake", "fake_state", "rec", "blur")]


def test_folder_and_loader_routing(tmp_path, monkeypatch):
    from ccvs_amd.tools.pytorch_metrics import metrics as M
    from ccvs_amd.tools.tf_fvd import fvd
    from ccvs_amd.tools import apng
    assert fvd.get_video_files is M.get_video_files and fvd.load_videos is M.load_videos
    d = tmp_path / "png"
    d.mkdir()
    z = R.mirrored("smooth_8x8/f-1/b0")["stream"]
    for name in ("vid_00001.png", "vid_00000.png"):
        apng.write_apng(str(d / name), [z, z], 4, 8, 8)
    assert [os.path.basename(f) for f in M.get_video_files(str(d))] == ["vid_00000.png", "vid_00001.png"]
    np.save(str(d / "vid_00000.npy"), np.zeros((2, 8, 8, 3), np.uint8))
    assert [os.path.basename(f) for f in M.get_video_files(str(d))] == ["vid_00000.npy"]          # the arrays win
    with pytest.raises(RuntimeError, match="all .avi or all .npy"):
        M.load_videos(["a.avi", "b.png"], None, 1)
    with pytest.raises(RuntimeError, match="all .avi or all .npy"):
        M.load_videos(["a.npy", "b.png"], None, 1)
    # an all-.png batch is read on the host and uploaded once: the upload is what fails without a GPU, after the files were read
    read = []
    monkeypatch.setattr(apng, "read_apng", lambda p: read.append(os.path.basename(p)) or np.zeros((2, 8, 8, 3), np.uint8))
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    got = M.load_videos([str(d / "vid_00000.png"), str(d / "vid_00001.png")], None, 1)
    assert read == ["vid_00000.png", "vid_00001.png"] and got.shape == (2, 2, 8, 8, 3) and got.dtype == torch.uint8


# ------------------------------------------------------------------ 7
def test_size_against_zlibs_huffman_only_stream():
    """Recorded (printed), then bounded.  zlib's Z_HUFFMAN_ONLY codes the same filtered bytes with dynamic tables too, in blocks it cuts
    itself; the mirror adds, per band, its own header (at most 3700 bits), end-of-block, the stored block's 3 bits, padding and
    00 00 FF FF: `band_overhead_bytes()` = 470 bytes at most.  The allowance is that per band."""
    Image = pytest.importorskip("PIL.Image")
    for key in ("smooth_256x256/f-1/b0", "smooth_64x64/f-1/b0", "mixed_64x64/f-1/b0", "noise_64x64/f-1/b0"):
        m = R.mirrored(key)
        data = m["filtered"]
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
        huff = len(c.compress(data) + c.flush())
        buf = io.BytesIO()
        Image.fromarray(R.images()[key.split("/")[0]]).save(buf, format="PNG")
        raw = len(data)
        print(f"{key}: mirror {len(m['stream'])}, zlib Huffman-only {huff}, zlib level 6 {len(zlib.compress(data, 6))}, Pillow's PNG {buf.tell()}, "
              f"filtered {raw}; mirror / Huffman-only {len(m['stream']) / huff:.4f}, mirror / raw {len(m['stream']) / raw:.4f}")
        assert len(m["stream"]) <= huff + m["bands"] * R.band_overhead_bytes(), key


def test_noise_stays_within_nine_eighths():
    """257 symbols always have a prefix code of 8 and 9 bits, so the optimal code of a band costs at most 9 bits per byte where the
    limiter moves nothing (noise: depths of 7 .. 10); the rest is the per-band overhead."""
    for key, name, flt, r in R.rows():
        if name.startswith("noise"):
            m = R.mirrored(key)
            assert len(m["stream"]) <= 6 + len(m["filtered"]) * 9 // 8 + 1 + m["bands"] * R.band_overhead_bytes(), key

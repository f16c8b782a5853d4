"""Motion-JPEG AVI files around the scans `ops.mjpeg_encode` writes.  Host only: no torch, no GPU.

  jpeg_header(h, w, quality, restart_mcus,   the bytes in front of a frame's scan: SOI, DQT x 2, SOF0 (8 bit, three components; luminance
              sampling, huffman)             sampled 1 x 1, 2 x 1 or 2 x 2 for sampling 0 / 1 / 2 = 4:4:4 / 4:2:2 / 4:2:0, chrominance 1 x 1),
                                             DHT x 4 (the Annex K tables, or the frame's own: `huffman`), DRI, SOS.  header + scan + EOI is
                                             a JPEG file.
  huffman_from_spec(spec)                    a frame's row of `ops.mjpeg_encode_optimized`'s tables (uint8 [4, 272]) as that `huffman`.
  write_avi(path, frames, fps, h, w)         RIFF 'AVI ': hdrl (avih, one strl: strh vids/MJPG + strf BITMAPINFOHEADER), a movi list of
                                             '00dc' chunks padded to even length, idx1.
  read_avi(path) -> (fps, h, w, [jpeg])      the frames of such a file, byte for byte.
  probe_avi(path) -> (fps, h, w, n, index)   the same of ANY writer's MJPG AVI (JUNK, LIST INFO / odml / rec, other streams, idx1 from either
                                             base, no idx1) from the headers and the index alone; it says what it refuses and why.
  read_avi_frames(path, numbers, index)      the JPEG bytes of those frames only: one seek + read each (the video-file datasets).
  decode_frames(jpegs) -> uint8 [T, H, W, 3] with Pillow (ImportError where it is missing), on the host.

The way back on the GPU (`ops.mjpeg_decode`) has its host half here -- everything up to the bytes that go up:
  parse_jpeg(data)                           the marker walk of one baseline file: size, sampling, quantiser and Huffman tables, restart
                                             interval, where the scan lies.  ValueError with the reason for what is malformed or not decoded
                                             (progressive, arithmetic, 12 bit, greyscale, CMYK, other sampling factors, several scans).
  find_units(scans, offsets, ri, n_mcu)      the unit table of the frames' scans -- a unit is one restart interval, or the whole scan without
                                             DRI: int64 [units, 5] of frame, byte offset, byte length, first MCU, MCUs (one numpy pass finds
                                             the markers of all frames).
  huffman_table(bits, vals)                  a DHT table in the decoder's form (T.81 F.2.2.3 plus an 8-bit lookup).
  decode_tables(parsed)                      the 4008-byte table record of a frame (include/ccvs_hip_decode.h).
  plan_frames(jpegs)                         all of it for the frames of one call: scans, unit table, table records, record per frame.
"""
import struct

EOI = b"\xff\xd9"
# ITU-T T.81 Annex K.1 / K.2 (natural order) and K.3 - K.6 as (bits, vals); the encoder holds the same tables (csrc/jpeg.hip)
BASE_Q = (
    (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99),
    (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32)
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
_AC_LUMA = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546474849"
    "4a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5"
    "c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA = bytes.fromhex(
    "0001020311040521310612415107617113223281081442"
    "91a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748494a535455565758595a636465666768696a7374757677"
    "78797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8"
    "e9eaf2f3f4f5f6f7f8f9fa")
# DHT class / id byte -> (bits, vals): 0x00 DC luminance, 0x10 AC luminance, 0x01 DC chrominance, 0x11 AC chrominance (the order written)
HUFF = {
    0x00: (bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]), bytes(range(12))),
    0x10: (bytes([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125]), _AC_LUMA),
    0x01: (bytes([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]), bytes(range(12))),
    0x11: (bytes([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119]), _AC_CHROMA),
}


MAX_RESTART = (32, 24, 16)    # per sampling 0 / 1 / 2: the encoder's interval holds 96 blocks, an MCU has 3 / 4 / 6
_Y_FACTORS = (0x11, 0x21, 0x22)


def default_restart(w, sampling=0):
    """The encoder's default restart interval in MCUs: one row of MCUs (8 pixels wide in 4:4:4, 16 in 4:2:2 and 4:2:0), capped at the
    sampling's limit of 32 / 24 / 16."""
    if sampling not in (0, 1, 2):
        raise ValueError(f"default_restart: sampling {sampling!r} is none of 0 (4:4:4), 1 (4:2:2), 2 (4:2:0)")
    mw = 16 if sampling else 8
    return min((int(w) + mw - 1) // mw, MAX_RESTART[sampling])


def quant_tables(quality):
    """libjpeg's `jpeg_set_quality` (baseline): the two tables in natural order."""
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError(f"JPEG quality {quality} outside 1 .. 100")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(tuple(min(max((b * scale + 50) // 100, 1), 255) for b in base) for base in BASE_Q)


def _segment(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


def huffman_from_spec(spec):
    """The `huffman` argument of `jpeg_header` from one frame's row of the optimised encoder's `tables` (uint8 [4, 272]: per table
    bits[16] + huffval, zero-padded; DC luminance, AC luminance, DC chrominance, AC chrominance): four (bits, vals) of bytes."""
    out = []
    for row in spec:
        row = bytes(bytearray(row))
        if len(row) != 272 or sum(row[:16]) > 256:
            raise ValueError("huffman_from_spec: a table is 272 bytes, bits[16] + up to 256 symbols")
        out.append((row[:16], row[16:16 + sum(row[:16])]))
    if len(out) != 4:
        raise ValueError(f"huffman_from_spec: {len(out)} tables, a frame has 4")
    return tuple(out)


def jpeg_header(h, w, quality, restart_mcus=None, sampling=0, huffman=None):
    """Everything in front of the scan of an h x w frame encoded at `quality` with a restart interval of `restart_mcus` MCUs (of the
    sampling's size; None: `default_restart(w, sampling)`).  sampling: 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0.  huffman: None for the Annex K
    tables, else the frame's own four (bits, vals) -- DC luminance, AC luminance, DC chrominance, AC chrominance, the order in which
    libjpeg writes them and `huffman_from_spec` gives them -- written as the DHT segments in the same place."""
    h, w = int(h), int(w)
    if sampling not in (0, 1, 2):
        raise ValueError(f"jpeg_header: sampling {sampling!r} is none of 0 (4:4:4), 1 (4:2:2), 2 (4:2:0)")
    r = default_restart(w, sampling) if restart_mcus is None else int(restart_mcus)
    if not (1 <= h <= 65535 and 1 <= w <= 65535 and 1 <= r <= MAX_RESTART[sampling]):
        raise ValueError(f"jpeg_header: size {h} x {w} or restart interval {r} out of range")
    out = b"\xff\xd8"
    for t, table in enumerate(quant_tables(quality)):
        out += _segment(0xDB, bytes([t]) + bytes(table[k] for k in ZIGZAG))
    out += _segment(0xC0, struct.pack(">BHHB", 8, h, w, 3) + bytes([1, _Y_FACTORS[sampling], 0, 2, 0x11, 1, 3, 0x11, 1]))
    if huffman is None:
        tables = HUFF
    else:
        huffman = tuple(huffman)
        tables = {key: (bytes(bits), bytes(vals)) for key, (bits, vals) in zip(HUFF, huffman)}
        if len(huffman) != 4 or any(len(bits) != 16 or sum(bits) != len(vals) or len(vals) > 256 for bits, vals in tables.values()):
            raise ValueError("jpeg_header: huffman is four (bits[16], vals) with sum(bits) == len(vals) <= 256")
    for key, (bits, vals) in tables.items():
        out += _segment(0xC4, bytes([key]) + bits + vals)
    out += _segment(0xDD, struct.pack(">H", r))
    out += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


# ------------------------------------------------------------------ RIFF / AVI
def _chunk(tag, payload):
    return tag + struct.pack("<I", len(payload)) + payload + (b"\x00" if len(payload) & 1 else b"")


def _list(kind, payload):
    return b"LIST" + struct.pack("<I", len(payload) + 4) + kind + payload


def write_avi(path, frames, fps, h, w):
    """`frames`: complete JPEG files (bytes), one per video frame, all h x w."""
    frames = [bytes(f) for f in frames]
    fps, h, w = int(fps), int(h), int(w)
    if fps < 1 or not frames:
        raise ValueError("write_avi: needs at least one frame and a positive integer frame rate")
    biggest = max(len(f) for f in frames)
    avih = struct.pack("<14I", 1000000 // fps, biggest * fps, 0, 0x10, len(frames), 0, 1, biggest, w, h, 0, 0, 0, 0)   # 0x10: AVIF_HASINDEX
    strh = struct.pack("<4s4sIHHIIIIIIIIhhhh", b"vids", b"MJPG", 0, 0, 0, 0, 1, fps, 0, len(frames), biggest, 0xFFFFFFFF, 0, 0, 0, min(w, 32767), min(h, 32767))
    strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
    hdrl = _list(b"hdrl", _chunk(b"avih", avih) + _list(b"strl", _chunk(b"strh", strh) + _chunk(b"strf", strf)))
    movi, idx, pos = b"", b"", 4                                # idx1 offsets count from the 'movi' tag
    for f in frames:
        idx += struct.pack("<4sIII", b"00dc", 0x10, pos, len(f))   # 0x10: AVIIF_KEYFRAME
        c = _chunk(b"00dc", f)
        movi += c
        pos += len(c)
    body = b"AVI " + hdrl + _list(b"movi", movi) + _chunk(b"idx1", idx)
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def _chunks(data, start, end):
    """(tag, payload offset, payload size) of the chunks of data[start:end]."""
    pos = start
    while pos + 8 <= end:
        tag, size = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
        if pos + 8 + size > end:
            raise ValueError(f"AVI chunk {tag!r} at {pos} runs past its container")
        yield tag, pos + 8, size
        pos += 8 + size + (size & 1)


def read_avi(path):
    """(fps, h, w, [jpeg bytes]) of a file `write_avi` wrote (one MJPG video stream)."""
    with open(path, "rb") as fh:
        data = fh.read()
    if data[:4] != b"RIFF" or data[8:12] != b"AVI " or struct.unpack_from("<I", data, 4)[0] + 8 != len(data):
        raise ValueError(f"{path}: not a RIFF AVI file of the stated length")
    fps = h = w = None
    frames = []
    for tag, off, size in _chunks(data, 12, len(data)):
        if tag != b"LIST":
            continue
        kind = data[off:off + 4]
        if kind == b"hdrl":
            for t2, o2, s2 in _chunks(data, off + 4, off + size):
                if t2 == b"LIST" and data[o2:o2 + 4] == b"strl":
                    for t3, o3, s3 in _chunks(data, o2 + 4, o2 + s2):
                        if t3 == b"strh":
                            if data[o3:o3 + 8] != b"vidsMJPG":
                                raise ValueError(f"{path}: the stream is not MJPG video")
                            scale, rate = struct.unpack_from("<II", data, o3 + 20)
                            fps = rate // scale
                        elif t3 == b"strf":
                            w, h = struct.unpack_from("<ii", data, o3 + 4)
        elif kind == b"movi":
            frames = [bytes(data[o2:o2 + s2]) for t2, o2, s2 in _chunks(data, off + 4, off + size) if t2 == b"00dc"]
    if fps is None or h is None:
        raise ValueError(f"{path}: no video stream header")
    return fps, h, w, frames


# ---- reading other writers' files frame by frame: headers and index only, payloads by seek + read
_REENCODE = "re-encode it once as Motion-JPEG AVI (e.g. `ffmpeg -i IN -c:v mjpeg -q:v 2 -an OUT.avi`)"


def _head(fh, pos, n=8):
    fh.seek(pos)
    return fh.read(n)


def probe_avi(path):
    """(fps, h, w, n_frames, index) of a Motion-JPEG AVI file without reading a frame: `index` is a list of (payload offset in the file,
    payload bytes) per video frame, from `idx1` (offsets counted from the 'movi' tag or from the file start) or, where there is none,
    from a walk over the chunk headers of 'movi' with seeks.  JUNK chunks, LIST INFO / odml, 'LIST rec ' groups and other streams'
    chunks (01wb) are stepped over.  ValueError, naming the file and the reason: not RIFF AVI, a RIFF length that is not the file's,
    RIFF AVIX extensions (OpenDML), no or a non-MJPG video stream, zero-length video chunks (dropped frames: a frame number would no
    longer mean a picture), an index that points outside 'movi'."""
    import os
    size = os.path.getsize(path)
    with open(path, "rb") as fh:
        head = fh.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"AVI ":
            raise ValueError(f"{path}: not a RIFF AVI file ({_REENCODE})")
        riff_end = struct.unpack_from("<I", head, 4)[0] + 8
        if riff_end < size and _head(fh, riff_end + (riff_end & 1), 12)[8:12] == b"AVIX":
            raise ValueError(f"{path}: RIFF AVIX extensions (an OpenDML file of several RIFF chunks) are not read; {_REENCODE}")
        if riff_end != size:
            raise ValueError(f"{path}: the RIFF length says {riff_end} bytes, the file has {size}")
        fps = h = w = stream = movi = idx1 = None
        pos = 12
        while pos + 8 <= size:
            tag, n = struct.unpack("<4sI", _head(fh, pos))
            if pos + 8 + n > size:
                raise ValueError(f"{path}: chunk {tag!r} at {pos} runs past the file")
            if tag == b"LIST":
                kind = fh.read(4)
                if kind == b"hdrl":
                    hdrl = fh.read(n - 4)
                    number = 0
                    try:
                        streams = [(o2, s2) for t2, o2, s2 in _chunks(hdrl, 0, len(hdrl)) if t2 == b"LIST" and hdrl[o2:o2 + 4] == b"strl"]
                        streams = [list(_chunks(hdrl, o2 + 4, o2 + s2)) for o2, s2 in streams]
                    except ValueError as exc:
                        raise ValueError(f"{path}: {exc} (inside the header list)") from None
                    for parts in streams:
                        strh = strf = None
                        for t3, o3, s3 in parts:
                            if t3 == b"strh":
                                strh = hdrl[o3:o3 + s3]
                            elif t3 == b"strf":
                                strf = hdrl[o3:o3 + s3]
                        if strh is not None and strh[:4] == b"vids" and stream is None:
                            if strf is None or len(strh) < 28 or len(strf) < 20:
                                raise ValueError(f"{path}: truncated video stream header")
                            if strh[4:8].upper() != b"MJPG" and strf[16:20].upper() != b"MJPG":
                                raise ValueError(f"{path}: the video stream is {strh[4:8]!r} / {strf[16:20]!r}, not MJPG; {_REENCODE}")
                            scale, rate = struct.unpack_from("<II", strh, 20)
                            if scale == 0 or rate // scale < 1:
                                raise ValueError(f"{path}: frame rate {rate} / {scale}")
                            fps = rate // scale
                            w, h = struct.unpack_from("<ii", strf, 4)
                            w, h, stream = abs(w), abs(h), number
                        number += 1
                elif kind == b"movi":
                    movi = (pos + 8, pos + 8 + n)                     # from the 'movi' tag to the end of the list
            elif tag == b"idx1":
                idx1 = (pos + 8, n)
            pos += 8 + n + (n & 1)
        if stream is None:
            raise ValueError(f"{path}: no video stream header; {_REENCODE}")
        if movi is None:
            raise ValueError(f"{path}: no 'movi' list")
        tags = (b"%02ddc" % stream, b"%02ddb" % stream)
        index = []
        if idx1 is not None and idx1[1] >= 16:
            fh.seek(idx1[0])
            raw = fh.read(idx1[1] - idx1[1] % 16)
            entries = [(off, n) for tag, _, off, n in struct.iter_unpack("<4sIII", raw) if tag in tags]
            if entries:
                # the base of the offsets: the 'movi' tag (the AVI specification) or the file start (some writers); the first entry's own
                # chunk header tells which
                want = [struct.pack("<4sI", t, entries[0][1]) for t in tags]
                for base in (movi[0], 0):
                    at = base + entries[0][0]
                    if movi[0] + 4 <= at and at + 8 <= movi[1] and _head(fh, at) in want:
                        break
                else:
                    raise ValueError(f"{path}: idx1 points at no video chunk, neither counted from 'movi' nor from the file start")
                index = [(base + off + 8, n) for off, n in entries]
        if not index:                                                  # no index: the chunk headers of 'movi', payloads skipped
            pos = movi[0] + 4
            while pos + 8 <= movi[1]:
                tag, n = struct.unpack("<4sI", _head(fh, pos))
                if tag == b"LIST":                                     # 'LIST rec ': its chunks follow its 12-byte header
                    pos += 12
                    continue
                if pos + 8 + n > movi[1]:
                    raise ValueError(f"{path}: chunk {tag!r} at {pos} runs past the 'movi' list")
                if tag in tags:
                    index.append((pos + 8, n))
                pos += 8 + n + (n & 1)
    if not index:
        raise ValueError(f"{path}: no video frames")
    if any(n == 0 for _, n in index):
        k = [n for _, n in index].index(0)
        raise ValueError(f"{path}: video chunk {k} has zero length (a dropped frame): frame numbers would not name pictures; {_REENCODE}")
    if any(off < movi[0] + 12 or off + n > movi[1] for off, n in index):
        raise ValueError(f"{path}: the index points outside the 'movi' list")
    return fps, h, w, len(index), index


def read_avi_frames(path, frame_numbers, index=None):
    """The JPEG files (bytes) of the frames `frame_numbers` of a Motion-JPEG AVI file, in that order: one seek + read per frame,
    nothing else of the file is read.  index: `probe_avi(path)[4]` where the caller has it."""
    if index is None:
        index = probe_avi(path)[4]
    out = []
    with open(path, "rb") as fh:
        for k in frame_numbers:
            k = int(k)
            if not 0 <= k < len(index):
                raise IndexError(f"{path}: frame {k} of {len(index)}")
            off, n = index[k]
            fh.seek(off)
            data = fh.read(n)
            if len(data) != n:
                raise ValueError(f"{path}: frame {k} is cut short")
            out.append(data)
    return out


def decode_frames(jpegs):
    """uint8 [T, H, W, 3] of JPEG files (e.g. `read_avi(path)[3]`), decoded with Pillow."""
    try:
        from PIL import Image
    except ImportError as exc:
        raise ImportError("decode_frames needs Pillow (PIL): the MI355X path has no JPEG decoder of its own") from exc
    import io
    import numpy as np
    return np.stack([np.asarray(Image.open(io.BytesIO(j)).convert("RGB")) for j in jpegs])


# ------------------------------------------------------------------ the host half of the decoder
_UNSUPPORTED_SOF = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential sequential", 0xC6: "differential progressive",
                    0xC7: "differential lossless", 0xC9: "arithmetic-coded", 0xCA: "arithmetic-coded progressive", 0xCB: "arithmetic-coded lossless",
                    0xCD: "arithmetic-coded differential", 0xCE: "arithmetic-coded differential progressive", 0xCF: "arithmetic-coded differential lossless"}
SAMPLING = {(1, 1): 0, (2, 1): 1, (2, 2): 2}      # luminance (h, v) factors -> Pillow's `subsampling` number: 4:4:4, 4:2:2, 4:2:0
TABLE_BYTES = 4008


def parse_jpeg(data):
    """dict of one baseline JPEG file: h, w, sampling (0 / 1 / 2), quant (per component, 64 values in natural order), huffman
    ({class/id byte: (bits, vals)}; the Annex K tables for a file without DHT), dc_tables / ac_tables (table id per component),
    restart_interval (0: none), scan_offset, scan_length (the entropy-coded bytes between the SOS header and EOI).  ValueError
    says what is malformed or outside what the decoder takes."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise ValueError("parse_jpeg: no SOI marker at the start")
    if len(data) < 4 or data[-2:] != EOI:
        raise ValueError("parse_jpeg: no EOI marker at the end")
    qt, huff, sof, ri, pos = {}, {}, None, 0, 2
    while True:
        if pos + 4 > len(data) - 2:
            raise ValueError(f"parse_jpeg: truncated: no segment header at byte {pos}, no SOS so far")
        if data[pos] != 0xFF or data[pos + 1] in (0x00, 0xFF):
            raise ValueError(f"parse_jpeg: no marker at byte {pos}")
        marker, length = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        if length < 2 or pos + 2 + length > len(data) - 2:
            raise ValueError(f"parse_jpeg: truncated segment {marker:#04x} at byte {pos}: length {length}")
        p = data[pos + 4:pos + 2 + length]
        pos += 2 + length
        if marker in _UNSUPPORTED_SOF:
            raise ValueError(f"parse_jpeg: {_UNSUPPORTED_SOF[marker]} JPEG (SOF{marker - 0xC0}) is not decoded, only baseline (SOF0)")
        if marker == 0xCC:
            raise ValueError("parse_jpeg: arithmetic coding (DAC) is not decoded")
        if marker == 0xDB:
            i = 0
            while i < len(p):
                if p[i] >> 4:
                    raise ValueError("parse_jpeg: 16-bit quantiser tables belong to 12-bit JPEG, which is not decoded")
                if (p[i] & 15) > 3 or i + 65 > len(p):
                    raise ValueError("parse_jpeg: malformed DQT segment")
                nat = [0] * 64
                for k in range(64):
                    nat[ZIGZAG[k]] = p[i + 1 + k]
                qt[p[i] & 15] = tuple(nat)
                i += 65
        elif marker == 0xC4:
            i = 0
            while i < len(p):
                if i + 17 > len(p) or (p[i] >> 4) > 1 or (p[i] & 15) > 1:
                    raise ValueError("parse_jpeg: malformed DHT segment, or a table id that baseline JPEG does not have")
                bits = bytes(p[i + 1:i + 17])
                if sum(bits) > 256 or i + 17 + sum(bits) > len(p):
                    raise ValueError("parse_jpeg: malformed DHT segment")
                huff[p[i]] = (bits, bytes(p[i + 17:i + 17 + sum(bits)]))
                i += 17 + sum(bits)
        elif marker == 0xC0:
            if sof is not None or len(p) < 6 or len(p) != 6 + 3 * p[5]:
                raise ValueError("parse_jpeg: malformed or repeated SOF0 segment")
            if p[0] != 8:
                raise ValueError(f"parse_jpeg: {p[0]}-bit samples are not decoded, only 8 bit")
            if p[5] != 3:
                raise ValueError(f"parse_jpeg: {p[5]} component(s) ({ {1: 'greyscale', 4: 'CMYK'}.get(p[5], 'unusual') }) are not decoded, only three (YCbCr)")
            sof = ((p[1] << 8) | p[2], (p[3] << 8) | p[4], [(p[6 + 3 * c], p[7 + 3 * c] >> 4, p[7 + 3 * c] & 15, p[8 + 3 * c]) for c in range(3)])
        elif marker == 0xDD:
            if len(p) != 2:
                raise ValueError("parse_jpeg: malformed DRI segment")
            ri = (p[0] << 8) | p[1]
        elif marker == 0xDA:
            if sof is None:
                raise ValueError("parse_jpeg: SOS before SOF0")
            if len(p) < 1 or p[0] != 3 or len(p) != 10:
                raise ValueError("parse_jpeg: not one interleaved scan of the three components")
            if [p[1 + 2 * c] for c in range(3)] != [c[0] for c in sof[2]] or tuple(p[7:10]) != (0, 63, 0):
                raise ValueError("parse_jpeg: the scan header does not name the frame's components in order with Ss = 0, Se = 63, Ah = Al = 0")
            dc, ac = [p[2 + 2 * c] >> 4 for c in range(3)], [p[2 + 2 * c] & 15 for c in range(3)]
            break
        elif not (0xE0 <= marker <= 0xEF or marker == 0xFE):
            raise ValueError(f"parse_jpeg: marker {marker:#04x} is not expected in a baseline file")
    h, w, comps = sof
    if h < 1 or w < 1:
        raise ValueError(f"parse_jpeg: frame size {h} x {w}")
    factors = [c[1:3] for c in comps]
    if factors[1] != (1, 1) or factors[2] != (1, 1) or factors[0] not in SAMPLING:
        raise ValueError(f"parse_jpeg: sampling factors {factors} are not decoded, only luminance 1x1, 2x1 or 2x2 against 1x1 chrominance")
    sampling = SAMPLING[factors[0]]
    if sampling and w <= 4:
        raise ValueError(f"parse_jpeg: a subsampled frame {w} pixels wide has fewer than 3 chrominance columns; libjpeg takes another path there, which is not reproduced")
    if any(c[3] not in qt for c in comps):
        raise ValueError("parse_jpeg: a component names a quantiser table the file does not define")
    if not huff:
        huff = dict(HUFF)                       # Motion-JPEG frames may rely on the Annex K tables, as libjpeg lets them
    if any(d > 1 or a > 1 or d not in huff or (0x10 | a) not in huff for d, a in zip(dc, ac)):
        raise ValueError("parse_jpeg: the scan names a Huffman table the file does not define")
    return {"h": h, "w": w, "sampling": sampling, "quant": tuple(qt[c[3]] for c in comps), "huffman": huff, "dc_tables": tuple(dc), "ac_tables": tuple(ac),
            "restart_interval": ri, "scan_offset": pos, "scan_length": len(data) - 2 - pos}


def mcu_grid(h, w, sampling):
    """(MCUs per row, MCU rows) of an h x w frame."""
    hs, vs = ((1, 1), (2, 1), (2, 2))[sampling]
    return -(-w // (8 * hs)), -(-h // (8 * vs))


def find_units(scans, offsets, restart_intervals, n_mcu):
    """The unit table of the scans of a call's frames: int64 [units, 5] of (frame, byte offset, byte length, first MCU, MCUs).  scans:
    the entropy-coded bytes of all frames one behind the other, frame f at scans[offsets[f]:offsets[f + 1]]; restart_intervals: per
    frame, 0 = no DRI (the whole scan is one unit); n_mcu: the MCUs of a frame.  The RSTn markers of all frames are found in one numpy
    pass.  ValueError, naming the frame, for any other marker inside a scan, a 0xFF at its end, markers out of order (RSTn counts modulo
    8 from 0) or a number of units other than ceil(n_mcu / restart interval)."""
    import numpy as np
    a = np.frombuffer(bytes(scans), dtype=np.uint8) if not isinstance(scans, np.ndarray) else scans
    offsets = np.asarray(offsets, dtype=np.int64)
    ri = np.asarray(restart_intervals, dtype=np.int64)
    n = ri.size
    assert offsets.size == n + 1 and offsets[0] == 0 and offsets[-1] == a.size and (np.diff(offsets) >= 0).all()
    ff = np.flatnonzero(a == 0xFF)
    fr = np.searchsorted(offsets, ff, side="right") - 1            # the frame of every 0xFF
    at_end = ff == offsets[fr + 1] - 1
    if at_end.any():
        raise ValueError(f"find_units: frame {int(fr[at_end][0])}: the scan ends in 0xFF")
    nxt = a[ff + 1]
    is_rst = (nxt >= 0xD0) & (nxt <= 0xD7)
    other = (nxt != 0) & ~is_rst
    if other.any():
        k = int(np.flatnonzero(other)[0])
        raise ValueError(f"find_units: frame {int(fr[k])}: marker 0xff{int(nxt[k]):02x} at byte {int(ff[k] - offsets[fr[k]])} of the scan (only RSTn may stand there)")
    rst, rfr = ff[is_rst], fr[is_rst]
    counts = np.bincount(rfr, minlength=n)                          # markers per frame
    want = np.where(ri > 0, -(-n_mcu // np.maximum(ri, 1)), 1)
    if (counts + 1 != want).any():
        f = int(np.flatnonzero(counts + 1 != want)[0])
        raise ValueError(f"find_units: frame {f}: {int(counts[f]) + 1} unit(s) in the scan, {int(want[f])} expected for {n_mcu} MCUs at restart interval {int(ri[f])}")
    k = np.arange(rst.size) - np.repeat(np.cumsum(counts) - counts, counts)      # a marker's number within its frame
    wrong = nxt[is_rst] - 0xD0 != k % 8
    if wrong.any():
        m = int(np.flatnonzero(wrong)[0])
        raise ValueError(f"find_units: frame {int(rfr[m])}: restart marker {int(k[m])} is RST{int(nxt[is_rst][m]) - 0xD0}, RST{int(k[m]) % 8} expected")
    first_unit = np.cumsum(want) - want                             # a frame's first row of the table
    units = np.empty((int(want.sum()), 5), dtype=np.int64)
    is_first = np.zeros(units.shape[0], dtype=bool)
    is_first[first_unit] = True
    is_last = np.zeros(units.shape[0], dtype=bool)
    is_last[first_unit + counts] = True
    units[:, 0] = np.repeat(np.arange(n), want)
    units[is_first, 1], units[~is_first, 1] = offsets[:-1], rst + 2
    ends = np.empty(units.shape[0], dtype=np.int64)
    ends[is_last], ends[~is_last] = offsets[1:], rst
    units[:, 2] = ends - units[:, 1]
    step = ri[units[:, 0]]
    units[:, 3] = (np.arange(units.shape[0]) - first_unit[units[:, 0]]) * step
    units[:, 4] = np.minimum(np.where(step > 0, step, n_mcu), n_mcu - units[:, 3])
    return units


_HUFF_DTYPE = [("look", "<u2", 256), ("maxcode", "<i4", 17), ("valoff", "<i4", 17), ("vals", "u1", 256)]
_TABLE_DTYPE = [("q", "<u2", (3, 64)), ("dc_sel", "u1", 3), ("ac_sel", "u1", 3), ("pad", "u1", 2), ("huff", _HUFF_DTYPE, 4)]


def huffman_table(bits, vals):
    """(look [256], maxcode [17], valoff [17], vals [256]) of a DHT table: codes assigned as T.81 Annex C does, decoded as F.2.2.3
    does -- maxcode[l] the largest code of length l (-1: none), valoff[l] the index of its first symbol minus its first code -- behind
    look[8 bits ahead] = (length << 8) | symbol for the codes of up to 8 bits.  ValueError where the lengths do not form a prefix code."""
    import numpy as np
    bits, vals = list(bits), list(vals)
    if len(bits) != 16 or len(vals) != sum(bits) or len(vals) > 256:
        raise ValueError("huffman_table: bits / vals of the wrong length")
    look, maxcode, valoff = np.zeros(256, np.uint16), np.full(17, -1, np.int32), np.zeros(17, np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        if bits[length - 1]:
            valoff[length] = k - code
            for _ in range(bits[length - 1]):
                if length <= 8:
                    look[code << (8 - length):(code + 1) << (8 - length)] = (length << 8) | vals[k]
                code, k = code + 1, k + 1
            maxcode[length] = code - 1
            if code > (1 << length):
                raise ValueError("huffman_table: the code lengths do not form a prefix code")
        code <<= 1
    out = np.zeros(256, np.uint8)
    out[:len(vals)] = vals
    return look, maxcode, valoff, out


_HUFF_CACHE = {}


def decode_tables(parsed):
    """The table record of a parsed frame: TABLE_BYTES bytes as include/ccvs_hip_decode.h lays them out."""
    import numpy as np
    rec = np.zeros((), dtype=_TABLE_DTYPE)
    rec["q"] = np.asarray(parsed["quant"], dtype=np.uint16)
    rec["dc_sel"], rec["ac_sel"] = parsed["dc_tables"], parsed["ac_tables"]
    for slot, key in enumerate((0x00, 0x01, 0x10, 0x11)):
        if key in parsed["huffman"]:
            bv = tuple(bytes(x) for x in parsed["huffman"][key])
            if bv not in _HUFF_CACHE:
                _HUFF_CACHE[bv] = huffman_table(*bv)
            for name, value in zip(("look", "maxcode", "valoff", "vals"), _HUFF_CACHE[bv]):
                rec["huff"][name][slot] = value
        else:
            rec["huff"]["maxcode"][slot] = -1            # a table no component uses: no code is valid
    out = rec.tobytes()
    assert len(out) == TABLE_BYTES
    return out


def plan_frames(jpegs):
    """Everything `ccvs_mjpeg_decode` takes for the frames of one call (files of one size and sampling): dict of n, h, w, sampling, scans
    (uint8, all scans one behind the other), units (int64 [units, 5]), tables (uint8, the distinct table records), frame_table
    (int32 [n], the record of every frame).  ValueError names the frame that does not parse or does not match frame 0."""
    import numpy as np
    if not len(jpegs):
        raise ValueError("plan_frames: no frames")
    scans, intervals, records, frame_table, first = [], [], {}, [], None
    head = p = record = None
    for f, data in enumerate(jpegs):
        data = bytes(data)
        # the frames of a clip mostly share their header byte for byte: the same bytes parse to the same fields and the same record
        if head is None or not (data.startswith(head) and data.endswith(EOI) and len(data) >= len(head) + 2):
            try:
                p = parse_jpeg(data)
            except ValueError as exc:
                raise ValueError(f"frame {f}: {exc}") from None
            head, record = data[:p["scan_offset"]], decode_tables(p)
            geom = (p["h"], p["w"], p["sampling"])
            if first is None:
                first = geom
            elif geom != first:
                raise ValueError(f"frame {f}: size and sampling {geom} differ from frame 0's {first}")
        scans.append(data[len(head):-2])
        intervals.append(p["restart_interval"])
        frame_table.append(records.setdefault(record, len(records)))
    mx, my = mcu_grid(*first)
    stream = np.frombuffer(b"".join(scans), dtype=np.uint8)
    units = find_units(stream, np.cumsum([0] + [len(x) for x in scans]), intervals, mx * my)
    return {"n": len(jpegs), "h": first[0], "w": first[1], "sampling": first[2], "scans": stream,
            "units": units, "tables": np.frombuffer(b"".join(records), dtype=np.uint8), "frame_table": np.asarray(frame_table, dtype=np.int32)}

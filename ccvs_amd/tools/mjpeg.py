"""Motion-JPEG AVI files around the scans `ops.mjpeg_encode` writes.  Host only: no torch, no GPU.

  jpeg_header(h, w, quality, restart_mcus)   the bytes in front of a frame's scan: SOI, DQT x 2, SOF0 (8 bit, three components sampled
                                             1 x 1), DHT x 4 (the Annex K tables), DRI, SOS.  header + scan + EOI is a JPEG file.
  write_avi(path, frames, fps, h, w)         RIFF 'AVI ': hdrl (avih, one strl: strh vids/MJPG + strf BITMAPINFOHEADER), a movi list of
                                             '00dc' chunks padded to even length, idx1.
  read_avi(path) -> (fps, h, w, [jpeg])      the frames of such a file, byte for byte.
  decode_frames(jpegs) -> uint8 [T, H, W, 3] with Pillow (ImportError where it is missing): the `loader=` a caller can hand to
                                             `metrics_from_files` after `read_avi`.
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


def default_restart(w):
    """The encoder's default restart interval in MCUs: one row of MCUs, 32 at the most."""
    return min((int(w) + 7) // 8, 32)


def quant_tables(quality):
    """libjpeg's `jpeg_set_quality` (baseline): the two tables in natural order."""
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError(f"JPEG quality {quality} outside 1 .. 100")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(tuple(min(max((b * scale + 50) // 100, 1), 255) for b in base) for base in BASE_Q)


def _segment(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


def jpeg_header(h, w, quality, restart_mcus=None):
    """Everything in front of the scan of an h x w frame encoded at `quality` with a restart interval of `restart_mcus` MCUs."""
    h, w = int(h), int(w)
    r = default_restart(w) if restart_mcus is None else int(restart_mcus)
    if not (1 <= h <= 65535 and 1 <= w <= 65535 and 1 <= r <= 32):
        raise ValueError(f"jpeg_header: size {h} x {w} or restart interval {r} out of range")
    out = b"\xff\xd8"
    for t, table in enumerate(quant_tables(quality)):
        out += _segment(0xDB, bytes([t]) + bytes(table[k] for k in ZIGZAG))
    out += _segment(0xC0, struct.pack(">BHHB", 8, h, w, 3) + bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for key, (bits, vals) in HUFF.items():
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


def decode_frames(jpegs):
    """uint8 [T, H, W, 3] of JPEG files (e.g. `read_avi(path)[3]`), decoded with Pillow."""
    try:
        from PIL import Image
    except ImportError as exc:
        raise ImportError("decode_frames needs Pillow (PIL): the MI355X path has no JPEG decoder of its own") from exc
    import io
    import numpy as np
    return np.stack([np.asarray(Image.open(io.BytesIO(j)).convert("RGB")) for j in jpegs])

"""APNG on the host: the container around the zlib streams `ops.png_encode` makes on the GPU, and a reader for
8-bit RGB PNG / APNG files.  The counterpart of `tools/mjpeg.py` for the lossless clips `--video_format apng` writes.

  write_apng(path, zstreams, fps, h, w)   signature, IHDR (8-bit, colour type 2, no interlace), acTL (T frames, played for ever), then per
                                          frame an fcTL (the full frame, delay 1 / fps, dispose none, blend source) and the frame's zlib
                                          stream as IDAT (frame 0) or fdAT (the others), then IEND.  Every frame is a whole image; a
                                          player that knows nothing of APNG shows frame 0.
  read_apng(path) -> uint8 [T, H, W, 3]   walks the chunks, checks their CRCs, inflates with zlib and undoes the filters in numpy.  It
                                          reads anybody's RGB8 non-interlaced PNG or full-frame APNG and says why it refuses another.
  apng_streams(data_or_path) -> (h, w, [zlib stream per frame])   the same walk without the inflate: what `ops.png_decode` takes
                                          (DESIGN.md section 4.23); png_gpu_decodable(path) is the header probe in front of it.
Nothing here touches the GPU.
"""
import struct
import zlib
from fractions import Fraction

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunk(tag, payload):
    return struct.pack(">I", len(payload)) + tag + payload + struct.pack(">I", zlib.crc32(tag + payload) & 0xFFFFFFFF)


def delay_fraction(fps):
    """1 / fps as (numerator, denominator), both below 65536: fcTL's delay."""
    d = (1 / Fraction(fps)).limit_denominator(65535)
    if not (0 <= d.numerator <= 65535 and d.denominator >= 1) or d <= 0:
        raise ValueError(f"write_apng: fps {fps!r} gives no frame delay that fits 16-bit parts")
    return d.numerator, d.denominator


def write_apng(path, zstreams, fps, h, w):
    """Write the frames' zlib streams (bytes each, in order) as one APNG of h x w 8-bit RGB frames at `fps`."""
    zstreams = list(zstreams)
    if not zstreams:
        raise ValueError("write_apng: no frames")
    if not (1 <= h < 2 ** 31 and 1 <= w < 2 ** 31):
        raise ValueError(f"write_apng: size {h} x {w}")
    num, den = delay_fraction(fps)
    out = [SIGNATURE, _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)), _chunk(b"acTL", struct.pack(">II", len(zstreams), 0))]
    seq = 0
    for i, z in enumerate(zstreams):
        out.append(_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, w, h, 0, 0, num, den, 0, 0)))
        seq += 1
        if i == 0:
            out.append(_chunk(b"IDAT", bytes(z)))
        else:
            out.append(_chunk(b"fdAT", struct.pack(">I", seq) + bytes(z)))
            seq += 1
    out.append(_chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(b"".join(out))


def chunks(data):
    """[(tag, payload)] of a PNG file's bytes; ValueError on a bad signature, a chunk that runs past the end or a wrong CRC."""
    if data[:8] != SIGNATURE:
        raise ValueError("read_apng: not a PNG file (signature)")
    out, pos = [], 8
    while pos < len(data):
        if pos + 12 > len(data):
            raise ValueError(f"read_apng: a chunk header at byte {pos} runs past the end of the file")
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        if pos + 12 + n > len(data):
            raise ValueError(f"read_apng: chunk {tag!r} at byte {pos} runs past the end of the file")
        payload = data[pos + 8:pos + 8 + n]
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != zlib.crc32(tag + payload) & 0xFFFFFFFF:
            raise ValueError(f"read_apng: chunk {tag!r} at byte {pos} has a wrong CRC")
        out.append((tag, payload))
        pos += 12 + n
        if tag == b"IEND":
            break
    return out


def unfilter(raws, h, w):
    """The inverse of PNG's row filters for bpp = 3: the inflated bytes of T images of one size -> uint8 [T, h, w, 3].  A pixel needs
    its left, upper and upper-left neighbours, which lie on the two anti-diagonals before its own: the images are walked one
    anti-diagonal at a time, all rows, channels and frames of it in one numpy step."""
    rb = 3 * w
    for i, raw in enumerate(raws):
        if len(raw) != h * (rb + 1):
            raise ValueError(f"read_apng: frame {i} inflates to {len(raw)} bytes, not {h} rows of {rb + 1}")
    rows = np.frombuffer(b"".join(raws), np.uint8).reshape(len(raws), h, rb + 1)
    types = rows[:, :, 0].astype(np.int64)
    if types.max(initial=0) > 4:
        t, y = np.argwhere(types > 4)[0]
        raise ValueError(f"read_apng: frame {t}, row {y} has filter type {types[t, y]}")
    res = rows[:, :, 1:].reshape(len(raws), h, w, 3).astype(np.int64)
    out = np.zeros((len(raws), h + 1, w + 1, 3), np.int64)              # a row of zeros above and a column of zeros to the left
    if types.max(initial=0) == 0:
        return res.astype(np.uint8)
    for d in range(h + w - 1):
        ys = np.arange(max(0, d - w + 1), min(h, d + 1))
        xs = d - ys
        a, b, c = out[:, ys + 1, xs], out[:, ys, xs + 1], out[:, ys, xs]
        t = types[:, ys][..., None]
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        pred = np.where(t == 1, a, np.where(t == 2, b, np.where(t == 3, (a + b) >> 1, np.where(t == 4, paeth, 0))))
        out[:, ys + 1, xs + 1] = (res[:, ys, xs] + pred) & 255
    return out[:, 1:, 1:].astype(np.uint8)


def apng_streams(data_or_path):
    """(h, w, [the zlib stream of every frame, bytes]) of an 8-bit RGB, non-interlaced PNG (one frame) or APNG whose frames are all full
    frames with blend = source and dispose = none: the chunk walk, CRC check and refusals of `read_apng`, without the inflate.  Takes
    the file's bytes or its path."""
    if isinstance(data_or_path, (bytes, bytearray, memoryview)):
        data = bytes(data_or_path)
    else:
        with open(data_or_path, "rb") as f:
            data = f.read()
    cs = chunks(data)
    if not cs or cs[0][0] != b"IHDR" or len(cs[0][1]) != 13:
        raise ValueError("read_apng: the first chunk is not an IHDR")
    w, h, depth, colour, comp, flt, interlace = struct.unpack(">IIBBBBB", cs[0][1])
    if colour != 2:
        raise ValueError(f"read_apng: colour type {colour} is not 2 (RGB)")
    if depth != 8:
        raise ValueError(f"read_apng: bit depth {depth} is not 8")
    if interlace != 0:
        raise ValueError("read_apng: interlaced (Adam7) files are not read")
    if comp != 0 or flt != 0:
        raise ValueError(f"read_apng: compression method {comp} / filter method {flt}")
    animated = any(tag == b"acTL" for tag, _ in cs)
    frames, current, want_seq, idat = [], None, 0, []
    for tag, payload in cs[1:]:
        if tag == b"fcTL":
            seq, fw, fh, x0, y0, _, _, dispose, blend = struct.unpack(">IIIIIHHBB", payload)
            if seq != want_seq:
                raise ValueError(f"read_apng: sequence number {seq} where {want_seq} is due")
            want_seq += 1
            if (fw, fh, x0, y0) != (w, h, 0, 0):
                raise ValueError(f"read_apng: a partial frame ({fw} x {fh} at {x0}, {y0} of {w} x {h}) is not read")
            if blend != 0 or dispose != 0:
                raise ValueError(f"read_apng: blend {blend} / dispose {dispose} other than source / none are not read")
            if current is not None:
                frames.append(current)
            current = []
        elif tag == b"IDAT":
            idat.append(payload)
            if current is not None:                                     # an fcTL stands before IDAT: the default image is frame 0
                current.append(payload)
        elif tag == b"fdAT":
            seq = struct.unpack(">I", payload[:4])[0]
            if seq != want_seq:
                raise ValueError(f"read_apng: sequence number {seq} where {want_seq} is due")
            want_seq += 1
            if current is None:
                raise ValueError("read_apng: fdAT before any fcTL")
            current.append(payload[4:])
    if current is not None:
        frames.append(current)
    if not idat:
        raise ValueError("read_apng: no IDAT chunk")
    if not animated:
        frames = [idat]
    else:
        count = struct.unpack(">II", next(p for t, p in cs if t == b"acTL"))[0]
        if count != len(frames) or any(not f for f in frames):
            raise ValueError(f"read_apng: acTL says {count} frames, the file holds {sum(bool(f) for f in frames)}")
    return h, w, [b"".join(parts) for parts in frames]


def read_apng(path):
    """uint8 [T, H, W, 3] of an 8-bit RGB, non-interlaced PNG (T = 1) or APNG whose frames are all full frames with blend = source and
    dispose = none.  ValueError names what else the file holds."""
    h, w, streams = apng_streams(path)
    raws = []
    for i, z in enumerate(streams):
        try:
            raws.append(zlib.decompress(z))
        except zlib.error as exc:
            raise ValueError(f"read_apng: frame {i} does not inflate: {exc}") from None
    return unfilter(raws, h, w)


def png_gpu_decodable(path):
    """True where the file's first 29 bytes are a PNG signature and an IHDR of colour type 2 (RGB), bit depth 8, no interlace and the
    standard compression and filter methods: what `ccvs_amd.ops.png_decode` takes.  A cheap probe: nothing else of the file is read."""
    try:
        with open(path, "rb") as f:
            head = f.read(29)
    except OSError:
        return False
    if len(head) < 29 or head[:8] != SIGNATURE or head[8:16] != b"\x00\x00\x00\rIHDR":
        return False
    w, h, depth, colour, comp, flt, interlace = struct.unpack(">IIBBBBB", head[16:29])
    return (depth, colour, comp, flt, interlace) == (8, 2, 0, 0, 0) and 1 <= w <= 65535 and 1 <= h <= 65535

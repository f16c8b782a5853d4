"""GIF on the host: the container around the colour table and the LZW-coded frames `ops.gif_encode` makes on the GPU (DESIGN.md section
4.27), and a small reader for such files.  The counterpart of `tools/apng.py` for the clips `--video_format gif` writes.

  write_gif(path, payloads, palette, fps, h, w)   the file around the frames' payloads and the clip's palette
  read_gif(path) -> uint8 [T, H, W, 3]            a decoder of our own for files of this shape (global table, full frames, no
                                                  transparency, no interlace): what the tests hold against Pillow's

With --video_delta a frame may be the rectangle of what changed, with a transparent index: `write_gif(...,
rects=...)` writes such files and `read_gif(..., delta=True)` composites them.

The files are quantised to 256 colours per clip: they are for showing, not for scoring -- the metrics and FVD commands do not read them.
"""
import struct

import numpy as np


def delay_cs(fps):
    """A frame's delay in centiseconds: max(2, round(100 / fps)).  Browsers play a delay below 2 centiseconds as 10, so 50 frames per
    second is the fastest a GIF can ask for; faster clips are written at that rate."""
    if not fps > 0:
        raise ValueError(f"write_gif: fps {fps!r}")
    d = max(2, int(round(100.0 / fps)))
    if d > 65535:
        raise ValueError(f"write_gif: fps {fps!r} gives no frame delay that fits 16 bits")
    return d


TRANSPARENT = 255   # the transparent index of the changed-rectangle frames


def write_gif(path, payloads, palette, fps, h, w, rects=None):
    """GIF89a: header, logical screen descriptor with a global colour table of 256 entries (`palette`: 768 bytes or uint8 [256, 3]), the
    NETSCAPE2.0 extension (looping for ever), then per frame a graphic control extension (delay `delay_cs(fps)`: max(2, round(100 / fps))
    centiseconds -- browsers treat delays below 2 as 10; no disposal, no transparency), an image descriptor of the full h x w without a
    local table, and the frame's payload (the byte 08, the LZW data in sub-blocks, the byte 00: `ops.gif_encode_to_host`); the trailer.
    rects (None: the file above): per frame the x0, y0, width and height its payload covers (`ops.gif_encode_to_host(delta=True)`; the
    first is the full frame), which the image descriptors then carry; the graphic control extensions' packed byte is 0x04 for the first
    frame (disposal 1: do not dispose) and 0x05 for the others (and the transparent colour flag), with transparent index 255."""
    payloads = list(payloads)
    if not payloads:
        raise ValueError("write_gif: no frames")
    if not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError(f"write_gif: size {h} x {w}")
    pal = np.asarray(palette, np.uint8).reshape(-1).tobytes() if not isinstance(palette, (bytes, bytearray)) else bytes(palette)
    if len(pal) != 768:
        raise ValueError(f"write_gif: a palette of {len(pal)} bytes, not 768")
    gce = b"\x21\xF9\x04\x00" + struct.pack("<H", delay_cs(fps)) + b"\x00\x00"
    desc = b"\x2C" + struct.pack("<HHHHB", 0, 0, w, h, 0)
    if rects is not None:
        rects = [tuple(int(v) for v in r) for r in rects]
        if len(rects) != len(payloads) or rects[0] != (0, 0, w, h):
            raise ValueError(f"write_gif: {len(rects)} rectangles for {len(payloads)} frames, the first {rects[:1]}")
        if any(not (0 <= x0 and 0 <= y0 and rw >= 1 and rh >= 1 and x0 + rw <= w and y0 + rh <= h) for x0, y0, rw, rh in rects):
            raise ValueError(f"write_gif: a rectangle outside the {h} x {w} frame")
    with open(path, "wb") as f:
        f.write(b"GIF89a" + struct.pack("<HHBBB", w, h, 0xF7, 0, 0) + pal)
        f.write(b"\x21\xFF\x0BNETSCAPE2.0\x03\x01\x00\x00\x00")
        for k, p in enumerate(payloads):
            if rects is not None:
                gce = b"\x21\xF9\x04" + (b"\x05" if k else b"\x04") + struct.pack("<HB", delay_cs(fps), TRANSPARENT) + b"\x00"
                desc = b"\x2C" + struct.pack("<HHHHB", *rects[k], 0)
            f.write(gce + desc + bytes(p))
        f.write(b"\x3B")


def _sub_blocks(data, pos, what):
    out = bytearray()
    while True:
        if pos >= len(data):
            raise ValueError(f"read_gif: {what} runs past the end of the file")
        n = data[pos]
        pos += 1
        if n == 0:
            return bytes(out), pos
        if pos + n > len(data):
            raise ValueError(f"read_gif: {what} runs past the end of the file")
        out += data[pos:pos + n]
        pos += n


def lzw_decode(data, min_size, count):
    """`count` indices of LZW data (GIF's variable-width codes, LSB first, deferred clear codes not needed)."""
    clear, eoi = 1 << min_size, (1 << min_size) + 1
    out = np.empty(count, np.uint8)
    n = 0
    acc = nacc = pos = 0
    width, free, prev = min_size + 1, eoi + 1, None
    prefix, suffix, first = [0] * 4096, list(range(256)) + [0] * 3840, list(range(256)) + [0] * 3840
    stack = []
    while n < count:
        while nacc < width:
            if pos >= len(data):
                raise ValueError(f"read_gif: the LZW data ends after {n} of {count} pixels")
            acc |= data[pos] << nacc
            nacc += 8
            pos += 1
        code = acc & ((1 << width) - 1)
        acc >>= width
        nacc -= width
        if code == clear:
            width, free, prev = min_size + 1, eoi + 1, None
            continue
        if code == eoi:
            raise ValueError(f"read_gif: end of information after {n} of {count} pixels")
        if prev is None:
            if code >= clear:
                raise ValueError(f"read_gif: code {code} right after a clear code")
            out[n] = code
            n += 1
            prev = code
            continue
        if code < free:
            cur, head = code, first[code]
        elif code == free and free < 4096:
            cur, head = prev, first[prev]
            stack.append(head)
        else:
            raise ValueError(f"read_gif: code {code} where {free} codes are defined")
        while cur >= clear:
            stack.append(suffix[cur])
            cur = prefix[cur]
        stack.append(cur)
        if free < 4096:
            prefix[free], suffix[free], first[free] = prev, head, first[prev]
            free += 1
            if free == (1 << width) and width < 12:
                width += 1
        prev = code
        while stack and n < count:
            out[n] = stack.pop()
            n += 1
        stack.clear()
    return out


def read_gif(path, with_info=False, delta=False):
    """uint8 [T, H, W, 3] of a GIF whose frames are full images in the global colour table, as `write_gif` writes them.  with_info: also a
    dict of loop (None: no NETSCAPE2.0 extension), the delays in centiseconds and the palette.  Local tables, partial frames, interlace
    and transparency are refused.  delta: partial frames and a transparent index are read, composited over the frames before under
    disposal 0 or 1 (the first frame is to be a full one without transparent pixels); disposal 2 and 3 are refused; the dict then also
    holds the frames' rectangles (x0, y0, width, height), disposals and transparent indices (None: none)."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:6] not in (b"GIF89a", b"GIF87a") or len(data) < 13:
        raise ValueError("read_gif: not a GIF file (signature)")
    w, h, flags = struct.unpack("<HHB", data[6:11])
    if not flags & 0x80:
        raise ValueError("read_gif: no global colour table")
    ncol = 2 << (flags & 7)
    pos = 13 + 3 * ncol
    if pos > len(data):
        raise ValueError("read_gif: the colour table runs past the end of the file")
    pal = np.frombuffer(data, np.uint8, 3 * ncol, 13).reshape(ncol, 3)
    frames, delays, loop, delay = [], [], None, 0
    rects, disposals, clear_idx, disposal, transparent, canvas = [], [], [], 0, None, None
    while True:
        if pos >= len(data):
            raise ValueError("read_gif: no trailer")
        tag = data[pos]
        pos += 1
        if tag == 0x3B:
            break
        if tag == 0x21:
            label = data[pos]
            body, pos = _sub_blocks(data, pos + 1, f"extension {label:#x}")
            if label == 0xF9:
                if len(body) != 4:
                    raise ValueError("read_gif: a graphic control extension of the wrong size")
                if body[0] & 1 and not delta:
                    raise ValueError("read_gif: transparency is not read")
                disposal, transparent = (body[0] >> 2) & 7, body[3] if body[0] & 1 else None
                if disposal > 1 and delta:
                    raise ValueError(f"read_gif: disposal method {disposal} is not read")
                delay = struct.unpack("<H", body[1:3])[0]
            elif label == 0xFF and body[:11] == b"NETSCAPE2.0" and len(body) >= 14 and body[11] == 1:
                loop = struct.unpack("<H", body[12:14])[0]
        elif tag == 0x2C:
            x0, y0, fw, fh, fl = struct.unpack("<HHHHB", data[pos:pos + 9])
            pos += 9
            if (x0, y0, fw, fh) != (0, 0, w, h) and not (delta and frames and fw >= 1 and fh >= 1 and x0 + fw <= w and y0 + fh <= h):
                raise ValueError(f"read_gif: a partial frame ({fw} x {fh} at {x0}, {y0} of {w} x {h}) is not read")
            if fl & 0xC0:
                raise ValueError("read_gif: local colour tables and interlace are not read")
            min_size = data[pos]
            if not 2 <= min_size <= 8:
                raise ValueError(f"read_gif: LZW minimum code size {min_size}")
            body, pos = _sub_blocks(data, pos + 1, f"frame {len(frames)}")
            idx = lzw_decode(body, min_size, fh * fw)
            if idx.max(initial=0) >= ncol:
                raise ValueError(f"read_gif: frame {len(frames)} has an index beyond the colour table")
            if delta:
                shown = pal[idx].reshape(fh, fw, 3)
                seen = np.ones((fh, fw), bool) if transparent is None else (idx != transparent).reshape(fh, fw)
                if canvas is None:
                    if not seen.all():
                        raise ValueError("read_gif: transparent pixels in the first frame")
                    canvas = shown.copy()
                else:
                    canvas = canvas.copy()
                    part = canvas[y0:y0 + fh, x0:x0 + fw]
                    part[seen] = shown[seen]
                frames.append(canvas)
                rects.append((x0, y0, fw, fh))
                disposals.append(disposal)
                clear_idx.append(transparent)
                disposal, transparent = 0, None                          # (a graphic control extension holds for one image)
            else:
                frames.append(pal[idx].reshape(h, w, 3))
            delays.append(delay)
        else:
            raise ValueError(f"read_gif: block {tag:#x} at byte {pos - 1}")
    if not frames:
        raise ValueError("read_gif: no frames")
    out = np.stack(frames)
    info = {"loop": loop, "delays": delays, "palette": pal.copy()}
    if delta:
        info.update(rects=rects, disposals=disposals, transparent=clear_idx)
    return (out, info) if with_info else out

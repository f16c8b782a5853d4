"""Host mirror of the GIF output stage (ccvs_amd/csrc/gif.hip, include/ccvs_hip_output_gif.h), written in plain
integer numpy and Python: the specification the kernels are held to, byte for byte.

  histogram(clip)                      the 32768 bins' pixel counts and channel sums of a clip uint8 [T, H, W, 3]
  median_cut(cnt)                      the occupied bins' boxes
  palette(clip)                        (palette uint8 [256, 3], table uint8 [32768], used)
  indices(clip, table)                 uint8 [T, H, W]
  band_rows_of(w, band_rows), bands    how a frame is cut
  lzw_band(idx, first, last)           one band's (code, width) pairs
  frame_data(idx2d, band_rows)         a frame's packed LZW bytes
  payload(data)                        08, the sub-blocks, 00
  encode(clip, band_rows)              (stream bytes, offsets, palette, table, used) of a clip -- what `ops.gif_encode` gives
  stream_bound(n, h, w, band_rows)     `ccvs_gif_stream_bound`
  gif_file(payloads, palette, fps, h, w)   the whole file as bytes -- what `tools.gif.write_gif` writes
"""
import functools
import struct

import numpy as np

NBINS = 32768
CLEAR, EOI, FIRST, FULL = 256, 257, 258, 4096
DEFAULT_BAND = 4096


# ---------------------------------------------------------------- palette
def bins_of(rgb):
    rgb = np.asarray(rgb, np.uint8).astype(np.int64)
    return ((rgb[..., 0] >> 3) << 10) | ((rgb[..., 1] >> 3) << 5) | (rgb[..., 2] >> 3)


def histogram(clip):
    clip = np.asarray(clip, np.uint8).reshape(-1, 3)
    b = bins_of(clip)
    cnt = np.bincount(b, minlength=NBINS).astype(np.int64)
    sums = np.stack([np.bincount(b, weights=clip[:, c].astype(np.float64), minlength=NBINS) for c in range(3)], 1)
    return cnt, np.rint(sums).astype(np.int64)   # (float64 sums of integers below 2^53 are exact)


def _coords(bins):
    return np.stack([bins >> 10, (bins >> 5) & 31, bins & 31], 1)


def median_cut(cnt):
    """(occupied bins ascending, their box numbers, number of boxes) of the counts [32768]."""
    cnt = np.asarray(cnt, np.int64)
    occ = np.nonzero(cnt)[0]
    if occ.size == 0:
        raise ValueError("median_cut: no pixels")
    xyz, pop = _coords(occ), cnt[occ]
    box = np.zeros(occ.size, np.int64)
    nbox = 1

    def rate(k):                                                 # (population x longest extent, the axis of that extent)
        m = box == k
        ext = xyz[m].max(0) - xyz[m].min(0)
        longest = int(ext.max())
        axis = 1 if ext[1] == longest else (0 if ext[0] == longest else 2)   # ties: G, then R, then B
        return int(pop[m].sum()) * longest, axis                 # Python integers: no overflow

    rated = [rate(0)]
    while nbox < 256:
        best, best_score = -1, 0
        for k in range(nbox):                                    # (a box of two bins or more has an extent, so a score above 0)
            if rated[k][0] > best_score:                         # ties: the lowest box
                best, best_score = k, rated[k][0]
        if best < 0:
            break
        best_axis = rated[best][1]
        m = box == best
        c = xyz[m, best_axis]
        lo, hi, total = int(c.min()), int(c.max()), int(pop[m].sum())
        marg = np.zeros(32, np.int64)
        np.add.at(marg, c, pop[m])
        run, cut = 0, hi - 1
        for v in range(lo, hi):
            run += int(marg[v])
            if run >= (total + 1) // 2:
                cut = v
                break
        box[m & (xyz[:, best_axis] > cut)] = nbox
        rated[best] = rate(best)
        rated.append(rate(nbox))
        nbox += 1
    return occ, box, nbox


def _mean(s, n):
    return (2 * s + n) // (2 * n)


def palette(clip):
    cnt, sums = histogram(clip)
    return palette_of(cnt, sums)


def palette_of(cnt, sums):
    occ, box, used = median_cut(cnt)
    pal = np.zeros((256, 3), np.int64)
    for k in range(used):
        m = box == k
        n = int(cnt[occ[m]].sum())
        pal[k] = [_mean(int(sums[occ[m], c].sum()), n) for c in range(3)]
    own = _mean(sums[occ], cnt[occ][:, None])
    d = ((own[:, None, :] - pal[None, :used, :]) ** 2).sum(-1)
    table = np.zeros(NBINS, np.uint8)
    table[occ] = d.argmin(1).astype(np.uint8)                    # (argmin: the first of equals)
    return pal.astype(np.uint8), table, used


def indices(clip, table):
    return np.asarray(table, np.uint8)[bins_of(clip)]


# ---------------------------------------------------------------- LZW
def band_rows_of(w, band_rows):
    return int(band_rows) if band_rows > 0 else max(1, DEFAULT_BAND // int(w))


def bands(h, w, band_rows):
    r = band_rows_of(w, band_rows)
    return (h + r - 1) // r


def lzw_band(idx, first, last):
    """The (code, width) pairs of one band's indices (a flat sequence of at least one)."""
    idx = [int(v) for v in np.asarray(idx).reshape(-1)]
    out = [(CLEAR, 9)] if first else []
    table, free, width = {}, FIRST, 9
    prefix = idx[0]
    for c in idx[1:]:
        key = (prefix << 8) | c
        hit = table.get(key)
        if hit is not None:
            prefix = hit
            continue
        out.append((prefix, width))
        if free < FULL:
            table[key] = free
            free += 1
            if free > (1 << width) and width < 12:
                width += 1
        if free >= FULL:
            out.append((CLEAR, width))
            table, free, width = {}, FIRST, 9
        prefix = c
    out.append((prefix, width))
    if free < FULL:
        free += 1
        if free > (1 << width) and width < 12:
            width += 1
    out.append((EOI if last else CLEAR, width))
    return out


def pack(pairs):
    """LSB-first bytes of (code, width) pairs, the last byte padded with zero bits."""
    codes = np.array([p[0] for p in pairs], np.int64)
    widths = np.array([p[1] for p in pairs], np.int64)
    bits = (codes[:, None] >> np.arange(12)[None, :]) & 1
    keep = np.arange(12)[None, :] < widths[:, None]
    return np.packbits(bits[keep].astype(np.uint8), bitorder="little").tobytes()


def frame_pairs(idx2d, band_rows=0):
    idx2d = np.asarray(idx2d)
    h, w = idx2d.shape
    r, nb = band_rows_of(w, band_rows), bands(h, w, band_rows)
    pairs = []
    for b in range(nb):
        pairs += lzw_band(idx2d[b * r:(b + 1) * r], b == 0, b == nb - 1)
    return pairs


def frame_data(idx2d, band_rows=0):
    return pack(frame_pairs(idx2d, band_rows))


def payload(data):
    out = bytearray([8])
    for k in range(0, len(data), 255):
        blk = data[k:k + 255]
        out.append(len(blk))
        out += blk
    out.append(0)
    return bytes(out)


def encode_indices(idx, band_rows=0):
    """(stream, offsets) of index frames [n, H, W]."""
    parts = [payload(frame_data(f, band_rows)) for f in np.asarray(idx)]
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return b"".join(parts), off


def encode(clip, band_rows=0):
    clip = np.asarray(clip, np.uint8)
    pal, table, used = palette(clip)
    stream, off = encode_indices(indices(clip, table), band_rows)
    return stream, off, pal, table, used


def stream_bound(n, h, w, band_rows=0):
    r, nb = band_rows_of(w, band_rows), bands(h, w, band_rows)

    def band_bits(rows):
        L = rows * w
        return 12 * (L + L // 3838 + 2)
    bits = (nb - 1) * band_bits(min(r, h)) + band_bits(h - (nb - 1) * r)
    data = (bits + 7) // 8
    return n * (2 + data + (data + 254) // 255)


# ---------------------------------------------------------------- the file
def delay_cs(fps):
    return max(2, int(round(100.0 / fps)))


def gif_file(payloads, pal, fps, h, w):
    out = bytearray(b"GIF89a")
    out += struct.pack("<HHBBB", w, h, 0xF7, 0, 0)               # a global table of 256 entries, 8 bits of colour resolution
    out += np.asarray(pal, np.uint8).reshape(256, 3).tobytes()
    out += b"\x21\xFF\x0BNETSCAPE2.0\x03\x01\x00\x00\x00"         # loop for ever
    for p in payloads:
        out += b"\x21\xF9\x04\x00" + struct.pack("<H", delay_cs(fps)) + b"\x00\x00"
        out += b"\x2C" + struct.pack("<HHHHB", 0, 0, w, h, 0)
        out += p
    out += b"\x3B"
    return bytes(out)


# ---------------------------------------------------------------- the cases both test modules share (computed once)
BAND_SWEEP = (list(range(250, 263)) + list(range(506, 520)) + list(range(760, 775)) + list(range(1784, 1798))
              + list(range(3830, 3848)))                          # band ends around every change of the code width and the full table
SWEEP_TAIL = 37                                                   # indices of the band that follows


def direct_colours():
    """256 colours in 256 different bins and the table that maps colour i to index i: frames of chosen INDICES for `ccvs_gif_encode`."""
    i = np.arange(256)
    colours = np.stack([(i & 31) << 3, (i >> 5) << 3, np.zeros(256, np.int64)], 1).astype(np.uint8)
    table = np.zeros(NBINS, np.uint8)
    table[bins_of(colours)] = i
    return colours, table


@functools.lru_cache(None)
def sweep_indices(L, kind):
    """A 1-pixel-wide index frame [L + SWEEP_TAIL, 1] whose first band (band_rows = L) has L indices: noise, flat or two-valued."""
    rng = np.random.default_rng(1000 * L + {"noise": 0, "flat": 1, "two": 2}[kind])
    h = L + SWEEP_TAIL
    if kind == "noise":                                           # noise in which no pair of neighbours comes twice: every index a miss, so
        idx, seen = [int(rng.integers(0, 256))], set()            # that the code width changes at L = 256, 768 and 1792 and the table
        for v in rng.integers(0, 256, h - 1):                     # is full at L = 3839, inside the sweep's ranges
            while (idx[-1], int(v)) in seen:
                v = (int(v) + 1) & 255
            seen.add((idx[-1], int(v)))
            idx.append(int(v))
        idx = np.array(idx)
    elif kind == "flat":
        idx = np.full(h, int(rng.integers(0, 256)))
    else:
        idx = rng.choice(rng.integers(0, 256, 2), h)
    return idx.astype(np.uint8).reshape(h, 1)


@functools.lru_cache(None)
def clips():
    rng = np.random.default_rng(27)

    def smooth(t, h, w):
        y, x, f = np.meshgrid(np.arange(h), np.arange(w), np.arange(t), indexing="ij")
        rgb = np.stack([128 + 100 * np.sin((x + 3 * f) / 17.0), 128 + 100 * np.cos((y - 2 * f) / 11.0), (2 * x + 3 * y + 5 * f) % 256], -1)
        return np.clip(np.rint(rgb), 0, 255).astype(np.uint8).transpose(2, 0, 1, 3).copy()

    def two(t, h, w):
        pick = rng.integers(0, 2, (t, h, w)).astype(bool)
        return np.where(pick[..., None], np.array([250, 10, 30], np.uint8), np.array([12, 200, 77], np.uint8)).astype(np.uint8)

    out = {"smooth_5x64x96": smooth(5, 64, 96), "noise_2x33x65": rng.integers(0, 256, (2, 33, 65, 3)).astype(np.uint8),
           "flat_3x17x23": np.full((3, 17, 23, 3), 93, np.uint8), "two_4x40x31": two(4, 40, 31),
           "noise_1x1x1": rng.integers(0, 256, (1, 1, 1, 3)).astype(np.uint8), "smooth_1x1x9": smooth(1, 1, 9), "two_2x9x1": two(2, 9, 1),
           "smooth_3x23x17": smooth(3, 23, 17)}
    for v in out.values():
        v.setflags(write=False)
    return out


def rows():
    """(clip name, band_rows) of every decode check: band_rows 0, 1, 3 and h."""
    return [(name, r) for name, clip in clips().items() for r in sorted({0, 1, 3, clip.shape[1]})]


@functools.lru_cache(None)
def clip_palette(name):
    return palette(clips()[name])


@functools.lru_cache(None)
def mirrored(name, band_rows):
    pal, table, used = clip_palette(name)
    idx = indices(clips()[name], table)
    stream, off = encode_indices(idx, band_rows)
    return {"stream": stream, "off": [int(v) for v in off], "pal": pal, "table": table, "used": used, "idx": idx}


def clip_of_bins(bins):
    """A clip [1, 1, N, 3] with `pop` pixels in each bin (r, g, b, pop) of a hand-made histogram, every pixel at the bin's lowest colour."""
    px = [[r << 3, g << 3, b << 3] for r, g, b, pop in bins for _ in range(pop)]
    return np.array(px, np.uint8).reshape(1, 1, -1, 3)


@functools.lru_cache(None)
def edge_frame(target):
    """A 1-pixel-wide noise index frame whose LZW data has exactly `target` bytes (the sub-block edges), found by a deterministic search."""
    for h in range(max(1, target * 8 // 11), target + 2):
        for seed in range(8):
            idx = np.random.default_rng(7000 + 10 * h + seed).integers(0, 256, (h, 1)).astype(np.uint8)
            if len(frame_data(idx, 0)) == target:
                return idx
    raise AssertionError(f"no frame with {target} bytes of data")


def colours_200():
    """A clip of 200 colours in 200 different bins, arranged at random: stored exactly."""
    rng = np.random.default_rng(200)
    bins = rng.choice(NBINS, 200, replace=False)
    colours = np.stack([(bins >> 10) << 3, ((bins >> 5) & 31) << 3, (bins & 31) << 3], 1) + rng.integers(0, 8, (200, 3))
    return colours.astype(np.uint8)[rng.integers(0, 200, (3, 24, 40))]

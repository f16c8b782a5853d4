"""Host mirror of the GIF output stage's changed-rectangle frames (ccvs_amd/csrc/gif.hip, include/ccvs_hip_output_gif_delta.h, DESIGN.md
section 4.29), in plain integer numpy and Python on top of tests/gif_ref.py, which it leaves as it is: the specification the kernels
are held to, byte for byte.

  median_cut_n(cnt, max_colours), palette_n(clip, max_colours)   `ccvs_gif_palette_n`: the median cut stops at max_colours boxes
  changed_rect(prev, cur)               (x0, y0, rw, rh) of the indices that differ; none: (0, 0, 1, 1)
  candidates(prev, cur, band_rows)      ((rect, payload) of F, (rect, payload) of D) -- D is None for a clip's first frame (prev None)
  encode_indices(idx, band_rows, t)     (stream, offsets, rects, full-frame sizes, rectangle sizes) of index frames [n, H, W], clips of t
  encode(clip, band_rows)               (stream, offsets, palette, table, used, rects) of a clip -- `ops.gif_encode(delta=True)`
  gif_file(payloads, rects, palette, fps, h, w)   the whole file -- what `tools.gif.write_gif(rects=...)` writes
"""
import functools
import struct

import numpy as np

import gif_ref as G

TRANSPARENT = 255
MAX_COLOURS = 255
NOTHING = bytes([0x08, 0x04, 0x00, 0xFF, 0x05, 0x04, 0x00])       # D of a frame that changes nothing: clear, 255, end of information at 9 bits


# ---------------------------------------------------------------- palette
def median_cut_n(cnt, max_colours):
    """`gif_ref.median_cut` stopping at max_colours boxes: (occupied bins ascending, their box numbers, number of boxes)."""
    assert 2 <= max_colours <= 256, max_colours
    cnt = np.asarray(cnt, np.int64)
    occ = np.nonzero(cnt)[0]
    if occ.size == 0:
        raise ValueError("median_cut_n: no pixels")
    xyz, pop = np.stack([occ >> 10, (occ >> 5) & 31, occ & 31], 1), cnt[occ]
    box = np.zeros(occ.size, np.int64)
    nbox = 1

    def rate(k):                                                 # (population x longest extent, the axis of that extent)
        m = box == k
        ext = xyz[m].max(0) - xyz[m].min(0)
        longest = int(ext.max())
        axis = 1 if ext[1] == longest else (0 if ext[0] == longest else 2)   # ties: G, then R, then B
        return int(pop[m].sum()) * longest, axis

    rated = [rate(0)]
    while nbox < max_colours:
        best, best_score = -1, 0
        for k in range(nbox):
            if rated[k][0] > best_score:                         # ties: the lowest box
                best, best_score = k, rated[k][0]
        if best < 0:
            break
        axis = rated[best][1]
        m = box == best
        c = xyz[m, axis]
        lo, hi, total = int(c.min()), int(c.max()), int(pop[m].sum())
        marg = np.zeros(32, np.int64)
        np.add.at(marg, c, pop[m])
        run, cut = 0, hi - 1
        for v in range(lo, hi):
            run += int(marg[v])
            if run >= (total + 1) // 2:
                cut = v
                break
        box[m & (xyz[:, axis] > cut)] = nbox
        rated[best] = rate(best)
        rated.append(rate(nbox))
        nbox += 1
    return occ, box, nbox


def palette_of_n(cnt, sums, max_colours):
    occ, box, used = median_cut_n(cnt, max_colours)
    mean = lambda s, n: (2 * s + n) // (2 * n)
    pal = np.zeros((256, 3), np.int64)
    for k in range(used):
        m = box == k
        n = int(cnt[occ[m]].sum())
        pal[k] = [mean(int(sums[occ[m], c].sum()), n) for c in range(3)]
    own = mean(sums[occ], cnt[occ][:, None])
    d = ((own[:, None, :] - pal[None, :used, :]) ** 2).sum(-1)
    table = np.zeros(G.NBINS, np.uint8)
    table[occ] = d.argmin(1).astype(np.uint8)                    # (argmin: the first of equals)
    return pal.astype(np.uint8), table, used


def palette_n(clip, max_colours=MAX_COLOURS):
    cnt, sums = G.histogram(clip)
    return palette_of_n(cnt, sums, max_colours)


# ---------------------------------------------------------------- frames
def changed_rect(prev, cur):
    changed = np.asarray(prev) != np.asarray(cur)
    if not changed.any():
        return (0, 0, 1, 1)
    ys, xs = np.nonzero(changed.any(1))[0], np.nonzero(changed.any(0))[0]
    return (int(xs[0]), int(ys[0]), int(xs[-1] - xs[0] + 1), int(ys[-1] - ys[0] + 1))


def candidates(prev, cur, band_rows=0):
    """((rect, payload) of the full frame, (rect, payload) of the changed rectangle or None where `prev` is None).  Either is cut into
    bands of band_rows rows of ITS rectangle (`gif_ref.frame_data` on the rectangle's own array does exactly that)."""
    cur = np.asarray(cur)
    h, w = cur.shape
    full = ((0, 0, w, h), G.payload(G.frame_data(cur, band_rows)))
    if prev is None:
        return full, None
    x0, y0, rw, rh = rect = changed_rect(prev, cur)
    sl = (slice(y0, y0 + rh), slice(x0, x0 + rw))
    part = np.where(np.asarray(prev)[sl] != cur[sl], cur[sl], TRANSPARENT).astype(np.uint8)
    return full, (rect, G.payload(G.frame_data(part, band_rows)))


def encode_indices(idx, band_rows=0, t=None):
    """Index frames [n, H, W] as clips of t frames (None: one clip): (stream, offsets int64 [n + 1], rects int32 [n, 4], the full
    frames' payload sizes, the rectangles' (None for a clip's first frame)).  The rectangle is written where it is strictly shorter."""
    idx = np.asarray(idx)
    n = len(idx)
    t = n if t is None else t
    parts, rects, fsize, dsize = [], [], [], []
    for f in range(n):
        full, part = candidates(idx[f - 1] if f % t else None, idx[f], band_rows)
        pick = part if part is not None and len(part[1]) < len(full[1]) else full
        parts.append(pick[1])
        rects.append(pick[0])
        fsize.append(len(full[1]))
        dsize.append(None if part is None else len(part[1]))
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return b"".join(parts), off, np.array(rects, np.int32).reshape(n, 4), fsize, dsize


def encode(clip, band_rows=0):
    clip = np.asarray(clip, np.uint8)
    pal, table, used = palette_n(clip)
    stream, off, rects, _, _ = encode_indices(G.indices(clip, table), band_rows)
    return stream, off, pal, table, used, rects


def gif_file(payloads, rects, pal, fps, h, w):
    out = bytearray(b"GIF89a")
    out += struct.pack("<HHBBB", w, h, 0xF7, 0, 0)
    out += np.asarray(pal, np.uint8).reshape(256, 3).tobytes()
    out += b"\x21\xFF\x0BNETSCAPE2.0\x03\x01\x00\x00\x00"
    for k, (p, r) in enumerate(zip(payloads, rects)):
        out += b"\x21\xF9\x04" + bytes([0x05 if k else 0x04]) + struct.pack("<HB", G.delay_cs(fps), TRANSPARENT) + b"\x00"
        out += b"\x2C" + struct.pack("<HHHHB", *(int(v) for v in r), 0)
        out += p
    out += b"\x3B"
    return bytes(out)


def clip_file(clip, fps, band_rows=0):
    """(the mirror's delta file of a uint8 clip [T, H, W, 3], palette[indices], rects)."""
    stream, off, pal, table, _, rects = encode(clip, band_rows)
    t, h, w = clip.shape[:3]
    return gif_file([stream[off[i]:off[i + 1]] for i in range(t)], rects, pal, fps, h, w), pal[G.indices(clip, table)], rects


# ---------------------------------------------------------------- the cases both test modules share (computed once)
# the hand-made histograms of the palette tests (tests/test_gif_host.py): bins (r, g, b, population)
HAND = ([(0, 2, 0, 1), (2, 0, 0, 1), (1, 1, 0, 2)], [(0, 0, 2, 1), (2, 0, 0, 1), (1, 0, 1, 2)], [(0, 0, 0, 1), (1, 0, 0, 1), (10, 0, 0, 1), (11, 0, 0, 1)],
        [(0, 0, 0, 1), (1, 0, 0, 1), (10, 0, 0, 1), (12, 0, 0, 1)], [(0, 0, 0, 2), (2, 0, 0, 2), (4, 0, 0, 4)], [(0, 0, 0, 2), (2, 0, 0, 1), (4, 0, 0, 4)],
        [(0, 5, 0, 1), (0, 9, 0, 10)], [(r, (3 * r) % 32, (7 * r) % 32, 1 + r % 3) for r in range(20)], [(31, 31, 31, 5)])


def direct_colours():
    """255 colours in 255 different bins and the table that maps colour i to index i < 255: frames of chosen INDICES for
    `ccvs_gif_encode_delta` (index 255 is the transparent one and stands for no colour)."""
    colours, table = G.direct_colours()
    table = table.copy()
    table[G.bins_of(colours[255:])] = 0
    return colours[:255], table


@functools.lru_cache(None)
def index_cases():
    """name -> (index frames [n, H, W] below 255, frames per clip): what both modules code and compare."""
    rng = np.random.default_rng(29)
    out = {}
    base = rng.integers(0, 255, (40, 56)).astype(np.uint8)
    out["identical_5x40x56"] = (np.stack([base] * 5), 5)

    def with_changes(shape, spots, n=None):
        frames = [rng.integers(0, 4, shape).astype(np.uint8)]
        for sl in spots:
            f = frames[-1].copy()
            f[sl] = (f[sl].astype(np.int64) + 1 + rng.integers(0, 200, f[sl].shape)) % 255   # every touched index changes (below 255)
            frames.append(f)
        return np.stack(frames)
    s = np.s_
    out["corners_5x24x40"] = (with_changes((24, 40), [s[0, 0], s[0, 39], s[23, 0], s[23, 39]]), 5)
    out["edges_5x24x40"] = (with_changes((24, 40), [s[0, :], s[23, :], s[:, 0], s[:, 39]]), 5)
    out["thin_3x24x40"] = (with_changes((24, 40), [s[3:20, 17], s[11, 5:33]]), 3)                 # 1 pixel wide, 1 pixel high
    out["all_changed_3x17x23"] = (with_changes((17, 23), [s[:, :], s[:, :]]), 3)                   # D = F in size: F is written
    # two-valued noise: about half the pixels keep their index, scattered; D's three symbols (0, 1, 255) cost more than F's two
    noise = rng.integers(0, 2, (3, 33, 65)).astype(np.uint8)
    out["noise_kept_3x33x65"] = (noise, 3)
    two = with_changes((20, 30), [s[4:9, 6:20], s[2:5, 1:4]])
    out["two_clips_6x20x30"] = (np.concatenate([two, two[::-1]]), 3)                               # clip 1 begins with clip 0's last frame
    tall = with_changes((160, 9), [s[5:155, 1:8]])                                                 # 7 x 150 = 1050 indices in one band: across
    out["chunk_2x160x9"] = (tall, 2)                                                               # the 1024-index chunk, 7 does not divide it
    wide = with_changes((64, 100), [s[:, 18:82]])                                                  # a band of 64 x 64 = 4096 > 4000
    out["big_band_2x64x100"] = (wide, 2)
    for v, _ in out.values():
        assert v.max() < 255
        v.setflags(write=False)
    return out


def index_rows():
    """(case, band_rows): 0 everywhere, and 1, 3, h on the small ones."""
    rows = []
    for name, (idx, _) in index_cases().items():
        h = idx.shape[1]
        rows += [(name, r) for r in (sorted({0, 1, 3, h}) if h <= 40 else [0])]
    return rows


@functools.lru_cache(None)
def mirrored_indices(name, band_rows):
    idx, t = index_cases()[name]
    stream, off, rects, fsize, dsize = encode_indices(idx, band_rows, t)
    return {"stream": stream, "off": [int(v) for v in off], "rects": rects, "fsize": fsize, "dsize": dsize, "idx": idx, "t": t}


@functools.lru_cache(None)
def mirrored(name, band_rows):
    """A clip of `gif_ref.clips()` in delta mode."""
    clip = G.clips()[name]
    stream, off, pal, table, used, rects = encode(clip, band_rows)
    return {"stream": stream, "off": [int(v) for v in off], "pal": pal, "table": table, "used": used, "rects": rects,
            "idx": G.indices(clip, table)}


def colours_255():
    """A clip of 255 colours in 255 different bins, a block of which moves: stored exactly, with changed rectangles."""
    rng = np.random.default_rng(255)
    bins = rng.choice(G.NBINS, 255, replace=False)
    colours = (np.stack([(bins >> 10) << 3, ((bins >> 5) & 31) << 3, (bins & 31) << 3], 1) + rng.integers(0, 8, (255, 3))).astype(np.uint8)
    idx = np.tile(rng.permutation(255 * 4)[:24 * 40].reshape(1, 24, 40) % 255, (3, 1, 1))
    idx[1, 5:12, 8:30] = rng.integers(0, 255, (7, 22))
    idx[2, 5:12, 8:30] = idx[1, 5:12, 8:30]
    idx[2, 20, 3] = (idx[2, 20, 3] + 1) % 255
    assert len(np.unique(idx)) == 255
    return colours[idx]


def many_bins_clip():
    """A clip with more than 300 occupied bins, static but for a moving patch: used == 255."""
    y, x = np.meshgrid(np.arange(32), np.arange(48), indexing="ij")
    back = np.stack([(5 * x) % 256, (7 * y) % 256, (3 * x + 11 * y) % 256], -1).astype(np.uint8)
    clip = np.stack([back] * 4)
    for f in range(1, 4):
        clip[f, 4 + 3 * f:12 + 3 * f, 6 + 5 * f:20 + 5 * f] = (200, 30 + 40 * f, 90)
    return clip


def prototype_clip(sigma=0.0, seed=1):
    """8 x 64 x 96: a smooth static background, a flat patch that moves, optional pixel noise."""
    y, x = np.meshgrid(np.arange(64), np.arange(96), indexing="ij")
    back = np.stack([128 + 100 * np.sin(x / 17.0), 128 + 100 * np.cos(y / 11.0), (2 * x + 3 * y) % 256], -1)
    clip = np.stack([back] * 8)
    for f in range(8):
        clip[f, 10 + 4 * f:26 + 4 * f, 8 + 9 * f:28 + 9 * f] = (230, 40, 60)
    if sigma:
        clip = clip + np.random.default_rng(seed).normal(0, sigma, clip.shape)
    return np.clip(np.rint(clip), 0, 255).astype(np.uint8)

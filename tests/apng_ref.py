"""Pure-Python / numpy statement of the lossless output stage (include/ccvs_hip_output_lossless.h): what
`ccvs_apng_encode` writes, byte for byte, and the table of images the host and GPU tests share.

  filter_rows     PNG's five filters with bpp = 3; `filter = -1`: per row the type with the smallest sum of |signed byte|, ties low
  band_cut        a frame's bands of `band_rows` rows (0: as many rows as hold at most 32768 filtered bytes, at least one)
  code_lengths    a complete length-limited Huffman code from counts (the tree, T.81 K.2 down to the limit, lengths by count)
  canonical       RFC 1951 3.2.2 codes
  run_lengths     zlib's send_tree on the 259 code lengths as one sequence
  block_header    BFINAL, BTYPE = 2, HLIT = 0, HDIST = 1, HCLEN, the code-length code, the coded lengths -- as (value, bits) pairs
  encode_frame    the zlib stream of one frame: 78 01, a dynamic block per band, an empty stored block between bands, Adler-32
  encode          several frames: (bytes, offsets)
"""
import heapq

import numpy as np

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
DEFAULT_BAND_BYTES = 32768
ADLER = 65521
FILTERS = (-1, 0, 1, 2, 3, 4)


# ------------------------------------------------------------------ filters
def filter_candidates(img):
    """The five filtered forms of a frame: uint8 [5, h, 3 w]."""
    h, w = img.shape[:2]
    x = img.reshape(h, 3 * w).astype(np.int32)
    a = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, 3:] = x[:-1, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return (np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255).astype(np.uint8)


def filter_rows(img, filter=-1):
    """(filtered rows uint8 [h, 3 w + 1], the rows' types)."""
    cand = filter_candidates(img)
    h = img.shape[0]
    if filter == -1:
        v = cand.astype(np.int64)
        score = np.where(v < 128, v, 256 - v).sum(axis=2)              # [5, h]
        types = score.argmin(axis=0)                                    # the first minimum: ties go to the lowest type
    else:
        assert 0 <= filter <= 4
        types = np.full(h, filter, np.int64)
    rows = cand[types, np.arange(h)]
    return np.concatenate([types[:, None].astype(np.uint8), rows], axis=1), types


def default_band_rows(w):
    return max(1, DEFAULT_BAND_BYTES // (3 * w + 1))


def band_cut(h, w, band_rows=0):
    r = band_rows if band_rows > 0 else default_band_rows(w)
    return [(r0, min(h, r0 + r)) for r0 in range(0, h, r)]


# ------------------------------------------------------------------ tables
def code_lengths(counts, maxlen):
    """Lengths of a complete code of at most `maxlen` bits over the symbols with a count; where fewer than two have one, the lowest
    symbols without are counted once.  The two smallest nonzero counts are merged, among equal counts the larger symbol first, the
    sum staying with the first of the two, until one is left; depths beyond maxlen come down by the T.81 K.2 move (two codes of the
    longest length go: one takes the prefix of the pair, the other becomes the brother of a shorter code that grows by a bit), which
    keeps the Kraft sum at 1; the lengths, ascending, go to the symbols by descending count, then ascending symbol."""
    cnt = [int(c) for c in counts]
    n = len(cnt)
    used = sum(c > 0 for c in cnt)
    for i in range(n):
        if used >= 2:
            break
        if cnt[i] == 0:
            cnt[i] = 1
            used += 1
    parent = {}
    heap = [(c, -i, i) for i, c in enumerate(cnt) if c]                # the node of a merged pair keeps the first symbol's place in the order
    heapq.heapify(heap)
    node = {i: i for i in range(n)}                                     # symbol -> its current tree node
    fresh = n
    while len(heap) > 1:
        f0, k0, s0 = heapq.heappop(heap)
        f1, _, s1 = heapq.heappop(heap)
        parent[node[s0]] = parent[node[s1]] = fresh
        node[s0] = fresh
        fresh += 1
        heapq.heappush(heap, (f0 + f1, k0, s0))
    bits = [0] * (max(n, maxlen) + 2)
    for i in range(n):
        if cnt[i]:
            d, k = 0, i
            while k in parent:
                k = parent[k]
                d += 1
            bits[d] += 1
    for i in range(len(bits) - 1, maxlen, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    order = sorted((i for i in range(n) if cnt[i]), key=lambda i: (-cnt[i], i))
    ladder = [l for l in range(1, maxlen + 1) for _ in range(bits[l])]
    assert len(ladder) == len(order)
    lengths = [0] * n
    for i, l in zip(order, ladder):
        lengths[i] = l
    return lengths


def canonical(lengths):
    """RFC 1951 3.2.2: the codes (MSB-first values) of the lengths; 0 where a symbol has none."""
    maxlen = max(lengths)
    count = [0] * (maxlen + 1)
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * (maxlen + 1), 0
    for l in range(1, maxlen + 1):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    codes = [0] * len(lengths)
    for i, l in enumerate(lengths):
        if l:
            codes[i] = nxt[l]
            nxt[l] += 1
    return codes


def reverse_bits(v, n):
    return int(format(v, f"0{n}b")[::-1], 2) if n else 0


def run_lengths(seq):
    """zlib's send_tree: [(code-length symbol, extra value, extra bits)].  A run of a nonzero length is the length, then 16 (3 .. 6
    more); zeros are 17 (3 .. 10) or 18 (11 .. 138); shorter runs as they are."""
    out, prev, nxt, count = [], -1, seq[0], 0
    maxc, minc = (138, 3) if nxt == 0 else (7, 4)
    for k in range(len(seq)):
        cur, nxt = nxt, (seq[k + 1] if k + 1 < len(seq) else -1)
        count += 1
        if count < maxc and cur == nxt:
            continue
        if count < minc:
            out += [(cur, 0, 0)] * count
        elif cur != 0:
            if cur != prev:
                out.append((cur, 0, 0))
                count -= 1
            out.append((16, count - 3, 2))
        elif count <= 10:
            out.append((17, count - 3, 3))
        else:
            out.append((18, count - 11, 7))
        count, prev = 0, cur
        maxc, minc = (138, 3) if nxt == 0 else ((6, 3) if cur == nxt else (7, 4))
    return out


def block_header(lit_lengths, final):
    """The dynamic block's header up to its first literal, as (value, bits) pairs in stream order (values LSB-first, Huffman codes
    already reversed)."""
    assert len(lit_lengths) == 257
    runs = run_lengths(list(lit_lengths) + [1, 1])                      # two distance codes of length 1: a complete code nobody uses
    cl_counts = [0] * 19
    for s, _, _ in runs:
        cl_counts[s] += 1
    cl_len = code_lengths(cl_counts, 7)
    cl_code = canonical(cl_len)
    ncl = 19
    while ncl > 4 and cl_len[CL_ORDER[ncl - 1]] == 0:
        ncl -= 1
    out = [(1 if final else 0, 1), (2, 2), (0, 5), (1, 5), (ncl - 4, 4)]
    out += [(cl_len[CL_ORDER[i]], 3) for i in range(ncl)]
    for s, extra, nbits in runs:
        out.append((reverse_bits(cl_code[s], cl_len[s]), cl_len[s]))
        if s >= 16:
            out.append((extra, nbits))
    return out


def _bits_of(pairs):
    """(value, bits) pairs -> the bit list, LSB of every value first."""
    return np.array([(v >> k) & 1 for v, n in pairs for k in range(n)], np.uint8)


def band_block(data, final):
    """One band's filtered bytes -> (the dynamic block's bits as uint8 0 / 1, the literal/length code lengths)."""
    counts = np.bincount(data, minlength=257)
    counts[256] = 1
    lengths = code_lengths(counts, 15)
    codes = canonical(lengths)
    rev = np.array([reverse_bits(c, l) for c, l in zip(codes, lengths)], np.uint32)
    ln = np.array(lengths, np.int64)
    sym = np.concatenate([data.astype(np.int64), [256]])
    k = np.arange(15)
    grid = ((rev[sym][:, None] >> k) & 1).astype(np.uint8)             # [symbols, 15]: bit k of every code
    body = grid[k[None, :] < ln[sym][:, None]]                          # row-major: every code's bits in order
    return np.concatenate([_bits_of(block_header(lengths, final)), body]), lengths


def adler_parts(data):
    """(sum of the bytes, sum of (len - i) x byte i) mod 65521: what a band contributes."""
    d = data.astype(np.int64)
    n = len(d)
    return int(d.sum() % ADLER), int(((n - np.arange(n)) % ADLER * d).sum() % ADLER)


def encode_frame(img, filter=-1, band_rows=0):
    """dict(stream=the frame's zlib stream, filtered=the filtered bytes, types=the rows' filter types, bands=the band count)."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    assert img.shape == (h, w, 3)
    rows, types = filter_rows(img, filter)
    bands = band_cut(h, w, band_rows)
    out = bytearray(b"\x78\x01")
    A, B = 1, 0
    for i, (r0, r1) in enumerate(bands):
        data = rows[r0:r1].reshape(-1)
        final = i == len(bands) - 1
        bits, _ = band_block(data, final)
        if not final:
            bits = np.concatenate([bits, np.zeros(3, np.uint8)])        # the empty stored block's BFINAL = 0, BTYPE = 00
        out += np.packbits(bits, bitorder="little").tobytes()           # (pads with zero bits to a byte)
        if not final:
            out += b"\x00\x00\xff\xff"
        sa, sb = adler_parts(data)
        B = (B + len(data) % ADLER * A + sb) % ADLER
        A = (A + sa) % ADLER
    out += ((B << 16) | A).to_bytes(4, "big")
    return dict(stream=bytes(out), filtered=rows.tobytes(), types=types, bands=len(bands))


def encode(frames, filter=-1, band_rows=0):
    """(the frames' streams one after the other, the n + 1 offsets)."""
    streams = [encode_frame(f, filter, band_rows)["stream"] for f in frames]
    return b"".join(streams), [0] + list(np.cumsum([len(s) for s in streams]))


def band_overhead_bytes():
    """An upper bound of what a band costs beyond its bytes' own codes: the header (at most 3700 bits), end-of-block (at most 15),
    the stored block's 3 bits, the padding (at most 7), and 00 00 FF FF."""
    return (3700 + 15 + 3 + 7) // 8 + 4


# ------------------------------------------------------------------ the image table
def _contents(h, w, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = lambda v: np.stack([v, v + 40, 255 - v], -1) % 256
    smooth = 128 + 60 * np.sin(xx / 9.0 + 0.3) + 50 * np.cos(yy / 7.0) + 0.2 * xx
    smooth = np.stack([smooth, smooth * 0.8 + 20, 255 - smooth], -1) + rng.integers(-2, 3, (h, w, 3))
    # rows that each favour another filter: noise (None), a noisy row repeated with a step per pixel (Sub), the row above again
    # (Up), the mean of left and above plus little (Average), Paeth's own prediction plus or minus one (Paeth)
    mixed = np.zeros((h, w, 3), np.int64)
    for y in range(h):
        k = y % 5
        if k == 0 or y == 0:
            mixed[y] = rng.integers(0, 256, (w, 3))
        elif k == 1:
            mixed[y] = (np.cumsum(rng.integers(0, 2, (w, 3)), 0) * 3 + rng.integers(0, 256, (1, 3))) % 256
        elif k == 2:
            mixed[y] = mixed[y - 1]
        elif k == 3:
            for x in range(w):
                left = mixed[y, x - 1] if x else 0
                mixed[y, x] = ((left + mixed[y - 1, x]) >> 1) % 256
        else:
            for x in range(w):
                a = mixed[y, x - 1] if x else np.zeros(3, np.int64)
                b = mixed[y - 1, x]
                c = mixed[y - 1, x - 1] if x else np.zeros(3, np.int64)
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                mixed[y, x] = (np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c)) + rng.integers(-1, 2, 3)) % 256
    return {
        "zeros": np.zeros((h, w, 3)), "ones": np.full((h, w, 3), 255),
        "hramp": ramp(xx * 3), "vramp": ramp(yy * 5), "dramp": ramp(xx * 2 + yy * 3),
        "noise": rng.integers(0, 256, (h, w, 3)), "smooth": smooth, "mixed": mixed,
    }


SIZES = ((1, 1), (1, 7), (7, 1), (2, 2), (8, 8), (17, 23), (33, 65), (64, 64))
_IMAGES = None


def images():
    """{name: uint8 [h, w, 3]}: every content at every small size, and the smooth-plus-noise and noise frames at 256 x 256."""
    global _IMAGES
    if _IMAGES is None:
        rng = np.random.default_rng(20)
        out = {}
        for h, w in SIZES:
            for name, v in _contents(h, w, rng).items():
                out[f"{name}_{h}x{w}"] = np.clip(v, 0, 255).astype(np.uint8)
        big = _contents(256, 256, rng)
        out["smooth_256x256"] = np.clip(big["smooth"], 0, 255).astype(np.uint8)
        _IMAGES = out
    return _IMAGES


def deep_row():
    """One row of 43690 pixels whose bytes 0 .. 16 come 1, 2, 4, ... 32768, 65535 times, shuffled: with `filter = 0` the band's tree is a
    chain 17 deep (every merged pair is smaller than the next count but one), so the limiter has to run."""
    counts = [1 << k for k in range(16)] + [65535]
    data = np.random.default_rng(3).permutation(np.repeat(np.arange(17, dtype=np.uint8), counts))
    return data.reshape(1, -1, 3)


def band_choices(h):
    """band_rows of the table for a frame of h rows: 1, 2, h - 1, h and 0 (the default), where they differ."""
    out = []
    for r in (1, 2, h - 1, h, 0):
        if (r == 0 or 1 <= r <= h) and r not in out:
            out.append(r)
    return out


def rows():
    """[(key, image name, filter, band_rows)]: the table.  The 256 x 256 frame leaves out band_rows = 1 and 2 for all filters but the
    adaptive one (hundreds of bands each, which the 64 x 64 frames cover)."""
    out = []
    for name, img in images().items():
        h = img.shape[0]
        for flt in FILTERS:
            for r in band_choices(h):
                if h == 256 and r in (1, 2) and flt != -1:
                    continue
                out.append((f"{name}/f{flt}/b{r}", name, flt, r))
    return out


_MIRROR = {}


def mirrored(key):
    """`encode_frame` of a row of the table, computed once per process."""
    if key not in _MIRROR:
        name, flt, r = key.split("/")
        _MIRROR[key] = encode_frame(images()[name], int(flt[1:]), int(r[1:]))
    return _MIRROR[key]

"""Pure-Python / numpy statement of the lossless output stage WITH LZ77 matches (include/ccvs_hip_output_lossless_lz.h, DESIGN.md section
4.24): what `ccvs_apng_encode_lz` writes, byte for byte, and the table of rows the host and GPU tests share.  Filters, bands, the
Huffman builder, the run-length coding of the code lengths, the zlib framing and the images are those of tests/apng_ref.py.

  window        at a position: the same frame's filtered bytes before it (earlier bands of the frame included); distance 1 .. 32768
  length        3 .. 258, never past the end of the position's own band; overlapping copies (distance < length) are allowed
  candidates    distance 1, distance 3 (the pixel to the left), distance 3 w + 1 (the byte above), and the nearest earlier position of
                the SAME band whose three bytes hash alike (13 bits; positions whose three bytes do not fit into the band have no hash),
                if it is at most 32768 back.  The longest match wins, ties go to the smallest distance; a match of length 3 at a
                distance beyond 4096 is dropped.
  parse         greedy from the band's first byte: a match of 3 or more at the position is taken whole, else one literal
  coding        RFC 1951: 286 literal/length and 30 distance symbols, both codes from `apng_ref.code_lengths` at 15 bits, HLIT and HDIST
                trimmed, the two length lists run-length coded as ONE sequence by `apng_ref.run_lengths`, extra bits behind their symbols
  choice        per band the match block or the literal-only block of `apng_ref.band_block`, whichever has fewer bits; ties: literal-only
"""
import numpy as np

import apng_ref as R

WINDOW = 32768
MIN_LEN, MAX_LEN = 3, 258
FAR3 = 4096                      # a length-3 match further back than this is dropped (zlib's TOO_FAR)
HASH_BITS = 13
HASH_MUL = 0x9E3779B1

# RFC 1951 3.2.5
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)

_LEN_SYM = np.zeros(MAX_LEN + 1, np.int64)
for _s, _b in enumerate(LEN_BASE):
    _LEN_SYM[_b:] = _s
_LEN_BASE, _LEN_EXTRA = np.array(LEN_BASE, np.int64), np.array(LEN_EXTRA, np.int64)
_DIST_BASE, _DIST_EXTRA = np.array(DIST_BASE, np.int64), np.array(DIST_EXTRA, np.int64)


def hash3(b0, b1, b2):
    v = b0.astype(np.uint64) | (b1.astype(np.uint64) << np.uint64(8)) | (b2.astype(np.uint64) << np.uint64(16))
    return (((v * np.uint64(HASH_MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - HASH_BITS)).astype(np.int64)


# ------------------------------------------------------------------ matches
def _fixed_lengths(f, d, limit):
    """Match length of every position against the position d before it, at most limit[p]; 0 where that lies before the frame."""
    n = len(f)
    out = np.zeros(n, np.int64)
    if d < 1 or d > WINDOW or d >= n:
        return out
    ne = np.flatnonzero(np.concatenate([f[d:] != f[:-d], [True]])) + d          # the first position at or behind p that differs
    p = np.arange(d, n)
    out[d:] = np.minimum(ne[np.searchsorted(ne, p)] - p, limit[d:])
    return out


def _lengths(f, p, q, limit):
    """Match length of positions p against positions q < p, at most limit (one per p)."""
    n = np.zeros(len(p), np.int64)
    act = np.flatnonzero(limit > 0)
    while act.size:
        eq = f[p[act] + n[act]] == f[q[act] + n[act]]
        act = act[eq]
        n[act] += 1
        act = act[n[act] < limit[act]]
    return n


def candidates(f, spans, rowb):
    """f: one frame's filtered bytes; spans: [(start, end)] of its bands; rowb: the bytes of a filtered row.  ([(lengths, distances)]
    per candidate, the positions' length limits)."""
    n = len(f)
    end = np.zeros(n, np.int64)
    band = np.zeros(n, np.int64)
    for i, (s, e) in enumerate(spans):
        end[s:e], band[s:e] = e, i
    pos = np.arange(n)
    limit = np.minimum(MAX_LEN, end - pos)
    out = [(_fixed_lengths(f, d, limit), np.full(n, d, np.int64)) for d in (1, 3, rowb)]
    # the nearest earlier position of the same band with the same hash: a stable sort by (band, hash) puts it right in front
    hl = np.zeros(n, np.int64)
    hd = np.zeros(n, np.int64)
    ok = np.flatnonzero(pos + 2 < end)
    if ok.size:
        key = (band[ok] << HASH_BITS) | hash3(f[ok], f[ok + 1], f[ok + 2])
        order = np.argsort(key, kind="stable")
        sp, sk = ok[order], key[order]
        same = np.flatnonzero(sk[1:] == sk[:-1]) + 1
        p, q = sp[same], sp[same - 1]
        near = p - q <= WINDOW
        p, q = p[near], q[near]
        hl[p] = _lengths(f, p, q, limit[p])
        hd[p] = p - q
    out.append((hl, hd))
    return out, limit


def best_matches(f, spans, rowb):
    """(length, distance) of the best match at every position of the frame, length 0 where there is none."""
    cands, _ = candidates(f, spans, rowb)
    best_l = np.zeros(len(f), np.int64)
    best_d = np.zeros(len(f), np.int64)
    for l, d in cands:
        l = np.where((l < MIN_LEN) | ((l == MIN_LEN) & (d > FAR3)), 0, l)
        better = (l > best_l) | ((l == best_l) & (l > 0) & (d < best_d))
        best_l = np.where(better, l, best_l)
        best_d = np.where(better, d, best_d)
    return best_l, best_d


def parse(best_l, start, end):
    """Greedy: the band's token starts [(position, length)], length 0 for a literal."""
    out, p = [], start
    ls = best_l[start:end].tolist()
    while p < end:
        l = ls[p - start]
        out.append((p, l))
        p += l if l else 1
    return out


# ------------------------------------------------------------------ the match block
def _expand(values, nbits):
    """(value, bits) columns in stream order -> the bit list, LSB of every value first."""
    v, nb = np.asarray(values, np.int64).ravel(), np.asarray(nbits, np.int64).ravel()
    total = int(nb.sum())
    idx = np.repeat(np.arange(len(v)), nb)
    k = np.arange(total) - np.repeat(np.cumsum(nb) - nb, nb)
    return ((v[idx] >> k) & 1).astype(np.uint8)


def lz_header(ll_len, d_len, final):
    """The dynamic block's header with both codes, HLIT and HDIST trimmed, as (value, bits) pairs."""
    hlit = max(257, max(i + 1 for i, l in enumerate(ll_len) if l))
    hdist = max(1, max(i + 1 for i, l in enumerate(d_len) if l))
    runs = R.run_lengths(list(ll_len[:hlit]) + list(d_len[:hdist]))
    cl_counts = [0] * 19
    for s, _, _ in runs:
        cl_counts[s] += 1
    cl_len = R.code_lengths(cl_counts, 7)
    cl_code = R.canonical(cl_len)
    ncl = 19
    while ncl > 4 and cl_len[R.CL_ORDER[ncl - 1]] == 0:
        ncl -= 1
    out = [(1 if final else 0, 1), (2, 2), (hlit - 257, 5), (hdist - 1, 5), (ncl - 4, 4)]
    out += [(cl_len[R.CL_ORDER[i]], 3) for i in range(ncl)]
    for s, extra, nbits in runs:
        out.append((R.reverse_bits(cl_code[s], cl_len[s]), cl_len[s]))
        if s >= 16:
            out.append((extra, nbits))
    return out


def lz_block(f, tokens, final):
    """One band's tokens [(position, length)] with the distances in `tokens` third column -> the match block's bits."""
    pos = np.array([t[0] for t in tokens], np.int64)
    ln = np.array([t[1] for t in tokens], np.int64)
    ds = np.array([t[2] for t in tokens], np.int64)
    m = ln > 0
    lsym = np.where(m, 257 + _LEN_SYM[ln], f[pos].astype(np.int64))
    dsym = np.searchsorted(_DIST_BASE, np.where(m, ds, 1), side="right") - 1
    ll_counts = np.bincount(lsym, minlength=286)
    ll_counts[256] = 1
    d_counts = np.bincount(dsym[m], minlength=30)
    ll_len, d_len = R.code_lengths(ll_counts, 15), R.code_lengths(d_counts, 15)
    ll_rev = np.array([R.reverse_bits(c, l) for c, l in zip(R.canonical(ll_len), ll_len)], np.int64)
    d_rev = np.array([R.reverse_bits(c, l) for c, l in zip(R.canonical(d_len), d_len)], np.int64)
    ll_n, d_n = np.array(ll_len, np.int64), np.array(d_len, np.int64)
    li = np.where(m, _LEN_SYM[ln], 0)
    values = np.stack([ll_rev[lsym], np.where(m, ln - _LEN_BASE[li], 0), np.where(m, d_rev[dsym], 0), np.where(m, ds - _DIST_BASE[dsym], 0)], 1)
    nbits = np.stack([ll_n[lsym], np.where(m, _LEN_EXTRA[li], 0), np.where(m, d_n[dsym], 0), np.where(m, _DIST_EXTRA[dsym], 0)], 1)
    assert (nbits[:, 0] > 0).all() and (nbits[m, 2] > 0).all() and nbits.sum(1).max() <= 48
    eob = R._bits_of([(int(ll_rev[256]), int(ll_n[256]))])
    return np.concatenate([R._bits_of(lz_header(ll_len, d_len, final)), _expand(values, nbits), eob])


def replay(tokens, literals):
    """The bytes a band's tokens make behind `literals` (the frame's bytes before the band)."""
    out = bytearray(literals)
    for t in tokens:
        if isinstance(t, tuple):
            l, d = t
            for _ in range(l):
                out.append(out[-d])
        else:
            out.append(t)
    return bytes(out[len(literals):])


def encode_frame(img, filter=-1, band_rows=0):
    """dict(stream, filtered, types, bands, tokens=[per band: a literal as its byte, a match as (length, distance)],
    choice=[per band: "lz" or "literal"])."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    assert img.shape == (h, w, 3)
    rows, types = R.filter_rows(img, filter)
    rowb = 3 * w + 1
    f = rows.reshape(-1)
    bands = R.band_cut(h, w, band_rows)
    spans = [(r0 * rowb, r1 * rowb) for r0, r1 in bands]
    best_l, best_d = best_matches(f, spans, rowb)
    out = bytearray(b"\x78\x01")
    A, B = 1, 0
    tokens, choice = [], []
    for i, (s, e) in enumerate(spans):
        data = f[s:e]
        final = i == len(spans) - 1
        toks = [(p, l, int(best_d[p]) if l else 0) for p, l in parse(best_l, s, e)]
        tokens.append([(l, d) if l else int(f[p]) for p, l, d in toks])
        plain, _ = R.band_block(data, final)
        bits = plain
        choice.append("literal")
        if any(l for _, l, _ in toks):
            lz = lz_block(f, toks, final)
            if len(lz) < len(plain):
                bits, choice[-1] = lz, "lz"
        if not final:
            bits = np.concatenate([bits, np.zeros(3, np.uint8)])
        out += np.packbits(bits, bitorder="little").tobytes()
        if not final:
            out += b"\x00\x00\xff\xff"
        sa, sb = R.adler_parts(data)
        B = (B + len(data) % R.ADLER * A + sb) % R.ADLER
        A = (A + sa) % R.ADLER
    out += ((B << 16) | A).to_bytes(4, "big")
    return dict(stream=bytes(out), filtered=rows.tobytes(), types=types, bands=len(bands), tokens=tokens, choice=choice)


def encode(frames, filter=-1, band_rows=0):
    streams = [encode_frame(f, filter, band_rows)["stream"] for f in frames]
    return b"".join(streams), [0] + list(np.cumsum([len(s) for s in streams]))


# ------------------------------------------------------------------ the table
TABLE_SIZES = ((1, 1), (2, 2), (17, 23), (33, 65), (64, 64))
TABLE_FILTERS = (-1, 0, 4)
_IMAGES = None


def _row_image(data):
    """One row of pixels whose filtered bytes under filter 0 are the type byte 0 and `data` (a multiple of 3 long)."""
    assert len(data) % 3 == 0
    return np.asarray(data, np.uint8).reshape(1, -1, 3)


def _noise_without_repeats(rng, period):
    """`period` noise bytes, the first one 0, in which (read cyclically) no three consecutive bytes come twice: repeated with that
    period they match only at multiples of it."""
    b = rng.integers(0, 256, period).astype(np.uint8)
    b[0] = 0
    while True:
        c = np.concatenate([b, b[:2]]).astype(np.int64)
        _, first = np.unique(c[:-2] | (c[1:-1] << 8) | (c[2:] << 16), return_index=True)
        dup = np.setdiff1d(np.arange(period), first)
        if not dup.size:
            return b
        at = np.where((dup + 1) % period == 0, dup + 2, dup + 1) % period
        b[at] = rng.integers(0, 256, len(at))


def images():
    """`apng_ref.images()`, a 256 x 256 noise frame, and the constructed frames."""
    global _IMAGES
    if _IMAGES is None:
        out = dict(R.images())
        rng = np.random.default_rng(24)
        out["noise_256x256"] = rng.integers(0, 256, (256, 256, 3)).astype(np.uint8)
        for period in (32768, 32769):
            filtered = np.resize(_noise_without_repeats(rng, period), 3 * 21846 + 1)    # (its first byte, 0, is the row's type byte)
            out[f"period_{period}"] = _row_image(filtered[1:])
        run = np.concatenate([rng.integers(1, 256, 100), np.full(1 + 258 + 258, 77), rng.integers(1, 256, 103)])
        run[99], run[100 + 517] = 1, 2                                  # the run is exactly 517 long
        out["run_517"] = _row_image(run)
        two = rng.integers(0, 256, (2, 40, 3)).astype(np.uint8)
        two[0, 30:] = 0                                                 # 30 flat bytes up to the first band's end, the type byte 0 and
        two[1, :20] = 0                                                 # 60 more behind it
        out["run_to_band_end"] = two
        _IMAGES = out
    return _IMAGES


def rows():
    """[(key, image name, filter, band_rows)]."""
    out = []
    for h, w in TABLE_SIZES:
        for name in ("zeros", "ones", "hramp", "vramp", "dramp", "noise", "smooth", "mixed"):
            for flt in TABLE_FILTERS:
                for r in dict.fromkeys((1, h, 0)):
                    out.append((f"{name}_{h}x{w}/f{flt}/b{r}", f"{name}_{h}x{w}", flt, r))
    out += [(f"{name}/f-1/b0", name, -1, 0) for name in ("smooth_256x256", "noise_256x256")]
    out += [(f"{name}/f0/b1", name, 0, 1) for name in ("period_32768", "period_32769", "run_517", "run_to_band_end")]
    return out


_MIRROR = {}


def mirrored(key):
    """`encode_frame` of a row of the table, computed once per process."""
    if key not in _MIRROR:
        name, flt, r = key.split("/")
        _MIRROR[key] = encode_frame(images()[name], int(flt[1:]), int(r[1:]))
    return _MIRROR[key]

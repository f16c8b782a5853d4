"""Spec mirror of the inflate of the PNG decoder (ccvs_amd/csrc/png_decode_core.h): RFC 1950 / 1951 in plain
Python with the kernel's status words, zlib's acceptance rules and the order of checks of the core, plus per-stream token statistics
(block types, length and distance codes used, overlapping copies, the largest distance).  Also the streams the tests share: the
table of plain streams, the planted buffer, the hand-assembled streams and the mutations.  Nothing here loads the library."""
import functools
import zlib

import numpy as np

import apng_ref as R

OK, BAD_STREAM, BAD_HEADER, BAD_BLOCK, BAD_TABLE, BAD_CODE, BAD_DISTANCE, OVERRUN, TOO_LONG, TOO_SHORT, BAD_CHECK, BAD_FILTER = range(12)
NAMES = ("OK", "BAD_STREAM", "BAD_HEADER", "BAD_BLOCK", "BAD_TABLE", "BAD_CODE", "BAD_DISTANCE", "OVERRUN", "TOO_LONG", "TOO_SHORT", "BAD_CHECK", "BAD_FILTER")
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CODES, LENS, DISTS = 0, 1, 2


class _Stop(Exception):
    def __init__(self, status):
        self.status = status


def build(lens, kind):
    """zlib's acceptance rules (inftrees.c).  Returns a lookup over the next 15 bits (LSB first) -> (length, symbol) or None; an empty
    set gives a lookup of Nones."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    look = [None] * 32768
    if count[0] == len(lens):
        return look
    left = 1
    for l in range(1, 16):
        left = (left << 1) - count[l]
        if left < 0:
            raise _Stop(BAD_TABLE)
    longest = max(l for l in range(16) if count[l])
    if left > 0 and (kind == CODES or longest != 1):
        raise _Stop(BAD_TABLE)
    code, nxt = 0, [0] * 16
    for l in range(1, 16):
        code = (code + count[l - 1] * (l > 1)) << 1
        nxt[l] = code
    for s, l in enumerate(lens):
        if l:
            rev = R.reverse_bits(nxt[l], l)
            nxt[l] += 1
            look[rev::1 << l] = [(l, s)] * (32768 >> l)
    return look


class _Bits:
    def __init__(self, data, pos):
        self.d, self.pos, self.acc, self.n = data, pos, 0, 0

    def fill(self):
        while self.n <= 56 and self.pos < len(self.d):
            self.acc |= self.d[self.pos] << self.n
            self.pos += 1
            self.n += 8

    def bits(self, k):
        if self.n < k:
            raise _Stop(OVERRUN)
        v = self.acc & ((1 << k) - 1)
        self.acc >>= k
        self.n -= k
        return v

    def symbol(self, look):
        e = look[self.acc & 32767]
        if e is None:
            raise _Stop(BAD_CODE if self.n >= 15 else OVERRUN)
        if e[0] > self.n:
            raise _Stop(OVERRUN)
        self.acc >>= e[0]
        self.n -= e[0]
        return e[1]


@functools.lru_cache(None)
def _fixed():
    return build([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, LENS), build([5] * 32, DISTS)


def _dynamic(b):
    b.fill()
    v = b.bits(14)
    hlit, hdist, hclen = (v & 31) + 257, ((v >> 5) & 31) + 1, (v >> 10) + 4
    if hlit > 286 or hdist > 30:
        raise _Stop(BAD_TABLE)
    cl = [0] * 19
    for i in range(hclen):
        b.fill()
        cl[R.CL_ORDER[i]] = b.bits(3)
    look = build(cl, CODES)
    if not any(cl):
        raise _Stop(BAD_TABLE)
    lens = []
    while len(lens) < hlit + hdist:
        b.fill()
        s = b.symbol(look)
        if s < 16:
            lens.append(s)
            continue
        prev = 0
        if s == 16:
            if not lens:
                raise _Stop(BAD_TABLE)
            prev, rep = lens[-1], 3 + b.bits(2)
        elif s == 17:
            rep = 3 + b.bits(3)
        else:
            rep = 11 + b.bits(7)
        if len(lens) + rep > hlit + hdist:
            raise _Stop(BAD_TABLE)
        lens += [prev] * rep
    if lens[256] == 0:
        raise _Stop(BAD_TABLE)
    return build(lens[:hlit], LENS), build(lens[hlit:], DISTS)


def new_stats():
    return {"blocks": [0, 0, 0], "length_codes": set(), "distance_codes": set(), "overlapping": 0, "largest_distance": 0, "longest": 0, "matches": 0}


def inflate(data, expect, stats=None):
    """(status, the bytes produced so far): one zlib stream that is to hold exactly `expect` bytes."""
    data = bytes(data)
    st = stats if stats is not None else new_stats()
    out = bytearray()
    try:
        if len(data) < 2:
            raise _Stop(OVERRUN)
        cmf, flg = data[0], data[1]
        if (cmf & 15) != 8 or (cmf >> 4) > 7 or ((cmf << 8) | flg) % 31 or flg & 32:
            raise _Stop(BAD_HEADER)
        b = _Bits(data, 2)
        final = 0
        while not final:
            b.fill()
            v = b.bits(3)
            final, kind = v & 1, v >> 1
            if kind == 3:
                raise _Stop(BAD_BLOCK)
            st["blocks"][kind] += 1
            if kind == 0:
                b.bits(b.n & 7)
                b.fill()
                n, nn = b.bits(16), b.bits(16)
                if n ^ nn != 0xFFFF:
                    raise _Stop(BAD_BLOCK)
                b.pos -= b.n >> 3
                b.n = b.acc = 0
                if n > len(data) - b.pos:
                    raise _Stop(OVERRUN)
                if n > expect - len(out):
                    raise _Stop(TOO_LONG)
                out += data[b.pos:b.pos + n]
                b.pos += n
                continue
            lit, dist = _fixed() if kind == 1 else _dynamic(b)
            while True:
                if b.n < 48:
                    b.fill()
                s = b.symbol(lit)
                if s < 256:
                    if len(out) >= expect:
                        raise _Stop(TOO_LONG)
                    out.append(s)
                    continue
                if s == 256:
                    break
                if s >= 286:
                    raise _Stop(BAD_CODE)
                length = LENGTH_BASE[s - 257] + b.bits(LENGTH_EXTRA[s - 257])
                ds = b.symbol(dist)
                if ds >= 30:
                    raise _Stop(BAD_CODE)
                d = DIST_BASE[ds] + b.bits(DIST_EXTRA[ds])
                if d > len(out):
                    raise _Stop(BAD_DISTANCE)
                if length > expect - len(out):
                    raise _Stop(TOO_LONG)
                st["length_codes"].add(s - 257)
                st["distance_codes"].add(ds)
                st["matches"] += 1
                st["overlapping"] += d < length
                st["largest_distance"] = max(st["largest_distance"], d)
                st["longest"] = max(st["longest"], length)
                if d >= length:
                    out += out[len(out) - d:len(out) - d + length]
                else:
                    for _ in range(length):
                        out.append(out[-d])
        if len(out) != expect:
            raise _Stop(TOO_SHORT)
        b.bits(b.n & 7)
        b.fill()
        if b.n < 32:
            raise _Stop(OVERRUN)
        if int.from_bytes(b.bits(32).to_bytes(4, "little"), "big") != zlib.adler32(bytes(out)):
            raise _Stop(BAD_CHECK)
    except _Stop as stop:
        return stop.status, bytes(out)
    return OK, bytes(out)


def zlib_verdict(data, expect):
    """(True where `zlib.decompress` accepts the stream with `expect` bytes, the bytes or zlib's message)."""
    try:
        raw = zlib.decompress(bytes(data))
    except zlib.error as exc:
        return False, str(exc)
    return len(raw) == expect, raw


# ------------------------------------------------------------------ the streams of the tests
CONFIGS = (("l0", 0, zlib.Z_DEFAULT_STRATEGY), ("l1", 1, zlib.Z_DEFAULT_STRATEGY), ("l6", 6, zlib.Z_DEFAULT_STRATEGY), ("l9", 9, zlib.Z_DEFAULT_STRATEGY),
           ("fixed", 9, zlib.Z_FIXED), ("rle", 6, zlib.Z_RLE), ("huff", 6, zlib.Z_HUFFMAN_ONLY))
SIZES = ((1, 1), (1, 7), (2, 2), (8, 8), (17, 23), (33, 65), (65, 67))


def deflate(raw, level, strategy, wbits=15):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    return c.compress(bytes(raw)) + c.flush()


@functools.lru_cache(None)
def filtered_images():
    """{name: the filtered bytes of an image}: flat, tiled, smooth plus noise and noise at every size, and two frames whose rows repeat
    with a period (matches at multiples of the row stride): 64 x 64 with period 3 and 256 x 256 with period 5."""
    rng = np.random.default_rng(23)
    out = {}
    for h, w in SIZES:
        yy, xx = np.mgrid[0:h, 0:w]
        smooth = 128 + 60 * np.sin(xx / 9.0 + 0.3) + 50 * np.cos(yy / 7.0)
        imgs = {"flat": np.full((h, w, 3), 77), "tiled": np.stack([(xx % 4) * 60 + (yy % 3) * 5, (xx % 4) * 11, (yy % 3) * 90], -1),
                "smooth": np.stack([smooth, smooth * 0.8 + 20, 255 - smooth], -1) + rng.integers(-2, 3, (h, w, 3)), "noise": rng.integers(0, 256, (h, w, 3))}
        for name, v in imgs.items():
            out[f"{name}_{h}x{w}"] = R.filter_rows(np.clip(v, 0, 255).astype(np.uint8), -1)[0].tobytes()
    for h, w, period in ((64, 64, 3), (256, 256, 5)):
        rows = rng.integers(0, 256, (period, w, 3))
        img = rows[np.arange(h) % period].astype(np.uint8)
        out[f"periodic_{h}x{w}"] = R.filter_rows(img, 0)[0].tobytes()
    return out


@functools.lru_cache(None)
def planted():
    """33,000 noise bytes, then for every length L (each length code's base, base + 1, 257, 258) and distance D (each distance code's
    base, 2 base - 1, 32768) a copy of L bytes from D back, a byte that breaks the match and 5 noise bytes."""
    rng = np.random.default_rng(5)
    buf = bytearray(rng.integers(0, 256, 33000, dtype=np.uint8).tobytes())
    ls = sorted({v for b in LENGTH_BASE for v in (b, b + 1) if v <= 258} | {257, 258})
    ds = sorted({min(v, 32768) for b in DIST_BASE for v in (b, 2 * b - 1)} | {32768})
    for L in ls:
        for D in ds:
            for _ in range(L):
                buf.append(buf[-D])
            buf.append(buf[-D] ^ 0x5A)
            buf += rng.integers(0, 256, 5, dtype=np.uint8).tobytes()
    return bytes(buf)


@functools.lru_cache(None)
def plain_streams():
    """[(name, stream, the bytes it holds)]: every filtered image and the planted buffer at every configuration, the mirrored rows of
    apng_ref with the adaptive filter at every band_rows, a stored stream of several blocks and a wbits = 9 stream."""
    out = []
    for name, raw in list(filtered_images().items()) + [("planted", planted())]:
        for cfg, level, strategy in CONFIGS:
            out.append((f"{name}/{cfg}", deflate(raw, level, strategy), raw))
    for key, name, flt, r in R.rows():
        if flt == -1 and (not name.endswith("256x256") or r in (0, 255)):
            m = R.mirrored(key)
            out.append((f"apng_ref/{key}", bytes(m["stream"]), bytes(m["filtered"])))
    big = np.random.default_rng(6).integers(0, 256, 150001, dtype=np.uint8).tobytes()
    out.append(("stored_150001/l0", deflate(big, 0, zlib.Z_DEFAULT_STRATEGY), big))
    raw = filtered_images()["smooth_33x65"]
    out.append(("smooth_33x65/wbits9", deflate(raw, 6, zlib.Z_DEFAULT_STRATEGY, 9), raw))
    return out


# ---- hand-assembled streams: a bit writer with the fixed codes
class Writer:
    def __init__(self):
        self.acc, self.n = 0, 0

    def bits(self, v, n):                       # a number, LSB first
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        return self

    def code(self, c, n):                       # a Huffman code, MSB first
        return self.bits(R.reverse_bits(c, n), n)

    def align(self):
        return self.bits(0, -self.n % 8)

    def raw(self, data):
        assert self.n % 8 == 0
        for v in data:
            self.bits(v, 8)
        return self

    def lit(self, s):                           # a literal/length symbol in the fixed code
        if s < 144:
            return self.code(0x30 + s, 8)
        if s < 256:
            return self.code(0x190 + s - 144, 9)
        if s < 280:
            return self.code(s - 256, 7)
        return self.code(0xC0 + s - 280, 8)

    def match(self, length, dist):              # in the fixed codes
        li = max(i for i in range(29) if LENGTH_BASE[i] <= length and (i < 28 or length == 258))
        self.lit(257 + li).bits(length - LENGTH_BASE[li], LENGTH_EXTRA[li])
        di = max(i for i in range(30) if DIST_BASE[i] <= dist)
        return self.code(di, 5).bits(dist - DIST_BASE[di], DIST_EXTRA[di])

    def stored(self, data, final=0, nlen=None):
        self.bits(final, 1).bits(0, 2).align().bits(len(data), 16).bits(~len(data) if nlen is None else nlen, 16)
        return self.raw(data)

    def dynamic(self, cl, symbols, hlit, hdist, final=1):
        """A dynamic header: the code-length code's lengths cl[19] and the (code-length symbol, extra value) pairs."""
        hclen = max(4, max((i + 1 for i in range(19) if cl[R.CL_ORDER[i]]), default=4))
        self.bits(final, 1).bits(2, 2).bits(hlit - 257, 5).bits(hdist - 1, 5).bits(hclen - 4, 4)
        for i in range(hclen):
            self.bits(cl[R.CL_ORDER[i]], 3)
        codes = R.canonical(list(cl))
        for s, extra in symbols:
            self.code(codes[s], cl[s])
            if s >= 16:
                self.bits(extra, (2, 3, 7)[s - 16])
        return self

    def bytes(self):
        return self.align().acc.to_bytes(self.n // 8, "little")


def zwrap(body, raw, header=b"\x78\x01", adler=None, tail=b""):
    return header + body + (zlib.adler32(bytes(raw)) if adler is None else adler).to_bytes(4, "big") + tail


CL_PLAIN = [4] * 16 + [0] * 3                   # the code-length code of the hand-made dynamic headers: lengths 0 .. 15 in 4 bits each


def _lengths(lit, dist, hlit=None, hdist=None):
    """(symbols, hlit, hdist) of a dynamic header that states the given {symbol: length} sets under CL_PLAIN."""
    hlit = hlit or max(257, max(lit) + 1)
    hdist = hdist or max(1, max(dist, default=0) + 1)
    return [(lit.get(i, 0), 0) for i in range(hlit)] + [(dist.get(i, 0), 0) for i in range(hdist)], hlit, hdist


@functools.lru_cache(None)
def hand_streams():
    """[(name, stream, expected bytes, the status word)]."""
    rng = np.random.default_rng(8)
    noise = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    out = []
    add = lambda name, stream, expect, status: out.append((name, bytes(stream), expect, status))
    fixed = lambda w=None: (w or Writer()).bits(1, 1).bits(1, 2)
    raw = noise + noise[:10]
    add("distance_32768", zwrap(fixed(Writer().stored(noise)).match(10, 32768).lit(256).bytes(), raw), len(raw), OK)
    raw = noise[:100] + noise[:5]
    add("distance_all_produced", zwrap(fixed(Writer().stored(noise[:100])).match(5, 100).lit(256).bytes(), raw), 105, OK)
    add("distance_one_before", zwrap(fixed(Writer().stored(noise[:100])).match(5, 101).lit(256).bytes(), raw), 105, BAD_DISTANCE)
    add("overlap_258_dist_1", zwrap(fixed().lit(65).match(258, 1).lit(256).bytes(), b"A" * 259), 259, OK)
    add("block_type_3", zwrap(Writer().bits(1, 1).bits(3, 2).bytes(), b""), 0, BAD_BLOCK)
    add("len_nlen", zwrap(Writer().stored(b"abc", 1, nlen=0x1234).bytes(), b"abc"), 3, BAD_BLOCK)
    add("symbol_286", zwrap(fixed().lit(65).lit(286).lit(256).bytes(), b"A"), 1, BAD_CODE)
    add("distance_symbol_30", zwrap(fixed().lit(65).lit(257).code(30, 5).lit(256).bytes(), b"A"), 1, BAD_CODE)
    body = lambda lit, dist, tokens, **k: tokens(Writer().dynamic(CL_PLAIN, *_lengths(lit, dist, **k))).bytes()
    add("oversubscribed", zwrap(body({65: 1, 66: 1, 256: 1}, {}, lambda w: w.bits(0, 8)), b""), 0, BAD_TABLE)
    add("incomplete", zwrap(body({65: 2, 256: 2}, {}, lambda w: w.bits(0, 8)), b""), 0, BAD_TABLE)
    # 'A' is 0, end-of-block 10, length 3 is 11; the one distance code (distance 1) is the bit 0
    one = {65: 1, 256: 2, 257: 2}
    add("single_distance_code", zwrap(body(one, {0: 1}, lambda w: w.code(0, 1).code(3, 2).code(0, 1).code(2, 2)), b"AAAA"), 4, OK)
    add("single_distance_code_unused_bit", zwrap(body(one, {0: 1}, lambda w: w.code(0, 1).code(3, 2).code(1, 1).code(2, 2).bits(0, 16)), b"AAAA"), 4, BAD_CODE)
    add("no_distance_codes", zwrap(body(one, {}, lambda w: w.code(0, 1).code(0, 1).code(2, 2)), b"AA"), 2, OK)
    add("no_distance_codes_match", zwrap(body(one, {}, lambda w: w.code(0, 1).code(3, 2).bits(0, 16)), b"A"), 1, BAD_CODE)
    add("no_end_of_block", zwrap(body({65: 1, 66: 1}, {}, lambda w: w.bits(0, 8)), b""), 0, BAD_TABLE)
    cl = [4] * 14 + [0, 0, 4, 4, 0]
    add("repeat_without_previous", zwrap(Writer().dynamic(cl, [(16, 0)] + [(1, 0)] * 20, 257, 1).bits(0, 16).bytes(), b""), 0, BAD_TABLE)
    cl = [4] * 14 + [0, 0, 0, 4, 4]
    add("repeat_past_the_end", zwrap(Writer().dynamic(cl, [(1, 0)] * 250 + [(18, 127)], 257, 1).bits(0, 16).bytes(), b""), 0, BAD_TABLE)
    add("hlit_287", zwrap(Writer().bits(1, 1).bits(2, 2).bits(30, 5).bits(0, 5).bits(0, 4).bits(0, 64).bytes(), b""), 0, BAD_TABLE)
    add("hdist_31", zwrap(Writer().bits(1, 1).bits(2, 2).bits(0, 5).bits(30, 5).bits(0, 4).bits(0, 64).bytes(), b""), 0, BAD_TABLE)
    good = fixed().lit(104).lit(105).lit(256).bytes()
    add("fdict", zwrap(good, b"hi", header=b"\x78\x20"), 2, BAD_HEADER)
    add("fcheck", zwrap(good, b"hi", header=b"\x78\x02"), 2, BAD_HEADER)
    add("method_7", zwrap(good, b"hi", header=b"\x77\x09"), 2, BAD_HEADER)
    add("window_64k", zwrap(good, b"hi", header=b"\x88\x1c"), 2, BAD_HEADER)
    add("adler", zwrap(good, b"hi", adler=zlib.adler32(b"hi") ^ 0x100), 2, BAD_CHECK)
    add("good", zwrap(good, b"hi"), 2, OK)
    add("expected_one_more", zwrap(good, b"hi"), 3, TOO_SHORT)
    add("expected_one_less", zwrap(good, b"hi"), 1, TOO_LONG)
    add("match_expected_one_less", zwrap(fixed().lit(65).match(258, 1).lit(256).bytes(), b"A" * 259), 258, TOO_LONG)
    add("stored_expected_one_less", zwrap(Writer().stored(b"abc", 1).bytes(), b"abc"), 2, TOO_LONG)
    add("garbage_behind", zwrap(good, b"hi", tail=b"\xde\xad\xbe\xef\x01"), 2, OK)
    add("adler_cut", zwrap(good, b"hi")[:-1], 2, OVERRUN)
    add("empty", b"", 0, OVERRUN)
    add("empty_stream", zwrap(fixed().lit(256).bytes(), b""), 0, OK)
    return out


@functools.lru_cache(None)
def mutations(count=2000):
    """[(name, stream, expected bytes)]: deterministic mutations of the plain streams of up to 4000 bytes -- truncation, one byte
    altered, a random tail, a wrong expected size.  Every fourth source carries six bytes behind its Adler-32, which zlib ignores, so
    that a mutation there is one zlib accepts."""
    rng = np.random.RandomState(11)
    src = [(n, s, len(raw)) for n, s, raw in plain_streams() if len(s) <= 4000 and len(raw) > 0]
    out = []
    for i in range(count):
        k = rng.randint(len(src))
        name, s, expect = src[k]
        if k % 4 == 0:
            s = s + b"\x00\x11\x22\x33\x44\x55"
        s = bytearray(s)
        kind = i % 4
        if kind == 0:
            s = s[:rng.randint(0, len(s))]
        elif kind == 1:
            s[rng.randint(len(s))] ^= rng.randint(1, 256)
        elif kind == 2:
            cut = rng.randint(0, len(s))
            s[cut:] = rng.randint(0, 256, size=len(s) - cut).astype(np.uint8).tobytes()
        else:
            expect = max(0, expect + (1, -1, 7, -expect // 2)[(i // 4) % 4])
        out.append((f"{name}/m{i}", bytes(s), expect))
    return out


@functools.lru_cache(None)
def judged(which):
    """[(name, stream, expected bytes, the mirror's status, the mirror's output)] of "plain", "hand" or "mutations": computed once per
    process, shared by the host, sanitizer and GPU tests."""
    if which == "plain":
        cases = [(n, s, len(raw)) for n, s, raw in plain_streams()]
    elif which == "hand":
        cases = [(n, s, e) for n, s, e, _ in hand_streams()]
    else:
        cases = mutations()
    return [(n, s, e) + inflate(s, e) for n, s, e in cases]

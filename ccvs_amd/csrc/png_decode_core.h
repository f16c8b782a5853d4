// The inflate of the PNG decoder (png_decode.hip): a complete RFC 1950 / RFC 1951 decoder of ONE zlib stream
// -- the bit reader, the header check, stored, fixed and dynamic blocks, canonical tables under zlib's acceptance rules, matches and
// the Adler-32 sums.  Plain C++ behind PD_FN, which is `__host__ __device__` under hipcc and empty otherwise, so that the same text
// runs in the kernel and in a host program under the sanitizers (tests/test_png_decode_core.py).
//
// The serial part (`pd_run`, which the kernel's wave runs uniformly: see PD_U) touches three small buffers only, which the kernel
// keeps in LDS: the block's tables, a STAGE
// of the next input bytes (PD_STAGE, a ring over the stream's byte positions) and a RING of the last output bytes (PD_RING: the 32768
// a match may reach and what is not flushed yet).  It stops at token boundaries when the stage runs low (`pd_refill_lane`: all lanes
// copy the next bytes of the stream into the stage) or PD_FLUSH bytes wait in the ring (`pd_flush_lane`: all lanes copy them to the
// output and fold them into the Adler-32 sums), and goes on from its state (`PdStream`).  Whatever the bytes hold: nothing outside
// data[0 .. len) is read, nothing outside out[0 .. expect) is written, a match never reaches before the first produced byte, stage
// and ring are indexed under their masks, and every loop consumes input or produces output (or counts a table index up to its
// bound), so it ends.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define PD_FN __host__ __device__ inline
#else
#define PD_FN inline
#endif

// status of a stream (`ccvs_amd.ops.PD_STATUS` and tests/png_decode_ref.py keep the same list)
#define PD_OK 0
#define PD_BAD_STREAM 1     // the table row points outside the call's buffers
#define PD_BAD_HEADER 2     // CM != 8, CINFO > 7, FCHECK wrong or FDICT set
#define PD_BAD_BLOCK 3      // block type 3, or a stored block whose LEN != ~NLEN
#define PD_BAD_TABLE 4      // HLIT > 286, HDIST > 30, a repeat with nothing before it or past the end, an over-subscribed or incomplete
                            // set of lengths, no end-of-block code
#define PD_BAD_CODE 5       // no code starts so; literal/length symbol 286 / 287, distance symbol 30 / 31
#define PD_BAD_DISTANCE 6   // a match reaches before the first byte of the output
#define PD_OVERRUN 7        // the input ended
#define PD_TOO_LONG 8       // more output than expected
#define PD_TOO_SHORT 9      // the final block ended before the expected output was there
#define PD_BAD_CHECK 10     // the Adler-32 behind the last block is not that of the output
#define PD_BAD_FILTER 11    // a row's filter type byte is above 4 (set by the un-filter of ccvs_png_decode only)

// `pd_run` is written for the whole wave running it uniformly: every lane holds the same state and takes the same branches, and every
// value READ from a buffer passes PD_U, which on the device names it wave-uniform (the first lane's), so that the compiler keeps the
// serial loop on the scalar unit instead of spending a 64-lane vector instruction per step.  On the host PD_U is the value itself.
#if defined(__HIP_DEVICE_COMPILE__)
#define PD_U(x) ((unsigned)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define PD_U(x) ((unsigned)(x))
#endif

#define PD_LOOK_BITS 10
#define PD_ADLER_MOD 65521

// One canonical Huffman code: count[l] codes of length l, their symbols in code order, and a lookup of the next PD_LOOK_BITS bits
// (LSB first, as the stream holds them: a code's bits reversed) -> (length << 9) | symbol for codes of up to PD_LOOK_BITS bits, else 0.
struct PdHuff {
    uint16_t count[16];
    uint16_t sym[288];
    uint16_t look[1 << PD_LOOK_BITS];
};
// the tables of the block being decoded (in LDS in the kernel); `lens` is the scratch the code lengths are gathered in
struct PdTables {
    PdHuff lit, dist;
    uint8_t lens[320];
};

#define PD_KIND_CODES 0   // the code-length code
#define PD_KIND_LENS 1    // the literal/length code
#define PD_KIND_DISTS 2   // the distance code

// zlib's rules (inftrees.c): no code at all is accepted (it fails when a symbol is needed); over-subscribed is refused; incomplete is
// refused unless it is a literal/length or distance code whose longest code has one bit.  Returns PD_OK or PD_BAD_TABLE.
PD_FN int pd_build(PdHuff& h, const uint8_t* lens, int n, int kind) {
    for (int l = 0; l < 16; ++l) h.count[l] = 0;
    for (int i = 0; i < n; ++i) ++h.count[PD_U(lens[i]) & 15];
    for (int i = 0; i < (1 << PD_LOOK_BITS); ++i) h.look[i] = 0;
    if ((int)PD_U(h.count[0]) == n) return PD_OK;
    int left = 1, max = 0;
    for (int l = 1; l < 16; ++l) {
        const int c = (int)PD_U(h.count[l]);
        left = (left << 1) - c;
        if (left < 0) return PD_BAD_TABLE;
        if (c) max = l;
    }
    if (left > 0 && (kind == PD_KIND_CODES || max != 1)) return PD_BAD_TABLE;
    uint16_t offs[16], next[16];
    offs[1] = 0;
    next[1] = 0;
    for (int l = 1; l < 15; ++l) {
        const unsigned c = PD_U(h.count[l]);
        offs[l + 1] = (uint16_t)(offs[l] + c);
        next[l + 1] = (uint16_t)((next[l] + c) << 1);   // (the first code of each length, RFC 1951 3.2.2)
    }
    for (int i = 0; i < n; ++i) {
        const int l = (int)(PD_U(lens[i]) & 15);
        if (!l) continue;
        h.sym[offs[l]++] = (uint16_t)i;
        const unsigned code = next[l]++;
        if (l <= PD_LOOK_BITS) {
            unsigned rev = 0;
            for (int k = 0; k < l; ++k) rev |= ((code >> k) & 1u) << (l - 1 - k);
            for (unsigned k = rev; k < (1u << PD_LOOK_BITS); k += 1u << l) h.look[k] = (uint16_t)((l << 9) | i);
        }
    }
    return PD_OK;
}

// ---- the state of one stream between two runs of `pd_run`
#define PD_RING 65536    // bytes of the output ring (a power of two)
#define PD_STAGE 4096    // bytes of the input stage (a power of two)
#define PD_FLUSH 16384   // bytes waiting in the ring at which a run stops for a flush
#define PD_NEED 600      // staged bytes ahead below which a run stops for a refill: above a dynamic header's 14 + 19 * 3 + 316 * 14 bits
#define PD_BACK 8        // bytes behind `pos` the stage keeps: a stored block hands the accumulator's whole bytes back

// The ring holds the 32768 bytes a match may reach, up to PD_FLUSH - 1 bytes that wait when a run goes on, and what one more step adds
// before the next check: a stored piece of up to PD_FLUSH bytes, or a match of 258.
static_assert(PD_RING >= 32768 + 2 * PD_FLUSH && PD_FLUSH >= 258, "the output ring would overwrite match sources or unflushed bytes");
static_assert((PD_RING & (PD_RING - 1)) == 0 && (PD_STAGE & (PD_STAGE - 1)) == 0 && PD_STAGE >= 2 * PD_NEED + PD_BACK, "ring and stage sizes");

#define PD_PHASE_HEADER 0   // the two bytes of RFC 1950
#define PD_PHASE_BLOCK 1    // a block header is due
#define PD_PHASE_STORED 2   // `remain` bytes of a stored block are to be copied
#define PD_PHASE_CODES 3    // tokens of a fixed or dynamic block
#define PD_PHASE_CHECK 4    // the Adler-32

#define PD_RUN_INPUT (-1)   // pd_run wants more input staged
#define PD_RUN_FLUSH (-2)   // pd_run wants the ring flushed

struct PdStream {
    long len, expect;         // bytes of the stream; bytes it is to hold
    long pos, staged;         // input bytes taken into the accumulator; input bytes staged so far (stage[p & (PD_STAGE - 1)] holds byte p)
    long produced, flushed;   // output bytes made (ring[p & (PD_RING - 1)] holds byte p); output bytes flushed
    uint64_t acc;             // `n` valid bits, the stream's next bit lowest, zeros above
    int n, phase, final, remain;
    uint32_t check;           // the Adler-32 the stream states (after PD_OK)
};
PD_FN void pd_begin(PdStream& s, long len, long expect) {
    s.len = len, s.expect = expect, s.pos = 0, s.staged = 0, s.produced = 0, s.flushed = 0;
    s.acc = 0, s.n = 0, s.phase = PD_PHASE_HEADER, s.final = 0, s.remain = 0, s.check = 0;
}
// the stream positions [from, to) the stage may take next: as far as it reaches without overwriting a byte from pos - PD_BACK on
PD_FN long pd_refill_end(const PdStream& s) {
    const long to = s.pos - PD_BACK + PD_STAGE;
    return to < s.len ? to : s.len;
}
// lane `lane` of `lanes`: its share of data[from .. to) into the stage
PD_FN void pd_refill_lane(const uint8_t* data, uint8_t* stage, long from, long to, int lane, int lanes) {
    for (long i = from + lane; i < to; i += lanes) stage[i & (PD_STAGE - 1)] = data[i];
}

// ---- the bit reader over the stage: whole aligned 32-bit words where the position allows, bytes up to there and at the end.  After
// pd_fill at least 33 bits are valid unless the staged bytes end (a run starts a token only with PD_NEED bytes staged ahead, or all).
PD_FN void pd_fill(PdStream& s, const uint8_t* stage) {
    for (;;) {
        const long left = s.staged - s.pos;
        if (s.n <= 32 && (s.pos & 3) == 0 && left >= 4) {
            uint32_t v;
            memcpy(&v, __builtin_assume_aligned(stage + (s.pos & (PD_STAGE - 1)), 4), 4);   // (the stage is 4-byte aligned; little-endian hosts and the GPU)
            s.acc |= (uint64_t)PD_U(v) << s.n;
            s.n += 32;
            s.pos += 4;
        } else if (s.n <= 56 && left > 0 && ((s.pos & 3) != 0 || left < 4)) {
            s.acc |= (uint64_t)PD_U(stage[s.pos & (PD_STAGE - 1)]) << s.n;
            s.n += 8;
            ++s.pos;
        } else {
            return;
        }
    }
}
PD_FN void pd_drop(PdStream& b, int k) {
    b.acc >>= k;
    b.n -= k;
}
// k <= 16 bits as a number; PD_OVERRUN where fewer are left (the caller has filled)
PD_FN int pd_bits(PdStream& b, int k, int& v) {
    if (b.n < k) return PD_OVERRUN;
    v = (int)(b.acc & ((1u << k) - 1u));
    pd_drop(b, k);
    return PD_OK;
}
// One symbol (the caller has filled: 15 bits are there unless the input ends).
PD_FN int pd_symbol(PdStream& b, const PdHuff& h, int& sym) {
    const unsigned e = PD_U(h.look[b.acc & ((1u << PD_LOOK_BITS) - 1u)]);
    if (e) {
        const int l = (int)(e >> 9);
        if (l > b.n) return PD_OVERRUN;
        sym = (int)(e & 511u);
        pd_drop(b, l);
        return PD_OK;
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; ++l) {
        if (l > b.n) return PD_OVERRUN;
        code |= (int)((b.acc >> (l - 1)) & 1u);
        const int count = (int)PD_U(h.count[l]);
        if (code - count < first) {
            sym = (int)PD_U(h.sym[index + (code - first)]);
            pd_drop(b, l);
            return PD_OK;
        }
        index += count;
        first = (first + count) << 1;
        code <<= 1;
    }
    return PD_BAD_CODE;
}

PD_FN int pd_length_base(int i) {
    constexpr uint16_t t[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    return t[i];
}
PD_FN int pd_length_extra(int i) { return (i < 8 || i == 28) ? 0 : (i - 4) >> 2; }
PD_FN int pd_dist_base(int i) {
    constexpr uint16_t t[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    return t[i];
}
PD_FN int pd_dist_extra(int i) { return i < 4 ? 0 : (i - 2) >> 1; }

// the tables of a fixed block (RFC 1951 3.2.6): 288 and 32 codes, so that both sets are complete; symbols 286 / 287 and 30 / 31
// decode and are refused where they turn up
PD_FN void pd_fixed(PdTables& t) {
    for (int i = 0; i < 288; ++i) t.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    pd_build(t.lit, t.lens, 288, PD_KIND_LENS);
    for (int i = 0; i < 32; ++i) t.lens[i] = 5;
    pd_build(t.dist, t.lens, 32, PD_KIND_DISTS);
}

// the header of a dynamic block (RFC 1951 3.2.7) into t.lit and t.dist
PD_FN int pd_dynamic(PdStream& b, const uint8_t* stage, PdTables& t) {
    constexpr uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    int st, v;
    pd_fill(b, stage);
    if ((st = pd_bits(b, 14, v))) return st;
    const int hlit = (v & 31) + 257, hdist = ((v >> 5) & 31) + 1, hclen = (v >> 10) + 4;
    if (hlit > 286 || hdist > 30) return PD_BAD_TABLE;
    for (int i = 0; i < 19; ++i) t.lens[i] = 0;
    for (int i = 0; i < hclen; ++i) {
        pd_fill(b, stage);
        if ((st = pd_bits(b, 3, v))) return st;
        t.lens[order[i]] = (uint8_t)v;
    }
    if ((st = pd_build(t.dist, t.lens, 19, PD_KIND_CODES))) return st;
    if (PD_U(t.dist.count[0]) == 19) return PD_BAD_TABLE;   // (zlib reads such a set as zeros and then misses the end-of-block code)
    const int total = hlit + hdist;
    for (int i = 0; i < total;) {
        int sym;
        pd_fill(b, stage);
        if ((st = pd_symbol(b, t.dist, sym))) return st;
        if (sym < 16) {
            t.lens[i++] = (uint8_t)sym;
            continue;
        }
        int rep, prev = 0;
        if (sym == 16) {
            if (i == 0) return PD_BAD_TABLE;
            prev = (int)PD_U(t.lens[i - 1]);
            if ((st = pd_bits(b, 2, v))) return st;
            rep = 3 + v;
        } else if (sym == 17) {
            if ((st = pd_bits(b, 3, v))) return st;
            rep = 3 + v;
        } else {
            if ((st = pd_bits(b, 7, v))) return st;
            rep = 11 + v;
        }
        if (i + rep > total) return PD_BAD_TABLE;
        while (rep--) t.lens[i++] = (uint8_t)prev;
    }
    if (PD_U(t.lens[256]) == 0) return PD_BAD_TABLE;
    if ((st = pd_build(t.lit, t.lens, hlit, PD_KIND_LENS))) return st;
    return pd_build(t.dist, t.lens + hlit, hdist, PD_KIND_DISTS);
}

// `n` bytes from `dist` back (1 <= dist <= 32768 and <= at, checked by the caller) to ring position `at`: a byte may be one the copy
// itself wrote (dist < n).  Eight bytes at once where the distance keeps them apart and neither end wraps.
PD_FN void pd_copy(uint8_t* ring, long at, long dist, int n) {
    unsigned q = (unsigned)at & (PD_RING - 1), s = (unsigned)(at - dist) & (PD_RING - 1);
    if (dist >= 8)
        for (; n >= 8 && q <= PD_RING - 8 && s <= PD_RING - 8; n -= 8, q += 8, s += 8) {
            uint64_t v;
            memcpy(&v, ring + s, 8);
            memcpy(ring + q, &v, 8);
        }
    for (; n > 0; --n, ++q, ++s) ring[q & (PD_RING - 1)] = ring[s & (PD_RING - 1)];
}

// (Every lane of the wave calls it with the same state; the buffers' writes are the same value to the same address from every lane.)
// Runs the stream on from its state until it is done (returns its status: PD_OK means that it held exactly `expect` bytes, the last
// of them still in the ring, and s.check is the Adler-32 it states; bytes behind that are ignored), the stage runs low (PD_RUN_INPUT)
// or PD_FLUSH bytes wait in the ring (PD_RUN_FLUSH).  It stops between tokens only.
PD_FN int pd_run(PdStream& s, PdTables& t, const uint8_t* stage, uint8_t* ring) {
    int st, v;
    for (;;) {
        if (s.staged < s.len && s.staged - s.pos < PD_NEED) return PD_RUN_INPUT;
        if (s.produced - s.flushed >= PD_FLUSH) return PD_RUN_FLUSH;
        if (s.phase == PD_PHASE_CODES) {
            // A run of literals of up to PD_LOOK_BITS bits without the checks above: as many as the ring takes before its flush, as
            // the expected output has room for and as the staged input serves for certain (two bytes each at most, and a fill's
            // reach).  Whatever else comes -- a longer code, a match, the end of the block, an error -- is the general token's below.
            long quota = PD_FLUSH - (s.produced - s.flushed);
            if (quota > s.expect - s.produced) quota = s.expect - s.produced;
            if (quota > ((s.staged - s.pos) >> 1) - 8) quota = ((s.staged - s.pos) >> 1) - 8;
            if (quota > 0) {
                unsigned w = (unsigned)s.produced, left = (unsigned)quota;
                for (; left; --left) {
                    if (s.n < 15) pd_fill(s, stage);
                    const unsigned e = PD_U(t.lit.look[s.acc & ((1u << PD_LOOK_BITS) - 1u)]);
                    if (e == 0 || (e & 256u)) break;   // (symbols are below 288: bit 8 is set from 256 on)
                    ring[w++ & (PD_RING - 1)] = (uint8_t)e;
                    pd_drop(s, (int)(e >> 9));
                }
                s.produced += (long)((unsigned)quota - left);
            }
            int sym;
            pd_fill(s, stage);
            if ((st = pd_symbol(s, t.lit, sym))) return st;
            if (sym < 256) {
                if (s.produced >= s.expect) return PD_TOO_LONG;
                ring[s.produced++ & (PD_RING - 1)] = (uint8_t)sym;
                continue;
            }
            if (sym == 256) {
                s.phase = s.final ? PD_PHASE_CHECK : PD_PHASE_BLOCK;
                continue;
            }
            if (sym >= 286) return PD_BAD_CODE;
            if ((st = pd_bits(s, pd_length_extra(sym - 257), v))) return st;
            const int length = pd_length_base(sym - 257) + v;
            pd_fill(s, stage);
            if ((st = pd_symbol(s, t.dist, sym))) return st;
            if (sym >= 30) return PD_BAD_CODE;
            if ((st = pd_bits(s, pd_dist_extra(sym), v))) return st;
            const long dist = pd_dist_base(sym) + v;
            if (dist > s.produced) return PD_BAD_DISTANCE;
            if (length > s.expect - s.produced) return PD_TOO_LONG;
            pd_copy(ring, s.produced, dist, length);
            s.produced += length;
        } else if (s.phase == PD_PHASE_STORED) {
            // as many bytes as are staged and as the ring takes before its flush; the accumulator is empty here
            long k = s.remain;
            if (k > s.staged - s.pos) k = s.staged - s.pos;
            if (k > PD_FLUSH) k = PD_FLUSH;
            for (long i = 0; i < k; ++i) ring[(s.produced + i) & (PD_RING - 1)] = stage[(s.pos + i) & (PD_STAGE - 1)];
            s.pos += k;
            s.produced += k;
            s.remain -= (int)k;
            if (s.remain == 0) s.phase = s.final ? PD_PHASE_CHECK : PD_PHASE_BLOCK;
        } else if (s.phase == PD_PHASE_BLOCK) {
            pd_fill(s, stage);
            if ((st = pd_bits(s, 3, v))) return st;
            s.final = v & 1;
            const int type = v >> 1;
            if (type == 3) return PD_BAD_BLOCK;
            if (type == 0) {
                pd_drop(s, s.n & 7);
                pd_fill(s, stage);
                int n, nn;
                if ((st = pd_bits(s, 16, n)) || (st = pd_bits(s, 16, nn))) return st;
                if ((n ^ nn) != 0xFFFF) return PD_BAD_BLOCK;
                s.pos -= s.n >> 3;   // the whole bytes in the accumulator go back: the block's bytes are copied from the stage itself
                s.n = 0;
                s.acc = 0;
                if (n > s.len - s.pos) return PD_OVERRUN;
                if (n > s.expect - s.produced) return PD_TOO_LONG;
                s.remain = n;
                s.phase = n ? PD_PHASE_STORED : s.final ? PD_PHASE_CHECK : PD_PHASE_BLOCK;
            } else {
                if (type == 1) pd_fixed(t);
                else if ((st = pd_dynamic(s, stage, t))) return st;
                s.phase = PD_PHASE_CODES;
            }
        } else if (s.phase == PD_PHASE_HEADER) {
            if (s.len < 2) return PD_OVERRUN;
            const unsigned cmf = PD_U(stage[0]), flg = PD_U(stage[1]);
            if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u || (flg & 32u)) return PD_BAD_HEADER;
            s.pos = 2;
            s.phase = PD_PHASE_BLOCK;
        } else {
            if (s.produced != s.expect) return PD_TOO_SHORT;
            pd_drop(s, s.n & 7);
            pd_fill(s, stage);
            if (s.n < 32) return PD_OVERRUN;
            const uint32_t w = (uint32_t)s.acc;
            s.check = (w << 24) | ((w & 0xFF00u) << 8) | ((w >> 8) & 0xFF00u) | (w >> 24);
            return PD_OK;
        }
    }
}

// ---- Adler-32 by `lanes` lanes: of the bytes [from, to) of the stream's output, lane `lane` takes from + lane, from + lane + lanes,
// ... out of the ring into out[] and adds d[i] to s1 and (expect - i) d[i] to s2, the weight kept mod 65521 by subtraction
// (lanes < 65521).  The sums of all lanes over all flushes give adler = ((expect + S2) mod 65521) << 16 | ((1 + S1) mod 65521).
PD_FN void pd_flush_lane(const uint8_t* ring, uint8_t* out, long from, long to, long expect, int lane, int lanes, uint64_t& s1, uint64_t& s2) {
    long i = from + lane;
    if (i >= to) return;
    int32_t wt = (int32_t)((expect - i) % PD_ADLER_MOD);
    uint64_t a = 0, c = 0;
    for (; i < to; i += lanes) {
        const uint32_t d = ring[i & (PD_RING - 1)];
        out[i] = (uint8_t)d;
        a += d;
        c += (uint64_t)((uint32_t)wt * d);   // (below 2^24 each, at most PD_RING of them)
        wt -= lanes;
        if (wt < 0) wt += PD_ADLER_MOD;
    }
    s1 = (s1 + a) % PD_ADLER_MOD;
    s2 = (s2 + c) % PD_ADLER_MOD;
}
PD_FN uint32_t pd_adler_join(long n, uint64_t S1, uint64_t S2) {
    return (uint32_t)(((uint64_t)(n % PD_ADLER_MOD) + S2) % PD_ADLER_MOD) << 16 | (uint32_t)((1u + S1) % PD_ADLER_MOD);
}

// The whole of one stream as the kernel runs it, the lanes one after the other: for the host.  `stage` and `ring` are PD_STAGE and
// PD_RING bytes.
PD_FN int pd_inflate_checked(const uint8_t* data, long len, uint8_t* out, long expect, PdTables& t, uint8_t* stage, uint8_t* ring, int lanes) {
    PdStream s;
    pd_begin(s, len, expect);
    uint64_t S1 = 0, S2 = 0;
    for (;;) {
        const int r = pd_run(s, t, stage, ring);
        if (r == PD_RUN_INPUT) {
            const long to = pd_refill_end(s);
            for (int l = 0; l < lanes; ++l) pd_refill_lane(data, stage, s.staged, to, l, lanes);
            s.staged = to;
            continue;
        }
        if (r != PD_RUN_FLUSH && r != PD_OK) return r;
        for (int l = 0; l < lanes; ++l) {
            uint64_t s1 = 0, s2 = 0;
            pd_flush_lane(ring, out, s.flushed, s.produced, expect, l, lanes, s1, s2);
            S1 += s1;
            S2 += s2;
        }
        s.flushed = s.produced;
        if (r == PD_OK) return pd_adler_join(expect, S1, S2) == s.check ? PD_OK : PD_BAD_CHECK;
    }
}

// The serial parts of the GIF output stage (gif.hip, include/ccvs_hip_output_gif.h): the LZW coder of one band
// and the arithmetic that stitches a frame's bands into sub-blocks.  Plain C++ behind GIF_FN, which is `__host__ __device__` under hipcc
// and empty otherwise, so that the same text runs in the kernel and in a host program under the sanitizers (tests/gif_core_check.cpp).
//
// The coder is written for one wave running it uniformly: every lane holds the same state and takes the same branches, every value
// READ from a buffer passes GIF_U, which on the device names it wave-uniform (the first lane's), and only the lane whose `writer` is
// set stores.  The dictionary is an open-addressed hash of GIF_SLOTS words; a dictionary holds at most 4096 - 258 = 3838 strings, so
// it is never half full, and the probe loop is bounded by the slot count besides: it ends whatever the table holds.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define GIF_FN __host__ __device__ inline
#else
#define GIF_FN inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define GIF_U(x) ((unsigned)__builtin_amdgcn_readfirstlane((int)(x)))
// the writer lane's store to the dictionary is ordered before the wave's next reads of it
#define GIF_WAVE_SYNC()                                     \
    do {                                                    \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                    \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
    } while (0)
#else
#define GIF_U(x) ((unsigned)(x))
#define GIF_WAVE_SYNC() do { } while (0)
#endif

#define GIF_CLEAR 256
#define GIF_EOI 257
#define GIF_FIRST 258
#define GIF_FULL 4096
#define GIF_SLOTS 8192               // a power of two, more than twice the 3838 strings of a full dictionary
#define GIF_EMPTY 0xFFFFFFFFu        // (no entry looks so: its code would be 4095 and its prefix 4095 too, but a string's code is above its prefix's)
#define GIF_DEFAULT_BAND 4096        // indices of a band where the caller does not say
#define GIF_FILL 3838                // strings until the dictionary is full

// the state of one band's coder
struct GifCoder {
    int prefix;                      // the pending string's code; -1 before the band's first index
    int free, width;
    int full;                        // the dictionary was reset: the caller empties the hash before the next call
    int writer;                      // this lane stores (the host: always)
    unsigned long long acc;          // bits not yet stored, LSB first
    int nacc;
    long nbits;                      // the band's bits so far
    long nwords;                     // words stored
    unsigned* out;
};

GIF_FN void gif_put(GifCoder& s, unsigned code) {
    s.acc |= (unsigned long long)code << s.nacc;
    s.nacc += s.width;
    s.nbits += s.width;
    if (s.nacc >= 32) {
        if (s.writer) s.out[s.nwords] = (unsigned)s.acc;
        ++s.nwords;
        s.acc >>= 32;
        s.nacc -= 32;
    }
}

// free += 1 with the width rule
GIF_FN void gif_grow(GifCoder& s) {
    ++s.free;
    if (s.free > (1 << s.width) && s.width < 12) ++s.width;
}

GIF_FN void gif_start(GifCoder& s, unsigned* out, bool first, bool writer) {
    s.prefix = -1;
    s.free = GIF_FIRST;
    s.width = 9;
    s.full = 0;
    s.writer = writer ? 1 : 0;
    s.acc = 0;
    s.nacc = 0;
    s.nbits = 0;
    s.nwords = 0;
    s.out = out;
    if (first) gif_put(s, GIF_CLEAR);
}

GIF_FN unsigned gif_slot(unsigned key) { return (key * 2654435761u) >> 19; }   // 13 bits

// The next indices of the band, idx[0 .. n): returns how many were taken -- all of them, or fewer where the dictionary filled up and was
// reset (s.full: `hash` is to be emptied, every word GIF_EMPTY, before the call that goes on).  `hash`: GIF_SLOTS words.
GIF_FN int gif_code(GifCoder& s, unsigned* hash, const uint8_t* idx, int n) {
    int i = 0;
    if (s.prefix < 0 && n > 0) s.prefix = (int)GIF_U(idx[i++]);
    for (; i < n; ++i) {
        const unsigned c = GIF_U(idx[i]);
        const unsigned key = ((unsigned)s.prefix << 8) | c;
        unsigned slot = gif_slot(key);
        int hit = -1, probes = 0;
        for (; probes < GIF_SLOTS; ++probes) {
            const unsigned e = GIF_U(hash[slot]);
            if (e == GIF_EMPTY) break;
            if ((e >> 12) == key) {
                hit = (int)(e & 4095u);
                break;
            }
            slot = (slot + 1) & (GIF_SLOTS - 1);
        }
        if (hit >= 0) {
            s.prefix = hit;
            continue;
        }
        gif_put(s, (unsigned)s.prefix);
        if (s.free < GIF_FULL) {
            if (probes < GIF_SLOTS) {                           // (always: the hash is never full)
                if (s.writer) hash[slot] = (key << 12) | (unsigned)s.free;
                GIF_WAVE_SYNC();
            }
            gif_grow(s);
        }
        s.prefix = (int)c;
        if (s.free >= GIF_FULL) {
            gif_put(s, GIF_CLEAR);
            s.free = GIF_FIRST;
            s.width = 9;
            s.full = 1;
            return i + 1;
        }
    }
    return i;
}

// the end of the band: the pending string, the entry the decoder makes of it, then a clear code or (last) end of information; the
// last bits are stored.  Returns the band's bits.
GIF_FN long gif_finish(GifCoder& s, bool last) {
    if (s.prefix >= 0) gif_put(s, (unsigned)s.prefix);
    if (s.free < GIF_FULL) gif_grow(s);
    gif_put(s, last ? GIF_EOI : GIF_CLEAR);
    if (s.nacc > 0) {
        if (s.writer) s.out[s.nwords] = (unsigned)s.acc;
        ++s.nwords;
    }
    return s.nbits;
}

// ---- how a frame is cut, and what its bands can come to
GIF_FN int gif_band_rows(int w, int band_rows) {
    if (band_rows > 0) return band_rows;
    const int r = GIF_DEFAULT_BAND / w;
    return r < 1 ? 1 : r;
}
GIF_FN long gif_bands(int h, int w, int band_rows) {
    const int r = gif_band_rows(w, band_rows);
    return (h + (long)r - 1) / r;
}
// bits of a band of L indices at most: a code per index, a clear per filled dictionary, the leading clear or the code that ends the
// band, and the pending string's; 12 bits each
GIF_FN long gif_band_bits(long L) { return 12 * (L + L / GIF_FILL + 2); }
GIF_FN long gif_band_words(long L) { return (gif_band_bits(L) + 31) / 32 + 1; }
// a frame's payload around `data` bytes of LZW data: 08, a length byte per 255, 00
GIF_FN long gif_payload_bytes(long data) { return 2 + data + (data + 254) / 255; }

// ---- the stitch: byte j of a frame's LZW data, whose bands' bits (band b: words[b * wstride ...], bitoff[b + 1] - bitoff[b] of them, LSB
// first) follow each other without padding; bitoff: nb + 1 bit positions in the frame, bitoff[0] = 0.  Bits past the last are zero.
GIF_FN unsigned gif_data_byte(const unsigned* words, long wstride, const long* bitoff, int nb, long j) {
    long p = 8 * j;
    const long total = bitoff[nb];
    int lo = 0, hi = nb;                                        // the band p lies in: bitoff[lo] <= p < bitoff[lo + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (bitoff[mid] <= p) lo = mid; else hi = mid;
    }
    unsigned byte = 0;
    int got = 0;
    while (got < 8 && p < total && lo < nb) {
        const long end = bitoff[lo + 1];
        if (p >= end) {
            ++lo;
            continue;
        }
        const long q = p - bitoff[lo];
        const int take = (int)(end - p < 8 - got ? end - p : 8 - got);
        const unsigned* wd = words + lo * wstride + (q >> 5);
        const int sh = (int)(q & 31);
        unsigned v = wd[0] >> sh;
        if (sh + take > 32) v |= wd[1] << (32 - sh);
        byte |= (v & ((1u << take) - 1u)) << got;
        got += take;
        p += take;
    }
    return byte;
}
// where byte j of the data stands in the payload, and the length byte in front of the sub-block that begins at j (j a multiple of 255)
GIF_FN long gif_data_pos(long j) { return 2 + j + j / 255; }
GIF_FN unsigned gif_block_len(long data, long j) { return (unsigned)(data - j < 255 ? data - j : 255); }

// ---- changed-rectangle frames (include/ccvs_hip_output_gif_delta.h): a frame after its clip's first has two
// candidates, the full frame F and the bounding rectangle D of the indices that differ from the frame before, whose unchanged indices
// are GIF_TRANSPARENT.  Either is cut into bands of ITS rows and coded by the coder above; the shorter payload is written.
#define GIF_TRANSPARENT 255          // the palette entry no box of the median cut gets (at most 255 boxes)

struct GifRect {
    int x0, y0, rw, rh;
};
GIF_FN GifRect gif_full_rect(int h, int w) {
    GifRect r = {0, 0, w, h};
    return r;
}
// the bounding rectangle of the changed indices, whose columns span x_min .. x_max and rows y_min .. y_max; none (x_max < x_min): the
// frame's first pixel alone
GIF_FN GifRect gif_changed_rect(int x_min, int x_max, int y_min, int y_max) {
    GifRect r = {0, 0, 1, 1};
    if (x_max >= x_min) {
        r.x0 = x_min;
        r.y0 = y_min;
        r.rw = x_max - x_min + 1;
        r.rh = y_max - y_min + 1;
    }
    return r;
}
// band b of a rectangle: its first row within the rectangle and its number of rows; index i of the band is the frame's pixel
// (y0 + first row + i / rw, x0 + i % rw).  A rectangle has gif_bands(rh, rw, band_rows) bands, never more than its frame.
GIF_FN int gif_rect_band_first(const GifRect& r, int band_rows, int b) { return b * gif_band_rows(r.rw, band_rows); }
GIF_FN int gif_rect_band_count(const GifRect& r, int band_rows, int b) {
    const int rows = gif_band_rows(r.rw, band_rows), r0 = b * rows;
    return r0 + rows < r.rh ? rows : r.rh - r0;
}
GIF_FN long gif_rect_pixel(const GifRect& r, int w, int first_row, long i) {
    return (long)(r.y0 + first_row + (int)(i / r.rw)) * w + r.x0 + (int)(i % r.rw);
}
// indices of the largest band of any rectangle of an h x w frame (at least; what the bands' words are sized for).  With band_rows
// given it is the full frame's band.  With 0 a rectangle of rw <= 4096 columns has bands of (4096 / rw) rw <= 4096 indices -- more
// than the full frame's where w does not divide 4096 -- and a wider one has bands of one row.
GIF_FN long gif_rect_band_max(int h, int w, int band_rows) {
    if (band_rows > 0) return (long)(band_rows < h ? band_rows : h) * w;
    if (w > GIF_DEFAULT_BAND) return w;
    return (long)h * w < GIF_DEFAULT_BAND ? (long)h * w : GIF_DEFAULT_BAND;
}

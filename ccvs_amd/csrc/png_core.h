// What the two deflate writers share (png.hip: literals only; png_lz.hip: with LZ77 matches, section 4.24): the
// row filters and the filter launch's body, the length-limited Huffman builder, canonical codes, the bit packer, the block header
// (code-length code and run-length coded lengths) for one or two alphabets, the scan of the bands' positions, and the steps of the emit
// tile that do not depend on what a symbol is.  Everything in integers.
#pragma once
#include "common.h"

#define PNG_THREADS 256
#define PNG_WAVES (PNG_THREADS / WAVE)
#define PNG_ADLER 65521u
#define PNG_CODE_STRIDE 260          // unsigned per band: the 257 counts, then in their place the codes as (reversed code << 4) | length
#define PNG_HDR_STRIDE 128           // unsigned per band: the header's bit count, then its bits (at most 3700: see png_block_tables)
#define PNG_LZ_HDR_STRIDE 160        // the same with both alphabets in the header (at most 4498 bits)
#define PNG_DEFAULT_BAND_BYTES 32768
#define PNG_NLL 286                  // literal/length symbols of a block with matches
#define PNG_ND 30                    // distance symbols

struct PngArgs {
    const uint8_t* rgb;
    long frame_stride;
    int n, h, w, filter, band_rows, nb;   // nb: bands per frame
    long T, rowb;                         // bands in all; bytes of a filtered row: 3 w + 1
    uint8_t* stream;
    long capacity;
    long* offsets;
    long* boff;                           // [T] where a band's block starts in the stream
    long* sizes;                          // [T] bytes of the band's block with what follows it up to the next band
    unsigned* adler_part;                 // [T][2] the band's sum of bytes and weighted sum, mod 65521
    unsigned* adler;                      // [n]
    unsigned* codes;                      // [T][PNG_CODE_STRIDE]
    unsigned* hdr;                        // [T][PNG_HDR_STRIDE], or PNG_LZ_HDR_STRIDE with matches
    uint8_t* filt;                        // [n][h][rowb]
};

__device__ __forceinline__ int png_paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// byte i of a row under filter `type`; prev: the row above, null for row 0
__device__ __forceinline__ int png_filtered(const uint8_t* cur, const uint8_t* prev, int i, int type) {
    const int x = cur[i];
    if (type == 0) return x;
    const int a = i >= 3 ? cur[i - 3] : 0;
    if (type == 1) return (x - a) & 255;
    const int b = prev ? prev[i] : 0;
    if (type == 2) return (x - b) & 255;
    if (type == 3) return (x - ((a + b) >> 1)) & 255;
    const int c = (prev && i >= 3) ? prev[i - 3] : 0;
    return (x - png_paeth(a, b, c)) & 255;
}
__device__ __forceinline__ unsigned long long png_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// ---- filter: a workgroup of PNG_THREADS per band, a wave per row
__device__ __forceinline__ void png_filter_body(const PngArgs& a) {
    __shared__ unsigned s_hist[257];
    __shared__ unsigned long long s_ad[2];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int rb = 3 * a.w;
    for (long band = blockIdx.x; band < a.T; band += gridDim.x) {
        const long f = band / a.nb;
        const int r0 = (int)(band % a.nb) * a.band_rows;
        const int r1 = r0 + a.band_rows < a.h ? r0 + a.band_rows : a.h;
        const long L = (long)(r1 - r0) * a.rowb;
        for (int i = tid; i < 257; i += PNG_THREADS) s_hist[i] = i == 256 ? 1u : 0u;   // (end-of-block is emitted once)
        if (tid < 2) s_ad[tid] = 0;
        __syncthreads();
        for (int row = r0 + wave; row < r1; row += PNG_WAVES) {
            const uint8_t* cur = a.rgb + f * a.frame_stride + (long)row * rb;
            const uint8_t* prev = row ? cur - rb : nullptr;
            int type = a.filter;
            if (type < 0) {
                unsigned s[5] = {0, 0, 0, 0, 0};
                for (int i = lane; i < rb; i += WAVE) {
                    const int x = cur[i], p = i >= 3 ? cur[i - 3] : 0, b = prev ? prev[i] : 0, c = (prev && i >= 3) ? prev[i - 3] : 0;
                    const int v[5] = {x, (x - p) & 255, (x - b) & 255, (x - ((p + b) >> 1)) & 255, (x - png_paeth(p, b, c)) & 255};
#pragma unroll
                    for (int t = 0; t < 5; ++t) s[t] += v[t] < 128 ? v[t] : 256 - v[t];
                }
                unsigned best = 0;
#pragma unroll
                for (int t = 0; t < 5; ++t) {
                    const unsigned tot = (unsigned)png_wave_sum(s[t]);
                    if (t == 0 || tot < best) {
                        best = tot;
                        type = t;
                    }
                }
            }
            uint8_t* out = a.filt + (f * a.h + row) * a.rowb;
            const long pos0 = (long)(row - r0) * a.rowb;              // the type byte's place in the band
            unsigned long long sa = 0, sb = 0;
            if (lane == 0) {
                out[0] = (uint8_t)type;
                atomicAdd(&s_hist[type], 1u);
                sa = type;
                sb = (unsigned long long)((L - pos0) % PNG_ADLER) * type;
            }
            for (int i = lane; i < rb; i += WAVE) {
                const int v = png_filtered(cur, prev, i, type);
                out[1 + i] = (uint8_t)v;
                atomicAdd(&s_hist[v], 1u);
                sa += v;
                sb += (unsigned long long)((L - (pos0 + 1 + i)) % PNG_ADLER) * v;   // < 2^24 each, at most 3072 of them per lane
            }
            sa = png_wave_sum(sa);
            sb = png_wave_sum(sb);
            if (lane == 0) {
                atomicAdd(&s_ad[0], sa % PNG_ADLER);
                atomicAdd(&s_ad[1], sb % PNG_ADLER);
            }
        }
        __syncthreads();
        for (int i = tid; i < 257; i += PNG_THREADS) a.codes[band * PNG_CODE_STRIDE + i] = s_hist[i];
        if (tid < 2) a.adler_part[band * 2 + tid] = (unsigned)(s_ad[tid] % PNG_ADLER);
        __syncthreads();   // the LDS arrays are the next band's too
    }
}

// ---- tables: a wave per band, everything in LDS
#define PNG_TBL_THREADS 64
#define PNG_MAXD 64                  // a band has fewer than 2^31 bytes, so no Huffman tree of its counts is deeper than 46
#define PNG_NSYM 288                 // room for the largest alphabet (286)
#define PNG_NSEQ 320                 // room for the code lengths of a header: up to 286 + 30

struct PngTableLds {
    unsigned cnt[PNG_NSYM], freq[PNG_NSYM];
    int depth[PNG_NSYM], head[PNG_NSYM], bits[PNG_MAXD + 1], before[17], first[17];
    uint8_t len[PNG_NSYM];
};

// Code lengths of at most `maxlen` bits for the n symbols counted in t.cnt, into t.len: a complete code over the symbols with a count
// (where fewer than two have one, the lowest symbols without are counted once).  The tree is jpeg_tables_kernel's (jpeg.hip) without
// libjpeg's reserved symbol: the two smallest nonzero counts are merged, among equals the larger symbol first, the sum stays with the
// first of the two; depths beyond maxlen are brought down by T.81 K.2, which keeps the Kraft sum at 1; the lengths, ascending, go to
// the symbols by descending count, then ascending symbol.  One wave.
__device__ void png_code_lengths(PngTableLds& t, int n, int maxlen, int lane) {
    if (lane == 0) {
        int used = 0;
        for (int i = 0; i < n; ++i) used += t.cnt[i] != 0;
        for (int i = 0; i < n && used < 2; ++i)
            if (t.cnt[i] == 0) {
                t.cnt[i] = 1;
                ++used;
            }
    }
    __syncthreads();
    for (int i = lane; i < n; i += PNG_TBL_THREADS) {
        t.freq[i] = t.cnt[i];
        t.depth[i] = 0;
        t.head[i] = i;
        t.len[i] = 0;
    }
    for (int i = lane; i <= PNG_MAXD; i += PNG_TBL_THREADS) t.bits[i] = 0;
    __syncthreads();
    for (;;) {
        int c[2] = {-1, -1};
        for (int r = 0; r < 2; ++r) {
            unsigned long long key = ~0ull;
            for (int i = lane; i < n; i += PNG_TBL_THREADS) {
                const unsigned f = t.freq[i];
                const unsigned long long k = ((unsigned long long)f << 16) | (unsigned)(0xFFFF - i);
                if (f && i != c[0] && k < key) key = k;
            }
            for (int m = PNG_TBL_THREADS / 2; m > 0; m >>= 1) {
                const unsigned long long o = __shfl_xor(key, m, PNG_TBL_THREADS);
                key = o < key ? o : key;
            }
            if (key != ~0ull) c[r] = 0xFFFF - (int)(key & 0xFFFFu);
        }
        if (c[1] < 0) break;                               // (the same in every lane)
        __syncthreads();
        if (lane == 0) {
            t.freq[c[0]] += t.freq[c[1]];
            t.freq[c[1]] = 0;
        }
        for (int i = lane; i < n; i += PNG_TBL_THREADS) {
            const int h = t.head[i];
            if (h == c[0] || h == c[1]) {
                ++t.depth[i];
                t.head[i] = c[0];
            }
        }
        __syncthreads();
    }
    for (int i = lane; i < n; i += PNG_TBL_THREADS) {
        const int d = t.depth[i];
        if (d) atomicAdd(&t.bits[d < PNG_MAXD ? d : PNG_MAXD], 1);
    }
    __syncthreads();
    if (lane == 0) {
        for (int i = PNG_MAXD; i > maxlen; --i)
            while (t.bits[i] > 0) {
                int j = i - 2;
                while (j > 0 && t.bits[j] == 0) --j;
                t.bits[i] -= 2;
                t.bits[i - 1] += 1;
                t.bits[j + 1] += 2;
                t.bits[j] -= 1;
            }
        int k = 0;
        for (int len = 1; len <= maxlen + 1; ++len) {      // before[len]: the codes shorter than len
            t.before[len] = k;
            k += len <= maxlen ? t.bits[len] : 0;
        }
    }
    __syncthreads();
    for (int j = lane; j < n; j += PNG_TBL_THREADS) {
        const unsigned cj = t.cnt[j];
        if (!cj) continue;
        int p = 0;
        for (int k = 0; k < n; ++k) {
            const unsigned ck = t.cnt[k];
            p += ck > cj || (ck == cj && k < j);
        }
        int len = 1;
        while (len < maxlen && p >= t.before[len + 1]) ++len;
        t.len[j] = (uint8_t)len;
    }
    __syncthreads();
}

// Canonical codes (RFC 1951 3.2.2) of t.len, bit-reversed for deflate's LSB-first packing: code[j] = (reversed code << 4) | length, 0
// for a symbol without a code.  One wave.
__device__ void png_codes(PngTableLds& t, int n, int maxlen, unsigned* code, int lane) {
    if (lane == 0) {
        int count[17];
        for (int l = 0; l <= maxlen; ++l) count[l] = 0;
        for (int i = 0; i < n; ++i) ++count[t.len[i]];
        count[0] = 0;
        int c = 0;
        for (int l = 1; l <= maxlen; ++l) {
            c = (c + count[l - 1]) << 1;
            t.first[l] = c;
        }
    }
    __syncthreads();
    for (int j = lane; j < n; j += PNG_TBL_THREADS) {
        const int l = t.len[j];
        unsigned e = 0;
        if (l) {
            int c = t.first[l];
            for (int k = 0; k < j; ++k) c += t.len[k] == l;
            e = ((__brev((unsigned)c) >> (32 - l)) << 4) | (unsigned)l;
        }
        code[j] = e;
    }
    __syncthreads();
}

__device__ __forceinline__ void png_put(unsigned* words, int& nbits, unsigned value, int count) {   // LSB-first; words zeroed before
    const int w = nbits >> 5, sh = nbits & 31;
    words[w] |= value << sh;
    if (sh + count > 32) words[w + 1] |= value >> (32 - sh);
    nbits += count;
}

// extra bits behind a length symbol (257 .. 285) and a distance symbol (RFC 1951 3.2.5); literals and end-of-block have none
__device__ __forceinline__ int png_ll_extra(int sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }
__device__ __forceinline__ int png_d_extra(int sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }

struct PngHeaderLds {
    unsigned hdr[PNG_LZ_HDR_STRIDE];     // the header's bit count, then its bits
    unsigned clcode[19];
    uint8_t seq[PNG_NSEQ], rsym[PNG_NSEQ], rext[PNG_NSEQ], cllen[19];
    int nr, nseq, hlit, hdist;
};

// One dynamic block's tables, by one wave: from the counts of its literal/length alphabet (cnt_ll[nll]; 257 symbols: a block without
// matches, or PNG_NLL) and of its distance alphabet (cnt_d[PNG_ND]; null: no distance is used, and the header carries two distance
// codes of length 1) the codes into code_ll / code_d as (reversed code << 4) | length, and the header into H.hdr (`hdr_words` of them
// are cleared first): BFINAL, BTYPE = 2, HLIT and HDIST trimmed, HCLEN, the code-length code, the lengths of both alphabets run-length
// coded as one sequence.  Returns the block's bits: header, every counted symbol's code and extra bits.  All arrays are LDS.
// The header is at most 3 + 5 + 5 + 4 + 19 x 3 + (nll + 2 or PNG_ND) x (7 + 7) bits: 3700 without matches, 4498 with.
__device__ unsigned long long png_block_tables(PngTableLds& t, PngHeaderLds& H, const unsigned* cnt_ll, int nll, const unsigned* cnt_d,
                                               unsigned* code_ll, unsigned* code_d, bool last, int hdr_words, int lane) {
    for (int i = lane; i < nll; i += PNG_TBL_THREADS) t.cnt[i] = cnt_ll[i];
    __syncthreads();
    png_code_lengths(t, nll, 15, lane);
    png_codes(t, nll, 15, code_ll, lane);
    unsigned long long bits = 0;
    for (int i = lane; i < nll; i += PNG_TBL_THREADS) {
        bits += (unsigned long long)cnt_ll[i] * (t.len[i] + png_ll_extra(i));
        H.seq[i] = t.len[i];
    }
    __syncthreads();
    if (lane == 0) {
        int hlit = 257;
        for (int i = 257; i < nll; ++i)
            if (H.seq[i]) hlit = i + 1;
        H.hlit = hlit;
        if (!cnt_d) {
            H.seq[hlit] = H.seq[hlit + 1] = 1;
            H.hdist = 2;
        }
    }
    __syncthreads();
    if (cnt_d) {
        for (int i = lane; i < PNG_ND; i += PNG_TBL_THREADS) t.cnt[i] = cnt_d[i];
        __syncthreads();
        png_code_lengths(t, PNG_ND, 15, lane);
        png_codes(t, PNG_ND, 15, code_d, lane);
        if (lane < PNG_ND) {
            bits += (unsigned long long)cnt_d[lane] * (t.len[lane] + png_d_extra(lane));
            H.seq[H.hlit + lane] = t.len[lane];
        }
        __syncthreads();
        if (lane == 0) {
            int hdist = 1;
            for (int i = 1; i < PNG_ND; ++i)
                if (t.len[i]) hdist = i + 1;
            H.hdist = hdist;
        }
        __syncthreads();
    }
    bits = png_wave_sum(bits);
    if (lane == 0) {
        const int nseq = H.hlit + H.hdist;
        // zlib's send_tree on the lengths as one sequence: runs of a nonzero length as the length, then 16 (3 .. 6 more); runs of
        // zeros as 17 (3 .. 10) or 18 (11 .. 138); shorter runs as they are
        int nr = 0, prev = -1, next = H.seq[0], count = 0, maxc = next == 0 ? 138 : 7, minc = next == 0 ? 3 : 4;
        for (int k = 0; k < nseq; ++k) {
            const int cur = next;
            next = k + 1 < nseq ? H.seq[k + 1] : -1;
            if (++count < maxc && cur == next) continue;
            if (count < minc) {
                for (; count > 0; --count) {
                    H.rsym[nr] = (uint8_t)cur;
                    H.rext[nr++] = 0;
                }
            } else if (cur != 0) {
                if (cur != prev) {
                    H.rsym[nr] = (uint8_t)cur;
                    H.rext[nr++] = 0;
                    --count;
                }
                H.rsym[nr] = 16;
                H.rext[nr++] = (uint8_t)(count - 3);
            } else if (count <= 10) {
                H.rsym[nr] = 17;
                H.rext[nr++] = (uint8_t)(count - 3);
            } else {
                H.rsym[nr] = 18;
                H.rext[nr++] = (uint8_t)(count - 11);
            }
            count = 0;
            prev = cur;
            if (next == 0) maxc = 138, minc = 3;
            else if (cur == next) maxc = 6, minc = 3;
            else maxc = 7, minc = 4;
        }
        H.nr = nr;
        for (int i = 0; i < 19; ++i) t.cnt[i] = 0;
        for (int i = 0; i < nr; ++i) ++t.cnt[H.rsym[i]];
    }
    __syncthreads();
    png_code_lengths(t, 19, 7, lane);
    png_codes(t, 19, 7, H.clcode, lane);
    for (int i = lane; i < hdr_words; i += PNG_TBL_THREADS) H.hdr[i] = 0;
    if (lane < 19) H.cllen[lane] = t.len[lane];
    __syncthreads();
    if (lane == 0) {
        const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        int ncl = 19;
        while (ncl > 4 && H.cllen[order[ncl - 1]] == 0) --ncl;
        unsigned* w = H.hdr + 1;
        int nbits = 0;
        png_put(w, nbits, last ? 1u : 0u, 1);                  // BFINAL
        png_put(w, nbits, 2u, 2);                              // BTYPE: dynamic Huffman codes
        png_put(w, nbits, (unsigned)(H.hlit - 257), 5);        // HLIT
        png_put(w, nbits, (unsigned)(H.hdist - 1), 5);         // HDIST
        png_put(w, nbits, (unsigned)(ncl - 4), 4);             // HCLEN
        for (int i = 0; i < ncl; ++i) png_put(w, nbits, H.cllen[order[i]], 3);
        for (int i = 0; i < H.nr; ++i) {
            const int sym = H.rsym[i];
            const unsigned e = H.clcode[sym];
            png_put(w, nbits, e >> 4, (int)(e & 15));
            if (sym >= 16) png_put(w, nbits, H.rext[i], sym == 16 ? 2 : (sym == 17 ? 3 : 7));
        }
        H.hdr[0] = (unsigned)nbits;
    }
    __syncthreads();
    return bits + H.hdr[0];
}

// bytes of a band's block of `total` bits with what follows it: the last band is padded to a byte; the others are followed by 000, the
// padding and 00 00 FF FF
__device__ __forceinline__ long png_band_bytes(unsigned long long total, bool last) {
    return last ? (long)((total + 7) >> 3) : (long)((total + 3 + 7) >> 3) + 4;
}

// ---- scan: one workgroup of PNG_THREADS.  A lane sums a run of consecutive bands, the runs' sums are scanned through LDS, the lane
// walks its run again (jpeg_scan_kernel's form).  A frame's stream is 2 bytes of header, its bands, 4 bytes of Adler-32.
__device__ __forceinline__ void png_scan_body(const PngArgs& a) {
    __shared__ long s_sum[PNG_THREADS];
    const int tid = threadIdx.x;
    const long chunk = (a.T + PNG_THREADS - 1) / PNG_THREADS;
    const long i0 = tid * chunk < a.T ? tid * chunk : a.T;
    const long i1 = i0 + chunk < a.T ? i0 + chunk : a.T;
    long sum = 0;
    for (long i = i0; i < i1; ++i) sum += a.sizes[i];
    s_sum[tid] = sum;
    __syncthreads();
    long run = 0, total = 0;
    for (int j = 0; j < PNG_THREADS; ++j) {
        const long c = s_sum[j];
        run += j < tid ? c : 0;
        total += c;
    }
    for (long i = i0; i < i1; ++i) {
        const long f = i / a.nb;
        a.boff[i] = run + 6 * f + 2;
        if (i % a.nb == 0) a.offsets[f] = run + 6 * f;
        run += a.sizes[i];
    }
    if (tid == 0) a.offsets[a.n] = total + 6L * a.n;
    // Adler-32: the bands' (sum, weighted sum, length) combined in order
    for (int f = tid; f < a.n; f += PNG_THREADS) {
        unsigned long long A = 1, B = 0;
        for (int b = 0; b < a.nb; ++b) {
            const int r0 = b * a.band_rows;
            const int r1 = r0 + a.band_rows < a.h ? r0 + a.band_rows : a.h;
            const unsigned long long len = (unsigned long long)((long)(r1 - r0) * a.rowb) % PNG_ADLER;
            const unsigned* p = a.adler_part + ((long)f * a.nb + b) * 2;
            B = (B + len * A + p[1]) % PNG_ADLER;
            A = (A + p[0]) % PNG_ADLER;
        }
        a.adler[f] = (unsigned)((B << 16) | A);
    }
}

// ---- emit: a workgroup of PNG_THREADS per band.  The band's bits go through an LDS buffer in tiles: a lane takes PNG_SYMS
// consecutive positions, the lanes' bit counts are scanned, every lane ORs its bits into the buffer at its bit position, the tile's
// whole bytes are copied out and the bits left over (fewer than 8) open the next tile.  Every byte below offsets[n] is written, none is
// read.  The steps that do not depend on what a position's bits are:
#define PNG_SYMS 8
#define PNG_TILE (PNG_THREADS * PNG_SYMS)

__device__ __forceinline__ void png_store(const PngArgs& a, long pos, unsigned byte) {
    if (pos < a.capacity) a.stream[pos] = (uint8_t)byte;
}

// the bits of the lanes before this one in the tile and of the whole tile, from every lane's own count
__device__ __forceinline__ void png_tile_scan(int mine, int* s_wsum, int& before, int& total) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    int v = mine;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const int o = __shfl_up(v, d, WAVE);
        if (lane >= d) v += o;
    }
    if (lane == WAVE - 1) s_wsum[wave] = v;
    __syncthreads();
    before = v - mine;
    total = 0;
#pragma unroll
    for (int k = 0; k < PNG_WAVES; ++k) {
        before += k < wave ? s_wsum[k] : 0;
        total += s_wsum[k];
    }
}

// 32 bits (or the last ones) of a lane at bit p of the buffer
__device__ __forceinline__ void png_tile_or(unsigned* s_buf, int p, unsigned lo) {
    const int w = p >> 5, sh = p & 31;
    atomicOr(&s_buf[w], lo << sh);
    if (sh && (lo >> (32 - sh))) atomicOr(&s_buf[w + 1], lo >> (32 - sh));
}

// the tile's whole bytes out; the rest opens the next tile (the first `words` words of the buffer are cleared)
__device__ __forceinline__ void png_tile_out(const PngArgs& a, unsigned* s_buf, int words, long& pos, int& tb) {
    const int tid = threadIdx.x;
    const int full = tb >> 3;
    for (int i = tid; i < full; i += PNG_THREADS) png_store(a, pos + i, (s_buf[i >> 2] >> ((i & 3) * 8)) & 255u);
    const unsigned carry = (s_buf[full >> 2] >> ((full & 3) * 8)) & 255u;
    __syncthreads();
    for (int i = tid; i < words; i += PNG_THREADS) s_buf[i] = i == 0 ? carry : 0u;
    pos += full;
    tb &= 7;
    __syncthreads();
}

// what follows a band's last tile (one lane): the last bits, then the Adler-32 or the empty stored block
__device__ __forceinline__ void png_band_end(const PngArgs& a, unsigned carry, int tb, long pos, bool last, long f) {
    if (last) {
        if (tb) png_store(a, pos++, carry);
        const unsigned ad = a.adler[f];
        for (int k = 0; k < 4; ++k) png_store(a, pos++, (ad >> (24 - 8 * k)) & 255u);
    } else {
        png_store(a, pos++, carry);                // the last bits, then 000 of the stored block's header and the padding
        if (tb + 3 > 8) png_store(a, pos++, 0u);
        png_store(a, pos++, 0x00);                 // LEN = 0, NLEN = 0xFFFF
        png_store(a, pos++, 0x00);
        png_store(a, pos++, 0xFF);
        png_store(a, pos++, 0xFF);
    }
}

// ---- host
static inline int png_band_rows(int w, int band_rows) {
    if (band_rows > 0) return band_rows;
    const int r = PNG_DEFAULT_BAND_BYTES / (3 * w + 1);
    return r < 1 ? 1 : r;
}
static inline bool png_shape_ok(int n, int h, int w, int band_rows) {
    if (!(n >= 1 && h >= 1 && h <= 65535 && w >= 1 && w <= 65535 && band_rows >= 0)) return false;
    const long rows = png_band_rows(w, band_rows) < h ? png_band_rows(w, band_rows) : h;
    return rows * (3L * w + 1) < (1L << 31);
}
static inline long png_bands(int h, int w, int band_rows) {
    const int r = png_band_rows(w, band_rows);
    return (h + (long)r - 1) / r;
}
static inline size_t png_align8(size_t v) { return (v + 7) & ~(size_t)7; }

// the argument checks of both encoders, before any launch
#define PNG_REQUIRE_ARGS(who)                                                                                                                 \
    do {                                                                                                                                      \
        CCVS_REQUIRE(n >= 1, "%s: no frames (n = %d)", who, n);                                                                              \
        CCVS_REQUIRE(h >= 1 && h <= 65535 && w >= 1 && w <= 65535, "%s: frame size %d x %d outside 1 .. 65535", who, h, w);                  \
        CCVS_REQUIRE(filter >= -1 && filter <= 4, "%s: filter %d is none of -1 (per row), 0 .. 4 (None, Sub, Up, Average, Paeth)", who, filter); \
        CCVS_REQUIRE(band_rows >= 0, "%s: band_rows %d is negative", who, band_rows);                                                        \
        CCVS_REQUIRE(png_shape_ok(n, h, w, band_rows), "%s: band_rows %d makes a band of 2^31 filtered bytes or more", who, band_rows);      \
        CCVS_REQUIRE(capacity >= 0, "%s: negative capacity", who);                                                                           \
        CCVS_REQUIRE(frame_stride >= 3L * w * h, "%s: frame stride %ld is less than the frame's %ld bytes", who, frame_stride, 3L * w * h);  \
        CCVS_REQUIRE(rgb && offsets && workspace && (stream || capacity == 0), "%s: null frames, stream, offsets or workspace", who);        \
    } while (0)

// the arguments' part that both encoders fill alike; `p` walks the workspace: long boff[T], sizes[T]; unsigned adler_part[T][2],
// codes[T][260], hdr[T][hdr_stride], adler[n]; the filtered bytes
static inline char* png_fill_args(PngArgs& a, const uint8_t* rgb, long frame_stride, int n, int h, int w, int filter, int band_rows, uint8_t* stream,
                                  long capacity, long* offsets, void* workspace, int hdr_stride) {
    a.rgb = rgb; a.frame_stride = frame_stride;
    a.n = n; a.h = h; a.w = w; a.filter = filter;
    a.band_rows = png_band_rows(w, band_rows);
    a.nb = (int)png_bands(h, w, band_rows);
    a.T = (long)n * a.nb;
    a.rowb = 3L * w + 1;
    a.stream = stream; a.capacity = capacity; a.offsets = offsets;
    char* p = (char*)workspace;
    a.boff = (long*)p;                  p += 8 * (size_t)a.T;
    a.sizes = (long*)p;                 p += 8 * (size_t)a.T;
    a.adler_part = (unsigned*)p;        p += 8 * (size_t)a.T;
    a.codes = (unsigned*)p;             p += 4 * PNG_CODE_STRIDE * (size_t)a.T;
    a.hdr = (unsigned*)p;               p += 4 * (size_t)hdr_stride * (size_t)a.T;
    a.adler = (unsigned*)p;             p += png_align8(4 * (size_t)n);
    a.filt = (uint8_t*)p;               p += png_align8((size_t)n * h * (3 * (size_t)w + 1));
    return p;
}
static inline size_t png_workspace_bytes(int n, int h, int w, int band_rows, int hdr_stride) {
    const size_t T = (size_t)n * (size_t)png_bands(h, w, band_rows);
    return T * (8 + 8 + 8 + 4 * PNG_CODE_STRIDE + 4 * (size_t)hdr_stride) + png_align8(4 * (size_t)n) + png_align8((size_t)n * h * (3 * (size_t)w + 1));
}

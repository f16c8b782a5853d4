// The lossless output stage (include/ccvs_hip_output_lossless.h): uint8 RGB frames -> PNG-filtered rows ->
// Huffman-only deflate with dynamic tables, one complete zlib stream per frame.  A frame is cut into bands of rows; a band is one
// deflate block, and the empty stored block behind every band but the last brings the next one to a byte boundary (the pigz /
// sync-flush form), so the bands are coded independently.  Four launches, all in integers:
//   filter   per band: choose and apply every row's filter, store the filtered bytes, count them, sum the band's Adler-32 terms;
//   tables   per band: the literal/length code from the counts, the code-length code, the block header as bits, the block's size;
//   scan     the bands' positions in the stream, the frames' offsets and their Adler-32 values;
//   emit     per band: header bits, the bytes' codes and end-of-block, packed LSB-first through LDS, then the stored block or the
//            Adler-32.
// tests/apng_ref.py states the same algorithm in numpy; the kernels give its bytes.
#include "common.h"

#define PNG_THREADS 256
#define PNG_WAVES (PNG_THREADS / WAVE)
#define PNG_ADLER 65521u
#define PNG_CODE_STRIDE 260          // unsigned per band: the 257 counts, then in their place the codes as (reversed code << 4) | length
#define PNG_HDR_STRIDE 128           // unsigned per band: the header's bit count, then its bits (at most 3700: see png_tables_kernel)
#define PNG_DEFAULT_BAND_BYTES 32768

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
    unsigned* hdr;                        // [T][PNG_HDR_STRIDE]
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

// ---- filter: a workgroup per band, a wave per row
__global__ __launch_bounds__(PNG_THREADS) void png_filter_kernel(PngArgs a) {
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
#define PNG_NLEN 259                 // 257 literal/length code lengths, then the two distance code lengths

struct PngTableLds {
    unsigned cnt[257], freq[257];
    int depth[257], head[257], bits[PNG_MAXD + 1], before[17], first[17];
    uint8_t len[257];
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

// The block header is at most 3 + 5 + 5 + 4 + 19 x 3 + 259 x (7 + 7) = 3700 bits.
__global__ __launch_bounds__(PNG_TBL_THREADS) void png_tables_kernel(PngArgs a) {
    __shared__ PngTableLds t;
    __shared__ unsigned s_cnt[257], s_code[257], s_clcode[19], s_hdr[PNG_HDR_STRIDE];
    __shared__ uint8_t s_seq[PNG_NLEN], s_rsym[PNG_NLEN], s_rext[PNG_NLEN], s_cllen[19];
    __shared__ int s_nr;
    const int lane = threadIdx.x;
    for (long band = blockIdx.x; band < a.T; band += gridDim.x) {
        unsigned* codes = a.codes + band * PNG_CODE_STRIDE;
        for (int i = lane; i < 257; i += PNG_TBL_THREADS) s_cnt[i] = t.cnt[i] = codes[i];
        __syncthreads();
        png_code_lengths(t, 257, 15, lane);
        png_codes(t, 257, 15, s_code, lane);
        unsigned long long bits = 0;
        for (int i = lane; i < 257; i += PNG_TBL_THREADS) {
            bits += (unsigned long long)s_cnt[i] * t.len[i];
            codes[i] = s_code[i];
            s_seq[i] = t.len[i];
        }
        bits = png_wave_sum(bits);
        __syncthreads();
        if (lane == 0) {
            s_seq[257] = s_seq[258] = 1;
            // zlib's send_tree on the 259 lengths as one sequence: runs of a nonzero length as the length, then 16 (3 .. 6 more);
            // runs of zeros as 17 (3 .. 10) or 18 (11 .. 138); shorter runs as they are
            int nr = 0, prev = -1, next = s_seq[0], count = 0, maxc = next == 0 ? 138 : 7, minc = next == 0 ? 3 : 4;
            for (int k = 0; k < PNG_NLEN; ++k) {
                const int cur = next;
                next = k + 1 < PNG_NLEN ? s_seq[k + 1] : -1;
                if (++count < maxc && cur == next) continue;
                if (count < minc) {
                    for (; count > 0; --count) {
                        s_rsym[nr] = (uint8_t)cur;
                        s_rext[nr++] = 0;
                    }
                } else if (cur != 0) {
                    if (cur != prev) {
                        s_rsym[nr] = (uint8_t)cur;
                        s_rext[nr++] = 0;
                        --count;
                    }
                    s_rsym[nr] = 16;
                    s_rext[nr++] = (uint8_t)(count - 3);
                } else if (count <= 10) {
                    s_rsym[nr] = 17;
                    s_rext[nr++] = (uint8_t)(count - 3);
                } else {
                    s_rsym[nr] = 18;
                    s_rext[nr++] = (uint8_t)(count - 11);
                }
                count = 0;
                prev = cur;
                if (next == 0) maxc = 138, minc = 3;
                else if (cur == next) maxc = 6, minc = 3;
                else maxc = 7, minc = 4;
            }
            s_nr = nr;
            for (int i = 0; i < 19; ++i) t.cnt[i] = 0;
            for (int i = 0; i < nr; ++i) ++t.cnt[s_rsym[i]];
        }
        __syncthreads();
        png_code_lengths(t, 19, 7, lane);
        png_codes(t, 19, 7, s_clcode, lane);
        for (int i = lane; i < PNG_HDR_STRIDE; i += PNG_TBL_THREADS) s_hdr[i] = 0;
        if (lane < 19) s_cllen[lane] = t.len[lane];
        __syncthreads();
        if (lane == 0) {
            const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            const bool last = band % a.nb == a.nb - 1;
            int ncl = 19;
            while (ncl > 4 && s_cllen[order[ncl - 1]] == 0) --ncl;
            unsigned* w = s_hdr + 1;
            int nbits = 0;
            png_put(w, nbits, last ? 1u : 0u, 1);          // BFINAL
            png_put(w, nbits, 2u, 2);                      // BTYPE: dynamic Huffman codes
            png_put(w, nbits, 0u, 5);                      // HLIT: 257 literal/length codes
            png_put(w, nbits, 1u, 5);                      // HDIST: 2 distance codes
            png_put(w, nbits, (unsigned)(ncl - 4), 4);     // HCLEN
            for (int i = 0; i < ncl; ++i) png_put(w, nbits, s_cllen[order[i]], 3);
            for (int i = 0; i < s_nr; ++i) {
                const int sym = s_rsym[i];
                const unsigned e = s_clcode[sym];
                png_put(w, nbits, e >> 4, (int)(e & 15));
                if (sym >= 16) png_put(w, nbits, s_rext[i], sym == 16 ? 2 : (sym == 17 ? 3 : 7));
            }
            s_hdr[0] = (unsigned)nbits;
            const unsigned long long total = bits + (unsigned long long)nbits;
            // the last band is padded to a byte; the others are followed by 000, the padding and 00 00 FF FF
            a.sizes[band] = last ? (long)((total + 7) >> 3) : (long)((total + 3 + 7) >> 3) + 4;
        }
        __syncthreads();
        for (int i = lane; i < PNG_HDR_STRIDE; i += PNG_TBL_THREADS) a.hdr[band * PNG_HDR_STRIDE + i] = s_hdr[i];
        __syncthreads();
    }
}

// ---- scan: one workgroup.  A lane sums a run of consecutive bands, the runs' sums are scanned through LDS, the lane walks its run
// again (jpeg_scan_kernel's form).  A frame's stream is 2 bytes of header, its bands, 4 bytes of Adler-32.
__global__ __launch_bounds__(PNG_THREADS) void png_scan_kernel(PngArgs a) {
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

// ---- emit: a workgroup per band.  The band's bits go through an LDS buffer in tiles: a lane takes PNG_SYMS consecutive symbols, the
// lanes' bit counts are scanned, every lane ORs its codes into the buffer at its bit position, the tile's whole bytes are copied out
// and the bits left over (fewer than 8) open the next tile.  Every byte below offsets[n] is written, none is read.
#define PNG_SYMS 8
#define PNG_TILE (PNG_THREADS * PNG_SYMS)
#define PNG_BUF_WORDS ((7 + PNG_TILE * 15 + 31) / 32 + 2)

__device__ __forceinline__ void png_store(const PngArgs& a, long pos, unsigned byte) {
    if (pos < a.capacity) a.stream[pos] = (uint8_t)byte;
}

__global__ __launch_bounds__(PNG_THREADS) void png_emit_kernel(PngArgs a) {
    __shared__ unsigned s_buf[PNG_BUF_WORDS], s_code[257];
    __shared__ int s_wsum[PNG_WAVES];
    static_assert(PNG_BUF_WORDS >= PNG_HDR_STRIDE, "the block header is the first tile");
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    for (long band = blockIdx.x; band < a.T; band += gridDim.x) {
        const long f = band / a.nb;
        const int b = (int)(band % a.nb);
        const int r0 = b * a.band_rows;
        const int r1 = r0 + a.band_rows < a.h ? r0 + a.band_rows : a.h;
        const long L = (long)(r1 - r0) * a.rowb;
        const bool last = b == a.nb - 1;
        const uint8_t* src = a.filt + (f * a.h + r0) * a.rowb;
        const unsigned* hdr = a.hdr + band * PNG_HDR_STRIDE;
        long pos = a.boff[band];
        for (int i = tid; i < 257; i += PNG_THREADS) s_code[i] = a.codes[band * PNG_CODE_STRIDE + i];
        if (b == 0 && tid == 0) {                          // zlib's header: deflate with a 32 KiB window, no dictionary, fastest level
            png_store(a, pos - 2, 0x78);
            png_store(a, pos - 1, 0x01);
        }
        // the first tile is the header, already packed
        int tb = (int)hdr[0];                              // bits in the buffer
        for (int i = tid; i < PNG_BUF_WORDS; i += PNG_THREADS) s_buf[i] = i < (tb + 31) / 32 ? hdr[1 + i] : 0u;
        __syncthreads();
        for (long t0 = -PNG_TILE; t0 <= L; t0 += PNG_TILE) {
            if (t0 >= 0) {
                // symbols t0 + PNG_SYMS tid ... of the band; symbol L is end-of-block
                const long j0 = t0 + (long)tid * PNG_SYMS;
                unsigned e[PNG_SYMS];
                int mine = 0;
#pragma unroll
                for (int k = 0; k < PNG_SYMS; ++k) {
                    const long j = j0 + k;
                    e[k] = j < L ? s_code[src[j]] : (j == L ? s_code[256] : 0u);
                    mine += (int)(e[k] & 15);
                }
                int v = mine;
#pragma unroll
                for (int d = 1; d < WAVE; d <<= 1) {
                    const int o = __shfl_up(v, d, WAVE);
                    if (lane >= d) v += o;
                }
                if (lane == WAVE - 1) s_wsum[wave] = v;
                __syncthreads();
                int before = 0, total = 0;
#pragma unroll
                for (int k = 0; k < PNG_WAVES; ++k) {
                    before += k < wave ? s_wsum[k] : 0;
                    total += s_wsum[k];
                }
                int p = tb + before + v - mine;
                unsigned long long acc = 0;
                int nacc = 0;
#pragma unroll
                for (int k = 0; k <= PNG_SYMS; ++k) {
                    if (k < PNG_SYMS) {
                        acc |= (unsigned long long)(e[k] >> 4) << nacc;
                        nacc += (int)(e[k] & 15);
                    }
                    if (nacc >= 32 || (k == PNG_SYMS && nacc > 0)) {
                        const unsigned lo = (unsigned)acc;
                        const int w = p >> 5, sh = p & 31;
                        atomicOr(&s_buf[w], lo << sh);
                        if (sh && (lo >> (32 - sh))) atomicOr(&s_buf[w + 1], lo >> (32 - sh));
                        p += 32;
                        acc >>= 32;
                        nacc = nacc >= 32 ? nacc - 32 : 0;
                    }
                }
                tb += total;
                __syncthreads();
            }
            // the whole bytes out; the rest opens the next tile
            const int full = tb >> 3;
            for (int i = tid; i < full; i += PNG_THREADS) png_store(a, pos + i, (s_buf[i >> 2] >> ((i & 3) * 8)) & 255u);
            const unsigned carry = (s_buf[full >> 2] >> ((full & 3) * 8)) & 255u;
            __syncthreads();
            for (int i = tid; i < PNG_BUF_WORDS; i += PNG_THREADS) s_buf[i] = i == 0 ? carry : 0u;
            pos += full;
            tb &= 7;
            __syncthreads();
        }
        if (tid == 0) {
            const unsigned carry = s_buf[0] & 255u;
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
        __syncthreads();
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

extern "C" size_t ccvs_apng_workspace_bytes(int n, int h, int w, int band_rows) {
    if (!png_shape_ok(n, h, w, band_rows)) return 0;
    const size_t T = (size_t)n * (size_t)png_bands(h, w, band_rows);
    // long boff[T], sizes[T]; unsigned adler_part[T][2], codes[T][260], hdr[T][128], adler[n]; the filtered bytes
    return T * (8 + 8 + 8 + 4 * PNG_CODE_STRIDE + 4 * PNG_HDR_STRIDE) + png_align8(4 * (size_t)n) + png_align8((size_t)n * h * (3 * (size_t)w + 1));
}

extern "C" long ccvs_apng_stream_bound(int n, int h, int w, int band_rows) {
    if (!png_shape_ok(n, h, w, band_rows)) return 0;
    const long r = png_band_rows(w, band_rows), nb = png_bands(h, w, band_rows), rowb = 3L * w + 1;
    // a band: at most 3700 bits of header, 15 bits per byte and for end-of-block, 3 bits and the padding, 4 bytes
    const auto band = [](long bytes) { return (3700 + 15 * (bytes + 1) + 3 + 7) / 8 + 4; };
    const long full = r < h ? r : h, tail = h - (nb - 1) * r;
    return (long)n * (6 + (nb - 1) * band(full * rowb) + band(tail * rowb));
}

extern "C" int ccvs_apng_encode(const uint8_t* rgb, long frame_stride, int n, int h, int w, int filter, int band_rows, uint8_t* stream,
                                long capacity, long* offsets, void* workspace, void* hip_stream) {
    const char* who = "ccvs_apng_encode";
    CCVS_REQUIRE(n >= 1, "%s: no frames (n = %d)", who, n);
    CCVS_REQUIRE(h >= 1 && h <= 65535 && w >= 1 && w <= 65535, "%s: frame size %d x %d outside 1 .. 65535", who, h, w);
    CCVS_REQUIRE(filter >= -1 && filter <= 4, "%s: filter %d is none of -1 (per row), 0 .. 4 (None, Sub, Up, Average, Paeth)", who, filter);
    CCVS_REQUIRE(band_rows >= 0, "%s: band_rows %d is negative", who, band_rows);
    CCVS_REQUIRE(png_shape_ok(n, h, w, band_rows), "%s: band_rows %d makes a band of 2^31 filtered bytes or more", who, band_rows);
    CCVS_REQUIRE(capacity >= 0, "%s: negative capacity", who);
    CCVS_REQUIRE(frame_stride >= 3L * w * h, "%s: frame stride %ld is less than the frame's %ld bytes", who, frame_stride, 3L * w * h);
    CCVS_REQUIRE(rgb && offsets && workspace && (stream || capacity == 0), "%s: null frames, stream, offsets or workspace", who);
    PngArgs a;
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
    a.hdr = (unsigned*)p;               p += 4 * PNG_HDR_STRIDE * (size_t)a.T;
    a.adler = (unsigned*)p;             p += png_align8(4 * (size_t)n);
    a.filt = (uint8_t*)p;
    const unsigned grid = limited_grid(a.T, hip_stream, 8);
    hipLaunchKernelGGL(png_filter_kernel, dim3(grid), dim3(PNG_THREADS), 0, (hipStream_t)hip_stream, a);
    hipLaunchKernelGGL(png_tables_kernel, dim3(limited_grid(a.T, hip_stream, 16)), dim3(PNG_TBL_THREADS), 0, (hipStream_t)hip_stream, a);
    hipLaunchKernelGGL(png_scan_kernel, dim3(1), dim3(PNG_THREADS), 0, (hipStream_t)hip_stream, a);
    hipLaunchKernelGGL(png_emit_kernel, dim3(grid), dim3(PNG_THREADS), 0, (hipStream_t)hip_stream, a);
    CCVS_CHECK_LAUNCH(who);
    return CCVS_OK;
}

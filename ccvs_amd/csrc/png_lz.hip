// The lossless output stage with LZ77 matches (include/ccvs_hip_output_lossless_lz.h).  Filters, bands, the
// Huffman builder, the scan and the framing are png.hip's (png_core.h); a band's block is coded twice over -- with matches, and with
// literals only as png.hip codes it -- and the smaller one by exact bit count is written, so no stream is longer than png.hip's.
// Five launches, all in integers:
//   filter   png.hip's: the filtered frame is complete in the workspace behind it, so a band may look back into earlier bands;
//   match    a wave per band walks the band 64 positions at a time: a hash table in LDS gives every position the nearest earlier one
//            of the band with the same hash, the lanes measure their candidates, the greedy parse hops through the tile from match
//            to match (ballot, count-trailing-zeros, one readlane per match);
//            a token per position (0: inside a match) and the counts of both alphabets;
//   tables   a wave per band: the literal-only block and the match block (png_block_tables), their bits, the choice;
//   scan     png.hip's;
//   emit     png.hip's tiles with a token's up to 48 bits per position.
// tests/apng_lz_ref.py states the same algorithm in numpy; the kernels give its bytes.
#include "png_core.h"

#define LZ_WINDOW 32768
#define LZ_MAX_LEN 258
#define LZ_FAR3 4096                 // a match of length 3 further back than this is dropped
#define LZ_HASH_BITS 13
#define LZ_STRIDE 320                // unsigned per band: the counts of the 286 + 30 symbols, then in their place their codes; [316]: 1 = the match block is written
#define LZ_CHOICE (PNG_NLL + PNG_ND)
#define LZ_TOKEN_BITS 48             // 15 + 5 + 15 + 13

struct PngLzArgs {
    PngArgs p;
    unsigned* lz;                    // [T][LZ_STRIDE]
    unsigned* tok;                   // [n][h][rowb] per position: 0 inside a match, else (length << 16) | (distance - 1), a literal as length 1
};

__global__ __launch_bounds__(PNG_THREADS) void png_lz_filter_kernel(PngArgs a) { png_filter_body(a); }
__global__ __launch_bounds__(PNG_THREADS) void png_lz_scan_kernel(PngArgs a) { png_scan_body(a); }

// ---- match
__device__ __forceinline__ int lz_hash(unsigned v) {        // v: b0 | b1 << 8 | b2 << 16
    return (int)((v * 0x9E3779B1u) >> (32 - LZ_HASH_BITS));
}
// bytes that s and s - d have in common from their first one, at most m (8 at a time; a copy may overlap itself)
__device__ __forceinline__ int lz_common(const uint8_t* s, long d, int m) {
    const uint8_t* q = s - d;
    int n = 0;
    while (n + 8 <= m) {
        unsigned long long x, y;
        __builtin_memcpy(&x, s + n, 8);
        __builtin_memcpy(&y, q + n, 8);
        if (x != y) return n + (__builtin_ctzll(x ^ y) >> 3);
        n += 8;
    }
    while (n < m && s[n] == q[n]) ++n;
    return n;
}
__device__ __forceinline__ int lz_length_symbol(int len, int& extra_value) {   // RFC 1951 3.2.5
    if (len == LZ_MAX_LEN) {
        extra_value = 0;
        return 285;
    }
    const int l = len - 3;
    if (l < 8) {
        extra_value = 0;
        return 257 + l;
    }
    const int eb = 29 - __clz(l);                          // floor(log2 l) - 2
    extra_value = l & ((1 << eb) - 1);
    return 261 + 4 * eb + ((l >> eb) & 3);
}
__device__ __forceinline__ int lz_distance_symbol(int d1, int& extra_value) {   // d1 = distance - 1
    if (d1 < 4) {
        extra_value = 0;
        return d1;
    }
    const int eb = 30 - __clz(d1);                         // floor(log2 d1) - 1
    extra_value = d1 & ((1 << eb) - 1);
    return 2 * (eb + 1) + ((d1 >> eb) & 1);
}

__global__ __launch_bounds__(WAVE) void png_lz_match_kernel(PngLzArgs z) {
    __shared__ int s_head[1 << LZ_HASH_BITS];              // hash -> 1 + the last position of the band inserted with it, 0: none
    __shared__ unsigned s_cnt[LZ_STRIDE];
    const PngArgs& a = z.p;
    const int lane = threadIdx.x;
    for (long band = blockIdx.x; band < a.T; band += gridDim.x) {
        const long f = band / a.nb;
        const int r0 = (int)(band % a.nb) * a.band_rows;
        const int r1 = r0 + a.band_rows < a.h ? r0 + a.band_rows : a.h;
        const long L = (long)(r1 - r0) * a.rowb;
        const long g0 = (long)r0 * a.rowb;                 // the band's first byte in its frame
        const uint8_t* src = a.filt + f * a.h * a.rowb + g0;
        unsigned* tok = z.tok + f * a.h * a.rowb + g0;
        for (int i = lane; i < (1 << LZ_HASH_BITS); i += WAVE) s_head[i] = 0;
        for (int i = lane; i < LZ_STRIDE; i += WAVE) s_cnt[i] = i == 256 ? 1u : 0u;
        __syncthreads();
        long cur = 0;                                      // the parse's next position (the same in every lane)
        for (long t0 = 0; t0 < L; t0 += WAVE) {
            const long p = t0 + lane;
            const bool hashed = p + 2 < L;
            const bool open = cur < t0 + WAVE;             // some position of the tile is not inside a match
            // the position's next 8 bytes in one load where the band has them: the hash's three, and what every candidate is held against first
            const bool wide = p + 8 <= L;
            unsigned long long x = 0;
            if (wide) __builtin_memcpy(&x, src + p, 8);
            else if (hashed) x = (unsigned)src[p] | ((unsigned)src[p + 1] << 8) | ((unsigned)src[p + 2] << 16);
            const int hsh = hashed ? lz_hash((unsigned)x & 0xFFFFFFu) : -1 - lane;
            // the nearest earlier position of the band with this hash: the table's, from the tiles before, unless the tile itself
            // has one -- and it can only where some lane is not the last one of the tile with its hash
            const int before = hashed ? s_head[hsh] : 0;
            __syncthreads();
            if (hashed) atomicMax(&s_head[hsh], (int)p + 1);
            __syncthreads();
            const bool alone = !hashed || s_head[hsh] == (int)p + 1;
            int qi = -1;
            if (open && !__all(alone)) {
#pragma unroll
                for (int j = 0; j < WAVE - 1; ++j) {
                    const int o = __builtin_amdgcn_readlane(hsh, j);
                    if (j < lane && o == hsh) qi = j;
                }
            }
            const long q = qi >= 0 ? t0 + qi : (long)before - 1;
            int len = 0, dist = 0;
            if (open && p < L && p >= cur) {
                const long g = g0 + p;
                const int m = L - p < LZ_MAX_LEN ? (int)(L - p) : LZ_MAX_LEN;
                const long cand[4] = {1, 3, a.rowb, q >= 0 ? p - q : 0};
                unsigned long long y[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {              // (the four loads are in flight together)
                    y[c] = 0;
                    if (wide && cand[c] >= 1 && cand[c] <= g && cand[c] <= LZ_WINDOW) __builtin_memcpy(&y[c], src + p - cand[c], 8);
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const long d = cand[c];
                    if (d < 1 || d > g || d > LZ_WINDOW) continue;
                    if (len == m && d >= dist) continue;   // (it could only tie, and ties go to the smaller distance)
                    int l;
                    if (!wide) l = lz_common(src + p, d, m);
                    else if (x != y[c]) l = __builtin_ctzll(x ^ y[c]) >> 3;
                    else l = 8 + lz_common(src + p + 8, d, m - 8);
                    if (l < 3 || (l == 3 && d > LZ_FAR3)) l = 0;
                    if (l > len || (l == len && l > 0 && d < dist)) {
                        len = l;
                        dist = (int)d;
                    }
                }
            }
            // the greedy parse through the tile
            const long tend = t0 + WAVE < L ? t0 + WAVE : L;
            // (a literal at every position up to the next lane with a match, then over the match)
            const int nt = (int)(tend - t0);
            const unsigned long long matches = __ballot(len > 0);
            unsigned long long starts = 0;
            if (cur < tend) {
                int j = (int)(cur - t0);
                while (j < nt) {
                    const unsigned long long rest = (matches >> j) << j;
                    if (!rest) {
                        starts |= ~((1ull << j) - 1);
                        j = nt;
                        break;
                    }
                    const int k = __builtin_amdgcn_readfirstlane(__builtin_ctzll(rest));
                    starts |= (k >= 63 ? ~0ull : (2ull << k) - 1) & ~((1ull << j) - 1);
                    j = k + __builtin_amdgcn_readlane(len, k);
                }
                cur = t0 + j;
            }
            const bool start = (starts >> lane) & 1;
            if (p < L) {
                unsigned t = 0;
                if (start && len) {
                    int ev;
                    t = ((unsigned)len << 16) | (unsigned)(dist - 1);
                    atomicAdd(&s_cnt[lz_length_symbol(len, ev)], 1u);
                    atomicAdd(&s_cnt[PNG_NLL + lz_distance_symbol(dist - 1, ev)], 1u);
                } else if (start) {
                    t = 1u << 16;
                    atomicAdd(&s_cnt[src[p]], 1u);
                }
                tok[p] = t;
            }
            __syncthreads();
        }
        __syncthreads();
        for (int i = lane; i < LZ_STRIDE; i += WAVE) z.lz[band * LZ_STRIDE + i] = s_cnt[i];
        __syncthreads();
    }
}

// ---- tables: a wave per band
__global__ __launch_bounds__(PNG_TBL_THREADS) void png_lz_tables_kernel(PngLzArgs z) {
    __shared__ PngTableLds t;
    __shared__ PngHeaderLds H;
    __shared__ unsigned s_cnt[LZ_STRIDE], s_code[257], s_lzcode[LZ_STRIDE], s_hdr[PNG_HDR_STRIDE];
    const PngArgs& a = z.p;
    const int lane = threadIdx.x;
    for (long band = blockIdx.x; band < a.T; band += gridDim.x) {
        unsigned* codes = a.codes + band * PNG_CODE_STRIDE;
        unsigned* lz = z.lz + band * LZ_STRIDE;
        const bool last = band % a.nb == a.nb - 1;
        // the literal-only block, as png.hip writes it
        for (int i = lane; i < 257; i += PNG_TBL_THREADS) s_cnt[i] = codes[i];
        __syncthreads();
        const unsigned long long plain = png_block_tables(t, H, s_cnt, 257, nullptr, s_code, nullptr, last, PNG_HDR_STRIDE, lane);
        for (int i = lane; i < PNG_HDR_STRIDE; i += PNG_TBL_THREADS) s_hdr[i] = H.hdr[i];
        __syncthreads();
        // the match block, where the parse found a match
        unsigned matches = 0;
        for (int i = lane; i < LZ_STRIDE; i += PNG_TBL_THREADS) {
            s_cnt[i] = lz[i];
            matches += i >= PNG_NLL && i < LZ_CHOICE ? s_cnt[i] : 0u;
        }
        matches = (unsigned)png_wave_sum(matches);
        __syncthreads();
        bool use = false;
        unsigned long long total = plain;
        if (matches) {
            const unsigned long long with = png_block_tables(t, H, s_cnt, PNG_NLL, s_cnt + PNG_NLL, s_lzcode, s_lzcode + PNG_NLL, last, PNG_LZ_HDR_STRIDE, lane);
            use = with < plain;                            // ties: literal-only
            if (use) total = with;
        }
        for (int i = lane; i < 257; i += PNG_TBL_THREADS) codes[i] = s_code[i];
        for (int i = lane; i < LZ_CHOICE; i += PNG_TBL_THREADS) lz[i] = use ? s_lzcode[i] : 0u;
        for (int i = lane; i < PNG_LZ_HDR_STRIDE; i += PNG_TBL_THREADS)
            a.hdr[band * PNG_LZ_HDR_STRIDE + i] = use ? H.hdr[i] : (i < PNG_HDR_STRIDE ? s_hdr[i] : 0u);
        if (lane == 0) {
            lz[LZ_CHOICE] = use ? 1u : 0u;
            a.sizes[band] = png_band_bytes(total, last);
        }
        __syncthreads();
    }
}

// ---- emit: a position's bits are its token's: the literal's or length's code, the length's extra bits, the distance's code and extra
// bits -- at most LZ_TOKEN_BITS, gathered into one 64-bit value; a position inside a match has none; position L is end-of-block.
#define LZ_BUF_WORDS ((7 + PNG_TILE * LZ_TOKEN_BITS + 31) / 32 + 2)

__global__ __launch_bounds__(PNG_THREADS) void png_lz_emit_kernel(PngLzArgs z) {
    __shared__ unsigned s_buf[LZ_BUF_WORDS], s_code[LZ_STRIDE];
    __shared__ int s_wsum[PNG_WAVES];
    static_assert(LZ_BUF_WORDS >= PNG_LZ_HDR_STRIDE, "the block header is the first tile");
    const PngArgs& a = z.p;
    const int tid = threadIdx.x;
    for (long band = blockIdx.x; band < a.T; band += gridDim.x) {
        const long f = band / a.nb;
        const int b = (int)(band % a.nb);
        const int r0 = b * a.band_rows;
        const int r1 = r0 + a.band_rows < a.h ? r0 + a.band_rows : a.h;
        const long L = (long)(r1 - r0) * a.rowb;
        const bool last = b == a.nb - 1;
        const uint8_t* src = a.filt + (f * a.h + r0) * a.rowb;
        const unsigned* tok = z.tok + (f * a.h + r0) * a.rowb;
        const unsigned* hdr = a.hdr + band * PNG_LZ_HDR_STRIDE;
        const bool lz = z.lz[band * LZ_STRIDE + LZ_CHOICE] != 0;   // (the same in every lane)
        long pos = a.boff[band];
        for (int i = tid; i < LZ_STRIDE; i += PNG_THREADS)
            s_code[i] = lz ? z.lz[band * LZ_STRIDE + i] : (i < 257 ? a.codes[band * PNG_CODE_STRIDE + i] : 0u);
        if (b == 0 && tid == 0) {                          // zlib's header, as png.hip writes it
            png_store(a, pos - 2, 0x78);
            png_store(a, pos - 1, 0x01);
        }
        int tb = (int)hdr[0];
        int used = (tb + 31) / 32 + 1;                     // words of the buffer that may hold bits
        for (int i = tid; i < LZ_BUF_WORDS; i += PNG_THREADS) s_buf[i] = i < (tb + 31) / 32 ? hdr[1 + i] : 0u;
        __syncthreads();
        for (long t0 = -PNG_TILE; t0 <= L; t0 += PNG_TILE) {
            if (t0 >= 0) {
                const long j0 = t0 + (long)tid * PNG_SYMS;
                unsigned long long v[PNG_SYMS];
                int nv[PNG_SYMS], mine = 0;
#pragma unroll
                for (int k = 0; k < PNG_SYMS; ++k) {
                    const long j = j0 + k;
                    v[k] = 0;
                    nv[k] = 0;
                    const unsigned t = j < L ? (lz ? tok[j] : 1u << 16) : 0u;
                    const int len = (int)(t >> 16);
                    if (len == 1 || j == L) {
                        const unsigned e = s_code[j == L ? 256 : src[j]];
                        v[k] = e >> 4;
                        nv[k] = (int)(e & 15);
                    } else if (len) {
                        int lv, dv;
                        const int ls = lz_length_symbol(len, lv), ds = lz_distance_symbol((int)(t & 0xFFFFu), dv);
                        const unsigned el = s_code[ls], ed = s_code[PNG_NLL + ds];
                        int n = (int)(el & 15);
                        v[k] = el >> 4;
                        v[k] |= (unsigned long long)lv << n;
                        n += png_ll_extra(ls);
                        v[k] |= (unsigned long long)(ed >> 4) << n;
                        n += (int)(ed & 15);
                        v[k] |= (unsigned long long)dv << n;
                        nv[k] = n + png_d_extra(ds);
                    }
                    mine += nv[k];
                }
                int before, total;
                png_tile_scan(mine, s_wsum, before, total);
                int p = tb + before;
                unsigned long long acc = 0;
                int nacc = 0;                              // fewer than 32 bits wait in acc
#pragma unroll
                for (int k = 0; k < PNG_SYMS; ++k) {
#pragma unroll
                    for (int half = 0; half < 2; ++half) {  // a token's low 32 bits, then the rest
                        const int n = half == 0 ? (nv[k] < 32 ? nv[k] : 32) : (nv[k] > 32 ? nv[k] - 32 : 0);
                        acc |= (half == 0 ? (v[k] & 0xFFFFFFFFull) : (v[k] >> 32)) << nacc;
                        nacc += n;
                        if (nacc >= 32) {
                            png_tile_or(s_buf, p, (unsigned)acc);
                            p += 32;
                            acc >>= 32;
                            nacc -= 32;
                        }
                    }
                }
                if (nacc > 0) png_tile_or(s_buf, p, (unsigned)acc);
                tb += total;
                used = (tb + 31) / 32 + 1;
                __syncthreads();
            }
            png_tile_out(a, s_buf, used, pos, tb);
        }
        if (tid == 0) png_band_end(a, s_buf[0] & 255u, tb, pos, last, f);
        __syncthreads();
    }
}

// ---- host
extern "C" size_t ccvs_apng_lz_workspace_bytes(int n, int h, int w, int band_rows) {
    if (!png_shape_ok(n, h, w, band_rows)) return 0;
    const size_t T = (size_t)n * (size_t)png_bands(h, w, band_rows);
    // png.hip's workspace with the wider header; unsigned lz[T][320]; a token per filtered byte
    return png_workspace_bytes(n, h, w, band_rows, PNG_LZ_HDR_STRIDE) + T * 4 * LZ_STRIDE + 4 * (size_t)n * h * (3 * (size_t)w + 1);
}

extern "C" int ccvs_apng_encode_lz(const uint8_t* rgb, long frame_stride, int n, int h, int w, int filter, int band_rows, uint8_t* stream,
                                   long capacity, long* offsets, void* workspace, void* hip_stream) {
    const char* who = "ccvs_apng_encode_lz";
    PNG_REQUIRE_ARGS(who);
    PngLzArgs z;
    char* p = png_fill_args(z.p, rgb, frame_stride, n, h, w, filter, band_rows, stream, capacity, offsets, workspace, PNG_LZ_HDR_STRIDE);
    z.lz = (unsigned*)p;                p += 4 * LZ_STRIDE * (size_t)z.p.T;
    z.tok = (unsigned*)p;
    const long T = z.p.T;
    const unsigned grid = limited_grid(T, hip_stream, 8);
    hipLaunchKernelGGL(png_lz_filter_kernel, dim3(grid), dim3(PNG_THREADS), 0, (hipStream_t)hip_stream, z.p);
    hipLaunchKernelGGL(png_lz_match_kernel, dim3(limited_grid(T, hip_stream, 4)), dim3(WAVE), 0, (hipStream_t)hip_stream, z);
    hipLaunchKernelGGL(png_lz_tables_kernel, dim3(limited_grid(T, hip_stream, 16)), dim3(PNG_TBL_THREADS), 0, (hipStream_t)hip_stream, z);
    hipLaunchKernelGGL(png_lz_scan_kernel, dim3(1), dim3(PNG_THREADS), 0, (hipStream_t)hip_stream, z.p);
    hipLaunchKernelGGL(png_lz_emit_kernel, dim3(grid), dim3(PNG_THREADS), 0, (hipStream_t)hip_stream, z);
    CCVS_CHECK_LAUNCH(who);
    return CCVS_OK;
}

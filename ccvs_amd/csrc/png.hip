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
#include "png_core.h"

__global__ __launch_bounds__(PNG_THREADS) void png_filter_kernel(PngArgs a) { png_filter_body(a); }

// ---- tables: a wave per band (png_block_tables: 257 symbols, no distances)
__global__ __launch_bounds__(PNG_TBL_THREADS) void png_tables_kernel(PngArgs a) {
    __shared__ PngTableLds t;
    __shared__ PngHeaderLds H;
    __shared__ unsigned s_cnt[257], s_code[257];
    const int lane = threadIdx.x;
    for (long band = blockIdx.x; band < a.T; band += gridDim.x) {
        unsigned* codes = a.codes + band * PNG_CODE_STRIDE;
        for (int i = lane; i < 257; i += PNG_TBL_THREADS) s_cnt[i] = codes[i];
        __syncthreads();
        const bool last = band % a.nb == a.nb - 1;
        const unsigned long long total = png_block_tables(t, H, s_cnt, 257, nullptr, s_code, nullptr, last, PNG_HDR_STRIDE, lane);
        for (int i = lane; i < 257; i += PNG_TBL_THREADS) codes[i] = s_code[i];
        if (lane == 0) a.sizes[band] = png_band_bytes(total, last);
        for (int i = lane; i < PNG_HDR_STRIDE; i += PNG_TBL_THREADS) a.hdr[band * PNG_HDR_STRIDE + i] = H.hdr[i];
        __syncthreads();
    }
}

__global__ __launch_bounds__(PNG_THREADS) void png_scan_kernel(PngArgs a) { png_scan_body(a); }

// ---- emit: a position's bits are its byte's code; position L is end-of-block
#define PNG_BUF_WORDS ((7 + PNG_TILE * 15 + 31) / 32 + 2)

__global__ __launch_bounds__(PNG_THREADS) void png_emit_kernel(PngArgs a) {
    __shared__ unsigned s_buf[PNG_BUF_WORDS], s_code[257];
    __shared__ int s_wsum[PNG_WAVES];
    static_assert(PNG_BUF_WORDS >= PNG_HDR_STRIDE, "the block header is the first tile");
    const int tid = threadIdx.x;
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
                int before, total;
                png_tile_scan(mine, s_wsum, before, total);
                int p = tb + before;
                unsigned long long acc = 0;
                int nacc = 0;
#pragma unroll
                for (int k = 0; k <= PNG_SYMS; ++k) {
                    if (k < PNG_SYMS) {
                        acc |= (unsigned long long)(e[k] >> 4) << nacc;
                        nacc += (int)(e[k] & 15);
                    }
                    if (nacc >= 32 || (k == PNG_SYMS && nacc > 0)) {
                        png_tile_or(s_buf, p, (unsigned)acc);
                        p += 32;
                        acc >>= 32;
                        nacc = nacc >= 32 ? nacc - 32 : 0;
                    }
                }
                tb += total;
                __syncthreads();
            }
            png_tile_out(a, s_buf, PNG_BUF_WORDS, pos, tb);
        }
        if (tid == 0) png_band_end(a, s_buf[0] & 255u, tb, pos, last, f);
        __syncthreads();
    }
}

// ---- host
extern "C" size_t ccvs_apng_workspace_bytes(int n, int h, int w, int band_rows) {
    if (!png_shape_ok(n, h, w, band_rows)) return 0;
    // the filtered bytes and 1576 bytes per band
    return png_workspace_bytes(n, h, w, band_rows, PNG_HDR_STRIDE);
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
    PNG_REQUIRE_ARGS(who);
    PngArgs a;
    png_fill_args(a, rgb, frame_stride, n, h, w, filter, band_rows, stream, capacity, offsets, workspace, PNG_HDR_STRIDE);
    const unsigned grid = limited_grid(a.T, hip_stream, 8);
    hipLaunchKernelGGL(png_filter_kernel, dim3(grid), dim3(PNG_THREADS), 0, (hipStream_t)hip_stream, a);
    hipLaunchKernelGGL(png_tables_kernel, dim3(limited_grid(a.T, hip_stream, 16)), dim3(PNG_TBL_THREADS), 0, (hipStream_t)hip_stream, a);
    hipLaunchKernelGGL(png_scan_kernel, dim3(1), dim3(PNG_THREADS), 0, (hipStream_t)hip_stream, a);
    hipLaunchKernelGGL(png_emit_kernel, dim3(grid), dim3(PNG_THREADS), 0, (hipStream_t)hip_stream, a);
    CCVS_CHECK_LAUNCH(who);
    return CCVS_OK;
}

// The PNG decoder (include/ccvs_hip_decode_lossless.h): zlib streams -> bytes, and the zlib streams of 8-bit
// RGB PNG images -> uint8 frames [N, H, W, 3].  All arithmetic is integer.  Two stages on the caller's stream:
//   A. png_inflate_kernel: one workgroup of one wave per zlib stream, workgroups striding over the streams.  The wave runs RFC 1950 /
//      1951 (png_decode_core.h: stored, fixed and dynamic blocks, matches up to 32768 back) uniformly -- the same state in every
//      lane, on the scalar unit -- and on LDS alone: the block's tables, a 4 KiB stage of the next input bytes and a 64 KiB ring of
//      the last output bytes.  It stops at token boundaries, where the lanes share the refill of the stage from global memory or the
//      flush of the ring to it, folding the flushed bytes into the Adler-32 sums.  75 KiB of LDS: two workgroups per CU;
//   B. png_unfilter_kernel: one wave per frame at a time, 64 consecutive rows per pass, lane j on row base + j one column behind lane
//      j - 1, so that the left neighbour is the lane's own last result, the upper one comes from lane j - 1 by a shuffle and the
//      upper-left one is the upper one of the step before.
#include "common.h"
#include "png_decode_core.h"

struct PdArgs {
    const uint8_t* data;
    long data_bytes;
    const int64_t* rows;   // [n][4]: offset, bytes, out offset, expected bytes -- or [n][2]: offset, bytes (frame_bytes > 0)
    int n;
    long frame_bytes;      // > 0: stream i holds frame_bytes bytes and goes to out + i * frame_bytes
    uint8_t* out;
    long out_bytes;
    int32_t* status;
};

// ---- A
__global__ __launch_bounds__(64) void png_inflate_kernel(PdArgs a) {
    __shared__ PdTables s_t;
    __shared__ __align__(16) uint8_t s_ring[PD_RING];
    __shared__ __align__(16) uint8_t s_stage[PD_STAGE];
    const int lane = threadIdx.x;
    for (long s = blockIdx.x; s < a.n; s += gridDim.x) {
        long off, len, oo, expect;
        if (a.frame_bytes > 0) {
            off = a.rows[2 * s], len = a.rows[2 * s + 1], oo = s * a.frame_bytes, expect = a.frame_bytes;
        } else {
            off = a.rows[4 * s], len = a.rows[4 * s + 1], oo = a.rows[4 * s + 2], expect = a.rows[4 * s + 3];
        }
        // (written so that no sum can overflow)
        const bool ok = off >= 0 && len >= 0 && off <= a.data_bytes && len <= a.data_bytes - off && oo >= 0 && expect >= 0 && oo <= a.out_bytes &&
                        expect <= a.out_bytes - oo;
        int st = PD_BAD_STREAM;
        if (ok) {   // (the same for every lane)
            const uint8_t* data = a.data + off;
            uint8_t* out = a.out + oo;
            uint64_t s1 = 0, s2 = 0;   // this lane's Adler-32 sums
            PdStream me;               // the same in every lane: the wave runs pd_run uniformly
            pd_begin(me, len, expect);
            for (;;) {
                const int r = pd_run(me, s_t, s_stage, s_ring);
                __syncthreads();   // (one wave: orders the buffers' accesses of the serial part and of the lanes' shares)
                if (r == PD_RUN_INPUT) {
                    const long to = pd_refill_end(me);
                    pd_refill_lane(data, s_stage, me.staged, to, lane, 64);
                    me.staged = to;
                } else if (r == PD_RUN_FLUSH || r == PD_OK) {
                    pd_flush_lane(s_ring, out, me.flushed, me.produced, expect, lane, 64, s1, s2);
                    me.flushed = me.produced;
                }
                __syncthreads();
                if (r >= 0) {
                    st = r;
                    break;
                }
            }
            if (st == PD_OK) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {   // (64 sums below 65521 each)
                    s1 += (uint32_t)__shfl_xor((int)s1, o, 64);
                    s2 += (uint32_t)__shfl_xor((int)s2, o, 64);
                }
                if (pd_adler_join(expect, s1, s2) != me.check) st = PD_BAD_CHECK;
            }
        }
        if (lane == 0) a.status[s] = st;
        __syncthreads();   // the buffers are the next stream's too
    }
}

// ---- B
struct PuArgs {
    const uint8_t* filtered;   // [n][h][3 w + 1]
    int n, h, w;
    uint8_t* rgb;
    long frame_stride;
    int32_t* status;
};

__device__ __forceinline__ int pu_paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__global__ __launch_bounds__(64) void png_unfilter_kernel(PuArgs a) {
    const int lane = threadIdx.x;
    const long rb = 3L * a.w + 1;
    for (long f = blockIdx.x; f < a.n; f += gridDim.x) {
        if (a.status[f] != PD_OK) continue;   // (the same for every lane; the frame's filtered bytes are not all there)
        const uint8_t* src = a.filtered + f * a.h * rb;
        uint8_t* dst = a.rgb + f * a.frame_stride;
        int bad = 0;
        for (int base = 0; base < a.h; base += 64) {
            if (base) __threadfence();   // lane 63's row of the last pass, for lane 0's loads
            const int y = base + lane;
            const bool row = y < a.h;
            const uint8_t* in = src + (long)(row ? y : 0) * rb;
            uint8_t* out = dst + (long)(row ? y : 0) * 3 * a.w;
            const uint8_t* up = dst + (long)(base ? base - 1 : 0) * 3 * a.w;   // lane 0's upper row
            int type = row ? in[0] : 0;
            if (type > 4) {
                bad = 1;
                type = 0;
            }
            uint32_t left = 0, corner = 0;   // the pixel to the left (this lane's last result) and the one above it, as r | g << 8 | b << 16
            for (int t = 0; t < a.w + 63; ++t) {
                const int x = t - lane;
                const bool on = row && x >= 0 && x < a.w;
                uint32_t above = (uint32_t)__shfl_up((int)left, 1, 64);   // lane j - 1 did this column one step ago
                if (lane == 0) {
                    above = 0;
                    if (base && on) above = up[3 * x] | (uint32_t)up[3 * x + 1] << 8 | (uint32_t)up[3 * x + 2] << 16;
                }
                if (!on) {
                    left = 0;   // (left of the row; a lane behind its row's end is read by nobody)
                    corner = 0;
                    continue;
                }
                uint32_t cur = 0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int av = (left >> (8 * c)) & 255, bv = (above >> (8 * c)) & 255, cv = (corner >> (8 * c)) & 255;
                    const int pred = type == 1 ? av : type == 2 ? bv : type == 3 ? (av + bv) >> 1 : type == 4 ? pu_paeth(av, bv, cv) : 0;
                    const int v = (in[1 + 3 * x + c] + pred) & 255;
                    out[3 * x + c] = (uint8_t)v;
                    cur |= (uint32_t)v << (8 * c);
                }
                left = cur;
                corner = above;
            }
        }
        if (__any(bad) && lane == 0) a.status[f] = PD_BAD_FILTER;
    }
}

// ---- the host side
static inline bool pd_shape_ok(int n, int h, int w) { return n >= 1 && h >= 1 && h <= 65535 && w >= 1 && w <= 65535; }
static inline long pd_frame_bytes(int h, int w) { return (long)h * (3L * w + 1); }

extern "C" size_t ccvs_png_decode_workspace_bytes(int n, int h, int w) {
    if (!pd_shape_ok(n, h, w)) return 0;
    return ((size_t)n * pd_frame_bytes(h, w) + 15) & ~(size_t)15;
}

extern "C" int ccvs_zlib_inflate(const uint8_t* data, long data_bytes, const int64_t* rows, const int64_t* rows_host, int n, uint8_t* out, long out_bytes,
                                 int32_t* status, void* hip_stream) {
    CCVS_REQUIRE(n >= 1, "ccvs_zlib_inflate: %d streams", n);
    CCVS_REQUIRE(data_bytes >= 0 && out_bytes >= 0, "ccvs_zlib_inflate: a negative length of the data (%ld) or of the output (%ld)", data_bytes, out_bytes);
    CCVS_REQUIRE(data && rows && rows_host && out && status, "ccvs_zlib_inflate: null data, table, output or status");
    CCVS_REQUIRE((uintptr_t)rows % 8 == 0 && (uintptr_t)status % 4 == 0, "ccvs_zlib_inflate: a misaligned table (8) or status (4)");
    for (int i = 0; i < n; ++i) {
        const int64_t* e = rows_host + 4 * i;
        CCVS_REQUIRE(e[0] >= 0 && e[1] >= 0 && e[0] <= data_bytes && e[1] <= data_bytes - e[0],
                     "ccvs_zlib_inflate: stream %d (bytes %ld + %ld) points outside the data of %ld bytes", i, (long)e[0], (long)e[1], data_bytes);
        CCVS_REQUIRE(e[2] >= 0 && e[3] >= 0 && e[2] <= out_bytes && e[3] <= out_bytes - e[2],
                     "ccvs_zlib_inflate: stream %d (output bytes %ld + %ld) points outside the output of %ld bytes", i, (long)e[2], (long)e[3], out_bytes);
    }
    const PdArgs a = {data, data_bytes, rows, n, 0, out, out_bytes, status};
    hipLaunchKernelGGL(png_inflate_kernel, dim3(limited_grid(n, hip_stream, 8)), dim3(64), 0, (hipStream_t)hip_stream, a);
    CCVS_CHECK_LAUNCH("ccvs_zlib_inflate");
    return CCVS_OK;
}

extern "C" int ccvs_png_decode(const uint8_t* data, long data_bytes, const int64_t* rows, const int64_t* rows_host, int n, int h, int w, uint8_t* rgb,
                               long frame_stride, int32_t* status, void* workspace, void* hip_stream) {
    CCVS_REQUIRE(n >= 1, "ccvs_png_decode: %d frames", n);
    CCVS_REQUIRE(h >= 1 && h <= 65535 && w >= 1 && w <= 65535, "ccvs_png_decode: frame size %d x %d outside 1 .. 65535", h, w);
    CCVS_REQUIRE(data_bytes >= 0 && frame_stride >= (long)h * w * 3, "ccvs_png_decode: a negative length of the data, or a frame stride below a frame's bytes");
    CCVS_REQUIRE(data && rows && rows_host && rgb && status && workspace, "ccvs_png_decode: null data, table, frames, status or workspace");
    CCVS_REQUIRE((uintptr_t)rows % 8 == 0 && (uintptr_t)status % 4 == 0 && (uintptr_t)workspace % 16 == 0,
                 "ccvs_png_decode: a misaligned table (8), status (4) or workspace (16)");
    for (int i = 0; i < n; ++i) {
        const int64_t* e = rows_host + 2 * i;
        CCVS_REQUIRE(e[0] >= 0 && e[1] >= 0 && e[0] <= data_bytes && e[1] <= data_bytes - e[0],
                     "ccvs_png_decode: stream %d (bytes %ld + %ld) points outside the data of %ld bytes", i, (long)e[0], (long)e[1], data_bytes);
    }
    const long fb = pd_frame_bytes(h, w);
    const PdArgs a = {data, data_bytes, rows, n, fb, (uint8_t*)workspace, (long)n * fb, status};
    const PuArgs u = {(const uint8_t*)workspace, n, h, w, rgb, frame_stride, status};
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(png_inflate_kernel, dim3(limited_grid(n, hip_stream, 8)), dim3(64), 0, s, a);
    hipLaunchKernelGGL(png_unfilter_kernel, dim3(limited_grid(n, hip_stream, 8)), dim3(64), 0, s, u);
    CCVS_CHECK_LAUNCH("ccvs_png_decode");
    return CCVS_OK;
}

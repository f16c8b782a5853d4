// The input stage (include/ccvs_hip_input.h): uint8 frames [N, Hs, Ws, 3] -> crop -> Pillow's 8-bit bilinear
// resample (ImagingResample: integer weights of 22 fractional bits, a horizontal pass rounded to uint8, then a vertical one) -> uint8
// [N, Ho, Wo, 3] for a further stage, or fp32 planar through a 3 x 256 table (ToTensor + Normalize as the host computed them).
// All arithmetic on the device is integer, so the result does not depend on the tiling.
#include "common.h"

struct IngestArgs {
    const uint8_t* src;
    long frame_bytes, row_bytes;   // row_bytes = 3 Ws
    int N, top, left, hc, wc, Ho, Wo, hk, vk;
    const int* hcoef; const int* hbounds;
    const int* vcoef; const int* vbounds;
    uint8_t* out_u8; float* out_f32; long out_sN, out_sC;
    const float* lut;
};

#define IG_BITS 22
__device__ __forceinline__ unsigned clip8(int s) {
    s >>= IG_BITS;
    return (unsigned)(s < 0 ? 0 : (s > 255 ? 255 : s));
}
// (first tap, taps) of output index o, clamped to [0, in): a wrong table cannot make the kernel read outside the crop box
__device__ __forceinline__ void taps_of(const int* bounds, int o, int ksize, int in, int& lo, int& sz) {
    lo = bounds[2 * o];
    sz = bounds[2 * o + 1];
    lo = lo < 0 ? 0 : (lo > in ? in : lo);
    sz = sz < 0 ? 0 : sz;
    sz = sz > ksize ? ksize : sz;
    sz = sz > in - lo ? in - lo : sz;
}

// ---- no resample (BAIR: 256 -> 256): crop + uint8 HWC -> fp32 planar (or a cropped uint8 copy).  A lane takes 4 consecutive pixels of a
// row: 12 source bytes -- three dwords where the host has shown every such address to be dword-aligned (ALIGNED), byte loads otherwise --
// and writes one 16-byte store per channel plane.  Nothing passes through LDS but the 3 KB value table.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void ingest_convert_kernel(IngestArgs a) {
    __shared__ float s_lut[768];
    if (a.out_f32) {
        for (int i = threadIdx.x; i < 768; i += 256) s_lut[i] = a.lut[i];
        __syncthreads();
    }
    const int groups = (a.Wo + 3) >> 2;
    const long total = (long)a.N * a.Ho * groups;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int g = (int)(i % groups);
        const long r = i / groups;
        const int y = (int)(r % a.Ho);
        const long n = r / a.Ho;
        const int x = 4 * g;
        const int npx = a.Wo - x < 4 ? a.Wo - x : 4;
        const uint8_t* p = a.src + n * a.frame_bytes + (long)(a.top + y) * a.row_bytes + (long)(a.left + x) * 3;
        unsigned b[12];
        if (ALIGNED) {   // npx == 4: Wo is a multiple of 4
            const unsigned* q = (const unsigned*)p;
            const unsigned w[3] = {q[0], q[1], q[2]};
#pragma unroll
            for (int k = 0; k < 12; ++k) b[k] = (w[k >> 2] >> (8 * (k & 3))) & 255u;
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) b[k] = k < 3 * npx ? p[k] : 0u;
        }
        if (a.out_u8) {
            uint8_t* o = a.out_u8 + (((long)n * a.Ho + y) * a.Wo + x) * 3;
#pragma unroll
            for (int k = 0; k < 12; ++k)
                if (k < 3 * npx) o[k] = (uint8_t)b[k];
        } else {
            float* o = a.out_f32 + n * a.out_sN + (long)y * a.Wo + x;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                F32Quad v;
#pragma unroll
                for (int k = 0; k < 4; ++k) v.v[k] = s_lut[c * 256 + b[3 * k + c]];
                if (npx == 4) *(F32Quad*)(o + c * a.out_sC) = v;
                else
                    for (int k = 0; k < npx; ++k) o[c * a.out_sC + k] = v.v[k];
            }
        }
    }
}

// ---- resample.  A workgroup owns a tile of IG_TH output rows x IG_TW output pixels of one frame.  The source rows its tile needs go
// through the horizontal pass into LDS as uint8 (rounded and clipped: that is what makes the result Pillow's and not a 2-D filter's), in
// chunks of IG_R rows (one pixel -- three channels -- per lane); after each chunk every lane adds the chunk's share of the vertical sums
// of its own 12 output bytes (integer sums: the order does not matter), so a vertical support of any length needs no more LDS.  The finished uint8 tile goes through LDS once more,
// so that the fp32 epilogue reads 4 pixels of one channel per lane and writes 16 bytes per plane.
// Source bytes are read with byte loads: row bytes (3 Ws) and the crop's left edge are arbitrary, no address is known to be aligned.
#define IG_TW 64
#define IG_TD 48    // dwords of a tile row: 3 IG_TW / 4
#define IG_TH 16
#define IG_R 96
#define IG_J (IG_TH * IG_TD / 256)   // dwords of the output tile per lane

__global__ __launch_bounds__(256) void ingest_resample_kernel(IngestArgs a, GridWalk gw) {
    __shared__ unsigned s_rows[IG_R * IG_TD];   // 18 KB
    __shared__ unsigned s_out[IG_TH * IG_TD];   // 3 KB
    __shared__ float s_lut[768];
    const int tid = threadIdx.x;
    if (a.out_f32)
        for (int i = tid; i < 768; i += 256) s_lut[i] = a.lut[i];   // (read after the barriers below)
    GRID_WALK_BEGIN(gw, bx, by, n)
        const int x0 = bx * IG_TW, y0 = by * IG_TH;
        const int th = a.Ho - y0 < IG_TH ? a.Ho - y0 : IG_TH;
        const int tw = a.Wo - x0 < IG_TW ? a.Wo - x0 : IG_TW;
        // the source rows (relative to the crop box) this tile reads: the same in every lane
        int r_lo = y0, r_hi = y0 + th;
        if (a.vcoef) {
            r_lo = a.hc;
            r_hi = 0;
            for (int t = 0; t < th; ++t) {
                int lo, sz;
                taps_of(a.vbounds, y0 + t, a.vk, a.hc, lo, sz);
                if (sz > 0) {
                    r_lo = lo < r_lo ? lo : r_lo;
                    r_hi = lo + sz > r_hi ? lo + sz : r_hi;
                }
            }
        }
        // this lane's IG_J dwords of the output tile and their vertical taps
        int acc[IG_J][4], vlo[IG_J], vsz[IG_J];
#pragma unroll
        for (int j = 0; j < IG_J; ++j) {
            const int oy = (tid + j * 256) / IG_TD;
            vlo[j] = y0 + oy;
            vsz[j] = oy < th ? 1 : 0;
            if (a.vcoef && oy < th) taps_of(a.vbounds, y0 + oy, a.vk, a.hc, vlo[j], vsz[j]);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[j][k] = 1 << (IG_BITS - 1);
        }
        const uint8_t* frame = a.src + n * a.frame_bytes + (long)a.top * a.row_bytes + (long)a.left * 3;
        for (int c0 = r_lo; c0 < r_hi; c0 += IG_R) {
            const int nr = r_hi - c0 < IG_R ? r_hi - c0 : IG_R;
            // horizontal pass of source rows c0 .. c0 + nr - 1, columns of this tile, into LDS: a lane takes one pixel, so that the taps and
            // weights are read once for its three channels and the three sums are independent
            for (int it = tid; it < nr * IG_TW; it += 256) {
                const int row = it / IG_TW, xl = it - row * IG_TW, x = x0 + xl;
                unsigned v0 = 0, v1 = 0, v2 = 0;
                if (xl < tw) {
                    const uint8_t* srow = frame + (long)(c0 + row) * a.row_bytes;
                    if (a.hcoef) {
                        int lo, sz;
                        taps_of(a.hbounds, x, a.hk, a.wc, lo, sz);
                        const int* kk = a.hcoef + (long)x * a.hk;
                        const uint8_t* p = srow + (long)lo * 3;
                        int s0 = 1 << (IG_BITS - 1), s1 = s0, s2 = s0;
                        for (int i = 0; i < sz; ++i) {
                            const int k = kk[i];
                            s0 += k * (int)p[3 * i];
                            s1 += k * (int)p[3 * i + 1];
                            s2 += k * (int)p[3 * i + 2];
                        }
                        v0 = clip8(s0); v1 = clip8(s1); v2 = clip8(s2);
                    } else {
                        const uint8_t* p = srow + (long)x * 3;
                        v0 = p[0]; v1 = p[1]; v2 = p[2];
                    }
                }
                uint8_t* d = (uint8_t*)s_rows + row * (4 * IG_TD) + xl * 3;
                d[0] = (uint8_t)v0; d[1] = (uint8_t)v1; d[2] = (uint8_t)v2;
            }
            __syncthreads();
            // this chunk's share of the vertical sums: source row by source row, the lane's IG_J dwords side by side
            int i0[IG_J], i1[IG_J], i_lo = c0 + nr, i_hi = c0;
#pragma unroll
            for (int j = 0; j < IG_J; ++j) {
                i0[j] = vlo[j] > c0 ? vlo[j] : c0;
                i1[j] = vlo[j] + vsz[j] < c0 + nr ? vlo[j] + vsz[j] : c0 + nr;
                if (i0[j] < i1[j]) {
                    i_lo = i0[j] < i_lo ? i0[j] : i_lo;
                    i_hi = i1[j] > i_hi ? i1[j] : i_hi;
                }
            }
            for (int i = i_lo; i < i_hi; ++i) {
#pragma unroll
                for (int j = 0; j < IG_J; ++j) {
                    const int g = tid + j * 256;
                    const int oy = g / IG_TD, col = g - oy * IG_TD;
                    if (i >= i0[j] && i < i1[j]) {
                        const int k = a.vcoef ? a.vcoef[(long)(y0 + oy) * a.vk + (i - vlo[j])] : 1 << IG_BITS;
                        const unsigned w = s_rows[(i - c0) * IG_TD + col];
                        acc[j][0] += k * (int)(w & 255u);
                        acc[j][1] += k * (int)((w >> 8) & 255u);
                        acc[j][2] += k * (int)((w >> 16) & 255u);
                        acc[j][3] += k * (int)(w >> 24);
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < IG_J; ++j)
            s_out[tid + j * 256] = clip8(acc[j][0]) | (clip8(acc[j][1]) << 8) | (clip8(acc[j][2]) << 16) | (clip8(acc[j][3]) << 24);
        __syncthreads();
        if (a.out_u8) {
            const uint8_t* so = (const uint8_t*)s_out;
            for (int e = tid; e < th * 4 * IG_TD; e += 256) {
                const int oy = e / (4 * IG_TD), b = e - oy * 4 * IG_TD;
                if (b < 3 * tw) a.out_u8[(((long)n * a.Ho + y0 + oy) * a.Wo + x0) * 3 + b] = so[e];
            }
        } else {
            const uint8_t* so = (const uint8_t*)s_out;
            for (int it = tid; it < 3 * IG_TH * (IG_TW / 4); it += 256) {
                const int q = it % (IG_TW / 4), r = it / (IG_TW / 4);
                const int oy = r % IG_TH, c = r / IG_TH;
                const int npx = tw - 4 * q < 4 ? tw - 4 * q : 4;
                if (oy < th && npx > 0) {
                    float* o = a.out_f32 + n * a.out_sN + c * a.out_sC + (long)(y0 + oy) * a.Wo + x0 + 4 * q;
                    F32Quad v;
#pragma unroll
                    for (int k = 0; k < 4; ++k) v.v[k] = s_lut[c * 256 + so[oy * 4 * IG_TD + (4 * q + k) * 3 + c]];
                    if (npx == 4) *(F32Quad*)o = v;
                    else
                        for (int k = 0; k < npx; ++k) o[k] = v.v[k];
                }
            }
        }
        __syncthreads();   // s_out and s_rows are the next tile's too
    GRID_WALK_END
}

extern "C" int ccvs_ingest_u8(const uint8_t* src, int64_t src_frame_bytes, int32_t N, int32_t Hs, int32_t Ws, int32_t top, int32_t left,
                              int32_t hc, int32_t wc, const int32_t* hcoef, const int32_t* hbounds, int32_t hksize, const int32_t* vcoef,
                              const int32_t* vbounds, int32_t vksize, int32_t Ho, int32_t Wo, uint8_t* out_u8, float* out_f32, int64_t out_sN,
                              int64_t out_sC, const float* lut, void* stream) {
    CCVS_REQUIRE(src && N > 0 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0, "ccvs_ingest_u8: null source or empty shape");
    CCVS_REQUIRE(top >= 0 && left >= 0 && hc > 0 && wc > 0 && (long)top + hc <= Hs && (long)left + wc <= Ws,
                 "ccvs_ingest_u8: crop box (%d, %d, %d, %d) leaves the %d x %d frame", top, left, hc, wc, Hs, Ws);
    CCVS_REQUIRE(N == 1 || src_frame_bytes >= (int64_t)Hs * Ws * 3, "ccvs_ingest_u8: frame stride smaller than a frame");
    CCVS_REQUIRE((out_u8 != nullptr) != (out_f32 != nullptr), "ccvs_ingest_u8: exactly one of out_u8 / out_f32");
    CCVS_REQUIRE(!out_f32 || (lut && out_sC >= (int64_t)Ho * Wo && out_sN >= 0), "ccvs_ingest_u8: fp32 output needs the value table and plane strides");
    CCVS_REQUIRE(hcoef ? (hbounds && hksize >= 1) : Wo == wc, "ccvs_ingest_u8: no horizontal table: Wo must equal the crop's width");
    CCVS_REQUIRE(vcoef ? (vbounds && vksize >= 1) : Ho == hc, "ccvs_ingest_u8: no vertical table: Ho must equal the crop's height");
    IngestArgs a;
    a.src = src; a.frame_bytes = src_frame_bytes; a.row_bytes = 3L * Ws;
    a.N = N; a.top = top; a.left = left; a.hc = hc; a.wc = wc; a.Ho = Ho; a.Wo = Wo; a.hk = hksize; a.vk = vksize;
    a.hcoef = hcoef; a.hbounds = hbounds; a.vcoef = vcoef; a.vbounds = vbounds;
    a.out_u8 = out_u8; a.out_f32 = out_f32; a.out_sN = out_sN; a.out_sC = out_sC; a.lut = lut;
    if (!hcoef && !vcoef) {
        const long work = (long)N * Ho * ((Wo + 3) / 4);
        const unsigned blocks = strided_grid(work, stream, 8);
        const bool aligned = ((uintptr_t)src % 4 == 0) && src_frame_bytes % 4 == 0 && a.row_bytes % 4 == 0 && left % 4 == 0 && Wo % 4 == 0;
        if (aligned) hipLaunchKernelGGL(ingest_convert_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL(ingest_convert_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    } else {
        const GridWalk gw = grid_walk(cdiv(Wo, IG_TW), cdiv(Ho, IG_TH), N);
        hipLaunchKernelGGL(ingest_resample_kernel, dim3(limited_grid(gw.total, stream, 8)), dim3(256), 0, (hipStream_t)stream, a, gw);
    }
    CCVS_CHECK_LAUNCH("ccvs_ingest_u8");
    return CCVS_OK;
}

// ================================================================== ccvs_ingest_f32
// The input stage of the video-file datasets (include/ccvs_hip_video.h): the reference's tensor transform chain
// -- uint8 frames / 255, up to three (crop, torch-bilinear resize) stages with fp32 values between them, Normalize -- per output pixel.
// One device function evaluates a stage from the values of the stage below it; the kernel instantiated for ONE stage is the staged
// form (one launch per stage, intermediates in HBM), the one instantiated for all stages the fused form.  Every operation is a single
// correctly rounded fp32 one: contraction is switched off for this part of the file AND inside every function body, so no multiply and
// add fuse into an FMA (plain operators, not __fmul_rn / __fadd_rn: those are header functions compiled under the default contraction
// mode and fuse again once inlined), and a value handed from stage to stage in a register has the bits it would have had in memory,
// so the two forms agree bit for bit.
// HBM-bound at most: a lane takes 4 consecutive output pixels of a row and writes them with one 16-byte store; the reads hit the small
// source (or the previous stage's tensor) through the caches.  No LDS.
#pragma clang fp contract(off)

struct F32Stage {
    int top, left, hin, win, ho, wo;   // the crop box inside the stage's input (hin x win pixels of it) and the output size
    float sh, sw;                      // (float)hin / (float)ho, (float)win / (float)wo
};
struct IngestF32Args {
    const void* src;
    long src_sN, src_sC;
    int Ws, N, C, pre, post;
    F32Stage st[CCVS_INGEST_MAX_STAGES];
    float* out;
    long out_sN, out_sC;
    float mean[3], std[3];
};

// (first sample, second sample, weights) of output index `dst` on an axis of `in` samples: torch's area_pixel_compute_source_index
__device__ __forceinline__ void axis_taps(float scale, int dst, int in, int& i0, int& i1, float& l0, float& l1) {
#pragma clang fp contract(off)
    const float s = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f);
    i0 = (int)s;
    i0 = i0 < in - 1 ? i0 : in - 1;   // (arithmetically never taken: s < in - 0.5; keeps every read inside the box whatever the arguments)
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = s - (float)i0;
    l0 = 1.f - l1;
}

// the value of stage S's output at (y, x) of frame `frame` (a pointer to the frame's first source element), channel c; S == -1: the source
template <int S, bool U8>
__device__ __forceinline__ float chain_value(const IngestF32Args& a, const void* frame, int c, int y, int x) {
#pragma clang fp contract(off)
    if constexpr (S < 0) {
        float v;
        if constexpr (U8) v = (float)((const uint8_t*)frame)[((long)y * a.Ws + x) * 3 + c];
        else v = ((const float*)frame)[c * a.src_sC + (long)y * a.Ws + x];
        if (a.pre == CCVS_INGEST_PRE_DIV255) v = v / 255.f;
        else if (a.pre == CCVS_INGEST_PRE_X2M1) v = v * 2.f - 1.f;
        return v;
    } else {
        const F32Stage& s = a.st[S];
        int y0, y1, x0, x1;
        float ly0, ly1, lx0, lx1;
        axis_taps(s.sh, y, s.hin, y0, y1, ly0, ly1);
        axis_taps(s.sw, x, s.win, x0, x1, lx0, lx1);
        const float p00 = chain_value<S - 1, U8>(a, frame, c, s.top + y0, s.left + x0);
        const float p01 = chain_value<S - 1, U8>(a, frame, c, s.top + y0, s.left + x1);
        const float p10 = chain_value<S - 1, U8>(a, frame, c, s.top + y1, s.left + x0);
        const float p11 = chain_value<S - 1, U8>(a, frame, c, s.top + y1, s.left + x1);
        const float r0 = lx0 * p00 + lx1 * p01;
        const float r1 = lx0 * p10 + lx1 * p11;
        return ly0 * r0 + ly1 * r1;
    }
}

template <int NS, bool U8>
__global__ __launch_bounds__(256) void ingest_f32_kernel(IngestF32Args a) {
#pragma clang fp contract(off)
    const int Ho = a.st[NS - 1].ho, Wo = a.st[NS - 1].wo;
    const int groups = (Wo + 3) >> 2;
    const long total = (long)a.N * a.C * Ho * groups;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int g = (int)(i % groups);
        long r = i / groups;
        const int y = (int)(r % Ho);
        r /= Ho;
        const int c = (int)(r % a.C);
        const long n = r / a.C;
        const int x = 4 * g;
        const int npx = Wo - x < 4 ? Wo - x : 4;
        const void* frame = U8 ? (const void*)((const uint8_t*)a.src + n * a.src_sN) : (const void*)((const float*)a.src + n * a.src_sN);
        F32Quad v;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float t = 0.f;
            if (k < npx) {
                t = chain_value<NS - 1, U8>(a, frame, c, y, x + k);
                if (a.post) t = (t - a.mean[c]) / a.std[c];
            }
            v.v[k] = t;
        }
        float* o = a.out + n * a.out_sN + c * a.out_sC + (long)y * Wo + x;
        if (npx == 4) *(F32Quad*)o = v;
        else
            for (int k = 0; k < npx; ++k) o[k] = v.v[k];
    }
}

template <bool U8>
static void launch_ingest_f32(const IngestF32Args& a, int n_stages, unsigned blocks, hipStream_t stream) {
    if (n_stages == 1) hipLaunchKernelGGL((ingest_f32_kernel<1, U8>), dim3(blocks), dim3(256), 0, stream, a);
    else if (n_stages == 2) hipLaunchKernelGGL((ingest_f32_kernel<2, U8>), dim3(blocks), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((ingest_f32_kernel<3, U8>), dim3(blocks), dim3(256), 0, stream, a);
}

extern "C" int ccvs_ingest_f32(const void* src, int32_t src_is_u8, int64_t src_sN, int64_t src_sC, int32_t N, int32_t C, int32_t Hs, int32_t Ws,
                               int32_t pre, const int32_t* stages, int32_t n_stages, const float* mean_std, float* out, int64_t out_sN,
                               int64_t out_sC, void* stream) {
    CCVS_REQUIRE(src && out && stages, "ccvs_ingest_f32: null source, output or stage list");
    CCVS_REQUIRE(N > 0 && Hs > 0 && Ws > 0 && (long)Hs * Ws < (1L << 30), "ccvs_ingest_f32: empty shape, or a frame of 2^30 pixels or more");
    CCVS_REQUIRE(src_is_u8 ? C == 3 : (C == 1 || C == 3), "ccvs_ingest_f32: %d channels (uint8 frames have 3, fp32 planes 1 or 3)", C);
    CCVS_REQUIRE(pre >= CCVS_INGEST_PRE_NONE && pre <= CCVS_INGEST_PRE_X2M1, "ccvs_ingest_f32: pre-op %d is none of CCVS_INGEST_PRE_*", pre);
    CCVS_REQUIRE(n_stages >= 1 && n_stages <= CCVS_INGEST_MAX_STAGES, "ccvs_ingest_f32: %d stages, 1 .. %d are evaluated", n_stages, CCVS_INGEST_MAX_STAGES);
    if (src_is_u8) CCVS_REQUIRE(N == 1 || src_sN >= (int64_t)Hs * Ws * 3, "ccvs_ingest_f32: frame stride smaller than a frame");
    else CCVS_REQUIRE((C == 1 || src_sC >= (int64_t)Hs * Ws) && (N == 1 || src_sN >= (int64_t)Hs * Ws), "ccvs_ingest_f32: source plane or frame stride smaller than a plane");
    IngestF32Args a;
    a.src = src; a.src_sN = src_sN; a.src_sC = src_sC; a.Ws = Ws; a.N = N; a.C = C; a.pre = pre; a.post = mean_std ? 1 : 0;
    int hin = Hs, win = Ws;
    for (int s = 0; s < CCVS_INGEST_MAX_STAGES; ++s) {
        F32Stage& st = a.st[s];
        if (s >= n_stages) {
            st = a.st[n_stages - 1];
            continue;
        }
        const int32_t* e = stages + 6 * s;
        CCVS_REQUIRE(e[0] >= 0 && e[1] >= 0 && e[2] > 0 && e[3] > 0 && (long)e[0] + e[2] <= hin && (long)e[1] + e[3] <= win,
                     "ccvs_ingest_f32: stage %d: crop box (%d, %d, %d, %d) leaves its %d x %d input", s, e[0], e[1], e[2], e[3], hin, win);
        CCVS_REQUIRE(e[4] > 0 && e[5] > 0 && (long)e[4] * e[5] < (1L << 30), "ccvs_ingest_f32: stage %d: output size %d x %d", s, e[4], e[5]);
        st.top = e[0]; st.left = e[1]; st.hin = e[2]; st.win = e[3]; st.ho = e[4]; st.wo = e[5];
        st.sh = (float)st.hin / (float)st.ho;
        st.sw = (float)st.win / (float)st.wo;
        hin = st.ho; win = st.wo;
    }
    CCVS_REQUIRE((C == 1 || out_sC >= (int64_t)hin * win) && out_sN >= 0, "ccvs_ingest_f32: output plane stride smaller than a plane, or a negative frame stride");
    for (int c = 0; c < 3; ++c) {
        a.mean[c] = mean_std && c < C ? mean_std[c] : 0.f;
        a.std[c] = mean_std && c < C ? mean_std[C + c] : 1.f;
    }
    a.out = out; a.out_sN = out_sN; a.out_sC = out_sC;
    const long work = (long)N * C * hin * ((win + 3) / 4);
    const unsigned blocks = strided_grid(work, stream, 8);
    if (src_is_u8) launch_ingest_f32<true>(a, n_stages, blocks, (hipStream_t)stream);
    else launch_ingest_f32<false>(a, n_stages, blocks, (hipStream_t)stream);
    CCVS_CHECK_LAUNCH("ccvs_ingest_f32");
    return CCVS_OK;
}

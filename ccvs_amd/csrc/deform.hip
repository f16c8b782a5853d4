// The flow-decoder variants of Matching (skip_autoencoder.py:131-206): the deformable 3 x 3 convolution of the context
// features with one offset per pixel (--q_use_deformed_conv), the grouped x2 transposed convolution of the trade-off feature
// (--q_use_tradeoff) and the masked-flow / trade-off epilogue of the plain back-warp (--q_use_masked_flow, --q_use_tradeoff).
//
// Deformable convolution as an implicit GEMM on the matrix cores: M = output channels, N = 256 output pixels of one image,
// K = 9 taps x C channels.  A step is one (tap, 16-channel chunk): every thread owns one pixel of the tile and gathers its
// 16 channels bilinearly (4 corners each, the corners and weights shared by the chunks of the tap) into LDS in the operand
// layout of the split-bf16 convolution ([half][hi|lo][pixel][8 bf16], conv2d_bf16_kernels.h) or as fp32 [channel][pixel] for
// the strict mode; the weights are the convolution's packed forms (ops.pack_conv_weight, no scale).  Activations and weights
// are double-buffered in LDS with one barrier per step, the loads of step s + 1 issued before the MFMAs of step s.
#include "common.h"
#include "conv_common.h"
#include "conv2d_bf16_kernels.h"

namespace {

struct DfCtx {
    int k;
    const float* p[CCVS_MAX_CTX];
    long sN[CCVS_MAX_CTX];
};

struct DeformK {
    DfCtx ctx;
    long x_sC;
    const float* flow;
    long flow_sN;
    float mult;
    const void* w;
    int CoutPad;
    const float* bias;
    const float* occ;
    long occ_sN;
    const float* toff;
    long toff_sN, toff_sC;
    float* y;
    long y_sN, y_sC;
    int N, C, H, W, act;
};

constexpr int DF_PIX = 256;   // output pixels per workgroup (4 waves x 2 blocks of 32)

// torchvision's bilinear_interpolate (deform_conv2d kernel): 0 outside (-1, H) x (-1, W), a corner outside the image adds 0.
// Corner offsets are clamped into the image and the weight of an outside corner is zero.
struct Corners {
    int o[4];
    float w[4];
};
__device__ __forceinline__ Corners df_corners(float hy, float wx, int H, int W, bool valid) {
    Corners c;
    if (!valid || hy <= -1.f || hy >= (float)H || wx <= -1.f || wx >= (float)W) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { c.o[i] = 0; c.w[i] = 0.f; }
        return c;
    }
    const float hf = floorf(hy), wf = floorf(wx);
    const int h0 = (int)hf, w0 = (int)wf, h1 = h0 + 1, w1 = w0 + 1;
    const float lh = hy - hf, lw = wx - wf, hh = 1.f - lh, hw = 1.f - lw;
    const bool r0 = h0 >= 0, r1 = h1 <= H - 1, c0 = w0 >= 0, c1 = w1 <= W - 1;
    const int ch0 = max(h0, 0) * W, ch1 = min(h1, H - 1) * W, cw0 = max(w0, 0), cw1 = min(w1, W - 1);
    c.o[0] = ch0 + cw0; c.w[0] = (r0 && c0) ? hh * hw : 0.f;
    c.o[1] = ch0 + cw1; c.w[1] = (r0 && c1) ? hh * lw : 0.f;
    c.o[2] = ch1 + cw0; c.w[2] = (r1 && c0) ? lh * hw : 0.f;
    c.o[3] = ch1 + cw1; c.w[3] = (r1 && c1) ? lh * lw : 0.f;
    return c;
}

template <int MB, bool F32>
__global__ __launch_bounds__(256) void deform_conv3x3_kernel(DeformK p) {
    constexpr int NT = 32 * MB;
    // activations: bf16 [2 buf][4 = half x hi|lo][256] uint4, fp32 [2 buf][16][256] float: 32 KB either way
    // weights:     bf16 [2 buf][4][NT] uint4,             fp32 [2 buf][16][NT] float: NT x 128 B
    __shared__ __attribute__((aligned(16))) uint4 in_s[2 * 4 * DF_PIX];
    __shared__ __attribute__((aligned(16))) uint4 w_s[2 * 4 * NT];
    constexpr int WU = (4 * NT + 255) / 256;   // 16-byte weight units per thread and step

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, khalf = lane >> 5;
    const int HW = p.H * p.W;
    const int pix0 = blockIdx.x * DF_PIX;
    const int n0 = blockIdx.y * NT;
    const int n = blockIdx.z;
    const int jn = n % p.ctx.k;
    const float* xn = p.ctx.p[jn] + (long)(n / p.ctx.k) * p.ctx.sN[jn];

    // this thread's gather pixel and its shared offset (flow x -> rows, flow y -> columns: torchvision's (dy, dx) order)
    const int gp = pix0 + tid;
    const bool gvalid = gp < HW;
    const int gy = gvalid ? gp / p.W : 0, gx = gvalid ? gp - gy * p.W : 0;
    const float* fl = p.flow + (long)n * p.flow_sN + (gvalid ? gp : 0);
    const float offh = fl[0] * p.mult, offw = fl[HW] * p.mult;

    const int nch = p.C / CB_CC;
    const int S = 9 * nch;

    f32x16 acc[MB][2];
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int pp = 0; pp < 2; ++pp)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][pp][r] = 0.f;

    float raw[CB_CC][4];
    uint4 wr[WU];
    Corners cn;

    auto load_step = [&](int s) {
        const int tap = s / nch, c0 = (s - tap * nch) * CB_CC;
        const int ti = tap / 3, tj = tap - 3 * ti;
        cn = df_corners((float)(gy - 1 + ti) + offh, (float)(gx - 1 + tj) + offw, p.H, p.W, gvalid);
        const float* src = xn + (long)c0 * p.x_sC;
#pragma unroll
        for (int c = 0; c < CB_CC; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) raw[c][q] = src[(long)c * p.x_sC + cn.o[q]];
#pragma unroll
        for (int u = 0; u < WU; ++u) {
            const int i = tid + 256 * u;
            if (i < 4 * NT) {
                if constexpr (F32) {
                    const int kk = i / (NT / 4), q = i - kk * (NT / 4);
                    const float* wf = (const float*)p.w + ((long)tap * p.C + c0 + kk) * p.CoutPad + n0;
                    wr[u] = reinterpret_cast<const uint4*>(wf)[q];
                } else {
                    const int hp = i / NT, co = i - hp * NT;
                    const int CinG = p.C / 8;
                    wr[u] = ((const uint4*)p.w)[(((long)tap * CinG + (c0 >> 3) + (hp >> 1)) * 2 + (hp & 1)) * p.CoutPad + n0 + co];
                }
            }
        }
    };
    auto store_step = [&](int buf) {
        float v[CB_CC];
#pragma unroll
        for (int c = 0; c < CB_CC; ++c) v[c] = cn.w[0] * raw[c][0] + cn.w[1] * raw[c][1] + cn.w[2] * raw[c][2] + cn.w[3] * raw[c][3];
        if constexpr (F32) {
            float* inf = reinterpret_cast<float*>(in_s) + buf * CB_CC * DF_PIX;
#pragma unroll
            for (int c = 0; c < CB_CC; ++c) inf[c * DF_PIX + tid] = v[c];
        } else {
            uint4* it = in_s + buf * 4 * DF_PIX;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float v8[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) v8[i] = v[8 * h + i];
                uint4 hi, lo;
                split8(v8, hi, lo);
                it[(2 * h + 0) * DF_PIX + tid] = hi;
                it[(2 * h + 1) * DF_PIX + tid] = lo;
            }
        }
#pragma unroll
        for (int u = 0; u < WU; ++u) {
            const int i = tid + 256 * u;
            if (i < 4 * NT) w_s[buf * 4 * NT + i] = wr[u];
        }
    };

    load_step(0);
    store_step(0);
    __syncthreads();
    for (int s = 0; s < S; ++s) {
        const int buf = s & 1;
        if (s + 1 < S) load_step(s + 1);
        if constexpr (F32) {
            const float* inf = reinterpret_cast<const float*>(in_s) + buf * CB_CC * DF_PIX;
            const float* wf = reinterpret_cast<const float*>(w_s) + buf * CB_CC * NT;
#pragma unroll
            for (int kk = 0; kk < CB_CC / 2; ++kk) {
                const int kr = 2 * kk + khalf;
                float b[2];
#pragma unroll
                for (int pp = 0; pp < 2; ++pp) b[pp] = inf[kr * DF_PIX + (wave * 2 + pp) * 32 + l32];
#pragma unroll
                for (int m = 0; m < MB; ++m) {
                    const float a = wf[kr * NT + m * 32 + l32];
#pragma unroll
                    for (int pp = 0; pp < 2; ++pp) acc[m][pp] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[pp], acc[m][pp], 0, 0, 0);
                }
            }
        } else {
            const uint4* it = in_s + buf * 4 * DF_PIX + (khalf * 2) * DF_PIX;
            const uint4* wt = w_s + buf * 4 * NT + (khalf * 2) * NT + l32;
            bf16x8 bh[2], bl[2];
#pragma unroll
            for (int pp = 0; pp < 2; ++pp) {
                const int col = (wave * 2 + pp) * 32 + l32;
                bh[pp] = __builtin_bit_cast(bf16x8, it[col]);
                bl[pp] = __builtin_bit_cast(bf16x8, it[DF_PIX + col]);
            }
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                const bf16x8 ah = __builtin_bit_cast(bf16x8, wt[m * 32]);
                const bf16x8 al = __builtin_bit_cast(bf16x8, wt[NT + m * 32]);
#pragma unroll
                for (int pp = 0; pp < 2; ++pp) {
                    acc[m][pp] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh[pp], acc[m][pp], 0, 0, 0);
                    acc[m][pp] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl[pp], acc[m][pp], 0, 0, 0);
                    acc[m][pp] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh[pp], acc[m][pp], 0, 0, 0);
                }
            }
        }
        if (s + 1 < S) store_step(buf ^ 1);
        __syncthreads();
    }

    // epilogue: a lane owns one pixel and 16 channels of each 32 x 32 block
#pragma unroll
    for (int pp = 0; pp < 2; ++pp) {
        const int pix = pix0 + (wave * 2 + pp) * 32 + l32;
        if (pix >= HW) continue;
        float keep = 1.f;
        if (p.occ) keep = 1.f - 1.f / (1.f + expf(-p.occ[(long)n * p.occ_sN + pix]));
        float* yb = p.y + (long)n * p.y_sN + pix;
        const float* tb = p.toff ? p.toff + (long)n * p.toff_sN + pix : nullptr;
#pragma unroll
        for (int m = 0; m < MB; ++m) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = n0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
                if (co < p.C) {
                    float v = acc[m][pp][r] + (p.bias ? p.bias[co] : 0.f);
                    if (p.occ) v *= keep;
                    if (tb) v += tb[(long)co * p.toff_sC];
                    if (p.act == CCVS_ACT_LRELU) v = lrelu01(v);
                    yb[(long)co * p.y_sC] = v;
                }
            }
        }
    }
}

// y[n][o] = sum of the (up to) 2 x 2 taps of ConvTranspose2d(4, stride 2, padding 1) on input channel o / mult:
// output row Y takes taps ky = (Y + 1) & 1 and ky + 2 at input rows (Y + 1 - ky) / 2.
__global__ __launch_bounds__(256) void gconvT4x4s2_kernel(const float* __restrict__ x, long x_sN, const float* __restrict__ w,
                                                          float* __restrict__ y, long y_sN, long y_sC, long N, int G, int mult,
                                                          int H, int W) {
    const int Ho = 2 * H, Wo = 2 * W, Co = G * mult;
    const long total = N * Co * (long)Ho * Wo;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int ox = (int)(i % Wo);
        long t = i / Wo;
        const int oy = (int)(t % Ho);
        t /= Ho;
        const int o = (int)(t % Co);
        const long n = t / Co;
        const float* xp = x + n * x_sN + (long)(o / mult) * H * W;
        const float* wp = w + (long)o * 16;
        const int ky0 = (oy + 1) & 1, kx0 = (ox + 1) & 1;
        float acc = 0.f;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int ky = ky0 + 2 * a, iy = (oy + 1 - ky) >> 1;
            if (iy < 0 || iy >= H) continue;
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int kx = kx0 + 2 * b, ix = (ox + 1 - kx) >> 1;
                if (ix < 0 || ix >= W) continue;
                acc += xp[(long)iy * W + ix] * wp[ky * 4 + kx];
            }
        }
        y[n * y_sN + (long)o * y_sC + (long)oy * Wo + ox] = acc;
    }
}

__global__ __launch_bounds__(256) void flow_mask_toff_kernel(float* __restrict__ x, long x_sN, long x_sC, const float* __restrict__ occ,
                                                             long occ_sN, const float* __restrict__ toff, long toff_sN, long toff_sC,
                                                             long N, int C, long HW, int act) {
    const long total = N * C * HW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long pix = i % HW;
        const long t = i / HW;
        const int c = (int)(t % C);
        const long n = t / C;
        float* xp = x + n * x_sN + (long)c * x_sC + pix;
        float v = *xp;
        if (occ) v *= 1.f - 1.f / (1.f + expf(-occ[n * occ_sN + pix]));
        if (toff) v += toff[n * toff_sN + (long)c * toff_sC + pix];
        if (act == CCVS_ACT_LRELU) v = lrelu01(v);
        *xp = v;
    }
}

template <int MB>
void launch_deform(const DeformK& k, int f32, hipStream_t st) {
    const dim3 grid(cdiv(k.H * k.W, DF_PIX), k.CoutPad / (32 * MB), k.N);
    if (f32) hipLaunchKernelGGL((deform_conv3x3_kernel<MB, true>), grid, dim3(256), 0, st, k);
    else hipLaunchKernelGGL((deform_conv3x3_kernel<MB, false>), grid, dim3(256), 0, st, k);
}

}  // namespace

extern "C" int ccvs_deform_conv3x3_ctx(const ccvs_ctx_list* ctx, int64_t x_sC, const float* flow, int64_t flow_sN, float flow_mult,
                                       const void* w, int32_t CoutPad, int32_t precision, const float* bias, const float* occ, int64_t occ_sN,
                                       const float* toff, int64_t toff_sN, int64_t toff_sC, float* y, int64_t y_sN, int64_t y_sC, int32_t N,
                                       int32_t C, int32_t H, int32_t W, int32_t act, void* stream) {
    CCVS_REQUIRE(ctx && flow && w && y, "ccvs_deform_conv3x3_ctx: null pointer");
    CCVS_REQUIRE(ctx->k >= 1 && ctx->k <= CCVS_MAX_CTX, "ccvs_deform_conv3x3_ctx: context list of 1..%d entries expected", CCVS_MAX_CTX);
    CCVS_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && N <= 65535, "ccvs_deform_conv3x3_ctx: bad shape");
    CCVS_REQUIRE(C % 16 == 0, "ccvs_deform_conv3x3_ctx: C %% 16 == 0 required, got %d", C);
    CCVS_REQUIRE(precision == 0 || precision == 1, "ccvs_deform_conv3x3_ctx: precision %d unknown", precision);
    CCVS_REQUIRE(CoutPad % 32 == 0 && CoutPad >= C, "ccvs_deform_conv3x3_ctx: CoutPad %d invalid for C %d", CoutPad, C);
    CCVS_REQUIRE(x_sC >= (int64_t)H * W, "ccvs_deform_conv3x3_ctx: channel stride %lld below H*W", (long long)x_sC);
    DeformK k = {};
    k.ctx.k = ctx->k;
    for (int j = 0; j < ctx->k; ++j) {
        CCVS_REQUIRE(ctx->p[j], "ccvs_deform_conv3x3_ctx: null context %d", j);
        k.ctx.p[j] = ctx->p[j];
        k.ctx.sN[j] = (long)ctx->sN[j];
    }
    k.x_sC = (long)x_sC; k.flow = flow; k.flow_sN = (long)flow_sN; k.mult = flow_mult;
    k.w = w; k.CoutPad = CoutPad; k.bias = bias; k.occ = occ; k.occ_sN = (long)occ_sN;
    k.toff = toff; k.toff_sN = (long)toff_sN; k.toff_sC = (long)toff_sC;
    k.y = y; k.y_sN = (long)y_sN; k.y_sC = (long)y_sC;
    k.N = N; k.C = C; k.H = H; k.W = W; k.act = act;
    const int nb = CoutPad / 32;
    hipStream_t st = (hipStream_t)stream;
    const int f32 = precision == 0;
    if (nb % 4 == 0) launch_deform<4>(k, f32, st);
    else if (nb % 3 == 0) launch_deform<3>(k, f32, st);
    else if (nb % 2 == 0) launch_deform<2>(k, f32, st);
    else launch_deform<1>(k, f32, st);
    CCVS_CHECK_LAUNCH("ccvs_deform_conv3x3_ctx");
    return CCVS_OK;
}

extern "C" int ccvs_gconvT4x4s2(const float* x, int64_t x_sN, const float* w, float* y, int64_t y_sN, int64_t y_sC, int32_t N, int32_t G,
                                int32_t mult, int32_t H, int32_t W, void* stream) {
    CCVS_REQUIRE(x && w && y, "ccvs_gconvT4x4s2: null pointer");
    CCVS_REQUIRE(N > 0 && G > 0 && mult > 0 && H > 0 && W > 0, "ccvs_gconvT4x4s2: bad shape");
    CCVS_REQUIRE(y_sC >= 4LL * H * W, "ccvs_gconvT4x4s2: output channel stride %lld below 4*H*W", (long long)y_sC);
    const long total = (long)N * G * mult * 4L * H * W;
    const unsigned grid = (unsigned)std::min<long>(cdiv64(total, 256), 1L << 20);
    hipLaunchKernelGGL(gconvT4x4s2_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (long)x_sN, w, y, (long)y_sN, (long)y_sC,
                       (long)N, G, mult, H, W);
    CCVS_CHECK_LAUNCH("ccvs_gconvT4x4s2");
    return CCVS_OK;
}

extern "C" int ccvs_flow_mask_toff(float* x, int64_t x_sN, int64_t x_sC, const float* occ, int64_t occ_sN, const float* toff, int64_t toff_sN,
                                   int64_t toff_sC, int32_t N, int32_t C, int32_t H, int32_t W, int32_t act, void* stream) {
    CCVS_REQUIRE(x, "ccvs_flow_mask_toff: null pointer");
    CCVS_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "ccvs_flow_mask_toff: bad shape");
    const long total = (long)N * C * H * W;
    const unsigned grid = (unsigned)std::min<long>(cdiv64(total, 256), 1L << 20);
    hipLaunchKernelGGL(flow_mask_toff_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (long)x_sN, (long)x_sC, occ, (long)occ_sN,
                       toff, (long)toff_sN, (long)toff_sC, (long)N, C, (long)H * W, act);
    CCVS_CHECK_LAUNCH("ccvs_flow_mask_toff");
    return CCVS_OK;
}

// Output head of the STFT decoder (skip_autoencoder.py:550,555): ConvLayer(hsize, 1, 1) -- a 1 x 1 EqualConv2d to ONE channel, its bias,
// LeakyReLU(0.1) -- and the tanh behind the stack, in one pass:
//   y[n, p] = tanh(lrelu(bias + sum_c (w[c] * scale) x[n, c, p])),   p = 0 .. H W - 1.
// A pure stream, 4 C bytes in and 4 bytes out per pixel (0.5 FLOP per byte): through the MFMA convolution the layer would fill 1 of 32
// output rows.  A lane owns four consecutive pixels of a plane and reads them as one 16-byte load per channel plane (one pixel per lane
// where H W is not a multiple of 4).  A 256-thread workgroup owns 256 / G such items; the G thread groups split the channels into G
// consecutive ranges and group 0 adds the partial sums in group order through LDS: no atomics, the same bits on every run.  G grows as
// the launch shrinks (`channel_head_form`), as for ToRGB (resample.hip).  The [C] scaled weights sit in LDS.
#include "common.h"

struct ChannelHeadK {
    const float* x;
    const float* w;      // [C]
    const float* bias;   // [1] or NULL
    float* y;            // [N, H W]
    long x_sN, items;    // items = N * HW / PX
    int C, HW, per_img;  // per_img = HW / PX
    float scale;
    int act, tanh_out;
};

template <int G, int PX>
__global__ __launch_bounds__(256) void channel_head_kernel(ChannelHeadK p) {
    constexpr int Q = 256 / G;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* wl = smem;                           // [C]: w * scale, the fp32 product EqualConv2d forms
    float* red = smem + ((p.C + 3) & ~3);       // [PX][256]: partial sums of groups 1 .. G-1
    const int tid = threadIdx.x, g = tid / Q, j = tid - g * Q;
    for (int c = tid; c < p.C; c += 256) wl[c] = p.w[c] * p.scale;
    const int c0 = (int)(((long)g * p.C) / G), c1 = (int)(((long)(g + 1) * p.C) / G);
    const float b = p.bias ? p.bias[0] : 0.f;
    const long nblocks = (p.items + Q - 1) / Q;
    for (long blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        __syncthreads();   // the weights are staged / the previous block's partials have been read
        const long r = blk * Q + j;
        const bool live = r < p.items;
        float acc[PX];
#pragma unroll
        for (int o = 0; o < PX; ++o) acc[o] = 0.f;
        long n = 0;
        int pix = 0;
        if (live) {
            n = r / p.per_img;
            pix = (int)(r - n * p.per_img) * PX;
            const float* xp = p.x + n * p.x_sN + pix;
            if (PX == 4) {
#pragma unroll 8
                for (int k = c0; k < c1; ++k) {
                    const F32Quad v = *reinterpret_cast<const F32Quad*>(xp + (long)k * p.HW);
                    const float wk = wl[k];
#pragma unroll
                    for (int o = 0; o < PX; ++o) acc[o] = fmaf(wk, v.v[o], acc[o]);
                }
            } else {
#pragma unroll 8
                for (int k = c0; k < c1; ++k) acc[0] = fmaf(wl[k], xp[(long)k * p.HW], acc[0]);
            }
        }
        if (G > 1) {
            if (g > 0) {
#pragma unroll
                for (int o = 0; o < PX; ++o) red[o * 256 + tid] = acc[o];
            }
            __syncthreads();
        }
        if (g == 0 && live) {
#pragma unroll 1
            for (int gg = 1; gg < G; ++gg)
#pragma unroll
                for (int o = 0; o < PX; ++o) acc[o] += red[o * 256 + gg * Q + j];
            float out[PX];
#pragma unroll
            for (int o = 0; o < PX; ++o) {
                float v = acc[o] + b;
                if (p.act) v = lrelu01(v);
                if (p.tanh_out) v = (float)tanh((double)v);   // one value per 4 C bytes read: float64 costs nothing here and rounds once
                out[o] = v;
            }
            float* yp = p.y + n * p.HW + pix;
            if (PX == 4) {
                F32Quad o4;
#pragma unroll
                for (int o = 0; o < PX; ++o) o4.v[o] = out[o];
                *reinterpret_cast<F32Quad*>(yp) = o4;
            } else {
                yp[0] = out[0];
            }
        }
    }
}

// Channel groups per item of a launch of `items` items: 4 (one wave per channel range, 64 items per workgroup) from 1024 such
// workgroups up, 16 from 256 workgroups of 16 items up, 64 (4 items per workgroup) below.
static inline int channel_head_form(long items) {
    if (cdiv64(items, 64) >= 1024) return 4;
    if (cdiv64(items, 16) >= 256) return 16;
    return 64;
}

template <int PX>
static void channel_head_launch(const ChannelHeadK& p, void* stream) {
    const size_t lds = (size_t)(((p.C + 3) & ~3) + PX * 256) * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    switch (channel_head_form(p.items)) {
        case 4: hipLaunchKernelGGL((channel_head_kernel<4, PX>), dim3(limited_grid(cdiv64(p.items, 64), stream, 8)), dim3(256), lds, st, p); break;
        case 16: hipLaunchKernelGGL((channel_head_kernel<16, PX>), dim3(limited_grid(cdiv64(p.items, 16), stream, 8)), dim3(256), lds, st, p); break;
        default: hipLaunchKernelGGL((channel_head_kernel<64, PX>), dim3(limited_grid(cdiv64(p.items, 4), stream, 8)), dim3(256), lds, st, p); break;
    }
}

extern "C" int ccvs_channel_head(const float* x, int64_t x_sN, const float* w, float scale, const float* bias, float* y, int32_t N, int32_t C,
                                 int32_t H, int32_t W, int32_t act, int32_t tanh_out, void* stream) {
    CCVS_REQUIRE(x && w && y, "ccvs_channel_head: null pointer");
    CCVS_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "ccvs_channel_head: empty tensor");
    CCVS_REQUIRE(C <= 8192, "ccvs_channel_head: C = %d (at most 8192)", C);
    CCVS_REQUIRE((int64_t)H * W < 2147483647L / 4, "ccvs_channel_head: H W = %lld is too large", (long long)H * W);
    CCVS_REQUIRE(x_sN >= (int64_t)C * H * W, "ccvs_channel_head: batch stride %lld below C H W", (long long)x_sN);
    ChannelHeadK p;
    p.x = x; p.w = w; p.bias = bias; p.y = y;
    p.x_sN = x_sN; p.C = C; p.HW = H * W; p.scale = scale; p.act = act ? 1 : 0; p.tanh_out = tanh_out ? 1 : 0;
    if (p.HW % 4 == 0) {
        p.per_img = p.HW / 4;
        p.items = (long)N * p.per_img;
        channel_head_launch<4>(p, stream);
    } else {
        p.per_img = p.HW;
        p.items = (long)N * p.per_img;
        channel_head_launch<1>(p, stream);
    }
    CCVS_CHECK_LAUNCH("ccvs_channel_head");
    return CCVS_OK;
}

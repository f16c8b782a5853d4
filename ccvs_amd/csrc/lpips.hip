// The memory-bound passes of LPIPS (piq.LPIPS(reduction='mean'), piq 0.5.4; tools/pytorch_metrics/metrics.py:12-13; DESIGN.md section
// 4.19) around its VGG16 convolutions, which are ccvs_conv2d / ccvs_conv2d_bf16x3 as they stand (bias, no activation):
//
//   ccvs_lpips_prep      (x - mean[c]) / std[c]: the ImageNet normalisation in front of the network
//   ccvs_relu_           nn.ReLU in place, for the convolutions that are neither tapped nor followed by a pool
//   ccvs_relu_maxpool2   nn.ReLU + nn.MaxPool2d(2, 2) of a pre-activation map in one read
//   ccvs_lpips_layer     one tapped layer's distance: channel-normalise both images' features (ReLU on read), weight the squared
//                        difference by the linear head, mean over the positions -- float64 per image
//
// The house style of metrics.hip: float64 accumulation, no float atomics, every partial sum written by one workgroup and added in a
// fixed order (the same bits on every run), 16-byte loads where the rows allow them.
#include "common.h"

// ---- prep ------------------------------------------------------------------------------------------------------------------------
struct LpipsNorm { float mean[3], std[3]; };

// item i is a quad of plane i / per_plane (VEC: HW % 4 == 0, so a quad never crosses a plane) or an element
template <bool VEC>
__global__ __launch_bounds__(256) void lpips_prep_kernel(const float* __restrict__ x, float* __restrict__ out, long items, long per_plane, LpipsNorm nm) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        const int c = (int)((i / per_plane) % 3);
        const float m = nm.mean[c], s = nm.std[c];
        if (VEC) {
            const float4 v = reinterpret_cast<const float4*>(x)[i];
            reinterpret_cast<float4*>(out)[i] = make_float4((v.x - m) / s, (v.y - m) / s, (v.z - m) / s, (v.w - m) / s);   // true divisions
        } else {
            out[i] = (x[i] - m) / s;
        }
    }
}

extern "C" int ccvs_lpips_prep(const float* x, float* out, int64_t planes, int64_t HW, const float* mean, const float* std, void* stream) {
    CCVS_REQUIRE(x && out && mean && std, "ccvs_lpips_prep: null pointer");
    CCVS_REQUIRE(planes > 0 && planes % 3 == 0 && HW > 0, "ccvs_lpips_prep: planes %ld (a multiple of 3), HW %ld", (long)planes, (long)HW);
    LpipsNorm nm;
    for (int c = 0; c < 3; ++c) { nm.mean[c] = mean[c]; nm.std[c] = std[c]; }
    const bool vec = HW % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const long per_plane = vec ? (long)HW / 4 : (long)HW, items = (long)planes * per_plane;
    const unsigned grid = strided_grid(items, stream, 8);
    if (vec) hipLaunchKernelGGL(lpips_prep_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, out, items, per_plane, nm);
    else hipLaunchKernelGGL(lpips_prep_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, out, items, per_plane, nm);
    CCVS_CHECK_LAUNCH("ccvs_lpips_prep");
    return CCVS_OK;
}

// ---- ReLU ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.f ? 0.f : v; }   // (NaN < 0 is false: a NaN stays)

// n4 quads from a 16-byte aligned base, then the elements behind the last whole quad; n4 = 0 when the base is not aligned
__global__ __launch_bounds__(256) void relu_kernel(float* __restrict__ x, long n, long n4) {
    const long first = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
    float4* x4 = reinterpret_cast<float4*>(x);
    for (long i = first; i < n4; i += step) {
        const float4 v = x4[i];
        x4[i] = make_float4(relu_keep_nan(v.x), relu_keep_nan(v.y), relu_keep_nan(v.z), relu_keep_nan(v.w));
    }
    for (long i = 4 * n4 + first; i < n; i += step) x[i] = relu_keep_nan(x[i]);
}

extern "C" int ccvs_relu_(float* x, int64_t n, void* stream) {
    CCVS_REQUIRE(x, "ccvs_relu_: null pointer");
    CCVS_REQUIRE(n > 0, "ccvs_relu_: no elements");
    const long n4 = (reinterpret_cast<uintptr_t>(x) & 15) == 0 ? (long)n / 4 : 0;
    const unsigned grid = strided_grid(n4 > 0 ? n4 : (long)n, stream, 8);
    hipLaunchKernelGGL(relu_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (long)n, n4);
    CCVS_CHECK_LAUNCH("ccvs_relu_");
    return CCVS_OK;
}

// ---- ReLU + 2 x 2 max pool -------------------------------------------------------------------------------------------------------
// torch's pool takes a value when it is larger than the running maximum OR is a NaN: a NaN in the window comes out
__device__ __forceinline__ float pool_take(float m, float v) { return (v > m || v != v) ? v : m; }
__device__ __forceinline__ float relu_pool4(float a, float b, float c, float d) {   // window in torch's order: row 0 left, right, row 1 left, right
    return relu_keep_nan(pool_take(pool_take(pool_take(a, b), c), d));
}

// VEC (W % 4 == 0 and 16-byte aligned bases: every input row starts on 16 bytes, every output row on 8): an item is two neighbouring
// output pixels -- two 16-byte loads, one 8-byte store.  Otherwise an item is one output pixel.
template <bool VEC>
__global__ __launch_bounds__(256) void relu_maxpool2_kernel(const float* __restrict__ x, float* __restrict__ out, long planes, int H, int W) {
    const int OH = H / 2, OW = W / 2, IW = VEC ? OW / 2 : OW;   // items per output row
    const long items = planes * OH * IW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        const int ix = (int)(i % IW);
        const long r = i / IW;
        const int oy = (int)(r % OH);
        const long pl = r / OH;
        const float* r0 = x + (pl * H + 2 * oy) * W;   // rows 2 oy and 2 oy + 1 <= H - 1
        const float* r1 = r0 + W;
        float* o = out + (pl * OH + oy) * OW;
        if (VEC) {
            const float4 a = reinterpret_cast<const float4*>(r0)[ix], b = reinterpret_cast<const float4*>(r1)[ix];
            reinterpret_cast<float2*>(o)[ix] = make_float2(relu_pool4(a.x, a.y, b.x, b.y), relu_pool4(a.z, a.w, b.z, b.w));
        } else {
            o[ix] = relu_pool4(r0[2 * ix], r0[2 * ix + 1], r1[2 * ix], r1[2 * ix + 1]);   // 2 ix + 1 <= 2 OW - 1 <= W - 1
        }
    }
}

extern "C" int ccvs_relu_maxpool2(const float* x, float* out, int64_t planes, int32_t H, int32_t W, void* stream) {
    CCVS_REQUIRE(x && out, "ccvs_relu_maxpool2: null pointer");
    CCVS_REQUIRE(planes > 0 && H >= 2 && W >= 2, "ccvs_relu_maxpool2: planes %ld of %d x %d (at least 2 x 2)", (long)planes, H, W);
    const bool vec = W % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const long items = (long)planes * (H / 2) * (vec ? W / 4 : W / 2);
    const unsigned grid = strided_grid(items, stream, 8);
    if (vec) hipLaunchKernelGGL(relu_maxpool2_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, out, (long)planes, H, W);
    else hipLaunchKernelGGL(relu_maxpool2_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, out, (long)planes, H, W);
    CCVS_CHECK_LAUNCH("ccvs_relu_maxpool2");
    return CCVS_OK;
}

// ---- the distance of one tapped layer --------------------------------------------------------------------------------------------
// f [2 M, C, HW].  A 256-thread workgroup owns image pair m = blockIdx.y and 64 PX consecutive positions: the lanes of a wave run along
// the positions (PX = 4: a 16-byte load per lane and channel, where HW % 4 == 0 and the base is 16-byte aligned; PX = 1 otherwise), so
// every channel plane is read in coalesced runs; the four waves share the channels, wave v taking c = v, v + 4, ...
//   pass 1  the waves' partial sums of a_c^2 and b_c^2 (float64) meet in LDS and are added in wave order: both channel norms;
//   pass 2  the same channels again -- from L2, as in l2_normalize_channels_kernel: a workgroup's slice is 2 C x 64 PX floats -- for
//           sum_c w[c] (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2 in float64.
// The lanes' sums are added by butterfly, the waves' in index order, and the workgroup writes ONE float64 partial part[m][tile]; the
// finish kernel adds an image's partials in a fixed order and divides by HW.  No atomics: the same bits on every run.
#define LP_EPS 1e-10

template <int PX> struct LpLoad;
template <> struct LpLoad<1> {
    static __device__ __forceinline__ void get(const float* p, float (&v)[1]) { v[0] = *p; }
};
template <> struct LpLoad<4> {
    static __device__ __forceinline__ void get(const float* p, float (&v)[4]) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
};

template <int PX, bool RELU>
__global__ __launch_bounds__(256) void lpips_layer_kernel(const float* __restrict__ f, const float* __restrict__ w, double* __restrict__ part, long M,
                                                           int C, long HW) {
    __shared__ double sq[4][2][PX][64];   // [wave][image][pixel of the lane][lane]
    __shared__ double wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long m = blockIdx.y;
    const long p0 = ((long)blockIdx.x * 64 + lane) * PX;   // PX = 4: HW % 4 == 0, the lane's four positions are inside the plane or all outside
    const bool in = p0 < HW;
    const float* fa = f + m * C * HW + p0;          // + c * HW
    const float* fb = f + (M + m) * C * HW + p0;

    double sa[PX], sb[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) sa[j] = sb[j] = 0.0;
    if (in) {
#pragma unroll 4
        for (int c = wave; c < C; c += 4) {
            float a[PX], b[PX];
            LpLoad<PX>::get(fa + (long)c * HW, a);
            LpLoad<PX>::get(fb + (long)c * HW, b);
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                const double u = RELU ? (double)relu_keep_nan(a[j]) : (double)a[j], v = RELU ? (double)relu_keep_nan(b[j]) : (double)b[j];
                sa[j] += u * u;
                sb[j] += v * v;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < PX; ++j) { sq[wave][0][j][lane] = sa[j]; sq[wave][1][j][lane] = sb[j]; }
    __syncthreads();
    double acc = 0.0;
    if (in) {
        double ia[PX], ib[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const double na = ((sq[0][0][j][lane] + sq[1][0][j][lane]) + sq[2][0][j][lane]) + sq[3][0][j][lane];
            const double nb = ((sq[0][1][j][lane] + sq[1][1][j][lane]) + sq[2][1][j][lane]) + sq[3][1][j][lane];
            ia[j] = sqrt(na) + LP_EPS;
            ib[j] = sqrt(nb) + LP_EPS;
        }
#pragma unroll 4
        for (int c = wave; c < C; c += 4) {
            float a[PX], b[PX];
            LpLoad<PX>::get(fa + (long)c * HW, a);
            LpLoad<PX>::get(fb + (long)c * HW, b);
            const double wc = (double)w[c];
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                const double u = RELU ? (double)relu_keep_nan(a[j]) : (double)a[j], v = RELU ? (double)relu_keep_nan(b[j]) : (double)b[j];
                const double d = u / ia[j] - v / ib[j];
                acc += wc * (d * d);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[m * gridDim.x + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// one wave per image: lane t adds the partials t, t + 64, ... in that order, the lanes meet by butterfly
__global__ __launch_bounds__(64) void lpips_layer_finish_kernel(const double* __restrict__ part, double* __restrict__ out, long tiles, double hw, int accumulate) {
    const double* p = part + (long)blockIdx.x * tiles;
    double acc = 0.0;
    for (long t = threadIdx.x; t < tiles; t += 64) acc += p[t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (threadIdx.x == 0) out[blockIdx.x] = accumulate ? out[blockIdx.x] + acc / hw : acc / hw;
}

// positions per lane of a call: 4 where every channel row splits into whole, 16-byte aligned quads
static inline int lpips_px(const float* f, int64_t HW) { return (HW % 4 == 0 && (reinterpret_cast<uintptr_t>(f) & 15) == 0) ? 4 : 1; }

extern "C" int64_t ccvs_lpips_layer_workspace_bytes(int64_t M, int64_t HW) {
    if (M <= 0 || M > 65535 || HW <= 0) return 0;
    return M * cdiv64(HW, 64) * (int64_t)sizeof(double);   // the one-position-per-lane tiling: the larger of the two
}

extern "C" int ccvs_lpips_layer(const float* f, const float* w, double* out, void* workspace, int64_t M, int32_t C, int64_t HW, int32_t relu,
                                int32_t accumulate, void* stream) {
    CCVS_REQUIRE(f && w && out && workspace, "ccvs_lpips_layer: null pointer");
    CCVS_REQUIRE(M > 0 && M <= 65535 && C > 0 && HW > 0, "ccvs_lpips_layer: 1 .. 65535 image pairs per call, C > 0, HW > 0; got M %ld, C %d, HW %ld", (long)M,
                 C, (long)HW);
    const int px = lpips_px(f, HW);
    const long tiles = cdiv64(HW, 64 * px);
    CCVS_REQUIRE(tiles < 2147483647L, "ccvs_lpips_layer: HW %ld too large", (long)HW);
    const dim3 grid((unsigned)tiles, (unsigned)M);
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)workspace;
#define LP_LAUNCH(PXv, RELUv) hipLaunchKernelGGL((lpips_layer_kernel<PXv, RELUv>), grid, dim3(256), 0, st, f, w, part, (long)M, C, (long)HW)
    if (px == 4) { if (relu) LP_LAUNCH(4, true); else LP_LAUNCH(4, false); }
    else { if (relu) LP_LAUNCH(1, true); else LP_LAUNCH(1, false); }
#undef LP_LAUNCH
    CCVS_CHECK_LAUNCH("ccvs_lpips_layer");
    hipLaunchKernelGGL(lpips_layer_finish_kernel, dim3((unsigned)M), dim3(64), 0, st, (const double*)part, out, tiles, (double)HW, accumulate ? 1 : 0);
    CCVS_CHECK_LAUNCH("ccvs_lpips_layer");
    return CCVS_OK;
}

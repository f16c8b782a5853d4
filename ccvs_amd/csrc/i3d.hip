// The passes of the FVD embedding (the Kinetics-400 RGB Inception-I3D of tools/tf_fvd/fvd.py) around its
// convolutions, which are ccvs_conv2d / ccvs_conv2d_bf16x3 as they stand.  Activations live as [N T, C, H, W]: frames are the batch.
//
//   ccvs_fvd_prep        uint8 clips -> TF1 resize_bilinear to 224 x 224 and 2 v / 255 - 1, channel-first, fp32 step by step
//   ccvs_time_unfold     the kt C time-stacked channels a kt-tap 3-D convolution reads as a 2-D one (SAME in time, zero borders, ReLU on read)
//   ccvs_maxpool3d_same  the network's max pools with TensorFlow's SAME geometry (padding never wins, ReLU on read)
//   ccvs_i3d_head        (2, 7, 7) average pool, logits and their mean over time, in float64
//
// The house style of lpips.hip / metrics.hip: float64 wherever something is summed, no float atomics, a fixed summation order (the
// same bits on every run), 16-byte accesses where the rows allow them.
#include "common.h"

__device__ __forceinline__ float i3d_relu(float v) { return v < 0.f ? 0.f : v; }   // (NaN < 0 is false: a NaN stays)
// torch's pools take a value when it is larger than the running maximum OR is a NaN
__device__ __forceinline__ float i3d_take(float m, float v) { return (v > m || v != v) ? v : m; }

// TensorFlow's SAME padding in front of an axis
static inline int same_out(int n, int s) { return (n + s - 1) / s; }
static inline int same_before(int n, int k, int s) {
    const int total = (same_out(n, s) - 1) * s + k - n;
    return total > 0 ? total / 2 : 0;
}
static inline bool aligned16(const void* a, const void* b) { return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0; }

// ---- preprocess ------------------------------------------------------------------------------------------------------------------
// an item is PX neighbouring output pixels of a row, all three channels (PX = 4: OW % 4 == 0 and a 16-byte aligned base: three 16-byte stores)
template <int PX>
__global__ __launch_bounds__(256) void fvd_prep_kernel(const uint8_t* __restrict__ u8, float* __restrict__ out, long frames, int H, int W, int OH, int OW,
                                                        float sy, float sx, int flip) {
#pragma clang fp contract(off)   // every product and sum rounds on its own, as TensorFlow's kernel and the numpy mirror do
    const int IW = OW / PX;
    const long items = frames * OH * IW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        const int ix = (int)(i % IW);
        const long r = i / IW;
        const int oy = (int)(r % OH);
        const long f = r / OH;
        const float srcy = (float)oy * sy;
        int y0 = (int)floorf(srcy);
        y0 = y0 < H - 1 ? y0 : H - 1;              // (never taken for src < H; keeps every read inside the frame)
        const int y1 = y0 + 1 < H - 1 ? y0 + 1 : H - 1;
        const float fy = srcy - (float)y0;
        const uint8_t* r0 = u8 + (f * H + y0) * (long)W * 3;
        const uint8_t* r1 = u8 + (f * H + y1) * (long)W * 3;
        float v[3][PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const float srcx = (float)(ix * PX + j) * sx;
            int x0 = (int)floorf(srcx);
            x0 = x0 < W - 1 ? x0 : W - 1;
            const int x1 = x0 + 1 < W - 1 ? x0 + 1 : W - 1;
            const float fx = srcx - (float)x0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int ci = flip ? 2 - c : c;
                const float tl = (float)r0[x0 * 3 + ci], tr = (float)r0[x1 * 3 + ci], bl = (float)r1[x0 * 3 + ci], br = (float)r1[x1 * 3 + ci];
                const float top = tl + (tr - tl) * fx;
                const float bot = bl + (br - bl) * fx;
                const float val = top + (bot - top) * fy;
                v[c][j] = (2.f * val) / 255.f - 1.f;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* o = out + ((f * 3 + c) * OH + oy) * (long)OW + (long)ix * PX;
            if (PX == 4) *reinterpret_cast<float4*>(o) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
            else o[0] = v[c][0];
        }
    }
}

extern "C" int ccvs_fvd_prep(const uint8_t* u8, float* out, int64_t frames, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t flip, void* stream) {
    CCVS_REQUIRE(u8 && out, "ccvs_fvd_prep: null pointer");
    CCVS_REQUIRE(frames > 0 && H > 0 && W > 0 && OH > 0 && OW > 0 && H <= 16384 && W <= 16384 && OH <= 16384 && OW <= 16384,
                 "ccvs_fvd_prep: %ld frames of %d x %d to %d x %d (every side 1 .. 16384)", (long)frames, H, W, OH, OW);
    const float sy = (float)H / (float)OH, sx = (float)W / (float)OW;
    const bool vec = OW % 4 == 0 && aligned16(out, out);
    const long items = (long)frames * OH * (vec ? OW / 4 : OW);
    const unsigned grid = strided_grid(items, stream, 8);
    if (vec) hipLaunchKernelGGL(fvd_prep_kernel<4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, u8, out, (long)frames, H, W, OH, OW, sy, sx, flip ? 1 : 0);
    else hipLaunchKernelGGL(fvd_prep_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, u8, out, (long)frames, H, W, OH, OW, sy, sx, flip ? 1 : 0);
    CCVS_CHECK_LAUNCH("ccvs_fvd_prep");
    return CCVS_OK;
}

// ---- time unfold -----------------------------------------------------------------------------------------------------------------
struct UnfoldGeom {
    long in_sN, in_sC;
    int T, To, C, H, W, kt, st, before, pt, pl, Ho, Wo, ps;   // Ho x Wo: an output plane, (H + pt + pb) / ps x (W + pl + pr) / ps
};

// VEC (no spatial border, ps 1, H W % 4 == 0, both strides % 4 == 0, 16-byte aligned bases): an item is a quad of a plane -- one 16-byte
// load (or none: a frame outside the clip), one 16-byte store.  Otherwise an item is one output element; with ps = 2 output channel
// (j C + c) 4 + 2 py + px holds the bordered frame's pixels (2 y + py, 2 x + px).
template <bool VEC, bool RELU>
__global__ __launch_bounds__(256) void time_unfold_kernel(const float* __restrict__ x, float* __restrict__ out, long items, UnfoldGeom g) {
    const long per_plane = VEC ? (long)g.Ho * g.Wo / 4 : (long)g.Ho * g.Wo;
    const int pp = g.ps * g.ps, KC = g.kt * g.C * pp;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        const long q = i % per_plane, r = i / per_plane;
        const int ch = (int)(r % KC);
        const long fo = r / KC;
        const int jc = ch / pp, ph = ch - jc * pp;
        const int j = jc / g.C, c = jc - j * g.C;
        const long n = fo / g.To;
        const int t = (int)(fo - n * g.To) * g.st + j - g.before;     // the frame of clip n this channel block shows; outside the clip: zeros
        const bool live = t >= 0 && t < g.T;
        const float* src = x + (n * g.T + (live ? t : 0)) * g.in_sN + (long)c * g.in_sC;
        if (VEC) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live) {
                v = reinterpret_cast<const float4*>(src)[q];
                if (RELU) v = make_float4(i3d_relu(v.x), i3d_relu(v.y), i3d_relu(v.z), i3d_relu(v.w));
            }
            reinterpret_cast<float4*>(out)[i] = v;
        } else {
            const int oy = (int)(q / g.Wo), ox = (int)(q - (long)oy * g.Wo);
            const int yy = oy * g.ps + ph / g.ps - g.pt, xx = ox * g.ps + ph % g.ps - g.pl;
            float v = 0.f;
            if (live && yy >= 0 && yy < g.H && xx >= 0 && xx < g.W) {
                v = src[(long)yy * g.W + xx];
                if (RELU) v = i3d_relu(v);
            }
            out[i] = v;
        }
    }
}

extern "C" int ccvs_time_unfold(const float* x, int64_t in_sN, int64_t in_sC, float* out, int32_t clips, int32_t T, int32_t C, int32_t H, int32_t W,
                                int32_t kt, int32_t st, int32_t pt, int32_t pb, int32_t pl, int32_t pr, int32_t phases, int32_t relu, void* stream) {
    CCVS_REQUIRE(x && out, "ccvs_time_unfold: null pointer");
    CCVS_REQUIRE(clips > 0 && T > 0 && C > 0 && H > 0 && W > 0, "ccvs_time_unfold: empty tensor (clips %d, T %d, C %d, %d x %d)", clips, T, C, H, W);
    CCVS_REQUIRE(kt >= 1 && kt <= 7 && (st == 1 || st == 2), "ccvs_time_unfold: kt %d (1 .. 7), st %d (1 or 2)", kt, st);
    CCVS_REQUIRE(pt >= 0 && pb >= 0 && pl >= 0 && pr >= 0 && pt <= 8 && pb <= 8 && pl <= 8 && pr <= 8, "ccvs_time_unfold: borders %d %d %d %d (0 .. 8)", pt, pb,
                 pl, pr);
    CCVS_REQUIRE(phases == 1 || (phases == 2 && (H + pt + pb) % 2 == 0 && (W + pl + pr) % 2 == 0),
                 "ccvs_time_unfold: phases %d (1, or 2 on a bordered frame of even sides; got %d x %d)", phases, H + pt + pb, W + pl + pr);
    CCVS_REQUIRE(in_sC >= (int64_t)H * W && in_sN >= in_sC * C, "ccvs_time_unfold: strides %ld / %ld under a dense [C, H, W] frame", (long)in_sN, (long)in_sC);
    UnfoldGeom g;
    g.in_sN = (long)in_sN; g.in_sC = (long)in_sC;
    g.T = T; g.To = same_out(T, st); g.C = C; g.H = H; g.W = W; g.kt = kt; g.st = st; g.before = same_before(T, kt, st);
    g.pt = pt; g.pl = pl; g.ps = phases; g.Ho = (H + pt + pb) / phases; g.Wo = (W + pl + pr) / phases;
    const long hw = (long)g.Ho * g.Wo;
    const bool vec = pt + pb + pl + pr == 0 && phases == 1 && hw % 4 == 0 && in_sN % 4 == 0 && in_sC % 4 == 0 && aligned16(x, out);
    const long items = (long)clips * g.To * kt * C * phases * phases * (vec ? hw / 4 : hw);
    const unsigned grid = strided_grid(items, stream, 8);
    hipStream_t s = (hipStream_t)stream;
#define TU_LAUNCH(VECv, RELUv) hipLaunchKernelGGL((time_unfold_kernel<VECv, RELUv>), dim3(grid), dim3(256), 0, s, x, out, items, g)
    if (vec) { if (relu) TU_LAUNCH(true, true); else TU_LAUNCH(true, false); }
    else { if (relu) TU_LAUNCH(false, true); else TU_LAUNCH(false, false); }
#undef TU_LAUNCH
    CCVS_CHECK_LAUNCH("ccvs_time_unfold");
    return CCVS_OK;
}

// ---- max pool, SAME ----------------------------------------------------------------------------------------------------------------
struct PoolGeom {
    int T, C, H, W, To, Ho, Wo, kt, kh, kw, st, sh, sw, bt, bh, bw;
};

// one output element per item; the window is clipped to the clip's frames and the frame's rows and columns (SAME padding never wins),
// and is never empty: before <= k - 1.  Walked in torch's order (time, row, column).
template <bool RELU>
__global__ __launch_bounds__(256) void maxpool3d_same_kernel(const float* __restrict__ x, float* __restrict__ out, long items, PoolGeom g) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        const int ox = (int)(i % g.Wo);
        long r = i / g.Wo;
        const int oy = (int)(r % g.Ho);
        r /= g.Ho;
        const int c = (int)(r % g.C);
        const long fo = r / g.C;
        const long n = fo / g.To;
        const int to = (int)(fo - n * g.To);
        const int t0 = to * g.st - g.bt, y0 = oy * g.sh - g.bh, x0 = ox * g.sw - g.bw;
        const int ta = t0 > 0 ? t0 : 0, tb = t0 + g.kt < g.T ? t0 + g.kt : g.T;
        const int ya = y0 > 0 ? y0 : 0, yb = y0 + g.kh < g.H ? y0 + g.kh : g.H;
        const int xa = x0 > 0 ? x0 : 0, xb = x0 + g.kw < g.W ? x0 + g.kw : g.W;
        float m = -INFINITY;
        for (int t = ta; t < tb; ++t) {
            const float* plane = x + ((n * g.T + t) * g.C + c) * (long)g.H * g.W;
            for (int y = ya; y < yb; ++y)
                for (int xx = xa; xx < xb; ++xx) {
                    const float v = plane[(long)y * g.W + xx];
                    m = i3d_take(m, RELU ? i3d_relu(v) : v);
                }
        }
        out[i] = m;
    }
}

extern "C" int ccvs_maxpool3d_same(const float* x, float* out, int32_t clips, int32_t T, int32_t C, int32_t H, int32_t W, int32_t kt, int32_t kh,
                                   int32_t kw, int32_t st, int32_t sh, int32_t sw, int32_t relu, void* stream) {
    CCVS_REQUIRE(x && out, "ccvs_maxpool3d_same: null pointer");
    CCVS_REQUIRE(clips > 0 && T > 0 && C > 0 && H > 0 && W > 0, "ccvs_maxpool3d_same: empty tensor (clips %d, T %d, C %d, %d x %d)", clips, T, C, H, W);
    const bool kernel_ok = (kt == 1 && kh == 3 && kw == 3) || (kt == 3 && kh == 3 && kw == 3) || (kt == 2 && kh == 2 && kw == 2);
    const bool stride_ok = (st == 1 && sh == 2 && sw == 2) || (st == 2 && sh == 2 && sw == 2) || (st == 1 && sh == 1 && sw == 1);
    CCVS_REQUIRE(kernel_ok && stride_ok, "ccvs_maxpool3d_same: kernel (%d,%d,%d) stride (%d,%d,%d): kernels (1,3,3) (3,3,3) (2,2,2), strides (1,2,2) (2,2,2) (1,1,1)",
                 kt, kh, kw, st, sh, sw);
    PoolGeom g;
    g.T = T; g.C = C; g.H = H; g.W = W;
    g.To = same_out(T, st); g.Ho = same_out(H, sh); g.Wo = same_out(W, sw);
    g.kt = kt; g.kh = kh; g.kw = kw; g.st = st; g.sh = sh; g.sw = sw;
    g.bt = same_before(T, kt, st); g.bh = same_before(H, kh, sh); g.bw = same_before(W, kw, sw);
    const long items = (long)clips * g.To * C * g.Ho * g.Wo;
    const unsigned grid = strided_grid(items, stream, 8);
    if (relu) hipLaunchKernelGGL(maxpool3d_same_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, out, items, g);
    else hipLaunchKernelGGL(maxpool3d_same_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, out, items, g);
    CCVS_CHECK_LAUNCH("ccvs_maxpool3d_same");
    return CCVS_OK;
}

// ---- head --------------------------------------------------------------------------------------------------------------------------
// One 256-thread workgroup per clip.  Phase 1: wave v takes the channels v, v + 4, ...; its lanes run along the HW positions of a plane
// (coalesced), frame after frame, each frame weighted by the number of (2, H, W) windows it lies in (1 at the clip's ends, 2 inside);
// the lanes meet by butterfly and p[c] = sum / (2 HW (T - 1)) goes to LDS.  Phase 2: wave v takes the logits v, v + 4, ...; lane l adds
// w[k][c] p[c] for c = l, l + 64, ... in that order, the lanes meet by butterfly.  All float64, no atomics: the same bits on every run.
#define I3D_HEAD_MAX_C 4096
template <bool RELU>
__global__ __launch_bounds__(256) void i3d_head_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                        double* __restrict__ out, int T, int C, int HW, int K) {
    __shared__ double p[I3D_HEAD_MAX_C];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long n = blockIdx.x;
    const float* xc = x + n * T * (long)C * HW;
    const double inv = 1.0 / (2.0 * (double)HW * (double)(T - 1));
    for (int c = wave; c < C; c += 4) {
        double acc = 0.0;
        for (int t = 0; t < T; ++t) {
            const float* plane = xc + ((long)t * C + c) * HW;
            const double wt = (t == 0 || t == T - 1) ? 1.0 : 2.0;
            for (int q = lane; q < HW; q += 64) {
                const float v = plane[q];
                acc += wt * (double)(RELU ? i3d_relu(v) : v);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) p[c] = acc * inv;
    }
    __syncthreads();
    for (int k = wave; k < K; k += 4) {
        const float* wk = w + (long)k * C;
        double acc = 0.0;
        for (int c = lane; c < C; c += 64) acc += (double)wk[c] * p[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) out[n * K + k] = acc + (double)b[k];
    }
}

extern "C" int ccvs_i3d_head(const float* x, const float* w, const float* b, double* out, int32_t clips, int32_t T, int32_t C, int32_t HW, int32_t K,
                             int32_t relu, void* stream) {
    CCVS_REQUIRE(x && w && b && out, "ccvs_i3d_head: null pointer");
    CCVS_REQUIRE(clips > 0 && T >= 2 && C > 0 && C <= I3D_HEAD_MAX_C && HW > 0 && K > 0,
                 "ccvs_i3d_head: clips %d, T %d (at least 2: one average-pool window), C %d (1 .. %d), HW %d, K %d", clips, T, C, I3D_HEAD_MAX_C, HW, K);
    if (relu) hipLaunchKernelGGL(i3d_head_kernel<true>, dim3((unsigned)clips), dim3(256), 0, (hipStream_t)stream, x, w, b, out, T, C, HW, K);
    else hipLaunchKernelGGL(i3d_head_kernel<false>, dim3((unsigned)clips), dim3(256), 0, (hipStream_t)stream, x, w, b, out, T, C, HW, K);
    CCVS_CHECK_LAUNCH("ccvs_i3d_head");
    return CCVS_OK;
}

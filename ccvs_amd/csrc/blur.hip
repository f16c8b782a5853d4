// Gaussian blur of the deblurring mode: torchvision's GaussianBlur (helpers/generator.py:381-390 `blur`) -- reflect padding of k / 2 on
// every side, then the k x k depthwise filter outer(w, w) -- as two 1-D passes through LDS.  HBM-bound: 4 bytes read and 4 written per
// output pixel (the halo is re-read from L2 by the neighbouring tiles).
//
// ccvs_gaussian_blur <- transforms.GaussianBlur(kernel_size=k, sigma=s)(img), img [N, C, H, W] fp32, k odd in 3 .. 13.
#include "common.h"

#define GB_TH 32     // output rows of a tile
#define GB_TW 64     // output columns of a tile
#define GB_MAXK 13

struct GaussK {
    const float* x;
    float* y;
    long x_sN, x_sC;
    int C, H, W, tiles_x;
    float w[GB_MAXK];
};

// torch.nn.functional.pad(mode="reflect") index for i in [-(n-1), 2(n-1)]; the clamp only keeps the loads of halo cells no output
// reads (the tile's overhang past the plane) inside the plane
__device__ __forceinline__ int reflect_idx(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

// A 256-thread workgroup owns a 32 x 64 output tile of one plane.  Its (32 + 2R) x (64 + 2R) input window is staged in LDS once (reflected
// addresses, 16 bytes per lane where four columns lie inside the row), the horizontal pass writes (32 + 2R) x 64 row sums to a second
// LDS buffer, and each thread produces two rows of four consecutive outputs from it, written as 16-byte stores.
template <int R>
__global__ __launch_bounds__(256) void gaussian_blur_kernel(GaussK p, GridWalk gw) {
    constexpr int K = 2 * R + 1;
    constexpr int IH = GB_TH + 2 * R;
    constexpr int IQ = (GB_TW + 2 * R + 3) / 4;   // quads per staged row
    constexpr int IWp = 4 * IQ + 4;                // (+4: rows of consecutive lanes start on different banks)
    constexpr int HWp = GB_TW + 4;
    __shared__ __attribute__((aligned(16))) float tile[IH * IWp];
    __shared__ __attribute__((aligned(16))) float hrow[IH * HWp];
    const int tid = threadIdx.x;
    float w[K];
#pragma unroll
    for (int j = 0; j < K; ++j) w[j] = p.w[j];
    GRID_WALK_BEGIN(gw, bx, by, bz)
    (void)bz;
    const int ty = bx / p.tiles_x, tx = bx - ty * p.tiles_x;
    const int n = by / p.C, c = by - n * p.C;
    if (w_ != (long)blockIdx.x) __syncthreads();   // persistent walk: the previous tile's buffers have been read by everyone
    const float* xp = p.x + n * p.x_sN + c * p.x_sC;
    const int iy0 = ty * GB_TH - R, ix0 = tx * GB_TW - R;
    for (int e = tid; e < IH * IQ; e += 256) {
        const int r = e / IQ, q = (e - r * IQ) * 4;
        const int iy = reflect_idx(iy0 + r, p.H), ix = ix0 + q;
        const float* row = xp + (long)iy * p.W;
        f32x4 t4;
        if (ix >= 0 && ix + 3 < p.W) {
            const F32Quad v = *reinterpret_cast<const F32Quad*>(row + ix);
            t4 = f32x4{v.v[0], v.v[1], v.v[2], v.v[3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) t4[j] = row[reflect_idx(ix + j, p.W)];
        }
        *reinterpret_cast<f32x4*>(&tile[r * IWp + q]) = t4;
    }
    __syncthreads();
    // horizontal pass: four consecutive row sums per item, taps in torch's order (left to right)
    for (int e = tid; e < IH * (GB_TW / 4); e += 256) {
        const int r = e / (GB_TW / 4), q = (e - r * (GB_TW / 4)) * 4;
        const float* src = &tile[r * IWp + q];
        float a[4 + 2 * R];
#pragma unroll
        for (int j = 0; j < 4 + 2 * R; ++j) a[j] = src[j];
        f32x4 h;
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < K; ++j) s = fmaf(w[j], a[o + j], s);
            h[o] = s;
        }
        *reinterpret_cast<f32x4*>(&hrow[r * HWp + q]) = h;
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < GB_TH / 16; ++rr) {
        const int row = (tid >> 4) + 16 * rr, col = (tid & 15) * 4;
        const int oy = ty * GB_TH + row, ox0 = tx * GB_TW + col;
        if (oy < p.H && ox0 < p.W) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const f32x4 h = *reinterpret_cast<const f32x4*>(&hrow[(row + j) * HWp + col]);
#pragma unroll
                for (int o = 0; o < 4; ++o) s[o] = fmaf(w[j], h[o], s[o]);
            }
            float* yp = p.y + ((long)by * p.H + oy) * p.W + ox0;
            const int nv = min(4, p.W - ox0);
            if (nv == 4) {   // 16-byte store at any dword alignment (odd widths)
                F32Quad o4;
#pragma unroll
                for (int o = 0; o < 4; ++o) o4.v[o] = s[o];
                *reinterpret_cast<F32Quad*>(yp) = o4;
            } else {
                for (int o = 0; o < nv; ++o) yp[o] = s[o];
            }
        }
    }
    GRID_WALK_END
}

extern "C" int ccvs_gaussian_blur(const float* x, int64_t x_sN, int64_t x_sC, float* y, int32_t N, int32_t C, int32_t H, int32_t W,
                                  int32_t k, const float* weights, void* stream) {
    CCVS_REQUIRE(x && y && weights, "ccvs_gaussian_blur: null pointer");
    CCVS_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "ccvs_gaussian_blur: empty tensor");
    CCVS_REQUIRE(k >= 3 && k <= GB_MAXK && (k & 1), "ccvs_gaussian_blur: kernel size %d (odd, 3 .. %d)", k, GB_MAXK);
    CCVS_REQUIRE(k / 2 < H && k / 2 < W, "ccvs_gaussian_blur: reflect padding %d needs a plane larger than %d x %d", k / 2, H, W);
    GaussK p;
    p.x = x; p.y = y; p.x_sN = x_sN; p.x_sC = x_sC; p.C = C; p.H = H; p.W = W;
    for (int j = 0; j < GB_MAXK; ++j) p.w[j] = j < k ? weights[j] : 0.f;
    p.tiles_x = cdiv(W, GB_TW);
    const GridWalk gw = grid_walk((long)p.tiles_x * cdiv(H, GB_TH), (long)N * C, 1);
    const unsigned grid = limited_grid(gw.total, stream, 8);
    hipStream_t st = (hipStream_t)stream;
    switch (k / 2) {
        case 1: hipLaunchKernelGGL(gaussian_blur_kernel<1>, dim3(grid), dim3(256), 0, st, p, gw); break;
        case 2: hipLaunchKernelGGL(gaussian_blur_kernel<2>, dim3(grid), dim3(256), 0, st, p, gw); break;
        case 3: hipLaunchKernelGGL(gaussian_blur_kernel<3>, dim3(grid), dim3(256), 0, st, p, gw); break;
        case 4: hipLaunchKernelGGL(gaussian_blur_kernel<4>, dim3(grid), dim3(256), 0, st, p, gw); break;
        case 5: hipLaunchKernelGGL(gaussian_blur_kernel<5>, dim3(grid), dim3(256), 0, st, p, gw); break;
        default: hipLaunchKernelGGL(gaussian_blur_kernel<6>, dim3(grid), dim3(256), 0, st, p, gw); break;
    }
    CCVS_CHECK_LAUNCH("ccvs_gaussian_blur");
    return CCVS_OK;
}

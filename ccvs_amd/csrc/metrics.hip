// Evaluation metrics on the clips the path produces (tools/pytorch_metrics/metrics.py:15-25).
//
//   get_psnr -> piq.psnr(x, y, data_range=1., reduction='mean')                  (piq 0.5.4, env.yml:234)
//   get_ssim -> skimage.metrics.structural_similarity(x[i, c], y[i, c]) per 2-D plane, defaults of scikit-image 0.17.2
//               (env.yml:164): 7 x 7 uniform window, sample covariance (49 / 48), K1 = 0.01, K2 = 0.03, data_range taken from
//               the dtype (float: 2), computed in float64, mean over the windows that lie inside the plane.
//
// Both are HBM-bound reductions: every pixel is read once (the SSIM tile re-reads a 3-pixel halo through L2).
#include "common.h"

// ---- PSNR / MSE ------------------------------------------------------------------------------
// the lanes' float64 partial sums of one 1024-thread workgroup: per wave, then the 16 waves in index order (the same bits on every
// run).  The total is valid in thread 0.
__device__ __forceinline__ double block_sum_f64(double acc) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    __shared__ double part[16];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < 16; ++w) s += part[w];   // fixed order: the same bits on every run
    return s;
}

// sum ((x - y) * inv_range)^2 over `count` elements by one 1024-thread workgroup, in float64 (`block_sum_f64`).
__device__ __forceinline__ double block_sum_sq_diff(const float* __restrict__ x, const float* __restrict__ y, long count, double inv_range) {
    double acc = 0.0;
    const long n4 = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0 ? count / 4 : 0;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    const float4* y4 = reinterpret_cast<const float4*>(y);
    for (long i = threadIdx.x; i < n4; i += 1024) {
        const float4 a = x4[i], b = y4[i];
        const double d0 = ((double)a.x - (double)b.x) * inv_range, d1 = ((double)a.y - (double)b.y) * inv_range;
        const double d2 = ((double)a.z - (double)b.z) * inv_range, d3 = ((double)a.w - (double)b.w) * inv_range;
        acc += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
    }
    for (long i = 4 * n4 + threadIdx.x; i < count; i += 1024) {
        const double d = ((double)x[i] - (double)y[i]) * inv_range;
        acc += d * d;
    }
    return block_sum_f64(acc);
}

// one workgroup per image: score = -10 log10(mse / R^2 + 1e-8)
__global__ __launch_bounds__(1024) void psnr_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ out, long per_image,
                                                     double inv_range) {
    const long base = (long)blockIdx.x * per_image;
    const double s = block_sum_sq_diff(x + base, y + base, per_image, inv_range);
    if (threadIdx.x == 0) out[blockIdx.x] = (float)(-10.0 * log10(s / (double)per_image + 1e-8));
}

// F.mse_loss(a, b) (reduction 'mean') of n fp32 elements into one fp32: the float64 sum rounded once.  One workgroup -- the figures
// this serves are validation scalars over a clip's spectrograms or states, a few MB at most.
__global__ __launch_bounds__(1024) void mse_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, long n) {
    const double s = block_sum_sq_diff(a, b, n, 1.0);
    if (threadIdx.x == 0) out[0] = (float)(s / (double)n);
}

extern "C" int ccvs_psnr(const float* x, const float* y, float* out, int64_t N, int64_t per_image, float data_range, void* stream) {
    CCVS_REQUIRE(x && y && out, "ccvs_psnr: null pointer");
    CCVS_REQUIRE(N > 0 && N < 2147483647L && per_image > 0 && data_range > 0.f, "ccvs_psnr: bad arguments");
    hipLaunchKernelGGL(psnr_kernel, dim3((unsigned)N), dim3(1024), 0, (hipStream_t)stream, x, y, out, (long)per_image, 1.0 / (double)data_range);
    CCVS_CHECK_LAUNCH("ccvs_psnr");
    return CCVS_OK;
}

extern "C" int ccvs_mse(const float* a, const float* b, float* out, int64_t n, void* stream) {
    CCVS_REQUIRE(a && b && out, "ccvs_mse: null pointer");
    CCVS_REQUIRE(n > 0, "ccvs_mse: no elements");
    hipLaunchKernelGGL(mse_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a, b, out, (long)n);
    CCVS_CHECK_LAUNCH("ccvs_mse");
    return CCVS_OK;
}

// ---- teacher-forced NLL (transformer_model.py:229,239: F.cross_entropy over selected rows of the logits) -----------------------
// nll[m] = logsumexp(row[0 : ncols]) - row[target[m]] for row = logits + rows[m] * ld.  HBM-bound: a row's logits are loaded ONCE into
// registers (columns past ncols stand as -inf and are never read), the maximum and the sum of exp(x - max) are taken from the
// registers, so a row of 16384 fp32 is 64 registers per lane of a 256-thread workgroup.  A team of lanes owns a row:
//   ONE_WAVE  a wave per row, four rows per workgroup, 4 * NQ = 16 logits per lane (ncols <= 1024): no LDS, no barrier -- the
//             BAIR vocabulary and the state heads, where a workgroup per row would leave 4 KB in flight per workgroup;
//   otherwise a 256-thread workgroup per row, 4 * NQ = 16 or 64 logits per lane (ncols <= 4096 / 16384), the four waves' partial
//             results through LDS, combined as (w0 . w1) . (w2 . w3).
// VEC: 16-byte loads, lane t taking quads t, t + team, ...; a quad that crosses ncols is read column by column.  Not VEC (ld % 4 != 0
// or an unaligned base): 4-byte loads, lane t taking columns t, t + team, ... -- coalesced all the same.
// The butterfly and the fixed LDS order make the result the same bits on every run; there are no atomics.
// exp is v_exp_f32 (__expf): a term e^d, d <= 0, is off by |d| * 6e-8 of itself, so the sum by at most max(|d| e^d) * 6e-8 = 2e-8 of
// itself -- below the rounding of the fp32 sum.
template <int NQ, bool VEC, int TEAM>
__device__ __forceinline__ void nll_load_row(const float* __restrict__ row, int ncols, int t, float (&v)[4 * NQ]) {
    if (VEC) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int c = 4 * (t + TEAM * j);
            if (c + 3 < ncols) {
                const float4 a = *reinterpret_cast<const float4*>(row + c);
                v[4 * j] = a.x; v[4 * j + 1] = a.y; v[4 * j + 2] = a.z; v[4 * j + 3] = a.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[4 * j + e] = c + e < ncols ? row[c + e] : -INFINITY;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4 * NQ; ++k) {
            const int c = t + TEAM * k;
            v[k] = c < ncols ? row[c] : -INFINITY;
        }
    }
}

template <int NQ, bool VEC, bool ONE_WAVE>
__global__ __launch_bounds__(256) void token_nll_kernel(const float* __restrict__ logits, long ld, const int* __restrict__ rows,
                                                         const int64_t* __restrict__ target, long n_rows, int ncols, float* __restrict__ nll) {
    constexpr int TEAM = ONE_WAVE ? 64 : 256;
    __shared__ float wmax[4], wsum[4];
    const int t = threadIdx.x & (TEAM - 1), wave = threadIdx.x >> 6;
    const long m = ONE_WAVE ? (long)blockIdx.x * 4 + wave : (long)blockIdx.x;
    if (ONE_WAVE && m >= n_rows) return;   // a whole wave leaves; this form has no barrier
    const float* row = logits + (long)(rows ? rows[m] : m) * ld;
    const int64_t tgt = target[m];
    const bool ok = tgt >= 0 && tgt < ncols;   // outside: NaN, and nothing is read for it
    const float xt = ok && t == 0 ? row[tgt] : 0.f;
    float v[4 * NQ];
    nll_load_row<NQ, VEC, TEAM>(row, ncols, t, v);
    float mx = v[0];
#pragma unroll
    for (int k = 1; k < 4 * NQ; ++k) mx = fmaxf(mx, v[k]);
    mx = wave_max(mx);
    if (!ONE_WAVE) {
        if ((threadIdx.x & 63) == 0) wmax[wave] = mx;
        __syncthreads();
        mx = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4 * NQ; ++k) s += __expf(v[k] - mx);   // -inf (a masked logit, a column past ncols) adds 0
    s = wave_sum(s);
    if (!ONE_WAVE) {
        if ((threadIdx.x & 63) == 0) wsum[wave] = s;
        __syncthreads();
        s = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    }
    if (t == 0) nll[m] = ok ? logf(s) + (mx - xt) : __builtin_nanf("");
}

template <int NQ, bool ONE_WAVE>
static void launch_token_nll(bool vec, const float* logits, long ld, const int* rows, const int64_t* target, long n_rows, int ncols, float* nll,
                             hipStream_t stream) {
    const dim3 grid((unsigned)(ONE_WAVE ? cdiv64(n_rows, 4) : n_rows));
    if (vec)
        hipLaunchKernelGGL((token_nll_kernel<NQ, true, ONE_WAVE>), grid, dim3(256), 0, stream, logits, ld, rows, target, n_rows, ncols, nll);
    else
        hipLaunchKernelGGL((token_nll_kernel<NQ, false, ONE_WAVE>), grid, dim3(256), 0, stream, logits, ld, rows, target, n_rows, ncols, nll);
}

extern "C" int ccvs_token_nll(const float* logits, int64_t ld, const int32_t* rows, const int64_t* target, int64_t n_rows, int32_t ncols, float* nll,
                              void* stream) {
    CCVS_REQUIRE(logits && target && nll, "ccvs_token_nll: null pointer");
    CCVS_REQUIRE(n_rows > 0 && n_rows < 2147483647L, "ccvs_token_nll: 1 .. 2^31 - 2 rows per call");
    CCVS_REQUIRE(ncols > 0 && ncols <= 16384 && ld >= ncols, "ccvs_token_nll: 1 <= ncols <= 16384 (a row is held in registers), ncols <= ld; got ncols %d, ld %ld",
                 ncols, (long)ld);
    const bool vec = (reinterpret_cast<uintptr_t>(logits) & 15) == 0 && ld % 4 == 0;   // every row starts on 16 bytes
    if (ncols <= 1024)
        launch_token_nll<4, true>(vec, logits, (long)ld, rows, target, (long)n_rows, ncols, nll, (hipStream_t)stream);
    else if (ncols <= 4096)
        launch_token_nll<4, false>(vec, logits, (long)ld, rows, target, (long)n_rows, ncols, nll, (hipStream_t)stream);
    else
        launch_token_nll<16, false>(vec, logits, (long)ld, rows, target, (long)n_rows, ncols, nll, (hipStream_t)stream);
    CCVS_CHECK_LAUNCH("ccvs_token_nll");
    return CCVS_OK;
}

// mean of n fp32 into one fp32: float64 sums in index order by one workgroup, rounded once (the shape of mse_kernel).  A NaN element
// gives a NaN mean.
__global__ __launch_bounds__(1024) void mean_kernel(const float* __restrict__ x, float* __restrict__ out, long n) {
    double acc = 0.0;
    for (long i = threadIdx.x; i < n; i += 1024) acc += (double)x[i];
    const double s = block_sum_f64(acc);
    if (threadIdx.x == 0) out[0] = (float)(s / (double)n);
}

extern "C" int ccvs_mean_f32(const float* x, int64_t n, float* out, void* stream) {
    CCVS_REQUIRE(x && out, "ccvs_mean_f32: null pointer");
    CCVS_REQUIRE(n > 0, "ccvs_mean_f32: no elements");
    hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, x, out, (long)n);
    CCVS_CHECK_LAUNCH("ccvs_mean_f32");
    return CCVS_OK;
}

// ---- frame autoencoder validation (quantized_video_model.py:460-480, quantize.py:59-68) ------------------------------------------
// Three HBM-bound reductions behind `eval_img_to_img_generator`: the L1 between a frame batch and its reconstruction, the quantiser's
// loss term with the code histogram, and the perplexity of that histogram.  float64 inside, no float atomics, every partial sum
// written by one workgroup and added in a fixed order: the same bits on every run.

// torch.mean(torch.abs(a - b)), stage 1: workgroup g of G adds |a[i] - b[i]| over the quads g * 1024 + t, (g + G) * 1024 + t, ...
// (16-byte loads where both bases are 16-byte aligned) and over the elements behind the last whole quad -- all of them when a base is
// not aligned -- with the same stride, and writes one float64 partial.  G is a function of n alone (`l1_groups`).
#define L1_PER_GROUP 16384   // elements a workgroup is given before another one is launched: 4 quads per lane
#define L1_MAX_GROUPS 1024
static inline long l1_groups(long n) {
    const long g = cdiv64(n, L1_PER_GROUP);
    return g < 1 ? 1 : (g > L1_MAX_GROUPS ? L1_MAX_GROUPS : g);
}

__global__ __launch_bounds__(1024) void l1_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, double* __restrict__ part, long n) {
    double acc = 0.0;
    const long n4 = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0 ? n / 4 : 0;
    const float4* a4 = reinterpret_cast<const float4*>(a);
    const float4* b4 = reinterpret_cast<const float4*>(b);
    const long first = (long)blockIdx.x * 1024 + threadIdx.x, step = (long)gridDim.x * 1024;
    for (long i = first; i < n4; i += step) {
        const float4 u = a4[i], v = b4[i];
        acc += (fabs((double)u.x - (double)v.x) + fabs((double)u.y - (double)v.y)) + (fabs((double)u.z - (double)v.z) + fabs((double)u.w - (double)v.w));
    }
    for (long i = 4 * n4 + first; i < n; i += step) acc += fabs((double)a[i] - (double)b[i]);
    const double s = block_sum_f64(acc);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// stage 2 of a two-stage mean: `count` (<= 1024) float64 partials through LDS, added by thread 0 in index order, divided by n and
// rounded once to fp32.  A NaN partial gives NaN.
__global__ __launch_bounds__(1024) void partials_mean_kernel(const double* __restrict__ part, int count, double n, float* __restrict__ out) {
    __shared__ double p[1024];
    if ((int)threadIdx.x < count) p[threadIdx.x] = part[threadIdx.x];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int g = 0; g < count; ++g) s += p[g];
    out[0] = (float)(s / n);
}

extern "C" int64_t ccvs_l1_workspace_bytes(int64_t n) { return n > 0 ? l1_groups((long)n) * (int64_t)sizeof(double) : 0; }

extern "C" int ccvs_l1_mean(const float* a, const float* b, float* out, void* workspace, int64_t n, void* stream) {
    CCVS_REQUIRE(a && b && out && workspace, "ccvs_l1_mean: null pointer");
    CCVS_REQUIRE(n > 0, "ccvs_l1_mean: no elements");
    const long groups = l1_groups((long)n);
    hipLaunchKernelGGL(l1_partial_kernel, dim3((unsigned)groups), dim3(1024), 0, (hipStream_t)stream, a, b, (double*)workspace, (long)n);
    CCVS_CHECK_LAUNCH("ccvs_l1_mean");
    hipLaunchKernelGGL(partials_mean_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const double*)workspace, (int)groups, (double)n, out);
    CCVS_CHECK_LAUNCH("ccvs_l1_mean");
    return CCVS_OK;
}

// The quantiser's statistics.  z [N, C, HW] is read once: a 256-thread workgroup owns 64 consecutive positions p = n * HW + hw (the
// lanes of a wave: every channel row of z is read as coalesced runs) and VQ_CB consecutive channels, which its four waves share in
// blocks of four -- wave w takes the channels c0 + 4 (w + 4 j) .. + 3.  A lane gathers its code's four entries of those channels with
// one 16-byte load where the codebook allows it (C % 4 == 0, 16-byte aligned base), entry by entry otherwise; the rows come from L2.
// (s * e - z)^2 is formed and added in float64; the workgroup's sum (butterfly, then its waves in index order) is one float64 partial,
// part[channel block][position tile].  A lane whose index is outside [0, n_e) reads no codebook row, counts nothing and adds NaN.
// The histogram is integer: the workgroups of channel block 0 add 1 to counts[idx[p]] with a vector atomic (order-independent).
#define VQ_CB 64
__global__ __launch_bounds__(256) void vq_stats_kernel(const float* __restrict__ z, const int64_t* __restrict__ idx, const float* __restrict__ cb,
                                                        const float* __restrict__ row_scale, double* __restrict__ part, int* __restrict__ counts,
                                                        long P, int C, int HW, int n_e, int vec) {
    __shared__ double wpart[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long p = (long)blockIdx.x * 64 + lane;
    const int c0 = blockIdx.y * VQ_CB, c1 = min(C, c0 + VQ_CB);
    double acc = 0.0;
    if (p < P) {
        const int64_t code = idx[p];
        const bool ok = code >= 0 && code < n_e;
        if (!ok) {
            acc = __builtin_nan("");
        } else {
            if (blockIdx.y == 0 && wave == 0) atomicAdd(counts + code, 1);
            const long n = p / HW;
            const float* zp = z + n * (long)C * HW + (p - n * HW);   // + c * HW
            const float* e = cb + code * (long)C;
            const double s = row_scale ? (double)row_scale[code] : 1.0;
            for (int c = c0 + 4 * wave; c < c1; c += 16) {
                float ev[4];
                if (vec) {   // C % 4 == 0: the four channels are inside the row
                    const float4 q = *reinterpret_cast<const float4*>(e + c);
                    ev[0] = q.x; ev[1] = q.y; ev[2] = q.z; ev[3] = q.w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) ev[k] = c + k < c1 ? e[c + k] : 0.f;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c + k < c1) {
                        const double d = s * (double)ev[k] - (double)zp[(long)(c + k) * HW];
                        acc += d * d;
                    }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) wpart[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(long)blockIdx.y * gridDim.x + blockIdx.x] = ((wpart[0] + wpart[1]) + wpart[2]) + wpart[3];
}

// `count` float64 partials -> their sum / n as fp32: thread t adds the partials t, t + 1024, ... in that order, then `block_sum_f64`.
__global__ __launch_bounds__(1024) void partials_mean_strided_kernel(const double* __restrict__ part, long count, double n, float* __restrict__ out) {
    double acc = 0.0;
    for (long i = threadIdx.x; i < count; i += 1024) acc += part[i];
    const double s = block_sum_f64(acc);
    if (threadIdx.x == 0) out[0] = (float)(s / n);
}

extern "C" int64_t ccvs_vq_stats_workspace_bytes(int64_t N, int32_t C, int32_t HW) {
    if (N <= 0 || C <= 0 || HW <= 0) return 0;
    return cdiv64(N * HW, 64) * cdiv64(C, VQ_CB) * (int64_t)sizeof(double);
}

extern "C" int ccvs_vq_stats(const float* z, const int64_t* idx, const float* codebook, const float* row_scale, float* sq_sum_out, int32_t* counts,
                             void* workspace, int64_t N, int32_t C, int32_t HW, int32_t n_e, void* stream) {
    CCVS_REQUIRE(z && idx && codebook && sq_sum_out && counts && workspace, "ccvs_vq_stats: null pointer");
    CCVS_REQUIRE(N > 0 && C > 0 && HW > 0 && n_e > 0, "ccvs_vq_stats: bad arguments");
    const long P = (long)N * HW, tiles = cdiv64(P, 64), blocks = cdiv64(C, VQ_CB);
    CCVS_REQUIRE(tiles < 2147483647L && blocks <= 65535, "ccvs_vq_stats: N * HW < 2^37, C <= 4194240; got N %ld, HW %d, C %d", (long)N, HW, C);
    if (hipMemsetAsync(counts, 0, (size_t)n_e * sizeof(int32_t), (hipStream_t)stream) != hipSuccess) {
        ccvs_set_error("ccvs_vq_stats: clearing counts failed");
        return CCVS_ERR_LAUNCH;
    }
    const int vec = C % 4 == 0 && (reinterpret_cast<uintptr_t>(codebook) & 15) == 0;
    hipLaunchKernelGGL(vq_stats_kernel, dim3((unsigned)tiles, (unsigned)blocks), dim3(256), 0, (hipStream_t)stream, z, idx, codebook, row_scale,
                       (double*)workspace, counts, P, C, HW, n_e, vec);
    CCVS_CHECK_LAUNCH("ccvs_vq_stats");
    hipLaunchKernelGGL(partials_mean_strided_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const double*)workspace, tiles * blocks,
                       (double)P * (double)C, sq_sum_out);
    CCVS_CHECK_LAUNCH("ccvs_vq_stats");
    return CCVS_OK;
}

// quantize.py:67-68: exp(-sum_j p_j log(p_j + 1e-10)), p_j = counts[j] / total, by one workgroup in float64: thread t adds the terms
// of the run j = t * run .. (t + 1) * run - 1 in index order, thread 0 adds the 1024 runs in index order; rounded once to fp32.
__global__ __launch_bounds__(1024) void code_perplexity_kernel(const int* __restrict__ counts, int n_e, double total, float* __restrict__ out) {
    __shared__ double runs[1024];
    const int run = (n_e + 1023) / 1024;
    double acc = 0.0;
    for (int j = threadIdx.x * run; j < min(n_e, (int)(threadIdx.x + 1) * run); ++j) {
        const double pj = (double)counts[j] / total;
        acc += pj * log(pj + 1e-10);
    }
    runs[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int t = 0; t < 1024; ++t) s += runs[t];
    out[0] = (float)exp(-s);
}

extern "C" int ccvs_code_perplexity(const int32_t* counts, int32_t n_e, int64_t total, float* out, void* stream) {
    CCVS_REQUIRE(counts && out, "ccvs_code_perplexity: null pointer");
    CCVS_REQUIRE(n_e > 0 && n_e <= 1048576 && total > 0, "ccvs_code_perplexity: 1 <= n_e <= 2^20, total > 0; got n_e %d, total %ld", n_e, (long)total);
    hipLaunchKernelGGL(code_perplexity_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, counts, n_e, (double)total, out);
    CCVS_CHECK_LAUNCH("ccvs_code_perplexity");
    return CCVS_OK;
}

// ---- SSIM -------------------------------------------------------------------------------------
// A workgroup owns a 32 x 32 block of window CENTRES of one plane: the 38 x 38 pixels under them go to LDS, the five window sums
// (x, y, xx, yy, xy) are formed separably in float64 -- 7 columns, then 7 rows -- and the block's sum of S is written to
// part[plane][block]; a second kernel adds the blocks of a plane in index order (no atomics: run-to-run identical).
#define SS_T 32
#define SS_W 7
#define SS_H (SS_T + SS_W - 1)

__global__ __launch_bounds__(256) void ssim_tile_kernel(const float* __restrict__ x, const float* __restrict__ y, double* __restrict__ part, int H, int W,
                                                         int tiles_x, int tiles_y, double c1, double c2) {
#pragma clang fp contract(off)   // numpy's arithmetic: with fused multiply-adds SSIM(x, x) is 1 - 1e-16 instead of 1
    __shared__ float sx[SS_H][SS_H + 1], sy[SS_H][SS_H + 1];
    __shared__ double row[5][SS_H][SS_T + 1];
    __shared__ double wsum[4];
    const int plane = blockIdx.y, tile = blockIdx.x;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * SS_T, x0 = tx * SS_T;            // first window's top-left pixel = first centre - 3
    const int vh = H - (SS_W - 1), vw = W - (SS_W - 1);  // window positions of the plane
    const float* xp = x + (long)plane * H * W;
    const float* yp = y + (long)plane * H * W;
    for (int e = threadIdx.x; e < SS_H * SS_H; e += 256) {
        const int r = e / SS_H, c = e - r * SS_H;
        const int gy = y0 + r, gx = x0 + c;
        const bool in = gy < H && gx < W;
        sx[r][c] = in ? xp[(long)gy * W + gx] : 0.f;
        sy[r][c] = in ? yp[(long)gy * W + gx] : 0.f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < SS_H * SS_T; e += 256) {
        const int r = e / SS_T, c = e - r * SS_T;
        double a = 0, b = 0, aa = 0, bb = 0, ab = 0;
#pragma unroll
        for (int k = 0; k < SS_W; ++k) {
            const double u = sx[r][c + k], v = sy[r][c + k];
            a += u; b += v; aa += u * u; bb += v * v; ab += u * v;
        }
        row[0][r][c] = a; row[1][r][c] = b; row[2][r][c] = aa; row[3][r][c] = bb; row[4][r][c] = ab;
    }
    __syncthreads();
    double acc = 0.0;
    for (int e = threadIdx.x; e < SS_T * SS_T; e += 256) {
        const int r = e / SS_T, c = e - r * SS_T;
        if (y0 + r >= vh || x0 + c >= vw) continue;
        double s[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            double t = 0;
#pragma unroll
            for (int k = 0; k < SS_W; ++k) t += row[q][r + k][c];
            s[q] = t / 49.0;
        }
        const double ux = s[0], uy = s[1];
        const double cov = 49.0 / 48.0;   // use_sample_covariance
        const double vx = cov * (s[2] - ux * ux), vy = cov * (s[3] - uy * uy), vxy = cov * (s[4] - ux * uy);
        const double a1 = 2 * ux * uy + c1, a2 = 2 * vxy + c2, b1 = ux * ux + uy * uy + c1, b2 = vx + vy + c2;
        acc += (a1 * a2) / (b1 * b2);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(long)plane * tiles_x * tiles_y + tile] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

__global__ __launch_bounds__(64) void ssim_finish_kernel(const double* __restrict__ part, double* __restrict__ out, int tiles, double count) {
    if (threadIdx.x != 0) return;
    const double* p = part + (long)blockIdx.x * tiles;
    double s = 0.0;
    for (int t = 0; t < tiles; ++t) s += p[t];
    out[blockIdx.x] = s / count;   // a division like numpy's mean: n ones give exactly 1
}

extern "C" int64_t ccvs_ssim_workspace_bytes(int64_t planes, int32_t H, int32_t W) {
    if (planes <= 0 || H < SS_W || W < SS_W) return 0;
    return planes * cdiv64(H - (SS_W - 1), SS_T) * cdiv64(W - (SS_W - 1), SS_T) * (int64_t)sizeof(double);
}

extern "C" int ccvs_ssim(const float* x, const float* y, double* out, void* workspace, int64_t planes, int32_t H, int32_t W, double data_range,
                         void* stream) {
    CCVS_REQUIRE(H >= SS_W && W >= SS_W, "ccvs_ssim: the 7 x 7 window exceeds the %d x %d plane", H, W);
    CCVS_REQUIRE(x && y && out && workspace, "ccvs_ssim: null pointer");
    CCVS_REQUIRE(planes > 0 && planes <= 65535 && data_range > 0, "ccvs_ssim: 1 .. 65535 planes per call, data_range > 0");
    const int tiles_y = (int)cdiv64(H - (SS_W - 1), SS_T), tiles_x = (int)cdiv64(W - (SS_W - 1), SS_T);
    const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
    hipLaunchKernelGGL(ssim_tile_kernel, dim3(tiles_x * tiles_y, (unsigned)planes), dim3(256), 0, (hipStream_t)stream, x, y, (double*)workspace, H, W,
                       tiles_x, tiles_y, c1, c2);
    CCVS_CHECK_LAUNCH("ccvs_ssim");
    hipLaunchKernelGGL(ssim_finish_kernel, dim3((unsigned)planes), dim3(64), 0, (hipStream_t)stream, (const double*)workspace, out, tiles_x * tiles_y,
                       (double)(H - (SS_W - 1)) * (double)(W - (SS_W - 1)));
    CCVS_CHECK_LAUNCH("ccvs_ssim");
    return CCVS_OK;
}

// ---- bilinear resize (metrics.py:115-124 `upscale`: F.interpolate(videos, size, mode='bilinear'), align_corners=False) --------
// torch's formulation: src = max(scale * (dst + 0.5) - 0.5, 0) with scale = in / out in fp32, the two rows blended after the
// two columns.
__global__ __launch_bounds__(256) void resize_bilinear_kernel(const float* __restrict__ x, float* __restrict__ out, long planes, int H, int W, int OH,
                                                               int OW, float sh, float sw) {
#pragma clang fp contract(off)
    const long total = planes * OH * OW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int ox = (int)(i % OW);
        const long r = i / OW;
        const int oy = (int)(r % OH);
        const long pl = r / OH;
        const float fy = fmaxf(sh * ((float)oy + 0.5f) - 0.5f, 0.f), fx = fmaxf(sw * ((float)ox + 0.5f) - 0.5f, 0.f);
        const int y0 = (int)fy, x0 = (int)fx;
        const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
        const float ly = fy - (float)y0, lx = fx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
        const float* p = x + pl * H * W;
        out[i] = hy * (hx * p[(long)y0 * W + x0] + lx * p[(long)y0 * W + x1]) + ly * (hx * p[(long)y1 * W + x0] + lx * p[(long)y1 * W + x1]);
    }
}

extern "C" int ccvs_resize_bilinear(const float* x, float* out, int64_t planes, int32_t H, int32_t W, int32_t OH, int32_t OW, void* stream) {
    CCVS_REQUIRE(x && out, "ccvs_resize_bilinear: null pointer");
    CCVS_REQUIRE(planes > 0 && H > 0 && W > 0 && OH > 0 && OW > 0, "ccvs_resize_bilinear: bad arguments");
    const long total = (long)planes * OH * OW;
    const long blocks = cdiv64(total, 256) < 1048576 ? cdiv64(total, 256) : 1048576;
    hipLaunchKernelGGL(resize_bilinear_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, out, (long)planes, H, W, OH, OW,
                       (float)H / (float)OH, (float)W / (float)OW);
    CCVS_CHECK_LAUNCH("ccvs_resize_bilinear");
    return CCVS_OK;
}

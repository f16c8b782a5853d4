// Launcher of the reference's 7x7 correlation kernel (test oracle, never linked into the product).
//
// `oracle/build_ref_correlation.py` writes the reference's `kernel_Correlation_rearrange` / `kernel_Correlation_updateOutput`
// (one copy per stride, names suffixed _s1 / _s2) to `oracle/_ref/ref_correlation_kernels.inc` and compiles this file with
// it.  `ref_correlation7x7` restates `_FunctionCorrelation.forward` (reference modules/correlation.py:281-338):
//   * zeroed rbot0 / rbot1 [N, H+6s, W+6s, C] (a scratch buffer owned here, grown on demand);
//   * a zeroed output [N, 49, ceil(H/s), ceil(W/s)];
//   * `rearrange` of first and of second: grid (ceil(HW/16), C, N), block 16;
//   * `updateOutput`: grid (Wo, Ho, N), block 32, C*4 bytes of dynamic LDS.
// SIZE_k(t) in the kernels reads `__constant__ int t_sz[4]`, stored on the launch stream ahead of each launch.  The call
// ends with a stream synchronisation, so the sizes and the scratch buffer are never shared by two calls in flight.
//
// The reference reduces its per-lane partial sums through `__shared__ float sum[32]` with no barrier between lane 0's read
// of sum[] and the other lanes' reset of it for the next output channel: correct only because the 32-thread block is a
// single wave.  On gfx950 the block is one wave64 with half of its lanes active, so the reduction is race-free and
// deterministic (the tests check bit-equal repeated runs).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ref_correlation_kernels.inc"

namespace {

float* g_scratch = nullptr;
size_t g_scratch_bytes = 0;

#define REF_TRY(x)                                   \
    do {                                             \
        const hipError_t e_ = (x);                   \
        if (e_ != hipSuccess) return (int)e_;        \
    } while (0)

// host copies of the four size arrays: they outlive the asynchronous copies (the call synchronises before it returns)
int g_sizes[4][4];

int set_sizes(int slot, const void* symbol, int s0, int s1, int s2, int s3, hipStream_t st) {
    int* v = g_sizes[slot];
    v[0] = s0; v[1] = s1; v[2] = s2; v[3] = s3;
    REF_TRY(hipMemcpyToSymbolAsync(symbol, v, 4 * sizeof(int), 0, hipMemcpyHostToDevice, st));
    return 0;
}

}  // namespace

// Returns 0 or a hipError_t.  first, second: [N, C, H, W] contiguous float32; out: [N, 49, ceil(H/s), ceil(W/s)].
extern "C" int ref_correlation7x7(const float* first, const float* second, float* out, int32_t N, int32_t C, int32_t H,
                                  int32_t W, int32_t stride, void* stream) {
    if (!first || !second || !out || N <= 0 || C <= 0 || H <= 0 || W <= 0) return (int)hipErrorInvalidValue;
    if (stride != 1 && stride != 2) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const int s = stride, Hp = H + 6 * s, Wp = W + 6 * s;
    const int Ho = (H + s - 1) / s, Wo = (W + s - 1) / s;
    const size_t rb = (size_t)N * Hp * Wp * C;
    if (g_scratch_bytes < 2 * rb * sizeof(float)) {
        REF_TRY(hipStreamSynchronize(st));
        if (g_scratch) REF_TRY(hipFree(g_scratch));
        g_scratch = nullptr;
        g_scratch_bytes = 0;
        REF_TRY(hipMalloc((void**)&g_scratch, 2 * rb * sizeof(float)));
        g_scratch_bytes = 2 * rb * sizeof(float);
    }
    float* rbot0 = g_scratch;
    float* rbot1 = g_scratch + rb;
    REF_TRY(hipMemsetAsync(g_scratch, 0, 2 * rb * sizeof(float), st));
    REF_TRY(hipMemsetAsync(out, 0, (size_t)N * 49 * Ho * Wo * sizeof(float), st));

    // rearrange: input [N, C, H, W] -> output [N, Hp, Wp, C] (the same sizes for first and second)
    REF_TRY((hipError_t)set_sizes(0, HIP_SYMBOL(input_sz), N, C, H, W, st));
    REF_TRY((hipError_t)set_sizes(1, HIP_SYMBOL(output_sz), N, Hp, Wp, C, st));
    const int n = H * W;
    const dim3 rgrid((n + 16 - 1) / 16, C, N);
    if (s == 1) {
        hipLaunchKernelGGL(kernel_Correlation_rearrange_s1, rgrid, dim3(16), 0, st, n, first, rbot0);
        hipLaunchKernelGGL(kernel_Correlation_rearrange_s1, rgrid, dim3(16), 0, st, n, second, rbot1);
    } else {
        hipLaunchKernelGGL(kernel_Correlation_rearrange_s2, rgrid, dim3(16), 0, st, n, first, rbot0);
        hipLaunchKernelGGL(kernel_Correlation_rearrange_s2, rgrid, dim3(16), 0, st, n, second, rbot1);
    }
    REF_TRY(hipGetLastError());

    // updateOutput: rbot0 [N, Hp, Wp, C], top [N, 49, Ho, Wo]
    REF_TRY((hipError_t)set_sizes(2, HIP_SYMBOL(rbot0_sz), N, Hp, Wp, C, st));
    REF_TRY((hipError_t)set_sizes(3, HIP_SYMBOL(top_sz), N, 49, Ho, Wo, st));
    const int nt = 49 * Ho * Wo;
    const dim3 ugrid(Wo, Ho, N);
    if (s == 1)
        hipLaunchKernelGGL(kernel_Correlation_updateOutput_s1, ugrid, dim3(32), C * 4, st, nt, rbot0, rbot1, out);
    else
        hipLaunchKernelGGL(kernel_Correlation_updateOutput_s2, ugrid, dim3(32), C * 4, st, nt, rbot0, rbot1, out);
    REF_TRY(hipGetLastError());
    REF_TRY(hipStreamSynchronize(st));
    return 0;
}

/* libccvs_hip.so: the memory-bound passes of LPIPS (piq.LPIPS: a VGG16 feature distance) around the
 * convolutions, which are ccvs_conv2d / ccvs_conv2d_bf16x3 as they stand.  Additive to ABI version 6; include/ccvs_hip.h includes this
 * header (inside its extern "C" block), so a program that includes that one needs nothing else.  Status codes and conventions are those
 * of ccvs_hip.h: every pointer is a device pointer unless said otherwise, `stream` a hipStream_t, nothing synchronises with the host, no
 * state is kept between calls.  All tensors are dense fp32.  Reductions are float64 inside, use no atomics and add in a fixed order:
 * the same bits on every run. */
#ifndef CCVS_HIP_LPIPS_H
#define CCVS_HIP_LPIPS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* out[p][i] = (x[p][i] - mean[p % 3]) / std[p % 3] for the `planes` (a multiple of 3: [N, 3] images) planes of HW pixels, a true fp32
 * division as torch's `(x - mean) / std`.  mean, std: HOST pointers to 3 floats, read before the call returns.  x and out do not overlap. */
int ccvs_lpips_prep(const float* x, float* out, int64_t planes, int64_t HW, const float* mean, const float* std, void* stream);

/* x[i] = x[i] < 0 ? 0 : x[i] for n elements, in place (a NaN stays a NaN, as torch.relu leaves it). */
int ccvs_relu_(float* x, int64_t n, void* stream);

/* out[p][oy][ox] = relu(max of x[p][2 oy .. 2 oy + 1][2 ox .. 2 ox + 1]) for [planes, H, W] -> [planes, H / 2, W / 2]: nn.ReLU followed
 * by nn.MaxPool2d(2, 2) in floor mode (an odd last row or column is dropped).  A NaN in a window gives NaN, as torch's pool does. */
int ccvs_relu_maxpool2(const float* x, float* out, int64_t planes, int32_t H, int32_t W, void* stream);

/* The distance of one tapped layer.  f: [2 M, C, HW], images 0 .. M - 1 from x and M .. 2 M - 1 from y; w: the layer's linear head [C];
 * relu != 0: f holds pre-activations and max(f, 0) is what is compared.  Per image m and position p, with a = f[m, :, p],
 * b = f[M + m, :, p]:
 *     d[m, p] = sum_c w[c] (a[c] / (sqrt(sum a^2) + 1e-10) - b[c] / (sqrt(sum b^2) + 1e-10))^2        (all in float64)
 * and out[m] = (accumulate ? out[m] : 0) + (sum_p d[m, p]) / HW as float64.  An all-zero vector contributes 0 / 1e-10 = 0, not NaN.
 * workspace: ccvs_lpips_layer_workspace_bytes(M, HW) bytes (a float64 partial per image and workgroup; 0 for arguments the call
 * refuses).  M <= 65535 per call. */
int64_t ccvs_lpips_layer_workspace_bytes(int64_t M, int64_t HW);
int ccvs_lpips_layer(const float* f, const float* w, double* out, void* workspace, int64_t M, int32_t C, int64_t HW, int32_t relu,
                     int32_t accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CCVS_HIP_LPIPS_H */

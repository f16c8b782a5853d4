/* libccvs_hip.so: the passes of the Frechet Video Distance's I3D embedding (the Kinetics-400 RGB Inception-I3D of tools/tf_fvd/fvd.py;
 * DESIGN.md section 4.20) around its convolutions, which are ccvs_conv2d / ccvs_conv2d_bf16x3 as they stand: the activations live as
 * [N T, C, H, W] (frames are the batch), a k_t-tap 3-D convolution is a 2-D one over the k_t C channels of time-stacked frames.
 * Additive to ABI version 6; include/ccvs_hip.h includes this header (inside its extern "C" block), so a program that includes that
 * one needs nothing else.  Status codes and conventions are those of ccvs_hip.h: every pointer is a device pointer, `stream` a
 * hipStream_t, nothing synchronises with the host, no state is kept between calls.  Reductions are float64 inside, use no atomics and
 * add in a fixed order: the same bits on every run.
 *
 * TensorFlow's SAME geometry, per axis of n elements, kernel k, stride s: out = ceil(n / s), total = max((out - 1) s + k - n, 0),
 * before = total / 2 (rounded down), after = total - before. */
#ifndef CCVS_HIP_FVD_H
#define CCVS_HIP_FVD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* fvd.py:34-51 `preprocess`: uint8 frames u8 [frames, H, W, 3] -> out [frames, 3, OH, OW] fp32, TF1's tf.image.resize_bilinear
 * (align_corners False, no half-pixel centres) followed by 2 v / 255 - 1, every step a separate fp32 operation (nothing contracted):
 *     scale = (float)in / (float)out, src = (float)dst * scale, i0 = floor(src), i1 = min(i0 + 1, in - 1), f = src - i0   per axis,
 *     top = tl + (tr - tl) fx, bot = bl + (br - bl) fx, v = top + (bot - top) fy, out = (2 v) / 255 - 1.
 * flip != 0: output channel c is input channel 2 - c. */
int ccvs_fvd_prep(const uint8_t* u8, float* out, int64_t frames, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t flip, void* stream);

/* The time-stacked input of a kt-tap, stride-st 3-D convolution with SAME padding in time.  x: `clips` clips of T frames
 * [clips T, C, H, W], frame stride in_sN and channel stride in_sC in elements (rows and planes dense) -> out
 * [clips To, kt C, H + pt + pb, W + pl + pr] dense, To = ceil(T / st): channel j C + c of output frame t' of a clip is channel c of
 * that clip's frame t' st + j - before (SAME's `before` of T, kt, st), zeros where that frame lies outside the clip; the pt / pb / pl /
 * pr border rows and columns are zeros.  phases = 2 (both bordered sides even) also splits the frame into its four pixel phases, out
 * [clips To, 4 kt C, (H + pt + pb) / 2, (W + pl + pr) / 2]: channel (j C + c) 4 + 2 py + px holds the bordered frame's pixels
 * (2 y + py, 2 x + px) -- a stride-2 convolution of the bordered frame is then a stride-1 convolution of half the kernel size over
 * these channels.  relu != 0: max(x, 0) is what is written (a NaN stays).  x and out do not overlap. */
int ccvs_time_unfold(const float* x, int64_t in_sN, int64_t in_sC, float* out, int32_t clips, int32_t T, int32_t C, int32_t H, int32_t W,
                     int32_t kt, int32_t st, int32_t pt, int32_t pb, int32_t pl, int32_t pr, int32_t phases, int32_t relu, void* stream);

/* A 3-D max pool with SAME geometry over x [clips T, C, H, W] (dense) -> out [clips ceil(T / st), C, ceil(H / sh), ceil(W / sw)]:
 * kernel (kt, kh, kw) one of (1,3,3), (3,3,3), (2,2,2), stride (st, sh, sw) one of (1,2,2), (2,2,2), (1,1,1).  A window is clipped to
 * the clip (padding never wins: TensorFlow's pool); relu != 0 pools max(x, 0); a NaN in a window comes out, as in torch's pools. */
int ccvs_maxpool3d_same(const float* x, float* out, int32_t clips, int32_t T, int32_t C, int32_t H, int32_t W, int32_t kt, int32_t kh,
                        int32_t kw, int32_t st, int32_t sh, int32_t sw, int32_t relu, void* stream);

/* The I3D head.  x [clips T, C, HW] fp32 (dense; T >= 2, C <= 4096), w [K, C] and b [K] fp32 -> out [clips, K] float64:
 *     p[c] = mean over the T - 1 windows j of the mean of x[j .. j + 1, c, :]      (the (2, H, W) average pool, stride 1, VALID)
 *     out[k] = sum_c w[k, c] p[c] + b[k]                                             (the logits, then their mean over time)
 * all in float64 (the logits are linear, so the mean over time is taken first).  relu != 0: max(x, 0) is what is averaged. */
int ccvs_i3d_head(const float* x, const float* w, const float* b, double* out, int32_t clips, int32_t T, int32_t C, int32_t HW, int32_t K,
                  int32_t relu, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CCVS_HIP_FVD_H */

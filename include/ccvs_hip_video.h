/* libccvs_hip.so: the input stage of the video-file datasets -- the reference's TENSOR transform chain (data/base_dataset.py:205, 341-386
 * with is_PIL=False: torchvision's Resize on a float tensor, i.e. F.interpolate(mode="bilinear", align_corners=False) without
 * antialiasing, crops, Normalize) for N frames in one launch.  Additive to ABI version 6; include/ccvs_hip.h
 * includes this header (inside its extern "C" block).  Status codes and conventions are those of ccvs_hip.h: `src` and `out` are device
 * pointers, `stages` and `mean_std` HOST pointers read before the call returns, `stream` a hipStream_t, nothing synchronises with the
 * host, no state is kept between calls.  (The Pillow-exact uint8 chain of the frame-folder datasets is ccvs_hip_input.h.) */
#ifndef CCVS_HIP_VIDEO_H
#define CCVS_HIP_VIDEO_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CCVS_INGEST_PRE_NONE 0
#define CCVS_INGEST_PRE_DIV255 1 /* v / 255.0f, a correctly rounded fp32 division (`vid.float() / 255`) */
#define CCVS_INGEST_PRE_X2M1 2   /* v * 2 - 1, two fp32 operations (the STFT stream, base_dataset.py:229) */
#define CCVS_INGEST_MAX_STAGES 3

/* Source, one of
 *   src_is_u8 != 0   uint8 [N, Hs, Ws, 3] interleaved RGB, rows dense, frame n at (uint8_t*)src + n * src_sN (bytes); C must be 3;
 *   src_is_u8 == 0   fp32 planar: element (n, c, y, x) at ((float*)src)[n * src_sN + c * src_sC + y * Ws + x] (strides in elements), C 1 or 3.
 * pre: one of CCVS_INGEST_PRE_*, applied to every source value as it is read.
 *
 * stages: n_stages (1 .. 3) rows of int32 (top, left, hc, wc, Ho, Wo): crop the stage's input -- the source for stage 0, the previous
 * stage's Ho x Wo output after that -- to the box, then resize the box to Ho x Wo as torch's upsample_bilinear2d(align_corners=False)
 * does, in fp32 and in this order of operations, no fused multiply-add:
 *   scale = (float)in / (float)out;  s = max(scale * ((float)dst + 0.5f) - 0.5f, 0);  i0 = (int)s;  i1 = i0 + (i0 < in - 1);
 *   l1 = s - (float)i0;  l0 = 1 - l1;  out = l0h * (l0w * a + l1w * b) + l1h * (l0w * c + l1w * d)
 * so an axis with in == out copies.  ALL stages are evaluated per output pixel in one launch, by recursion over the stages: each
 * stage's value is rounded to fp32 exactly as if it had been stored, so the result has the bits of running the stages one launch each
 * through fp32 intermediates (which is what a call with n_stages == 1 per stage does).  4^n_stages source reads per output value.
 *
 * mean_std: NULL, or 2 C floats (mean[0 .. C), std[0 .. C)): (y - mean[c]) / std[c] as two fp32 operations on the last stage's value.
 *
 * out: fp32, element (n, c, y, x) at out[n * out_sN + c * out_sC + y * Wo + x] (rows dense) -- a [B, T, C, H, W] clip or a slice of one. */
int ccvs_ingest_f32(const void* src, int32_t src_is_u8, int64_t src_sN, int64_t src_sC, int32_t N, int32_t C, int32_t Hs, int32_t Ws,
                    int32_t pre, const int32_t* stages, int32_t n_stages, const float* mean_std,
                    float* out, int64_t out_sN, int64_t out_sC, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CCVS_HIP_VIDEO_H */

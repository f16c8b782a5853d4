/* libccvs_hip.so: the input stage -- uint8 frames as an image decoder gives them to the fp32 clip the models read (DESIGN.md section
 * 4.14).  Additive to ABI version 6; include/ccvs_hip.h includes this header (inside its extern "C" block), so a program that includes
 * that one needs nothing else.  Status codes and conventions are those of ccvs_hip.h: every pointer is a device pointer, `stream` a
 * hipStream_t, nothing synchronises with the host, no state is kept between calls. */
#ifndef CCVS_HIP_INPUT_H
#define CCVS_HIP_INPUT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* One crop + resample stage of the reference's per-frame transform chain (data/base_dataset.py:341-386), with Pillow's 8-bit bilinear
 * resampler (ImagingResample) reproduced bit for bit in integer arithmetic.
 *
 * src: N frames of uint8 [Hs, Ws, 3] (interleaved RGB, rows dense), frame n at src + n * src_frame_bytes.  The stage reads the crop box
 * rows top .. top + hc - 1, columns left .. left + wc - 1 and nothing outside it.
 *
 * Tables (int32, built on the host: `ccvs_amd.ops.resample_tables`), per axis: coef [out, ksize] -- Pillow's normalised weights as
 * int(w * 2^22 + 0.5) -- and bounds [out, 2] = (first tap, number of taps), RELATIVE TO THE CROP BOX.  A pass is
 *   out = clip(((1 << 21) + sum_i coef[o][i] * p[first + i]) >> 22, 0, 255)
 * horizontal first, rounded to uint8, then vertical.  hcoef == NULL: no horizontal pass (then Wo == wc); vcoef == NULL: no vertical pass
 * (then Ho == hc); both NULL: crop + convert only, nothing is staged.  Taps are clamped to the crop box on the device, so a wrong table
 * gives wrong pixels, never an access outside the frames.
 *
 * Output, one of (the other pointer NULL):
 *   out_u8   uint8 [N, Ho, Wo, 3] dense -- the input of a further stage;
 *   out_f32  fp32 planar: element (n, c, y, x) at out_f32[n * out_sN + c * out_sC + y * Wo + x] (strides in elements, rows dense), its value
 *            lut[c * 256 + v] for the uint8 result v.  lut: float [3][256] on the device, filled by the host with ToTensor + Normalize in
 *            the framework's own arithmetic -- the kernel does no floating-point arithmetic.  Writes straight into a [B, T, 3, H, W] clip
 *            or a slice of one.
 * The arithmetic is integer: the result does not depend on the tiling.  A vertical support of any length is handled (the source rows
 * of a tile pass through LDS in chunks). */
int ccvs_ingest_u8(const uint8_t* src, int64_t src_frame_bytes, int32_t N, int32_t Hs, int32_t Ws,
                   int32_t top, int32_t left, int32_t hc, int32_t wc,
                   const int32_t* hcoef, const int32_t* hbounds, int32_t hksize,
                   const int32_t* vcoef, const int32_t* vbounds, int32_t vksize,
                   int32_t Ho, int32_t Wo,
                   uint8_t* out_u8, float* out_f32, int64_t out_sN, int64_t out_sC, const float* lut, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CCVS_HIP_INPUT_H */

/* libccvs_hip.so: the decoder's motion export (flowviz.hip).  Additive to ABI version 6; include/ccvs_hip.h
 * includes this header (inside its extern "C" block), so a program that includes that one needs nothing else.  Status codes and
 * conventions are those of ccvs_hip.h.
 *
 * The motion buffer of a clip batch is fp32 [B, T, 3, H, W]: planes 0 / 1 the flow (x, y) in pixels at full resolution towards the
 * frame's first context, plane 2 the fused occlusion mask in [0, 1] (1 = the decoder's own features, 0 = the warped contexts).  The
 * three planes of a frame are dense (stride H * W); the frame and batch strides are the caller's. */
#ifndef CCVS_HIP_FLOWVIZ_H
#define CCVS_HIP_FLOWVIZ_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* One frame slot of the motion buffer from the last InterBlock's (flow | occ) rows.  fo: row n of B * k rows at fo + n * fo_sN, three
 * dense H x W planes (flow x, flow y, occlusion logit); rows b * k .. b * k + k - 1 are the k contexts of clip b (1 <= k <= 16).
 * out: slot of clip b at out + b * out_sB, three dense planes:
 *     out[b, 0:2] = fo[b * k, 0:2] * flow_mult                                         (one fp32 product)
 *     out[b, 2]   = sigmoid(occ),  occ = fo[b, 2] for k = 1, else sum_j occ_j conf_j / sum_j conf_j with
 *                   conf_j = 1 - sigmoid(occ_j) + 1e-6 over the k rows of the clip     (the mask the decoder's blend uses). */
int ccvs_flow_export(const float* fo, int64_t fo_sN, int32_t B, int32_t k, int32_t H, int32_t W, float flow_mult, float* out,
                     int64_t out_sB, void* stream);

/* out[b] = the largest sqrt(fx^2 + fy^2) (each step rounded to fp32, no fused multiply-add) over the pixels of clip b whose magnitude
 * is finite; 0 where there is none.  motion: frame (b, t) at motion + b * sB + t * sT.  An integer maximum on the bit pattern of the
 * non-negative magnitude: the same bits on every run, under any CU budget. */
int ccvs_flow_max(const float* motion, int64_t sB, int64_t sT, int32_t B, int32_t T, int32_t H, int32_t W, float* out, void* stream);

/* The motion buffer as two uint8 clips [B, T, H, W, 3] (channels last, dense, 4-byte aligned).
 * flow_u8: r = min(1, |f| / max_px[b]), theta = (1 + atan2(fy, fx) / pi) / 2, idx = min(int(theta * 128), 127), and byte c is
 * (uint8)(clamp(r * lut[idx][c], 0, 1) * 255), truncated.  A clip whose max_px[b] is not > 0 is black (no division); so is a pixel with
 * a NaN or infinite component.  lut: 128 x 3 fp32 on the device.  occ_u8: (uint8)(clamp(mask, 0, 1) * 255) on the three channels
 * (a NaN mask gives 0). */
int ccvs_flow_render(const float* motion, int64_t sB, int64_t sT, int32_t B, int32_t T, int32_t H, int32_t W, const float* max_px,
                     const float* lut, uint8_t* flow_u8, uint8_t* occ_u8, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CCVS_HIP_FLOWVIZ_H */

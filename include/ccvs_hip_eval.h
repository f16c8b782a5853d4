/* libccvs_hip.so: the reductions behind the frame autoencoder's validation figures.  Additive to ABI
 * version 6; include/ccvs_hip.h includes this header (inside its extern "C" block), so a program that includes that one needs nothing
 * else.  Status codes and conventions are those of ccvs_hip.h: every pointer is a device pointer, `stream` a hipStream_t, nothing
 * synchronises with the host. */
#ifndef CCVS_HIP_EVAL_H
#define CCVS_HIP_EVAL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* torch.mean(torch.abs(a - b)) of quantized_video_model.py:474 (eval_img_to_img_generator) over n dense fp32 elements, into out[1]
 * fp32 on the device (no host synchronisation).  |a[i] - b[i]| is formed in float64; a grid of workgroups writes one float64 partial
 * each into workspace (ccvs_l1_workspace_bytes(n) bytes: their number depends on n alone), a second launch adds the partials in
 * index order, divides by n and rounds once.  16-byte loads where a and b are both 16-byte aligned, 4-byte loads otherwise.  No
 * atomics: the same bits on every run.  A NaN element gives NaN. */
int64_t ccvs_l1_workspace_bytes(int64_t n);
int ccvs_l1_mean(const float* a, const float* b, float* out, void* workspace, int64_t n, void* stream);
/* The two diagnostics of quantize.py:59-68 without the one-hot matrix.  z: [N, C, HW] fp32 (the encoder output, NCHW); idx: [N * HW]
 * int64 in (n, hw) order; codebook: [n_e, C] fp32; row_scale: [n_e] fp32 or NULL (normalize: 1 / ||e_j||).
 *   counts[j]      int32 [n_e]: how often code j occurs in idx.  Zeroed by this call, then integer atomics.
 *   sq_sum_out[0]  fp32: the mean over all N * C * HW elements of (s * codebook[idx[p]][c] - z[n, c, p])^2, s = row_scale[idx[p]] or 1,
 *                  difference, square and sums in float64 without atomics (partials in workspace, ccvs_vq_stats_workspace_bytes
 *                  bytes, added in a fixed order), rounded once: the same bits on every run.
 * An index outside [0, n_e) is not counted and makes the mean NaN; nothing is read or written out of bounds for it (the convention
 * of ccvs_token_nll).  z is read once. */
int64_t ccvs_vq_stats_workspace_bytes(int64_t N, int32_t C, int32_t HW);
int ccvs_vq_stats(const float* z, const int64_t* idx, const float* codebook, const float* row_scale, float* sq_sum_out, int32_t* counts,
                  void* workspace, int64_t N, int32_t C, int32_t HW, int32_t n_e, void* stream);
/* quantize.py:67-68: out[0] = exp(-sum_j p_j log(p_j + 1e-10)) with p_j = counts[j] / total, in float64 in index order by one
 * workgroup, rounded once to fp32.  counts: int32 [n_e] on the device; total > 0 (the number of positions counted). */
int ccvs_code_perplexity(const int32_t* counts, int32_t n_e, int64_t total, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CCVS_HIP_EVAL_H */

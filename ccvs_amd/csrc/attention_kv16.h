// What gpt.hip's launch chain needs of attention_kv16.hip (the bf16-KV-cache kernels; include/ccvs_hip_kv16.h has the public entries).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The decode form over bf16 caches, one workgroup per (row, head) of n_bh, `smem` = (16 + 1024 + Tmax) floats of LDS.  k_new / v_new
// (fp32 rows, batch stride kv_sB; both or neither): the appending form.  grp_rows > 0: pos_dev holds one length per row group.
// The caller checks the launch under its own name.
void ccvs_kv16_launch_attention_decode(int D, int n_bh, size_t smem, hipStream_t st, const float* q, long q_sB, const float* k_new,
                                       const float* v_new, long kv_sB, uint16_t* kc, uint16_t* vc, float* out, int H, int pos0,
                                       const int32_t* pos_dev, int grp_rows, int Tmax, float scale);

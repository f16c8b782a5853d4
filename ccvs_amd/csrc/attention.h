// What gpt.hip's launch chain needs of attention.hip (include/ccvs_hip.h and include/ccvs_hip_kv16.h have the public entries).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The decode form (Tq = 1), one workgroup per (row, head) of n_bh, `smem` = (16 + 1024 + Tmax) floats of LDS.  bf16 = false: kc / vc
// are fp32 caches, k_new / v_new NULL.  bf16 = true: bf16 caches; k_new / v_new (fp32 rows, batch stride kv_sB; both or neither): the
// appending form.  grp_rows > 0: pos_dev holds one length per row group.  The caller checks the launch under its own name.
void ccvs_launch_attention_decode(bool bf16, int D, int n_bh, size_t smem, hipStream_t st, const float* q, long q_sB, const float* k_new,
                                  const float* v_new, long kv_sB, void* kc, void* vc, float* out, int H, int pos0, const int32_t* pos_dev,
                                  int grp_rows, int Tmax, float scale);

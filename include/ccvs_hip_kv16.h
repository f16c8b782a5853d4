/* The token loop on a bfloat16 KV cache (opt-in: `--x_kv_dtype bf16`; ccvs_amd/csrc/attention.hip, the entry of the step in gpt.hip).
 * Included by ccvs_hip.h.
 *
 * THE MODE.  Every key and value row is rounded to bfloat16 when it is appended to the cache: round to nearest, ties to even, on the
 * fp32 bit pattern -- bits = (u + 0x7fff + ((u >> 16) & 1)) >> 16, a NaN becomes 0x7fc0 -- the rule of torch.Tensor.to(torch.bfloat16)
 * for every fp32 input (the largest finite fp32 rounds to inf).  The fp32 values that are rounded are the ones the fp32 mode stores: the
 * same QKV GEMM, the same bits.  Every attention product reads the STORED values -- prefill, the decode step, the re-prefill of a slid
 * window; the query at position t sees its own key and value rounded as well --, each widened exactly to fp32 (bits << 16), and from
 * there on the arithmetic is the fp32 kernels': fp32 products, fp32 softmax, fp32 sums.  Nothing else changes its type: weights,
 * activations, logits and the pick stay fp32.  The caches are [B,H,Tmax,D] of 16-bit words, half the bytes of the fp32 caches.
 * The fp32 entry points refuse nothing and know nothing of this: a cache is bf16 exactly where it is handed to the calls below.
 */
#ifndef CCVS_HIP_KV16_H
#define CCVS_HIP_KV16_H

/* ccvs_kv_append with bf16 caches: rounds and scatters K/V rows [B,Tq,H*D] (fp32, batch stride sB, row stride ld; D % 8 == 0, sB and ld
 * multiples of 4 floats, k, v and the caches 16-byte aligned) into kcache / vcache [B,H,Tmax,D] (bf16) at positions pos0 (+ *pos_dev) + t.  A position at or beyond Tmax
 * (reachable through pos_dev only) is skipped.  16 bytes per lane and store. */
int ccvs_kv_append_bf16(const float* k, const float* v, int64_t sB, int64_t ld, void* kcache, void* vcache, int32_t B, int32_t H,
                        int32_t Tq, int32_t pos0, const int32_t* pos_dev, int32_t Tmax, int32_t D, void* stream);

/* ccvs_attention over bf16 caches: q [B,Tq,H*D] fp32 (batch stride q_sB, row stride ldq), out [B,Tq,H*D] fp32 dense, D in {16, 32, 64}.
 * Tq > 1: the flash-style fp32-MFMA form; the tile loader widens the bf16 rows while it stages them in LDS.  k_new / v_new must be NULL.
 * Tq == 1: one workgroup per (row, head) streams the bf16 K, then V rows.
 *   k_new == v_new == NULL: the cache already holds position pos0 (+ *pos_dev) (ccvs_kv_append_bf16 ran).
 *   k_new, v_new given (fp32 [B,H*D] each, batch stride kv_sB: the two upper thirds of a [B,3C] QKV output): the APPENDING form -- the
 *   call rounds those rows, stores them in the caches at that position and uses the rounded values for it; whatever the caches held
 *   there before is not used.  One workgroup writes a given (row, head, position).  A position at or beyond Tmax appends nothing.
 *   grp_rows > 0 (with pos_dev; B % grp_rows == 0): ROW GROUPS as in a grouped decode step -- pos_dev is int32 [B / grp_rows] and row b
 *   sits at pos0 + pos_dev[b / grp_rows]; 0: one word for all rows. */
int ccvs_attention_bf16(const float* q, int64_t q_sB, int64_t ldq, const float* k_new, const float* v_new, int64_t kv_sB, void* kcache,
                        void* vcache, float* out, int32_t B, int32_t H, int32_t Tq, int32_t pos0, const int32_t* pos_dev, int32_t grp_rows,
                        int32_t Tmax, int32_t D, void* stream);

/* ccvs_gpt_decode_step on bf16 caches: the same descriptor, the same launch chain (5 * n_layer + 3 launches, hipGraph-capturable, no
 * allocation, no synchronisation) with two phases different per layer: ln1 + QKV is the plain GEMM into d->q with row stride 3C (no
 * scatter), and the attention is the appending decode form above, fed the K / V thirds of that buffer.  CONVENTIONS OF THE DESCRIPTOR
 * IN THIS MODE: layers[i].kcache / vcache point to bf16 [B,H,Tmax,C/H] (the struct's `float*` is a plain address here), and d->q holds
 * 3C floats per row ([B,3C]).  top_p, groups, noise / noise_stream / rng and w_tiled act exactly as in ccvs_gpt_decode_step.
 * persistent = 1 is refused (CCVS_ERR_ARG, with the reason): the persistent step reads fp32 caches only. */
int ccvs_gpt_decode_step_bf16kv(const ccvs_gpt_decode* d, void* stream);

#endif

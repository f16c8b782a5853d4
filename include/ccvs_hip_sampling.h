/* libccvs_hip.so: nucleus (top-p) sampling in the token pick (gpt.hip, sample_topk_row's TOPP form).  Additive to
 * ABI version 6; include/ccvs_hip.h includes this header (inside its extern "C" block), so a program that includes that one needs
 * nothing else.  Status codes and conventions are those of ccvs_hip.h.
 *
 * The definition.  Per row, after xs = logit / temperature in fp32 and the top-k mask exactly as in the top-k pick:
 *     e_j = exp(xs_j - max) on the top-k set,  T = sum e,
 *     G_j = (the sum of e_i over the entries i of the top-k set with xs_i > xs_j, by float comparison) / T,
 * and entry j is in the nucleus iff it is in the top-k set and G_j < top_p: the rule of the `transformers` TopPLogitsWarper (Holtzman et
 * al.), applied after top-k on the renormalised distribution.  The most likely token is always kept.  Entries with equal xs share one
 * fate (-0.0 == +0.0, as in the top-k mask), so a tie at the boundary is kept whole.  The pick is then the top-k pick on the smaller
 * set: argmax(e) when greedy, argmax(e / noise) otherwise, the lowest index among equals; the row total is a common factor and is not
 * renormalised, and the Philox counter of an element does not depend on any mask -- the draws are the top-k pick's, word for word.
 * A row that is NaN or +-inf throughout returns token 0.
 *
 * The arithmetic of the decision is integer: the mass of an entry is floor(e_j * 2^46) with e_j the fp32 expf of the pick itself, T and
 * every partial sum are 64-bit integer sums, and G_j < top_p is decided as G_j < ceil((double) top_p * (double) T) on those integers.
 * The kept set is therefore the same bits on every run, in every launch form and in every batch slot.
 *
 * top_p: inside (0, 1) the nucleus is on; 1 is "off" (the call then runs the top-k pick, bit for bit); anything else is refused by name.
 * The form keeps 524 more words of LDS than the top-k pick, so its largest vocabulary is smaller: ccvs_sample_topp_max_vocab(). */
#ifndef CCVS_HIP_SAMPLING_H
#define CCVS_HIP_SAMPLING_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ccvs_sample_topk with the nucleus: the same arguments plus top_p. */
int ccvs_sample_topp(const float* logits, int64_t ld, const float* noise, int64_t* out, int64_t out_stride, int32_t B, int32_t V,
                     int32_t top_k, float temperature, float top_p, void* stream);
/* ccvs_sample_topk_philox with the nucleus: the same arguments plus top_p. */
int ccvs_sample_topp_philox(const float* logits, int64_t ld, int64_t* out, int64_t out_stride, int32_t B, int32_t V, int32_t top_k,
                            float temperature, float top_p, uint32_t key0, uint32_t key1, uint32_t row0, uint32_t step, uint32_t call,
                            void* stream);

/* Host only, no GPU needed: the largest V the nucleus form takes (40164; the top-k pick takes 40688).  One more is refused with a
 * message that names the top_p form, by the two calls above and by ccvs_gpt_decode_step with an active ccvs_gpt_decode.top_p. */
int32_t ccvs_sample_topp_max_vocab(void);

#ifdef __cplusplus
}
#endif
#endif /* CCVS_HIP_SAMPLING_H */

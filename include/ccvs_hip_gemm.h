/* libccvs_hip.so: the TILED weight layout of the decode GEMMs (gpt.hip, gemm16_tile) and an entry point that runs
 * one decode GEMM on it.  Additive to ABI version 6; include/ccvs_hip.h includes this header (inside its extern "C" block), so a program
 * that includes that one needs nothing else.  Status codes and conventions are those of ccvs_hip.h.
 *
 * The layout.  W [N,K] (torch Linear layout), K % 16 == 0, N padded up to a multiple of 16 by repeating its last row, is cut into blocks of
 * 16 rows x 16 columns.  Block (ct, kb) = rows 16 ct .., columns 16 kb .. is the 256 floats at offset (ct * K / 16 + kb) * 256; inside
 * it, float 4 * (li + 16 g) + j is W[16 ct + li][16 kb + 4 g + j], i.e. element (r, c) of W sits at
 *     ((((r / 16) * (K / 16) + c / 16) * 4 + (c % 16) / 4) * 16 + r % 16) * 4 + c % 4
 * = W.view(N / 16, 16, K / 16, 4, 4).permute(0, 2, 3, 1, 4).  A block is what one wave of the weight-stream kernel loads at a time (lane
 * li + 16 g: 16 bytes): 1 KB of whole, aligned 128-byte lines, where the row-major layout makes it 16 half-used ones.  The same floats
 * reach the same lanes, so every result is bit-identical to the row-major kernel's.  ccvs_gpt_decode.w_tiled makes the decode step read
 * its weight matrices in this layout.
 *
 * The entry point below: ONE decode GEMM (single position, M <= 256 rows) on tiled weights.  w_rowsum NULL: what ccvs_gemm_nt computes
 * (`workspace` as there); w_rowsum given: ccvs_gemm_ln, epilogue 0 or 1; kcache / vcache given as well: ccvs_gemm_ln_qkv with Tq = 1
 * (N = 3 K, y = q with ldy = K, H heads, position pos0 + *pos_dev, caches [M,H,Tmax,K/H]).  x, y, res, bias, w_rowsum and the caches are
 * laid out as in those calls; whole-sequence calls and more rows are refused. */
#ifndef CCVS_HIP_GEMM_H
#define CCVS_HIP_GEMM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int ccvs_gemm_tiled(const float* x, int64_t ldx, const float* w_tiled, const float* bias, const float* res, const float* w_rowsum,
                    float eps, float* y, int64_t ldy, int32_t M, int32_t N, int32_t K, int32_t epilogue, float* kcache, float* vcache,
                    int32_t H, int32_t pos0, const int32_t* pos_dev, int32_t Tmax, void* workspace, void* stream);

/* The most rows a GEMM on tiled weights takes (256), hence the most rows B of a decode step with ccvs_gpt_decode.w_tiled = 1: a step of
 * more rows runs the row-blocked kernel, which reads row-major weights, and is refused with tiled ones -- the caller keeps w_tiled = 0
 * and the row-major pointers for it. */
int32_t ccvs_gemm_tiled_max_rows(void);

#ifdef __cplusplus
}
#endif
#endif /* CCVS_HIP_GEMM_H */

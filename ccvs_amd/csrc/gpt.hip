// Transformer kernels: embedding, LayerNorm, nn.Linear GEMM on the fp32 matrix cores,
// the top-k / softmax / pick of the sampling loop and the decode step (KV-cached causal attention: attention.hip).
// Reference: models/skip_vid_generator/models/mingpt.py:33-117,186-305 and
// models/skip_vid_generator/models/transformer_model.py:256-260,395-409.
#include "act_access.h"
#include "attention.h"
#include "attention_core.h"   // attention_decode_item, the attention phase of gpt_step_kernel
#include "common.h"

// ---------------------------------------------------------------------------------------
// x[(b,t)][:] = tok_emb[idx[b*idx_sB + t]] + pos_table[pos_off[b] + pos0 + t]
// (mingpt.py:234-236,242-244; the factored s_emb/t_emb (+delta_length) or flat pos_emb rows
// are pre-summed by the host into pos_table once per call).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpt_embed_kernel(const int64_t* __restrict__ idx, long idx_sB, const int32_t* __restrict__ pos_off,
                                                        int pos0, const int32_t* __restrict__ pos_dev, int grp_rows, int Tq,
                                                        const float* __restrict__ tok, const float* __restrict__ pos,
                                                        float* __restrict__ x, long total, int C, int vocab) {
    // device-resident position: lets a captured hipGraph replay at advancing positions; with row groups (grp_rows > 0)
    // batch row b reads the word of its group, pos_dev[b / grp_rows]
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / C;
        const int c = (int)(i - r * C);
        const long b = r / Tq;
        const int tq = (int)(r - b * Tq);
        long t = idx[b * idx_sB + tq];
        t = t < 0 ? 0 : (t >= vocab ? vocab - 1 : t);
        const long prow = (pos_off ? pos_off[b] : 0) + pos0 + (pos_dev ? pos_dev[grp_rows > 0 ? b / grp_rows : 0] : 0) + tq;
        x[i] = tok[t * C + c] + pos[prow * C + c];
    }
}

extern "C" int ccvs_gpt_embed(const int64_t* idx, int64_t idx_sB, const int32_t* pos_off, int32_t pos0, const int32_t* pos_dev, int32_t Tq,
                              const float* tok_emb, const float* pos_table, float* x, int32_t B, int32_t C, int32_t vocab, void* stream) {
    CCVS_REQUIRE(idx && tok_emb && pos_table && x, "ccvs_gpt_embed: null pointer");
    CCVS_REQUIRE(B > 0 && Tq > 0 && C > 0 && vocab > 0 && (pos0 >= 0 || pos_dev), "ccvs_gpt_embed: empty tensor");
    const long total = (long)B * Tq * C;
    hipLaunchKernelGGL(gpt_embed_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, (hipStream_t)stream, idx, (long)idx_sB, pos_off,
                       pos0, pos_dev, 0, Tq, tok_emb, pos_table, x, total, C, vocab);
    CCVS_CHECK_LAUNCH("ccvs_gpt_embed");
    return CCVS_OK;
}

// ---------------------------------------------------------------------------------------
// LayerNorm (eps 1e-5), one wave per row.  The row is shifted before anything is summed, by the mean of its first four elements
// (its first element where it has fewer): the terms of the mean then have the size of the row's spread, not of its mean (a row of
// mean 1e3 and std 1 keeps fp32 accuracy relative to its std; a constant row gives exactly beta).  Four elements, as the folded
// LayerNorm of the GEMMs below (ln_shift): shifted by its first element alone, a row whose first element is its outlier (1 in
// front of N(0, 1e-3)) sums terms of the outlier's size and missed the test's tolerance 1.1 to 2.1 times.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                        const float* __restrict__ b, float* __restrict__ y, int rows, int C) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* xr = x + (long)row * C;
    const float x0 = C >= 4 ? ((xr[0] + xr[1]) + (xr[2] + xr[3])) * 0.25f : xr[0];
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += xr[c] - x0;
    const float mean = wave_sum(s) / C;   // of x - x0
    float v = 0.f;
    for (int c = lane; c < C; c += 64) { const float d = (xr[c] - x0) - mean; v += d * d; }
    const float rstd = rsqrtf(wave_sum(v) / C + 1e-5f);
    float* yr = y + (long)row * C;
    for (int c = lane; c < C; c += 64) yr[c] = ((xr[c] - x0) - mean) * rstd * g[c] + b[c];
}

extern "C" int ccvs_layernorm(const float* x, const float* gamma, const float* beta, float* y, int32_t rows, int32_t C, void* stream) {
    CCVS_REQUIRE(x && gamma && beta && y, "ccvs_layernorm: null pointer");
    CCVS_REQUIRE(rows > 0 && C > 0, "ccvs_layernorm: empty tensor");
    hipLaunchKernelGGL(layernorm_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, y, rows, C);
    CCVS_CHECK_LAUNCH("ccvs_layernorm");
    return CCVS_OK;
}

// ---------------------------------------------------------------------------------------
// nn.Linear as a weight stream on v_mfma_f32_16x16x4_f32:  y[M,N] = epi(x[M,K] @ W[N,K]^T + b).
//
// The decode regime (M = batch = 16 rows) is a pure HBM stream of W, split over many small
// dependent launches: what matters is bytes in flight per CU and a short critical path.
//   * workgroup = 16 rows x 16 columns, 8 waves = 8 K slices; each lane issues ALL its float4
//     loads of a 128-deep K batch before the first MFMA (W: row n = lane&15, k = k0+4*(lane>>4)+t;
//     x: same k map, row = lane&15, served by L1/L2), so a wave keeps 16 KiB in flight;
//   * no LDS staging, no barrier in the main loop; the 8 K slices are summed through LDS in a
//     fixed order (bitwise reproducible, no float atomics);
//   * LayerNorm is folded in algebraically: with W' = W*gamma, s[n] = sum_k W'[n][k] and
//     b' = b + W beta (packed once by the host),
//         LN(x) @ W^T + b = rstd * (x @ W'^T - mean * s) + b'
//     so the GEMM needs no normalised activations and the row statistics are applied in the
//     epilogue: the separate LayerNorm launch and its round trip through HBM disappear.
//     LayerNorm does not change when a constant is added to a row, and the fold is run on
//     d = x - c, c = the mean of the row's first four elements (ln_shift): what the lanes feed
//     to the MFMA and what they sum (sum d, sum d^2, from the very values they feed) is d.  On
//     the raw x both `sum x^2 / K - mean^2` and `x @ W'^T - mean * s` subtract two numbers of
//     the size of mean^2 resp. |mean| |s| to get one of the size of the variance resp. of the
//     output: the error is eps (mean / std)^2 resp. eps |mean| / std in units of the result
//     (a residual row of mean 1e3 and std 1: 3e-3 of the output's scale).  With c within a few
//     std of the mean both differences are between numbers of the result's own size.  Four
//     elements and not the first alone: a row whose first element is its outlier (|x0 - mean|
//     up to sqrt(K) std) would otherwise get the cancellation back from the shift itself;
//   * the QKV projection can scatter its K and V column blocks straight into the KV cache at a
//     host- or device-resident position (no separate append launch).
// Larger M (prefill) runs the same kernel over ceil(M/16) row blocks, W then coming from L2.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); }

// row statistics of the folded LayerNorm: one definition, floating-point contraction off, so that the plain and the
// row-blocked kernel (and any future variant) accumulate bit-identically
__device__ __forceinline__ void ln_accum(const float4& v, float& sx, float& sxx) {
#pragma clang fp contract(off)
    sx += (v.x + v.y) + (v.z + v.w);
    sxx += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
}

__device__ __forceinline__ void ln_accum(const f32x4& v, float& sx, float& sxx) {
#pragma clang fp contract(off)
    sx += (v[0] + v[1]) + (v[2] + v[3]);
    sxx += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
}

// the shift of the folded LayerNorm (see above): c = the mean of the row's first four elements, a function of the row alone, and
// d = x - c, which every form feeds to its MFMAs and to ln_accum instead of x.  One definition, contraction off, as ln_accum.
__device__ __forceinline__ float ln_shift(const float4& h) {
#pragma clang fp contract(off)
    return ((h.x + h.y) + (h.z + h.w)) * 0.25f;
}
__device__ __forceinline__ float ln_shift(const f32x4& h) {
#pragma clang fp contract(off)
    return ((h[0] + h[1]) + (h[2] + h[3])) * 0.25f;
}
template <bool B> struct ln_on { static constexpr bool value = B; };   // a K loop's kind: with / without the folded LayerNorm
__device__ __forceinline__ void ln_center(float4& v, float c) { v.x -= c; v.y -= c; v.z -= c; v.w -= c; }
__device__ __forceinline__ void ln_center(f32x4& v, float c) { v[0] -= c; v[1] -= c; v[2] -= c; v[3] -= c; }

// 16 bytes at descriptor `r`, per-lane byte offset `voff` + wave-uniform byte offset `soff` (buffer_load_dwordx4 ... offen)
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
template <int AUX = 0>   // AUX = 16: sc1 (see act_access.h)
__device__ __forceinline__ f32x4 buf_load4(__amdgpu_buffer_rsrc_t r, unsigned voff, int soff) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, AUX);
    return __builtin_bit_cast(f32x4, v);
}

// a wave-uniform operand of the phase table, opaque to the optimiser when OPAQUE: what the tile body derives from it for its epilogue alone
// -- the reciprocal of a divisor, (float)K -- is loop-invariant, and hoisted in front of the phase's tile loop it holds a VECTOR register
// (integer division and conversions run on the vector ALU) across the K loop, under the persistent step's 64-register cap.
// These are answers to one compiler's register allocation, not to the hardware: with hipcc of ROCm 7.2.0 (AMD clang 22.0.0git,
// roc-7.2.0 26014) and the LayerNorm shifts in the K loop, gpt_step_kernel spilled 12 to 28 bytes per lane without them -- (float)K, the
// reciprocals of D / Tq / grp_rows, the K loops' entry tests, the barrier's poll address and target, and the lane maps of the row-major
// body, all held in vector registers across the loop -- and none with them.  Under another compiler, build with
// -Rpass-analysis=kernel-resource-usage and drop whichever of them no longer buys a scratch-free gpt_step_kernel.
template <bool OPAQUE>
__device__ __forceinline__ int opaque_if(int v) {
    if constexpr (OPAQUE) asm volatile("" : "+s"(v));
    return v;
}
// a pointer read from the persistent step's phase table (constant memory) is a GENERIC pointer to the compiler: the cast through
// address_space(1) makes its accesses global_* instead of flat_* (COH = false: the kernel's own argument, already global)
template <bool COH, typename T>
__device__ __forceinline__ T* gp_(T* p) {
    if constexpr (COH) return (T*)(__attribute__((address_space(1))) T*)p;
    else return p;
}

struct Gemm16 {
    const float* x; long ldx;
    const float* w; const float* bias; const float* res; float* y; long ldy;
    int M, N, K, epi, ks;
    const float* ln_s; float ln_eps;
    float* kcache; float* vcache; int C, H, D, Tq, Tmax, pos0; const int32_t* pos_dev;
    int seq;           // 1: whole-sequence call (CCVS_GEMM_SEQ): the row-blocked form whatever M is (see launch_gemm16)
    int grp_rows;      // > 0: batch row b takes its device-resident position from pos_dev[b / grp_rows] (row groups of a decode step)
    int kz;            // K slices across workgroups (gridDim.z); > 1 only with a workspace
    float* ws_slabs;   // [tile][kz][64 lanes][4] partial accumulators
    int* ws_count;     // [tile] arrival counters, zero between launches
    int wt;            // 1: w is in the tiled layout (below: WT) -- the decode forms only
};

#define GEMM_U 4  // one-block form: K steps (of 16) whose loads are issued together (4 float4 of W + 4 of x per lane: the 48-VGPR budget)
#define GEMM_U_RB 8  // the same for the prefill form (512 threads, its own CU)
#define GEMM_WS_TILES 1024  // 16 x 16 output tiles a workspace covers (64 column tiles x 16 row blocks: gemm_kz splits K only where every decode launch fits)
#define GEMM_KZ_MAX 4       // cap of the split-K depth of the decode GEMMs (the workspace holds GEMM_KZ_MAX slabs per tile)
#define GEMM_KZ_MIN_K 2048  // the shallowest K that is split over workgroups
#define GEMM_DECODE_MAX_M 256  // up to this many rows the weight-stream kernel below runs; beyond, the prefill form

// LayerNorm statistics -> (mean, rstd) and the epilogue of one output value: single definitions with floating-point
// contraction off, so that every instantiation of the kernel below rounds identically (a row's result must not depend on
// how many other rows share its launch: the grouped decode step is bit-identical to one step per batch).
__device__ __forceinline__ void ln_finish(float a, float b, int K, float eps, float& mean, float& rstd) {
#pragma clang fp contract(off)
    mean = a / K;
    const float var = fmaxf(b / K - mean * mean, 0.f);
    rstd = rsqrtf(var + eps);
}
__device__ __forceinline__ float gemm_epilogue(float v, bool ln, float rstd, float mean, float sn, float bv, int epi, float rv) {
#pragma clang fp contract(off)
    if (ln) v = rstd * (v - mean * sn);
    v += bv;
    if (epi == 1) v = gelu_erf(v);
    if (epi == 2) v += rv;
    return v;
}

// The weight-stream kernel (M <= GEMM_DECODE_MAX_M rows: decode steps, small prefills).
//
// FOOTPRINT FIRST.  The decode step runs beside the frame decoder of another batch, whose convolution workgroups (8 waves x
// 210-225 VGPRs, ~100 KB of LDS) hold every CU: two such waves per SIMD leave 48 VGPRs per lane and ~56 KB of LDS.  A
// workgroup that fits into that remainder is dispatched at once next to the convolution; one that does not waits for a
// convolution workgroup to retire (~100 us).  Measured with a chain of dependent 16 MB weight-stream launches beside the
// real decoder (tools/chain_probe.py, profiles/r03_chain_probe.txt): 512 threads x 200 VGPRs 41 us per launch, 512 x 100
// (the round-2 kernel) 16 us, 256 x 56 14 us, 256 x <= 48 VGPRs with <= 56 KB LDS 10 us (5.8 us alone).  Hence: 256 threads,
// at most 48 VGPRs, a few KB of LDS -- bytes in flight per workgroup are what the registers allow (4 float4 of W and of x
// per lane), and the launch gets its bandwidth from the NUMBER of workgroups.
//   * workgroup = 16 rows x 16 columns (up to 16 rows in the launch; 2 x 2 such blocks beyond: see the template), 4 waves = 4 K
//     slices; each lane issues the float4 loads of a 64-deep K batch of W
//     (row n = lane&15, k = k0+4*(lane>>4)+t) and of x (same k map, row = lane&15, served by L2) before the MFMAs of the batch;
//   * no LDS staging, no barrier in the main loop; the K slices are summed through LDS in a fixed order (wave 0 first;
//     bitwise reproducible, no float atomics); deep K (>= 2048) also splits over `kz` workgroups (last-arriver reduction);
//   * more rows than 16 (the stacked rows of several batches in one decode step, ccvs_gpt_decode.groups) = more row blocks
//     in gridDim.y: they run at the same time on other CUs and share the weight tile through L2 / the Infinity Cache.  A
//     row's arithmetic depends on N and K only (K slicing, MFMA order, slab order, epilogue), never on M;
//   * LayerNorm folded in algebraically and the K / V column blocks of the QKV projection scattered straight into the KV
//     cache, as described above.
// The operands of the address arithmetic come first and as plain kernel arguments: with -mllvm
// -amdgpu-kernarg-preload-count they are delivered in SGPRs when the wave starts (gfx950 kernarg preload), so the weight
// and activation loads of this latency-bound kernel go out without first waiting for a scalar load of the argument block.
#define GEMM_WAVES 4
// RB x CB blocks of 16 x 16 outputs per workgroup (round 5).  With one block per workgroup the rows' activations are re-read by
// every column tile and the weights by every row block: a 64-row step moved 8 x its unique bytes through the CUs' vector-memory
// pipelines (33.5 MB per 1024 x 1024 layer for 4 MB of weights), and that pipeline -- ~12 bytes per clock and CU, L2 hits
// included -- is what the token loops and the frame decoder beside them compete for: with those re-reads switched off
// (every lane reading row 0 of x and of W -- wrong results; an experiment switch of the round, removed again: reading it cost the one-block form 0.5 us in front of its first load) the bench line went from 213 to 237 frames/s (profiles/r05_gemm_tile_ab.txt).  A 2 x 2 block
// tile halves both re-reads at 8 + 8 + 16 registers for the two operands and the four accumulators (one 16-deep K batch in
// flight instead of four: U) -- 32 VGPRs + 16 AGPRs, the same 48; the blocks' arithmetic is the one-block kernel's, bit for bit
// -- the same K slices per wave, the same MFMA order per block, the same slice order in the reduction -- so a row does not
// depend on the tile it falls into.  Same box, 20 batches: 210.5 -> 227.8 frames/s, the token step beside the decoder 7.88 ->
// 7.22 ms, the convolutions beside it 87 -> 95 TFLOP/s; alone the step costs the same (3.17 against 3.25 ms).  Larger tiles
// (4 x 2, 2 x 4: 112 registers, a quarter of the workgroups) lose: 206-208 frames/s, 4.07 ms alone.
// LDS of one tile: the K slices' partial blocks, their LayerNorm sums, the rows' (mean, rstd)
#define GEMM16_RED_WORDS(NB) (GEMM_WAVES * (NB) * 64 * 4)
#define GEMM16_STAT_WORDS(RB) (GEMM_WAVES * (RB) * 16 * 2)
#define GEMM16_FIN_WORDS(RB) ((RB) * 16 * 2)
// One tile (block (bx, by, bz) of the launch's grid) of the weight-stream GEMM: the body of gemm16_kernel, and of the GEMM phases of
// the persistent decode step (gpt_step_kernel: COH = true -- the activations x / res / y / the new cache rows are handed over
// between workgroups of ONE launch, so they are read and written with sc1 accesses; the arithmetic is the same instruction for
// instruction, so a row's bits do not depend on which of the two forms computed it).
// PT: `Gemm16` (the kernel's own argument block) or `__attribute__((address_space(4))) Gemm16` (an entry of the persistent step's phase
// table in constant memory: every `p.field` is then a scalar load at its point of use -- the epilogue's operands are not held
// in registers across the K loop -- and the pointers read from it are generic, hence GP() = the cast through the global address space).
// WT: W in the TILED layout (ccvs_gpt_decode.w_tiled; include/ccvs_hip_gemm.h).  Row-major, the 16 lanes of a quarter-wave read 16 bytes each
// from 16 different rows: one 1-KB wave load touches 16 128-byte lines and uses half of each (the other half is the next K batch's).
// Tiled, the 1 KB that a wave loads for column tile ct and K batch kb IS one block of memory, at float offset (ct * K / 16 + kb) * 256,
// lane l = li + 16 g owning floats 4 l .. 4 l + 3 = W[16 ct + li][16 kb + 4 g ..]: 8 whole, aligned lines per wave load, the next batch
// 1 KB on.  The same floats reach the same lanes: registers, MFMA order, K slices and reduction are untouched, so the bits are too.
// N is padded to whole column tiles by the packer (last row repeated), so a ragged tile needs no clamp; a column tile wholly outside reads the last one.
template <int RB, int CB, int U, bool COH, bool WT, typename PT>
__device__ __forceinline__ void gemm16_tile(const float* __restrict__ x_, const float* __restrict__ w_, long ldx_, int K_, int N_, int M_, int ks_,
                                            int kz_, const PT& p, int bx_, int by_, int bz_, float* __restrict__ red, float* __restrict__ stat,
                                            float* __restrict__ fin) {
#define GP(ptr) gp_<COH>(ptr)
    constexpr int NB = RB * CB;
    constexpr int XAUX = COH ? 16 : 0;   // sc1 on the activation loads
    int tid = thread_id<COH>(), lane = tid & 63, wave = tid >> 6;
    int li = lane & 15, g = lane >> 4;
    const int m0 = by_ * 16 * RB, ncol0 = bx_ * 16 * CB;
    const int kper = opaque_if<COH>(K_ / (ks_ * kz_));   // (opaque: the K loops' entry tests are otherwise evaluated once per phase and parked, as booleans, in vector registers)
    const int kbase = bz_ * (K_ / kz_);
    const bool active = wave < ks_;
    // Buffer loads: a wave-uniform 128-bit descriptor per tensor in SGPRs + ONE 32-bit byte offset per lane and block (the
    // K position goes into the scalar offset / the instruction's immediate) instead of 64-bit pointer pairs and their
    // adds -- the 48-VGPR budget.  The launcher checks that both tensors stay below 2^31 bytes.
    const unsigned koff = kbase + (active ? wave : 0) * kper + 4 * g;
    unsigned wofs[CB], xofs[RB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {   // tails: computed on a valid row, dropped at the store
        if constexpr (WT) {   // (every slice boundary is a multiple of 16: gemm16_plan)
            const int ct = min(bx_ * CB + cb, ((N_ + 15) >> 4) - 1);
            wofs[cb] = (((unsigned)ct * (unsigned)(K_ >> 4) + ((koff - 4 * g) >> 4)) * 256u + 4u * lane) * 4u;
        } else {
            const int nrow = min(ncol0 + 16 * cb + li, N_ - 1);
            wofs[cb] = ((unsigned)nrow * (unsigned)K_ + koff) * 4u;
        }
    }
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const int mrow = min(m0 + 16 * rb + li, M_ - 1);
        xofs[rb] = ((unsigned)mrow * (unsigned)ldx_ + koff) * 4u;
    }
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(w_), 0, (WT ? (N_ + 15) & ~15 : N_) * K_ * 4, 0x00020000);
    constexpr int WSTEP = WT ? 1024 : 64;   // bytes from one 16-deep K batch of a lane's W to the next
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x_), 0, (int)(M_ * ldx_ * 4), 0x00020000);
    f32x4 acc[RB][CB];
    float sx[RB], sxx[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        sx[rb] = 0.f; sxx[rb] = 0.f;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) acc[rb][cb] = {0.f, 0.f, 0.f, 0.f};
    }
    // The K loop, once per kind of launch (LN: the folded LayerNorm's): the LayerNorm copy subtracts the row's shift (ln_shift, from the
    // row's first 16 bytes) from every x it has loaded and sums the statistics of what it then feeds to the MFMAs; the plain copy is
    // the loop without either -- no test of p.ln_s inside a batch.
    auto k_loop = [&](auto ln_tag) {
        constexpr bool LN = decltype(ln_tag)::value;
        float lc[RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) lc[rb] = LN ? ln_shift(buf_load4<XAUX>(xr, xofs[rb] - koff * 4u, 0)) : 0.f;
        // full batches: U unconditional 16-byte loads per block row of W and of x in flight per lane, then the MFMAs (one
        // accumulator chain per block: the dependent MFMAs of a chain cost a few cycles each)
        int k0 = 0;
        for (; k0 + 16 * U <= kper; k0 += 16 * U) {
            f32x4 wv[CB][U], xv[RB][U];
#pragma unroll
            for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                for (int u = 0; u < U; ++u) wv[cb][u] = buf_load4(wr, wofs[cb], k0 * (WSTEP / 16) + WSTEP * u);
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int u = 0; u < U; ++u) xv[rb][u] = buf_load4<XAUX>(xr, xofs[rb], k0 * 4 + 64 * u);
            __builtin_amdgcn_sched_barrier(0);   // every load of the batch goes out before its first MFMA (hipcc otherwise sinks half of them between the MFMAs)
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) {
                    if constexpr (LN) ln_center(xv[rb][u], lc[rb]);
#pragma unroll
                    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                        for (int t = 0; t < 4; ++t) acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[rb][u][t], wv[cb][u][t], acc[rb][cb], 0, 0, 0);
                    if constexpr (LN) ln_accum(xv[rb][u], sx[rb], sxx[rb]);
                }
            }
        }
        for (; k0 < kper; k0 += 16) {  // remainder (small K only)
            f32x4 w1[CB], x1[RB];
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) w1[cb] = buf_load4(wr, wofs[cb], k0 * (WSTEP / 16));
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) x1[rb] = buf_load4<XAUX>(xr, xofs[rb], k0 * 4);
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                if constexpr (LN) ln_center(x1[rb], lc[rb]);
#pragma unroll
                for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(x1[rb][t], w1[cb][t], acc[rb][cb], 0, 0, 0);
                if constexpr (LN) ln_accum(x1[rb], sx[rb], sxx[rb]);
            }
        }
    };
    if (active) {
        // (the persistent step: tested on the pointer's own words where it is used -- as a loop-invariant boolean it is parked in a vector register)
        const unsigned long long lnp = (unsigned long long)p.ln_s;
        if (opaque_if<COH>((int)((unsigned)lnp | (unsigned)(lnp >> 32))) != 0) k_loop(ln_on<true>{});
        else k_loop(ln_on<false>{});
    }
    if constexpr (WT || COH) {
        // the lane maps of the reduction and the epilogue, derived again from a thread index the optimiser cannot see through: ONE register
        // live across the K loop instead of the maps themselves (with them, the tiled 2 x 2 form took 36 + 16 registers, not 32 + 16; the
        // persistent step's row-major 2 x 2 body, under its 64-register cap, spilled the thread index once the LayerNorm shifts joined them)
        asm volatile("" : "+v"(tid));
        // (the launch form knows threadIdx.x's range and runs the finishing loop below at most once: say so again.  The persistent form never
        // knew -- thread_id<true> -- and with the loop unrolled its phase loop spills 52-84 bytes)
        if constexpr (!COH) __builtin_assume(tid >= 0 && tid < 64 * GEMM_WAVES);
        lane = tid & 63; wave = tid >> 6; li = lane & 15; g = lane >> 4;
    }
    if (p.ln_s) {  // lanes li, li+16, li+32, li+48 hold the four k-groups of row li
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            float a = sx[rb], b = sxx[rb];
            a += __shfl_xor(a, 16, 64); a += __shfl_xor(a, 32, 64);
            b += __shfl_xor(b, 16, 64); b += __shfl_xor(b, 32, 64);
            if (g == 0) { stat[((wave * RB + rb) * 16 + li) * 2] = a; stat[((wave * RB + rb) * 16 + li) * 2 + 1] = b; }
        }
    }
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) *reinterpret_cast<f32x4*>(red + ((wave * NB + rb * CB + cb) * 64 + lane) * 4) = acc[rb][cb];
    __syncthreads();
    if (p.ln_s && tid < 16 * RB) {
        const int rb = tid >> 4, r = tid & 15;
        float a = 0.f, b = 0.f;
        for (int w = 0; w < GEMM_WAVES; ++w) { a += stat[((w * RB + rb) * 16 + r) * 2]; b += stat[((w * RB + rb) * 16 + r) * 2 + 1]; }
        float mean, rstd;
        ln_finish(a, b, opaque_if<COH>(p.K), p.ln_eps, mean, rstd);
        fin[tid * 2] = mean;
        fin[tid * 2 + 1] = rstd;
    }
    __syncthreads();
    // wave w finishes the blocks w, w + 4, ... (one block per workgroup: wave 0, as before)
#pragma unroll 1
    for (int blk = wave; blk < NB; blk += GEMM_WAVES) {
        const int rb = blk / CB, cb = blk - rb * CB;
        f32x4 a4;
        if constexpr (NB == 1) a4 = acc[0][0];   // (wave 0: its own slice is still in registers)
        else a4 = *reinterpret_cast<const f32x4*>(red + (blk * 64 + lane) * 4);
#pragma unroll
        for (int s = 1; s < GEMM_WAVES; ++s) a4 += *reinterpret_cast<const f32x4*>(red + ((s * NB + blk) * 64 + lane) * 4);
        const int mb0 = m0 + 16 * rb, nb0 = ncol0 + 16 * cb;
        if (mb0 >= p.M || nb0 >= p.N) continue;   // a block wholly outside the matrix (ragged row / column counts)

        bool finisher = true;
        if (p.kz > 1) {
            // K is also split over gridDim.z workgroups (few output columns: keeps all 256 CUs streaming W).
            // Each publishes its 16x16 partial, the LAST arriver sums the slabs in slice order (bitwise
            // reproducible) and runs the epilogue.  The slabs are written and read with agent-scope (sc1)
            // accesses, which go through to memory and bypass the per-XCD L2s: no release / acquire fence is
            // needed -- on this chip a fence is an L2 write-back + invalidate costing several us, and all the
            // hand-off needs is slab stores acknowledged (vmcnt 0) before the ticket, and slab loads after it.
            const int tile = (mb0 >> 4) * ((p.N + 15) >> 4) + (nb0 >> 4);   // the 16 x 16 block's own slabs and counter
            float* slabs = GP(p.ws_slabs) + (long)tile * p.kz * 256;
            float* mine = slabs + (bz_ * 64 + lane) * 4;
#pragma unroll
            for (int c = 0; c < 4; ++c) __hip_atomic_store(mine + c, a4[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            int ticket = 0;
            if (lane == 0) ticket = __hip_atomic_fetch_add(GP(p.ws_count) + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ticket = __builtin_amdgcn_readfirstlane(ticket);
            finisher = ticket == p.kz - 1;
            if (finisher) {
#pragma unroll
                for (int c = 0; c < 4; ++c) a4[c] = __hip_atomic_load(slabs + lane * 4 + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                for (int z = 1; z < p.kz; ++z) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) a4[c] += __hip_atomic_load(slabs + (z * 64 + lane) * 4 + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                if (lane == 0) __hip_atomic_store(GP(p.ws_count) + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }

        // D[row = 4*g + r][col = li]
        const int col = nb0 + li;
        if (finisher && col < p.N) {
            const float bv = p.bias ? GP(p.bias)[col] : 0.f;
            const float sn = p.ln_s ? GP(p.ln_s)[col] : 0.f;
            const int pD = opaque_if<COH>(p.D), pTq = opaque_if<COH>(p.Tq);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = mb0 + 4 * g + r;
                if (row >= p.M) continue;
                const float rv = p.epi == 2 ? ld_act<COH>(GP(p.res) + (long)row * p.ldy + col) : 0.f;
                const float v = gemm_epilogue(a4[r], p.ln_s != nullptr, fin[(rb * 16 + 4 * g + r) * 2 + 1], fin[(rb * 16 + 4 * g + r) * 2], sn, bv, p.epi, rv);
                if (p.kcache && col >= p.C) {
                    const int cc = col - p.C;
                    float* cache = cc >= p.C ? GP(p.vcache) : GP(p.kcache);
                    const int c2 = cc >= p.C ? cc - p.C : cc;
                    const int h = c2 / pD, d = c2 - h * pD;
                    const int b = row / pTq, t = row - b * pTq;
                    const int pos = p.pos0 + (p.pos_dev ? GP(p.pos_dev)[p.grp_rows > 0 ? b / opaque_if<COH>(p.grp_rows) : 0] : 0);
                    if (pos + t < p.Tmax) st_act<COH>(cache + (((long)b * p.H + h) * p.Tmax + pos + t) * pD + d, v);
                } else {
                    st_act<COH>(GP(p.y) + (long)row * p.ldy + col, v);
                }
            }
        }
    }
#undef GP
}

template <int RB, int CB, int U, bool WT>
__global__ __launch_bounds__(64 * GEMM_WAVES) void gemm16_kernel(const float* __restrict__ x_, const float* __restrict__ w_, long ldx_, int K_, int N_,
                                                                int M_, int ks_, int kz_, Gemm16 p) {
    __shared__ __attribute__((aligned(16))) float red[GEMM16_RED_WORDS(RB * CB)];
    __shared__ float stat[GEMM16_STAT_WORDS(RB)];
    __shared__ float fin[GEMM16_FIN_WORDS(RB)];
    gemm16_tile<RB, CB, U, false, WT>(x_, w_, ldx_, K_, N_, M_, ks_, kz_, p, blockIdx.x, blockIdx.y, blockIdx.z, red, stat, fin);
}

// Prefill form (M > GEMM_DECODE_MAX_M rows): one workgroup computes RB row blocks of 16 against the SAME 16 output columns,
// so a weight tile is fetched once per 16*RB rows.  K sliced over the 8 waves only (kz = 1: with hundreds of row blocks
// the chip is full without split-K), argument block read the ordinary way.
template <int RB>
__global__ __launch_bounds__(512) void gemm16_rb_kernel(Gemm16 p) {
    __shared__ __attribute__((aligned(16))) float red[RB * 8 * 64 * 4];
    __shared__ float stat[RB * 8 * 16 * 2];
    __shared__ float fin[RB * 16 * 2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, g = lane >> 4;
    const int m0 = blockIdx.y * 16 * RB, ncol0 = blockIdx.x * 16;
    const int nrow = min(ncol0 + li, p.N - 1);
    const int kper = p.K / p.ks;
    const bool active = wave < p.ks;
    const float* wp = p.w + (long)nrow * p.K + (active ? wave : 0) * kper + 4 * g;
    const float* xp[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) xp[rb] = p.x + (long)min(m0 + 16 * rb + li, p.M - 1) * p.ldx + (active ? wave : 0) * kper + 4 * g;
    f32x4 acc0[RB], acc1[RB];
    float sx[RB], sxx[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) { acc0[rb] = {0.f, 0.f, 0.f, 0.f}; acc1[rb] = {0.f, 0.f, 0.f, 0.f}; sx[rb] = 0.f; sxx[rb] = 0.f; }
    float lc[RB];   // the folded LayerNorm's shift of this lane's rows (ln_shift)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
        lc[rb] = active && p.ln_s ? ln_shift(*reinterpret_cast<const float4*>(p.x + (long)min(m0 + 16 * rb + li, p.M - 1) * p.ldx)) : 0.f;
    if (active) {
        int k0 = 0;
        for (; k0 + 16 * GEMM_U_RB <= kper; k0 += 16 * GEMM_U_RB) {
            float4 wv[GEMM_U_RB];
#pragma unroll
            for (int u = 0; u < GEMM_U_RB; ++u) wv[u] = *reinterpret_cast<const float4*>(wp + k0 + 16 * u);
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                float4 xv[GEMM_U_RB];
#pragma unroll
                for (int u = 0; u < GEMM_U_RB; ++u) xv[u] = *reinterpret_cast<const float4*>(xp[rb] + k0 + 16 * u);
#pragma unroll
                for (int u = 0; u < GEMM_U_RB; ++u) {
                    if (p.ln_s) { ln_center(xv[u], lc[rb]); ln_accum(xv[u], sx[rb], sxx[rb]); }
                    acc0[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[u].x, wv[u].x, acc0[rb], 0, 0, 0);
                    acc1[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[u].y, wv[u].y, acc1[rb], 0, 0, 0);
                    acc0[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[u].z, wv[u].z, acc0[rb], 0, 0, 0);
                    acc1[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[u].w, wv[u].w, acc1[rb], 0, 0, 0);
                }
            }
        }
        for (; k0 < kper; k0 += 16) {
            const float4 w1 = *reinterpret_cast<const float4*>(wp + k0);
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                float4 x1 = *reinterpret_cast<const float4*>(xp[rb] + k0);
                if (p.ln_s) { ln_center(x1, lc[rb]); ln_accum(x1, sx[rb], sxx[rb]); }
                acc0[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.x, w1.x, acc0[rb], 0, 0, 0);
                acc1[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.y, w1.y, acc1[rb], 0, 0, 0);
                acc0[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.z, w1.z, acc0[rb], 0, 0, 0);
                acc1[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.w, w1.w, acc1[rb], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const f32x4 acc = acc0[rb] + acc1[rb];
        if (p.ln_s) {
            float a = sx[rb], b = sxx[rb];
            a += __shfl_xor(a, 16, 64); a += __shfl_xor(a, 32, 64);
            b += __shfl_xor(b, 16, 64); b += __shfl_xor(b, 32, 64);
            if (g == 0) { stat[((rb * 8 + wave) * 16 + li) * 2] = a; stat[((rb * 8 + wave) * 16 + li) * 2 + 1] = b; }
        }
        *reinterpret_cast<f32x4*>(red + ((rb * 8 + wave) * 64 + lane) * 4) = acc;
    }
    __syncthreads();
    if (p.ln_s && tid < 16 * RB) {
        const int rb = tid >> 4, r = tid & 15;
        float a = 0.f, b = 0.f;
        for (int w = 0; w < 8; ++w) { a += stat[((rb * 8 + w) * 16 + r) * 2]; b += stat[((rb * 8 + w) * 16 + r) * 2 + 1]; }
        float mean, rstd;
        ln_finish(a, b, p.K, p.ln_eps, mean, rstd);
        fin[tid * 2] = mean;
        fin[tid * 2 + 1] = rstd;
    }
    __syncthreads();
    if (wave >= RB) return;  // wave rb finishes row block rb
    const int rb = wave;
    f32x4 acc = *reinterpret_cast<const f32x4*>(red + ((rb * 8) * 64 + lane) * 4);
#pragma unroll
    for (int s2 = 1; s2 < 8; ++s2) acc += *reinterpret_cast<const f32x4*>(red + ((rb * 8 + s2) * 64 + lane) * 4);
    const int col = ncol0 + li;
    if (col >= p.N) return;
    const float bv = p.bias ? p.bias[col] : 0.f;
    const float sn = p.ln_s ? p.ln_s[col] : 0.f;
    int pos0 = p.pos0;
    if (p.kcache && p.pos_dev) pos0 += *p.pos_dev;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = m0 + 16 * rb + 4 * g + r;
        if (row >= p.M) continue;
        const float v = gemm_epilogue(acc[r], p.ln_s != nullptr, fin[(rb * 16 + 4 * g + r) * 2 + 1], fin[(rb * 16 + 4 * g + r) * 2], sn, bv, p.epi,
                                      p.epi == 2 ? p.res[(long)row * p.ldy + col] : 0.f);
        if (p.kcache && col >= p.C) {
            const int cc = col - p.C;
            float* cache = cc >= p.C ? p.vcache : p.kcache;
            const int c2 = cc >= p.C ? cc - p.C : cc;
            const int h = c2 / p.D, d = c2 - h * p.D;
            const int b = row / p.Tq, t = row - b * p.Tq;
            if (pos0 + t < p.Tmax) cache[(((long)b * p.H + h) * p.Tmax + pos0 + t) * p.D + d] = v;
        } else {
            p.y[(long)row * p.ldy + col] = v;
        }
    }
}

// Whole-sequence form (CCVS_GEMM_SEQ: prefill, teacher-forced forward, re-prefill of a slid window): a dense LDS-tiled GEMM
// on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 products, 157 TFLOP/s peak).  With hundreds to thousands of rows
// the weights are no longer a stream to be read once but operands to be re-used: the row-blocked kernel above fetches every
// operand from global memory per 64 rows x 16 columns (52-82 TFLOP/s).
//   * workgroup = 4 waves = a 128 x 128 output tile, wave w the 64 x 64 quadrant (w >> 1, w & 1): 2 x 2 MFMA blocks, 64
//     accumulator registers; K in stages of 16;
//   * both operands go global -> LDS by LDS-DMA (global_load_lds_dwordx4: no staging registers, the next stage is in flight
//     while this one is multiplied), double-buffered, one barrier per stage.  LDS image of an operand stage:
//     [k quad q = 0..3][row 0..127][4 floats], quads 129 units apart -- a wave-instruction of the DMA fills 64 consecutive
//     rows of one quad (the per-lane SOURCE address does the transposition), and the fragment read of a 32-row block is 32
//     consecutive 16-byte units per lane half: conflict-free ds_read_b128;
//   * lane half h reads k = 8 s + 4 h .. + 3 of sub-step s for both operands, and MFMA j of the sub-step contracts the pair
//     (8 s + j, 8 s + 4 + j): the contraction order over k is free as long as both operands agree;
//   * the folded LayerNorm: the stages hold the raw x; the shifts of the lane's two fragment rows (ln_shift: read from global memory
//     once) are subtracted from the x fragments as they leave LDS, and the row statistics are summed from those very fragments (lane
//     half h: k quads h and 2 + h of rows 64 wr + 32 bi + l31; the two waves of a tile row hold the same fragments and sum the same bits);
//   * epilogue as everywhere (LayerNorm fold, bias, GELU, residual, K / V scatter into the cache); a 32 x 32 block leaves as
//     128-byte row segments.
// A row's arithmetic depends on (N, K) only -- never on M or on the tile the row falls into -- so a batch prefilled alone and
// the same batch inside a stacked token group agree bit for bit (tests/test_pipeline_gpu.py).
// Workgroup order: XCD j (linear id % 8) walks the row tiles j, j + 8, ...: the workgroups that share a row tile of x meet
// in one L2, and every XCD streams the weights once per round of eight row tiles.
#define GS_BM 128
#define GS_QS (GS_BM + 1)   // 16-byte units between the k quads of an operand stage
typedef __attribute__((address_space(3))) void gs_lds_void;
__global__ __launch_bounds__(256, 4) void gemm_seq_kernel(Gemm16 p, int row_tiles, int col_tiles) {
    // two separate LDS variables, one per stage buffer, and the stage loop unrolled by two: hipcc orders a ds_read behind an
    // in-flight LDS-DMA unless the two provably touch different LDS objects -- with one array indexed by (stage & 1) every
    // fragment read waited (vmcnt 0) for the DMA of the NEXT stage issued just before it, and nothing overlapped
    __shared__ __attribute__((aligned(16))) f32x4 sm0[2 * 4 * GS_QS];   // [x | w][quad][row]
    __shared__ __attribute__((aligned(16))) f32x4 sm1[2 * 4 * GS_QS];
    __shared__ float fin[GS_BM * 2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int rt, ct;
    {
        const int w = blockIdx.x;
        if (row_tiles % 8 == 0) {
            const int i = w >> 3;
            rt = (w & 7) + 8 * (i / col_tiles);
            ct = i % col_tiles;
        } else {
            rt = w / col_tiles;
            ct = w - rt * col_tiles;
        }
    }
    const int m0 = rt * GS_BM, n0 = ct * GS_BM;
    // DMA: 16 wave-instructions per stage, 4 per wave: wave q fills k quad q of both operands, two halves of 64 rows each.
    // buffer_load ... lds: a 128-bit descriptor per operand in SGPRs, a per-lane byte offset that never changes and the
    // stage's K offset as the scalar offset -- no address VGPR is rewritten inside the loop (with global_load_lds hipcc builds
    // a 64-bit address in a VGPR pair per DMA and waits, vmcnt 0, for the previous DMA before it overwrites the pair).
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, (int)((long)p.M * p.ldx * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w), 0, (int)((long)p.N * p.K * 4), 0x00020000);
    unsigned xoff[2], woff[2];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        xoff[hf] = (unsigned)((long)min(m0 + 64 * hf + lane, p.M - 1) * p.ldx + 4 * wave) * 4u;
        woff[hf] = (unsigned)((long)min(n0 + 64 * hf + lane, p.N - 1) * p.K + 4 * wave) * 4u;
    }
    int wr = wave >> 1, wc = wave & 1, l31 = lane & 31, h = lane >> 5;
    f32x16 acc[2][2];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[bi][bj][r] = 0.f;
    float sx[2] = {0.f, 0.f}, sxx[2] = {0.f, 0.f};
    float lca[2] = {0.f, 0.f};   // ln_shift of the rows of a[..][0] and a[..][1] (LDS row r = x row min(m0 + r, M - 1)); 0 without LayerNorm
    if (p.ln_s) {
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
            lca[bi] = ln_shift(*reinterpret_cast<const float4*>(p.x + (long)min(m0 + 64 * wr + 32 * bi + l31, p.M - 1) * p.ldx));
    }
    const int nst = p.K / 16;
#define GS_DMA(k0, SM)                                                                                             \
    _Pragma("unroll") for (int hf = 0; hf < 2; ++hf) {                                                             \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (gs_lds_void*)((SM) + wave * GS_QS + 64 * hf), 16, xoff[hf], (k0) * 4, 0, 0);               \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (gs_lds_void*)((SM) + 4 * GS_QS + wave * GS_QS + 64 * hf), 16, woff[hf], (k0) * 4, 0, 0);  \
    }
#define GS_STAGE(SM, NEXT_DMA)                                                                                     \
    {                                                                                                              \
        const f32x4* xa = (SM);                                                                                    \
        const f32x4* wb = (SM) + 4 * GS_QS;                                                                        \
        f32x4 a[2][2], b[2][2];                                                                                    \
        _Pragma("unroll") for (int s2 = 0; s2 < 2; ++s2) {                                                         \
            const int q = 2 * s2 + h;                                                                              \
            _Pragma("unroll") for (int bi = 0; bi < 2; ++bi) a[s2][bi] = xa[q * GS_QS + 64 * wr + 32 * bi + l31];  \
            _Pragma("unroll") for (int bj = 0; bj < 2; ++bj) b[s2][bj] = wb[q * GS_QS + 64 * wc + 32 * bj + l31];  \
        }                                                                                                          \
        /* every LDS read of this stage is issued BEFORE the next stage's DMA: hipcc orders a ds_read behind any */ \
        /* LDS-DMA still in flight (s_waitcnt vmcnt(0)), which would serialise the stages                        */ \
        NEXT_DMA                                                                                                   \
        /* lca is 0 in a launch without LayerNorm, and x - 0 is x, bit for bit */                                  \
        _Pragma("unroll") for (int s2 = 0; s2 < 2; ++s2)                                                           \
            _Pragma("unroll") for (int bi = 0; bi < 2; ++bi) ln_center(a[s2][bi], lca[bi]);                        \
        _Pragma("unroll") for (int s2 = 0; s2 < 2; ++s2)                                                           \
            _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                          \
                _Pragma("unroll") for (int bi = 0; bi < 2; ++bi)                                                   \
                    _Pragma("unroll") for (int bj = 0; bj < 2; ++bj)                                               \
                        acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s2][bi][j], b[s2][bj][j], acc[bi][bj], 0, 0, 0); \
        if (p.ln_s) {                                                                                              \
            _Pragma("unroll") for (int s2 = 0; s2 < 2; ++s2)                                                       \
                _Pragma("unroll") for (int bi = 0; bi < 2; ++bi) ln_accum(a[s2][bi], sx[bi], sxx[bi]);             \
        }                                                                                                          \
    }
    GS_DMA(0, sm0)
    for (int st = 0; st < nst; st += 2) {
        __syncthreads();                                   // stage st has landed (the barrier drains vmcnt) and the other buffer is free
        GS_STAGE(sm0, if (st + 1 < nst) { GS_DMA(16 * (st + 1), sm1) })
        if (st + 1 >= nst) break;
        __syncthreads();
        GS_STAGE(sm1, if (st + 2 < nst) { GS_DMA(16 * (st + 2), sm0) })
    }
#undef GS_DMA
#undef GS_STAGE
    {   // the epilogue's lane maps, derived again from a thread index the optimiser cannot see through: the stage loop runs at the
        // 128-register cap of four workgroups per CU, and a map kept across it for the epilogue's sake is spilled
        int t = threadIdx.x;
        asm volatile("" : "+v"(t));
        wr = t >> 7; wc = (t >> 6) & 1; l31 = t & 31; h = (t >> 5) & 1;
    }
    if (p.ln_s) {
#pragma unroll
        for (int bi = 0; bi < 2; ++bi) {
            const float a = sx[bi] + __shfl_xor(sx[bi], 32, 64), b = sxx[bi] + __shfl_xor(sxx[bi], 32, 64);
            if (wc == 0 && h == 0) {
                float mean, rstd;
                ln_finish(a, b, p.K, p.ln_eps, mean, rstd);
                fin[(64 * wr + 32 * bi + l31) * 2] = mean;
                fin[(64 * wr + 32 * bi + l31) * 2 + 1] = rstd;
            }
        }
        __syncthreads();
    }
    int pos0 = p.pos0;
    if (p.kcache && p.pos_dev) pos0 += *p.pos_dev;
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
        const int col = n0 + 64 * wc + 32 * bj + l31;
        if (col >= p.N) continue;
        const float bv = p.bias ? p.bias[col] : 0.f;
        const float sn = p.ln_s ? p.ln_s[col] : 0.f;
#pragma unroll
        for (int bi = 0; bi < 2; ++bi) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lr = 64 * wr + 32 * bi + (r & 3) + 8 * (r >> 2) + 4 * h;
                const int row = m0 + lr;
                if (row >= p.M) continue;
                const float v = gemm_epilogue(acc[bi][bj][r], p.ln_s != nullptr, p.ln_s ? fin[lr * 2 + 1] : 0.f, p.ln_s ? fin[lr * 2] : 0.f, sn, bv,
                                              p.epi, p.epi == 2 ? p.res[(long)row * p.ldy + col] : 0.f);
                if (p.kcache && col >= p.C) {
                    const int cc = col - p.C;
                    float* cache = cc >= p.C ? p.vcache : p.kcache;
                    const int c2 = cc >= p.C ? cc - p.C : cc;
                    const int hh = c2 / p.D, d = c2 - hh * p.D;
                    const int b = row / p.Tq, t = row - b * p.Tq;
                    if (pos0 + t < p.Tmax) cache[(((long)b * p.H + hh) * p.Tmax + pos0 + t) * p.D + d] = v;
                } else {
                    p.y[(long)row * p.ldy + col] = v;
                }
            }
        }
    }
}

// K slices across workgroups (split-K): spreads GEMMs with few output columns over the chip.  Pays only for deep K:
// the release/acquire hand-off costs ~3-4 us (measured).
// A function of N and K only -- never of M -- so that a row's K partition, hence its rounding,
// does not depend on how many rows share the launch.  Hence only where the workspace covers the blocks of EVERY decode launch
// of these N columns, GEMM_DECODE_MAX_M rows included (at most 64 column tiles): whether this launch's rows happen to fit is
// not asked.
static int gemm_kz(const Gemm16& g) {
    const int tiles = cdiv(g.N, 16);
    int kz = 1;
    if (g.ws_slabs && !g.ln_s && tiles * cdiv(GEMM_DECODE_MAX_M, 16) <= GEMM_WS_TILES)
        while (g.K >= GEMM_KZ_MIN_K && kz < GEMM_KZ_MAX && tiles * kz * 2 <= 256 && g.K % (16 * GEMM_WAVES * kz * 2) == 0) kz *= 2;
    return kz;
}

// CCVS_GEMM_TILE2=0 (a test hook: tests/gemm_tile_worker.py): one 16 x 16 block per workgroup (rounds 3-4) whatever M is -- same bits
static bool gemm_tile2() {
    static const bool v = getenv_int("CCVS_GEMM_TILE2", 1) != 0;
    return v;
}

// How a GEMM runs, as a function of its descriptor alone: the form (below), and into g the K slicing -- kz workgroups x ks waves --
// that a row's rounding depends on.  launch_gemm16 and the phase table of the persistent decode step both take it from here.
// Which kernel runs is a property of the CALL KIND, never of how many rows share the launch: the two forms partition K
// differently (4 waves x kz slices and one accumulator chain vs 8 waves and two chains), so their low bits differ, and a
// row must come out the same whether its batch is prefilled alone or stacked with the other batches of a token group
// (B t0 <= 256 alone, G B t0 > 256 stacked).  Whole-sequence calls (prefill, teacher-forced forward, re-prefill of a slid
// window: CCVS_GEMM_SEQ in the epilogue word, Tq > 1 for the QKV form) always take the row-blocked form; single-position
// calls (decode steps) take the weight-stream form up to GEMM_DECODE_MAX_M rows and the row-blocked one beyond.
// weight-stream form with one 16 x 16 block / 2 x 2 blocks per workgroup (the blocks' bits do not depend on the tile) | row-blocked | dense whole-sequence
enum GemmForm { GEMM_FORM_TILE1, GEMM_FORM_TILE2, GEMM_FORM_RB, GEMM_FORM_SEQ };
static GemmForm gemm16_plan(Gemm16& g) {
    const bool decode_form = !g.seq && g.M <= GEMM_DECODE_MAX_M;
    g.kz = decode_form ? gemm_kz(g) : 1;
    g.ks = decode_form ? GEMM_WAVES : 8;
    while (g.ks > 1 && g.K % (16 * g.ks * g.kz) != 0) g.ks >>= 1;
    // 2 x 2 blocks from three row blocks on (stacked batches): with two, N / 32 workgroups are too few alone (2.03 against 1.53 ms per step)
    if (decode_form) return gemm_tile2() && g.M > 32 && g.N >= 32 ? GEMM_FORM_TILE2 : GEMM_FORM_TILE1;
    static const int seq_dense = getenv_int("CCVS_GEMM_SEQ_DENSE", 1);   // 0 (a test hook: tests/gemm_seq_worker.py): the row-blocked weight-stream form of rounds 2-3
    const bool fits = (long)g.M * g.ldx * 4 < (1L << 31) && (long)g.N * g.K * 4 < (1L << 31);   // (buffer descriptors: 32-bit byte offsets)
    return g.seq && seq_dense && fits ? GEMM_FORM_SEQ : GEMM_FORM_RB;
}

// gemm_kz grants split-K only where the workspace holds every block of a decode launch (M <= GEMM_DECODE_MAX_M): a planned launch that
// outgrows it is a bug in this file -- refused by both forms of the step, never run on another K partition (a row's bits would then
// depend on M) or past the workspace's end
static bool gemm_ws_holds(const Gemm16& g) { return g.kz == 1 || cdiv(g.N, 16) * cdiv(g.M, 16) <= GEMM_WS_TILES; }

// Tiled weights (g.wt; after gemm16_plan): a wave's K slice starts and ends on a 16-deep block -- the plan's slices always do -- and the
// padded matrix stays below 2^31 bytes (32-bit buffer offsets).  Checked by both forms of the step and by ccvs_gemm_tiled.
static bool gemm_wt_holds(const Gemm16& g) {
    return !g.wt || ((long)cdiv(g.N, 16) * 16 * g.K * 4 < (1L << 31) && g.K % (g.ks * g.kz) == 0 && (g.K / (g.ks * g.kz)) % 16 == 0);
}

static int launch_gemm16(Gemm16& g, hipStream_t st, const char* name) {
    if (!(g.x && g.w && g.y)) { ccvs_set_error("%s: null pointer", name); return CCVS_ERR_ARG; }
    if (!(g.M > 0 && g.N > 0 && g.K > 0)) { ccvs_set_error("%s: empty tensor", name); return CCVS_ERR_ARG; }
    if (g.K % 16 != 0 || g.ldx % 4 != 0) { ccvs_set_error("%s: K=%d must be a multiple of 16 (ldx %% 4 == 0)", name, g.K); return CCVS_ERR_ARG; }
    if (g.epi < 0 || g.epi > 2 || (g.epi == 2 && !g.res)) { ccvs_set_error("%s: bad epilogue", name); return CCVS_ERR_ARG; }
    const GemmForm form = gemm16_plan(g);
    const bool decode_form = form == GEMM_FORM_TILE1 || form == GEMM_FORM_TILE2;
    if (!gemm_ws_holds(g)) { ccvs_set_error("%s: split-K over %d x %d blocks outgrows the workspace", name, cdiv(g.M, 16), cdiv(g.N, 16)); return CCVS_ERR_ARG; }
    if (decode_form && ((long)g.N * g.K * 4 >= (1L << 31) || (long)g.M * g.ldx * 4 >= (1L << 31))) {
        ccvs_set_error("%s: operand beyond 2^31 bytes (32-bit buffer offsets)", name);
        return CCVS_ERR_ARG;
    }
    if (g.wt && !decode_form) { ccvs_set_error("%s: tiled weights are read by the decode forms only (single position, M <= %d)", name, GEMM_DECODE_MAX_M); return CCVS_ERR_ARG; }
    if (!gemm_wt_holds(g)) {
        ccvs_set_error("%s: tiled weights need K slices of whole 16-deep batches and fewer than 2^31 bytes", name);
        return CCVS_ERR_ARG;
    }
    if (!decode_form && g.grp_rows > 0) { ccvs_set_error("%s: row groups need M <= %d", name, GEMM_DECODE_MAX_M); return CCVS_ERR_ARG; }
    if (form == GEMM_FORM_SEQ) {
        const int rt = cdiv(g.M, GS_BM), ct = cdiv(g.N, GS_BM);
        hipLaunchKernelGGL(gemm_seq_kernel, dim3(rt * ct), dim3(256), 0, st, g, rt, ct);
    } else if (form == GEMM_FORM_RB)
        hipLaunchKernelGGL((gemm16_rb_kernel<4>), dim3(cdiv(g.N, 16), cdiv(g.M, 64), 1), dim3(512), 0, st, g);
    else {
#define GEMM16_LAUNCH(RBv, CBv, Uv, WTv)                                                                                                         \
    hipLaunchKernelGGL((gemm16_kernel<RBv, CBv, Uv, WTv>), dim3(cdiv(g.N, 16 * CBv), cdiv(g.M, 16 * RBv), g.kz), dim3(64 * GEMM_WAVES), 0, st, g.x, \
                       g.w, g.ldx, g.K, g.N, g.M, g.ks, g.kz, g)
        if (form == GEMM_FORM_TILE2) { if (g.wt) GEMM16_LAUNCH(2, 2, 1, true); else GEMM16_LAUNCH(2, 2, 1, false); }
        else { if (g.wt) GEMM16_LAUNCH(1, 1, GEMM_U, true); else GEMM16_LAUNCH(1, 1, GEMM_U, false); }
#undef GEMM16_LAUNCH
    }
    CCVS_CHECK_LAUNCH(name);
    return CCVS_OK;
}

// Workspace layout: [GEMM_WS_TILES x kz<=GEMM_KZ_MAX x 256 floats of split-K slabs][GEMM_WS_TILES arrival counters][StepBar: the grid barrier of
// the persistent decode step, below] -- zeroed once by the caller, left consistent by every launch.
#define GEMM_WS_SLAB_BYTES ((size_t)GEMM_WS_TILES * GEMM_KZ_MAX * 256 * sizeof(float))
#define GEMM_WS_BAR_OFFSET (GEMM_WS_SLAB_BYTES + (size_t)GEMM_WS_TILES * sizeof(int))   // 4 MB + 4 KB: 128-byte aligned
#define GEMM_WS_BAR_BYTES 2048
extern "C" int64_t ccvs_gemm_workspace_bytes(void) { return (int64_t)(GEMM_WS_BAR_OFFSET + GEMM_WS_BAR_BYTES); }

extern "C" int ccvs_gemm_nt(const float* x, int64_t ldx, const float* w, const float* bias, const float* res, float* y, int64_t ldy,
                            int32_t M, int32_t N, int32_t K, int32_t epilogue, void* workspace, void* stream) {
    Gemm16 g = {};
    g.x = x; g.ldx = ldx; g.w = w; g.bias = bias; g.res = res; g.y = y; g.ldy = ldy; g.M = M; g.N = N; g.K = K;
    g.epi = epilogue & 0xff; g.seq = (epilogue & CCVS_GEMM_SEQ) ? 1 : 0;
    if (workspace) {
        g.ws_slabs = (float*)workspace;
        g.ws_count = (int*)((char*)workspace + GEMM_WS_SLAB_BYTES);
    }
    return launch_gemm16(g, (hipStream_t)stream, "ccvs_gemm_nt");
}

extern "C" int ccvs_gemm_ln(const float* x, int64_t ldx, const float* w_gamma, const float* bias_beta, const float* w_rowsum, float eps,
                            float* y, int64_t ldy, int32_t M, int32_t N, int32_t K, int32_t epilogue, void* stream) {
    CCVS_REQUIRE(w_rowsum, "ccvs_gemm_ln: null pointer");
    CCVS_REQUIRE((epilogue & 0xff) == 0 || (epilogue & 0xff) == 1, "ccvs_gemm_ln: bad epilogue");
    Gemm16 g = {};
    g.x = x; g.ldx = ldx; g.w = w_gamma; g.bias = bias_beta; g.y = y; g.ldy = ldy; g.M = M; g.N = N; g.K = K;
    g.epi = epilogue & 0xff; g.seq = (epilogue & CCVS_GEMM_SEQ) ? 1 : 0;
    g.ln_s = w_rowsum; g.ln_eps = eps;
    return launch_gemm16(g, (hipStream_t)stream, "ccvs_gemm_ln");
}

extern "C" int ccvs_gemm_ln_qkv(const float* x, int64_t ldx, const float* w_gamma, const float* bias_beta, const float* w_rowsum, float eps,
                                float* q, float* kcache, float* vcache, int32_t B, int32_t Tq, int32_t C, int32_t H, int32_t pos0,
                                const int32_t* pos_dev, int32_t Tmax, void* stream) {
    CCVS_REQUIRE(w_rowsum && kcache && vcache, "ccvs_gemm_ln_qkv: null pointer");
    CCVS_REQUIRE(B > 0 && Tq > 0 && H > 0 && C % H == 0 && pos0 >= 0 && pos0 + Tq <= Tmax, "ccvs_gemm_ln_qkv: bad shape / positions");
    Gemm16 g = {};
    g.x = x; g.ldx = ldx; g.w = w_gamma; g.bias = bias_beta; g.y = q; g.ldy = C; g.M = B * Tq; g.N = 3 * C; g.K = C; g.epi = 0;
    g.ln_s = w_rowsum; g.ln_eps = eps;
    g.kcache = kcache; g.vcache = vcache; g.C = C; g.H = H; g.D = C / H; g.Tq = Tq; g.Tmax = Tmax; g.pos0 = pos0; g.pos_dev = pos_dev;
    g.seq = Tq > 1 ? 1 : 0;
    return launch_gemm16(g, (hipStream_t)stream, "ccvs_gemm_ln_qkv");
}

// the most rows the forms that read tiled weights take: a step of more rows runs the row-blocked form, which reads row-major weights only
extern "C" int32_t ccvs_gemm_tiled_max_rows(void) { return GEMM_DECODE_MAX_M; }

// One decode GEMM (single position, M <= GEMM_DECODE_MAX_M) against TILED weights: the three calls above in one signature, as the
// decode step issues them (w_rowsum: the folded LayerNorm; kcache / vcache: the QKV scatter with Tq = 1, N = 3 K, y = q).
extern "C" int ccvs_gemm_tiled(const float* x, int64_t ldx, const float* w_tiled, const float* bias, const float* res, const float* w_rowsum,
                               float eps, float* y, int64_t ldy, int32_t M, int32_t N, int32_t K, int32_t epilogue, float* kcache, float* vcache,
                               int32_t H, int32_t pos0, const int32_t* pos_dev, int32_t Tmax, void* workspace, void* stream) {
    CCVS_REQUIRE((epilogue & ~0xff) == 0 && M <= GEMM_DECODE_MAX_M, "ccvs_gemm_tiled: a single-position call of at most %d rows", GEMM_DECODE_MAX_M);
    CCVS_REQUIRE(!w_rowsum || epilogue == 0 || epilogue == 1, "ccvs_gemm_tiled: bad epilogue");
    CCVS_REQUIRE((kcache != nullptr) == (vcache != nullptr), "ccvs_gemm_tiled: one cache without the other");
    Gemm16 g = {};
    g.x = x; g.ldx = ldx; g.w = w_tiled; g.bias = bias; g.res = res; g.y = y; g.ldy = ldy; g.M = M; g.N = N; g.K = K; g.epi = epilogue; g.wt = 1;
    g.ln_s = w_rowsum; g.ln_eps = eps;
    if (kcache) {
        CCVS_REQUIRE(w_rowsum && epilogue == 0 && N == 3 * K && ldy == K && H > 0 && K % H == 0 && pos0 >= 0 && pos0 < Tmax, "ccvs_gemm_tiled: bad QKV shape / position");
        g.kcache = kcache; g.vcache = vcache; g.C = K; g.H = H; g.D = K / H; g.Tq = 1; g.Tmax = Tmax; g.pos0 = pos0; g.pos_dev = pos_dev;
    }
    if (workspace) {
        g.ws_slabs = (float*)workspace;
        g.ws_count = (int*)((char*)workspace + GEMM_WS_SLAB_BYTES);
    }
    return launch_gemm16(g, (hipStream_t)stream, "ccvs_gemm_tiled");
}

// ---------------------------------------------------------------------------------------
// get_icode: temperature, top-k mask (ties with the k-th value kept), softmax, then
// argmax(p) (greedy) or argmax(p / Exp(1) noise) (== torch.multinomial(p, 1)).
// One workgroup per row; the k-th largest value is found by a 32-step radix descent on
// order-preserving integer keys.
// ZEROS: -0.0 and +0.0 share one key, as they compare equal in the reference's `out < v[-1]` mask: a k-th value of +0.0 keeps
// every -0.0 logit and the other way round.
// NON-FINITE ROWS: a NaN or +inf logit, or a row of -inf throughout, makes the row's total -- and with it every score -- NaN, so
// no score compares greater than any other.  Such a row returns token 0 (vq_argmin_kernel's rule, and torch.argmax's on an all-NaN
// row); sample_topn returns 0, 1, ..., n - 1: in any round without a winner, the lowest index not yet taken.  A stored index is
// always inside [0, V).
// PHILOX COUNTER: (c0, c1, c2, c3) = (element j, row0 + row inside its group, step, call), key (key0, key1), output word 0;
// step = 0xffffffff for the eager first pick of a call, then state[0] = 0, 1, ... in the decode steps.
// NUCLEUS (the TOPP form only; include/ccvs_hip_sampling.h has the definition): on the top-k set, e_j = expf(xs_j - max) as the pick
// itself computes it, m_j = (uint64) floor(e_j * 2^46) -- the scaling is exact, the conversion truncates: e >= 2^-22 converts exactly,
// a smaller one loses less than 2^-46, and V < 2^16 entries of at most 2^46 cannot overflow.  T = sum m and every bin mass of the
// radix descent are sums of these INTEGERS (64-bit LDS adds, wave shuffles): the same bits in any order, so the kept set does not
// depend on the run, the launch form or the batch slot.  Entry j is kept iff G_j < P, G_j = sum of m_i over the top-k entries with
// xs_i > xs_j (by key: ties share one fate, -0.0 == +0.0) and P = (uint64) ceil((double) top_p * (double) T), the ONE floating-point
// product of the decision (for an integer G, G < P is G < top_p * T).  G is not increasing along the descending order, so the kept set
// is {key >= c}, c = the largest key whose mass at or above it reaches P: found as kth_largest_key finds its key, with per-bin mass
// in place of per-bin counts and expf recomputed in each pass from xs, which stays in LDS until c is known.  The most likely token
// has G = 0 < P and is always kept.  The scores then are the top-k form's own bits -- e_j / (the fp32 total of the top-k set) / noise --
// on the smaller set: the total is a common factor.  A non-finite row (its fp32 total is NaN) skips the descent and ends as above.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned fkey(float f) {
    unsigned u = __float_as_uint(f);
    if (u == 0x80000000u) u = 0u;   // -0.0 == +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Philox4x32-10 (Salmon et al., SC'11): counter-based, so every (row, element, step) gets its own draw
// with no generator state to advance between hipGraph replays.
__device__ __forceinline__ unsigned philox_first(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

struct Advance {       // decode-step bookkeeping folded into the sampling kernel (all null outside ccvs_gpt_decode_step)
    int64_t* codes;    // [B][codes_sB] generated sequence: codes[b][*widx] = picked token
    long codes_sB;
    int32_t* widx;     // device-resident write index, +1 per step
    int32_t* len;      // device-resident cache length, +1 per step
    int rng;           // draw the Exp(1) noise here: Philox keyed by state[4..5], counter (element, state[6] + row, step = state[0], call = state[3])
    unsigned imm[5];   // rng == 2: immediate Philox words (key0, key1, global row of row 0, step, call) instead of `state`
    int* state;        // int32[8]: [0] completed steps, [2] arrival ticket of this kernel's rows, [3] call index, [4..5] Philox key, [6] global index of row 0
    int grp_rows;      // > 0: rows [g * grp_rows, (g+1) * grp_rows) form group g with its own widx[g], len[g] and state[8g .. 8g+7]
    const float* const* noise_stream;   // host-drawn noise as a whole stream: entry g -> [steps][rows of group g][V]; the block read is state[0] of the group
};

// k-th largest key of xs[0..V) by a 4-pass radix-256 descent (LDS histogram + suffix scan per pass).
__device__ __forceinline__ unsigned kth_largest_key(const float* xs, int V, int top_k, int* hist, int* wtot, int* sel, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    unsigned prefix = 0u, mask = 0u;
    int need = top_k;
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        for (int j = tid; j < V; j += 256) {
            const unsigned key = fkey(xs[j]);
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
        }
        __syncthreads();
        const int h = hist[tid];
        int s = h;  // suffix sum over bins >= tid
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_down(s, o, 64);
            if (lane + o < 64) s += t;
        }
        if (lane == 0) wtot[wave] = s;
        __syncthreads();
        for (int w = wave + 1; w < 4; ++w) s += wtot[w];
        if (s >= need && s - h < need) { sel[0] = tid; sel[1] = need - (s - h); }
        __syncthreads();
        prefix |= (unsigned)sel[0] << shift;
        mask |= 255u << shift;
        need = sel[1];
    }
    return prefix;
}

// The nucleus' integer mass of one entry (NUCLEUS above): floor(e * 2^46); 0 for a NaN.
#define TOPP_MASS_SCALE 70368744177664.0f   // 2^46
__device__ __forceinline__ unsigned long long topp_mass(float e) {
    return e == e ? (unsigned long long)(e * TOPP_MASS_SCALE) : 0ull;
}

// The nucleus' boundary key: the largest key c such that the entries of the top-k set (key >= thr) with key >= c hold a mass of at least
// `need` (1 <= need <= their total mass).  kth_largest_key's 4-pass radix-256 descent with per-bin mass in place of per-bin counts.
__device__ __forceinline__ unsigned topp_boundary_key(const float* xs, int V, unsigned thr, float gmax, unsigned long long need,
                                                      unsigned long long* mass, unsigned long long* wtot, unsigned long long* sel, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    unsigned prefix = 0u, mask = 0u;
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
        mass[tid] = 0ull;
        __syncthreads();
        for (int j = tid; j < V; j += 256) {
            const unsigned key = fkey(xs[j]);
            if (key >= thr && (key & mask) == prefix) atomicAdd(&mass[(key >> shift) & 255u], topp_mass(expf(xs[j] - gmax)));
        }
        __syncthreads();
        const unsigned long long h = mass[tid];
        unsigned long long s = h;  // suffix sum over bins >= tid
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long t = __shfl_down(s, o, 64);
            if (lane + o < 64) s += t;
        }
        if (lane == 0) wtot[wave] = s;
        __syncthreads();
        for (int w = wave + 1; w < 4; ++w) s += wtot[w];
        if (s >= need && s - h < need) { sel[0] = (unsigned long long)tid; sel[1] = need - (s - h); }
        __syncthreads();
        prefix |= (unsigned)sel[0] << shift;
        mask |= 255u << shift;
        need = sel[1];
    }
    return prefix;
}

// (b = the row, B_all = the rows of the launch; smem = PICK_SMEM_WORDS(V) floats.  COH: the logits were written by the head GEMM phase
//  of the same launch -- sc1 loads.  TOPP: the nucleus form -- smem = PICK_TOPP_SMEM_WORDS(V) floats, 0 < top_p < 1; without it top_p
//  is not read and the body is the one this function had before it took the parameter.)
template <bool COH, bool TOPP = false>
__device__ __forceinline__ void sample_topk_row(const float* __restrict__ logits, long ld, const float* __restrict__ noise,
                                                int64_t* __restrict__ out, long out_stride, int V, int top_k, float temperature,
                                                Advance adv, int b, int B_all, float* smem, float top_p = 0.f) {
    float* xs = smem;                  // [V]
    float* redf = smem + V;            // [4]
    int* redj = (int*)(smem + V + 4);  // [4]
    int* wtot = (int*)(smem + V + 8);  // [4]
    int* sel = (int*)(smem + V + 12);  // [2]
    int* hist = (int*)(smem + V + 16); // [256]
    const int tid = thread_id<COH>(), lane = tid & 63, wave = tid >> 6;
    // row group of this row: its own counters / Philox words; `brow` = the row's index inside the group
    const int grp = adv.grp_rows > 0 ? b / adv.grp_rows : 0;
    const int brow = b - grp * (adv.grp_rows > 0 ? adv.grp_rows : 0);
    const int nrows = adv.grp_rows > 0 ? min(adv.grp_rows, B_all - grp * adv.grp_rows) : B_all;
    if (adv.grp_rows > 0) { adv.state += 8 * grp; adv.widx += grp; adv.len += grp; }
    const float* lr = logits + (long)b * ld;
    float lmax = -INFINITY;
    for (int j = tid; j < V; j += 256) {
        const float v = ld_act<COH>(lr + j) / temperature;
        xs[j] = v;
        lmax = fmaxf(lmax, v);
    }
    lmax = wave_max(lmax);
    if (lane == 0) redf[wave] = lmax;
    __syncthreads();
    const float gmax = fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));

    unsigned thr = 0u;  // key of the k-th largest value; 0 keeps everything
    if (top_k > 0 && top_k < V) thr = kth_largest_key(xs, V, top_k, hist, wtot, sel, tid);
    float lsum = 0.f;
    unsigned long long msum = 0ull;   // TOPP: this thread's share of the integer total T
    for (int j = tid; j < V; j += 256) {
        const float e = (fkey(xs[j]) >= thr) ? expf(xs[j] - gmax) : 0.f;
        if constexpr (TOPP) msum += topp_mass(e);   // xs stays: the descent below needs the order of entries whose e round equal
        else xs[j] = e;
        lsum += e;
    }
    lsum = wave_sum(lsum);
    __syncthreads();
    if (lane == 0) redf[wave] = lsum;
    __syncthreads();
    const float tot = ((redf[0] + redf[1]) + redf[2]) + redf[3];
    if constexpr (TOPP) {
        // the 64-bit words lie behind the top-k form's block, on an 8-byte boundary: mass bins [256], wave totals [4], the selected bin [2]
        unsigned long long* mass = (unsigned long long*)(smem + ((V + 16 + 256 + 1) & ~1));
        unsigned long long* wtot64 = mass + 256;
        unsigned long long* sel64 = mass + 260;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) msum += __shfl_xor(msum, o, 64);
        if (lane == 0) wtot64[wave] = msum;
        __syncthreads();
        const unsigned long long T = wtot64[0] + wtot64[1] + wtot64[2] + wtot64[3];
        __syncthreads();   // (the descent writes wtot64 again)
        if (tot == tot) {  // a finite row: T >= 2^46 (the maximum's own mass), 1 <= P <= T
            const unsigned long long P = (unsigned long long)ceil((double)top_p * (double)T);
            thr = topp_boundary_key(xs, V, thr, gmax, P, mass, wtot64, sel64, tid);
        }
    }
    // counter = (element, GLOBAL row = state[6] of the row's group + its index inside the group (mod 2^32), step, call = state[3]):
    // a clip's draws do not depend on which rank / batch slot it runs in, nor on how many other clips share the launch
    // (tests/pick_ref.py mirrors the draw on the host; tests/test_pick_gpu.py compares every pick with it)
    unsigned k0 = 0u, k1 = 0u, step = 0u, row0 = 0u, call = 0u;
    if (adv.rng == 2) {
        k0 = adv.imm[0]; k1 = adv.imm[1]; row0 = adv.imm[2]; step = adv.imm[3]; call = adv.imm[4];
    } else if (adv.rng) {
        k0 = (unsigned)adv.state[4]; k1 = (unsigned)adv.state[5]; step = (unsigned)adv.state[0];
        call = (unsigned)adv.state[3]; row0 = (unsigned)adv.state[6];
    }
    // host-drawn noise: the [B, V] block of an eager pick, or this row's slice of block `state[0]` (the steps its group has
    // completed) of the group's pre-drawn stream -- the captured step then consumes the reference's generator stream in order
    const float* nrow = noise ? noise + (long)b * V : nullptr;
    if (adv.noise_stream) nrow = adv.noise_stream[grp] + ((long)adv.state[0] * nrows + brow) * V;
    float best = -1.f;
    int bi = 0x7fffffff;
    for (int j = tid; j < V; j += 256) {
        float p;
        if constexpr (TOPP) p = ((fkey(xs[j]) >= thr) ? expf(xs[j] - gmax) : 0.f) / tot;   // the e of the total's pass, on the nucleus
        else p = xs[j] / tot;
        if (nrow) p = p / nrow[j];
        else if (adv.rng) {
            const float u = ((float)philox_first((unsigned)j, row0 + (unsigned)brow, step, call, k0, k1) + 0.5f) * 2.3283064365386963e-10f;  // (0, 1]
            p = p / fmaxf(-logf(u), 1e-30f);
        }
        if (p > best) { best = p; bi = j; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    __syncthreads();
    if (lane == 0) { redf[wave] = best; redj[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w)
            if (redf[w] > best || (redf[w] == best && redj[w] < bi)) { best = redf[w]; bi = redj[w]; }
        if (bi >= V) bi = 0;   // no score compared greater than any other (NaN throughout): token 0, never an index outside [0, V)
        out[(long)b * out_stride] = bi;
        if (adv.codes) {
            adv.codes[(long)b * adv.codes_sB + *adv.widx] = bi;
            // the last row to finish advances the device-resident counters (every row has read them by then)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            const int ticket = __hip_atomic_fetch_add(adv.state + 2, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (ticket == nrows - 1) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                *adv.widx += 1;
                *adv.len += 1;
                adv.state[0] += 1;
                __hip_atomic_store(adv.state + 2, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

__global__ __launch_bounds__(256) void sample_topk_kernel(const float* __restrict__ logits, long ld, const float* __restrict__ noise,
                                                          int64_t* __restrict__ out, long out_stride, int V, int top_k, float temperature,
                                                          Advance adv) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    sample_topk_row<false>(logits, ld, noise, out, out_stride, V, top_k, temperature, adv, blockIdx.x, gridDim.x, smem);
}

#define PICK_SMEM_WORDS(V) ((V) + 16 + 256)
// the pick keeps a row's logits in dynamic LDS: up to 160 KB, allowed once per process
static void pick_allow_big_lds() {
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)sample_topk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_set = true;
    }
}

extern "C" int ccvs_sample_topk(const float* logits, int64_t ld, const float* noise, int64_t* out, int64_t out_stride, int32_t B, int32_t V,
                                int32_t top_k, float temperature, void* stream) {
    CCVS_REQUIRE(logits && out, "ccvs_sample_topk: null pointer");
    CCVS_REQUIRE(B > 0 && V > 0 && temperature > 0.f, "ccvs_sample_topk: bad arguments");
    const size_t smem = (size_t)PICK_SMEM_WORDS(V) * sizeof(float);
    pick_allow_big_lds();
    CCVS_REQUIRE(smem <= 160 * 1024, "ccvs_sample_topk: vocabulary %d too large", V);
    hipLaunchKernelGGL(sample_topk_kernel, dim3(B), dim3(256), smem, (hipStream_t)stream, logits, (long)ld, noise, out, (long)out_stride, V,
                       top_k, temperature, Advance{});
    CCVS_CHECK_LAUNCH("ccvs_sample_topk");
    return CCVS_OK;
}

extern "C" int ccvs_sample_topk_philox(const float* logits, int64_t ld, int64_t* out, int64_t out_stride, int32_t B, int32_t V, int32_t top_k,
                                       float temperature, uint32_t key0, uint32_t key1, uint32_t row0, uint32_t step, uint32_t call,
                                       void* stream) {
    CCVS_REQUIRE(logits && out, "ccvs_sample_topk_philox: null pointer");
    CCVS_REQUIRE(B > 0 && V > 0 && temperature > 0.f, "ccvs_sample_topk_philox: bad arguments");
    const size_t smem = (size_t)PICK_SMEM_WORDS(V) * sizeof(float);
    pick_allow_big_lds();
    CCVS_REQUIRE(smem <= 160 * 1024, "ccvs_sample_topk_philox: vocabulary %d too large", V);
    Advance adv = {};
    adv.rng = 2;
    adv.imm[0] = key0; adv.imm[1] = key1; adv.imm[2] = row0; adv.imm[3] = step; adv.imm[4] = call;
    hipLaunchKernelGGL(sample_topk_kernel, dim3(B), dim3(256), smem, (hipStream_t)stream, logits, (long)ld, (const float*)nullptr, out,
                       (long)out_stride, V, top_k, temperature, adv);
    CCVS_CHECK_LAUNCH("ccvs_sample_topk_philox");
    return CCVS_OK;
}

// The nucleus form of the pick (include/ccvs_hip_sampling.h): the same row body with TOPP, in a kernel of its own -- sample_topk_kernel
// and what reaches it stay as they are.  Its LDS: the top-k form's block, then (on an 8-byte boundary) 262 64-bit words.
__global__ __launch_bounds__(256) void sample_topp_kernel(const float* __restrict__ logits, long ld, const float* __restrict__ noise,
                                                          int64_t* __restrict__ out, long out_stride, int V, int top_k, float temperature,
                                                          float top_p, Advance adv) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    sample_topk_row<false, true>(logits, ld, noise, out, out_stride, V, top_k, temperature, adv, blockIdx.x, gridDim.x, smem, top_p);
}

#define PICK_TOPP_SMEM_WORDS(V) ((((V) + 16 + 256 + 1) & ~1) + 2 * 262)
static void pick_topp_allow_big_lds() {
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)sample_topp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_set = true;
    }
}

// the largest vocabulary whose PICK_TOPP_SMEM_WORDS fit the 160 KB of dynamic LDS
extern "C" int32_t ccvs_sample_topp_max_vocab(void) {
    int32_t v = 160 * 1024 / 4 - (16 + 256 + 1 + 2 * 262);
    while ((size_t)PICK_TOPP_SMEM_WORDS(v + 1) * sizeof(float) <= 160 * 1024) ++v;
    return v;
}

// 0 < top_p < 1: the nucleus is on.  1: off (the callers below then run the top-k form).  Anything else, NaN included, is refused.
static bool topp_on(float top_p) { return top_p > 0.f && top_p < 1.f; }

static int launch_sample_topp(const char* who, const float* logits, int64_t ld, const float* noise, int64_t* out, int64_t out_stride,
                              int32_t B, int32_t V, int32_t top_k, float temperature, float top_p, const Advance& adv, hipStream_t st) {
    CCVS_REQUIRE(logits && out, "%s: null pointer", who);
    CCVS_REQUIRE(B > 0 && V > 0 && temperature > 0.f, "%s: bad arguments", who);
    CCVS_REQUIRE(topp_on(top_p) || top_p == 1.f, "%s: top_p %g is neither inside (0, 1) nor 1 (off)", who, (double)top_p);
    if (!topp_on(top_p)) {   // off: the top-k form, its own cap
        const size_t smem = (size_t)PICK_SMEM_WORDS(V) * sizeof(float);
        CCVS_REQUIRE(smem <= 160 * 1024, "%s: vocabulary %d too large", who, V);
        pick_allow_big_lds();
        hipLaunchKernelGGL(sample_topk_kernel, dim3(B), dim3(256), smem, st, logits, (long)ld, noise, out, (long)out_stride, V, top_k, temperature, adv);
    } else {
        const size_t smem = (size_t)PICK_TOPP_SMEM_WORDS(V) * sizeof(float);
        CCVS_REQUIRE(smem <= 160 * 1024, "%s: vocabulary %d too large for the top_p form (at most %d)", who, V, ccvs_sample_topp_max_vocab());
        pick_topp_allow_big_lds();
        hipLaunchKernelGGL(sample_topp_kernel, dim3(B), dim3(256), smem, st, logits, (long)ld, noise, out, (long)out_stride, V, top_k, temperature,
                           top_p, adv);
    }
    CCVS_CHECK_LAUNCH(who);
    return CCVS_OK;
}

extern "C" int ccvs_sample_topp(const float* logits, int64_t ld, const float* noise, int64_t* out, int64_t out_stride, int32_t B, int32_t V,
                                int32_t top_k, float temperature, float top_p, void* stream) {
    return launch_sample_topp("ccvs_sample_topp", logits, ld, noise, out, out_stride, B, V, top_k, temperature, top_p, Advance{}, (hipStream_t)stream);
}

extern "C" int ccvs_sample_topp_philox(const float* logits, int64_t ld, int64_t* out, int64_t out_stride, int32_t B, int32_t V, int32_t top_k,
                                       float temperature, float top_p, uint32_t key0, uint32_t key1, uint32_t row0, uint32_t step, uint32_t call,
                                       void* stream) {
    Advance adv = {};
    adv.rng = 2;
    adv.imm[0] = key0; adv.imm[1] = key1; adv.imm[2] = row0; adv.imm[3] = step; adv.imm[4] = call;
    return launch_sample_topp("ccvs_sample_topp_philox", logits, ld, nullptr, out, out_stride, B, V, top_k, temperature, top_p, adv, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------
// get_icode with n picks per row (the proposals of beam search, transformer_model.py:358-391,395-409): temperature, top-k
// mask, softmax, then the n best of p (sample = False: torch.topk) or of p / Exp(1) noise (sample = True: what
// torch.multinomial(p, n) without replacement computes), best first, ties to the lowest index; also log p of every pick.
// One workgroup per row: probabilities and scores in LDS, n rounds of a block-wide argmax.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sample_topn_kernel(const float* __restrict__ logits, long ld, const float* __restrict__ noise,
                                                          int64_t* __restrict__ out_idx, float* __restrict__ out_logp, int V, int top_k,
                                                          float temperature, int n) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* xs = smem;                       // [V] scaled logits, then probabilities
    float* sc = smem + V;                   // [V] scores the picks are taken from
    float* redf = smem + 2 * V;             // [4]
    int* redj = (int*)(smem + 2 * V + 4);   // [4]
    int* wtot = (int*)(smem + 2 * V + 8);   // [4]
    int* sel = (int*)(smem + 2 * V + 12);   // [2]
    int* hist = (int*)(smem + 2 * V + 16);  // [256]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const float* lr = logits + (long)b * ld;
    float lmax = -INFINITY;
    for (int j = tid; j < V; j += 256) {
        const float v = lr[j] / temperature;
        xs[j] = v;
        lmax = fmaxf(lmax, v);
    }
    lmax = wave_max(lmax);
    if (lane == 0) redf[wave] = lmax;
    __syncthreads();
    const float gmax = fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));
    unsigned thr = 0u;
    if (top_k > 0 && top_k < V) thr = kth_largest_key(xs, V, top_k, hist, wtot, sel, tid);
    float lsum = 0.f;
    for (int j = tid; j < V; j += 256) {
        const float e = (fkey(xs[j]) >= thr) ? expf(xs[j] - gmax) : 0.f;
        xs[j] = e;
        lsum += e;
    }
    lsum = wave_sum(lsum);
    __syncthreads();
    if (lane == 0) redf[wave] = lsum;
    __syncthreads();
    const float tot = ((redf[0] + redf[1]) + redf[2]) + redf[3];
    for (int j = tid; j < V; j += 256) {
        const float p = xs[j] / tot;
        xs[j] = p;
        sc[j] = noise ? p / noise[(long)b * V + j] : p;
    }
    __syncthreads();
    int free_lo = 0;   // (thread 0) no index below it is free: taken indices stay taken, so it only moves up
    // log p = (x_i - max) - log(sum e), in double: the difference of two fp32 values is exact there, so a pick's log p carries
    // the roundings of the sum and one rounding to fp32, not those of its own expf, division and a logf of a result far below -1
    // (half an ulp of a log p in [-16, -8) is 2^-21; logf(p) was off by up to four times that on the least probable entries).
    const double ltot = tid == 0 ? log((double)tot) : 0.0;
    for (int r = 0; r < n; ++r) {
        float best = -1.f;
        int bi = 0x7fffffff;
        for (int j = tid; j < V; j += 256) {
            const float v = sc[j];
            if (v > best) { best = v; bi = j; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if (lane == 0) { redf[wave] = best; redj[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 4; ++w)
                if (redf[w] > best || (redf[w] == best && redj[w] < bi)) { best = redf[w]; bi = redj[w]; }
            if (bi >= V) {   // no winner (the scores left are NaN): the lowest index not yet taken
                while (free_lo < V - 1 && sc[free_lo] == -2.f) ++free_lo;   // (fewer than n <= V are taken: one is free)
                bi = free_lo;
            }
            out_idx[(long)b * n + r] = bi;
            const float p = xs[bi];   // 0 (masked or underflowed: log p = -inf) and NaN rows keep logf's answer
            out_logp[(long)b * n + r] = p > 0.f ? (float)(((double)(lr[bi] / temperature) - (double)gmax) - ltot) : logf(p);
            sc[bi] = -2.f;   // taken
        }
        __syncthreads();
    }
}

extern "C" int ccvs_sample_topn(const float* logits, int64_t ld, const float* noise, int64_t* out_idx, float* out_logp, int32_t B, int32_t V,
                                int32_t top_k, float temperature, int32_t n, void* stream) {
    CCVS_REQUIRE(logits && out_idx && out_logp, "ccvs_sample_topn: null pointer");
    CCVS_REQUIRE(B > 0 && V > 0 && temperature > 0.f && n >= 1 && n <= V, "ccvs_sample_topn: bad arguments");
    const size_t smem = (size_t)(2 * V + 16 + 256) * sizeof(float);
    CCVS_REQUIRE(smem <= 160 * 1024, "ccvs_sample_topn: vocabulary %d too large", V);
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)sample_topn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_set = true;
    }
    hipLaunchKernelGGL(sample_topn_kernel, dim3(B), dim3(256), smem, (hipStream_t)stream, logits, (long)ld, noise, out_idx, out_logp, V, top_k,
                       temperature, n);
    CCVS_CHECK_LAUNCH("ccvs_sample_topn");
    return CCVS_OK;
}

// ---------------------------------------------------------------------------------------
// The decode step as ONE launch (ccvs_gpt_decode.persistent): 256-thread workgroups that stay resident for
// the whole step -- one per CU -- and walk its phases themselves,
//     embed | per layer: ln1+QKV+cache scatter | attention | proj+res | ln2+fc+GELU | fc2+res | ln_f+head | pick,
// instead of 5 n_layer + 3 dependent launches.  A phase is the launch it replaces, tile for tile: workgroup w takes the tiles
// w, w + G, ... of the phase's grid and runs the SAME tile body (gemm16_tile / attention_decode_item / sample_topk_row), so a row's
// arithmetic -- K slices per wave, MFMA order, slab order, reduction order -- is the launch chain's instruction for instruction and
// the tokens are bit-identical (tests/test_persistent_step_gpu.py).  What changes is how a phase's output reaches the next phase's
// readers on OTHER CUs (MI355X_MICROARCH.md, "Workgroup dispatch, XCD placement & inter-workgroup visibility": per-XCD L2s are not
// coherent, a CU's L1 is never refreshed by another CU's stores):
//   * every buffer handed over inside the launch -- x, q, the cache row of the current position, att, h, logits, the split-K slabs --
//     is written with sc1 (write-through) stores and read with sc1 loads (L1 bypassed): COH = true in the tile bodies; weights, the
//     older cache rows, the embedding tables and the device-resident counters were written by EARLIER launches and stay plain;
//   * the grid barrier between two phases: every wave drains its stores (s_waitcnt vmcnt(0)), the workgroup meets (s_barrier), ONE
//     lane adds 1 to the workgroup's shard of a monotonic arrival counter (8 shards on lines of their own: 32 agent-scope adds per
//     word instead of 256), wave 0 polls the 8 shards with sc1 loads + s_sleep until their sum reaches base + phases passed x G,
//     the workgroup meets again and goes on -- no fence instruction anywhere (the "Valid forms" table, first row: one lane of each
//     storing workgroup signals for all of that workgroup's stores after every storing wave's vmcnt(0) and the workgroup's barrier;
//     the poller loads after its poll has matched, the other waves after a barrier it then joins; sc1 stores of 4 / 16 bytes, sc1
//     loads of 4 / 16 bytes).  `base` = the arrivals counted before this launch, kept in a word of its own that workgroup 0 moves
//     forward once per launch (read by the NEXT launch only: a kernel boundary apart), so nothing is zeroed between launches and a
//     captured step replays unchanged; comparisons are on the wrapped difference.  A poll that sees nothing for 5 s gives up, sets
//     StepBar.err and lets the workgroup run on; the word is sticky -- every later barrier of this workspace gives up at once, so a lost
//     workgroup costs ONE time-out, not one per phase -- the tokens since are garbage, and ccvs_gpt_decode_status reports it and
//     starts the barrier block over.
// Residency: G = the number of CUs; a workgroup (256 threads, 64 registers, <= 18 KB of LDS at BAIR size) fits beside the 3 x 3
// convolution workgroups of the frame decoder (two waves of 208 / 214 registers per SIMD) but not beside the 1 x 1 forms' 225, and it
// HOLDS its slot for the whole step: two token chains' persistent steps cannot both be resident beside the decoder on one CU, and
// partially resident grids that wait for each other's slots stall until convolution workgroups retire -- a schedule with ONE token
// chain is what this form is for.  MEASURED (profiles/r06_persistent_step.txt): bit-identical and 1.4-1.9 x slower than the launch
// chain, alone and in the run -- ~7 us per grid barrier against 1.5-2 per kernel boundary, and one workgroup per CU where the chain
// oversubscribes the chip (the attention phases run at ~2 TB/s instead of 5.7).  An opt-in, not the default.
// ---------------------------------------------------------------------------------------
#define STEP_SPIN_TICKS 500000000ULL   // 5 s of the 100 MHz s_memrealtime counter
struct StepBar {
    unsigned shard[8][32];   // arrivals, monotonic; one 128-byte line per shard
    unsigned base[32];       // arrivals counted when the current launch started
    unsigned err[32];        // != 0: a barrier of some launch gave up (phase index + 1)
};
static_assert(sizeof(StepBar) <= GEMM_WS_BAR_BYTES, "StepBar outgrew its slot in the workspace");

// One phase of the step, built once per descriptor by the host (ccvs_gpt_decode_prepare) into a caller-provided device buffer: the
// kernel reads phase ph's operands by scalar loads when it gets there.  (Operands selected inside the kernel from a by-value argument
// block -- 24 layers x 12 pointers -- are loop-invariant to the compiler: it kept them ALL live across the phase loop, ran out of
// scalar registers (106) and parked uniform values in vector registers: 96 + 16 registers per lane instead of the tile bodies' 48.)
#define STEP_GEMM 0
#define STEP_ATTENTION 1
struct StepPhase {
    int kind, pad_;
    Gemm16 g;   // STEP_GEMM: the launch this phase replaces; STEP_ATTENTION: x = q, y = att, kcache / vcache, H, Tmax, M = rows
};

struct StepArgs {
    int B, C, V, vocab, grp_rows, pos_off, n_phases, H;
    const float *tok_emb, *pos_table;
    const int64_t* tok;
    const int32_t* len;
    float *x, *logits;
    StepBar* bar;
    const StepPhase* prog;
    float scale;
    const float* noise;
    int top_k;
    float temperature;
    Advance adv;
    float top_p;   // read by the TOPP form of the step only
};

__device__ __forceinline__ void step_barrier(StepBar* bar, unsigned target, int phase) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // EVERY wave: its sc1 stores of this phase have left
    __syncthreads();
    if (threadIdx.x < 64) {
        if (threadIdx.x == 0) __hip_atomic_fetch_add(&bar->shard[blockIdx.x & 7][0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned* sp = &bar->shard[thread_id<true>() & 7][0];   // (opaque: otherwise built once in front of the phase loop and held in a register pair across every phase)
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        for (unsigned spins = 1;; ++spins) {
            unsigned v = __hip_atomic_load(sp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            v += __shfl_xor(v, 1, 64);
            v += __shfl_xor(v, 2, 64);
            v += __shfl_xor(v, 4, 64);
            if ((int)(v - target) >= 0) break;
            __builtin_amdgcn_s_sleep(2);
            if ((spins & 255u) == 0) {
                // give up: after 5 s without the others, or AT ONCE when any workgroup of this workspace has given up before (the word is
                // sticky until ccvs_gpt_decode_status clears the whole barrier block) -- a lost workgroup costs one time-out, not one per phase
                const bool late = __builtin_amdgcn_s_memrealtime() - t0 > STEP_SPIN_TICKS;
                if (late || __hip_atomic_load(&bar->err[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
                    if (late && threadIdx.x == 0) __hip_atomic_store(&bar->err[0], (unsigned)(phase + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
            }
        }
    }
    __syncthreads();
}

template <int RB, int CB, int U, bool WT>
__device__ __forceinline__ void step_gemm(const __attribute__((address_space(4))) Gemm16& g, float* smem) {
    float* red = smem;
    float* stat = red + GEMM16_RED_WORDS(RB * CB);
    float* fin = stat + GEMM16_STAT_WORDS(RB);
    const int N = g.N, M = g.M, K = g.K, ks = g.ks, kz = g.kz;
    const long ldx = g.ldx;
    const float* x = gp_<true>(g.x);
    const float* w = gp_<true>(g.w);
    const int gx = (N + 16 * CB - 1) / (16 * CB), gy = (M + 16 * RB - 1) / (16 * RB);
    const int total = gx * gy * kz;
    // tile order = the launch's dispatch order (x fastest): the row blocks of a column tile are 96 / 32 / 128 tiles apart, a multiple
    // of 8, so with workgroups dealt to the XCDs round-robin they meet in one L2, as in the launch chain
    for (int vb = blockIdx.x; vb < total; vb += gridDim.x) {
        const int bx = vb % gx, r = vb / gx;
        gemm16_tile<RB, CB, U, true, WT>(x, w, ldx, K, N, M, ks, kz, g, bx, r % gy, r / gy, red, stat, fin);
        __syncthreads();   // the tile's LDS is the next tile's
    }
}

#define STEP_GEMM_WORDS(RB, CB) (GEMM16_RED_WORDS((RB) * (CB)) + GEMM16_STAT_WORDS(RB) + GEMM16_FIN_WORDS(RB))

// The argument block and the phase table live in device memory (d->program) and are read through CONSTANT-address-space pointers:
//   * as by-value kernel arguments the whole block -- the pick's sampler words included -- was loaded at the entry and stayed live in
//     scalar registers across all 122 phases (106 SGPRs, uniform values parked in vector registers);
//   * through an ordinary pointer the compiler must assume the kernel's own stores may alias the table: it then reads the (uniform)
//     operands with FLAT vector loads into vector registers and every pointer among them is a generic pointer -- flat loads and stores
//     for the tensors too, which s_waitcnt vmcnt does not even cover alone.  address_space(4) says "constant for this launch" (scalar
//     loads), and every pointer read from the table is cast through address_space(1) so that the accesses are global_* / buffer_*.
#define STEP_CONST __attribute__((address_space(4)))
#define STEP_GLOBAL __attribute__((address_space(1)))
template <typename T>
__device__ __forceinline__ T* as_global(T* p) {
    return (T*)(STEP_GLOBAL T*)p;
}
// amdgpu_waves_per_eu(8, 8): at most 64 registers per lane (no finer cap exists: amdgpu_num_vgpr is not honoured here).  Left alone,
// hipcc allocates 73 + 16 for this body although no phase needs more than the launch chain's 48: with 256 threads per workgroup it
// sees no reason to be frugal.  64 fit beside two convolution waves of up to 216 registers per SIMD (the 3 x 3 forms that carry
// the decoder's time: 208 / 214), not beside the 1 x 1 forms' 225 -- there the step's workgroup waits for one to retire, once per step.
// WT: every weight matrix of the phase table is tiled (ccvs_gpt_decode.w_tiled).  TOPP: the pick phase is the nucleus form
// (ccvs_gpt_decode.top_p inside (0, 1)) -- instantiations of their own, so that the ones without it are what they were.
template <int D, bool T2, bool WT, bool TOPP = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void gpt_step_kernel(const StepArgs* __restrict__ ap_) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int RB = T2 ? 2 : 1, CB = T2 ? 2 : 1, U = T2 ? 1 : GEMM_U;
    const unsigned G = gridDim.x;
    const STEP_CONST StepArgs* ap = (const STEP_CONST StepArgs*)ap_;
    StepBar* bar = as_global(ap->bar);
    const STEP_CONST StepPhase* prog = (const STEP_CONST StepPhase*)ap->prog;
    const int n_phases = ap->n_phases;
    const float att_scale = ap->scale;
    // (a vector load of a uniform word: read into a scalar register, or the barriers' target holds a vector register across every phase)
    unsigned target = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&bar->base[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    {   // embedding of the last picked token at row pos_off + *len (gpt_embed_kernel)
        const int B = ap->B, C = ap->C, vocab = ap->vocab, grp_rows = ap->grp_rows, pos_off = ap->pos_off;
        const int64_t* tok = as_global(ap->tok);
        const int32_t* len = as_global(ap->len);
        const float* tok_emb = as_global(ap->tok_emb);
        const float* pos_table = as_global(ap->pos_table);
        float* x = as_global(ap->x);
        const long total = (long)B * C;
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)G * 256) {
            const long b = i / C;
            const int c = (int)(i - b * C);
            long t = tok[b];
            t = t < 0 ? 0 : (t >= vocab ? vocab - 1 : t);
            const long prow = pos_off + len[grp_rows > 0 ? b / grp_rows : 0];
            st_act<true>(x + i, tok_emb[t * C + c] + pos_table[prow * C + c]);
        }
    }
    target += G; step_barrier(bar, target, 0);
    // ONE call site per tile body, operands from the phase table (per layer: ln1+QKV | attention | proj | ln2+fc | fc2; then ln_f+head)
#pragma unroll 1
    for (int ph = 0; ph < n_phases; ++ph) {
        const STEP_CONST StepPhase* P = prog + ph;
        if (P->kind == STEP_ATTENTION) {
            const STEP_CONST Gemm16& g = P->g;
            const int n_bh = g.M * g.H, H = g.H, Tmax = g.Tmax, grp_rows = g.grp_rows;
            const long q_sB = g.ldx;
            const float* q = as_global(g.x);
            const float* kc = as_global(g.kcache);
            const float* vc = as_global(g.vcache);
            float* att = as_global(g.y);
            const int32_t* len = as_global(g.pos_dev);
            for (int bh = blockIdx.x; bh < n_bh; bh += G) {   // attention over the cache
                attention_decode_item<D, KvF32, true>(q, q_sB, nullptr, nullptr, 0, kc, vc, att, H, 0, len, grp_rows, Tmax, att_scale, bh, smem);
                __syncthreads();
            }
        } else {
            step_gemm<RB, CB, U, WT>(P->g, smem);
        }
        target += G; step_barrier(bar, target, ph + 1);
    }
    // (workgroup 0, past the last barrier: the arrivals counted so far are the next launch's base -- no workgroup of THIS launch reads it again)
    if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(&bar->base[0], target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    {   // pick + bookkeeping
        const int B = ap->B, V = ap->V;
        Advance adv;
        adv.codes = as_global(ap->adv.codes); adv.codes_sB = ap->adv.codes_sB; adv.widx = as_global(ap->adv.widx); adv.len = as_global(ap->adv.len);
        adv.rng = ap->adv.rng;
#pragma unroll
        for (int i = 0; i < 5; ++i) adv.imm[i] = 0u;
        adv.state = as_global(ap->adv.state); adv.grp_rows = ap->adv.grp_rows; adv.noise_stream = as_global(ap->adv.noise_stream);
        for (int b = blockIdx.x; b < B; b += G) {
            if constexpr (TOPP)
                sample_topk_row<true, true>(as_global(ap->logits), (long)V, as_global(ap->noise), const_cast<int64_t*>(as_global(ap->tok)), 1L, V,
                                            ap->top_k, ap->temperature, adv, b, B, smem, ap->top_p);
            else
                sample_topk_row<true>(as_global(ap->logits), (long)V, as_global(ap->noise), const_cast<int64_t*>(as_global(ap->tok)), 1L, V, ap->top_k,
                                      ap->temperature, adv, b, B, smem);
            __syncthreads();
        }
    }
}

// 0 when the persistent steps launched with this workspace so far all completed their barriers (the stream is synchronised first)
extern "C" int ccvs_gpt_decode_status(const void* workspace, void* stream) {
    CCVS_REQUIRE(workspace, "ccvs_gpt_decode_status: null pointer");
    unsigned err = 0;
    const StepBar* bar = (const StepBar*)((const char*)workspace + GEMM_WS_BAR_OFFSET);
    hipError_t e = hipMemcpyAsync(&err, &bar->err[0], sizeof(err), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) { ccvs_set_error("ccvs_gpt_decode_status: %s", hipGetErrorString(e)); return CCVS_ERR_LAUNCH; }
    if (err) {
        // the arrival counters of the failed launch are inconsistent: start the workspace's barrier block over (every later step would
        // otherwise give up at once on the sticky word), then report
        (void)hipMemsetAsync((void*)bar, 0, sizeof(StepBar), (hipStream_t)stream);
        (void)hipStreamSynchronize((hipStream_t)stream);
        ccvs_set_error("ccvs_gpt_decode_status: a grid barrier of the persistent decode step gave up (phase %u): the tokens of the steps since the last check are invalid", err - 1);
        return CCVS_ERR_LAUNCH;
    }
    return CCVS_OK;
}

// d->program = [StepArgs, padded to STEP_HEAD_BYTES][5 n_layer + 1 phases]
#define STEP_HEAD_BYTES 512
static_assert(sizeof(StepArgs) <= STEP_HEAD_BYTES, "StepArgs outgrew the head of the program buffer");
extern "C" int64_t ccvs_gpt_program_bytes(int32_t n_layer) { return (int64_t)STEP_HEAD_BYTES + (int64_t)(5 * (n_layer > 0 ? n_layer : 0) + 1) * sizeof(StepPhase); }

static int step_check(const ccvs_gpt_decode* d, const char* who) {
    // what the persistent step covers -- what the pipelined generation uses -- and says so otherwise: no silent fall-back
    if (!(d->workspace && d->program)) { ccvs_set_error("%s: the persistent step needs `workspace` (ccvs_gemm_workspace_bytes, zeroed once) and `program` (ccvs_gpt_program_bytes)", who); return CCVS_ERR_ARG; }
    if (d->B > GEMM_DECODE_MAX_M) { ccvs_set_error("%s: the persistent step takes at most %d rows", who, GEMM_DECODE_MAX_M); return CCVS_ERR_ARG; }
    if (!gemm_tile2()) { ccvs_set_error("%s: the persistent step is built for the default tile (CCVS_GEMM_TILE2=1)", who); return CCVS_ERR_ARG; }
    if (!(d->C >= 32 && d->F >= 32 && d->V >= 32 && d->C % 16 == 0 && d->F % 16 == 0)) { ccvs_set_error("%s: the persistent step needs >= 32 output columns per GEMM and K %% 16 == 0", who); return CCVS_ERR_ARG; }
    if (!((long)d->V * d->C * 4 < (1L << 31) && (long)d->F * d->C * 4 < (1L << 31) && (long)d->B * d->F * 4 < (1L << 31))) { ccvs_set_error("%s: operand beyond 2^31 bytes (32-bit buffer offsets)", who); return CCVS_ERR_ARG; }
    return CCVS_OK;
}

// rows per group of a grouped step; 0: one group (widx / len / state are single words)
static int step_grp_rows(const ccvs_gpt_decode* d) { return d->groups > 1 ? d->B / d->groups : 0; }

// the bookkeeping block of the step's pick
static Advance step_advance(const ccvs_gpt_decode* d, int grp_rows) {
    Advance adv = {};
    adv.codes = d->codes; adv.codes_sB = (long)d->codes_sB; adv.widx = d->widx; adv.len = d->len;
    adv.rng = (d->rng && !d->noise && !d->noise_stream) ? 1 : 0; adv.state = d->state; adv.grp_rows = grp_rows;
    adv.noise_stream = d->noise ? nullptr : d->noise_stream;
    return adv;
}

// ln_f + head, the step's last GEMM
static Gemm16 step_head_gemm(const ccvs_gpt_decode* d) {
    Gemm16 g = {};
    g.x = d->x; g.ldx = d->C; g.w = d->head_w; g.bias = d->head_b; g.y = d->logits; g.ldy = d->V; g.M = d->B; g.N = d->V; g.K = d->C;
    g.ln_s = d->head_s; g.ln_eps = d->ln_eps; g.wt = d->w_tiled ? 1 : 0;
    return g;
}

// The tile of the persistent kernel's GEMM phases: the one gemm16_plan gives the step's last GEMM.  ccvs_gpt_decode_prepare checks that
// every GEMM phase of the table plans to it (they all have d->B rows and, by step_check, >= 32 columns).
static bool step_tile2(const ccvs_gpt_decode* d) {
    Gemm16 g = step_head_gemm(d);
    return gemm16_plan(g) == GEMM_FORM_TILE2;
}

// The step of d between its embedding and its pick, phase by phase in execution order: per layer ln1+QKV+scatter | attention | proj+res |
// ln2+fc+GELU | fc2+res, then ln_f+head.  BOTH forms of the step are produced by this one walk: the launch chain launches each phase,
// ccvs_gpt_decode_prepare plans it (gemm16_plan) and stores it in the persistent step's table.  visit(kind, g, name): `g` the phase's
// descriptor (STEP_ATTENTION: x = q, y = att, kcache / vcache, H, Tmax, M = rows), `name` its launch name in error texts; a result
// other than CCVS_OK ends the walk and is returned.  `who` names the caller in the layers' null-pointer check.
// kv16 (ccvs_gpt_decode_step_bf16kv, launch chain only): the caches are bf16 -- ln1 + QKV is the plain GEMM into d->q with row stride 3C
// (no scatter), and the attention phase carries q_sB = ldx = 3C; its K / V rows are the two upper thirds of that buffer.
template <typename Visit>
static int step_phases(const ccvs_gpt_decode* d, const char* who, Visit visit, bool kv16 = false) {
    const int D = d->C / d->H, grp_rows = step_grp_rows(d), wt = d->w_tiled ? 1 : 0;
    float* ws_slabs = (float*)d->workspace;
    int* ws_count = d->workspace ? (int*)((char*)d->workspace + GEMM_WS_SLAB_BYTES) : nullptr;
    int rc;
    for (int l = 0; l < d->n_layer; ++l) {
        const ccvs_gpt_layer& L = d->layers[l];
        CCVS_REQUIRE(L.qkv_w && L.qkv_b && L.qkv_s && L.proj_w && L.proj_b && L.fc_w && L.fc_b && L.fc_s && L.fc2_w && L.fc2_b && L.kcache && L.vcache,
                     "%s: null pointer in layer %d", who, l);
        Gemm16 g = {};  // ln1 + QKV + cache scatter
        g.x = d->x; g.ldx = d->C; g.w = L.qkv_w; g.bias = L.qkv_b; g.y = d->q; g.ldy = d->C; g.M = d->B; g.N = 3 * d->C; g.K = d->C;
        g.ln_s = L.qkv_s; g.ln_eps = d->ln_eps;
        g.kcache = L.kcache; g.vcache = L.vcache; g.C = d->C; g.H = d->H; g.D = D; g.Tq = 1; g.Tmax = d->Tmax; g.pos0 = 0; g.pos_dev = d->len; g.grp_rows = grp_rows;
        g.wt = wt;
        if (kv16) { g.ldy = 3 * d->C; g.kcache = g.vcache = nullptr; g.C = g.H = g.D = g.Tq = g.Tmax = 0; g.pos_dev = nullptr; g.grp_rows = 0; }
        if ((rc = visit(STEP_GEMM, g, kv16 ? "ccvs_gpt_decode_step_bf16kv(qkv)" : "ccvs_gpt_decode_step(qkv)")) != CCVS_OK) return rc;
        g = Gemm16{};  // attention over the cache
        g.x = d->q; g.ldx = kv16 ? 3 * d->C : d->C; g.y = d->att; g.kcache = L.kcache; g.vcache = L.vcache; g.H = d->H; g.M = d->B; g.Tmax = d->Tmax;
        g.pos_dev = d->len; g.grp_rows = grp_rows;
        if ((rc = visit(STEP_ATTENTION, g, kv16 ? "ccvs_gpt_decode_step_bf16kv(attention)" : "ccvs_gpt_decode_step(attention)")) != CCVS_OK) return rc;
        g = Gemm16{};  // proj + residual (in place on x)
        g.x = d->att; g.ldx = d->C; g.w = L.proj_w; g.bias = L.proj_b; g.res = d->x; g.y = d->x; g.ldy = d->C; g.M = d->B; g.N = d->C; g.K = d->C; g.epi = 2;
        g.ws_slabs = ws_slabs; g.ws_count = ws_count;
        g.wt = wt;
        if ((rc = visit(STEP_GEMM, g, kv16 ? "ccvs_gpt_decode_step_bf16kv(proj)" : "ccvs_gpt_decode_step(proj)")) != CCVS_OK) return rc;
        g = Gemm16{};  // ln2 + fc + GELU
        g.x = d->x; g.ldx = d->C; g.w = L.fc_w; g.bias = L.fc_b; g.y = d->h; g.ldy = d->F; g.M = d->B; g.N = d->F; g.K = d->C; g.epi = 1;
        g.ln_s = L.fc_s; g.ln_eps = d->ln_eps;
        g.wt = wt;
        if ((rc = visit(STEP_GEMM, g, kv16 ? "ccvs_gpt_decode_step_bf16kv(fc)" : "ccvs_gpt_decode_step(fc)")) != CCVS_OK) return rc;
        g = Gemm16{};  // fc2 + residual (in place on x)
        g.x = d->h; g.ldx = d->F; g.w = L.fc2_w; g.bias = L.fc2_b; g.res = d->x; g.y = d->x; g.ldy = d->C; g.M = d->B; g.N = d->C; g.K = d->F; g.epi = 2;
        g.ws_slabs = ws_slabs; g.ws_count = ws_count;
        g.wt = wt;
        if ((rc = visit(STEP_GEMM, g, kv16 ? "ccvs_gpt_decode_step_bf16kv(fc2)" : "ccvs_gpt_decode_step(fc2)")) != CCVS_OK) return rc;
    }
    Gemm16 g = step_head_gemm(d);
    return visit(STEP_GEMM, g, kv16 ? "ccvs_gpt_decode_step_bf16kv(head)" : "ccvs_gpt_decode_step(head)");
}

// The phase table of d's persistent step, written to d->program (device memory): the phases of step_phases, each GEMM planned by
// gemm16_plan -- the walk and the plan that the launch chain runs.  A synchronous copy on `stream`: once per descriptor, outside graph capture.
extern "C" int ccvs_gpt_decode_prepare(const ccvs_gpt_decode* d, void* stream) {
    CCVS_REQUIRE(d && d->layers && d->n_layer > 0 && d->C > 0 && d->H > 0 && d->C % d->H == 0, "ccvs_gpt_decode_prepare: bad descriptor");
    int rc = step_check(d, "ccvs_gpt_decode_prepare");
    if (rc != CCVS_OK) return rc;
    CCVS_REQUIRE(d->top_p == 0.f || d->top_p == 1.f || topp_on(d->top_p), "ccvs_gpt_decode_prepare: top_p %g is neither inside (0, 1) nor 0 / 1 (off)", (double)d->top_p);
    const int grp_rows = step_grp_rows(d), n_ph = 5 * d->n_layer + 1;
    const size_t bytes = (size_t)ccvs_gpt_program_bytes(d->n_layer);
    char* host = (char*)calloc(1, bytes);
    CCVS_REQUIRE(host, "ccvs_gpt_decode_prepare: out of host memory");
    StepPhase* prog = (StepPhase*)(host + STEP_HEAD_BYTES);
    {
        StepArgs& a = *(StepArgs*)host;
        a.B = d->B; a.C = d->C; a.V = d->V; a.vocab = d->vocab; a.grp_rows = grp_rows; a.pos_off = d->pos_off; a.n_phases = n_ph; a.H = d->H;
        a.tok_emb = d->tok_emb; a.pos_table = d->pos_table; a.tok = d->tok; a.len = d->len; a.x = d->x; a.logits = d->logits;
        a.bar = (StepBar*)((char*)d->workspace + GEMM_WS_BAR_OFFSET);
        a.prog = (const StepPhase*)((const char*)d->program + STEP_HEAD_BYTES);
        a.scale = 1.0f / sqrtf((float)(d->C / d->H));
        a.noise = d->noise; a.top_k = d->top_k; a.temperature = d->temperature; a.top_p = d->top_p;
        a.adv = step_advance(d, grp_rows);
    }
    // The kernel runs ONE tile (step_tile2) for all its GEMM phases and the table has n_ph slots: a walk or a plan that disagrees with
    // either is a bug in this file, never a caller's error -- reported all the same, before anything is written to d->program.
    const GemmForm tile = step_tile2(d) ? GEMM_FORM_TILE2 : GEMM_FORM_TILE1;
    int n = 0;
    rc = step_phases(d, "ccvs_gpt_decode_prepare", [&](int kind, Gemm16& g, const char* name) -> int {
        if (n == n_ph || (kind == STEP_GEMM && (gemm16_plan(g) != tile || !gemm_ws_holds(g) || !gemm_wt_holds(g)))) { ccvs_set_error("ccvs_gpt_decode_prepare: %s does not fit the persistent step's table", name); return CCVS_ERR_ARG; }
        prog[n].kind = kind;
        prog[n++].g = g;
        return CCVS_OK;
    });
    if (rc == CCVS_OK && n != n_ph) { ccvs_set_error("ccvs_gpt_decode_prepare: %d phases, the table holds %d", n, n_ph); rc = CCVS_ERR_ARG; }
    if (rc != CCVS_OK) { free(host); return rc; }
    hipError_t e = hipMemcpyAsync(d->program, host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    free(host);
    if (e != hipSuccess) { ccvs_set_error("ccvs_gpt_decode_prepare: %s", hipGetErrorString(e)); return CCVS_ERR_LAUNCH; }
    return CCVS_OK;
}

static int launch_step_persistent(const ccvs_gpt_decode* d, int D, hipStream_t st) {
    static int n_cu = 0;
    if (!n_cu) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) { ccvs_set_error("ccvs_gpt_decode_step: no device properties"); return CCVS_ERR_LAUNCH; }
        n_cu = prop.multiProcessorCount;
    }
    const StepArgs* a = (const StepArgs*)d->program;   // written by ccvs_gpt_decode_prepare
    // one workgroup per CU: more of them are all resident only with the chip to the step itself -- beside the frame decoder a CU has
    // room for one -- and every grid barrier then waits for 2-4 x the arrivals (profiles/r06_persistent_step.txt)
    const bool t2 = step_tile2(d);
    size_t words = t2 ? STEP_GEMM_WORDS(2, 2) : STEP_GEMM_WORDS(1, 1);
    const bool topp = topp_on(d->top_p);   // (the table's top_p is the one ccvs_gpt_decode_prepare saw: a descriptor changed since is prepared again)
    const size_t w_att = 16 + 4 * 256 + (size_t)d->Tmax, w_pick = topp ? PICK_TOPP_SMEM_WORDS(d->V) : PICK_SMEM_WORDS(d->V);
    if (w_att > words) words = w_att;
    if (w_pick > words) words = w_pick;
    const size_t smem = words * sizeof(float);
#define STEP_LAUNCH__(Dv, T2v, WTv, TPv)                                                                                               \
    do {                                                                                                                              \
        static bool attr_set = false;                                                                                                 \
        if (!attr_set) {                                                                                                              \
            (void)hipFuncSetAttribute((const void*)gpt_step_kernel<Dv, T2v, WTv, TPv>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); \
            attr_set = true;                                                                                                          \
        }                                                                                                                             \
        hipLaunchKernelGGL((gpt_step_kernel<Dv, T2v, WTv, TPv>), dim3(n_cu), dim3(256), smem, st, a);                                 \
    } while (0)
#define STEP_LAUNCH_(Dv, T2v, WTv) do { if (topp) STEP_LAUNCH__(Dv, T2v, WTv, true); else STEP_LAUNCH__(Dv, T2v, WTv, false); } while (0)
#define STEP_LAUNCH(Dv, T2v) do { if (d->w_tiled) STEP_LAUNCH_(Dv, T2v, true); else STEP_LAUNCH_(Dv, T2v, false); } while (0)
    if (D == 64) { if (t2) STEP_LAUNCH(64, true); else STEP_LAUNCH(64, false); }
    else if (D == 32) { if (t2) STEP_LAUNCH(32, true); else STEP_LAUNCH(32, false); }
    else { if (t2) STEP_LAUNCH(16, true); else STEP_LAUNCH(16, false); }
#undef STEP_LAUNCH
#undef STEP_LAUNCH_
#undef STEP_LAUNCH__
    CCVS_CHECK_LAUNCH("ccvs_gpt_decode_step(persistent)");
    return CCVS_OK;
}

// ---------------------------------------------------------------------------------------
// One decode step: the launch sequence of ccvs_gpt_embed / ccvs_gemm_ln_qkv / ccvs_attention /
// ccvs_gemm_nt / ccvs_gemm_ln / ccvs_sample_topk for a single new position, 5 * n_layer + 3 launches
// on one stream, every per-step quantity device-resident (hipGraph-capturable).
// ---------------------------------------------------------------------------------------
static int decode_step(const ccvs_gpt_decode* d, void* stream, bool kv16) {
    const char* who = kv16 ? "ccvs_gpt_decode_step_bf16kv" : "ccvs_gpt_decode_step";   // the entry the caller came through, in every error text
    CCVS_REQUIRE(d && d->layers && d->tok_emb && d->pos_table && d->head_w && d->head_b && d->head_s, "%s: null pointer", who);
    CCVS_REQUIRE(d->tok && d->codes && d->widx && d->len && d->x && d->q && d->att && d->h && d->logits && d->state,
                 "%s: null state pointer", who);
    CCVS_REQUIRE(d->B > 0 && d->C > 0 && d->H > 0 && d->C % d->H == 0 && d->F > 0 && d->n_layer > 0 && d->Tmax > 0 && d->vocab > 0 && d->V > 0,
                 "%s: bad shape", who);
    const int D = d->C / d->H;
    CCVS_REQUIRE(D == 64 || D == 32 || D == 16, "%s: head dim %d unsupported (16, 32, 64)", who, D);
    CCVS_REQUIRE(d->temperature > 0.f, "%s: bad temperature", who);
    CCVS_REQUIRE(d->groups >= 0 && (d->groups <= 1 || d->B % d->groups == 0), "%s: %d rows do not split into %d groups", who, d->B, d->groups);
    // (more rows than the weight-stream form takes run the row-blocked form inside launch_gemm16; row groups cannot)
    CCVS_REQUIRE(d->groups <= 1 || d->B <= GEMM_DECODE_MAX_M, "%s: at most %d rows per grouped step", who, GEMM_DECODE_MAX_M);
    const int grp_rows = step_grp_rows(d);
    const size_t smem_att = (size_t)(16 + 4 * 256 + d->Tmax) * sizeof(float);
    // the pick's form: top_p 0 or 1 = off (the top-k form), inside (0, 1) = the nucleus form with its own LDS size and cap
    CCVS_REQUIRE(d->top_p == 0.f || d->top_p == 1.f || topp_on(d->top_p), "%s: top_p %g is neither inside (0, 1) nor 0 / 1 (off)", who, (double)d->top_p);
    const bool topp = topp_on(d->top_p);
    const size_t smem_pick = (size_t)(topp ? PICK_TOPP_SMEM_WORDS(d->V) : PICK_SMEM_WORDS(d->V)) * sizeof(float);
    CCVS_REQUIRE(smem_att <= 64 * 1024, "%s: sequence too long for the LDS score buffer", who);
    if (topp) CCVS_REQUIRE(smem_pick <= 160 * 1024, "%s: vocabulary %d too large for the top_p form (at most %d)", who, d->V, ccvs_sample_topp_max_vocab());
    CCVS_REQUIRE(smem_pick <= 160 * 1024, "%s: vocabulary %d too large", who, d->V);
    hipStream_t st = (hipStream_t)stream;
    // (bf16 caches: gpt_step_kernel's attention phase and its QKV scatter read and write fp32 cache rows)
    CCVS_REQUIRE(!(kv16 && d->persistent), "ccvs_gpt_decode_step_bf16kv: persistent = 1 is refused: the persistent step (gpt_step_kernel) runs on fp32 KV caches only");
    if (d->persistent) {   // ONE launch (gpt_step_kernel) over the phase table ccvs_gpt_decode_prepare wrote to d->program
        int rc_ = step_check(d, who);
        if (rc_ != CCVS_OK) return rc_;
        return launch_step_persistent(d, D, st);
    }
    pick_allow_big_lds();

    {   // embedding of the last picked token at row pos_off + *len
        const long total = (long)d->B * d->C;
        hipLaunchKernelGGL(gpt_embed_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, d->tok, 1L, (const int32_t*)nullptr, d->pos_off,
                           (const int32_t*)d->len, grp_rows, 1, d->tok_emb, d->pos_table, d->x, total, d->C, d->vocab);
        CCVS_CHECK_LAUNCH(kv16 ? "ccvs_gpt_decode_step_bf16kv(embed)" : "ccvs_gpt_decode_step(embed)");
    }
    const float scale = 1.0f / sqrtf((float)D);
    const int rc = step_phases(d, who, [&](int kind, Gemm16& g, const char* name) -> int {
        if (kind == STEP_GEMM) return launch_gemm16(g, st, name);
        // bf16 caches, the appending form: K and V of this position are columns C.. and 2C.. of the QKV output
        ccvs_launch_attention_decode(kv16, D, g.M * g.H, smem_att, st, g.x, g.ldx, kv16 ? g.x + d->C : nullptr, kv16 ? g.x + 2 * d->C : nullptr,
                                     g.ldx, g.kcache, g.vcache, g.y, g.H, 0, g.pos_dev, g.grp_rows, g.Tmax, scale);
        CCVS_CHECK_LAUNCH(name);
        return CCVS_OK;
    }, kv16);
    if (rc != CCVS_OK) return rc;
    // pick + bookkeeping
    if (topp) {
        pick_topp_allow_big_lds();
        hipLaunchKernelGGL(sample_topp_kernel, dim3(d->B), dim3(256), smem_pick, st, d->logits, (long)d->V, d->noise, d->tok, 1L, d->V,
                           d->top_k, d->temperature, d->top_p, step_advance(d, grp_rows));
    } else {
        hipLaunchKernelGGL(sample_topk_kernel, dim3(d->B), dim3(256), smem_pick, st, d->logits, (long)d->V, d->noise, d->tok, 1L, d->V,
                           d->top_k, d->temperature, step_advance(d, grp_rows));
    }
    CCVS_CHECK_LAUNCH(kv16 ? "ccvs_gpt_decode_step_bf16kv(pick)" : "ccvs_gpt_decode_step(pick)");
    return CCVS_OK;
}

extern "C" int ccvs_gpt_decode_step(const ccvs_gpt_decode* d, void* stream) { return decode_step(d, stream, false); }

// The same chain on bf16 KV caches (include/ccvs_hip_kv16.h): layers[i].kcache / vcache point to bf16, d->q holds 3C floats per row.
extern "C" int ccvs_gpt_decode_step_bf16kv(const ccvs_gpt_decode* d, void* stream) { return decode_step(d, stream, true); }

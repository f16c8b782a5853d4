// KV-cached causal attention over fp32 and bfloat16 caches (head dim 16 / 32 / 64): the cache-row policies, the prefill kernel and
// the decode body.  attention.hip instantiates the kernels and holds the append kernels and the entries (include/ccvs_hip.h:
// ccvs_kv_append, ccvs_attention; include/ccvs_hip_kv16.h: the bf16 mode and its entries); gpt.hip runs the decode body as the attention
// phase of gpt_step_kernel.  Each algorithm is written once; what depends on the type of a cache row is in KvF32 / KvBf16.
// Positions may come from a device-resident int32 (`pos_dev`, added to pos0) so that a decode
// step captured in a hipGraph replays at advancing positions without re-capture.
#pragma once
#include <math.h>

#include "act_access.h"
#include "common.h"

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// fp32 -> bf16, round to nearest even on the bit pattern; NaN -> 0x7fc0.  torch.Tensor.to(torch.bfloat16), bit for bit, for every input.
__device__ __forceinline__ unsigned bf16_rne(float f) {
    const unsigned u = __float_as_uint(f);
    const unsigned r = (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
    return (u & 0x7fffffffu) > 0x7f800000u ? 0x7fc0u : r;
}
__device__ __forceinline__ unsigned bf16_rne2(float lo, float hi) { return bf16_rne(lo) | (bf16_rne(hi) << 16); }
// the two bf16 of a word, widened exactly
__device__ __forceinline__ float bf16_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }

// ---------------------------------------------------------------------------------------
// The cache-row policies.  For the prefill kernel: a UNIT is the 16 bytes of a cache row that a thread fetches, EPU head dims.
// For the decode body: a lane owns EPL consecutive head dims of a key row = 16 bytes (row_t) for either type, fetched with ONE
// non-temporal load (a stream read once); lane_base / load_nt hold each type's address form (fp32: a 64-bit pointer per lane and
// a 64-bit row offset; bf16: a workgroup-uniform base plus a 32-bit element offset per lane, one address register per load in
// flight instead of two); APPENDS: the form that writes the current position itself.
// The few statements that WIDEN a fetched unit or row (the prefill kernel's stores into its LDS tiles, the decode body's dot product
// and PV sum) are not functions of the policies: they stand in the one body, per type, under `if constexpr (EPU / EPL == 4)`.  Behind
// a function, or as one loop over widened elements, the fp32 kernels compile to other code than before the bodies were shared
// (profiles/attention_one_body.txt); in place, on the registers themselves, they compile to the same.
// ---------------------------------------------------------------------------------------
struct KvF32 {
    typedef float elem_t;
    typedef float4 unit_t;
    static constexpr int EPU = 4;
    static __device__ __forceinline__ unit_t zero_unit() { return make_float4(0.f, 0.f, 0.f, 0.f); }

    typedef const float* cache_t;   // the caches as the decode body takes them
    typedef f32x4 row_t;
    static constexpr int EPL = 4;
    static constexpr bool APPENDS = false;
    static __device__ __forceinline__ const float* lane_base(const float* head, int dc) { return head + 4 * dc; }
    template <int D>
    static __device__ __forceinline__ row_t load_nt(const float* base, int row, int) {
        return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(base + (long)row * D));
    }
};

struct KvBf16 {
    typedef uint16_t elem_t;
    typedef u32x4 unit_t;
    static constexpr int EPU = 8;
    static __device__ __forceinline__ unit_t zero_unit() { return unit_t{0u, 0u, 0u, 0u}; }   // (bf16 0 widens to 0.f)

    typedef uint16_t* cache_t;   // (not const: the appending form stores row L - 1)
    typedef u32x4 row_t;
    static constexpr int EPL = 8;
    static constexpr bool APPENDS = true;
    static __device__ __forceinline__ uint16_t* lane_base(uint16_t* head, int) { return head; }
    template <int D>
    static __device__ __forceinline__ row_t load_nt(const uint16_t* base, int row, int dc) {
        return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(base + (unsigned)(row * D) + (unsigned)(8 * dc)));
    }
};

// Prefill form (Tq > 1): flash-style attention on the fp32 matrix cores (v_mfma_f32_32x32x2_f32), exact fp32 products.
//
// A workgroup = 4 waves = 4 blocks of 32 queries of one (batch, head); the K / V rows of the cache are walked in tiles of
// 32 keys staged ONCE per workgroup in LDS (K transposed to [d][key], V as [key][d]) and shared by its 128 queries.
// Per wave and key tile:
//   S^T = K . Q^T   (A = K tile from LDS, B = the wave's Q block held in registers, pre-scaled by 1/sqrt(D)): the 32x32
//         accumulator layout gives every lane ONE query (column lane%32) and 16 of the 32 keys, so the causal mask, the
//         running max / sum of the online softmax and the exponentials are per-lane register work plus one xor-32 shuffle;
//   O^T += V^T . P^T   the probabilities are used as the B operand straight from the S accumulator registers: MFMA step
//         j contracts over the key that accumulator register j holds in each lane half (the contraction order over keys
//         is free), and the A operand reads the matching V row from LDS -- P never moves;
//   O is rescaled by exp(m_old - m_new) when the running max moves.
// Query t (position pos0 + t) sees keys 0 .. pos0 + t; tiles beyond a wave's last query are skipped by that wave.  Two
// tile buffers: tile i+1 is fetched into registers before tile i is consumed and stored after it, one barrier per tile.
// The result goes through LDS so that it is written with lanes along the head dimension (coalesced rows of `out`).
// Replaces the softmax(QK^T / sqrt(d) masked) V of mingpt.py:67-77 for whole sequences (prefill, teacher-forced forward,
// the re-prefill of a slid token window).
// A bf16 cache (KV = KvBf16) differs in the tile loader alone: a thread fetches 16 bytes = 8 head dims of a key row and of a value
// row instead of 4 and widens them while it stores them into the SAME fp32 LDS tiles.
template <int D, class KV>
__global__ __launch_bounds__(256) void attention_prefill_kernel(const float* __restrict__ q, long q_sB, long ldq,
                                                                const typename KV::elem_t* __restrict__ kc,
                                                                const typename KV::elem_t* __restrict__ vc, float* __restrict__ out, int H,
                                                                int Tq, int pos0, const int32_t* __restrict__ pos_dev, int Tmax, float scale) {
    typedef typename KV::unit_t unit_t;
    constexpr int MT = (D + 31) / 32;   // 32-row tiles of the head dimension in O^T
    constexpr int DP = MT * 32;         // head dimension padded to the tile (zero columns of V)
    constexpr int DK = D / 2;           // MFMA steps of S (K = 2 per step)
    constexpr int KS = 33;              // row stride of the transposed K tile
    constexpr int EPU = KV::EPU;        // head dims per 16-byte unit
    constexpr int UPR = D / EPU;        // units per cache row
    constexpr int NLD = (32 * UPR + 255) / 256;  // units per thread and tile
    constexpr int TILE_WORDS = D * KS + 32 * DP;
    constexpr int OUT_WORDS = 128 * (D + 1);
    constexpr int SMEM_WORDS = 2 * TILE_WORDS > OUT_WORDS ? 2 * TILE_WORDS : OUT_WORDS;
    __shared__ __attribute__((aligned(16))) float smem[SMEM_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qi = lane & 31, half = lane >> 5;
    // grid = (batch x head, query block): blocks are dispatched x-fastest, so ALL (batch, head) pairs of the last query block
    // -- the one with the most visible keys under the causal mask -- start first and the short blocks fill the tail
    const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
    if (pos_dev) pos0 += *pos_dev;
    const int q0 = (gridDim.y - 1 - blockIdx.y) * 128;     // first query of the workgroup
    const int qw = q0 + wave * 32;                         // first query of the wave
    const int qidx = qw + qi;                              // this lane's query
    const int q_last_wg = min(q0 + 127, Tq - 1), q_last_w = min(qw + 31, Tq - 1);
    const int ntiles = (min(pos0 + q_last_wg + 1, Tmax) + 31) >> 5;
    const typename KV::elem_t* kbase = kc + (long)bh * Tmax * D;
    const typename KV::elem_t* vbase = vc + (long)bh * Tmax * D;

    // Q block of the wave: lane holds Q[qidx][2i + half], i = 0 .. DK-1 (B operand of step i)
    float qreg[DK];
    {
        const float* qp = q + (long)b * q_sB + (long)min(qidx, Tq - 1) * ldq + h * D + half;
#pragma unroll
        // scores are kept in the log2 domain (scale * log2(e) folded into Q): the softmax then needs v_exp_f32 only
        for (int i = 0; i < DK; ++i) qreg[i] = (qidx < Tq) ? qp[2 * i] * (scale * 1.44269504088896340736f) : 0.f;
    }
    if (MT * 32 > D) {  // zero the padding columns of both V buffers once (D = 16)
        for (int e = tid; e < 2 * 32 * (DP - D); e += 256) {
            const int bsel = e / (32 * (DP - D)), r = e - bsel * 32 * (DP - D);
            smem[bsel * TILE_WORDS + D * KS + (r / (DP - D)) * DP + D + r % (DP - D)] = 0.f;
        }
    }

    unit_t kreg[NLD], vreg[NLD];
    auto fetch = [&](int kt) {
#pragma unroll
        for (int r = 0; r < NLD; ++r) {
            const int e = min(tid + 256 * r, 32 * UPR - 1);
            const int key = e / UPR, du = e - key * UPR;
            // cache rows >= pos0 + Tq have never been written: their scores are masked (select) but a 0 x NaN in the PV
            // product would still poison the sum, so such rows are staged as zeros (and never read: the address is clamped)
            const bool written = kt * 32 + key < pos0 + Tq;
            const long row = min(kt * 32 + key, pos0 + Tq - 1);
            const unit_t kv = *reinterpret_cast<const unit_t*>(kbase + row * D + EPU * du);
            const unit_t vv = *reinterpret_cast<const unit_t*>(vbase + row * D + EPU * du);
            kreg[r] = written ? kv : KV::zero_unit();
            vreg[r] = written ? vv : KV::zero_unit();
        }
    };
    auto stash = [&](int buf) {
        float* kt_s = smem + buf * TILE_WORDS;
        float* v_s = kt_s + D * KS;
#pragma unroll
        for (int r = 0; r < NLD; ++r) {
            const int e = tid + 256 * r;
            if (e < 32 * UPR) {
                const int key = e / UPR, du = e - key * UPR;
                // (each type's own statements, on kreg / vreg themselves: behind a function of the policy, or as one loop over EPU
                //  widened elements, the fp32 kernels compile to other code)
                if constexpr (EPU == 4) {
                    kt_s[(4 * du + 0) * KS + key] = kreg[r].x;
                    kt_s[(4 * du + 1) * KS + key] = kreg[r].y;
                    kt_s[(4 * du + 2) * KS + key] = kreg[r].z;
                    kt_s[(4 * du + 3) * KS + key] = kreg[r].w;
                    *reinterpret_cast<float4*>(v_s + key * DP + 4 * du) = vreg[r];
                } else {
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        kt_s[(8 * du + 2 * w + 0) * KS + key] = bf16_lo(kreg[r][w]);
                        kt_s[(8 * du + 2 * w + 1) * KS + key] = bf16_hi(kreg[r][w]);
                    }
                    *reinterpret_cast<float4*>(v_s + key * DP + 8 * du) =
                        make_float4(bf16_lo(vreg[r][0]), bf16_hi(vreg[r][0]), bf16_lo(vreg[r][1]), bf16_hi(vreg[r][1]));
                    *reinterpret_cast<float4*>(v_s + key * DP + 8 * du + 4) =
                        make_float4(bf16_lo(vreg[r][2]), bf16_hi(vreg[r][2]), bf16_lo(vreg[r][3]), bf16_hi(vreg[r][3]));
                }
            }
        }
    };

    f32x16 acc_o[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_o[mt][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    fetch(0);
    __syncthreads();   // padding columns zeroed
    stash(0);
    __syncthreads();
    for (int kt = 0; kt < ntiles; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < ntiles) fetch(kt + 1);
        const int key0 = kt * 32;
        if (key0 <= pos0 + q_last_w && qw < Tq) {   // wave-uniform: this tile holds keys visible to the wave
            const float* kt_s = smem + buf * TILE_WORDS;
            const float* v_s = kt_s + D * KS;
            f32x16 s;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
            for (int i = 0; i < DK; ++i) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kt_s[(2 * i + half) * KS + qi], qreg[i], s, 0, 0, 0);
            // s[r] = S[query qidx][key key0 + 8*(r/4) + 4*half + r%4]
            const int lim = pos0 + qidx - key0;   // keys with index <= lim are visible
            float m_t = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kk = 8 * (r >> 2) + 4 * half + (r & 3);
                s[r] = (kk <= lim && qidx < Tq) ? s[r] : -INFINITY;
                m_t = fmaxf(m_t, s[r]);
            }
            m_t = fmaxf(m_t, __shfl_xor(m_t, 32, 64));
            const float m_new = fmaxf(m_run, m_t);
            const float m_use = (m_new == -INFINITY) ? 0.f : m_new;   // nothing visible yet: every p below is 2^-inf = 0
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);  // m_run = -inf -> 0
            float l_t = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[r] = __builtin_amdgcn_exp2f(s[r] - m_use);
                l_t += s[r];
            }
            l_t += __shfl_xor(l_t, 32, 64);
            l_run = l_run * alpha + l_t;
            m_run = m_new;
            const bool rescale = __any(alpha != 1.f);   // wave-uniform: the running max of no lane moved -> O keeps its scale
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                if (rescale) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc_o[mt][r] *= alpha;
                }
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int kk = 8 * (j >> 2) + 4 * half + (j & 3);
                    acc_o[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(v_s[kk * DP + mt * 32 + qi], s[j], acc_o[mt], 0, 0, 0);
                }
            }
        }
        if (kt + 1 < ntiles) stash(buf ^ 1);   // the other buffer: its last readers passed the barrier of the previous tile
        __syncthreads();
    }
    // O[d][query] / l  ->  LDS [query][d]  ->  out rows (lanes along d)
    float* o_s = smem;
    const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int d = mt * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
            if (d < D) o_s[(wave * 32 + qi) * (D + 1) + d] = acc_o[mt][r] * inv;
        }
    __syncthreads();
    for (int e = tid; e < 128 * D; e += 256) {
        const int ql = e / D, d = e - ql * D;
        if (q0 + ql < Tq) out[((long)b * Tq + q0 + ql) * (H * D) + h * D + d] = o_s[ql * (D + 1) + d];
    }
}

// Decode form (Tq = 1): one workgroup per (batch, head) streams that head's K and V rows once.
// A key row is read by D/EPL consecutive lanes, 16 bytes each (a wave-instruction covers 64/(D/EPL) whole rows: 1 KiB,
// fully coalesced); the partial dots are summed across those lanes with xor shuffles.  PV uses the same lane map (lane
// owns EPL head dims of one key slot); the key slots of a wave and the 4 waves are reduced through LDS in a fixed order
// (wave, then slot), EPL / 4 rounds through the SAME 4 KB.
// Footprint (see gemm16_kernel): 256 threads, <= 48 VGPRs, LDS = scores + 4 KB -- the workgroup is dispatched next to a
// convolution workgroup of the frame decoder instead of waiting for one to retire; a stream of this shape keeps 3.5 TB/s
// beside the decoder (5.5 alone; tools/chain_probe.py).  Four key rows per lane are requested together (16 KB in flight
// per workgroup); the first V batch is requested before the softmax reduction starts.
// (bh = the (batch row, head) pair; smem = 16 + 1024 + Tmax floats.  COH: the persistent decode step -- q, the cache row of the
//  CURRENT position (written by the QKV phase of the same launch) and the output are handed between workgroups of one launch:
//  sc1 accesses; the older cache rows were written by earlier launches and stay on the plain / non-temporal stream.  fp32 caches only.)
// THE APPEND (KV::APPENDS and k_new != NULL): the lanes of slot 0 of wave 0 round the new K and V rows, store them at position L - 1
// and leave the same words in LDS; every lane takes them from there in place of whatever a load of a row >= L - 1 returned (row
// L - 1 itself and the clamped tail of the last batch): the stored bits and the used bits are the same words, and nothing read
// depends on the store.  Exactly one workgroup owns a (row, head), so no other workgroup reads or writes that cache row in this
// launch.  The words lie in the first 64 B of pv, which is free until the final reduction.  Registers: see DESIGN.md 4.28.
template <int D, class KV, bool COH>
__device__ __forceinline__ void attention_decode_item(const float* __restrict__ q, long q_sB, const float* __restrict__ k_new,
                                                      const float* __restrict__ v_new, long kv_sB, typename KV::cache_t __restrict__ kc,
                                                      typename KV::cache_t __restrict__ vc, float* __restrict__ out, int H, int pos0,
                                                      const int32_t* __restrict__ pos_dev, int grp_rows, int Tmax, float scale, int bh,
                                                      float* smem) {
    static_assert(!(COH && KV::APPENDS), "the persistent step appends in its QKV phase: fp32 caches only");
    typedef typename KV::row_t row_t;
    constexpr int EPL = KV::EPL;     // head dims per lane
    constexpr int LPK = D / EPL;     // lanes per key row
    constexpr int KPI = 64 / LPK;    // key rows per wave-instruction
    constexpr int NW = 4;
    constexpr int AU = 4;            // key rows per lane whose loads are issued together
    constexpr int BATCH = NW * KPI * AU;
    float* red = smem;                    // [16]
    float* pv = smem + 16;                // [NW][64][4]
    float* ps = smem + 16 + NW * 256;     // [Tmax]
    const int tid = thread_id<COH>(), lane = tid & 63, wave = tid >> 6;
    const int b = bh / H, h = bh - b * H;
    if (pos_dev) {   // row groups of a decode step: one cache length per group
        // (COH: the length words are constant for the whole launch until the pick's last row moves them on, after every other reader:
        //  a SCALAR load through the constant address space -- as a vector load of a uniform address the value, and with it the
        //  loop bounds and row addresses, is per-lane data to the compiler)
        if constexpr (COH) pos0 += ((const __attribute__((address_space(4))) int32_t*)pos_dev)[grp_rows > 0 ? b / grp_rows : 0];
        else pos0 += pos_dev[grp_rows > 0 ? b / grp_rows : 0];
    }
    [[maybe_unused]] bool append = false;
    if constexpr (KV::APPENDS) {
        pos0 = max(pos0, 0);   // (a negative device-resident position: no caller's contract, and no address below row 0)
        append = k_new != nullptr && pos0 < Tmax;
    }
    const int L = min(pos0 + 1, Tmax);
    const int kk = lane / LPK, dc = lane - kk * LPK;
    const auto kbase = KV::lane_base(kc + (long)bh * Tmax * D, dc);
    const auto vbase = KV::lane_base(vc + (long)bh * Tmax * D, dc);
    const int jw = wave * KPI + kk;  // this lane's row within a batch, + u * NW * KPI
    const int nbatch = (L + BATCH - 1) / BATCH;

    // unconditional loads from clamped rows (predicated loads would serialise)
    // COH: rows >= L - 1 (the position this step appends, and the clamped tail of the last batch) take the row fetched by ONE sc1
    // load instead of whatever the streaming load of that address returned -- same values, same arithmetic, no stale line
    [[maybe_unused]] row_t last[2] = {};   // row L - 1 of K, of V
    if constexpr (COH) {
        last[0] = ld_act4_sc1(kbase + (long)(L - 1) * D);
        last[1] = ld_act4_sc1(vbase + (long)(L - 1) * D);
    }
    [[maybe_unused]] unsigned* fresh_s = reinterpret_cast<unsigned*>(pv);   // APPENDS: [2][D / 2] words, the rounded new K row, then V
#define ATT_LOAD(dst, base, bi, which)                                                                                                    \
    _Pragma("unroll") for (int u = 0; u < AU; ++u) {                                                                                      \
        const int j_ = (bi) * BATCH + jw + u * NW * KPI;                                                                                  \
        dst[u] = KV::template load_nt<D>(base, min(j_, L - 1), dc);                                                                       \
        if constexpr (COH) { if (j_ >= L - 1) dst[u] = last[which]; }                                                                     \
        if constexpr (KV::APPENDS) {                                                                                                      \
            if (append && j_ >= L - 1) dst[u] = *reinterpret_cast<const row_t*>(fresh_s + (which) * (D / 2) + (EPL / 2) * dc);            \
        }                                                                                                                                 \
    }

    // (written out for 4 and 8 head dims per lane: as a loop over e with one trip, the fp32 kernels compile to another schedule)
    float qv[EPL];
#define ATT_LOAD_Q(e)                                                                  \
    {                                                                                  \
        const float* qp = q + (long)b * q_sB + h * D + EPL * dc + e;                   \
        if constexpr (COH) {                                                           \
            const f32x4 t = ld_act4_sc1(qp);                                           \
            qv[e] = t[0]; qv[e + 1] = t[1]; qv[e + 2] = t[2]; qv[e + 3] = t[3];        \
        } else {                                                                       \
            const float4 t = *reinterpret_cast<const float4*>(qp);                     \
            qv[e] = t.x; qv[e + 1] = t.y; qv[e + 2] = t.z; qv[e + 3] = t.w;            \
        }                                                                              \
    }
    ATT_LOAD_Q(0)
    if constexpr (EPL == 8) ATT_LOAD_Q(4)
#undef ATT_LOAD_Q
    if constexpr (KV::APPENDS) {
        if (append && wave == 0 && kk == 0) {
            row_t k_fresh, v_fresh;
            const float* kn = k_new + (long)b * kv_sB + h * D + EPL * dc;
            const float* vn = v_new + (long)b * kv_sB + h * D + EPL * dc;
#pragma unroll
            for (int e = 0; e < EPL; e += 4) {
                const float4 a = *reinterpret_cast<const float4*>(kn + e), c = *reinterpret_cast<const float4*>(vn + e);
                k_fresh[e / 2] = bf16_rne2(a.x, a.y); k_fresh[e / 2 + 1] = bf16_rne2(a.z, a.w);
                v_fresh[e / 2] = bf16_rne2(c.x, c.y); v_fresh[e / 2 + 1] = bf16_rne2(c.z, c.w);
            }
            *reinterpret_cast<row_t*>(kbase + (unsigned)((L - 1) * D) + (unsigned)(EPL * dc)) = k_fresh;
            *reinterpret_cast<row_t*>(vbase + (unsigned)((L - 1) * D) + (unsigned)(EPL * dc)) = v_fresh;
            *reinterpret_cast<row_t*>(fresh_s + (EPL / 2) * dc) = k_fresh;
            *reinterpret_cast<row_t*>(fresh_s + D / 2 + (EPL / 2) * dc) = v_fresh;
        }
        __syncthreads();   // the rounded row is in LDS for every wave
    }

    float lmax = -INFINITY;
#pragma unroll 1   // (one batch of AU rows in flight per lane: the 48-register budget; hipcc unrolls this loop by two once the body is an inlined function)
    for (int bi = 0; bi < nbatch; ++bi) {
        row_t kv[AU];
        ATT_LOAD(kv, kbase, bi, 0);
#pragma unroll
        for (int u = 0; u < AU; ++u) {
            const int j = bi * BATCH + jw + u * NW * KPI;
            // (each type's own statement on kv[u] itself, here and in the PV loop: through a function of the policy the fp32 kernels
            //  compile to another schedule)
            float s;
            if constexpr (EPL == 4) {
                s = kv[u][0] * qv[0] + kv[u][1] * qv[1] + kv[u][2] * qv[2] + kv[u][3] * qv[3];
            } else {
                s = 0.f;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    s += bf16_lo(kv[u][w]) * qv[2 * w];
                    s += bf16_hi(kv[u][w]) * qv[2 * w + 1];
                }
            }
#pragma unroll
            for (int o = 1; o < LPK; o <<= 1) s += __shfl_xor(s, o, 64);
            s *= scale;
            if (j < L) {
                if (dc == 0) ps[j] = s;
                lmax = fmaxf(lmax, s);
            }
        }
    }
    row_t vv[AU];
    ATT_LOAD(vv, vbase, 0, 1);  // in flight during the softmax reductions

    lmax = wave_max(lmax);
    if (lane == 0) red[wave] = lmax;
    __syncthreads();
    float gmax = red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) gmax = fmaxf(gmax, red[w]);
    float lsum = 0.f;
    for (int j = tid; j < L; j += NW * 64) {
        const float e = expf(ps[j] - gmax);
        ps[j] = e;
        lsum += e;
    }
    lsum = wave_sum(lsum);
    __syncthreads();
    if (lane == 0) red[wave] = lsum;
    __syncthreads();
    float tot = red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) tot += red[w];

    float acc[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
#pragma unroll 1
    for (int bi = 0; bi < nbatch; ++bi) {
        if (bi > 0) ATT_LOAD(vv, vbase, bi, 1);
#pragma unroll
        for (int u = 0; u < AU; ++u) {
            const int j = bi * BATCH + jw + u * NW * KPI;
            const float p = (j < L) ? ps[min(j, L - 1)] : 0.f;
            if constexpr (EPL == 4) {
                acc[0] += p * vv[u][0]; acc[1] += p * vv[u][1]; acc[2] += p * vv[u][2]; acc[3] += p * vv[u][3];
            } else {
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    acc[2 * w] += p * bf16_lo(vv[u][w]);
                    acc[2 * w + 1] += p * bf16_hi(vv[u][w]);
                }
            }
        }
    }
#undef ATT_LOAD
    // thread tid < D owns head dim tid = EPL * dd + comp: the sum over the waves, then the key slots, of that component
    const int dd = tid >> (EPL == 8 ? 3 : 2), comp = tid & (EPL - 1);
    // EPL / 4 rounds of 4 components (written out, not a loop over r: with one trip, the fp32 kernels compile to another schedule).
    // The barrier in front: pv is free once every wave is past its last read of the new row's words (APPENDS, r = 0) / of the previous round
#define ATT_REDUCE_ROUND(r)                                                                                                                    \
    {                                                                                                                                          \
        if (KV::APPENDS || r > 0) __syncthreads();                                                                                             \
        *reinterpret_cast<float4*>(pv + (wave * 64 + lane) * 4) = make_float4(acc[4 * r], acc[4 * r + 1], acc[4 * r + 2], acc[4 * r + 3]);     \
        __syncthreads();                                                                                                                       \
        if (tid < D && (comp >> 2) == r) {                                                                                                     \
            float o = 0.f;                                                                                                                     \
            for (int w = 0; w < NW; ++w)                                                                                                       \
                for (int s2 = 0; s2 < KPI; ++s2) o += pv[(w * 64 + s2 * LPK + dd) * 4 + (comp & 3)];                                           \
            st_act<COH>(out + (long)b * (H * D) + h * D + tid, o / tot);                                                                       \
        }                                                                                                                                      \
    }
    ATT_REDUCE_ROUND(0)
    if constexpr (EPL == 8) ATT_REDUCE_ROUND(1)
#undef ATT_REDUCE_ROUND
}

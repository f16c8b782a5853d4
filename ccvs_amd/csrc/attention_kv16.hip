// The token loop on a bfloat16 KV cache (include/ccvs_hip_kv16.h has the definition of the mode): append, the two attention forms and
// the launcher that the step's launch chain (gpt.hip, ccvs_gpt_decode_step_bf16kv) calls.  The fp32 kernels of gpt.hip are not touched:
// these are kernels of their own, the same algorithms on 16-bit cache rows.
#include <math.h>

#include "attention_kv16.h"
#include "common.h"

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
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
// Append: a lane rounds 8 consecutive head dims of one (row, position, head) of K and of V -- two 16-byte loads, one 16-byte store each.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kv_append_bf16_kernel(const float* __restrict__ k, const float* __restrict__ v, long sB, long ld,
                                                             uint16_t* __restrict__ kc, uint16_t* __restrict__ vc, long total, int H, int Tq,
                                                             int pos0, const int32_t* __restrict__ pos_dev, int Tmax, int D) {
    if (pos_dev) pos0 += *pos_dev;
    const int D8 = D >> 3;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int d8 = (int)(i % D8);
        long t = i / D8;
        const int h = (int)(t % H);
        t /= H;
        const int tq = (int)(t % Tq);
        const long b = t / Tq;
        if (pos0 + tq >= Tmax) continue;
        const long src = b * sB + tq * ld + h * D + 8 * d8;
        const long dst = ((b * H + h) * Tmax + pos0 + tq) * D + 8 * d8;
        const F32Quad k0 = *reinterpret_cast<const F32Quad*>(k + src), k1 = *reinterpret_cast<const F32Quad*>(k + src + 4);
        const F32Quad v0 = *reinterpret_cast<const F32Quad*>(v + src), v1 = *reinterpret_cast<const F32Quad*>(v + src + 4);
        const u32x4 kw = {bf16_rne2(k0.v[0], k0.v[1]), bf16_rne2(k0.v[2], k0.v[3]), bf16_rne2(k1.v[0], k1.v[1]), bf16_rne2(k1.v[2], k1.v[3])};
        const u32x4 vw = {bf16_rne2(v0.v[0], v0.v[1]), bf16_rne2(v0.v[2], v0.v[3]), bf16_rne2(v1.v[0], v1.v[1]), bf16_rne2(v1.v[2], v1.v[3])};
        *reinterpret_cast<u32x4*>(kc + dst) = kw;
        *reinterpret_cast<u32x4*>(vc + dst) = vw;
    }
}

extern "C" int ccvs_kv_append_bf16(const float* k, const float* v, int64_t sB, int64_t ld, void* kcache, void* vcache, int32_t B, int32_t H,
                                   int32_t Tq, int32_t pos0, const int32_t* pos_dev, int32_t Tmax, int32_t D, void* stream) {
    CCVS_REQUIRE(k && v && kcache && vcache, "ccvs_kv_append_bf16: null pointer");
    CCVS_REQUIRE(B > 0 && H > 0 && Tq > 0 && D > 0 && pos0 >= 0 && pos0 + Tq <= Tmax, "ccvs_kv_append_bf16: positions %d..%d exceed cache %d",
                 pos0, pos0 + Tq, Tmax);
    CCVS_REQUIRE(D % 8 == 0 && sB % 4 == 0 && ld % 4 == 0, "ccvs_kv_append_bf16: head dim %d must be a multiple of 8, the strides multiples of 4 floats", D);
    CCVS_REQUIRE(((uintptr_t)kcache | (uintptr_t)vcache | (uintptr_t)k | (uintptr_t)v) % 16 == 0, "ccvs_kv_append_bf16: k, v and the caches must be 16-byte aligned");
    const long total = (long)B * Tq * H * (D / 8);
    hipLaunchKernelGGL(kv_append_bf16_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, (hipStream_t)stream, k, v, (long)sB, (long)ld,
                       (uint16_t*)kcache, (uint16_t*)vcache, total, H, Tq, pos0, pos_dev, Tmax, D);
    CCVS_CHECK_LAUNCH("ccvs_kv_append_bf16");
    return CCVS_OK;
}

// ---------------------------------------------------------------------------------------
// Prefill form (Tq > 1): attention_prefill_kernel's algorithm (gpt.hip has the description: S^T = K Q^T and O^T += V^T P^T on
// v_mfma_f32_32x32x2_f32, online softmax in the log2 domain, two tile buffers, the output through LDS) on a bf16 cache.  What differs
// is the tile loader alone: a thread fetches 16 bytes = 8 head dims of a key row and of a value row and widens them while it stores
// them into the SAME fp32 LDS tile (K transposed to [d][key], V as [key][d]).  Rows >= pos0 + Tq: the address clamp plus the zero-fill.
// ---------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void attention_prefill_bf16_kernel(const float* __restrict__ q, long q_sB, long ldq,
                                                                     const uint16_t* __restrict__ kc, const uint16_t* __restrict__ vc,
                                                                     float* __restrict__ out, int H, int Tq, int pos0,
                                                                     const int32_t* __restrict__ pos_dev, int Tmax, float scale) {
    constexpr int MT = (D + 31) / 32;   // 32-row tiles of the head dimension in O^T
    constexpr int DP = MT * 32;         // head dimension padded to the tile (zero columns of V)
    constexpr int DK = D / 2;           // MFMA steps of S (K = 2 per step)
    constexpr int KS = 33;              // row stride of the transposed K tile
    constexpr int F8 = D / 8;           // 16-byte units per cache row
    constexpr int NLD = (32 * F8 + 255) / 256;  // units per thread and tile (1)
    constexpr int TILE_WORDS = D * KS + 32 * DP;
    constexpr int OUT_WORDS = 128 * (D + 1);
    constexpr int SMEM_WORDS = 2 * TILE_WORDS > OUT_WORDS ? 2 * TILE_WORDS : OUT_WORDS;
    __shared__ __attribute__((aligned(16))) float smem[SMEM_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qi = lane & 31, half = lane >> 5;
    const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
    if (pos_dev) pos0 += *pos_dev;
    const int q0 = (gridDim.y - 1 - blockIdx.y) * 128;     // first query of the workgroup (the longest blocks start first)
    const int qw = q0 + wave * 32;                         // first query of the wave
    const int qidx = qw + qi;                              // this lane's query
    const int q_last_wg = min(q0 + 127, Tq - 1), q_last_w = min(qw + 31, Tq - 1);
    const int ntiles = (min(pos0 + q_last_wg + 1, Tmax) + 31) >> 5;
    const uint16_t* kbase = kc + (long)bh * Tmax * D;
    const uint16_t* vbase = vc + (long)bh * Tmax * D;

    float qreg[DK];
    {
        const float* qp = q + (long)b * q_sB + (long)min(qidx, Tq - 1) * ldq + h * D + half;
#pragma unroll
        for (int i = 0; i < DK; ++i) qreg[i] = (qidx < Tq) ? qp[2 * i] * (scale * 1.44269504088896340736f) : 0.f;
    }
    if (MT * 32 > D) {  // zero the padding columns of both V buffers once (D = 16)
        for (int e = tid; e < 2 * 32 * (DP - D); e += 256) {
            const int bsel = e / (32 * (DP - D)), r = e - bsel * 32 * (DP - D);
            smem[bsel * TILE_WORDS + D * KS + (r / (DP - D)) * DP + D + r % (DP - D)] = 0.f;
        }
    }

    u32x4 kreg[NLD], vreg[NLD];
    auto fetch = [&](int kt) {
#pragma unroll
        for (int r = 0; r < NLD; ++r) {
            const int e = min(tid + 256 * r, 32 * F8 - 1);
            const int key = e / F8, d8 = e - key * F8;
            // rows >= pos0 + Tq have never been written: staged as zeros (bf16 0 widens to 0.f) and never read (the address is clamped)
            const bool written = kt * 32 + key < pos0 + Tq;
            const long row = min(kt * 32 + key, pos0 + Tq - 1);
            const u32x4 kv = *reinterpret_cast<const u32x4*>(kbase + row * D + 8 * d8);
            const u32x4 vv = *reinterpret_cast<const u32x4*>(vbase + row * D + 8 * d8);
            const u32x4 zero = {0u, 0u, 0u, 0u};
            kreg[r] = written ? kv : zero;
            vreg[r] = written ? vv : zero;
        }
    };
    auto stash = [&](int buf) {
        float* kt_s = smem + buf * TILE_WORDS;
        float* v_s = kt_s + D * KS;
#pragma unroll
        for (int r = 0; r < NLD; ++r) {
            const int e = tid + 256 * r;
            if (e < 32 * F8) {
                const int key = e / F8, d8 = e - key * F8;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    kt_s[(8 * d8 + 2 * w + 0) * KS + key] = bf16_lo(kreg[r][w]);
                    kt_s[(8 * d8 + 2 * w + 1) * KS + key] = bf16_hi(kreg[r][w]);
                }
                *reinterpret_cast<float4*>(v_s + key * DP + 8 * d8) =
                    make_float4(bf16_lo(vreg[r][0]), bf16_hi(vreg[r][0]), bf16_lo(vreg[r][1]), bf16_hi(vreg[r][1]));
                *reinterpret_cast<float4*>(v_s + key * DP + 8 * d8 + 4) =
                    make_float4(bf16_lo(vreg[r][2]), bf16_hi(vreg[r][2]), bf16_lo(vreg[r][3]), bf16_hi(vreg[r][3]));
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

// ---------------------------------------------------------------------------------------
// Decode form (Tq = 1): attention_decode_item's algorithm (gpt.hip) on a bf16 cache, with the append of the current position inside.
// One workgroup per (row, head) streams that head's K rows, then its V rows, once, with non-temporal loads.
// Lane map: a lane owns EPL = KV16_DECODE_EPL consecutive head dims of one key slot -- EPL = 8: one 16-byte load per row and lane,
// D/8 lanes per row (the width the HBM-bound streams of this library use), EPL = 4: 8 bytes, D/4 lanes per row as in the fp32 kernel.
// A wave-instruction covers 64 / (D/EPL) whole rows; AU = 32 / EPL rows per lane are requested together, so 16 KB are in flight per
// workgroup as in the fp32 kernel, and BATCH = 4 waves x rows per instruction x AU = 8192 / D rows for either EPL.  The partial dots
// are summed across the lanes of a row with xor shuffles; scores[Tmax] stay in LDS; the key slots of a wave and the 4 waves are
// reduced through LDS in a fixed order (wave, then slot), EPL / 4 rounds through the SAME 4 KB.
// THE APPEND (k_new != NULL): the lanes of slot 0 of wave 0 round the new K and V rows, store them at position L - 1 and leave the same
// words in LDS; every lane takes them from there in place of whatever a load of a row >= L - 1 returned (row L - 1 itself and the
// clamped tail of the last batch): the stored bits and the used bits are the same words, and nothing read depends on the store.
// Exactly one workgroup owns a (row, head), so no other workgroup reads or writes that cache row in this launch.
// Footprint: 256 threads, LDS = scores + 4 KB + 64 B; registers: see DESIGN.md 4.28.
// ---------------------------------------------------------------------------------------
#ifndef KV16_DECODE_EPL
#define KV16_DECODE_EPL 8
#endif

template <int EPL> struct Kv16Words;
template <> struct Kv16Words<8> { typedef u32x4 type; };
template <> struct Kv16Words<4> { typedef u32x2 type; };

template <int D, int EPL>
__global__ __launch_bounds__(256) void attention_decode_bf16_kernel(const float* __restrict__ q, long q_sB, const float* __restrict__ k_new,
                                                                    const float* __restrict__ v_new, long kv_sB, uint16_t* __restrict__ kc,
                                                                    uint16_t* __restrict__ vc, float* __restrict__ out, int H, int pos0,
                                                                    const int32_t* __restrict__ pos_dev, int grp_rows, int Tmax, float scale) {
    typedef typename Kv16Words<EPL>::type words_t;
    constexpr int NWD = EPL / 2;     // 32-bit words per lane and row
    constexpr int LPK = D / EPL;     // lanes per key row
    constexpr int KPI = 64 / LPK;    // key rows per wave-instruction
    constexpr int NW = 4;
    constexpr int AU = 32 / EPL;     // key rows per lane whose loads are issued together
    constexpr int BATCH = NW * KPI * AU;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* red = smem;                    // [16]
    float* pv = smem + 16;                // [NW][64][4]
    float* ps = smem + 16 + NW * 256;     // [Tmax]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
    if (pos_dev) pos0 += pos_dev[grp_rows > 0 ? b / grp_rows : 0];   // row groups of a decode step: one cache length per group
    pos0 = max(pos0, 0);   // (a negative device-resident position: no caller's contract, and no address below row 0)
    const int L = min(pos0 + 1, Tmax);
    const bool append = k_new != nullptr && pos0 < Tmax;
    const int kk = lane / LPK, dc = lane - kk * LPK;
    // (a workgroup-uniform base plus a 32-bit element offset per lane: one address register per load in flight instead of two)
    uint16_t* kbase = kc + (long)bh * Tmax * D;
    uint16_t* vbase = vc + (long)bh * Tmax * D;
    const unsigned doff = EPL * dc;
    unsigned* fresh_s = reinterpret_cast<unsigned*>(pv);   // [2][D / 2] words: the rounded new K row, then V (pv is free until the end)
    const int jw = wave * KPI + kk;  // this lane's row within a batch, + u * NW * KPI
    const int nbatch = (L + BATCH - 1) / BATCH;

    float qv[EPL];
#pragma unroll
    for (int e = 0; e < EPL; e += 4) {
        const float4 t = *reinterpret_cast<const float4*>(q + (long)b * q_sB + h * D + EPL * dc + e);
        qv[e] = t.x; qv[e + 1] = t.y; qv[e + 2] = t.z; qv[e + 3] = t.w;
    }
    if (append && wave == 0 && kk == 0) {
        words_t k_fresh, v_fresh;
        const float* kn = k_new + (long)b * kv_sB + h * D + EPL * dc;
        const float* vn = v_new + (long)b * kv_sB + h * D + EPL * dc;
#pragma unroll
        for (int e = 0; e < EPL; e += 4) {
            const float4 a = *reinterpret_cast<const float4*>(kn + e), c = *reinterpret_cast<const float4*>(vn + e);
            k_fresh[e / 2] = bf16_rne2(a.x, a.y); k_fresh[e / 2 + 1] = bf16_rne2(a.z, a.w);
            v_fresh[e / 2] = bf16_rne2(c.x, c.y); v_fresh[e / 2 + 1] = bf16_rne2(c.z, c.w);
        }
        *reinterpret_cast<words_t*>(kbase + (unsigned)((L - 1) * D) + doff) = k_fresh;
        *reinterpret_cast<words_t*>(vbase + (unsigned)((L - 1) * D) + doff) = v_fresh;
        *reinterpret_cast<words_t*>(fresh_s + NWD * dc) = k_fresh;
        *reinterpret_cast<words_t*>(fresh_s + D / 2 + NWD * dc) = v_fresh;
    }
    __syncthreads();   // the rounded row is in LDS for every wave
    // unconditional loads from clamped rows (predicated loads would serialise)
#define KV16_LOAD(dst, base, bi, fresh)                                                                                                  \
    _Pragma("unroll") for (int u = 0; u < AU; ++u) {                                                                                     \
        const int j_ = (bi) * BATCH + jw + u * NW * KPI;                                                                                 \
        dst[u] = __builtin_nontemporal_load(reinterpret_cast<const words_t*>(base + (unsigned)(min(j_, L - 1) * D) + doff));             \
        if (append && j_ >= L - 1) dst[u] = *reinterpret_cast<const words_t*>(fresh_s + (fresh) + NWD * dc);                             \
    }

    float lmax = -INFINITY;
#pragma unroll 1   // one batch of AU rows in flight per lane: the register budget
    for (int bi = 0; bi < nbatch; ++bi) {
        words_t kv[AU];
        KV16_LOAD(kv, kbase, bi, 0);
#pragma unroll
        for (int u = 0; u < AU; ++u) {
            const int j = bi * BATCH + jw + u * NW * KPI;
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < NWD; ++w) {
                s += bf16_lo(kv[u][w]) * qv[2 * w];
                s += bf16_hi(kv[u][w]) * qv[2 * w + 1];
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
    words_t vv[AU];
    KV16_LOAD(vv, vbase, 0, D / 2);  // in flight during the softmax reductions

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
        if (bi > 0) KV16_LOAD(vv, vbase, bi, D / 2);
#pragma unroll
        for (int u = 0; u < AU; ++u) {
            const int j = bi * BATCH + jw + u * NW * KPI;
            const float p = (j < L) ? ps[min(j, L - 1)] : 0.f;
#pragma unroll
            for (int w = 0; w < NWD; ++w) {
                acc[2 * w] += p * bf16_lo(vv[u][w]);
                acc[2 * w + 1] += p * bf16_hi(vv[u][w]);
            }
        }
    }
#undef KV16_LOAD
    // thread tid < D owns head dim tid = EPL * dd + comp: the sum over the waves, then the key slots, of that component
    const int dd = tid / EPL, comp = tid - dd * EPL;
#pragma unroll
    for (int r = 0; r < EPL / 4; ++r) {
        __syncthreads();   // pv is free: every wave is past its last read of the new row's words (r = 0) / of the previous round
        *reinterpret_cast<float4*>(pv + (wave * 64 + lane) * 4) = make_float4(acc[4 * r], acc[4 * r + 1], acc[4 * r + 2], acc[4 * r + 3]);
        __syncthreads();
        if (tid < D && (comp >> 2) == r) {
            float o = 0.f;
            for (int w = 0; w < NW; ++w)
                for (int s2 = 0; s2 < KPI; ++s2) o += pv[(w * 64 + s2 * LPK + dd) * 4 + (comp & 3)];
            out[(long)b * (H * D) + h * D + tid] = o / tot;
        }
    }
}

void ccvs_kv16_launch_attention_decode(int D, int n_bh, size_t smem, hipStream_t st, const float* q, long q_sB, const float* k_new,
                                       const float* v_new, long kv_sB, uint16_t* kc, uint16_t* vc, float* out, int H, int pos0,
                                       const int32_t* pos_dev, int grp_rows, int Tmax, float scale) {
#define KV16_DECODE_LAUNCH(Dv)                                                                                                       \
    hipLaunchKernelGGL((attention_decode_bf16_kernel<Dv, KV16_DECODE_EPL>), dim3((unsigned)n_bh), dim3(256), smem, st, q, q_sB, k_new, v_new, \
                       kv_sB, kc, vc, out, H, pos0, pos_dev, grp_rows, Tmax, scale)
    if (D == 64) KV16_DECODE_LAUNCH(64);
    else if (D == 32) KV16_DECODE_LAUNCH(32);
    else KV16_DECODE_LAUNCH(16);
#undef KV16_DECODE_LAUNCH
}

extern "C" int ccvs_attention_bf16(const float* q, int64_t q_sB, int64_t ldq, const float* k_new, const float* v_new, int64_t kv_sB,
                                   void* kcache, void* vcache, float* out, int32_t B, int32_t H, int32_t Tq, int32_t pos0,
                                   const int32_t* pos_dev, int32_t grp_rows, int32_t Tmax, int32_t D, void* stream) {
    CCVS_REQUIRE(q && kcache && vcache && out, "ccvs_attention_bf16: null pointer");
    CCVS_REQUIRE(D == 64 || D == 32 || D == 16, "ccvs_attention_bf16: head dim %d unsupported (16, 32, 64)", D);
    CCVS_REQUIRE(B > 0 && H > 0 && Tq > 0 && pos0 >= 0 && pos0 + Tq <= Tmax, "ccvs_attention_bf16: bad positions");
    CCVS_REQUIRE(cdiv(Tq, 128) <= 65535, "ccvs_attention_bf16: %d queries too many for one launch", Tq);
    CCVS_REQUIRE((k_new != nullptr) == (v_new != nullptr), "ccvs_attention_bf16: one new row without the other");
    CCVS_REQUIRE(grp_rows == 0 || (grp_rows > 0 && Tq == 1 && pos_dev && B % grp_rows == 0),
                 "ccvs_attention_bf16: row groups (%d rows each) need the decode form, a device-resident position per group and B %% grp_rows == 0", grp_rows);
    CCVS_REQUIRE(!k_new || Tq == 1, "ccvs_attention_bf16: the appending form is the decode form (Tq = 1), got Tq = %d", Tq);
    CCVS_REQUIRE(((uintptr_t)kcache | (uintptr_t)vcache) % 16 == 0, "ccvs_attention_bf16: caches must be 16-byte aligned");
    const float scale = 1.0f / sqrtf((float)D);
    hipStream_t st = (hipStream_t)stream;
    uint16_t* kc = (uint16_t*)kcache;
    uint16_t* vc = (uint16_t*)vcache;
    if (Tq == 1) {
        CCVS_REQUIRE(q_sB % 4 == 0 && (uintptr_t)q % 16 == 0, "ccvs_attention_bf16: q must be 16-byte aligned, its stride a multiple of 4 floats");
        CCVS_REQUIRE(!k_new || (kv_sB % 4 == 0 && ((uintptr_t)k_new | (uintptr_t)v_new) % 16 == 0),
                     "ccvs_attention_bf16: the new rows must be 16-byte aligned, their stride a multiple of 4 floats");
        // with a device-side position the visible length is unknown to the host: size LDS for the whole cache
        const int maxL = pos_dev ? Tmax : pos0 + 1;
        const size_t smem = (size_t)(16 + 4 * 256 + maxL) * sizeof(float);
        CCVS_REQUIRE(smem <= 64 * 1024, "ccvs_attention_bf16: sequence too long for the LDS score buffer");
        ccvs_kv16_launch_attention_decode(D, B * H, smem, st, q, (long)q_sB, k_new, v_new, (long)kv_sB, kc, vc, out, H, pos0, pos_dev, grp_rows, Tmax, scale);
    } else {
        const dim3 grid((unsigned)(B * H), (unsigned)cdiv(Tq, 128));
#define KV16_PREFILL_LAUNCH(Dv) \
    hipLaunchKernelGGL((attention_prefill_bf16_kernel<Dv>), grid, dim3(256), 0, st, q, (long)q_sB, (long)ldq, kc, vc, out, H, Tq, pos0, pos_dev, Tmax, scale)
        if (D == 64) KV16_PREFILL_LAUNCH(64);
        else if (D == 32) KV16_PREFILL_LAUNCH(32);
        else KV16_PREFILL_LAUNCH(16);
#undef KV16_PREFILL_LAUNCH
    }
    CCVS_CHECK_LAUNCH("ccvs_attention_bf16");
    return CCVS_OK;
}

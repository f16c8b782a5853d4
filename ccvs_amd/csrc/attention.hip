// KV cache append and causal attention over the cache, fp32 and bfloat16 (attention_core.h has the kernels' bodies and the cache-row
// policies; include/ccvs_hip_kv16.h the definition of the bf16 mode): the two append kernels, the kernels' instantiations, their
// launchers and the four entries.
// Reference: models/skip_vid_generator/models/mingpt.py:33-117.
#include "attention.h"
#include "attention_core.h"

// ---------------------------------------------------------------------------------------
// Append.  fp32: a copy, one element per lane and step.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kv_append_kernel(const float* __restrict__ k, const float* __restrict__ v, long sB, long ld,
                                                        float* __restrict__ kc, float* __restrict__ vc, long total, int H, int Tq,
                                                        int pos0, const int32_t* __restrict__ pos_dev, int Tmax, int D) {
    if (pos_dev) pos0 += *pos_dev;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int d = (int)(i % D);
        long t = i / D;
        const int h = (int)(t % H);
        t /= H;
        const int tq = (int)(t % Tq);
        const long b = t / Tq;
        if (pos0 + tq >= Tmax) continue;
        const long src = b * sB + tq * ld + h * D + d;
        const long dst = ((b * H + h) * Tmax + pos0 + tq) * D + d;
        kc[dst] = k[src];
        vc[dst] = v[src];
    }
}

extern "C" int ccvs_kv_append(const float* k, const float* v, int64_t sB, int64_t ld, float* kcache, float* vcache, int32_t B, int32_t H,
                              int32_t Tq, int32_t pos0, const int32_t* pos_dev, int32_t Tmax, int32_t D, void* stream) {
    CCVS_REQUIRE(k && v && kcache && vcache, "ccvs_kv_append: null pointer");
    CCVS_REQUIRE(B > 0 && H > 0 && Tq > 0 && D > 0 && pos0 >= 0 && pos0 + Tq <= Tmax, "ccvs_kv_append: positions %d..%d exceed cache %d",
                 pos0, pos0 + Tq, Tmax);
    const long total = (long)B * Tq * H * D;
    hipLaunchKernelGGL(kv_append_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, (hipStream_t)stream, k, v, (long)sB, (long)ld, kcache,
                       vcache, total, H, Tq, pos0, pos_dev, Tmax, D);
    CCVS_CHECK_LAUNCH("ccvs_kv_append");
    return CCVS_OK;
}

// bf16: a lane rounds 8 consecutive head dims of one (row, position, head) of K and of V -- two 16-byte loads, one 16-byte store each.
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
// The decode kernels: attention_decode_item per workgroup.  The two differ in their arguments alone (the new rows of the appending form).
// ---------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void attention_decode_kernel(const float* __restrict__ q, long q_sB, const float* __restrict__ kc,
                                                               const float* __restrict__ vc, float* __restrict__ out, int H, int pos0,
                                                               const int32_t* __restrict__ pos_dev, int grp_rows, int Tmax, float scale) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    attention_decode_item<D, KvF32, false>(q, q_sB, nullptr, nullptr, 0, kc, vc, out, H, pos0, pos_dev, grp_rows, Tmax, scale, blockIdx.x, smem);
}

template <int D>
__global__ __launch_bounds__(256) void attention_decode_bf16_kernel(const float* __restrict__ q, long q_sB, const float* __restrict__ k_new,
                                                                    const float* __restrict__ v_new, long kv_sB, uint16_t* __restrict__ kc,
                                                                    uint16_t* __restrict__ vc, float* __restrict__ out, int H, int pos0,
                                                                    const int32_t* __restrict__ pos_dev, int grp_rows, int Tmax, float scale) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    attention_decode_item<D, KvBf16, false>(q, q_sB, k_new, v_new, kv_sB, kc, vc, out, H, pos0, pos_dev, grp_rows, Tmax, scale, blockIdx.x, smem);
}

// one launch ladder per form; KV = KvF32 / KvBf16 selects the cache type
#define ATT_FOR_D(LAUNCH)        \
    do {                         \
        if (D == 64) LAUNCH(64); \
        else if (D == 32) LAUNCH(32); \
        else LAUNCH(16);         \
    } while (0)

template <class KV>
static void launch_decode(int D, int n_bh, size_t smem, hipStream_t st, const float* q, long q_sB, const float* k_new, const float* v_new,
                          long kv_sB, typename KV::cache_t kc, typename KV::cache_t vc, float* out, int H, int pos0, const int32_t* pos_dev,
                          int grp_rows, int Tmax, float scale) {
#define ATT_DECODE_LAUNCH(Dv)                                                                                                                      \
    do {                                                                                                                                           \
        if constexpr (KV::APPENDS)                                                                                                                 \
            hipLaunchKernelGGL((attention_decode_bf16_kernel<Dv>), dim3((unsigned)n_bh), dim3(256), smem, st, q, q_sB, k_new, v_new, kv_sB, kc, vc, \
                               out, H, pos0, pos_dev, grp_rows, Tmax, scale);                                                                      \
        else                                                                                                                                       \
            hipLaunchKernelGGL((attention_decode_kernel<Dv>), dim3((unsigned)n_bh), dim3(256), smem, st, q, q_sB, kc, vc, out, H, pos0, pos_dev,   \
                               grp_rows, Tmax, scale);                                                                                             \
    } while (0)
    ATT_FOR_D(ATT_DECODE_LAUNCH);
#undef ATT_DECODE_LAUNCH
}

void ccvs_launch_attention_decode(bool bf16, int D, int n_bh, size_t smem, hipStream_t st, const float* q, long q_sB, const float* k_new,
                                  const float* v_new, long kv_sB, void* kc, void* vc, float* out, int H, int pos0, const int32_t* pos_dev,
                                  int grp_rows, int Tmax, float scale) {
    if (bf16)
        launch_decode<KvBf16>(D, n_bh, smem, st, q, q_sB, k_new, v_new, kv_sB, (uint16_t*)kc, (uint16_t*)vc, out, H, pos0, pos_dev, grp_rows, Tmax, scale);
    else
        launch_decode<KvF32>(D, n_bh, smem, st, q, q_sB, nullptr, nullptr, 0, (const float*)kc, (const float*)vc, out, H, pos0, pos_dev, grp_rows, Tmax, scale);
}

template <class KV>
static void launch_prefill(int D, int n_bh, hipStream_t st, const float* q, long q_sB, long ldq, const typename KV::elem_t* kc,
                           const typename KV::elem_t* vc, float* out, int H, int Tq, int pos0, const int32_t* pos_dev, int Tmax, float scale) {
    const dim3 grid((unsigned)n_bh, (unsigned)cdiv(Tq, 128));
#define ATT_PREFILL_LAUNCH(Dv) \
    hipLaunchKernelGGL((attention_prefill_kernel<Dv, KV>), grid, dim3(256), 0, st, q, q_sB, ldq, kc, vc, out, H, Tq, pos0, pos_dev, Tmax, scale)
    ATT_FOR_D(ATT_PREFILL_LAUNCH);
#undef ATT_PREFILL_LAUNCH
}

// the argument checks that ccvs_attention and ccvs_attention_bf16 share, under the entry's own name
static int attention_check(const char* who, const void* q, const void* kcache, const void* vcache, const void* out, int B, int H, int Tq,
                           int pos0, int Tmax, int D) {
    CCVS_REQUIRE(q && kcache && vcache && out, "%s: null pointer", who);
    CCVS_REQUIRE(D == 64 || D == 32 || D == 16, "%s: head dim %d unsupported (16, 32, 64)", who, D);
    CCVS_REQUIRE(B > 0 && H > 0 && Tq > 0 && pos0 >= 0 && pos0 + Tq <= Tmax, "%s: bad positions", who);
    CCVS_REQUIRE(cdiv(Tq, 128) <= 65535, "%s: %d queries too many for one launch", who, Tq);
    return CCVS_OK;
}
// LDS of the decode form at position pos0 (+ *pos_dev); refused beyond 64 KB
static int attention_decode_lds(const char* who, int pos0, const int32_t* pos_dev, int Tmax, size_t* smem) {
    // with a device-side position the visible length is unknown to the host: size LDS for the whole cache
    const int maxL = pos_dev ? Tmax : pos0 + 1;
    *smem = (size_t)(16 + 4 * 256 + maxL) * sizeof(float);
    CCVS_REQUIRE(*smem <= 64 * 1024, "%s: sequence too long for the LDS score buffer", who);
    return CCVS_OK;
}

extern "C" int ccvs_attention(const float* q, int64_t q_sB, int64_t ldq, const float* kcache, const float* vcache, float* out, int32_t B,
                              int32_t H, int32_t Tq, int32_t pos0, const int32_t* pos_dev, int32_t Tmax, int32_t D, void* stream) {
    int rc = attention_check("ccvs_attention", q, kcache, vcache, out, B, H, Tq, pos0, Tmax, D);
    if (rc != CCVS_OK) return rc;
    const float scale = 1.0f / sqrtf((float)D);
    hipStream_t st = (hipStream_t)stream;
    if (Tq == 1) {
        size_t smem;
        if ((rc = attention_decode_lds("ccvs_attention", pos0, pos_dev, Tmax, &smem)) != CCVS_OK) return rc;
        launch_decode<KvF32>(D, B * H, smem, st, q, (long)q_sB, nullptr, nullptr, 0, kcache, vcache, out, H, pos0, pos_dev, 0, Tmax, scale);
    } else {
        launch_prefill<KvF32>(D, B * H, st, q, (long)q_sB, (long)ldq, kcache, vcache, out, H, Tq, pos0, pos_dev, Tmax, scale);
    }
    CCVS_CHECK_LAUNCH("ccvs_attention");
    return CCVS_OK;
}

extern "C" int ccvs_attention_bf16(const float* q, int64_t q_sB, int64_t ldq, const float* k_new, const float* v_new, int64_t kv_sB,
                                   void* kcache, void* vcache, float* out, int32_t B, int32_t H, int32_t Tq, int32_t pos0,
                                   const int32_t* pos_dev, int32_t grp_rows, int32_t Tmax, int32_t D, void* stream) {
    int rc = attention_check("ccvs_attention_bf16", q, kcache, vcache, out, B, H, Tq, pos0, Tmax, D);
    if (rc != CCVS_OK) return rc;
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
        size_t smem;
        if ((rc = attention_decode_lds("ccvs_attention_bf16", pos0, pos_dev, Tmax, &smem)) != CCVS_OK) return rc;
        launch_decode<KvBf16>(D, B * H, smem, st, q, (long)q_sB, k_new, v_new, (long)kv_sB, kc, vc, out, H, pos0, pos_dev, grp_rows, Tmax, scale);
    } else {
        launch_prefill<KvBf16>(D, B * H, st, q, (long)q_sB, (long)ldq, kc, vc, out, H, Tq, pos0, pos_dev, Tmax, scale);
    }
    CCVS_CHECK_LAUNCH("ccvs_attention_bf16");
    return CCVS_OK;
}

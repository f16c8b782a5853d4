// The decoder's motion export (include/ccvs_hip_flowviz.h): the last InterBlock's (flow | occ) rows of a new
// frame -> one slot of the clip's motion buffer [B, T, 3, H, W] (flow in pixels towards context 0, the fused occlusion mask), the
// per-clip largest flow magnitude, and the buffer rendered as two uint8 clips (the reference's get_flow_rgb colours, tools/logger.py:95-103,
// with its radius a parameter; the mask as grey).  All three are HBM-bound passes: four consecutive pixels per lane, 16-byte loads and
// stores wherever the four lie in one plane (dword-aligned wide accesses, common.h), scalar access for the ragged tail of a plane.
//
// ccvs_flow_export <- skip_autoencoder.py:255-263 (confs, occ, occ_mask) on the rows of one frame
// ccvs_flow_render <- tools/logger.py:95-103 get_flow_rgb, boost = sqrt(2) / max_px
#include <math.h>
#include "common.h"

#define FV_PI 3.14159274101257324f   // (float) pi, the divisor of torch's fp32 `atan2(...) / np.pi`

__device__ __forceinline__ float fv_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// four consecutive floats of a dense plane from p; the tail of a plane (nv < 4) one by one, the rest zero
__device__ __forceinline__ void fv_load4(const float* p, int nv, float (&v)[4]) {
    if (nv == 4) {
        const F32Quad q = *reinterpret_cast<const F32Quad*>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = q.v[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < nv ? p[j] : 0.f;
    }
}
__device__ __forceinline__ void fv_store4(float* p, int nv, const float (&v)[4]) {
    if (nv == 4) {
        F32Quad q;
#pragma unroll
        for (int j = 0; j < 4; ++j) q.v[j] = v[j];
        *reinterpret_cast<F32Quad*>(p) = q;
    } else {
        for (int j = 0; j < nv; ++j) p[j] = v[j];
    }
}

struct FlowExportK {
    const float* fo;
    float* out;
    long fo_sN, out_sB, items;
    int k, HW, quads;   // quads: items of four pixels per clip
    float mult;
};

__global__ __launch_bounds__(256) void flow_export_kernel(FlowExportK p) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.items; i += (long)gridDim.x * 256) {
        const long b = i / p.quads;
        const int p0 = (int)(i - b * p.quads) * 4;
        const int nv = min(4, p.HW - p0);
        const float* row0 = p.fo + b * p.k * p.fo_sN + p0;
        float* o = p.out + b * p.out_sB + p0;
        float fx[4], fy[4], occ[4];
        fv_load4(row0, nv, fx);
        fv_load4(row0 + p.HW, nv, fy);
        fv_load4(row0 + 2 * (long)p.HW, nv, occ);
        if (p.k > 1) {   // the confidence-weighted mean of the k logits (skip_autoencoder.py:256-259)
            float num[4], den[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float c = 1.f - fv_sigmoid(occ[j]) + 1e-6f;
                num[j] = occ[j] * c;
                den[j] = c;
            }
            for (int r = 1; r < p.k; ++r) {
                float oj[4];
                fv_load4(row0 + r * p.fo_sN + 2 * (long)p.HW, nv, oj);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float c = 1.f - fv_sigmoid(oj[j]) + 1e-6f;
                    num[j] += oj[j] * c;
                    den[j] += c;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) occ[j] = num[j] / den[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            fx[j] *= p.mult;
            fy[j] *= p.mult;
            occ[j] = fv_sigmoid(occ[j]);
        }
        fv_store4(o, nv, fx);
        fv_store4(o + p.HW, nv, fy);
        fv_store4(o + 2 * (long)p.HW, nv, occ);
    }
}

extern "C" int ccvs_flow_export(const float* fo, int64_t fo_sN, int32_t B, int32_t k, int32_t H, int32_t W, float flow_mult, float* out,
                                int64_t out_sB, void* stream) {
    CCVS_REQUIRE(fo && out, "ccvs_flow_export: null pointer");
    CCVS_REQUIRE(B > 0 && H > 0 && W > 0 && (long)H * W <= (1L << 28), "ccvs_flow_export: bad shape %d x %d x %d", B, H, W);
    CCVS_REQUIRE(k >= 1 && k <= CCVS_MAX_CTX, "ccvs_flow_export: %d contexts (1 .. %d)", k, CCVS_MAX_CTX);
    CCVS_REQUIRE(fo_sN >= 3L * H * W && out_sB >= 3L * H * W, "ccvs_flow_export: a stride shorter than the three planes");
    FlowExportK p;
    p.fo = fo; p.out = out; p.fo_sN = fo_sN; p.out_sB = out_sB; p.k = k; p.HW = H * W; p.quads = cdiv(H * W, 4); p.mult = flow_mult;
    p.items = (long)B * p.quads;
    hipLaunchKernelGGL(flow_export_kernel, dim3(strided_grid(p.items, stream, 8)), dim3(256), 0, (hipStream_t)stream, p);
    CCVS_CHECK_LAUNCH("ccvs_flow_export");
    return CCVS_OK;
}

// |f| as the fp32 mirror computes it: every step rounded on its own
__device__ __forceinline__ float fv_mag(float fx, float fy) {
#pragma clang fp contract(off)
    const float xx = fx * fx, yy = fy * fy;
    return sqrtf(xx + yy);
}

struct FlowMaxK {
    const float* m;
    unsigned* out;
    long sB, sT, per_clip;   // per_clip: T * HW pixels
    int HW;
};

#define FV_MAX_TILES 8   // 1024-pixel tiles per workgroup: one atomic per 8192 pixels

// Workgroup (bx, b) takes 8 x 1024 consecutive pixels of clip b, four per lane and tile; the workgroup's maximum (wave shuffles, then
// LDS) goes into out[b] as an integer maximum on the bits of a non-negative float, whose order is the floats' order: no float atomics,
// the same bits in any order.
__global__ __launch_bounds__(256) void flow_max_kernel(FlowMaxK p, GridWalk gw) {
    __shared__ float wave_mx[256 / WAVE];
    GRID_WALK_BEGIN(gw, bx, b, bz)
    (void)bz;
    const float* clip = p.m + b * p.sB;
    float mx = 0.f;
    for (int tile = 0; tile < FV_MAX_TILES; ++tile) {
        const long j0 = (((long)bx * FV_MAX_TILES + tile) * 256 + threadIdx.x) * 4;
        if (j0 >= p.per_clip) break;
        const long t = j0 / p.HW;
        const int px = (int)(j0 - t * p.HW);
        float fx[4], fy[4];
        int nv = 4;
        if (px + 3 < p.HW) {
            const float* f = clip + t * p.sT + px;
            fv_load4(f, 4, fx);
            fv_load4(f + p.HW, 4, fy);
        } else {   // the four pixels straddle two frames, or the clip ends: one by one
            nv = (int)min(4L, p.per_clip - j0);
            for (int j = 0; j < 4; ++j) {
                fx[j] = fy[j] = 0.f;
                if (j < nv) {
                    const long tj = (j0 + j) / p.HW;
                    const float* f = clip + tj * p.sT + (j0 + j - tj * p.HW);
                    fx[j] = f[0];
                    fy[j] = f[p.HW];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float mag = fv_mag(fx[j], fy[j]);
            if (j < nv && mag < INFINITY) mx = fmaxf(mx, mag);   // (NaN compares false)
        }
    }
    mx = wave_max(mx);
    if ((threadIdx.x & (WAVE - 1)) == 0) wave_mx[threadIdx.x / WAVE] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int v = 1; v < 256 / WAVE; ++v) mx = fmaxf(mx, wave_mx[v]);
        if (mx > 0.f) atomicMax(p.out + b, __float_as_uint(mx));
    }
    __syncthreads();   // persistent walk: wave_mx is written again
    GRID_WALK_END
}

extern "C" int ccvs_flow_max(const float* motion, int64_t sB, int64_t sT, int32_t B, int32_t T, int32_t H, int32_t W, float* out, void* stream) {
    CCVS_REQUIRE(motion && out, "ccvs_flow_max: null pointer");
    CCVS_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0 && (long)H * W <= (1L << 28) && (long)T * H * W <= (1L << 40), "ccvs_flow_max: bad shape %d x %d x %d x %d", B, T, H, W);
    CCVS_REQUIRE(sT >= 3L * H * W && sB >= 3L * H * W, "ccvs_flow_max: a stride shorter than the three planes");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(out, 0, sizeof(float) * B, st) != hipSuccess) {
        ccvs_set_error("ccvs_flow_max: clearing the output failed");
        return CCVS_ERR_LAUNCH;
    }
    FlowMaxK p;
    p.m = motion; p.out = reinterpret_cast<unsigned*>(out); p.sB = sB; p.sT = sT; p.HW = H * W; p.per_clip = (long)T * H * W;
    const long tiles = cdiv64(p.per_clip, 1024 * FV_MAX_TILES);
    CCVS_REQUIRE(tiles <= 0x7fffffffL, "ccvs_flow_max: clip too long");
    const GridWalk gw = grid_walk(tiles, B, 1);
    hipLaunchKernelGGL(flow_max_kernel, dim3(limited_grid(gw.total, stream, 8)), dim3(256), 0, st, p, gw);
    CCVS_CHECK_LAUNCH("ccvs_flow_max");
    return CCVS_OK;
}

struct FlowRenderK {
    const float* m;
    const float* max_px;
    const float* lut;
    uint8_t* flow;
    uint8_t* occ;
    long sB, sT, total;   // total: B * T * HW pixels
    int T, HW;
};

// one pixel: its three flow-colour bytes and its mask byte.  Every product and quotient is one fp32 operation, as in the mirror.
__device__ __forceinline__ void fv_render_px(float fx, float fy, float mk, float mp, const float* lut, uint8_t (&f3)[3], uint8_t& o) {
#pragma clang fp contract(off)
    const bool ok = mp > 0.f && fabsf(fx) < INFINITY && fabsf(fy) < INFINITY;   // (NaN compares false)
    float r = 0.f;
    int idx = 0;
    if (ok) {
        r = fminf(1.f, fv_mag(fx, fy) / mp);
        const float theta = (1.f + atan2f(fy, fx) / FV_PI) / 2.f;
        idx = max(0, min((int)(theta * 128.f), 127));
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = fminf(fmaxf(r * lut[idx * 3 + c], 0.f), 1.f);
        f3[c] = (uint8_t)(v * 255.f);
    }
    o = (uint8_t)(fminf(fmaxf(mk, 0.f), 1.f) * 255.f);   // (fmaxf(NaN, 0) = 0)
}

struct __attribute__((packed, aligned(4))) U32Triple { unsigned v[3]; };

// A lane takes four consecutive pixels of the flat [B * T * H * W] pixel order: their 12 output bytes per clip start on a dword of the
// dense channels-last output whatever H * W is, and are written as three dwords; the inputs are 16-byte loads where the four
// pixels lie in one frame.
__global__ __launch_bounds__(256) void flow_render_kernel(FlowRenderK p) {
    __shared__ float lut[128 * 3];
    for (int e = threadIdx.x; e < 128 * 3; e += 256) lut[e] = p.lut[e];
    __syncthreads();
    const long quads = (p.total + 3) / 4;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long)gridDim.x * 256) {
        const long i0 = q * 4;
        const long n0 = i0 / p.HW;
        const int px = (int)(i0 - n0 * p.HW);
        const int nv = (int)min(4L, p.total - i0);
        float fx[4], fy[4], mk[4], mp[4];
        if (px + 3 < p.HW) {   // (then nv = 4 too)
            const long b = n0 / p.T, t = n0 - b * p.T;
            const float* f = p.m + b * p.sB + t * p.sT + px;
            fv_load4(f, 4, fx);
            fv_load4(f + p.HW, 4, fy);
            fv_load4(f + 2 * (long)p.HW, 4, mk);
            const float m = p.max_px[b];
#pragma unroll
            for (int j = 0; j < 4; ++j) mp[j] = m;
        } else {
            for (int j = 0; j < 4; ++j) {
                fx[j] = fy[j] = mk[j] = mp[j] = 0.f;
                if (j < nv) {
                    const long n = (i0 + j) / p.HW;
                    const int pj = (int)(i0 + j - n * p.HW);
                    const long b = n / p.T, t = n - b * p.T;
                    const float* f = p.m + b * p.sB + t * p.sT + pj;
                    fx[j] = f[0];
                    fy[j] = f[p.HW];
                    mk[j] = f[2 * (long)p.HW];
                    mp[j] = p.max_px[b];
                }
            }
        }
        uint8_t fb[12], ob[12];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint8_t f3[3], o;
            fv_render_px(fx[j], fy[j], mk[j], mp[j], lut, f3, o);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                fb[3 * j + c] = f3[c];
                ob[3 * j + c] = o;
            }
        }
        uint8_t* fo = p.flow + 3 * i0;
        uint8_t* oo = p.occ + 3 * i0;
        if (nv == 4) {
            U32Triple fw, ow;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                fw.v[d] = fb[4 * d] | (fb[4 * d + 1] << 8) | (fb[4 * d + 2] << 16) | ((unsigned)fb[4 * d + 3] << 24);
                ow.v[d] = ob[4 * d] | (ob[4 * d + 1] << 8) | (ob[4 * d + 2] << 16) | ((unsigned)ob[4 * d + 3] << 24);
            }
            *reinterpret_cast<U32Triple*>(fo) = fw;
            *reinterpret_cast<U32Triple*>(oo) = ow;
        } else {
            for (int e = 0; e < 3 * nv; ++e) {
                fo[e] = fb[e];
                oo[e] = ob[e];
            }
        }
    }
}

extern "C" int ccvs_flow_render(const float* motion, int64_t sB, int64_t sT, int32_t B, int32_t T, int32_t H, int32_t W, const float* max_px,
                                const float* lut, uint8_t* flow_u8, uint8_t* occ_u8, void* stream) {
    CCVS_REQUIRE(motion && max_px && lut && flow_u8 && occ_u8, "ccvs_flow_render: null pointer");
    CCVS_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0 && (long)H * W <= (1L << 28) && (long)B * T * H * W <= (1L << 40), "ccvs_flow_render: bad shape %d x %d x %d x %d", B, T, H, W);
    CCVS_REQUIRE(sT >= 3L * H * W && sB >= 3L * H * W, "ccvs_flow_render: a stride shorter than the three planes");
    CCVS_REQUIRE((((uintptr_t)flow_u8 | (uintptr_t)occ_u8) & 3) == 0, "ccvs_flow_render: the uint8 outputs must start on a 4-byte boundary");
    FlowRenderK p;
    p.m = motion; p.max_px = max_px; p.lut = lut; p.flow = flow_u8; p.occ = occ_u8; p.sB = sB; p.sT = sT; p.T = T; p.HW = H * W;
    p.total = (long)B * T * H * W;
    hipLaunchKernelGGL(flow_render_kernel, dim3(strided_grid((p.total + 3) / 4, stream, 8)), dim3(256), 0, (hipStream_t)stream, p);
    CCVS_CHECK_LAUNCH("ccvs_flow_render");
    return CCVS_OK;
}

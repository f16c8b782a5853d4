// The JPEG decoder (include/ccvs_hip_decode.h): baseline JPEG scans -> uint8 frames [N, H, W, 3] whose pixels
// are libjpeg's, bit for bit.  All arithmetic is integer.  Three stages on the caller's stream:
//   A. entropy decoding, one lane per unit (a restart interval, or the whole scan of a frame without DRI): jpeg_decode_core.h, the
//      frame's tables staged in LDS, quantised int16 coefficients in natural order into a zero-filled buffer, a status word per unit;
//   B. dequantisation and jidctint's inverse DCT, one lane per block, both passes in registers: uint8 component planes padded to whole
//      MCUs;
//   C. libjpeg's "fancy" chrominance upsampling and YCbCr -> RGB, one lane per four pixels of a row, three dword stores where the
//      address allows.
#include "common.h"
#include "jpeg_decode_core.h"

#define JD_UNITS 64   // units (lanes) of a workgroup of stage A: one wave
#define JD_CONST_BITS 13
#define JD_PASS1_BITS 2
#define JD_FIX_0_298631336 2446
#define JD_FIX_0_390180644 3196
#define JD_FIX_0_541196100 4433
#define JD_FIX_0_765366865 6270
#define JD_FIX_0_899976223 7373
#define JD_FIX_1_175875602 9633
#define JD_FIX_1_501321110 12299
#define JD_FIX_1_847759065 15137
#define JD_FIX_1_961570560 16069
#define JD_FIX_2_053119869 16819
#define JD_FIX_2_562915447 20995
#define JD_FIX_3_072711026 25172

struct JdArgs {
    const uint8_t* scans;
    long scan_bytes;
    const int64_t* units;   // [n_units][5]: frame, byte offset, byte length, first MCU, MCUs
    long n_units;
    const JdTables* tables;
    int n_tables;
    const int32_t* frame_table;   // [n]: the frame's entry of `tables`
    int n, h, w, sampling;
    JdGeom g;
    long frame_blocks;            // blocks of a frame's coefficient buffer
    int wy, hy, wc, hc;           // the padded planes: Y wy x hy, Cb and Cr wc x hc
    long plane_bytes;             // wy hy + 2 wc hc
    int cw, ch;                   // the real chrominance samples: ceil(w / hs) x ceil(h / vs)
    int16_t* coef;
    uint8_t* planes;
    uint8_t* rgb;
    long frame_stride;
    int32_t* status;
};

// ---- A
__global__ __launch_bounds__(JD_UNITS) void jd_entropy_kernel(JdArgs a) {
    __shared__ JdTables s_tab;
    __shared__ int s_next;
    const int tid = threadIdx.x;
    const long nmcu = (long)a.g.mcux * a.g.mcuy;
    for (long base = (long)blockIdx.x * JD_UNITS; base < a.n_units; base += (long)gridDim.x * JD_UNITS) {
        const long u = base + tid;
        long frame = 0, off = 0, len = 0, first = 0, count = 0;
        int tix = 0, st = JD_OK, done = 1;
        if (u < a.n_units) {
            frame = a.units[5 * u], off = a.units[5 * u + 1], len = a.units[5 * u + 2], first = a.units[5 * u + 3], count = a.units[5 * u + 4];
            // (written so that no sum can overflow)
            const bool ok = frame >= 0 && frame < a.n && off >= 0 && len >= 0 && off <= a.scan_bytes && len <= a.scan_bytes - off &&
                            first >= 0 && count >= 0 && first <= nmcu && count <= nmcu - first;
            if (ok) {
                tix = a.frame_table[frame];
                if (tix >= 0 && tix < a.n_tables) done = 0;
            }
            if (done) st = JD_BAD_UNIT;
        }
        // the lanes' frames may use different tables: one round per table index among them, lowest first
        for (;;) {
            if (tid == 0) s_next = 0x7fffffff;
            __syncthreads();
            if (!done) atomicMin(&s_next, tix);
            __syncthreads();
            const int t = s_next;
            if (t == 0x7fffffff) break;   // (the same for every lane)
            const uint32_t* src = (const uint32_t*)(a.tables + t);
            uint32_t* dst = (uint32_t*)&s_tab;
            for (int i = tid; i < (int)(sizeof(JdTables) / 4); i += JD_UNITS) dst[i] = src[i];
            __syncthreads();
            if (!done && tix == t) {
                st = jd_decode_unit(a.scans + off, len, s_tab, a.g, first, count, a.coef + frame * a.frame_blocks * 64);
                done = 1;
            }
            __syncthreads();
        }
        if (u < a.n_units) a.status[u] = st;
        __syncthreads();   // s_next is the next round's too
    }
}

// ---- B: libjpeg's jidctint.c ("islow"): one 1-D pass over d[0], d[S], ..., d[7 S], descaled by N bits
template <int S, int N>
__device__ __forceinline__ void idct_pass(int* d) {
    int z2 = d[2 * S], z3 = d[6 * S];
    int z1 = (z2 + z3) * JD_FIX_0_541196100;
    int tmp2 = z1 + z3 * (-JD_FIX_1_847759065), tmp3 = z1 + z2 * JD_FIX_0_765366865;
    int tmp0 = (d[0] + d[4 * S]) * (1 << JD_CONST_BITS), tmp1 = (d[0] - d[4 * S]) * (1 << JD_CONST_BITS);
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = d[7 * S]; tmp1 = d[5 * S]; tmp2 = d[3 * S]; tmp3 = d[S];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * JD_FIX_1_175875602;
    tmp0 *= JD_FIX_0_298631336; tmp1 *= JD_FIX_2_053119869; tmp2 *= JD_FIX_3_072711026; tmp3 *= JD_FIX_1_501321110;
    z1 *= -JD_FIX_0_899976223; z2 *= -JD_FIX_2_562915447;
    z3 = z3 * (-JD_FIX_1_961570560) + z5;
    z4 = z4 * (-JD_FIX_0_390180644) + z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    constexpr int half = 1 << (N - 1);
    d[0] = (tmp10 + tmp3 + half) >> N;
    d[7 * S] = (tmp10 - tmp3 + half) >> N;
    d[S] = (tmp11 + tmp2 + half) >> N;
    d[6 * S] = (tmp11 - tmp2 + half) >> N;
    d[2 * S] = (tmp12 + tmp1 + half) >> N;
    d[5 * S] = (tmp12 - tmp1 + half) >> N;
    d[3 * S] = (tmp13 + tmp0 + half) >> N;
    d[4 * S] = (tmp13 - tmp0 + half) >> N;
}
__device__ __forceinline__ unsigned clamp255(int v) { return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

__global__ __launch_bounds__(256) void jd_idct_kernel(JdArgs a) {
    const long total = (long)a.n * a.frame_blocks;
    const long ny = (long)a.g.mcux * a.g.mcuy * a.g.hs * a.g.vs, nc = (long)a.g.mcux * a.g.mcuy;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long frame = i / a.frame_blocks;
        long blk = i - frame * a.frame_blocks;
        uint8_t* plane = a.planes + frame * a.plane_bytes;
        int comp = 0, bw = a.wy >> 3, pw = a.wy;
        if (blk >= ny) {
            comp = blk >= ny + nc ? 2 : 1;
            blk -= ny + (comp - 1) * nc;
            plane += (long)a.wy * a.hy + (long)(comp - 1) * a.wc * a.hc;
            bw = a.wc >> 3;
            pw = a.wc;
        }
        const int by = (int)(blk / bw), bx = (int)(blk - (long)by * bw);
        int tix = a.frame_table[frame];
        tix = tix < 0 || tix >= a.n_tables ? 0 : tix;   // (such a frame's units all carry JD_BAD_UNIT)
        const uint16_t* q = a.tables[tix].q[comp];
        const uint4* src = (const uint4*)(a.coef + i * 64);
        int d[64];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint4 v = src[k];
            const unsigned wds[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                d[8 * k + 2 * j] = (int)(short)(wds[j] & 0xffffu) * (int)q[8 * k + 2 * j];
                d[8 * k + 2 * j + 1] = (int)(short)(wds[j] >> 16) * (int)q[8 * k + 2 * j + 1];
            }
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) idct_pass<8, JD_CONST_BITS - JD_PASS1_BITS>(d + c);
#pragma unroll
        for (int r = 0; r < 8; ++r) idct_pass<1, JD_CONST_BITS + JD_PASS1_BITS + 3>(d + 8 * r);
        uint8_t* dst = plane + (long)by * 8 * pw + bx * 8;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            uint2 o;
            o.x = clamp255(d[8 * r] + 128) | clamp255(d[8 * r + 1] + 128) << 8 | clamp255(d[8 * r + 2] + 128) << 16 | clamp255(d[8 * r + 3] + 128) << 24;
            o.y = clamp255(d[8 * r + 4] + 128) | clamp255(d[8 * r + 5] + 128) << 8 | clamp255(d[8 * r + 6] + 128) << 16 | clamp255(d[8 * r + 7] + 128) << 24;
            *(uint2*)(dst + (long)r * pw) = o;   // 8-byte aligned: the planes' widths and offsets are multiples of 8
        }
    }
}

// ---- C: a chrominance sample at full resolution.  SAMPLING 1 (h2v1): (3 near + far + 1 or 2) >> 2 along the row; 2 (h2v2): the same
// triangle over s = 3 near row + far row with + 8 or 7 and >> 4.  Neighbours beyond the cw x ch real samples replicate the edge.
template <int SAMPLING>
__device__ __forceinline__ int chroma_at(const uint8_t* c, int pw, int cw, int ch, int y, int x) {
    if (SAMPLING == 0) return c[(long)y * pw + x];
    const int i = x >> 1, odd = x & 1;
    int j = odd ? i + 1 : i - 1;
    j = j < 0 ? 0 : (j > cw - 1 ? cw - 1 : j);
    if (SAMPLING == 1) {
        const uint8_t* r = c + (long)y * pw;
        return (3 * r[i] + r[j] + 1 + odd) >> 2;
    }
    const int cy = y >> 1;
    int fy = (y & 1) ? cy + 1 : cy - 1;
    fy = fy < 0 ? 0 : (fy > ch - 1 ? ch - 1 : fy);
    const uint8_t *near = c + (long)cy * pw, *far = c + (long)fy * pw;
    const int s0 = 3 * near[i] + far[i], s1 = 3 * near[j] + far[j];
    return (3 * s0 + s1 + 8 - odd) >> 4;
}

template <int SAMPLING>
__global__ __launch_bounds__(256) void jd_colour_kernel(JdArgs a) {
    const int w4 = (a.w + 3) >> 2;
    const long per_frame = (long)a.h * w4, total = (long)a.n * per_frame;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long frame = i / per_frame;
        const long rem = i - frame * per_frame;
        const int y = (int)(rem / w4), x0 = (int)(rem - (long)y * w4) * 4;
        const uint8_t* py = a.planes + frame * a.plane_bytes;
        const uint8_t* pcb = py + (long)a.wy * a.hy;
        const uint8_t* pcr = pcb + (long)a.wc * a.hc;
        const int npx = a.w - x0 < 4 ? a.w - x0 : 4;
        uint8_t o[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = x0 + k < a.w ? x0 + k : a.w - 1;
            const int Y = py[(long)y * a.wy + x];
            const int cb = chroma_at<SAMPLING>(pcb, a.wc, a.cw, a.ch, y, x) - 128, cr = chroma_at<SAMPLING>(pcr, a.wc, a.cw, a.ch, y, x) - 128;
            o[3 * k] = (uint8_t)clamp255(Y + ((91881 * cr + 32768) >> 16));
            o[3 * k + 1] = (uint8_t)clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
            o[3 * k + 2] = (uint8_t)clamp255(Y + ((116130 * cb + 32768) >> 16));
        }
        uint8_t* dst = a.rgb + frame * a.frame_stride + ((long)y * a.w + x0) * 3;
        if (npx == 4 && ((uintptr_t)dst & 3) == 0) {
            unsigned* d32 = (unsigned*)dst;
#pragma unroll
            for (int k = 0; k < 3; ++k) d32[k] = o[4 * k] | (unsigned)o[4 * k + 1] << 8 | (unsigned)o[4 * k + 2] << 16 | (unsigned)o[4 * k + 3] << 24;
        } else {
            for (int k = 0; k < 3 * npx; ++k) dst[k] = o[k];
        }
    }
}

// ---- the host side
static inline bool jd_shape_ok(int n, int h, int w, int sampling) {
    return n >= 1 && h >= 1 && h <= 65535 && w >= 1 && w <= 65535 && sampling >= 0 && sampling <= 2 && (sampling == 0 || w > 4);
}
static void jd_geometry(JdArgs& a, int n, int h, int w, int sampling) {
    a.n = n; a.h = h; a.w = w; a.sampling = sampling;
    a.g.hs = sampling == 0 ? 1 : 2;
    a.g.vs = sampling == 2 ? 2 : 1;
    a.g.mcux = (w + 8 * a.g.hs - 1) / (8 * a.g.hs);
    a.g.mcuy = (h + 8 * a.g.vs - 1) / (8 * a.g.vs);
    a.frame_blocks = jd_frame_blocks(a.g);
    a.wc = 8 * a.g.mcux; a.hc = 8 * a.g.mcuy;
    a.wy = a.wc * a.g.hs; a.hy = a.hc * a.g.vs;
    a.plane_bytes = (long)a.wy * a.hy + 2L * a.wc * a.hc;
    a.cw = (w + a.g.hs - 1) / a.g.hs;
    a.ch = (h + a.g.vs - 1) / a.g.vs;
}
// the coefficients (128 bytes per block), then the planes; both parts multiples of 256 bytes
static inline size_t jd_coef_bytes(const JdArgs& a) { return ((size_t)a.n * a.frame_blocks * 128 + 255) & ~(size_t)255; }

extern "C" size_t ccvs_mjpeg_decode_workspace_bytes(int n, int h, int w, int sampling) {
    if (!jd_shape_ok(n, h, w, sampling)) return 0;
    JdArgs a;
    jd_geometry(a, n, h, w, sampling);
    return jd_coef_bytes(a) + (((size_t)n * a.plane_bytes + 255) & ~(size_t)255);
}

extern "C" int ccvs_mjpeg_decode(const uint8_t* scans, long scan_bytes, const int64_t* units, const int64_t* units_host, long n_units,
                                 const void* tables, int n_tables, const int32_t* frame_table, int n, int h, int w, int sampling,
                                 uint8_t* rgb, long frame_stride, int32_t* status, void* workspace, void* hip_stream) {
    CCVS_REQUIRE(sampling >= 0 && sampling <= 2, "ccvs_mjpeg_decode: sampling %d is none of 0 (4:4:4), 1 (4:2:2), 2 (4:2:0)", sampling);
    CCVS_REQUIRE(h >= 1 && h <= 65535 && w >= 1 && w <= 65535, "ccvs_mjpeg_decode: frame size %d x %d outside 1 .. 65535", h, w);
    CCVS_REQUIRE(sampling == 0 || w > 4, "ccvs_mjpeg_decode: a subsampled frame %d pixels wide has fewer than 3 chrominance columns", w);
    CCVS_REQUIRE(n >= 1 && n_units >= 1 && n_tables >= 1, "ccvs_mjpeg_decode: no frames, no units or no tables");
    CCVS_REQUIRE(scan_bytes >= 0 && frame_stride >= (long)h * w * 3, "ccvs_mjpeg_decode: a negative stream length, or a frame stride below a frame's bytes");
    CCVS_REQUIRE(scans && units && units_host && tables && frame_table && rgb && status && workspace,
                 "ccvs_mjpeg_decode: null stream, unit table, tables, frames, status or workspace");
    CCVS_REQUIRE((uintptr_t)units % 8 == 0 && (uintptr_t)tables % 4 == 0 && (uintptr_t)frame_table % 4 == 0 && (uintptr_t)status % 4 == 0 &&
                     (uintptr_t)workspace % 16 == 0, "ccvs_mjpeg_decode: a misaligned unit table (8), tables, frame table, status (4) or workspace (16)");
    JdArgs a;
    jd_geometry(a, n, h, w, sampling);
    const long nmcu = (long)a.g.mcux * a.g.mcuy;
    for (long u = 0; u < n_units; ++u) {
        const int64_t* e = units_host + 5 * u;
        CCVS_REQUIRE(e[0] >= 0 && e[0] < n, "ccvs_mjpeg_decode: unit %ld names frame %ld of %d", u, (long)e[0], n);
        CCVS_REQUIRE(e[1] >= 0 && e[2] >= 0 && e[1] <= scan_bytes && e[2] <= scan_bytes - e[1],
                     "ccvs_mjpeg_decode: unit %ld (bytes %ld + %ld) points outside the stream of %ld bytes", u, (long)e[1], (long)e[2], scan_bytes);
        CCVS_REQUIRE(e[3] >= 0 && e[4] >= 0 && e[3] <= nmcu && e[4] <= nmcu - e[3],
                     "ccvs_mjpeg_decode: unit %ld (MCUs %ld + %ld) points outside the frame's %ld MCUs", u, (long)e[3], (long)e[4], nmcu);
    }
    a.scans = scans; a.scan_bytes = scan_bytes; a.units = units; a.n_units = n_units;
    a.tables = (const JdTables*)tables; a.n_tables = n_tables; a.frame_table = frame_table;
    a.coef = (int16_t*)workspace;
    a.planes = (uint8_t*)workspace + jd_coef_bytes(a);
    a.rgb = rgb; a.frame_stride = frame_stride; a.status = status;
    hipStream_t s = (hipStream_t)hip_stream;
    if (hipMemsetAsync(a.coef, 0, (size_t)n * a.frame_blocks * 128, s) != hipSuccess) {
        ccvs_set_error("ccvs_mjpeg_decode: clearing the coefficients failed: %s", hipGetErrorString(hipGetLastError()));
        return CCVS_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(jd_entropy_kernel, dim3(limited_grid((n_units + JD_UNITS - 1) / JD_UNITS, hip_stream, 8)), dim3(JD_UNITS), 0, s, a);
    hipLaunchKernelGGL(jd_idct_kernel, dim3(strided_grid((long)n * a.frame_blocks, hip_stream, 8)), dim3(256), 0, s, a);
    const dim3 grid(strided_grid((long)n * h * ((w + 3) / 4), hip_stream, 8));
    if (sampling == 0) hipLaunchKernelGGL(jd_colour_kernel<0>, grid, dim3(256), 0, s, a);
    else if (sampling == 1) hipLaunchKernelGGL(jd_colour_kernel<1>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(jd_colour_kernel<2>, grid, dim3(256), 0, s, a);
    CCVS_CHECK_LAUNCH("ccvs_mjpeg_decode");
    return CCVS_OK;
}

// The GIF output stage (include/ccvs_hip_output_gif.h): uint8 RGB clips -> a colour table per clip and every
// frame's LZW data in sub-blocks.  All in integers; tests/gif_ref.py states the same algorithm in numpy, the kernels give its bytes.
//   ccvs_gif_palette   bins      every pixel into its clip's 32768 bins: count and channel sums (the stage's only atomics);
//                      cut       a workgroup per clip: median cut over the occupied bins, the palette, the bins' index table;
//   ccvs_gif_encode    code      a wave per band: the pixels' indices through the table, LZW-coded from an empty dictionary (gif_core.h);
//                      scan      the bands' bit positions in their frames, the frames' sizes and offsets;
//                      stitch    a thread per byte of a frame's data: the bands' bits shifted together, the sub-blocks' length bytes.
#include "common.h"
#include "gif_core.h"

#define GIF_NBINS 32768
#define GIF_HIST_RUN 16              // consecutive pixels of a lane in the bins launch
#define GIF_CUT_THREADS 1024
#define GIF_CHUNK 1024               // indices staged in LDS at a time by the band coder
#define GIF_THREADS 256

struct GifPalArgs {
    const uint8_t* clips;
    long clip_stride, frame_stride;
    int b, t, h, w;
    unsigned long long* hist;        // [b][4][32768]: count, sum R, sum G, sum B
    uint8_t* palette;                // [b][256][3]
    uint8_t* table;                  // [b][32768]
    int* used;                       // [b]
};

__device__ __forceinline__ int gif_bin(const uint8_t* p) { return ((p[0] >> 3) << 10) | ((p[1] >> 3) << 5) | (p[2] >> 3); }

// ---- bins: an item is GIF_HIST_RUN consecutive pixels of a frame; equal bins that follow each other share one set of atomics
__global__ __launch_bounds__(GIF_THREADS) void gif_bins_kernel(GifPalArgs a) {
    const long hw = (long)a.h * a.w;
    const long per_frame = (hw + GIF_HIST_RUN - 1) / GIF_HIST_RUN;
    const long items = per_frame * a.t * a.b;
    for (long it = (long)blockIdx.x * GIF_THREADS + threadIdx.x; it < items; it += (long)gridDim.x * GIF_THREADS) {
        const long fr = it / per_frame, p0 = (it % per_frame) * GIF_HIST_RUN;
        const long clip = fr / a.t, f = fr % a.t;
        const uint8_t* src = a.clips + clip * a.clip_stride + f * a.frame_stride;
        unsigned long long* hist = a.hist + clip * 4 * GIF_NBINS;
        const long p1 = p0 + GIF_HIST_RUN < hw ? p0 + GIF_HIST_RUN : hw;
        int bin = -1;
        unsigned n = 0, r = 0, g = 0, bl = 0;
        for (long p = p0; p <= p1; ++p) {
            const int cur = p < p1 ? gif_bin(src + 3 * p) : -1;
            if (cur != bin) {
                if (n) {
                    atomicAdd(&hist[bin], (unsigned long long)n);
                    atomicAdd(&hist[GIF_NBINS + bin], (unsigned long long)r);
                    atomicAdd(&hist[2 * GIF_NBINS + bin], (unsigned long long)g);
                    atomicAdd(&hist[3 * GIF_NBINS + bin], (unsigned long long)bl);
                }
                bin = cur;
                n = r = g = bl = 0;
            }
            if (p < p1) {
                ++n;
                r += src[3 * p];
                g += src[3 * p + 1];
                bl += src[3 * p + 2];
            }
        }
    }
}

// ---- cut: one workgroup of 1024 per clip.  The bins' boxes (a byte each) and an occupancy bit per bin live in LDS; the counts stay
// in global memory.  A box's figures come from its marginals: thread (c, j) walks the 32 bins with coordinate c on the axis and j on
// the next, the 32 lanes of a c sum up, and what the box occupies along the axis is where the marginal is not empty.
struct GifCutLds {
    uint8_t box[GIF_NBINS];
    unsigned occ[GIF_NBINS / 32];
    unsigned long long pop[256];
    int nbins[256];
    uint8_t lo[256][4], hi[256][4];
    unsigned long long mpop[32];
    int mn[32];
    int pick[3];                     // the box to split (-1: none), its axis, the cut
    uint8_t pal[256][4];
};

__device__ __forceinline__ int gif_bin_at(int axis, int c, int j, int k) {
    return axis == 0 ? (c << 10) | (j << 5) | k : (axis == 1 ? (j << 10) | (c << 5) | k : (j << 10) | (k << 5) | c);
}
__device__ __forceinline__ bool gif_occupied(const GifCutLds& s, int bin) { return (s.occ[bin >> 5] >> (bin & 31)) & 1u; }

__device__ void gif_marginal(GifCutLds& s, const unsigned long long* cnt, int box, int axis) {
    const int tid = threadIdx.x, c = tid >> 5, j = tid & 31;
    unsigned long long pop = 0;
    int n = 0;
    for (int k = 0; k < 32; ++k) {
        const int bin = gif_bin_at(axis, c, j, k);
        if (gif_occupied(s, bin) && s.box[bin] == box) {
            pop += cnt[bin];
            ++n;
        }
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
        pop += __shfl_xor(pop, o, WAVE);
        n += __shfl_xor(n, o, WAVE);
    }
    if (j == 0) {
        s.mpop[c] = pop;
        s.mn[c] = n;
    }
    __syncthreads();
}

__device__ void gif_box_stats(GifCutLds& s, const unsigned long long* cnt, int box) {
    for (int axis = 0; axis < 3; ++axis) {
        gif_marginal(s, cnt, box, axis);
        if (threadIdx.x == 0) {
            int lo = 31, hi = 0, n = 0;
            unsigned long long pop = 0;
            for (int c = 0; c < 32; ++c)
                if (s.mn[c]) {
                    lo = c < lo ? c : lo;
                    hi = c;
                    n += s.mn[c];
                    pop += s.mpop[c];
                }
            s.lo[box][axis] = (uint8_t)lo;
            s.hi[box][axis] = (uint8_t)hi;
            s.pop[box] = pop;
            s.nbins[box] = n;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(GIF_CUT_THREADS) void gif_cut_kernel(GifPalArgs a) {
    __shared__ GifCutLds s;
    const int tid = threadIdx.x;
    for (int clip = blockIdx.x; clip < a.b; clip += gridDim.x) {
        const unsigned long long* cnt = a.hist + (long)clip * 4 * GIF_NBINS;
        {
            unsigned m = 0;
            for (int k = 0; k < 32; ++k) {
                m |= cnt[tid * 32 + k] ? 1u << k : 0u;
                s.box[tid * 32 + k] = 0;
            }
            s.occ[tid] = m;
        }
        __syncthreads();
        gif_box_stats(s, cnt, 0);
        int nbox = 1;
        while (nbox < 256) {
            if (tid < WAVE) {                                   // the box with the largest population x longest extent, the lowest of equals
                unsigned long long best = 0;
                int which = -1;
                for (int k = tid; k < nbox; k += WAVE) {
                    int ext = 0;
                    for (int x = 0; x < 3; ++x) ext = max(ext, (int)s.hi[k][x] - (int)s.lo[k][x]);
                    const unsigned long long score = s.nbins[k] >= 2 ? s.pop[k] * (unsigned long long)ext : 0ull;
                    if (score > best) {
                        best = score;
                        which = k;
                    }
                }
#pragma unroll
                for (int o = WAVE / 2; o > 0; o >>= 1) {
                    const unsigned long long ob = __shfl_xor(best, o, WAVE);
                    const int ow = __shfl_xor(which, o, WAVE);
                    if (ow >= 0 && (ob > best || (ob == best && (which < 0 || ow < which)))) {
                        best = ob;
                        which = ow;
                    }
                }
                if (tid == 0) {
                    s.pick[0] = which;
                    if (which >= 0) {
                        const int er = s.hi[which][0] - s.lo[which][0], eg = s.hi[which][1] - s.lo[which][1], eb = s.hi[which][2] - s.lo[which][2];
                        const int longest = max(er, max(eg, eb));
                        s.pick[1] = eg == longest ? 1 : (er == longest ? 0 : 2);      // ties: G, then R, then B
                    }
                }
            }
            __syncthreads();
            const int which = s.pick[0], axis = s.pick[1];
            if (which < 0) break;                               // (the same in every thread)
            gif_marginal(s, cnt, which, axis);
            if (tid == 0) {
                const int lo = s.lo[which][axis], hi = s.hi[which][axis];
                const unsigned long long half = (s.pop[which] + 1) / 2;
                unsigned long long run = 0;
                int cut = hi - 1;
                for (int c = lo; c < hi; ++c) {
                    run += s.mpop[c];
                    if (run >= half) {
                        cut = c;
                        break;
                    }
                }
                s.pick[2] = cut;
            }
            __syncthreads();
            const int cut = s.pick[2];
            for (int k = 0; k < 32; ++k) {
                const int bin = tid * 32 + k;
                const int c = axis == 0 ? bin >> 10 : (axis == 1 ? (bin >> 5) & 31 : bin & 31);
                if (gif_occupied(s, bin) && s.box[bin] == which && c > cut) s.box[bin] = (uint8_t)nbox;
            }
            __syncthreads();
            gif_box_stats(s, cnt, which);
            gif_box_stats(s, cnt, nbox);
            ++nbox;
        }
        // the palette: four threads per box, a quarter of the bins each
        {
            const int box = tid >> 2, part = tid & 3;
            unsigned long long n = 0, sum[3] = {0, 0, 0};
            for (int bin = part * (GIF_NBINS / 4); bin < (part + 1) * (GIF_NBINS / 4); ++bin)
                if (gif_occupied(s, bin) && s.box[bin] == box) {
                    n += cnt[bin];
                    for (int x = 0; x < 3; ++x) sum[x] += cnt[(x + 1) * GIF_NBINS + bin];
                }
            for (int o = 1; o < 4; o <<= 1) {
                n += __shfl_xor(n, o, WAVE);
                for (int x = 0; x < 3; ++x) sum[x] += __shfl_xor(sum[x], o, WAVE);
            }
            if (part == 0)
                for (int x = 0; x < 3; ++x) {
                    const unsigned v = box < nbox && n ? (unsigned)((2 * sum[x] + n) / (2 * n)) : 0u;
                    s.pal[box][x] = (uint8_t)v;
                    a.palette[((long)clip * 256 + box) * 3 + x] = (uint8_t)v;
                }
            if (tid == 0) a.used[clip] = nbox;
        }
        __syncthreads();
        // the table: an occupied bin's own mean colour to the nearest entry, the lowest of equals
        for (int k = 0; k < 32; ++k) {
            const int bin = tid * 32 + k;
            int best = 0;
            if (gif_occupied(s, bin)) {
                const unsigned long long n = cnt[bin];
                int own[3];
                for (int x = 0; x < 3; ++x) own[x] = (int)((2 * cnt[(x + 1) * GIF_NBINS + bin] + n) / (2 * n));
                int bd = 0x7fffffff;
                for (int e = 0; e < nbox; ++e) {
                    const int dr = own[0] - s.pal[e][0], dg = own[1] - s.pal[e][1], db = own[2] - s.pal[e][2];
                    const int d = dr * dr + dg * dg + db * db;
                    if (d < bd) {
                        bd = d;
                        best = e;
                    }
                }
            }
            a.table[(long)clip * GIF_NBINS + bin] = (uint8_t)best;
        }
        __syncthreads();   // the LDS is the next clip's too
    }
}

// ---- the encoder
struct GifArgs {
    const uint8_t* clips;
    long clip_stride, frame_stride;
    int t, n, h, w, band_rows, nb;   // n = b t frames; nb: bands per frame
    long T, wstride;                 // bands in all; words of a band's bits
    const uint8_t* table;
    uint8_t* stream;
    long capacity;
    long* offsets;
    long* bitoff;                    // [n][nb + 1] a band's first bit in its frame's data; [nb]: the frame's bits
    long* fsize;                     // [n] bytes of a frame's payload
    unsigned* words;                 // [T][wstride]
};

// code: a wave per band
__global__ __launch_bounds__(WAVE) void gif_code_kernel(GifArgs a) {
    __shared__ unsigned s_hash[GIF_SLOTS];
    __shared__ uint8_t s_idx[GIF_CHUNK];
    const int lane = threadIdx.x;
    for (long band = blockIdx.x; band < a.T; band += gridDim.x) {
        const long f = band / a.nb;
        const int b = (int)(band % a.nb);
        const int r0 = b * a.band_rows;
        const int r1 = r0 + a.band_rows < a.h ? r0 + a.band_rows : a.h;
        const long L = (long)(r1 - r0) * a.w;
        const uint8_t* src = a.clips + (f / a.t) * a.clip_stride + (f % a.t) * a.frame_stride + 3L * r0 * a.w;
        const uint8_t* table = a.table + (f / a.t) * GIF_NBINS;
        for (int i = lane; i < GIF_SLOTS; i += WAVE) s_hash[i] = GIF_EMPTY;
        GifCoder s;
        gif_start(s, a.words + band * a.wstride, b == 0, lane == 0);
        for (long c0 = 0; c0 < L; c0 += GIF_CHUNK) {
            const int n = (int)(L - c0 < GIF_CHUNK ? L - c0 : GIF_CHUNK);
            __syncthreads();                                    // the chunk before is coded, the hash is empty
            for (int i = lane; i < n; i += WAVE) s_idx[i] = table[gif_bin(src + 3 * (c0 + i))];
            __syncthreads();
            int pos = 0;
            while (pos < n) {
                pos += gif_code(s, s_hash, s_idx + pos, n - pos);
                if (s.full) {                                   // (the same in every lane)
                    __syncthreads();
                    for (int i = lane; i < GIF_SLOTS; i += WAVE) s_hash[i] = GIF_EMPTY;
                    __syncthreads();
                    s.full = 0;
                }
            }
        }
        const long bits = gif_finish(s, b == a.nb - 1);
        if (lane == 0) a.bitoff[f * (a.nb + 1) + b + 1] = bits;   // (the scan turns the sizes into positions)
        __syncthreads();
    }
}

// scan: one workgroup.  Per frame the bands' bit positions and the payload's size; then the frames' offsets (png_scan_body's form)
__global__ __launch_bounds__(GIF_THREADS) void gif_scan_kernel(GifArgs a) {
    __shared__ long s_sum[GIF_THREADS];
    const int tid = threadIdx.x;
    for (long f = tid; f < a.n; f += GIF_THREADS) {
        long* off = a.bitoff + f * (a.nb + 1);
        long run = 0;
        off[0] = 0;
        for (int b = 1; b <= a.nb; ++b) {
            run += off[b];
            off[b] = run;
        }
        a.fsize[f] = gif_payload_bytes((run + 7) >> 3);
    }
    __syncthreads();
    const long chunk = (a.n + GIF_THREADS - 1) / GIF_THREADS;
    const long i0 = tid * chunk < a.n ? tid * chunk : a.n;
    const long i1 = i0 + chunk < a.n ? i0 + chunk : a.n;
    long sum = 0;
    for (long i = i0; i < i1; ++i) sum += a.fsize[i];
    s_sum[tid] = sum;
    __syncthreads();
    long run = 0, total = 0;
    for (int j = 0; j < GIF_THREADS; ++j) {
        const long c = s_sum[j];
        run += j < tid ? c : 0;
        total += c;
    }
    for (long i = i0; i < i1; ++i) {
        a.offsets[i] = run;
        run += a.fsize[i];
    }
    if (tid == 0) a.offsets[a.n] = total;
}

__device__ __forceinline__ void gif_store(const GifArgs& a, long pos, unsigned byte) {
    if (pos < a.capacity) a.stream[pos] = (uint8_t)byte;
}

// stitch: a block of the walk is GIF_THREADS consecutive bytes of one frame's data; `per_frame` blocks cover the largest a frame can have
__global__ __launch_bounds__(GIF_THREADS) void gif_stitch_kernel(GifArgs a, long per_frame) {
    const long blocks = per_frame * a.n;
    for (long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
        const long f = blk / per_frame;
        const long j = (blk % per_frame) * GIF_THREADS + threadIdx.x;
        const long* bitoff = a.bitoff + f * (a.nb + 1);
        const long data = (bitoff[a.nb] + 7) >> 3;
        if (j >= data) continue;
        const long base = a.offsets[f];
        const unsigned byte = gif_data_byte(a.words + f * a.nb * a.wstride, a.wstride, bitoff, a.nb, j);
        gif_store(a, base + gif_data_pos(j), byte);
        if (j % 255 == 0) gif_store(a, base + gif_data_pos(j) - 1, gif_block_len(data, j));
        if (j == 0) gif_store(a, base, 8u);                     // the LZW minimum code size
        if (j == data - 1) gif_store(a, base + gif_payload_bytes(data) - 1, 0u);
    }
}

// ---- host
static inline bool gif_shape_ok(long n, int h, int w, int band_rows) {
    if (!(n >= 1 && n < (1L << 24) && h >= 1 && h <= 65535 && w >= 1 && w <= 65535 && band_rows >= 0)) return false;
    const long rows = gif_band_rows(w, band_rows) < h ? gif_band_rows(w, band_rows) : h;
    return rows * w < (1L << 24);
}
static inline size_t gif_align8(size_t v) { return (v + 7) & ~(size_t)7; }
static inline long gif_band_max(int h, int w, int band_rows) {
    const long r = gif_band_rows(w, band_rows);
    return (r < h ? r : h) * w;
}

extern "C" size_t ccvs_gif_workspace_bytes(int b, int t, int h, int w, int band_rows) {
    if (b < 1 || t < 1 || !gif_shape_ok((long)b * t, h, w, band_rows)) return 0;
    const size_t n = (size_t)b * t, nb = (size_t)gif_bands(h, w, band_rows);
    // the bins; the bands' positions, the frames' sizes, the bands' bits
    return (size_t)b * 4 * GIF_NBINS * 8 + n * (nb + 1) * 8 + n * 8 + gif_align8(n * nb * (size_t)gif_band_words(gif_band_max(h, w, band_rows)) * 4);
}

extern "C" long ccvs_gif_stream_bound(int n, int h, int w, int band_rows) {
    if (!gif_shape_ok(n, h, w, band_rows)) return 0;
    const long r = gif_band_rows(w, band_rows), nb = gif_bands(h, w, band_rows);
    const long full = r < h ? r : h, tail = h - (nb - 1) * r;
    const long bits = (nb - 1) * gif_band_bits(full * w) + gif_band_bits(tail * w);
    return (long)n * gif_payload_bytes((bits + 7) >> 3);
}

#define GIF_REQUIRE_CLIPS(who)                                                                                                        \
    do {                                                                                                                              \
        CCVS_REQUIRE(b >= 1 && t >= 1 && (long)b * t < (1L << 24), "%s: %d clips of %d frames (1 .. 2^24 - 1 frames in all)", who, b, t); \
        CCVS_REQUIRE(h >= 1 && h <= 65535 && w >= 1 && w <= 65535, "%s: frame size %d x %d outside 1 .. 65535", who, h, w);          \
        CCVS_REQUIRE(frame_stride >= 3L * w * h, "%s: frame stride %ld is less than the frame's %ld bytes", who, frame_stride, 3L * w * h); \
        CCVS_REQUIRE(clip_stride >= (t - 1) * frame_stride + 3L * w * h, "%s: clip stride %ld is less than the clip's %ld bytes", who, \
                     clip_stride, (t - 1) * frame_stride + 3L * w * h);                                                              \
    } while (0)

extern "C" int ccvs_gif_palette(const uint8_t* clips, long clip_stride, long frame_stride, int b, int t, int h, int w, uint8_t* palette,
                                uint8_t* table, int* used, void* workspace, void* hip_stream) {
    const char* who = "ccvs_gif_palette";
    GIF_REQUIRE_CLIPS(who);
    CCVS_REQUIRE(clips && palette && table && used && workspace, "%s: null clips, palette, table, used or workspace", who);
    GifPalArgs a;
    a.clips = clips; a.clip_stride = clip_stride; a.frame_stride = frame_stride;
    a.b = b; a.t = t; a.h = h; a.w = w;
    a.hist = (unsigned long long*)workspace;
    a.palette = palette; a.table = table; a.used = used;
    hipStream_t st = (hipStream_t)hip_stream;
    if (hipMemsetAsync(a.hist, 0, (size_t)b * 4 * GIF_NBINS * 8, st) != hipSuccess) {
        ccvs_set_error("%s: clearing the bins failed: %s", who, hipGetErrorString(hipGetLastError()));
        return CCVS_ERR_LAUNCH;
    }
    const long items = (((long)h * w + GIF_HIST_RUN - 1) / GIF_HIST_RUN) * t * b;
    hipLaunchKernelGGL(gif_bins_kernel, dim3(strided_grid(items, hip_stream, 8)), dim3(GIF_THREADS), 0, st, a);
    hipLaunchKernelGGL(gif_cut_kernel, dim3(limited_grid(b, hip_stream, 1)), dim3(GIF_CUT_THREADS), 0, st, a);
    CCVS_CHECK_LAUNCH(who);
    return CCVS_OK;
}

extern "C" int ccvs_gif_encode(const uint8_t* clips, long clip_stride, long frame_stride, int b, int t, int h, int w, int band_rows,
                               const uint8_t* table, uint8_t* stream, long capacity, long* offsets, void* workspace, void* hip_stream) {
    const char* who = "ccvs_gif_encode";
    GIF_REQUIRE_CLIPS(who);
    CCVS_REQUIRE(band_rows >= 0, "%s: band_rows %d is negative", who, band_rows);
    CCVS_REQUIRE(gif_shape_ok((long)b * t, h, w, band_rows), "%s: band_rows %d makes a band of 2^24 indices or more", who, band_rows);
    CCVS_REQUIRE(capacity >= 0, "%s: negative capacity", who);
    CCVS_REQUIRE(clips && table && offsets && workspace && (stream || capacity == 0), "%s: null clips, table, stream, offsets or workspace", who);
    GifArgs a;
    a.clips = clips; a.clip_stride = clip_stride; a.frame_stride = frame_stride;
    a.t = t; a.n = b * t; a.h = h; a.w = w;
    a.band_rows = gif_band_rows(w, band_rows);
    a.nb = (int)gif_bands(h, w, band_rows);
    a.T = (long)a.n * a.nb;
    a.wstride = gif_band_words(gif_band_max(h, w, band_rows));
    a.table = table; a.stream = stream; a.capacity = capacity; a.offsets = offsets;
    char* p = (char*)workspace + (size_t)b * 4 * GIF_NBINS * 8;    // (behind the palette's bins)
    a.bitoff = (long*)p;                p += 8 * (size_t)a.n * (a.nb + 1);
    a.fsize = (long*)p;                 p += 8 * (size_t)a.n;
    a.words = (unsigned*)p;
    hipStream_t st = (hipStream_t)hip_stream;
    const long full = a.band_rows < h ? a.band_rows : h, tail = h - (long)(a.nb - 1) * a.band_rows;
    const long data_max = ((a.nb - 1) * gif_band_bits(full * w) + gif_band_bits(tail * w) + 7) >> 3;
    const long per_frame = (data_max + GIF_THREADS - 1) / GIF_THREADS;
    hipLaunchKernelGGL(gif_code_kernel, dim3(limited_grid(a.T, hip_stream, 4)), dim3(WAVE), 0, st, a);
    hipLaunchKernelGGL(gif_scan_kernel, dim3(1), dim3(GIF_THREADS), 0, st, a);
    hipLaunchKernelGGL(gif_stitch_kernel, dim3(limited_grid(per_frame * a.n, hip_stream, 8)), dim3(GIF_THREADS), 0, st, a, per_frame);
    CCVS_CHECK_LAUNCH(who);
    return CCVS_OK;
}

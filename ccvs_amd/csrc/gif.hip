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

// `cap`: the median cut stops at so many boxes (2 .. 256).  CAPPED = false: at 256 whatever `cap` says -- the constant keeps this
// instantiation, which max_colours = 256 launches, instruction for instruction the kernel from before the argument
template <bool CAPPED>
__global__ __launch_bounds__(GIF_CUT_THREADS) void gif_cut_kernel(GifPalArgs a, int cap) {
    __shared__ GifCutLds s;
    const int tid = threadIdx.x;
    const int max_boxes = CAPPED ? cap : 256;
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
        while (nbox < max_boxes) {
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

static int gif_palette_launch(const char* who, const uint8_t* clips, long clip_stride, long frame_stride, int b, int t, int h, int w,
                              int max_colours, uint8_t* palette, uint8_t* table, int* used, void* workspace, void* hip_stream) {
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
    hipLaunchKernelGGL(max_colours == 256 ? gif_cut_kernel<false> : gif_cut_kernel<true>, dim3(limited_grid(b, hip_stream, 1)),
                       dim3(GIF_CUT_THREADS), 0, st, a, max_colours);
    CCVS_CHECK_LAUNCH(who);
    return CCVS_OK;
}

extern "C" int ccvs_gif_palette(const uint8_t* clips, long clip_stride, long frame_stride, int b, int t, int h, int w, uint8_t* palette,
                                uint8_t* table, int* used, void* workspace, void* hip_stream) {
    return gif_palette_launch("ccvs_gif_palette", clips, clip_stride, frame_stride, b, t, h, w, 256, palette, table, used, workspace, hip_stream);
}

extern "C" int ccvs_gif_palette_n(const uint8_t* clips, long clip_stride, long frame_stride, int b, int t, int h, int w, int max_colours,
                                  uint8_t* palette, uint8_t* table, int* used, void* workspace, void* hip_stream) {
    const char* who = "ccvs_gif_palette_n";
    CCVS_REQUIRE(max_colours >= 2 && max_colours <= 256, "%s: max_colours %d outside 2 .. 256", who, max_colours);
    return gif_palette_launch(who, clips, clip_stride, frame_stride, b, t, h, w, max_colours, palette, table, used, workspace, hip_stream);
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

// ---- changed-rectangle frames (include/ccvs_hip_output_gif_delta.h).  Candidate 2 f of frame f is the full
// frame, candidate 2 f + 1 the rectangle of what changed against the frame before (none for a clip's first frame); each has the
// full frame's number of band slots, of which a rectangle uses its own first ones.
//   rect     a workgroup per frame: the bounding rectangle of the indices that differ from the frame before;
//   code     a wave per band of a candidate, over its rectangle; the rectangle's unchanged indices are GIF_TRANSPARENT;
//   scan     per frame the shorter candidate, its rectangle and size; the frames' offsets;
//   stitch   as above, of the chosen candidate's words.
struct GifDeltaArgs {
    const uint8_t* clips;
    long clip_stride, frame_stride;
    int t, n, h, w, band_rows, nb;   // band_rows as the caller gave it (0: by each rectangle's width); nb: band slots per candidate
    long wstride;
    const uint8_t* table;
    uint8_t* stream;
    long capacity;
    long* offsets;
    int* rects;                      // [n][4] the written candidate's x0, y0, rw, rh
    int* drect;                      // [n][4] the changed rectangle (frames after a clip's first)
    int* choice;                     // [n] 1: the rectangle is written
    long* bitoff;                    // [2 n][nb + 1]
    long* fsize;                     // [n]
    unsigned* words;                 // [2 n][nb][wstride]
};

__device__ __forceinline__ const uint8_t* gif_frame(const GifDeltaArgs& a, long f) {
    return a.clips + (f / a.t) * a.clip_stride + (f % a.t) * a.frame_stride;
}
__device__ __forceinline__ GifRect gif_candidate_rect(const GifDeltaArgs& a, long cand) {
    if (!(cand & 1)) return gif_full_rect(a.h, a.w);
    const int* r = a.drect + 4 * (cand >> 1);
    GifRect out = {r[0], r[1], r[2], r[3]};
    return out;
}
// ... for a wave that codes one band: named wave-uniform, so that the band's arithmetic stays on the scalar unit
__device__ __forceinline__ GifRect gif_uniform_rect(const GifRect& r) {
    GifRect out = {(int)GIF_U(r.x0), (int)GIF_U(r.y0), (int)GIF_U(r.rw), (int)GIF_U(r.rh)};
    return out;
}

__global__ __launch_bounds__(GIF_THREADS) void gif_rect_kernel(GifDeltaArgs a) {
    __shared__ int s_box[GIF_THREADS / WAVE][4];
    const long hw = (long)a.h * a.w;
    const long items = (hw + GIF_HIST_RUN - 1) / GIF_HIST_RUN;
    for (long f = blockIdx.x; f < a.n; f += gridDim.x) {
        if (f % a.t == 0) continue;                             // (the same in every thread)
        const uint8_t* cur = gif_frame(a, f);
        const uint8_t* prev = gif_frame(a, f - 1);
        const uint8_t* table = a.table + (f / a.t) * GIF_NBINS;
        int x_min = a.w, x_max = -1, y_min = a.h, y_max = -1;
        for (long it = threadIdx.x; it < items; it += GIF_THREADS) {
            const long p0 = it * GIF_HIST_RUN, p1 = p0 + GIF_HIST_RUN < hw ? p0 + GIF_HIST_RUN : hw;
            int y = (int)(p0 / a.w), x = (int)(p0 % a.w);
            for (long p = p0; p < p1; ++p) {
                if (table[gif_bin(cur + 3 * p)] != table[gif_bin(prev + 3 * p)]) {
                    x_min = min(x_min, x);
                    x_max = max(x_max, x);
                    y_min = min(y_min, y);
                    y_max = max(y_max, y);
                }
                if (++x == a.w) {
                    x = 0;
                    ++y;
                }
            }
        }
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) {
            x_min = min(x_min, __shfl_xor(x_min, o, WAVE));
            x_max = max(x_max, __shfl_xor(x_max, o, WAVE));
            y_min = min(y_min, __shfl_xor(y_min, o, WAVE));
            y_max = max(y_max, __shfl_xor(y_max, o, WAVE));
        }
        if (threadIdx.x % WAVE == 0) {
            int* box = s_box[threadIdx.x / WAVE];
            box[0] = x_min; box[1] = x_max; box[2] = y_min; box[3] = y_max;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int k = 1; k < GIF_THREADS / WAVE; ++k) {
                x_min = min(x_min, s_box[k][0]);
                x_max = max(x_max, s_box[k][1]);
                y_min = min(y_min, s_box[k][2]);
                y_max = max(y_max, s_box[k][3]);
            }
            const GifRect r = gif_changed_rect(x_min, x_max, y_min, y_max);
            int* out = a.drect + 4 * f;
            out[0] = r.x0; out[1] = r.y0; out[2] = r.rw; out[3] = r.rh;
        }
        __syncthreads();                                        // the LDS is the next frame's too
    }
}

// code: a wave per band slot of a candidate
__global__ __launch_bounds__(WAVE) void gif_code_rect_kernel(GifDeltaArgs a) {
    __shared__ unsigned s_hash[GIF_SLOTS];
    __shared__ uint8_t s_idx[GIF_CHUNK];
    const int lane = threadIdx.x;
    const long units = 2L * a.n * a.nb;
    for (long unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const long cand = unit / a.nb, f = cand >> 1;
        const int b = (int)(unit % a.nb);
        const bool mask = cand & 1;                             // against the frame before
        if (mask && f % a.t == 0) continue;                     // (every `continue` is the same in every lane)
        const GifRect r = gif_uniform_rect(gif_candidate_rect(a, cand));
        const int nbr = (int)gif_bands(r.rh, r.rw, a.band_rows);
        if (b >= nbr) continue;
        const int r0 = gif_rect_band_first(r, a.band_rows, b);
        const long L = (long)gif_rect_band_count(r, a.band_rows, b) * r.rw;
        const uint8_t* src = gif_frame(a, f);
        const uint8_t* table = a.table + (f / a.t) * GIF_NBINS;
        for (int i = lane; i < GIF_SLOTS; i += WAVE) s_hash[i] = GIF_EMPTY;
        GifCoder s;
        gif_start(s, a.words + unit * a.wstride, b == 0, lane == 0);
        for (long c0 = 0; c0 < L; c0 += GIF_CHUNK) {
            const int n = (int)(L - c0 < GIF_CHUNK ? L - c0 : GIF_CHUNK);
            __syncthreads();                                    // the chunk before is coded, the hash is empty
            for (int i = lane; i < n; i += WAVE) {
                const long p = gif_rect_pixel(r, a.w, r0, c0 + i);
                uint8_t v = table[gif_bin(src + 3 * p)];
                if (mask && table[gif_bin(src - a.frame_stride + 3 * p)] == v) v = GIF_TRANSPARENT;
                s_idx[i] = v;
            }
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
        const long bits = gif_finish(s, b == nbr - 1);
        if (lane == 0) a.bitoff[cand * (a.nb + 1) + b + 1] = bits;
        __syncthreads();
    }
}

// a candidate's band sizes turned into bit positions; returns its payload's bytes
__device__ __forceinline__ long gif_scan_candidate(const GifDeltaArgs& a, long cand, const GifRect& r) {
    const int nbr = (int)gif_bands(r.rh, r.rw, a.band_rows);
    long* off = a.bitoff + cand * (a.nb + 1);
    long run = 0;
    off[0] = 0;
    for (int b = 1; b <= nbr; ++b) {
        run += off[b];
        off[b] = run;
    }
    return gif_payload_bytes((run + 7) >> 3);
}

// scan: one workgroup.  Per frame both candidates' band positions and payload sizes, the choice and its rectangle; then the offsets
__global__ __launch_bounds__(GIF_THREADS) void gif_scan_delta_kernel(GifDeltaArgs a) {
    __shared__ long s_sum[GIF_THREADS];
    const int tid = threadIdx.x;
    for (long f = tid; f < a.n; f += GIF_THREADS) {
        GifRect rect = gif_full_rect(a.h, a.w);
        long size = gif_scan_candidate(a, 2 * f, rect);
        int pick = 0;
        if (f % a.t != 0) {
            const GifRect drect = gif_candidate_rect(a, 2 * f + 1);
            const long dsize = gif_scan_candidate(a, 2 * f + 1, drect);
            if (dsize < size) {
                pick = 1;
                size = dsize;
                rect = drect;
            }
        }
        a.choice[f] = pick;
        a.fsize[f] = size;
        int* out = a.rects + 4 * f;
        out[0] = rect.x0; out[1] = rect.y0; out[2] = rect.rw; out[3] = rect.rh;
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

__global__ __launch_bounds__(GIF_THREADS) void gif_stitch_delta_kernel(GifDeltaArgs a, long per_frame) {
    const long blocks = per_frame * a.n;
    for (long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
        const long f = blk / per_frame;
        const long j = (blk % per_frame) * GIF_THREADS + threadIdx.x;
        const long cand = 2 * f + a.choice[f];
        const int* r = a.rects + 4 * f;
        const int nbr = (int)gif_bands(r[3], r[2], a.band_rows);
        const long* bitoff = a.bitoff + cand * (a.nb + 1);
        const long data = (bitoff[nbr] + 7) >> 3;
        if (j >= data) continue;
        const long base = a.offsets[f];
        const unsigned byte = gif_data_byte(a.words + cand * a.nb * a.wstride, a.wstride, bitoff, nbr, j);
        const auto store = [&](long pos, unsigned v) {
            if (pos < a.capacity) a.stream[pos] = (uint8_t)v;
        };
        store(base + gif_data_pos(j), byte);
        if (j % 255 == 0) store(base + gif_data_pos(j) - 1, gif_block_len(data, j));
        if (j == 0) store(base, 8u);                            // the LZW minimum code size
        if (j == data - 1) store(base + gif_payload_bytes(data) - 1, 0u);
    }
}

// the workspace behind the palette's bins: the changed rectangles, the choices, both candidates' band positions, the frames' sizes, the
// bands' bits
static inline size_t gif_delta_tables_bytes(size_t n, size_t nb) { return n * 16 + gif_align8(n * 4) + 2 * n * (nb + 1) * 8 + n * 8; }

extern "C" size_t ccvs_gif_delta_workspace_bytes(int b, int t, int h, int w, int band_rows) {
    if (b < 1 || t < 1 || !gif_shape_ok((long)b * t, h, w, band_rows)) return 0;
    const size_t n = (size_t)b * t, nb = (size_t)gif_bands(h, w, band_rows);
    return (size_t)b * 4 * GIF_NBINS * 8 + gif_delta_tables_bytes(n, nb) +
           gif_align8(2 * n * nb * (size_t)gif_band_words(gif_rect_band_max(h, w, band_rows)) * 4);
}

extern "C" int ccvs_gif_encode_delta(const uint8_t* clips, long clip_stride, long frame_stride, int b, int t, int h, int w, int band_rows,
                                     const uint8_t* table, uint8_t* stream, long capacity, long* offsets, int* rects, void* workspace,
                                     void* hip_stream) {
    const char* who = "ccvs_gif_encode_delta";
    GIF_REQUIRE_CLIPS(who);
    CCVS_REQUIRE(band_rows >= 0, "%s: band_rows %d is negative", who, band_rows);
    CCVS_REQUIRE(gif_shape_ok((long)b * t, h, w, band_rows), "%s: band_rows %d makes a band of 2^24 indices or more", who, band_rows);
    CCVS_REQUIRE(capacity >= 0, "%s: negative capacity", who);
    CCVS_REQUIRE(clips && table && offsets && rects && workspace && (stream || capacity == 0),
                 "%s: null clips, table, stream, offsets, rects or workspace", who);
    GifDeltaArgs a;
    a.clips = clips; a.clip_stride = clip_stride; a.frame_stride = frame_stride;
    a.t = t; a.n = b * t; a.h = h; a.w = w;
    a.band_rows = band_rows;
    a.nb = (int)gif_bands(h, w, band_rows);
    a.wstride = gif_band_words(gif_rect_band_max(h, w, band_rows));
    a.table = table; a.stream = stream; a.capacity = capacity; a.offsets = offsets; a.rects = rects;
    char* p = (char*)workspace + (size_t)b * 4 * GIF_NBINS * 8;    // (behind the palette's bins)
    a.drect = (int*)p;                  p += 16 * (size_t)a.n;
    a.choice = (int*)p;                 p += gif_align8(4 * (size_t)a.n);
    a.bitoff = (long*)p;                p += 8 * 2 * (size_t)a.n * (a.nb + 1);
    a.fsize = (long*)p;                 p += 8 * (size_t)a.n;
    a.words = (unsigned*)p;
    hipStream_t st = (hipStream_t)hip_stream;
    const long rows = gif_band_rows(w, band_rows);                 // no payload is written that is longer than the full frame's can be
    const long full = rows < h ? rows : h, tail = h - (long)(a.nb - 1) * rows;
    const long data_max = ((a.nb - 1) * gif_band_bits(full * w) + gif_band_bits(tail * w) + 7) >> 3;
    const long per_frame = (data_max + GIF_THREADS - 1) / GIF_THREADS;
    hipLaunchKernelGGL(gif_rect_kernel, dim3(limited_grid(a.n, hip_stream, 8)), dim3(GIF_THREADS), 0, st, a);
    hipLaunchKernelGGL(gif_code_rect_kernel, dim3(limited_grid(2L * a.n * a.nb, hip_stream, 4)), dim3(WAVE), 0, st, a);
    hipLaunchKernelGGL(gif_scan_delta_kernel, dim3(1), dim3(GIF_THREADS), 0, st, a);
    hipLaunchKernelGGL(gif_stitch_delta_kernel, dim3(limited_grid(per_frame * a.n, hip_stream, 8)), dim3(GIF_THREADS), 0, st, a, per_frame);
    CCVS_CHECK_LAUNCH(who);
    return CCVS_OK;
}

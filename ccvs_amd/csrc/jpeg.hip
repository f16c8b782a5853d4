// The output stage (include/ccvs_hip_output.h): uint8 frames [N, H, W, 3] -> baseline JPEG scans whose bytes
// are libjpeg's, bit for bit.  All arithmetic is integer.  The restart interval (1 .. 32 MCUs of 8 x 8 pixels) is the unit of parallel
// work: an interval is byte-aligned and predicts its DC values from nothing outside it, so one workgroup encodes one interval.  Where
// an interval's bytes go depends on the sizes of all the intervals before it, so the kernel runs twice: a first pass writes every
// interval's size, one workgroup scans the sizes into offsets (and the frames' offsets), a second pass encodes again and writes at the
// final offsets.  No atomic decides an offset; the LDS atomics below only OR disjoint bits into shared words.
// The kernel is a template over the sampling (include/ccvs_hip_output_sampled.h): 0 is the kernel above word
// for word; 1 (4:2:2) and 2 (4:2:0) have MCUs of 16 x 8 / 16 x 16 pixels and 4 / 6 blocks, stage finished planes instead of raw RGB and
// know dummy blocks.  An interval never has more than 96 blocks, so every buffer keeps its size.
// It is a template over what it does with the coefficients, too (include/ccvs_hip_output_optimized.h): code them
// with the Annex K tables (the two encoders above, unchanged), count their symbols per frame, or code them with that frame's own tables
// -- libjpeg's optimize_coding: gather, jpeg_gen_optimal_table (jpeg_tables_kernel below), then the same two passes.
#include "common.h"

#define JP_THREADS 128
#define JP_MAXR 32
#define JP_MAXBLK (3 * JP_MAXR)
// worst case of a block: a chrominance DC of category 11 (11 + 11 bits) and 63 AC coefficients of category 10 behind 16-bit codes
// (26 bits each) = 1660 bits, about 208 bytes: 52 words.  put_bits refuses any word beyond the buffer whatever the data.
#define JP_BLK_WORDS 52
#define JP_WORDS (JP_MAXBLK * JP_BLK_WORDS + 2)
#define JP_CSTRIDE 66   // int16 coefficients of a block in LDS: 33 dwords, so that the lanes' rows fall on different banks

// ---- the Annex K tables
static const unsigned char k_base_q[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

struct HuffSpec {
    unsigned char bits[16];   // codes of length 1 .. 16
    unsigned char vals[162];  // the symbols in code order
};
static constexpr HuffSpec k_dc_luma = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
static constexpr HuffSpec k_dc_chroma = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
static constexpr HuffSpec k_ac_luma = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};
static constexpr HuffSpec k_ac_chroma = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

// The code of every symbol as (code << 5) | length (length 0: the table has no such symbol), derived from the specification's
// (bits, vals) form at compile time (T.81 Annex C): [0] DC luminance, [1] DC chrominance, [2] AC luminance, [3] AC chrominance.
struct HuffCodes { unsigned t[4][256]; };
static constexpr HuffCodes make_huff_codes() {
    HuffCodes h = {};
    const HuffSpec* specs[4] = {&k_dc_luma, &k_dc_chroma, &k_ac_luma, &k_ac_chroma};
    for (int s = 0; s < 4; ++s) {
        unsigned code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < specs[s]->bits[len - 1]; ++i) h.t[s][specs[s]->vals[k++]] = (code++ << 5) | (unsigned)len;
            code <<= 1;
        }
    }
    return h;
}
__constant__ HuffCodes c_huff = make_huff_codes();

// zigzag position -> natural (row-major) index
static constexpr int k_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct JpegArgs {
    const uint8_t* rgb;
    long frame_stride;
    int h, w, R, mcux, nmcu, nI;   // per frame: MCUs per row, MCUs, intervals
    int wby, hby;                  // the luminance component's width and height in blocks (subsampled forms: blocks beyond are dummies)
    long T;                        // intervals of all frames
    uint8_t* stream;
    long capacity;
    int* sizes;                    // [T]: bytes of every interval, its RSTn marker included
    const long* ioff;              // [T]: where every interval starts in `stream` (second pass)
    int write;                     // 0: the first pass (sizes), 1: the second (bytes)
    int aligned;                   // every 4-byte group of a row that lies inside the row is dword-aligned
    unsigned short qd[2][64];      // 8 x the quantiser tables (natural order): [0] luminance, [1] chrominance
    unsigned* counts;              // JP_GATHER: [n][4][257], how often every frame's scan emits every symbol (the tables in DHT order)
    const unsigned* emit;          // JP_FRAME_TABLES: [n][4][256], every frame's codes as c_huff holds the constant ones
};
// what jpeg_interval_kernel does with the coefficients
#define JP_STANDARD 0       // codes them with the Annex K tables
#define JP_GATHER 1         // counts the symbols it would emit, per frame
#define JP_FRAME_TABLES 2   // codes them with the tables of the interval's frame
#define JP_SPEC_BYTES 272   // a table for the host: bits[16] + huffval[256]

// ---- libjpeg's jfdctint.c ("islow"): one 1-D pass over d[0], d[S], ..., d[7 S].  FIRST: the row pass (results scaled up by
// PASS1_BITS); else the column pass (that scaling and the pass's own factor of 8 removed again -- the block stays 8 x the true DCT).
#define JP_CONST_BITS 13
#define JP_PASS1_BITS 2
#define JP_FIX_0_298631336 2446
#define JP_FIX_0_390180644 3196
#define JP_FIX_0_541196100 4433
#define JP_FIX_0_765366865 6270
#define JP_FIX_0_899976223 7373
#define JP_FIX_1_175875602 9633
#define JP_FIX_1_501321110 12299
#define JP_FIX_1_847759065 15137
#define JP_FIX_1_961570560 16069
#define JP_FIX_2_053119869 16819
#define JP_FIX_2_562915447 20995
#define JP_FIX_3_072711026 25172
__device__ __forceinline__ int jp_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

template <bool FIRST, int S>
__device__ __forceinline__ void fdct_pass(int* d) {
    const int tmp0 = d[0] + d[7 * S], tmp7 = d[0] - d[7 * S];
    const int tmp1 = d[S] + d[6 * S], tmp6 = d[S] - d[6 * S];
    const int tmp2 = d[2 * S] + d[5 * S], tmp5 = d[2 * S] - d[5 * S];
    const int tmp3 = d[3 * S] + d[4 * S], tmp4 = d[3 * S] - d[4 * S];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    constexpr int N = FIRST ? JP_CONST_BITS - JP_PASS1_BITS : JP_CONST_BITS + JP_PASS1_BITS;
    if (FIRST) {
        d[0] = (tmp10 + tmp11) * (1 << JP_PASS1_BITS);
        d[4 * S] = (tmp10 - tmp11) * (1 << JP_PASS1_BITS);
    } else {
        d[0] = jp_descale(tmp10 + tmp11, JP_PASS1_BITS);
        d[4 * S] = jp_descale(tmp10 - tmp11, JP_PASS1_BITS);
    }
    int z1 = (tmp12 + tmp13) * JP_FIX_0_541196100;
    d[2 * S] = jp_descale(z1 + tmp13 * JP_FIX_0_765366865, N);
    d[6 * S] = jp_descale(z1 + tmp12 * (-JP_FIX_1_847759065), N);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * JP_FIX_1_175875602;
    const int t4 = tmp4 * JP_FIX_0_298631336, t5 = tmp5 * JP_FIX_2_053119869, t6 = tmp6 * JP_FIX_3_072711026, t7 = tmp7 * JP_FIX_1_501321110;
    z1 *= -JP_FIX_0_899976223;
    z2 *= -JP_FIX_2_562915447;
    z3 = z3 * (-JP_FIX_1_961570560) + z5;
    z4 = z4 * (-JP_FIX_0_390180644) + z5;
    d[7 * S] = jp_descale(t4 + z1 + z3, N);
    d[5 * S] = jp_descale(t5 + z2 + z4, N);
    d[3 * S] = jp_descale(t6 + z2 + z3, N);
    d[S] = jp_descale(t7 + z1 + z4, N);
}

// ---- the bit stream of an interval in LDS: word k holds bytes 4k .. 4k + 3, the first byte in the top bits (JPEG sends the most
// significant bit first).  Blocks of different lanes meet inside a word, hence the OR; the words are zero before the first one.
__device__ __forceinline__ void put_bits(unsigned* words, int& pos, unsigned v, int len) {   // v < 2^len, len <= 27
    if (len > 0) {
        const int wi = pos >> 5;
        const unsigned long long x = (unsigned long long)v << (64 - len - (pos & 31));
        if (wi + 1 < JP_WORDS) {
            atomicOr(&words[wi], (unsigned)(x >> 32));
            if ((unsigned)x) atomicOr(&words[wi + 1], (unsigned)x);
        }
    }
    pos += len;
}
__device__ __forceinline__ int bit_length(int v) { return 32 - __clz(v); }   // of v >= 0

// One symbol of table `t` and the `cat` bits behind it.  JP_SIZE: only counts the bits; JP_EMIT: writes them; JP_COUNT: `t` is the
// table's histogram (in LDS) and the symbol is counted.
#define JP_SIZE 0
#define JP_EMIT 1
#define JP_COUNT 2
template <int OP>
__device__ __forceinline__ void code_symbol(const unsigned* t, int sym, unsigned bits, int cat, unsigned* words, int& pos) {
    if (OP == JP_COUNT) {
        atomicAdd(const_cast<unsigned*>(t) + sym, 1u);
    } else {
        const unsigned e = t[sym];
        if (OP == JP_EMIT) put_bits(words, pos, ((e >> 5) << cat) | bits, (int)(e & 31u) + cat);
        else pos += (int)(e & 31u) + cat;
    }
}

// One block: the DC difference and the 63 AC coefficients (zigzag order, `coef[1 .. 63]`).  Returns the bit position behind the block
// (JP_COUNT: `pos` as it came).
template <int OP>
__device__ __forceinline__ int code_block(const short* coef, int diff, const unsigned* dc, const unsigned* ac, unsigned* words, int pos) {
    {
        const int a = diff < 0 ? -diff : diff;
        int cat = bit_length(a);
        cat = cat > 11 ? 11 : cat;
        code_symbol<OP>(dc, cat, (unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1u), cat, words, pos);
    }
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = coef[k];
        if (v == 0) {
            ++run;
            continue;
        }
        while (run > 15) {   // ZRL: sixteen zeros
            code_symbol<OP>(ac, 0xF0, 0u, 0, words, pos);
            run -= 16;
        }
        const int a = v < 0 ? -v : v;
        int cat = bit_length(a);
        cat = cat > 10 ? 10 : cat;
        code_symbol<OP>(ac, (run << 4) | cat, (unsigned)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u), cat, words, pos);
        run = 0;
    }
    if (run > 0) code_symbol<OP>(ac, 0x00, 0u, 0, words, pos);   // EOB, only when the block ends in zeros
    return pos;
}

// The two DCT passes of a block in registers and the quantiser: the DC value to `dc`, the AC coefficients in zigzag order to coef[1 .. 63].
__device__ __forceinline__ void transform_block(int* d, const unsigned short* qd, int* dc, short* coef) {
#pragma unroll
    for (int r = 0; r < 8; ++r) fdct_pass<true, 1>(d + 8 * r);
#pragma unroll
    for (int c = 0; c < 8; ++c) fdct_pass<false, 8>(d + c);
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        const int nat = k_zigzag[k];
        const int q = qd[nat], v = d[nat];
        const int m = ((v < 0 ? -v : v) + (q >> 1)) / q;
        const int s = v < 0 ? -m : m;
        if (k == 0) *dc = s;
        else coef[k] = (short)s;
    }
}

// Sampling S (1: 4:2:2, 2: 4:2:0): whether luminance block k (raster order inside the MCU) of MCU (mx, my) lies outside the component.
template <int S>
__device__ __forceinline__ bool dummy_block(const JpegArgs& a, int mx, int my, int k) {
    return k < 2 * S && (2 * mx + (k & 1) >= a.wby || (S == 2 && 2 * my + (k >> 1) >= a.hby));
}
// ... and the block of the interval whose DC value block t of the interval carries: itself, or for a dummy the nearest real block
// before it in its MCU (block 0 of an MCU is always real).
template <int S>
__device__ __forceinline__ int dc_source(const JpegArgs& a, int first, int t) {
    constexpr int BPM = 2 * S + 2;
    const int m = t / BPM, g = first + m, my = g / a.mcux, mx = g - my * a.mcux;
    int k = t - m * BPM;
    while (dummy_block<S>(a, mx, my, k)) --k;
    return m * BPM + k;
}

// JP_GATHER: the frame's histograms, kept in s_huff, go to a.counts with integer atomics (sums of integers: the same on every run).
// The slots of s_huff are DC luminance, DC chrominance, AC luminance, AC chrominance; a.counts has the DHT order (AC luminance second).
__device__ __forceinline__ void flush_counts(unsigned* s_huff, unsigned* counts, long frame, int tid) {
    for (int i = tid; i < 4 * 256; i += JP_THREADS) {
        const unsigned c = s_huff[i];
        const int slot = i >> 8, t = slot == 1 ? 2 : (slot == 2 ? 1 : slot);
        if (c) atomicAdd(&counts[(frame * 4 + t) * 257 + (i & 255)], c);
        s_huff[i] = 0;
    }
}

template <int S, int M>
__global__ __launch_bounds__(JP_THREADS) void jpeg_interval_kernel(JpegArgs a) {
    constexpr int BPM = S == 0 ? 3 : 2 * S + 2;           // blocks per MCU: Y Cb Cr, Y0 Y1 Cb Cr, Y00 Y01 Y10 Y11 Cb Cr
    constexpr int VS = S == 2 ? 2 : 1;                    // luminance rows per chrominance row
    // S = 0: the interval's MCUs as [MCU][row][24 bytes RGB]; else finished samples, [block in stream order][64 bytes]: 6 KB either way
    __shared__ unsigned s_px[JP_MAXR * 48];
    __shared__ short s_coef[JP_MAXBLK * JP_CSTRIDE];      // quantised coefficients in zigzag order, 12.4 KB
    __shared__ unsigned s_words[JP_WORDS];                // the bit stream before byte stuffing, 19.5 KB
    __shared__ unsigned s_huff[4 * 256];
    __shared__ unsigned short s_qd[2 * 64];
    __shared__ int s_dc[JP_MAXBLK], s_cnt[JP_MAXBLK], s_ff[JP_THREADS];
    const int tid = threadIdx.x;
    if constexpr (M == JP_STANDARD)
        for (int i = tid; i < 4 * 256; i += JP_THREADS) s_huff[i] = c_huff.t[i >> 8][i & 255];
    if constexpr (M == JP_GATHER)
        for (int i = tid; i < 4 * 256; i += JP_THREADS) s_huff[i] = 0;
    long held = -1;   // JP_GATHER / JP_FRAME_TABLES: the frame whose histograms / codes s_huff holds
    if (tid < 128) s_qd[tid] = a.qd[tid >> 6][tid & 63];
    const int mcu = tid / BPM;
    const int comp = S == 0 ? tid % 3 : (tid - mcu * BPM < BPM - 2 ? 0 : tid - mcu * BPM - (BPM - 3));
    for (long iv = blockIdx.x; iv < a.T; iv += gridDim.x) {
        const long n = iv / a.nI;
        const int ii = (int)(iv - n * a.nI);
        const int first = ii * a.R;
        const int nm = a.nmcu - first < a.R ? a.nmcu - first : a.R;   // MCUs of this interval
        const int nb = BPM * nm;                                       // its blocks, in stream order: block t = (MCU t / BPM, block t % BPM of it)
        const uint8_t* frame = a.rgb + n * a.frame_stride;
        // (the barrier at the loop's end lies behind s_huff's last use, the one behind step 1 before its next)
        if constexpr (M != JP_STANDARD)
            if (n != held) {
                if constexpr (M == JP_GATHER) {
                    if (held >= 0) flush_counts(s_huff, a.counts, held, tid);
                } else {
                    for (int i = tid; i < 4 * 256; i += JP_THREADS) s_huff[i] = a.emit[n * 1024 + i];
                }
                held = n;
            }
        // 1. the MCUs' pixels, a dword at a time; rows below the frame and pixels right of it replicate the last row / pixel
        if constexpr (S == 0)
        for (int it = tid; it < nm * 48; it += JP_THREADS) {
            const int m = it / 48, rem = it - m * 48, row = rem / 6, k = rem - row * 6;
            const int g = first + m, my = g / a.mcux, mx = g - my * a.mcux;
            const int y = my * 8 + row < a.h ? my * 8 + row : a.h - 1;
            const uint8_t* rp = frame + (long)y * a.w * 3;
            const int xb = mx * 24 + 4 * k;
            unsigned v;
            if (a.aligned && xb + 3 < 3 * a.w) {
                v = *(const unsigned*)(rp + xb);
            } else {
                v = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int b = 4 * k + j, ch = b % 3;
                    const int px = mx * 8 + b / 3 < a.w ? mx * 8 + b / 3 : a.w - 1;
                    v |= (unsigned)rp[px * 3 + ch] << (8 * j);
                }
            }
            s_px[it] = v;
        }
        // 1s. subsampled: a lane per chrominance sample.  It converts the 2 x VS pixels under it once, stores their Y and the box-filtered
        // Cb and Cr (bias by the output column's parity).  Columns right of the frame replicate the last one.  Rows: luminance replicates
        // the last row; chrominance replicates the last row up to a multiple of VS BEFORE the filter and the last FILTERED row below that.
        if constexpr (S != 0) {
            uint8_t* planes = (uint8_t*)s_px;
            const int last_crow = (a.h + VS - 1) / VS - 1;
            for (int it = tid; it < nm * 64; it += JP_THREADS) {
                const int m = it >> 6, cy = (it >> 3) & 7, cx = it & 7;
                const int g = first + m, my = g / a.mcux, mx = g - my * a.mcux;
                const int crow = my * 8 + cy < last_crow ? my * 8 + cy : last_crow;
                int cb = 0, cr = 0;
#pragma unroll
                for (int j = 0; j < VS; ++j) {
                    const int yl = VS * cy + j;                                                  // the luminance row inside the MCU
                    const int ysrc = my * 8 * VS + yl < a.h ? my * 8 * VS + yl : a.h - 1;
                    const int csrc = VS * crow + j < a.h ? VS * crow + j : a.h - 1;
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int xl = 2 * cx + i;
                        const int x = mx * 16 + xl < a.w ? mx * 16 + xl : a.w - 1;
                        const uint8_t* q = frame + ((long)csrc * a.w + x) * 3;
                        int r = q[0], gg = q[1], b = q[2];
                        cb += (-11059 * r - 21709 * gg + 32768 * b + (128 << 16) + 32767) >> 16;
                        cr += (32768 * r - 27439 * gg - 5329 * b + (128 << 16) + 32767) >> 16;
                        if (ysrc != csrc) {
                            q = frame + ((long)ysrc * a.w + x) * 3;
                            r = q[0], gg = q[1], b = q[2];
                        }
                        const int kb = (S == 2 ? (yl >> 3) * 2 : 0) + (xl >> 3);
                        planes[(m * BPM + kb) * 64 + (yl & 7) * 8 + (xl & 7)] = (uint8_t)((19595 * r + 38470 * gg + 7471 * b + 32768) >> 16);
                    }
                }
                const int bias = S == 2 ? 1 + (cx & 1) : (cx & 1);
                planes[(m * BPM + BPM - 2) * 64 + cy * 8 + cx] = (uint8_t)((cb + bias) >> S);
                planes[(m * BPM + BPM - 1) * 64 + cy * 8 + cx] = (uint8_t)((cr + bias) >> S);
            }
        }
        __syncthreads();
        // 2s. subsampled: a lane per block reads its 64 finished samples; a dummy block has no AC coefficients and is not transformed
        if constexpr (S != 0)
        if (tid < nb) {
            const int g = first + mcu, my = g / a.mcux, mx = g - my * a.mcux;
            if (dummy_block<S>(a, mx, my, tid - mcu * BPM)) {
                for (int k = 1; k < 64; ++k) s_coef[tid * JP_CSTRIDE + k] = 0;
            } else {
                const uint8_t* p = (const uint8_t*)s_px + tid * 64;
                int d[64];
#pragma unroll
                for (int i = 0; i < 64; ++i) d[i] = (int)p[i] - 128;
                transform_block(d, s_qd + (comp == 0 ? 0 : 64), &s_dc[tid], s_coef + tid * JP_CSTRIDE);
            }
        }
        // 2. a lane per block: colour conversion of its component, the two DCT passes in registers, the quantiser
        if constexpr (S == 0)
        if (tid < nb) {
            const int cr = comp == 0 ? 19595 : (comp == 1 ? -11059 : 32768);
            const int cg = comp == 0 ? 38470 : (comp == 1 ? -21709 : -27439);
            const int cb = comp == 0 ? 7471 : (comp == 1 ? 32768 : -5329);
            const int c0 = comp == 0 ? 32768 : (128 << 16) + 32767;
            const uint8_t* p = (const uint8_t*)s_px + mcu * 192;
            int d[64];
#pragma unroll
            for (int i = 0; i < 64; ++i) d[i] = ((cr * (int)p[3 * i] + cg * (int)p[3 * i + 1] + cb * (int)p[3 * i + 2] + c0) >> 16) - 128;
            transform_block(d, s_qd + (comp == 0 ? 0 : 64), &s_dc[tid], s_coef + tid * JP_CSTRIDE);
        }
        __syncthreads();
        // 3. every block's length in bits
        int diff = 0;
        const unsigned* dc = s_huff + (comp == 0 ? 0 : 256);
        const unsigned* ac = s_huff + (comp == 0 ? 512 : 768);
        if (tid < nb) {
            // the block before this one in its component: 3 blocks back for Y Cb Cr; subsampled, the luminance block before (the last one
            // of the MCU before lies 3 back as well) or the MCU before's chrominance block -- each read through dc_source, dummies included
            if constexpr (S == 0) {
                diff = s_dc[tid] - (tid >= 3 ? s_dc[tid - 3] : 0);
            } else {
                const int kb = tid - mcu * BPM;
                const int prev = comp != 0 ? tid - BPM : (kb > 0 ? tid - 1 : tid - 3);
                diff = s_dc[dc_source<S>(a, first, tid)] - (prev >= 0 ? s_dc[dc_source<S>(a, first, prev)] : 0);
            }
            if constexpr (M == JP_GATHER) code_block<JP_COUNT>(s_coef + tid * JP_CSTRIDE, diff, dc, ac, nullptr, 0);
            else s_cnt[tid] = code_block<JP_SIZE>(s_coef + tid * JP_CSTRIDE, diff, dc, ac, nullptr, 0);
        }
        __syncthreads();
        if constexpr (M == JP_GATHER) continue;   // counted; the barrier above stands for the one at the loop's end
        // 4. where every block starts; clear the words the interval takes
        int start = 0, total = 0;
        for (int j = 0; j < nb; ++j) {
            const int c = s_cnt[j];
            start += j < tid ? c : 0;
            total += c;
        }
        const int nbytes = (total + 7) >> 3;
        const int nwords = (nbytes + 3) >> 2;
        for (int i = tid; i < nwords && i < JP_WORDS; i += JP_THREADS) s_words[i] = 0;
        __syncthreads();
        // 5. the bits; the last byte is padded with ones
        if (tid < nb) {
            int pos = code_block<JP_EMIT>(s_coef + tid * JP_CSTRIDE, diff, dc, ac, s_words, start);
            if (tid == nb - 1) put_bits(s_words, pos, (1u << (8 * nbytes - total)) - 1u, 8 * nbytes - total);
        }
        __syncthreads();
        // 6. byte stuffing: a lane takes a run of consecutive bytes and counts its 0xFF bytes
        const int chunk = (nbytes + JP_THREADS - 1) / JP_THREADS;
        const int b0 = tid * chunk < nbytes ? tid * chunk : nbytes;
        const int b1 = b0 + chunk < nbytes ? b0 + chunk : nbytes;
        int ff = 0;
        for (int j = b0; j < b1; ++j) ff += ((s_words[j >> 2] >> (24 - 8 * (j & 3))) & 255u) == 255u;
        s_ff[tid] = ff;
        __syncthreads();
        int ff_before = 0, ff_total = 0;
        for (int j = 0; j < JP_THREADS; ++j) {
            const int c = s_ff[j];
            ff_before += j < tid ? c : 0;
            ff_total += c;
        }
        const int last = ii == a.nI - 1;   // no RSTn behind a frame's last interval
        if (!a.write) {
            if (tid == 0) a.sizes[iv] = nbytes + ff_total + (last ? 0 : 2);
        } else {
            // 7. the bytes at their final place; nothing at or beyond `capacity`
            const long base = a.ioff[iv];
            long o = base + b0 + ff_before;
            for (int j = b0; j < b1; ++j) {
                const unsigned byte = (s_words[j >> 2] >> (24 - 8 * (j & 3))) & 255u;
                if (o < a.capacity) a.stream[o] = (uint8_t)byte;
                ++o;
                if (byte == 255u) {
                    if (o < a.capacity) a.stream[o] = 0;
                    ++o;
                }
            }
            if (tid == 0 && !last) {
                const long r = base + nbytes + ff_total;
                if (r < a.capacity) a.stream[r] = 0xFF;
                if (r + 1 < a.capacity) a.stream[r + 1] = (uint8_t)(0xD0 + (ii & 7));
            }
        }
        __syncthreads();   // the LDS arrays are the next interval's too
    }
    if constexpr (M == JP_GATHER)
        if (held >= 0) flush_counts(s_huff, a.counts, held, tid);
}

// ---- exclusive scan of the intervals' sizes by one workgroup: a lane sums a run of consecutive intervals, the runs' sums are scanned
// through LDS, the lane walks its run again.  offsets[f] = where frame f's first interval starts; offsets[n] = the total.
#define JP_SCAN_THREADS 256
__global__ __launch_bounds__(JP_SCAN_THREADS) void jpeg_scan_kernel(const int* sizes, long* ioff, long* offsets, long T, int nI) {
    __shared__ long s_sum[JP_SCAN_THREADS];
    const int tid = threadIdx.x;
    const long chunk = (T + JP_SCAN_THREADS - 1) / JP_SCAN_THREADS;
    const long i0 = tid * chunk < T ? tid * chunk : T;
    const long i1 = i0 + chunk < T ? i0 + chunk : T;
    long sum = 0;
    for (long i = i0; i < i1; ++i) sum += sizes[i];
    s_sum[tid] = sum;
    __syncthreads();
    long run = 0, total = 0;
    for (int j = 0; j < JP_SCAN_THREADS; ++j) {
        const long c = s_sum[j];
        run += j < tid ? c : 0;
        total += c;
    }
    for (long i = i0; i < i1; ++i) {
        ioff[i] = run;
        if (i % nI == 0) offsets[i / nI] = run;
        run += sizes[i];
    }
    if (tid == 0) offsets[T / nI] = total;
}

// ---- libjpeg's jpeg_gen_optimal_table (jchuff.c) for one table of one frame: one wave per table, everything in LDS.
//   tree     symbol 256 with frequency 1 keeps the all-ones code unused.  The two smallest nonzero frequencies are merged until one is
//            left; among equals the LARGER symbol is taken (libjpeg scans upwards with `<=`).  libjpeg walks the two `others` chains and
//            adds 1 to every code size on them; a chain is the set of symbols under its head, so here every symbol knows its head
//            (s_head) and the lanes add 1 to those whose head is one of the two.
//   limit    the code sizes (up to 32) are counted into bits[] and brought down to 16 as T.81 K.2 does; one code of the longest length
//            goes (the pseudo-symbol's).
//   huffval  the symbols by ascending code size BEFORE limiting, then by value: a lane finds each of its symbols' rank by counting.
//   codes    canonical from bits[] (T.81 Annex C): the symbol at rank p has the code first[len] + p - (codes shorter than len).
// A histogram without a symbol gives an empty table; a tree deeper than 32, where libjpeg stops with an error (it takes millions of
// symbols in Fibonacci proportions), is counted as 32 deep.
#define JP_TBL_THREADS 64
#define JP_MAX_CLEN 32
__global__ __launch_bounds__(JP_TBL_THREADS) void jpeg_tables_kernel(const unsigned* counts, uint8_t* tables, unsigned* emit) {
    __shared__ unsigned s_freq[257];
    __shared__ int s_size[257], s_head[257], s_bits[JP_MAX_CLEN + 1], s_before[18], s_first[18];
    const int lane = threadIdx.x, frame = blockIdx.x >> 2, t = blockIdx.x & 3;
    for (int i = lane; i < 257; i += JP_TBL_THREADS) {
        s_freq[i] = i < 256 ? counts[(long)blockIdx.x * 257 + i] : 1u;
        s_size[i] = 0;
        s_head[i] = i;
    }
    if (lane <= JP_MAX_CLEN) s_bits[lane] = 0;
    __syncthreads();
    for (;;) {
        // the smallest key (frequency, then 65535 - symbol) among the nonzero frequencies, and the smallest but that one
        int c[2] = {-1, -1};
        for (int r = 0; r < 2; ++r) {
            unsigned long long key = ~0ull;
            for (int i = lane; i < 257; i += JP_TBL_THREADS) {
                const unsigned f = s_freq[i];
                const unsigned long long k = ((unsigned long long)f << 16) | (unsigned)(0xFFFF - i);
                if (f && i != c[0] && k < key) key = k;
            }
            for (int m = JP_TBL_THREADS / 2; m > 0; m >>= 1) {
                const unsigned long long o = __shfl_xor(key, m, JP_TBL_THREADS);
                key = o < key ? o : key;
            }
            if (key != ~0ull) c[r] = 0xFFFF - (int)(key & 0xFFFFu);
        }
        if (c[1] < 0) break;                               // (the same in every lane)
        __syncthreads();
        if (lane == 0) {
            s_freq[c[0]] += s_freq[c[1]];
            s_freq[c[1]] = 0;
        }
        for (int i = lane; i < 257; i += JP_TBL_THREADS) {
            const int h = s_head[i];
            if (h == c[0] || h == c[1]) {
                ++s_size[i];
                s_head[i] = c[0];
            }
        }
        __syncthreads();
    }
    for (int i = lane; i < 257; i += JP_TBL_THREADS) {
        const int sz = s_size[i];
        if (sz) atomicAdd(&s_bits[sz < JP_MAX_CLEN ? sz : JP_MAX_CLEN], 1);
    }
    __syncthreads();
    if (lane == 0) {
        int i;
        for (i = JP_MAX_CLEN; i > 16; --i)
            while (s_bits[i] > 0) {
                int j = i - 2;
                while (j > 0 && s_bits[j] == 0) --j;
                s_bits[i] -= 2;
                s_bits[i - 1] += 1;
                s_bits[j + 1] += 2;
                s_bits[j] -= 1;
            }
        while (i > 0 && s_bits[i] == 0) --i;
        if (i > 0) --s_bits[i];
        int code = 0, k = 0;
        for (int len = 1; len <= 16; ++len) {
            s_before[len] = k;
            s_first[len] = code;
            k += s_bits[len];
            code = (code + s_bits[len]) << 1;
        }
        s_before[17] = k;
    }
    __syncthreads();
    uint8_t* spec = tables + (long)blockIdx.x * JP_SPEC_BYTES;
    const int slot = t == 1 ? 2 : (t == 2 ? 1 : t);        // jpeg_interval_kernel's order of the four tables
    unsigned* codes = emit + ((long)frame * 4 + slot) * 256;
    const int total = s_before[17];
    if (lane < 16) spec[lane] = (uint8_t)s_bits[lane + 1];
    for (int p = total + lane; p < 256; p += JP_TBL_THREADS) spec[16 + p] = 0;
    for (int j = lane; j < 256; j += JP_TBL_THREADS) {
        const int sz = s_size[j];
        unsigned e = 0;
        if (sz) {
            int p = 0;
            for (int k = 0; k < 256; ++k) {
                const int o = s_size[k];
                p += o && (o < sz || (o == sz && k < j));
            }
            int len = 1;
            while (len < 16 && p >= s_before[len + 1]) ++len;
            spec[16 + p] = (uint8_t)j;
            e = ((unsigned)(s_first[len] + p - s_before[len]) << 5) | (unsigned)len;
        }
        codes[j] = e;
    }
}

// MCUs are 8 x 8, 16 x 8 or 16 x 16 pixels; an interval holds at most JP_MAXBLK blocks: 32, 24 or 16 MCUs
static inline int jpeg_max_restart(int sampling) { return JP_MAXBLK / (sampling == 0 ? 3 : 2 * sampling + 2); }
static inline long jpeg_intervals(int n, int h, int w, int sampling, int R) {
    const int mw = sampling ? 16 : 8, mh = sampling == 2 ? 16 : 8;
    const long nmcu = (long)((w + mw - 1) / mw) * ((h + mh - 1) / mh);
    return (long)n * ((nmcu + R - 1) / R);
}
static inline bool jpeg_shape_ok(int n, int h, int w, int sampling, int R) {
    return n >= 1 && h >= 1 && h <= 65535 && w >= 1 && w <= 65535 && sampling >= 0 && sampling <= 2 && R >= 1 && R <= jpeg_max_restart(sampling);
}
static inline size_t jpeg_workspace(int n, int h, int w, int sampling, int R) {
    if (!jpeg_shape_ok(n, h, w, sampling, R)) return 0;
    const size_t T = (size_t)jpeg_intervals(n, h, w, sampling, R);
    return 8 * T + ((4 * T + 7) & ~(size_t)7);   // long ioff[T], then int sizes[T]
}

// The optimised form keeps, behind that, the frames' histograms (unsigned [n][4][257]) and their codes (unsigned [n][4][256]).
static inline size_t jpeg_optimized_workspace(int n, int h, int w, int sampling, int R) {
    const size_t base = jpeg_workspace(n, h, w, sampling, R);
    return base ? base + (size_t)n * 4 * (257 + 256) * 4 : 0;
}

template <int M>
static void (*jpeg_kernel(int sampling))(JpegArgs) {
    return sampling == 0 ? jpeg_interval_kernel<0, M> : (sampling == 1 ? jpeg_interval_kernel<1, M> : jpeg_interval_kernel<2, M>);
}

// `who`: the entry point's name for the messages; `sampling` has been checked by the caller.  tables: null for the Annex K tables, else
// where the frames' own tables go (uint8 [n][4][JP_SPEC_BYTES]).
static int jpeg_encode(const char* who, const uint8_t* rgb, long frame_stride, int n, int h, int w, int quality, int sampling, int restart_mcus,
                       uint8_t* stream, long capacity, long* offsets, uint8_t* tables, void* workspace, void* hip_stream) {
    const int maxr = jpeg_max_restart(sampling);
    CCVS_REQUIRE(quality >= 1 && quality <= 100, "%s: quality %d outside 1 .. 100", who, quality);
    CCVS_REQUIRE(restart_mcus >= 1 && restart_mcus <= maxr, "%s: restart interval %d outside 1 .. %d MCUs", who, restart_mcus, maxr);
    CCVS_REQUIRE(h >= 1 && h <= 65535 && w >= 1 && w <= 65535, "%s: frame size %d x %d outside 1 .. 65535", who, h, w);
    CCVS_REQUIRE(n >= 1 && frame_stride >= 0 && capacity >= 0, "%s: no frames, or a negative frame stride or capacity", who);
    CCVS_REQUIRE(rgb && offsets && workspace && (stream || capacity == 0), "%s: null frames, stream, offsets or workspace", who);
    const int mw = sampling ? 16 : 8, mh = sampling == 2 ? 16 : 8;
    JpegArgs a;
    a.rgb = rgb; a.frame_stride = frame_stride;
    a.h = h; a.w = w; a.R = restart_mcus; a.mcux = (w + mw - 1) / mw;
    a.wby = (w + 7) / 8; a.hby = (h + 7) / 8;
    const long nmcu = (long)a.mcux * ((h + mh - 1) / mh);
    a.nmcu = (int)nmcu;                                  // <= 8192^2
    a.nI = (int)((nmcu + restart_mcus - 1) / restart_mcus);
    a.T = (long)n * a.nI;
    a.stream = stream; a.capacity = capacity;
    long* ioff = (long*)workspace;
    a.sizes = (int*)(ioff + a.T);
    a.ioff = ioff;
    a.aligned = (uintptr_t)rgb % 4 == 0 && frame_stride % 4 == 0 && w % 4 == 0;
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            int q = (k_base_q[t][i] * scale + 50) / 100;
            q = q < 1 ? 1 : (q > 255 ? 255 : q);
            a.qd[t][i] = (unsigned short)(q << 3);
        }
    const unsigned grid = limited_grid(a.T, hip_stream, 8);
    void (*const kernel)(JpegArgs) = tables ? jpeg_kernel<JP_FRAME_TABLES>(sampling) : jpeg_kernel<JP_STANDARD>(sampling);
    a.counts = nullptr; a.emit = nullptr;
    if (tables) {
        const size_t base = jpeg_workspace(n, h, w, sampling, restart_mcus);
        a.counts = (unsigned*)((char*)workspace + base);
        unsigned* emit = a.counts + (size_t)n * 4 * 257;
        a.emit = emit;
        if (hipMemsetAsync(a.counts, 0, (size_t)n * 4 * 257 * 4, (hipStream_t)hip_stream) != hipSuccess) {
            ccvs_set_error("%s: clearing the histograms failed: %s", who, hipGetErrorString(hipGetLastError()));
            return CCVS_ERR_LAUNCH;
        }
        a.write = 0;
        hipLaunchKernelGGL(jpeg_kernel<JP_GATHER>(sampling), dim3(grid), dim3(JP_THREADS), 0, (hipStream_t)hip_stream, a);
        hipLaunchKernelGGL(jpeg_tables_kernel, dim3(4 * n), dim3(JP_TBL_THREADS), 0, (hipStream_t)hip_stream, a.counts, tables, emit);
    }
    a.write = 0;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(JP_THREADS), 0, (hipStream_t)hip_stream, a);
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(JP_SCAN_THREADS), 0, (hipStream_t)hip_stream, a.sizes, ioff, offsets, a.T, a.nI);
    a.write = 1;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(JP_THREADS), 0, (hipStream_t)hip_stream, a);
    CCVS_CHECK_LAUNCH(who);
    return CCVS_OK;
}

extern "C" size_t ccvs_mjpeg_workspace_bytes(int n, int h, int w, int restart_mcus) { return jpeg_workspace(n, h, w, 0, restart_mcus); }

extern "C" int ccvs_mjpeg_encode(const uint8_t* rgb, long frame_stride, int n, int h, int w, int quality, int restart_mcus, uint8_t* stream,
                                 long capacity, long* offsets, void* workspace, void* hip_stream) {
    return jpeg_encode("ccvs_mjpeg_encode", rgb, frame_stride, n, h, w, quality, 0, restart_mcus, stream, capacity, offsets, nullptr, workspace, hip_stream);
}

// ---- include/ccvs_hip_output_sampled.h
extern "C" size_t ccvs_mjpeg_sampled_workspace_bytes(int n, int h, int w, int sampling, int restart_mcus) {
    return jpeg_workspace(n, h, w, sampling, restart_mcus);
}

extern "C" int ccvs_mjpeg_encode_sampled(const uint8_t* rgb, long frame_stride, int n, int h, int w, int quality, int sampling, int restart_mcus,
                                         uint8_t* stream, long capacity, long* offsets, void* workspace, void* hip_stream) {
    CCVS_REQUIRE(sampling >= 0 && sampling <= 2, "ccvs_mjpeg_encode_sampled: sampling %d is none of 0 (4:4:4), 1 (4:2:2), 2 (4:2:0)", sampling);
    return jpeg_encode("ccvs_mjpeg_encode_sampled", rgb, frame_stride, n, h, w, quality, sampling, restart_mcus, stream, capacity, offsets, nullptr,
                       workspace, hip_stream);
}

// ---- include/ccvs_hip_output_optimized.h
extern "C" size_t ccvs_mjpeg_optimized_workspace_bytes(int n, int h, int w, int sampling, int restart_mcus) {
    return jpeg_optimized_workspace(n, h, w, sampling, restart_mcus);
}

extern "C" int ccvs_mjpeg_encode_optimized(const uint8_t* rgb, long frame_stride, int n, int h, int w, int quality, int sampling, int restart_mcus,
                                           uint8_t* stream, long capacity, long* offsets, uint8_t* tables, void* workspace, void* hip_stream) {
    const char* who = "ccvs_mjpeg_encode_optimized";
    CCVS_REQUIRE(sampling >= 0 && sampling <= 2, "%s: sampling %d is none of 0 (4:4:4), 1 (4:2:2), 2 (4:2:0)", who, sampling);
    CCVS_REQUIRE(tables, "%s: null tables", who);
    // libjpeg's own search for the smallest frequency stops at 10^9; a frame of 2^28 pixels emits at most 2^29 symbols per table
    CCVS_REQUIRE((long)h * w <= (1L << 28), "%s: frame size %d x %d has more than 2^28 pixels: its symbol counts could pass libjpeg's limit of 10^9", who, h, w);
    return jpeg_encode(who, rgb, frame_stride, n, h, w, quality, sampling, restart_mcus, stream, capacity, offsets, tables, workspace, hip_stream);
}

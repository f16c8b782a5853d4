// The entropy decoder of the JPEG decoder (jpeg_decode.hip): the bit reader and the block decoder of one
// UNIT -- one restart interval, or the whole scan of a frame without DRI.  Plain C++ behind JD_FN, which is `__host__ __device__` under
// hipcc and empty otherwise, so that the same text runs in the kernel (one lane per unit) and in a host program under the sanitizers
// (tests/test_mjpeg_decode_core.py).  Whatever the bytes hold, nothing outside data[0 .. len) is read and nothing outside the blocks
// of the unit's own MCUs is written: every read is bounded by `len`, every coefficient index by 63, every table index by its table.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define JD_FN __host__ __device__ inline
#else
#define JD_FN inline
#endif

// status of a unit
#define JD_OK 0
#define JD_BAD_UNIT 1    // the unit table's entry (frame, bytes, MCUs, table index) points outside what the call was given
#define JD_BAD_CODE 2    // no Huffman code starts so, a DC category above 11 or an AC size above 10
#define JD_OVERRUN 3     // the MCUs need more bits than the unit has
#define JD_BAD_INDEX 4   // a run leads past coefficient 63
#define JD_LEFTOVER 5    // whole bytes left behind the last MCU, or a 0xFF that no 0x00 follows inside the unit

// One Huffman table in the form of T.81 F.2.2.3, built by the host (`ccvs_amd.tools.mjpeg.huffman_table`): codes of up to 8 bits
// through `look` ((length << 8) | symbol for the 8 bits ahead, 0: the code is longer), longer ones through maxcode / valoff.
struct JdHuff {
    uint16_t look[256];
    int32_t maxcode[17];   // [l]: the largest code of length l, -1 where there is none ([0] unused)
    int32_t valoff[17];    // [l]: index into vals of the first code of length l, minus that code
    uint8_t vals[256];
};
// The tables of a frame: the quantiser of every component (natural order) and the Huffman tables DC 0, DC 1, AC 0, AC 1 with the
// components' choice among them (0 or 1).  4008 bytes; the layout is part of the C ABI (include/ccvs_hip_decode.h).
struct JdTables {
    uint16_t q[3][64];
    uint8_t dc_sel[3], ac_sel[3], pad[2];
    JdHuff huff[4];
};
static_assert(sizeof(JdHuff) == 904 && sizeof(JdTables) == 4008, "the table layout is part of the ABI");

// natural (row-major) index of zigzag position k
JD_FN int jd_natural(int k) {
    constexpr uint8_t z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return z[k & 63];
}

// ---- the bit reader: `n` valid bits at the top of `acc`, zeros below.  A 0xFF 0x00 pair gives the byte 0xFF; a 0xFF that nothing or
// anything else follows ends the data there (`cut`).
struct JdBits {
    const uint8_t* p;
    long pos, len;
    uint32_t acc;
    int n, cut;
};
JD_FN void jd_fill(JdBits& b) {
    while (b.n <= 24 && b.pos < b.len && !b.cut) {
        const uint32_t c = b.p[b.pos];
        if (c == 0xFFu) {
            if (b.pos + 1 < b.len && b.p[b.pos + 1] == 0) {
                b.pos += 2;
            } else {
                b.cut = 1;
                break;
            }
        } else {
            ++b.pos;
        }
        b.acc |= c << (24 - b.n);
        b.n += 8;
    }
}
// the next k <= 16 bits (zeros behind the end of the data), 25 or more of them valid after jd_fill unless the data ends
JD_FN uint32_t jd_peek(const JdBits& b, int k) { return b.acc >> (32 - k); }
JD_FN bool jd_skip(JdBits& b, int k) {   // k in 1 .. 16; false: fewer bits left
    if (b.n < k) return false;
    b.acc <<= k;
    b.n -= k;
    return true;
}

// One symbol; a status other than JD_OK ends the unit.
JD_FN int jd_symbol(JdBits& b, const JdHuff& h, int& sym) {
    jd_fill(b);
    const uint32_t e = h.look[jd_peek(b, 8)];
    int l = (int)(e >> 8);
    if (l >= 1 && l <= 8) {
        sym = (int)(e & 255u);
    } else {
        const int32_t code = (int32_t)jd_peek(b, 16);
        for (l = 9; l <= 16; ++l) {
            const int32_t c = code >> (16 - l);
            if (c <= h.maxcode[l]) {
                const int32_t i = h.valoff[l] + c;
                if (i < 0 || i > 255) return JD_BAD_CODE;
                sym = h.vals[i];
                break;
            }
        }
        if (l > 16) return JD_BAD_CODE;
    }
    return jd_skip(b, l) ? JD_OK : JD_OVERRUN;
}
// s in 1 .. 15 further bits as the signed value of category s (T.81 F.2.2.1)
JD_FN int jd_receive_extend(JdBits& b, int s, int& v) {
    jd_fill(b);
    const int r = (int)jd_peek(b, s);
    if (!jd_skip(b, s)) return JD_OVERRUN;
    v = r < (1 << (s - 1)) ? r - (1 << s) + 1 : r;
    return JD_OK;
}

// One block into coef[0 .. 63] (natural order; zero before): the DC difference added to `pred`, then the AC coefficients.
JD_FN int jd_block(JdBits& b, const JdHuff& dc, const JdHuff& ac, int& pred, int16_t* coef) {
    int s, st = jd_symbol(b, dc, s);
    if (st) return st;
    if (s > 11) return JD_BAD_CODE;
    if (s) {
        int diff;
        if ((st = jd_receive_extend(b, s, diff))) return st;
        pred = (int)((unsigned)pred + (unsigned)diff);
    }
    coef[0] = (int16_t)(uint16_t)(unsigned)pred;
    for (int k = 1; k < 64;) {
        int rs;
        if ((st = jd_symbol(b, ac, rs))) return st;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;   // EOB
            k += 16;              // ZRL
            continue;
        }
        if (s > 10) return JD_BAD_CODE;
        k += r;
        if (k > 63) return JD_BAD_INDEX;
        int v;
        if ((st = jd_receive_extend(b, s, v))) return st;
        coef[jd_natural(k)] = (int16_t)v;
        ++k;
    }
    return JD_OK;
}

// The geometry of a frame's coefficient buffer: the blocks of Y ([mcuy * vs][mcux * hs]), then those of Cb and of Cr ([mcuy][mcux]),
// 64 int16 each.
struct JdGeom {
    int hs, vs, mcux, mcuy;
};
JD_FN long jd_frame_blocks(const JdGeom& g) { return (long)g.mcux * g.mcuy * (g.hs * g.vs + 2); }

// One unit: MCUs first .. first + count - 1 of a frame (the caller has checked 0 <= first, 0 <= count, first + count <= MCUs of the
// frame) from data[0 .. len) into the frame's coefficients.  Returns the unit's status.
JD_FN int jd_decode_unit(const uint8_t* data, long len, const JdTables& t, const JdGeom& g, long first, long count, int16_t* coef) {
    JdBits b = {data, 0, len, 0u, 0, 0};
    int pred[3] = {0, 0, 0};
    const long ny = (long)g.mcux * g.mcuy * g.hs * g.vs, nc = (long)g.mcux * g.mcuy;
    for (long m = first; m < first + count; ++m) {
        const long my = m / g.mcux, mx = m - my * g.mcux;
        for (int v = 0; v < g.vs; ++v)
            for (int h = 0; h < g.hs; ++h) {
                const long blk = (my * g.vs + v) * ((long)g.mcux * g.hs) + mx * g.hs + h;
                const int st = jd_block(b, t.huff[t.dc_sel[0] & 1], t.huff[2 + (t.ac_sel[0] & 1)], pred[0], coef + 64 * blk);
                if (st) return st;
            }
        for (int c = 1; c < 3; ++c) {
            const int st = jd_block(b, t.huff[t.dc_sel[c] & 1], t.huff[2 + (t.ac_sel[c] & 1)], pred[c], coef + 64 * (ny + (c - 1) * nc + m));
            if (st) return st;
        }
    }
    jd_fill(b);
    return (b.cut || b.n >= 8 || b.pos != b.len) ? JD_LEFTOVER : JD_OK;
}

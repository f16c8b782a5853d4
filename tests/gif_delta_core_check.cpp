// The host side of tests/test_gif_delta_host.py: the rectangle / band arithmetic of the changed-rectangle GIF frames and the band coder
// (ccvs_amd/csrc/gif_core.h) as a program of its own, built with -fsanitize=address,undefined.  Reads a file of cases, each
//   int64 n, t, h, w, band_rows, chunk, bytes    then n * h * w indices, n * 4 int32 rectangles and the `bytes` of all frames' payloads
//                                                as tests/gif_delta_ref.py gives them (n frames in clips of t),
// finds every frame's changed rectangle, codes both candidates band by band the way the kernel does (a band's indices gathered through
// gif_rect_pixel, `chunk` at a time, the rectangle's unchanged ones GIF_TRANSPARENT), stitches the shorter payload and compares bytes
// and rectangles.  Every buffer has exactly the size the library gives it -- a candidate's words: the full frame's band slots, each of
// gif_band_words(gif_rect_band_max) -- so that the sanitizer sees any step beyond.  Prints "cases N wrong M"; exit status 1 where M > 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "gif_core.h"

struct Coded {
    unsigned* words;
    std::vector<long> bitoff;
    int nbr;
    long size;
};

// one candidate of a frame: `cur` over rectangle r, masked against `prev` where that is not null
static bool code_candidate(Coded& out, const uint8_t* cur, const uint8_t* prev, const GifRect& r, int h, int w, int band_rows, int chunk) {
    const int nb = (int)gif_bands(h, w, band_rows);
    const long wstride = gif_band_words(gif_rect_band_max(h, w, band_rows));
    out.nbr = (int)gif_bands(r.rh, r.rw, band_rows);
    if (out.nbr > nb) return false;                             // a rectangle never has more bands than its frame
    out.words = (unsigned*)malloc(sizeof(unsigned) * wstride * nb);
    out.bitoff.assign(nb + 1, 0);
    unsigned* hash = (unsigned*)malloc(sizeof(unsigned) * GIF_SLOTS);
    uint8_t* staged = (uint8_t*)malloc(chunk);
    bool ok = true;
    for (int b = 0; b < out.nbr && ok; ++b) {
        const int r0 = gif_rect_band_first(r, band_rows, b);
        const long L = (long)gif_rect_band_count(r, band_rows, b) * r.rw;
        if (L < 1 || L > gif_rect_band_max(h, w, band_rows)) ok = false;
        memset(hash, 0xFF, sizeof(unsigned) * GIF_SLOTS);
        GifCoder s;
        gif_start(s, out.words + b * wstride, b == 0, true);
        for (long c0 = 0; c0 < L && ok; c0 += chunk) {
            const int n = (int)(L - c0 < chunk ? L - c0 : chunk);
            for (int i = 0; i < n; ++i) {
                const long p = gif_rect_pixel(r, w, r0, c0 + i);
                if (p < 0 || p >= (long)h * w) {
                    ok = false;
                    break;
                }
                staged[i] = prev && prev[p] == cur[p] ? (uint8_t)GIF_TRANSPARENT : cur[p];
            }
            int pos = 0;
            while (ok && pos < n) {
                pos += gif_code(s, hash, staged + pos, n - pos);
                if (s.full) {
                    memset(hash, 0xFF, sizeof(unsigned) * GIF_SLOTS);
                    s.full = 0;
                }
            }
        }
        const long bits = gif_finish(s, b == out.nbr - 1);
        if (bits > gif_band_bits(L) || s.nwords > wstride) ok = false;
        out.bitoff[b + 1] = out.bitoff[b] + bits;
    }
    out.size = gif_payload_bytes((out.bitoff[out.nbr] + 7) >> 3);
    free(staged);
    free(hash);
    return ok;
}

static void stitch(const Coded& c, long wstride, uint8_t* out) {
    const long data = (c.bitoff[c.nbr] + 7) >> 3;
    out[0] = 8;
    out[c.size - 1] = 0;
    for (long j = 0; j < data; ++j) {
        out[gif_data_pos(j)] = (uint8_t)gif_data_byte(c.words, wstride, c.bitoff.data(), c.nbr, j);
        if (j % 255 == 0) out[gif_data_pos(j) - 1] = (uint8_t)gif_block_len(data, j);
    }
}

static bool run_case(const int64_t* head, const uint8_t* idx, const int32_t* rects, const uint8_t* want) {
    const int n = (int)head[0], t = (int)head[1], h = (int)head[2], w = (int)head[3], band_rows = (int)head[4], chunk = (int)head[5];
    const long bytes = head[6], hw = (long)h * w;
    const long wstride = gif_band_words(gif_rect_band_max(h, w, band_rows));
    // the capacity the library promises: no frame longer than the full frame's bound
    const long rows = gif_band_rows(w, band_rows), nb = gif_bands(h, w, band_rows);
    const long full = rows < h ? rows : h, tail = h - (nb - 1) * rows;
    const long bound = gif_payload_bytes(((nb - 1) * gif_band_bits(full * w) + gif_band_bits(tail * w) + 7) >> 3);
    long at = 0;
    bool ok = true;
    for (int f = 0; f < n && ok; ++f) {
        const uint8_t* cur = idx + f * hw;
        const uint8_t* prev = f % t ? cur - hw : nullptr;
        Coded cand[2];
        cand[1].words = nullptr;
        GifRect rect[2] = {gif_full_rect(h, w), gif_full_rect(h, w)};
        ok = code_candidate(cand[0], cur, nullptr, rect[0], h, w, band_rows, chunk);
        int pick = 0;
        if (prev) {
            int x_min = w, x_max = -1, y_min = h, y_max = -1;
            for (long p = 0; p < hw; ++p)
                if (cur[p] != prev[p]) {
                    const int y = (int)(p / w), x = (int)(p % w);
                    x_min = x < x_min ? x : x_min;
                    x_max = x > x_max ? x : x_max;
                    y_min = y < y_min ? y : y_min;
                    y_max = y > y_max ? y : y_max;
                }
            rect[1] = gif_changed_rect(x_min, x_max, y_min, y_max);
            ok = code_candidate(cand[1], cur, prev, rect[1], h, w, band_rows, chunk) && ok;
            pick = cand[1].size < cand[0].size ? 1 : 0;
        }
        const Coded& c = cand[pick];
        const int32_t* wr = rects + 4 * f;
        ok = ok && c.size <= bound && at + c.size <= bytes && wr[0] == rect[pick].x0 && wr[1] == rect[pick].y0 && wr[2] == rect[pick].rw &&
             wr[3] == rect[pick].rh;
        if (ok) {
            uint8_t* out = (uint8_t*)malloc(c.size);
            memset(out, 0xA5, c.size);
            stitch(c, wstride, out);
            ok = memcmp(out, want + at, c.size) == 0;
            free(out);
            at += c.size;
        }
        free(cand[0].words);
        free(cand[1].words);
    }
    return ok && at == bytes;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    long cases = 0, wrong = 0;
    int64_t head[7];
    while (fread(head, sizeof(int64_t), 7, f) == 7) {
        const long px = head[0] * head[2] * head[3];
        std::vector<uint8_t> idx(px), want(head[6]);
        std::vector<int32_t> rects(4 * head[0]);
        if ((long)fread(idx.data(), 1, px, f) != px || (long)fread(rects.data(), 4, rects.size(), f) != (long)rects.size() ||
            (long)fread(want.data(), 1, head[6], f) != head[6])
            return 2;
        ++cases;
        if (!run_case(head, idx.data(), rects.data(), want.data())) {
            ++wrong;
            fprintf(stderr, "case %ld (%ld frames of %ld x %ld, band_rows %ld, chunk %ld) differs\n", cases - 1, (long)head[0], (long)head[2],
                    (long)head[3], (long)head[4], (long)head[5]);
        }
    }
    fclose(f);
    printf("cases %ld wrong %ld\n", cases, wrong);
    return wrong ? 1 : 0;
}

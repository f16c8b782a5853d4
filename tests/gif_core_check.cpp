// The host side of tests/test_gif_host.py: ccvs_amd/csrc/gif_core.h -- the band coder and the stitch of the GIF output stage -- as a
// program of its own, built with -fsanitize=address,undefined.  Reads a file of cases, each
//   int64 h, w, band_rows, chunk, bytes     then h * w indices, then the `bytes` of the frame's payload as tests/gif_ref.py gives it,
// codes every band the way the kernel does (the indices handed over `chunk` at a time, the hash emptied where the coder asks for it),
// stitches the payload byte by byte and compares.  Every buffer has exactly the size the library gives it, so that the sanitizer sees
// any step beyond.  Prints "cases N wrong M"; exit status 1 where M > 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "gif_core.h"

static bool run_case(const int64_t* head, const uint8_t* idx, const uint8_t* want) {
    const int h = (int)head[0], w = (int)head[1], band_rows = (int)head[2], chunk = (int)head[3];
    const long bytes = head[4];
    const int r = gif_band_rows(w, band_rows);
    const int nb = (int)gif_bands(h, w, band_rows);
    const long lmax = (long)(r < h ? r : h) * w;
    const long wstride = gif_band_words(lmax);
    unsigned* words = (unsigned*)malloc(sizeof(unsigned) * wstride * nb);
    unsigned* hash = (unsigned*)malloc(sizeof(unsigned) * GIF_SLOTS);
    std::vector<long> bitoff(nb + 1, 0);
    long bound_bits = 0;
    for (int b = 0; b < nb; ++b) {
        const int r0 = b * r, r1 = r0 + r < h ? r0 + r : h;
        const long L = (long)(r1 - r0) * w;
        const uint8_t* src = idx + (long)r0 * w;
        memset(hash, 0xFF, sizeof(unsigned) * GIF_SLOTS);
        GifCoder s;
        gif_start(s, words + b * wstride, b == 0, true);
        for (long c0 = 0; c0 < L; c0 += chunk) {
            const int n = (int)(L - c0 < chunk ? L - c0 : chunk);
            int pos = 0;
            while (pos < n) {
                pos += gif_code(s, hash, src + c0 + pos, n - pos);
                if (s.full) {
                    memset(hash, 0xFF, sizeof(unsigned) * GIF_SLOTS);
                    s.full = 0;
                }
            }
        }
        const long bits = gif_finish(s, b == nb - 1);
        if (bits > gif_band_bits(L) || s.nwords > wstride) return false;
        bound_bits += gif_band_bits(L);
        bitoff[b + 1] = bitoff[b] + bits;
    }
    const long data = (bitoff[nb] + 7) >> 3;
    const long size = gif_payload_bytes(data);
    bool ok = size == bytes && size <= gif_payload_bytes((bound_bits + 7) >> 3);
    if (ok) {
        uint8_t* out = (uint8_t*)malloc(size);
        memset(out, 0xA5, size);
        out[0] = 8;
        out[size - 1] = 0;
        for (long j = 0; j < data; ++j) {
            out[gif_data_pos(j)] = (uint8_t)gif_data_byte(words, wstride, bitoff.data(), nb, j);
            if (j % 255 == 0) out[gif_data_pos(j) - 1] = (uint8_t)gif_block_len(data, j);
        }
        ok = memcmp(out, want, size) == 0;
        free(out);
    }
    free(hash);
    free(words);
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    long cases = 0, wrong = 0;
    int64_t head[5];
    while (fread(head, sizeof(int64_t), 5, f) == 5) {
        const long n = head[0] * head[1];
        std::vector<uint8_t> idx(n), want(head[4]);
        if ((long)fread(idx.data(), 1, n, f) != n || (long)fread(want.data(), 1, head[4], f) != head[4]) return 2;
        ++cases;
        if (!run_case(head, idx.data(), want.data())) {
            ++wrong;
            fprintf(stderr, "case %ld (%ld x %ld, band_rows %ld, chunk %ld) differs\n", cases - 1, (long)head[0], (long)head[1], (long)head[2], (long)head[3]);
        }
    }
    fclose(f);
    printf("cases %ld wrong %ld\n", cases, wrong);
    return wrong ? 1 : 0;
}

// Host check of the JPEG entropy decoder (ccvs_amd/csrc/jpeg_decode_core.h), built with -fsanitize=address,undefined and run as a
// program of its own by tests/test_mjpeg_decode_core.py.  Reads a file of cases and decodes each unit from a heap copy of exactly its
// bytes (so that a read beyond them is an error) into a coefficient buffer between two guards.
//
// A case: int64 hs, vs, mcux, mcuy, first, count, len, expect (0: the status must be 0, 1: it must not be), has_coef; the 4008-byte
// table record; len bytes; if has_coef, the expected int16 coefficients of the whole frame.  Whatever the status, the blocks of MCUs
// outside first .. first + count - 1 must stay zero and the guards whole.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_decode_core.h"

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    long cases = 0, clean = 0, failed = 0, bad = 0;
    int64_t head[9];
    while (fread(head, sizeof(head), 1, f) == 1) {
        const JdGeom g = {(int)head[0], (int)head[1], (int)head[2], (int)head[3]};
        const long first = head[4], count = head[5], len = head[6];
        const long blocks = jd_frame_blocks(g), nmcu = (long)g.mcux * g.mcuy;
        if (g.hs < 1 || g.hs > 2 || g.vs < 1 || g.vs > 2 || g.mcux < 1 || g.mcuy < 1 || blocks > (1 << 20) || first < 0 || count < 0 || first + count > nmcu ||
            len < 0 || len > (1 << 26)) {
            fprintf(stderr, "case %ld: malformed header\n", cases);
            return 2;
        }
        JdTables* t = (JdTables*)malloc(sizeof(JdTables));
        uint8_t* data = (uint8_t*)malloc(len ? len : 1);
        std::vector<int16_t> want(head[8] ? blocks * 64 : 0);
        if (!read_exact(f, t, sizeof(JdTables)) || !read_exact(f, data, len) || !read_exact(f, want.data(), want.size() * 2)) {
            fprintf(stderr, "case %ld: truncated\n", cases);
            return 2;
        }
        const long guard = 64;
        int16_t* buf = (int16_t*)malloc((blocks * 64 + 2 * guard) * sizeof(int16_t));
        for (long i = 0; i < guard; ++i) buf[i] = buf[guard + blocks * 64 + i] = 0x5A5A;
        int16_t* coef = buf + guard;
        memset(coef, 0, blocks * 64 * sizeof(int16_t));
        const int st = jd_decode_unit(data, len, *t, g, first, count, coef);
        bool ok = st >= JD_OK && st <= JD_LEFTOVER && (st != JD_OK) == (head[7] != 0);
        for (long i = 0; i < guard; ++i) ok = ok && buf[i] == 0x5A5A && buf[guard + blocks * 64 + i] == 0x5A5A;
        const long ny = nmcu * g.hs * g.vs;
        for (long b = 0; b < blocks; ++b) {
            long m;
            if (b < ny) {
                const long by = b / ((long)g.mcux * g.hs), bx = b % ((long)g.mcux * g.hs);
                m = (by / g.vs) * g.mcux + bx / g.hs;
            } else {
                m = (b - ny) % nmcu;
            }
            if (m >= first && m < first + count) continue;
            for (int k = 0; k < 64; ++k) ok = ok && coef[64 * b + k] == 0;
        }
        if (st == JD_OK && head[8]) ok = ok && memcmp(coef, want.data(), blocks * 64 * sizeof(int16_t)) == 0;
        if (!ok) {
            fprintf(stderr, "case %ld: status %d (expected %s), or coefficients / guards wrong\n", cases, st, head[7] ? "non-zero" : "0");
            ++bad;
        }
        ++cases;
        clean += st == JD_OK;
        failed += st != JD_OK;
        free(buf);
        free(data);
        free(t);
    }
    fclose(f);
    printf("cases %ld clean %ld failed %ld wrong %ld\n", cases, clean, failed, bad);
    return bad || !cases ? 1 : 0;
}

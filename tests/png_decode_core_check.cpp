// Host check of the inflate of the PNG decoder (ccvs_amd/csrc/png_decode_core.h), built with -fsanitize=address,undefined and run as a
// program of its own by tests/test_png_decode_core.py.  Reads a file of cases and inflates each stream from a heap copy of exactly its
// bytes (so that a read beyond them is an error) into a heap buffer of exactly the expected size between two guards; the tables, the
// input stage and the output ring are heap blocks of exactly their sizes too, refilled, flushed and summed by 64 lanes one after the
// other as the kernel's wave does it.
//
// A case: int64 len, expect, status (the spec mirror's), has_bytes; len bytes; if has_bytes, the `expect` bytes of the output.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "png_decode_core.h"

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
    int64_t head[4];
    while (fread(head, sizeof(head), 1, f) == 1) {
        const long len = head[0], expect = head[1];
        if (len < 0 || len > (1 << 26) || expect < 0 || expect > (1 << 26) || head[2] < 0 || head[2] > PD_BAD_CHECK) {
            fprintf(stderr, "case %ld: malformed header\n", cases);
            return 2;
        }
        uint8_t* data = (uint8_t*)malloc(len ? len : 1);
        std::vector<uint8_t> want(head[3] ? expect : 0);
        if (!read_exact(f, data, len) || !read_exact(f, want.data(), want.size())) {
            fprintf(stderr, "case %ld: truncated\n", cases);
            return 2;
        }
        const long guard = 64;
        uint8_t* buf = (uint8_t*)malloc(expect + 2 * guard);
        memset(buf, 0x5A, expect + 2 * guard);
        uint8_t* out = buf + guard;
        PdTables* t = (PdTables*)malloc(sizeof(PdTables));
        uint8_t* stage = (uint8_t*)malloc(PD_STAGE);
        uint8_t* ring = (uint8_t*)malloc(PD_RING);
        const int st = pd_inflate_checked(data, len, out, expect, *t, stage, ring, 64);
        bool ok = st == (int)head[2];
        for (long i = 0; i < guard; ++i) ok = ok && buf[i] == 0x5A && buf[guard + expect + i] == 0x5A;
        if (st == PD_OK && head[3] && expect) ok = ok && memcmp(out, want.data(), expect) == 0;
        if (!ok) {
            fprintf(stderr, "case %ld: status %d (the mirror's: %ld), or bytes / guards wrong\n", cases, st, (long)head[2]);
            ++bad;
        }
        ++cases;
        clean += st == PD_OK;
        failed += st != PD_OK;
        free(ring);
        free(stage);
        free(t);
        free(buf);
        free(data);
    }
    fclose(f);
    printf("cases %ld clean %ld failed %ld wrong %ld\n", cases, clean, failed, bad);
    return bad || !cases ? 1 : 0;
}

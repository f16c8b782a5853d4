/* libccvs_hip.so: the lossless output stage with LZ77 matches -- ccvs_hip_output_lossless.h's encoder (the same filters, bands, Huffman
 * builder, framing, conventions and refusals) whose deflate blocks may hold matches.  Additive to ABI
 * version 6; include/ccvs_hip.h includes this header (inside its extern "C" block), so a program that includes that one needs nothing
 * else.  Everything is computed in integers, and the bytes are the same on every run and under any CU budget. */
#ifndef CCVS_HIP_OUTPUT_LOSSLESS_LZ_H
#define CCVS_HIP_OUTPUT_LOSSLESS_LZ_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Arguments, stream layout, offsets and capacity rules are those of ccvs_apng_encode.  What differs is a band's block:
 * window   at a position: the same frame's filtered bytes before it, earlier bands of the frame included; distance 1 .. 32768.
 * length   3 .. 258, never past the end of the position's own band; a copy may overlap itself (distance < length).
 * matches  candidates at a position: distance 1, distance 3 (the pixel to the left), distance 3 w + 1 (the byte above), and the nearest
 *          earlier position of the same band whose three bytes have the same 13-bit hash ((b0 | b1 << 8 | b2 << 16) * 0x9E3779B1 mod
 *          2^32, top 13 bits; the band's last two positions have none) if it is at most 32768 back.  The longest wins, ties go to the
 *          smallest distance; a match of length 3 more than 4096 back is dropped.
 * parse    greedy from the band's first byte: a match at the position is taken whole, else one literal.
 * coding   RFC 1951 section 3.2.5: 286 literal/length and 30 distance symbols, both codes built as ccvs_apng_encode builds its one (15
 *          bits at most; a distance code with fewer than two used symbols counts the lowest unused ones once), HLIT and HDIST trimmed, the
 *          two lists of lengths run-length coded as one sequence, extra bits behind their symbols.
 * choice   per band the block with matches or the literal-only block of ccvs_apng_encode, whichever has fewer bits; ties and bands
 *          without any match: literal-only.  So every frame's stream is at most as long as ccvs_apng_encode's, and
 *          ccvs_apng_stream_bound remains a capacity that suffices for any pixels.
 * workspace: ccvs_apng_lz_workspace_bytes(n, h, w, band_rows) bytes, of any content: 5 n h (3 w + 1) bytes (the filtered bytes and a
 * token per byte) and 2984 bytes per band; 0 for arguments the encoder refuses.  Refusals: those of ccvs_apng_encode, named in
 * ccvs_last_error() before any launch. */
size_t ccvs_apng_lz_workspace_bytes(int n, int h, int w, int band_rows);
int ccvs_apng_encode_lz(const uint8_t* rgb, long frame_stride, int n, int h, int w, int filter, int band_rows, uint8_t* stream, long capacity,
                        long* offsets, void* workspace, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* CCVS_HIP_OUTPUT_LOSSLESS_LZ_H */

/* libccvs_hip.so: the lossless output stage -- uint8 RGB frames -> PNG-filtered rows, deflate-coded into one complete zlib stream per
 * frame, which is the payload of a PNG IDAT / APNG fdAT chunk (`ccvs_amd.tools.apng` writes the container on the
 * host).  Additive to ABI version 6; include/ccvs_hip.h includes this header (inside its extern "C" block), so a program that includes that
 * one needs nothing else.  Status codes and conventions are those of ccvs_hip.h: every pointer is a device pointer, `stream` a
 * hipStream_t, nothing synchronises with the host, no state is kept between calls, everything is computed in integers, and the bytes are
 * the same on every run and under any CU budget. */
#ifndef CCVS_HIP_OUTPUT_LOSSLESS_H
#define CCVS_HIP_OUTPUT_LOSSLESS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* rgb: uint8 [n][h][w][3], rows and pixels dense, frame i at rgb + i * frame_stride (frame_stride >= 3 w h; what lies between the
 * frames is never read).
 * filter   PNG's filter of every row (bpp = 3; pixels left of the row and above row 0 count as 0): 0 None, 1 Sub, 2 Up, 3 Average,
 *          4 Paeth, or -1: per row the type with the smallest sum of |signed byte| over the row's 3 w filtered bytes (libpng's
 *          heuristic), ties to the lowest type.  A filtered row is its type byte and the 3 w bytes; filtering reads raw pixels only.
 * bands    a frame is cut into bands of `band_rows` rows (the last one may be shorter; 0: as many rows as hold at most 32768 filtered
 *          bytes, at least one).  A band is ONE deflate block with dynamic Huffman tables (RFC 1951 section 3.2.7) built from the
 *          band's own bytes: literals 0 .. 255 and end-of-block 256, no matches.  Every band but the frame's last is followed by an empty
 *          stored block (bits 000, zero bits to the byte boundary, 00 00 FF FF), so every band starts at a byte; the last band's block has
 *          BFINAL = 1 and is padded with zero bits to a byte.
 * tables   literal/length code: the two smallest nonzero counts are merged, among equal counts the larger symbol first, the sum staying
 *          with the first of the two, until one is left; depths beyond 15 are brought down to 15 by the T.81 K.2 move, which keeps the
 *          code complete; the lengths, ascending, go to the symbols by descending count, then ascending symbol; codes are canonical
 *          (RFC 1951 3.2.2).  HLIT = 0 (257 codes); two distance codes of length 1 (HDIST = 1).  The 259 lengths are run-length coded
 *          as zlib's send_tree does it, as one sequence (symbols 16, 17 and 18 are all used); the code-length code is built the same
 *          way with a limit of 7 bits and sent in the RFC's permuted order with HCLEN trimmed.
 * stream   per frame: 78 01, the blocks, the big-endian Adler-32 of the frame's filtered bytes.  Frame i is
 *          stream[offsets[i] .. offsets[i + 1]); `offsets` (int64 [n + 1]) is complete also when offsets[n] > capacity; nothing is written
 *          at or beyond `capacity`, nor at or beyond offsets[n]; what the stream held before does not matter.
 * workspace: ccvs_apng_workspace_bytes(n, h, w, band_rows) bytes, of any content: the filtered bytes (n h (3 w + 1)) and 1576 bytes per
 * band.  ccvs_apng_stream_bound: a capacity that suffices for any pixels (15 bits per byte and 470 bytes per band, plus 6 per frame).
 * Both return 0 for arguments the encoder refuses.
 * Refused before any launch (CCVS_ERR_ARG, ccvs_last_error): null pointers (a null `stream` goes with capacity 0), n <= 0, h or w outside
 * 1 .. 65535, filter outside -1 .. 4, band_rows < 0 or a band of 2^31 filtered bytes or more, a negative capacity, frame_stride < 3 w h. */
size_t ccvs_apng_workspace_bytes(int n, int h, int w, int band_rows);
long ccvs_apng_stream_bound(int n, int h, int w, int band_rows);
int ccvs_apng_encode(const uint8_t* rgb, long frame_stride, int n, int h, int w, int filter, int band_rows, uint8_t* stream, long capacity,
                     long* offsets, void* workspace, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* CCVS_HIP_OUTPUT_LOSSLESS_H */

/* libccvs_hip.so: the output stage with per-frame optimised Huffman tables -- the JPEG encoder of ccvs_hip_output.h and
 * ccvs_hip_output_sampled.h writing what libjpeg writes with optimize_coding = TRUE.  Additive to ABI version 6;
 * include/ccvs_hip.h includes this header (inside its extern "C" block), so a program that includes that one needs nothing else.  Status
 * codes and conventions are those of ccvs_hip.h: every pointer is a device pointer, `stream` a hipStream_t, nothing synchronises with
 * the host, no state is kept between calls. */
#ifndef CCVS_HIP_OUTPUT_OPTIMIZED_H
#define CCVS_HIP_OUTPUT_OPTIMIZED_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* The quantised coefficients are those of ccvs_mjpeg_encode_sampled for the same pixels, quality, sampling (0 = 4:4:4, 1 = 4:2:2,
 * 2 = 4:2:0) and restart interval -- not one decoded pixel changes.  What changes is the code: every frame gets the four Huffman tables
 * that libjpeg's jpeg_gen_optimal_table builds from the symbols of THAT frame's scan, and its scan is coded with them.  Three steps on
 * `stream`, all in integers:
 *   gather   per frame and table, how often the scan emits every symbol: the DC category of every block's difference (predictors 0 at
 *            every restart interval; a dummy luminance block of a subsampled frame is coded like any block), (run << 4) | size per
 *            nonzero AC coefficient, 0xF0 per sixteen zeros, 0x00 where a block ends in zeros.  Integer sums: the same on every run;
 *   tables   jchuff.c's algorithm: a pseudo-symbol 256 of frequency 1 keeps the all-ones code unused; the two smallest nonzero
 *            frequencies are merged, ties to the larger symbol, until one is left; code sizes of up to 32 are brought down to 16 by
 *            T.81 K.2; symbols are listed by ascending size before that adjustment, then by value; codes are canonical (T.81 Annex C).
 *            A table with one symbol gives one code of length 1;
 *   emit     the two passes of ccvs_mjpeg_encode (sizes, prefix sum, bytes) with the frame's tables.
 * tables: uint8 [n][4][272], written completely: per frame the tables in the order libjpeg writes their DHT segments -- DC luminance,
 * AC luminance, DC chrominance, AC chrominance -- each as bits[16] (the number of codes of length 1 .. 16) and huffval (sum of bits
 * symbols), zero-padded to 272 bytes.  `ccvs_amd.tools.mjpeg.jpeg_header(h, w, quality, restart_mcus, sampling, huffman=...)` writes a
 * frame's four into its header; header + scan + EOI is the file libjpeg writes but for its JFIF APP0 segment.
 * rgb, frame_stride, quality, restart_mcus, stream, capacity, offsets: as ccvs_mjpeg_encode_sampled takes and gives them -- `offsets`
 * (int64 [n + 1]) is complete also when offsets[n] > capacity, nothing is written at or beyond `capacity`, the same bytes on every run.
 * workspace: ccvs_mjpeg_optimized_workspace_bytes(n, h, w, sampling, restart_mcus) bytes (what ccvs_mjpeg_sampled_workspace_bytes says
 * plus 8208 per frame for the histograms and the codes; 0 for arguments the encoder refuses).  Refused before any launch (CCVS_ERR_ARG,
 * ccvs_last_error): null `tables`, a frame of more than 2^28 pixels (libjpeg's own table search stops at 10^9 symbols), and everything
 * ccvs_mjpeg_encode_sampled refuses. */
size_t ccvs_mjpeg_optimized_workspace_bytes(int n, int h, int w, int sampling, int restart_mcus);
int ccvs_mjpeg_encode_optimized(const uint8_t* rgb, long frame_stride, int n, int h, int w, int quality, int sampling, int restart_mcus,
                                uint8_t* stream, long capacity, long* offsets, uint8_t* tables, void* workspace, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* CCVS_HIP_OUTPUT_OPTIMIZED_H */

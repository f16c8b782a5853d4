/* libccvs_hip.so: the output stage with chrominance subsampling -- the JPEG encoder of ccvs_hip_output.h writing 4:2:2 and 4:2:0 as well
 * as 4:4:4.  Additive to ABI version 6; include/ccvs_hip.h includes this header (inside its extern "C" block),
 * so a program that includes that one needs nothing else.  Status codes and conventions are those of ccvs_hip.h: every pointer is a
 * device pointer, `stream` a hipStream_t, nothing synchronises with the host, no state is kept between calls. */
#ifndef CCVS_HIP_OUTPUT_SAMPLED_H
#define CCVS_HIP_OUTPUT_SAMPLED_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* sampling: 0 = 4:4:4 (the bytes of ccvs_mjpeg_encode), 1 = 4:2:2 (libjpeg's h2v1), 2 = 4:2:0 (h2v2) -- the numbers Pillow's
 * `subsampling` and `ccvs_amd.tools.mjpeg.parse_jpeg` use.  For 1 and 2 the entropy-coded bytes equal, bit for bit, what libjpeg writes
 * for the same pixels, quality, sampling and restart interval.  Colour conversion, DCT, quantiser, zigzag, Huffman tables, byte stuffing,
 * interval padding and RSTn markers are those of ccvs_hip_output.h; what sampling adds, all in integers:
 *   components  Y sampled 2 x 1 (4:2:2) or 2 x 2 (4:2:0), Cb and Cr 1 x 1.  An MCU covers 16 x 8 or 16 x 16 pixels; its blocks are
 *               Y0 Y1 Cb Cr, or Y00 Y01 Y10 Y11 Cb Cr (the Y blocks in raster order inside the MCU);
 *   sizes       a component with factors (ch, cv) out of (hs, vs) is ceil(w ch / (8 hs)) blocks wide and ceil(h cv / (8 vs)) blocks high
 *               -- NOT rounded up to whole MCUs;
 *   order       RGB -> YCbCr at full resolution to 8-bit samples first, chrominance down-sampled after that;
 *   columns     before down-sampling the right column is replicated up to 2 x 8 x (chrominance width in blocks) pixels, for Y up to
 *               8 x (Y width in blocks);
 *   filter      a box with libjpeg's alternating bias by the OUTPUT column x:  h2v2 (a + b + c + d + (x even ? 1 : 2)) >> 2,
 *               h2v1 (a + b + (x even ? 0 : 1)) >> 1; no smoothing, no "fancy" down-sampling;
 *   rows        in two steps: before down-sampling the bottom row is replicated only up to the next multiple of the vertical factor
 *               (one row for odd h in 4:2:0); after it the last DOWN-SAMPLED row is replicated up to 8 x (height in blocks);
 *   dummies     a Y block position of an MCU outside Y's width or height in blocks (right edge: w mod 16 in 1 .. 8; bottom edge in
 *               4:2:0: h mod 16 in 1 .. 8) is a dummy block: not transformed, its 63 AC coefficients 0, its DC coefficient that of the
 *               block before it in the MCU's order (maybe a dummy itself).  It is coded like any block and updates Y's prediction;
 *   prediction  per component across the interval: Y's runs through all Y blocks of an MCU into the next MCU; 0 at every interval start.
 *
 * restart_mcus: the restart interval in MCUs OF THE SAMPLING'S SIZE, 1 .. 32 (4:4:4), 1 .. 24 (4:2:2), 1 .. 16 (4:2:0): an interval has
 * at most 96 blocks and is encoded by one workgroup.  rgb, frame_stride, stream, capacity, offsets: as ccvs_mjpeg_encode takes and
 * gives them -- frame i's scan is stream[offsets[i] : offsets[i + 1]], `offsets` (int64 [n + 1]) is complete also when
 * offsets[n] > capacity, nothing is written at or beyond `capacity`, the same bytes on every run.  The header in front of a scan is
 * `ccvs_amd.tools.mjpeg.jpeg_header(h, w, quality, restart_mcus, sampling)`.
 * workspace: ccvs_mjpeg_sampled_workspace_bytes(n, h, w, sampling, restart_mcus) bytes (12 per interval, rounded up; 0 for arguments
 * the encoder refuses).  Refused before any launch (CCVS_ERR_ARG, ccvs_last_error): sampling outside 0 .. 2, restart_mcus outside
 * 1 .. the sampling's limit, and everything ccvs_mjpeg_encode refuses. */
size_t ccvs_mjpeg_sampled_workspace_bytes(int n, int h, int w, int sampling, int restart_mcus);
int ccvs_mjpeg_encode_sampled(const uint8_t* rgb, long frame_stride, int n, int h, int w, int quality, int sampling, int restart_mcus,
                              uint8_t* stream, long capacity, long* offsets, void* workspace, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* CCVS_HIP_OUTPUT_SAMPLED_H */

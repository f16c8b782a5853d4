/* libccvs_hip.so: the output stage -- the uint8 clips `ccvs_pack_u8` / `ccvs_pack_u8_norm` write, as baseline JPEG scans for a
 * Motion-JPEG AVI file.  Additive to ABI version 6; include/ccvs_hip.h includes this header (inside its
 * extern "C" block), so a program that includes that one needs nothing else.  Status codes and conventions are those of ccvs_hip.h:
 * every pointer is a device pointer, `stream` a hipStream_t, nothing synchronises with the host, no state is kept between calls. */
#ifndef CCVS_HIP_OUTPUT_H
#define CCVS_HIP_OUTPUT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Baseline JPEG (ITU-T T.81: sequential DCT, Huffman, 8 bit, three components sampled 1 x 1) in libjpeg's integer arithmetic, so that
 * the entropy-coded bytes equal, bit for bit, what libjpeg writes for the same pixels, quality and restart interval:
 *   colour    F(x) = int(x * 65536 + 0.5);  Y = (F(.299) R + F(.587) G + F(.114) B + 32768) >> 16,
 *             Cb = (-F(.16874) R - F(.33126) G + F(.5) B + (128 << 16) + 32767) >> 16,
 *             Cr = (F(.5) R - F(.41869) G - F(.08131) B + (128 << 16) + 32767) >> 16;
 *   padding   the right column and the bottom row replicated up to multiples of 8; 128 subtracted;
 *   DCT       jfdctint ("islow": CONST_BITS 13, PASS1_BITS 2), rows then columns -- 8 x the true DCT;
 *   quantiser scale = 5000 / q (q < 50) or 200 - 2 q;  t = clip((base * scale + 50) / 100, 1, 255) on the Annex K.1 / K.2 tables;
 *             |c| -> (|c| + (8 t >> 1)) / (8 t), sign restored;
 *   entropy   zigzag, DC differences per component (0 at the start of every restart interval), the Annex K.3 - K.6 Huffman tables
 *             (luminance for Y, chrominance for Cb and Cr), blocks Y Cb Cr per MCU, MCUs in raster order, a 0xFF data byte followed by
 *             0x00, the last byte of an interval padded with 1-bits, intervals separated by FF D0+(i & 7).
 *
 * rgb: n frames of uint8 [h, w, 3] (interleaved RGB, rows dense), frame i at rgb + i * frame_stride (bytes, >= 0).
 * restart_mcus: the restart interval in MCUs (8 x 8 pixels), 1 .. 32.  An interval is byte-aligned and independent of every other
 * one: one workgroup encodes one interval.
 *
 * Output: frame i's SCAN -- everything between the SOS header and EOI, RSTn markers included -- is stream[offsets[i] : offsets[i + 1]],
 * offsets[0] = 0; the headers are constant per (h, w, quality, restart_mcus) and are the host's (`ccvs_amd.tools.mjpeg.jpeg_header`).
 * `offsets` (int64 [n + 1]) is always complete and correct, also when offsets[n] > capacity: then no byte at or beyond `capacity` is
 * written (the bytes below it are the right ones) and the caller runs again with a larger stream.  Two passes over the frames -- the
 * intervals' sizes, a scan over them, the bytes at their final offsets: no atomic decides an offset, the same bytes on every run.
 * workspace: ccvs_mjpeg_workspace_bytes(n, h, w, restart_mcus) bytes (12 per interval, rounded up; 0 for arguments the encoder
 * refuses).  Refused before any launch (CCVS_ERR_ARG, ccvs_last_error): quality outside 1 .. 100, restart_mcus outside 1 .. 32, h or w
 * outside 1 .. 65535, n < 1, a negative frame stride or capacity, a null pointer. */
size_t ccvs_mjpeg_workspace_bytes(int n, int h, int w, int restart_mcus);
int ccvs_mjpeg_encode(const uint8_t* rgb, long frame_stride, int n, int h, int w, int quality, int restart_mcus,
                      uint8_t* stream, long capacity, long* offsets, void* workspace, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* CCVS_HIP_OUTPUT_H */

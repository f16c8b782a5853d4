/* libccvs_hip.so: the way back from the output stage -- baseline JPEG scans, such as the frames of the Motion-JPEG AVI files
 * `ccvs_mjpeg_encode` fills, as uint8 frames.  Additive to ABI version 6; include/ccvs_hip.h includes this
 * header (inside its extern "C" block), so a program that includes that one needs nothing else.  Status codes and conventions are
 * those of ccvs_hip.h: `stream` a hipStream_t, nothing synchronises with the host, no state is kept between calls; every pointer is a
 * device pointer EXCEPT `units_host`. */
#ifndef CCVS_HIP_DECODE_H
#define CCVS_HIP_DECODE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Baseline JPEG (ITU-T T.81: sequential DCT, Huffman, 8 bit; three components, luminance sampled 1 x 1, 2 x 1 or 2 x 2 against 1 x 1
 * chrominance, one interleaved scan, with or without restart markers) in libjpeg's integer arithmetic, so that the pixels equal, bit
 * for bit, what libjpeg (libjpeg-turbo, "islow" DCT, "fancy" upsampling: the defaults) decodes from the same file:
 *   entropy   Huffman codes of up to 16 bits from the frame's own tables (T.81 F.2.2.3: maxcode / valptr / vals, an 8-bit lookup in
 *             front), 0xFF 0x00 read as 0xFF, DC predictions 0 at the start of every unit, values sign-extended (F.2.2.1);
 *   IDCT      coefficient x quantiser, then jidctint ("islow": CONST_BITS 13, PASS1_BITS 2): the column pass descaled by 11 bits, the
 *             row pass by 18; + 128, clamped to 0 .. 255;
 *   h2v1      on the ceil(w / 2) real chrominance columns: out[2i] = (3 in[i] + in[i-1] + 1) >> 2, out[2i+1] = (3 in[i] + in[i+1] + 2)
 *             >> 2, a column beyond either end replicating the end (the first and last output samples are copies);
 *   h2v2      per output row s = 3 near_row + far_row over the ceil(h / 2) real chrominance rows, rows beyond either end replicating
 *             it; out[2i] = (3 s[i] + s[i-1] + 8) >> 4, out[2i+1] = (3 s[i] + s[i+1] + 7) >> 4, columns replicating likewise;
 *   colour    R = Y + ((91881 (Cr - 128) + 32768) >> 16), B = Y + ((116130 (Cb - 128) + 32768) >> 16),
 *             G = Y + ((-22554 (Cb - 128) - 46802 (Cr - 128) + 32768) >> 16), each clamped to 0 .. 255 (>> is arithmetic).
 * Where the inverse DCT's value before the clamp leaves -512 .. 511, libjpeg's C code wraps and its SIMD code saturates; this decoder
 * clamps.  No encoder writes such blocks; streams that hold them are outside the bit-exact claim.
 *
 * One call decodes n frames of one geometry: h x w pixels, sampling 0 (4:4:4), 1 (4:2:2: luminance 2 x 1) or 2 (4:2:0: 2 x 2).
 *
 * scans: the entropy-coded bytes of all frames, one behind the other, scan_bytes of them (RSTn markers may stay in; no unit covers them).
 * units: int64 [n_units][5] -- frame, byte offset into `scans`, byte length, first MCU, MCUs.  A UNIT is one restart interval, or the
 * whole scan of a frame without DRI: it is byte-aligned and predicts its DC values from nothing outside it, so one lane decodes one
 * unit.  MCUs count in raster order over the frame's ceil(w / (8 hs)) x ceil(h / (8 vs)) MCUs.  units_host: the same table in HOST
 * memory; it is what the call checks before it launches anything (the kernel checks the device copy again and touches nothing outside
 * the stream and the frame whatever either holds).
 * tables: n_tables records of 4008 bytes, frame_table: int32 [n], the record of every frame.  A record:
 *   uint16 q[3][64]        the quantiser of Y, Cb, Cr in natural (row-major) order;
 *   uint8 dc_sel[3], ac_sel[3], pad[2]   which of the two DC and of the two AC tables below a component uses (0 or 1);
 *   4 x { uint16 look[256]; int32 maxcode[17]; int32 valoff[17]; uint8 vals[256]; }   DC 0, DC 1, AC 0, AC 1:
 *                          look[the next 8 bits] = (length << 8) | symbol for codes of up to 8 bits, else 0; maxcode[l] the largest
 *                          code of length l or -1; valoff[l] = index into vals of the first code of length l, minus that code.
 *   (`ccvs_amd.tools.mjpeg.decode_tables` builds it; a frame without DHT gets the Annex K tables there.)
 * rgb: frame i as uint8 [h, w, 3] (interleaved RGB, rows dense) at rgb + i * frame_stride (bytes, >= 3 h w).  Only those bytes are written.
 * status: int32 [n_units].  0: the unit decoded exactly its MCUs within its bytes.  1: its table entry points outside the call's
 * frames, stream, MCUs or tables; 2: no Huffman code starts so (or a DC category above 11, an AC size above 10); 3: the MCUs need
 * more bits than the unit has; 4: a run leads past coefficient 63; 5: whole bytes are left behind the last MCU, or the unit holds a
 * 0xFF that no 0x00 follows.  A failed unit ends there: its remaining blocks decode as zero coefficients, every other unit's pixels
 * are unaffected (outside the chrominance filter's one-sample reach).
 * workspace: ccvs_mjpeg_decode_workspace_bytes(n, h, w, sampling) bytes, 16-byte aligned (the coefficients, 128 bytes per block, and
 * the component planes padded to whole MCUs; 0 for arguments the decoder refuses).
 * Refused before any launch (CCVS_ERR_ARG, ccvs_last_error): a sampling other than 0, 1, 2; h or w outside 1 .. 65535; a subsampled
 * frame with w <= 4 (fewer than 3 chrominance columns: libjpeg takes another path there); n, n_units or n_tables < 1; a negative
 * scan_bytes; a frame stride below 3 h w; a null or misaligned pointer; an entry of units_host that points outside the frames, the
 * stream or the frame's MCUs.  The same bytes come out on every run. */
size_t ccvs_mjpeg_decode_workspace_bytes(int n, int h, int w, int sampling);
int ccvs_mjpeg_decode(const uint8_t* scans, long scan_bytes, const int64_t* units, const int64_t* units_host, long n_units,
                      const void* tables, int n_tables, const int32_t* frame_table, int n, int h, int w, int sampling,
                      uint8_t* rgb, long frame_stride, int32_t* status, void* workspace, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* CCVS_HIP_DECODE_H */

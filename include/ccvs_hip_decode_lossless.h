/* libccvs_hip.so: the way back from the lossless output stage -- zlib streams, such as the frames of the APNG files
 * `ccvs_apng_encode` fills or of anybody's 8-bit RGB PNG files, as bytes and as uint8 frames.  Additive to ABI
 * version 6; include/ccvs_hip.h includes this header (inside its extern "C" block), so a program that includes that one needs nothing
 * else.  Status codes and conventions are those of ccvs_hip.h: `stream` a hipStream_t, nothing synchronises with the host, no state is
 * kept between calls; every pointer is a device pointer EXCEPT `rows_host`. */
#ifndef CCVS_HIP_DECODE_LOSSLESS_H
#define CCVS_HIP_DECODE_LOSSLESS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* A complete inflate (RFC 1950 zlib wrapper, RFC 1951 deflate: stored, fixed and dynamic blocks, matches up to 32768 bytes back,
 * overlapping ones included) under zlib's own acceptance rules, so that a stream decodes here exactly where `zlib.decompress` decodes
 * it to the expected number of bytes:
 *   header    CM = 8, CINFO <= 7, (CMF * 256 + FLG) a multiple of 31, FDICT clear;
 *   tables    HLIT <= 286 and HDIST <= 30; a repeat needs a length before it and may not pass the last length; a set of lengths may
 *             not be over-subscribed; it may be incomplete only as a literal/length or distance set whose longest code has one bit; a
 *             distance set without any code is accepted until a distance is needed; the end-of-block code must have a length;
 *   codes     literal/length symbols 286 and 287 and distance symbols 30 and 31 are refused where they turn up;
 *   matches   a distance may reach the first byte of the stream's own output and no further (CINFO does not bound it, as in zlib);
 *   end       the Adler-32 behind the last block is checked; bytes behind it are ignored.
 * Whatever the bytes hold, nothing outside a stream's own bytes is read and nothing outside its own output range is written.
 *
 * data: the streams' bytes, data_bytes of them.  rows / rows_host: the same int64 table in device and in HOST memory, one row per
 * stream; rows_host is what a call checks before it launches anything (the kernel checks the device copy again).
 * status: int32 [n], one word per stream:
 *    0 OK            1 BAD_STREAM (the row points outside the call's buffers)    2 BAD_HEADER
 *    3 BAD_BLOCK (type 3, or LEN != ~NLEN)    4 BAD_TABLE    5 BAD_CODE    6 BAD_DISTANCE    7 OVERRUN (the input ended)
 *    8 TOO_LONG (more output than expected)    9 TOO_SHORT (the final block ended early)    10 BAD_CHECK (Adler-32)
 *   11 BAD_FILTER (a row's filter type byte is above 4; ccvs_png_decode only)
 * A failed stream ends where it failed: the rest of its output range keeps what it held; every other stream is unaffected.
 * The same bytes come out on every run.
 *
 * ccvs_zlib_inflate: n streams to n byte ranges of `out` (out_bytes long).  rows: int64 [n][4] -- byte offset into `data`, byte
 * length, byte offset into `out`, the number of bytes the stream is to hold.  The output ranges must not overlap (not checked).
 * Refused before any launch (CCVS_ERR_ARG, ccvs_last_error): n < 1; a negative data_bytes or out_bytes; a null or misaligned pointer
 * (the tables 8, status 4); a row of rows_host that points outside `data` or `out`.
 *
 * ccvs_png_decode: n streams, each the concatenated IDAT (or fdAT) payload of one h x w image of 8-bit RGB samples without
 * interlace, to frame i as uint8 [h, w, 3] (rows dense) at rgb + i * frame_stride (bytes, >= 3 h w); only those bytes are written.
 * rows: int64 [n][2] -- byte offset into `data`, byte length.  Every stream is inflated to the image's h (3 w + 1) filtered bytes in
 * the workspace, then PNG's filters are undone (types 0 .. 4: none, sub, up, average, Paeth, with bpp = 3; pixels left of a row and
 * above row 0 count as 0).  A frame whose status is not 0 has unspecified pixels.
 * workspace: ccvs_png_decode_workspace_bytes(n, h, w) bytes, 16-byte aligned (0 for arguments the decoder refuses).
 * Refused before any launch: n < 1; h or w outside 1 .. 65535; a negative data_bytes; a frame stride below 3 h w; a null or misaligned
 * pointer (the tables 8, status 4, workspace 16); a row of rows_host that points outside `data`. */
size_t ccvs_png_decode_workspace_bytes(int n, int h, int w);
int ccvs_zlib_inflate(const uint8_t* data, long data_bytes, const int64_t* rows, const int64_t* rows_host, int n, uint8_t* out, long out_bytes,
                      int32_t* status, void* hip_stream);
int ccvs_png_decode(const uint8_t* data, long data_bytes, const int64_t* rows, const int64_t* rows_host, int n, int h, int w, uint8_t* rgb,
                    long frame_stride, int32_t* status, void* workspace, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* CCVS_HIP_DECODE_LOSSLESS_H */

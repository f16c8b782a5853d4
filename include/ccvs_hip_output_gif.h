/* libccvs_hip.so: the GIF output stage -- uint8 RGB clips -> one colour table of 256 entries per clip, chosen from the clip's own pixels,
 * and every frame's LZW-coded image data, framed in sub-blocks: what stands behind an image descriptor in a GIF89a file (DESIGN.md section
 * 4.27; `ccvs_amd.tools.gif` writes the container on the host).  Additive to ABI version 6; include/ccvs_hip.h includes this header (inside
 * its extern "C" block), so a program that includes that one needs nothing else.  Status codes and conventions are those of ccvs_hip.h:
 * every pointer is a device pointer, `hip_stream` a hipStream_t, nothing synchronises with the host, no state is kept between calls,
 * everything is computed in integers, and the bytes are the same on every run and under any CU budget.  tests/gif_ref.py states the same
 * rules in numpy. */
#ifndef CCVS_HIP_OUTPUT_GIF_H
#define CCVS_HIP_OUTPUT_GIF_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* clips: uint8 [b][t][h][w][3], rows and pixels dense, frame j of clip i at clips + i * clip_stride + j * frame_stride (frame_stride >=
 * 3 w h, clip_stride >= (t - 1) frame_stride + 3 w h; what lies between is never read).
 *
 * ccvs_gif_palette, per clip:
 * bins     a pixel's bin is (R >> 3) << 10 | (G >> 3) << 5 | (B >> 3).  Over all t frames every bin gets its pixel count and the sums of
 *          R, G and B (64-bit integer atomics; nothing else in this stage is an atomic).
 * boxes    median cut over the occupied bins.  Box 0 holds them all.  While there are fewer than 256 boxes and some box holds at least two
 *          occupied bins: the box with the largest population x longest extent (64-bit; extent: max - min occupied bin coordinate, the
 *          largest of the three axes; ties to the lowest box) is split along its longest axis (ties: G, then R, then B).  With P(c) the
 *          population of the box's bins whose coordinate on that axis is <= c, the cut is the smallest c with P(c) >= ceil(total / 2),
 *          at most hi - 1 (hi: the box's largest occupied coordinate).  Bins with coordinate <= cut keep the box's index, the others
 *          become the next new box.
 * palette  [b][256][3]: entry i is, per channel, floor((2 sum + n) / (2 n)) over box i's pixels; entries without a box are 0, 0, 0.
 *          used[i] (int32 [b]): clip i's number of boxes.
 * table    [b][32768]: an occupied bin's own mean colour (the same rounding, of the bin's sums) goes to the palette entry below used[i]
 *          with the smallest squared distance, ties to the lowest entry; the entries of unoccupied bins are 0.  A pixel's index is the
 *          table entry of its bin.  A clip of at most 256 occupied bins that each hold one colour is therefore stored exactly.
 *
 * ccvs_gif_encode, per frame (n = b t frames, in the clips' order; `table` is ccvs_gif_palette's):
 * LZW      minimum code size 8: clear 256, end of information 257, first free code 258; codes are packed LSB first.  A frame is cut into
 *          bands of `band_rows` rows (0: as many rows as hold at most 4096 indices, at least one; the last band may be shorter).  Every band
 *          starts with an empty dictionary and 9-bit codes; only band 0 begins with a clear code.  At an index the pending string does not
 *          extend to (a miss): the string's code is written at the current width; if free < 4096 the extended string becomes entry `free`,
 *          free += 1, and if then free > (1 << width) and width < 12, width += 1; if now free = 4096 (the table is full) a clear code is
 *          written at the current width and the coder starts again: empty dictionary, free = 258, width 9.  At the end of a band: the
 *          pending string's code; the entry the decoder makes of it (if free < 4096: free += 1, the same width rule); then, at that width,
 *          a CLEAR code -- END OF INFORMATION in the frame's last band.  So a band's codes depend on nothing outside it while the frame
 *          stays one ordinary LZW stream (the clear between two bands has the width the earlier band ended with, which is why it ends
 *          that band).  A frame's bands follow each other bit by bit, without padding; the last byte is padded with zero bits.
 * stream   per frame: the byte 08, the data in sub-blocks of at most 255 bytes, each behind its length byte, the byte 00.  Frame i is
 *          stream[offsets[i] .. offsets[i + 1]); `offsets` (int64 [n + 1]) is complete also when offsets[n] > capacity; nothing is written
 *          at or beyond `capacity`, nor at or beyond offsets[n]; what the stream held before does not matter.
 * workspace: ccvs_gif_workspace_bytes(b, t, h, w, band_rows) bytes, of any content, for either call: 1 MiB of bins per clip, and per band
 *          its coded bits.  ccvs_gif_stream_bound(n, h, w, band_rows): a capacity that suffices for any pixels -- a band of L indices
 *          writes at most L + L / 3838 + 2 codes (one per index, a clear per table fill, the leading clear or the one at its end, and
 *          the pending string's), each of at most 12 bits; a frame's bits are rounded up to bytes, then one length byte per 255 and
 *          the two bytes around them.  Both return 0 for arguments the calls refuse.
 * Refused before any launch (CCVS_ERR_ARG, ccvs_last_error): null pointers (a null `stream` goes with capacity 0), b or t <= 0, h or w
 * outside 1 .. 65535, band_rows < 0 or a band of 2^24 indices or more, a negative capacity, frame_stride < 3 w h, clip_stride <
 * (t - 1) frame_stride + 3 w h, b t >= 2^24. */
size_t ccvs_gif_workspace_bytes(int b, int t, int h, int w, int band_rows);
long ccvs_gif_stream_bound(int n, int h, int w, int band_rows);
int ccvs_gif_palette(const uint8_t* clips, long clip_stride, long frame_stride, int b, int t, int h, int w, uint8_t* palette, uint8_t* table,
                     int* used, void* workspace, void* hip_stream);
int ccvs_gif_encode(const uint8_t* clips, long clip_stride, long frame_stride, int b, int t, int h, int w, int band_rows, const uint8_t* table,
                    uint8_t* stream, long capacity, long* offsets, void* workspace, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* CCVS_HIP_OUTPUT_GIF_H */

/* libccvs_hip.so: the GIF output stage with changed-rectangle frames -- a frame after its clip's first may be written as the bounding
 * rectangle of what changed against the frame before, with a transparent index where nothing did, where that takes fewer bytes than
 * the full frame (`ccvs_amd.tools.gif` writes the container on the host).  Additive to ABI version 6;
 * include/ccvs_hip.h includes this header (inside its extern "C" block).  Clips, strides, status codes and conventions are those of
 * ccvs_hip_output_gif.h: every pointer is a device pointer, `hip_stream` a hipStream_t, nothing synchronises with the host, no state is
 * kept between calls, everything is computed in integers, and the bytes are the same on every run and under any CU budget.
 * tests/gif_delta_ref.py states the same rules in numpy. */
#ifndef CCVS_HIP_OUTPUT_GIF_DELTA_H
#define CCVS_HIP_OUTPUT_GIF_DELTA_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ccvs_gif_palette_n: ccvs_gif_palette whose median cut stops at `max_colours` boxes (2 .. 256) instead of 256; with 256 it gives
 * ccvs_gif_palette's bytes.  The changed-rectangle frames take max_colours = 255: then used[i] <= 255, palette entry 255 is 0, 0, 0 and
 * no table entry is 255, which is free to be the TRANSPARENT INDEX.  A clip of at most 255 occupied bins that each hold one colour is
 * still stored exactly; one of 256 such colours no longer is.
 *
 * ccvs_gif_encode_delta, per frame (n = b t frames, in the clips' order; `table` is ccvs_gif_palette_n's at 255; idx[f]: a frame's
 * indices through the table, as ccvs_gif_encode codes them):
 * frame 0 of every clip: the full frame, F: the rectangle (0, 0, w, h) with the indices idx[f], coded exactly as ccvs_gif_encode does.
 * frame j >= 1 of a clip: changed = idx[f] != idx[f - 1], the frame before OF THE SAME CLIP.  Two candidates: F, and D, the bounding
 *          rectangle (x0, y0, rw, rh) of `changed` holding idx[f] where changed and 255 elsewhere; where nothing changed D is the
 *          rectangle (0, 0, 1, 1) holding the single index 255, whose payload is the 7 bytes 08 04 00 ff 05 04 00.
 * LZW      both candidates by the rules of ccvs_gif_encode, cut into bands of `band_rows` rows OF THE RECTANGLE (0: as many of its rows
 *          as hold at most 4096 of its indices, at least one: max(1, 4096 / rw)).  A rectangle never has more bands than the full frame;
 *          one of its bands can hold more indices than any of the full frame's (64 x 64 in a frame 100 wide: 4096 against 4000).
 * choice   D is written where its payload is strictly shorter than F's, else F: no frame's payload is longer than ccvs_gif_encode's of
 *          the same indices, and ccvs_gif_stream_bound stays a capacity that suffices.
 * rects    int32 [n][4]: x0, y0, rw, rh of the written candidate, complete whatever the capacity.  In the file the frame's image
 *          descriptor carries this rectangle; the graphic control extension's packed byte is 0x04 for a clip's frame 0 (disposal 1: do
 *          not dispose) and 0x05 for the others (disposal 1, transparent colour flag) with transparent index 255.  What a decoder shows
 *          at frame f is then palette[idx[f]] exactly.
 * stream, offsets: as ccvs_gif_encode's.
 * workspace: ccvs_gif_delta_workspace_bytes(b, t, h, w, band_rows) bytes, of any content, for ccvs_gif_palette_n and
 *          ccvs_gif_encode_delta: the bins, and both candidates' band bits.  0 for arguments the calls refuse.
 * Refused before any launch (CCVS_ERR_ARG, ccvs_last_error): what ccvs_gif_palette / ccvs_gif_encode refuse, max_colours outside
 * 2 .. 256, a null `rects`. */
int ccvs_gif_palette_n(const uint8_t* clips, long clip_stride, long frame_stride, int b, int t, int h, int w, int max_colours,
                       uint8_t* palette, uint8_t* table, int* used, void* workspace, void* hip_stream);
size_t ccvs_gif_delta_workspace_bytes(int b, int t, int h, int w, int band_rows);
int ccvs_gif_encode_delta(const uint8_t* clips, long clip_stride, long frame_stride, int b, int t, int h, int w, int band_rows,
                          const uint8_t* table, uint8_t* stream, long capacity, long* offsets, int* rects, void* workspace, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* CCVS_HIP_OUTPUT_GIF_DELTA_H */

/* pc_tiles.h -- C ABI of libpc_tiles.so: one 8-bit image cut into independent, equally sized tiles of float32 planes
 * (pc_tiles_cut_u8) and decoded tiles stitched back into any window of the 8-bit image, with the distortion sums
 * (pc_tiles_stitch_u8), on gfx950.  DESIGN.md section 11.
 *
 * Kept apart from libpcodec.so and from libpc_pixels.so: nothing here is part of the codec's numeric contract, byte strings or
 * profiles, and the two image-domain libraries do not depend on each other (the 256-entry quotient table is duplicated here).
 * Plain C, the conventions of pc_pixels.h: device pointers, int64 strides, status codes PC_OK / PC_ERR_* (pcodec.h), `stream` is a
 * hipStream_t passed as void* (NULL = default stream).  No call allocates device memory or synchronises the host.  Every argument
 * is checked before the first HIP call; a call that returns PC_ERR_ARG has launched nothing.  All offsets are 64-bit.
 *
 * Geometry.  Tile size T, a multiple of 64; overlap O, a multiple of 4 with 0 <= O <= T/2; stride S = T - O.  Along an axis of
 * length L there is 1 tile if L <= T, otherwise ceil((L - T) / S) + 1.  Tile i covers [i*S, i*S + T); what lies beyond the image is
 * +0.0f.  Tiles are numbered row-major over the ny x nx grid; a "grid rectangle" (ty0, tx0, nty, ntx) is nty x ntx of them, and
 * tile (ty0 + a, tx0 + b) is tile a*ntx + b of the rectangle.
 *
 * An 8-bit image ("u8 view") is a pointer, a layout and two strides in BYTES:
 *   PC_TILES_HWC  [h,w,3] interleaved: byte (y, x, c) at p[y*s_row + 3*x + c]; s_plane is ignored.
 *   PC_TILES_CHW  [3,h,w] planar:      byte (c, y, x) at p[c*s_plane + y*s_row + x].
 * s_row >= the bytes of a row (3*w or w), s_plane >= 1 (planar).  The pointer needs no alignment.  A destination view must be nested
 * rows-in-planes (planar: s_plane >= (h-1)*s_row + w), so that no byte is written twice.
 *
 * A float32 tile set is a pointer and tile, channel and row strides in ELEMENTS, unit stride along a row.
 */
#ifndef PC_TILES_H
#define PC_TILES_H

#include "pcodec.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PC_TILES_HWC = 0, PC_TILES_CHW = 1 };
enum { PC_TILES_NEAREST = 0, PC_TILES_TRUNC = 1 };
enum { PC_TILES_CUT = 0, PC_TILES_STITCH = 1 };

/* Host only: *ny, *nx = the tiles along H and W.  PC_ERR_ARG for H, W < 1, T < 64 or no multiple of 64, O < 0, no multiple of 4 or
 * > T/2, a grid of more than 2^31 - 1 tiles, or NULL outputs. */
PC_API int pc_tiles_grid(int H, int W, int T, int O, int* ny, int* nx);

/* dst[a*ntx + b][c][r][q] = (float)src(Y, X, c) / 255.0f with Y = (ty0 + a)*S + r, X = (tx0 + b)*S + q where (Y, X) lies inside the
 * H x W image, the correctly rounded float32 quotient (a 256-entry table of host-computed quotients, as pc_pixels_ingest_u8), and
 * +0.0f elsewhere.  One kernel.
 *   src           u8 view of the whole H x W image.
 *   dst           contiguous float32 [nty*ntx][3][T][T]; every element is written (no memset needed).  4-byte aligned.
 *   ty0 .. ntx    a rectangle inside the grid of pc_tiles_grid(H, W, T, O). */
PC_API int pc_tiles_cut_u8(const uint8_t* src, int layout, int64_t s_plane, int64_t s_row, int H, int W, int T, int O, int ty0, int tx0,
                           int nty, int ntx, float* dst, void* stream);

/* Bytes of device workspace pc_tiles_stitch_u8 needs when it is given `ref` for the window (., x0, h, w): 48 bytes per block of 1024
 * four-column groups; the groups are aligned to multiples of 4 in IMAGE columns, so a row has ceil((x0 + w) / 4) - floor(x0 / 4) of
 * them.  0 for arguments the call would refuse. */
PC_API size_t pc_tiles_stitch_workspace_size(int x0, int h, int w);

/* The window (y0, x0, h, w) of the image from the decoded tiles of a grid rectangle.  Per axis, tile i weighs a pixel at local
 * coordinate u = p - i*S with (2u + 1) / (2 O) in the band it shares with tile i - 1 (i > 0, u < O), with
 * (2 (O - 1 - (u - S)) + 1) / (2 O) in the band it shares with tile i + 1 (u >= S, tile i + 1 exists), and with 1.0f elsewhere: each
 * the correctly rounded float32 quotient.  A pixel's weight for a tile is the float32 product wy * wx.  Per element
 *   m = fmaf(w_t, fminf(fmaxf(v_t, 0), 1), acc)   chained from acc = +0.0f over the covering tiles t in ascending tile index
 * (NaN -> 0), then q = rintf(m * 255.0f) (PC_TILES_NEAREST, half to even) or truncf(m * 255.0f) (PC_TILES_TRUNC), stored to dst.
 *   x             float32 tile set of the rectangle: element (t, c, r, q) at x[t*sxt + c*sxc + r*sxh + q]; sxh >= T; 4-byte aligned.
 *   window        inside the image; the rectangle must hold EVERY tile that covers a pixel of the window (checked).
 *   dst           u8 view of h x w pixels, addressed relative to the window's first pixel; bytes outside the window are not
 *                 touched.  NULL with ref: the sums only, no image.
 *   ref           optional u8 view of the original image's window, addressed like dst.  With it (and then workspace, sse_u8 and
 *                 sse_f are required):
 *     sse_u8[c]   sum over the window of (q - ref)^2, in integers (exact).
 *     sse_f[c]    sum over the window of (x_ref - m)^2 with x_ref = ref / 255.0f as pc_tiles_cut_u8 gives it: the difference in
 *                 float32, its square in float64 (exact), accumulated in float64 in a fixed order (per thread, per block into the
 *                 workspace, then one ordered reduction).  No atomics: the sums depend on the window and its covering tiles only
 *                 and are bitwise the same from run to run, on any stream, on either access path and from any rectangle.
 *   workspace     at least pc_tiles_stitch_workspace_size(x0, h, w) bytes; PC_ERR_ARG if smaller.  Unused without ref.
 *                 workspace, sse_u8 and sse_f are 8-byte aligned.
 * One kernel, plus the ordered reduction when ref is given. */
PC_API int pc_tiles_stitch_u8(const float* x, int64_t sxt, int64_t sxc, int64_t sxh, int H, int W, int T, int O, int ty0, int tx0, int nty,
                              int ntx, int y0, int x0, int h, int w, int rounding, uint8_t* dst, int dst_layout, int64_t d_plane,
                              int64_t d_row, const uint8_t* ref, int ref_layout, int64_t r_plane, int64_t r_row, void* workspace,
                              size_t workspace_bytes, uint64_t* sse_u8, double* sse_f, void* stream);

/* Host only, launches nothing: *wide = 1 where the cut (op = PC_TILES_CUT: u8 is src, f32 is dst with strides 3*T*T, T*T, T; x0 is
 * ignored) or the stitch (op = PC_TILES_STITCH: u8 is dst, f32 is x, x0 the window's first column) with these arguments moves four
 * pixels per access (a 32-bit word of bytes, a 128-bit word of floats), 0 where it moves them byte by byte and float by float.  Both
 * give the same bits, sums included.  A work item is four consecutive columns of one row, aligned to a multiple of 4 in tile columns
 * (cut) or image columns (stitch); S is a multiple of 4, so the two agree.  The wide path needs: the f32 pointer 16-byte aligned and
 * its strides multiples of 4; every u8 view's strides multiples of 4 (s_plane: planar only) and the address of image column
 * 4*floor(x0 / 4) -- p - 3*(x0 % 4) interleaved, p - x0 % 4 planar; for the cut, p itself -- 4-byte aligned.  `ref` may be NULL; for the
 * stitch `u8` may be NULL when `ref` is not (sums only).  The calls decide with the same code.  PC_ERR_ARG for an unknown op or
 * layout, NULL pointers or x0 < 0. */
PC_API int pc_tiles_plan(int op, const void* u8, int layout, int64_t s_plane, int64_t s_row, const void* f32, int64_t ft, int64_t fc,
                         int64_t fh, int x0, const void* ref, int ref_layout, int64_t r_plane, int64_t r_row, int* wide);

PC_API const char* pc_tiles_strerror(int code);
PC_API int pc_tiles_last_hip_error(void);

#ifdef __cplusplus
}
#endif

#endif /* PC_TILES_H */

/* pc_frame_tiles.h -- C ABI of libpc_frame_tiles.so: one YUV 4:2:0 frame (NV12 / I420 / P010) cut straight into independent, equally
 * sized tiles of float32 RGB planes (pc_frame_tiles_cut) and decoded tiles stitched straight back into any admissible window of the
 * frame, with the per-plane distortion sums (pc_frame_tiles_stitch), on gfx950.  DESIGN.md section 14: the composition of section
 * 13 (pc_frames.h: formats, levels, ingest and emit arithmetic) and section 11 (pc_tiles.h: geometry, band weights, blend), with no
 * frame-sized float intermediate.
 *
 * Kept apart from libpcodec.so and from the other image-side libraries (libpc_pixels.so, libpc_tiles.so, libpc_rate.so,
 * libpc_frames.so): nothing here is part of the codec's numeric contract, byte strings or profiles, and no library of the image domain
 * links another (the device code this one shares with pc_frames.hip and pc_tiles.hip comes from the headers of image_csrc/, DESIGN.md
 * section 19).  Plain C, the
 * conventions of pc_frames.h and pc_tiles.h: device pointers, int64 strides, status codes PC_OK / PC_ERR_* (pcodec.h), `stream` is a
 * hipStream_t passed as void* (NULL = default stream).  No call allocates device memory or synchronises the host: the caller passes
 * the workspace, and every launch is ordered on `stream`.  Every argument is checked before the first HIP call; a call that returns
 * PC_ERR_ARG has launched nothing.  All offsets are 64-bit.
 *
 * A frame (pc_ft_frame, a typedef of the one record pc_frame, pc_yuv_frame.h) is ONE picture of H x W luma samples with Hc x Wc chroma
 * samples,
 * Hc = ceil(H/2), Wc = ceil(W/2), as strided planes; the batch strides are ignored.  Strides are in ELEMENTS: bytes for the 8-bit
 * formats, little-endian 16-bit words for PC_FT_P010.
 *   PC_FT_NV12  Y (r, q) at y[r*y_row + q];  Cb (i, j) at u[i*u_row + 2j], Cr one element after it;  v is ignored.  8-bit codes.
 *   PC_FT_I420  Y as above;  Cb at u[i*u_row + j], Cr at v[i*v_row + j].  8-bit codes.
 *   PC_FT_P010  the layout of NV12 in 16-bit words with the 10-bit code in the upper bits: code = word >> 6 on input (the low six
 *               bits are ignored), word = code << 6 on output.
 * y_row >= W, u_row >= 2*Wc (interleaved) or Wc, v_row >= Wc.  A pointer needs the alignment of its element only.  The planes of a
 * destination must not overlap each other (the caller's to keep).
 *
 * Levels (n = 8 or 10 bits, s = 2^(n-8)):   PC_FT_LIMITED  yo = 16s, ys = 219s, co = 128s, cs = 224s
 *                                           PC_FT_FULL     yo = 0,   ys = 2^n-1, co = 128s, cs = 2^n-1
 * The colour coefficients are plain float arguments, computed by the caller (float64 from Kr and Kb, rounded once).  Every product,
 * sum and quotient below is one IEEE float32 operation (the library is built with -ffp-contract=off).
 *
 * Geometry (pc_tiles.h).  Tile size T, a multiple of 64; overlap O, a multiple of 4 with 0 <= O <= T/2; stride S = T - O.  Along an
 * axis of length L there is 1 tile if L <= T, otherwise ceil((L - T) / S) + 1.  Tile i covers [i*S, i*S + T); what lies beyond the
 * frame is +0.0f.  Tiles are numbered row-major over the ny x nx grid; a "grid rectangle" (ty0, tx0, nty, ntx) is nty x ntx of them,
 * and tile (ty0 + a, tx0 + b) is tile a*ntx + b of the rectangle.
 *
 * A float32 tile set is a pointer and tile, channel and row strides in ELEMENTS, unit stride along a row.
 */
#ifndef PC_FRAME_TILES_H
#define PC_FRAME_TILES_H

#include "pcodec.h"
#include "pc_yuv_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PC_FT_NV12 = PC_YUV_NV12, PC_FT_I420 = PC_YUV_I420, PC_FT_P010 = PC_YUV_P010 };
enum { PC_FT_LIMITED = PC_YUV_LIMITED, PC_FT_FULL = PC_YUV_FULL };
enum { PC_FT_NEAREST = PC_YUV_NEAREST, PC_FT_LINEAR = PC_YUV_LINEAR };
enum { PC_FT_CUT = 0, PC_FT_STITCH = 1 };

typedef pc_frame pc_ft_frame;       /* pc_yuv_frame.h; y_batch, u_batch, v_batch: ignored (one picture per record) */

/* dst[a*ntx + b][0..2][r][q] = (R, G, B) of luma pixel (Y, X) = ((ty0 + a)*S + r, (tx0 + b)*S + q) of the frame where that pixel
 * lies inside H x W, and +0.0f elsewhere.  With C the Cb or Cr plane of codes of the WHOLE frame:
 *   i0 = Y >> 1, i1 = i0 + 1 if Y is odd else i0 - 1, clamped to [0, Hc-1]; j0, j1 likewise from X and Wc  (the frame's edges, never a
 *   tile's: a tile is the crop of the whole frame's ingest);
 *   c16 = 9 C[i0,j0] + 3 C[i0,j1] + 3 C[i1,j0] + C[i1,j1]   (PC_FT_LINEAR)   or   16 C[i0,j0]   (PC_FT_NEAREST)  -- integers, exact;
 *   y' = float(Ycode - yo) / float(ys);  cb' = float(c16_b - 16 co) / float(16 cs);  cr' likewise;
 *   R = y' + (cr' * a);  G = (y' - (cb' * b)) - (cr' * c);  B = y' + (cb' * d);  each then fminf(fmaxf(v, 0), 1).
 *   src           the whole H x W frame.
 *   dst           contiguous float32 [nty*ntx][3][T][T]; every element is written (no memset needed).  4-byte aligned.
 *   ty0 .. ntx    a rectangle inside the grid of an H x W frame.
 * One kernel. */
PC_API int pc_frame_tiles_cut(const pc_ft_frame* src, int fmt, int range, int upsample, float a, float b, float c, float d, int H, int W,
                              int T, int O, int ty0, int tx0, int nty, int ntx, float* dst, void* stream);

/* Bytes of device workspace pc_frame_tiles_stitch needs when it is given `ref` for the window (., x0, h, w): 24 bytes (three 64-bit
 * sums) per block of 256 work items; a work item is one row pair of the window by eight luma columns aligned to a multiple of 8 in
 * FRAME columns, so there are ceil(h / 2) * (ceil((x0 + w) / 8) - floor(x0 / 8)) of them.  0 for arguments the call would refuse. */
PC_API size_t pc_frame_tiles_stitch_workspace_size(int x0, int h, int w);

/* The window (y0, x0, h, w) of the frame from the decoded tiles of a grid rectangle.  For every luma pixel of the window
 *   m = fmaf(w_t, fminf(fmaxf(v_t, 0), 1), acc)   chained from acc = +0.0f over the covering tiles t in ascending tile index, with
 * w_t = wy * wx (a float32 product) of the correctly rounded band weights of pc_tiles.h; then, on m as the decoder's planes,
 *   (R, G, B) = fminf(fmaxf(m, 0), 1);  Y' = ((kr * R) + (kg * G)) + (kb * B);  Cb' = (B - Y') * ib;  Cr' = (R - Y') * ir;
 *   Ycode = clampi(rintf((Y' * float(ys)) + float(yo)), 0, 2^n-1);
 * and for chroma sample (i, j) of the window, with window rows 2i and min(2i+1, h-1), columns 2j and min(2j+1, w-1), u = Cb' * float(cs):
 *   code = clampi(rintf(((u00 + u01) + (u10 + u11)) * 0.25f + float(co)), 0, 2^n-1)   (subscripts: row, column); Cr likewise.
 *   x             float32 tile set of the rectangle: element (t, c, r, q) at x[t*sxt + c*sxc + r*sxh + q]; sxh >= T; 4-byte aligned.
 *   window        inside the frame and ADMISSIBLE: y0 and x0 even, h even or y0 + h == H, w even or x0 + w == W (the window's output is
 *                 then the crop of the whole frame's); the rectangle must hold EVERY tile that covers a pixel of the window (checked).
 *   dst           frame of the window in `fmt` (h x w luma, ceil(h/2) x ceil(w/2) chroma), addressed relative to the window's first
 *                 sample; elements outside its samples are not touched.  NULL with ref: the sums only.
 *   ref           optional frame in `fmt`: the original's window, addressed like dst (luma from (y0, x0), chroma from (y0/2, x0/2)).
 *                 With it (then workspace and sse are required):
 *     sse[p]      p = 0, 1, 2 for Y, Cb, Cr: the sum over the window of (code - refcode)^2 in unsigned 64-bit integers, exact.  No
 *                 atomics: thread, wave tree, block (into the workspace), then one reduction launch.  Every element is written.
 *   workspace     at least pc_frame_tiles_stitch_workspace_size(x0, h, w) bytes; PC_ERR_ARG if smaller.  Unused without ref.
 *                 workspace and sse are 8-byte aligned.
 * One kernel, plus the ordered reduction when ref is given. */
PC_API int pc_frame_tiles_stitch(const float* x, int64_t sxt, int64_t sxc, int64_t sxh, int H, int W, int T, int O, int ty0, int tx0,
                                 int nty, int ntx, int y0, int x0, int h, int w, int fmt, int range, float kr, float kg, float kb,
                                 float ib, float ir, const pc_ft_frame* dst, const pc_ft_frame* ref, void* workspace,
                                 size_t workspace_bytes, uint64_t* sse, void* stream);

/* Host only, launches nothing: *wide = 1 where the cut (op = PC_FT_CUT: frame is src, f32 is dst with strides 3*T*T, T*T, T; x0 is
 * ignored) or the stitch (op = PC_FT_STITCH: frame is dst, f32 is x, x0 the window's first column; O is ignored) with these
 * arguments moves four elements of a plane per access (a 32-bit word of an 8-bit plane, a 64-bit word of a 16-bit plane) and four
 * floats per access (128 bits), 0 where it moves them one by one.  Both give the same bits, sums included.  A work item is eight
 * consecutive columns: of one tile row, aligned in TILE columns, for the cut; of one row pair of the window, aligned to a multiple of
 * 8 in FRAME columns, for the stitch.  The wide path needs: the f32 pointer 16-byte aligned and its strides multiples of 4; every
 * plane's row stride a multiple of 4; for the cut every plane pointer aligned to four elements and O a multiple of 8 (S is then a
 * multiple of 8, an item's first luma column a multiple of 8 in the frame and its first chroma column a multiple of 4; with O = 4 a
 * tile's first chroma column is 2 mod 4); for the stitch the address of frame column 8*floor(x0 / 8) -- y - x0 % 8, u - x0 % 8
 * interleaved, u - (x0 % 8) / 2 and v likewise planar, in elements -- aligned to four elements, in dst and in ref.  Items that
 * straddle an edge of the frame or of the window go element by element on either path.  `ref` may be NULL; for the stitch `frame`
 * may be NULL when `ref` is not (sums only).  The calls decide with the same code.  PC_ERR_ARG for an unknown op or format, NULL
 * pointers, O < 0, or x0 negative or odd. */
PC_API int pc_frame_tiles_plan(int op, int fmt, const pc_ft_frame* frame, const void* f32, int64_t ft, int64_t fc, int64_t fh, int O,
                               int x0, const pc_ft_frame* ref, int* wide);

PC_API const char* pc_frame_tiles_strerror(int code);
PC_API int pc_frame_tiles_last_hip_error(void);

#ifdef __cplusplus
}
#endif

#endif /* PC_FRAME_TILES_H */

/* pc_chroma_tiles.h -- C ABI of libpc_chroma_tiles.so: one YUV frame of any of pc_chroma.h's formats (4:2:0 / 4:2:2 / 4:4:4, planar or
 * semi-planar, 8-bit or 10-bit) and chroma sitings cut straight into independent, equally sized tiles of float32 RGB planes
 * (pc_chroma_tiles_cut) and decoded tiles stitched straight back into any admissible window of the frame, with the per-plane
 * distortion sums (pc_chroma_tiles_stitch), on gfx950.  DESIGN.md section 23: the composition of section 21 (pc_chroma.h: formats,
 * sitings, levels, ingest and emit arithmetic) and section 11 (pc_tiles.h: geometry, band weights, blend), with no frame-sized float
 * intermediate; what pc_frame_tiles.h (section 14) is for NV12 / I420 / P010 with centre-sited chroma, and bit for bit that there.
 *
 * Kept apart from libpcodec.so and from the other image-side libraries; no library of the image domain links another.  Plain C, the
 * conventions of pc_chroma.h and pc_frame_tiles.h: device pointers, int64 strides, status codes PC_OK / PC_ERR_* (pcodec.h), `stream`
 * is a hipStream_t passed as void* (NULL = default stream).  No call allocates device memory or synchronises the host: the caller
 * passes the workspace, and every launch is ordered on `stream`.  Every argument is checked before the first HIP call; a call that
 * returns PC_ERR_ARG has launched nothing.  All offsets are 64-bit; the one exception is the row strides of the stitch's dst and ref
 * frames, which the kernels hold in 32 bits: the stitch refuses a row stride of 2^31 elements or more (pc_chroma_tiles_stitch).
 *
 * A format is pc_chroma.h's five integers:
 *   layout  PC_CHT_PLANAR      Cb (i, j) at u[i*u_row + j], Cr at v[i*v_row + j]
 *           PC_CHT_SEMIPLANAR  Cb at u[i*u_row + 2j], Cr one element after it; v is ignored
 *   bits    8 (elements are bytes) or 10 (elements are little-endian 16-bit words)
 *   shift   the bits below the code in an element: 0 for bits = 8; 0 or 6 for bits = 10.  code = (element >> shift) & (2^bits - 1)
 *           on input (the other bits of a word are ignored), element = code << shift on output
 *   sx, sy  luma samples per chroma sample along a row and along a column: (2, 2) 4:2:0, (2, 1) 4:2:2, (1, 1) 4:4:4
 * and a siting is two values, one per axis: PC_CHT_CENTRE or PC_CHT_COSITED (chroma sample j lies on luma sample 2j); an axis that
 * is not subsampled ignores its value.  A frame (pc_cht_frame, a typedef of the one record pc_frame, pc_yuv_frame.h) is ONE picture
 * of H x W luma samples (Y (r, q) at y[r*y_row + q]) with Hc x Wc chroma samples, Hc = ceil(H / sy), Wc = ceil(W / sx), as strided
 * planes; the batch strides are ignored.  Strides are in ELEMENTS.  y_row >= W, u_row >= 2*Wc (semi-planar) or Wc, v_row >= Wc.  A
 * pointer needs the alignment of its element only.  The planes of a destination must not overlap each other (the caller's to keep).
 *
 * Levels (n = bits, s = 2^(n-8)):   PC_CHT_LIMITED  yo = 16s, ys = 219s, co = 128s, cs = 224s
 *                                   PC_CHT_FULL     yo = 0,   ys = 2^n-1, co = 128s, cs = 2^n-1
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
#ifndef PC_CHROMA_TILES_H
#define PC_CHROMA_TILES_H

#include "pcodec.h"
#include "pc_yuv_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PC_CHT_PLANAR = 0, PC_CHT_SEMIPLANAR = 1 };
enum { PC_CHT_LIMITED = PC_YUV_LIMITED, PC_CHT_FULL = PC_YUV_FULL };
enum { PC_CHT_NEAREST = PC_YUV_NEAREST, PC_CHT_LINEAR = PC_YUV_LINEAR };
enum { PC_CHT_CENTRE = 0, PC_CHT_COSITED = 1 };
enum { PC_CHT_CUT = 0, PC_CHT_STITCH = 1 };

typedef pc_frame pc_cht_frame;      /* pc_yuv_frame.h; y_batch, u_batch, v_batch: ignored (one picture per record) */

/* dst[a*ntx + b][0..2][r][q] = (R, G, B) of luma pixel (Y, X) = ((ty0 + a)*S + r, (tx0 + b)*S + q) of the frame where that pixel
 * lies inside H x W, and +0.0f elsewhere: pc_chroma_ingest's arithmetic addressed by frame position.  Per axis, luma index Y against
 * the n = Hc chroma rows of the WHOLE frame gives two taps (i0, w0), (i1, w1), w0 + w1 = 4 (X against Wc likewise):
 *   axis not subsampled                 i0 = Y,      (4, 0)
 *   subsampled, PC_CHT_NEAREST          i0 = Y >> 1, (4, 0), for either siting
 *   subsampled, linear, PC_CHT_CENTRE   i0 = Y >> 1; i1 = i0 + 1 if Y is odd else i0 - 1, clamped to [0, n-1]; (3, 1)
 *   subsampled, linear, PC_CHT_COSITED  i0 = Y >> 1; Y even: (4, 0); Y odd: i1 = min(i0 + 1, n-1), (2, 2)
 * -- the taps clamp at the frame's Hc - 1, Wc - 1, never at a tile's: a tile is the crop of the whole frame's ingest.  With C the Cb
 * or Cr plane of codes:  c16 = sum over a, b of wy_a * wx_b * C[i_a, j_b]   -- integers, exact;
 *   y' = float(Ycode - yo) / float(ys);  cb' = float(c16_b - 16 co) / float(16 cs);  cr' likewise;
 *   R = y' + (cr' * a);  G = (y' - (cb' * b)) - (cr' * c);  B = y' + (cb' * d);  each then fminf(fmaxf(v, 0), 1).
 *   src           the whole H x W frame.
 *   dst           contiguous float32 [nty*ntx][3][T][T]; every element is written (no memset needed).  4-byte aligned.
 *   ty0 .. ntx    a rectangle inside the grid of an H x W frame.
 * One kernel. */
PC_API int pc_chroma_tiles_cut(const pc_cht_frame* src, int layout, int bits, int shift, int sx, int sy, int hsite, int vsite, int range,
                               int upsample, float a, float b, float c, float d, int H, int W, int T, int O, int ty0, int tx0, int nty,
                               int ntx, float* dst, void* stream);

/* Bytes of device workspace pc_chroma_tiles_stitch needs when it is given `ref` for the window (., x0, h, w): 24 bytes (three 64-bit
 * sums) per block of 256 work items; a work item is sy rows of the window by eight luma columns aligned to a multiple of 8 in FRAME
 * columns, so there are ceil(h / sy) * (ceil((x0 + w) / 8) - floor(x0 / 8)) of them.  0 for arguments the call would refuse. */
PC_API size_t pc_chroma_tiles_stitch_workspace_size(int x0, int h, int w, int sy);

/* The window (y0, x0, h, w) of the frame from the decoded tiles of a grid rectangle.  For every luma pixel
 *   m = fmaf(w_t, fminf(fmaxf(v_t, 0), 1), acc)   chained from acc = +0.0f over the covering tiles t in ascending tile index, with
 * w_t = wy * wx (a float32 product) of the correctly rounded band weights of pc_tiles.h; then pc_chroma_emit's arithmetic on m WITH
 * THE FRAME AS THE PICTURE, restricted to the window:
 *   (R, G, B) = fminf(fmaxf(m, 0), 1);  Y' = ((kr * R) + (kg * G)) + (kb * B);  Cb' = (B - Y') * ib;  Cr' = (R - Y') * ir;
 *   Ycode = clampi(rintf((Y' * float(ys)) + float(yo)), 0, 2^n-1);  u = Cb' * float(cs)  (Cr likewise),
 * and a chroma sample filters the u values along rows first, then along columns, by one rule per axis for chroma index j against the
 * N luma samples p[0 .. N-1] of the FRAME (N = W along a row, H along a column; j in frame coordinates):
 *   axis not subsampled   h = p[j],                                                                  scale 1
 *   PC_CHT_CENTRE         h = p[2j] + p[min(2j+1, N-1)],                                              scale 2
 *   PC_CHT_COSITED        a = p[max(2j-1, 0)], b = p[2j], c = p[min(2j+1, N-1)]; h = (a + c) + (b + b),  scale 4
 *   code = clampi(rintf(v * s + float(co)), 0, 2^n-1),  s = 1 / (scale_h * scale_v), a power of two.
 * The indices clamp at the frame's edges, never at the window's, so the window's output is the crop of the whole frame's stitch: luma
 * [y0 : y0+h], chroma [y0/sy : y0/sy + ceil(h/sy)], columns likewise.
 *   x             float32 tile set of the rectangle: element (t, c, r, q) at x[t*sxt + c*sxc + r*sxh + q]; sxh >= T; 4-byte aligned.
 *   window        inside the frame and ADMISSIBLE: y0 % sy == 0 and x0 % sx == 0, h % sy == 0 or y0 + h == H, w % sx == 0 or
 *                 x0 + w == W (at 4:4:4 every window, at 4:2:2 every y0 and h).
 *   the halo      under a co-sited horizontal axis (sx == 2, hsite == PC_CHT_COSITED) the first chroma sample of a window with
 *                 x0 > 0 reads frame column x0 - 1; under a co-sited vertical axis (sy == 2, vsite == PC_CHT_COSITED) with y0 > 0 the
 *                 first chroma row reads frame row y0 - 1.  Those pixels are blended from the tiles like any other, so the rectangle
 *                 must hold EVERY tile that covers a pixel of the window EXTENDED BY ITS HALO (one column left and / or one row
 *                 above where the rule applies) -- checked.  With O = 0 and x0 on a tile origin that is one more tile column than
 *                 pc_frame_tiles_stitch would need.
 *   dst           frame of the window (h x w luma, ceil(h/sy) x ceil(w/sx) chroma), addressed relative to the window's first sample;
 *                 elements outside its samples are not touched.  NULL with ref: the sums only.  The row strides of dst and of
 *                 ref must be below 2^31 elements (the kernels hold them in 32 bits); PC_ERR_ARG otherwise.
 *   ref           optional frame of the same format: the original's window, addressed like dst (luma from (y0, x0), chroma from
 *                 (y0/sy, x0/sx)).  With it (then workspace and sse are required):
 *     sse[p]      p = 0, 1, 2 for Y, Cb, Cr: the sum over the window of (code - refcode)^2 in unsigned 64-bit integers, exact.  No
 *                 atomics: thread, wave tree, waves in order, one 24-byte partial per block (into the workspace), then one ordered
 *                 reduction launch.  Every element is written.
 *   workspace     at least pc_chroma_tiles_stitch_workspace_size(x0, h, w, sy) bytes; PC_ERR_ARG if smaller.  Unused without ref.
 *                 workspace and sse are 8-byte aligned.
 * One kernel, plus the ordered reduction when ref is given. */
PC_API int pc_chroma_tiles_stitch(const float* x, int64_t sxt, int64_t sxc, int64_t sxh, int H, int W, int T, int O, int ty0, int tx0,
                                  int nty, int ntx, int y0, int x0, int h, int w, int layout, int bits, int shift, int sx, int sy,
                                  int hsite, int vsite, int range, float kr, float kg, float kb, float ib, float ir,
                                  const pc_cht_frame* dst, const pc_cht_frame* ref, void* workspace, size_t workspace_bytes, uint64_t* sse,
                                  void* stream);

/* Host only, launches nothing: *wide = 1 where the cut (op = PC_CHT_CUT: frame is src, f32 is dst with strides 3*T*T, T*T, T; x0 is
 * ignored) or the stitch (op = PC_CHT_STITCH: frame is dst, f32 is x, x0 the window's first column; O is ignored) with these
 * arguments moves four elements of a plane per access (a 32-bit word of an 8-bit plane, a 64-bit word of a 16-bit plane) and four
 * floats per access (128 bits), 0 where it moves them one by one.  Both give the same bits, sums included: the paths differ in
 * instructions only, never in which thread owns which sample or in the order of additions.  A work item is eight consecutive columns:
 * of one tile row, aligned in TILE columns, for the cut; of sy rows of the window, aligned to a multiple of 8 in FRAME columns, for
 * the stitch.  Preconditions of the wide path:
 *   - the f32 pointer 16-byte aligned and its three strides multiples of 4;
 *   - every plane's row stride a multiple of 4;
 *   - the address of the first element an item touches in every plane aligned to four elements.  For the cut that is: every plane
 *     pointer aligned to four elements and, at sx == 2, O a multiple of 8 (S is then a multiple of 8, an item's first luma column a
 *     multiple of 8 in the frame and its first chroma column a multiple of 4; with O = 4 a tile's first chroma column is 2 mod 4).
 *     At sx == 1 (4:4:4) a chroma column is a luma column and S is always a multiple of 4: every O qualifies.  For the stitch it is
 *     the address of frame column 8*floor(x0 / 8) in dst and in ref: with k = x0 % 8, y - k; for the chroma planes u - k (semi-planar,
 *     sx == 2), u - 2k (semi-planar, sx == 1), u - k/2 and v - k/2 (planar, sx == 2), u - k and v - k (planar, sx == 1), in elements.
 * Items that straddle an edge of the frame or of the window go element by element on either path.  `ref` may be NULL; for the
 * stitch `frame` may be NULL when `ref` is not (sums only).  The calls decide with the same code.  PC_ERR_ARG for an unknown op,
 * layout, depth or sx, NULL pointers, O < 0, or x0 negative or not a multiple of sx. */
PC_API int pc_chroma_tiles_plan(int op, int layout, int bits, int sx, const pc_cht_frame* frame, const void* f32, int64_t ft, int64_t fc,
                                int64_t fh, int O, int x0, const pc_cht_frame* ref, int* wide);

PC_API const char* pc_chroma_tiles_strerror(int code);
PC_API int pc_chroma_tiles_last_hip_error(void);

#ifdef __cplusplus
}
#endif

#endif /* PC_CHROMA_TILES_H */

/* pc_chroma_rate.h -- C ABI of libpc_chroma_rate.so: the per-tile, per-plane weighted squared error of decoded float32 RGB tiles
 * against the original YUV frame in any of pc_chroma.h's twelve formats (4:2:0 / 4:2:2 / 4:4:4, planar or semi-planar, 8-bit or 10-bit)
 * and three chroma sitings, measured in the frame's own code domain, on gfx950.  DESIGN.md section 24: the composition of section 21's
 * emit (pc_chroma.h), section 11's geometry (pc_tiles.h) and section 12's integer band weights (pc_rate.h).  It is what
 * rate-controlled tiled coding of those frames (chroma_rate.py) allocates bytes by; what pc_frame_rate.h (section 15) is for NV12 /
 * I420 / P010 with centre-sited chroma, and bit for bit that there.
 *
 * Kept apart from libpcodec.so and from the other image-side libraries; no library of the image domain links another (what this one
 * shares with them comes from the headers of image_csrc/).  Plain C, the conventions of pc_frame_rate.h and
 * pc_chroma_tiles.h: device pointers, int64 strides in ELEMENTS, status codes PC_OK / PC_ERR_* (pcodec.h), `stream` is a hipStream_t
 * passed as void* (NULL = default stream).  No call allocates device memory or synchronises the host: the caller passes the
 * workspace, and every launch is ordered on `stream`.  Every argument is checked before the first HIP call; a call that returns
 * PC_ERR_ARG has launched nothing.  All offsets are 64-bit.
 *
 * A format is pc_chroma.h's five integers:
 *   layout  PC_CHR_PLANAR      Cb (i, j) at u[i*u_row + j], Cr at v[i*v_row + j]
 *           PC_CHR_SEMIPLANAR  Cb at u[i*u_row + 2j], Cr one element after it; v is ignored
 *   bits    8 (elements are bytes) or 10 (elements are little-endian 16-bit words)
 *   shift   the bits below the code in an element: 0 for bits = 8; 0 or 6 for bits = 10.  code = (element >> shift) & (2^bits - 1)
 *           (the other bits of a word are ignored)
 *   sx, sy  luma samples per chroma sample along a row and along a column: (2, 2) 4:2:0, (2, 1) 4:2:2, (1, 1) 4:4:4
 * and a siting is two values, one per axis: PC_CHR_CENTRE or PC_CHR_COSITED (chroma sample j lies on luma sample 2j); an axis that
 * is not subsampled ignores its value.  A frame (pc_chr_frame, a typedef of the one record pc_frame, pc_yuv_frame.h) is ONE picture
 * of H x W luma samples (Y (r, q) at y[r*y_row + q]) with Hc x Wc chroma samples, Hc = ceil(H / sy), Wc = ceil(W / sx), as strided
 * planes; the batch strides are ignored.  y_row >= W, u_row >= 2*Wc (semi-planar) or Wc, v_row >= Wc.  A pointer needs the alignment
 * of its element only.
 *
 * Levels (n = bits, s = 2^(n-8)):   PC_CHR_LIMITED  yo = 16s, ys = 219s, co = 128s, cs = 224s
 *                                   PC_CHR_FULL     yo = 0,   ys = 2^n-1, co = 128s, cs = 2^n-1
 * The colour coefficients are plain float arguments, computed by the caller.  Every float product and sum below is one IEEE float32
 * operation (the library is built with -ffp-contract=off); everything that is accumulated is an integer.
 *
 * Geometry (pc_tiles.h, unchanged).  Tile size T, a multiple of 64, at most 2048 (bits = 8) or 1024 (bits = 10); overlap O, a
 * multiple of 4 with 0 <= O <= T/2; stride S = T - O.  Along an axis of length L there is 1 tile if L <= T, otherwise
 * ceil((L - T) / S) + 1.  Tiles are numbered row-major over the ny x nx grid; tile (i, j) covers rows [i*S, i*S + T) and columns
 * [j*S, j*S + T) of the frame, of which hh = min(T, H - i*S) rows and ww = min(T, W - j*S) columns lie inside it.
 *
 * Two consequences of the contract below.
 *   Identity with pc_frame_rate.h.  For (semi-planar, 8, 0, 2, 2), (planar, 8, 0, 2, 2) and (semi-planar, 10, 6, 2, 2) with both
 *   sitings PC_CHR_CENTRE every sum is pc_frame_rate_tile_sse's for NV12, I420 and P010, bit for bit.
 *   Relation to pc_chroma_tiles_stitch's sums at O = 0.  The sum over all tiles of out[t][p] equals the stitch's sse[p] of the whole
 *   frame exactly for luma, and for chroma on every axis that is not both subsampled and co-sited.  On a co-sited subsampled axis the
 *   first chroma column (row) of a tile with j > 0 (i > 0) reads its own first pixel where the stitch reads the neighbouring tile's
 *   last: the sums may differ in those samples and nowhere else.  A tile never reads another tile: the measurement stays separable
 *   across the tiles' levels, which is what the allocator needs.
 */
#ifndef PC_CHROMA_RATE_H
#define PC_CHROMA_RATE_H

#include "pcodec.h"
#include "pc_yuv_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PC_CHR_PLANAR = 0, PC_CHR_SEMIPLANAR = 1 };
enum { PC_CHR_LIMITED = PC_YUV_LIMITED, PC_CHR_FULL = PC_YUV_FULL };
enum { PC_CHR_CENTRE = 0, PC_CHR_COSITED = 1 };

typedef pc_frame pc_chr_frame;      /* pc_yuv_frame.h; y_batch, u_batch, v_batch: ignored (one picture per record) */

/* Bytes of device workspace pc_chroma_rate_tile_sse needs: 24 bytes (three 64-bit sums) per block of 256 work items; a work item is
 * sy rows of one tile by eight tile-aligned columns, so a tile has T*T/(8*sy) of them (a multiple of 256 for every admissible T) and
 * T*T/(2048*sy) blocks.  0 for arguments the call would refuse (T no multiple of 64 or above 2048, sy not 1 or 2, n_tiles < 1). */
PC_API size_t pc_chroma_rate_workspace_size(int T, int sy, int n_tiles);

/* out[t][p], p = 0, 1, 2 for Y, Cb, Cr, of the tiles first_tile .. first_tile + n_tiles - 1 (a LINEAR range of the row-major grid,
 * tile first_tile + t at x + t*sxt).  A tile is judged by its own rendering: pc_chroma_emit's arithmetic with the tile's in-frame
 * part hh x ww as the picture, in that kernel's order of operations:
 *   (R, G, B) = fminf(fmaxf(v, 0), 1) (NaN -> 0);  Y' = ((kr * R) + (kg * G)) + (kb * B);  Cb' = (B - Y') * ib;  Cr' = (R - Y') * ir;
 *   Ycode(r, q) = clampi(rintf((Y' * float(ys)) + float(yo)), 0, 2^n-1);  u = Cb' * float(cs)  (Cr likewise)        r < hh, q < ww
 * and a chroma sample filters the u values along rows first, then along columns, by one rule per axis for chroma index m against
 * the N luma samples p[0 .. N-1] of the TILE'S IN-FRAME PART (N = ww along a row, hh along a column; m in tile coordinates):
 *   axis not subsampled   h = p[m],                                                                  scale 1
 *   PC_CHR_CENTRE         h = p[2m] + p[min(2m+1, N-1)],                                              scale 2
 *   PC_CHR_COSITED        a = p[max(2m-1, 0)], b = p[2m], c = p[min(2m+1, N-1)]; h = (a + c) + (b + b),  scale 4
 *   code(k, m) = clampi(rintf(v * s + float(co)), 0, 2^n-1),  s = 1 / (scale_h * scale_v), a power of two.       k < ceil(hh/sy),
 * Every clamp of the filter is at the tile's in-frame part, never at the frame's and never in another tile.       m < ceil(ww/sx)
 * The codes are compared with the original's codes (code = (element >> shift) & (2^n - 1)): luma sample (r, q) at frame position
 * (i*S + r, j*S + q), chroma sample (k, m) at (i*S/sy + k, j*S/sx + m)  (S is a multiple of 4: a tile's chroma cells are the frame's).
 * With ay(r), ax(q) the integer numerators of the band weights over den = 2*O (den = 1 for O = 0; pc_rate.h):
 *   2u + 1 where the tile is not the first along the axis and u < O; 2(O - 1 - (u - S)) + 1 where it is not the last and u >= S; den
 *   elsewhere; and cy(k) = (ay(2k) + ay(2k+1)) / 2 at sy == 2 (an integer: O and S are even), ay(k) at sy == 1; cx(m) likewise with
 *   sx.  The weights depend on the subsampling, never on the siting; per sample of the frame they sum to den^2 over the covering tiles.
 *   out[t][0] = sum ay(r) ax(q) e^2,   out[t][1], out[t][2] = sum cy(k) cx(m) e^2      in unsigned 64-bit integers, exact:
 *   T^4 (2^n - 1)^2 < 2^60 for T <= 2048 at 8 bits and T <= 1024 at 10, for chroma at 4:4:4 just as for luma.
 *   x             float32 tile set: element (t, c, r, q) at x[t*sxt + c*sxc + r*sxh + q]; sxh >= T; 4-byte aligned.
 *   ref           the WHOLE original H x W frame in the format.
 *   workspace     at least pc_chroma_rate_workspace_size(T, sy, n_tiles) bytes, 8-byte aligned; PC_ERR_ARG if smaller.
 *   out           uint64 [n_tiles][3], 8-byte aligned; every element is written.
 * No atomics: thread, wave tree, the block's waves in order (into the workspace), then one wave per tile over its block partials.
 * Two launches. */
PC_API int pc_chroma_rate_tile_sse(const float* x, int64_t sxt, int64_t sxc, int64_t sxh, int H, int W, int T, int O, int first_tile,
                                   int n_tiles, int layout, int bits, int shift, int sx, int sy, int hsite, int vsite, int range,
                                   float kr, float kg, float kb, float ib, float ir, const pc_chr_frame* ref, void* workspace,
                                   size_t workspace_bytes, uint64_t* out, void* stream);

/* Host only, launches nothing: *wide = 1 where pc_chroma_rate_tile_sse with these arguments moves four floats per access (128 bits)
 * and four elements of a plane per access (a 32-bit word of an 8-bit plane, a 64-bit word of a 16-bit plane), 0 where it moves them
 * one by one.  Both give the same bits.  The wide path needs: the float pointer 16-byte aligned and its strides multiples of 4;
 * every plane pointer of ref aligned to four elements and every row stride a multiple of 4; at sx == 2, O a multiple of 8 (S is
 * then one, a work item's first luma column a multiple of 8 in the frame and its first chroma column a multiple of 4); at sx == 1
 * every O qualifies.  Items that straddle an edge of the frame go element by element on either path.  The call decides with the
 * same code.  PC_ERR_ARG for an unknown layout, depth or sx, NULL pointers or O < 0. */
PC_API int pc_chroma_rate_plan(const void* x, int64_t sxt, int64_t sxc, int64_t sxh, int O, int layout, int bits, int sx,
                               const pc_chr_frame* ref, int* wide);

PC_API const char* pc_chroma_rate_strerror(int code);
PC_API int pc_chroma_rate_last_hip_error(void);

#ifdef __cplusplus
}
#endif

#endif /* PC_CHROMA_RATE_H */

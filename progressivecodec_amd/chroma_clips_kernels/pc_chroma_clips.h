/* pc_chroma_clips.h -- C ABI of libpc_chroma_clips.so: what a CLIP of YUV frames of any of pc_chroma.h's twelve formats (4:2:0 / 4:2:2 /
 * 4:4:4, planar or semi-planar, 8-bit or 10-bit) and three chroma sitings needs beyond one frame, on gfx950.
 * pc_chroma_clips_tile_changes counts, per tile and plane, the samples of the tile's FOOTPRINT whose codes differ between two frames (a
 * tile whose three counts are zero would be cut, and so coded, to exactly the bytes it had in the previous frame);
 * pc_chroma_clips_cut_list cuts a LIST of tiles, scattered over the grid, into float32 RGB tiles in one launch (pc_chroma_tiles_cut
 * takes grid rectangles only).  DESIGN.md section 25: what pc_clips.h (section 16) is for NV12 / I420 / P010 with centre-sited chroma,
 * on top of section 23 (pc_chroma_tiles.h: the cut) and section 11 (pc_tiles.h: geometry).
 *
 * Kept apart from libpcodec.so and from the other image-side libraries; no library of the image domain links another.  Plain C, the
 * conventions of pc_clips.h and pc_chroma_tiles.h: device pointers, int64 strides in ELEMENTS, status codes PC_OK / PC_ERR_*
 * (pcodec.h), `stream` is a hipStream_t passed as void* (NULL = default stream).  No call allocates device memory or synchronises the
 * host: the caller passes the workspace, and every launch is ordered on `stream`.  Every argument is checked before the first HIP
 * call; a call that returns PC_ERR_ARG has launched nothing.  All offsets are 64-bit.
 *
 * A format is pc_chroma.h's five integers:
 *   layout  PC_CHC_PLANAR      Cb (i, j) at u[i*u_row + j], Cr at v[i*v_row + j]
 *           PC_CHC_SEMIPLANAR  Cb at u[i*u_row + 2j], Cr one element after it; v is ignored
 *   bits    8 (elements are bytes) or 10 (elements are little-endian 16-bit words)
 *   shift   the bits below the code in an element: 0 for bits = 8; 0 or 6 for bits = 10.  code = (element >> shift) & (2^bits - 1):
 *           the other bits of a word are ignored, and two frames that differ in them alone are equal
 *   sx, sy  luma samples per chroma sample along a row and along a column: (2, 2) 4:2:0, (2, 1) 4:2:2, (1, 1) 4:4:4
 * and a siting is two values, one per axis: PC_CHC_CENTRE or PC_CHC_COSITED (chroma sample j lies on luma sample 2j); an axis that
 * is not subsampled ignores its value.  A frame (pc_chc_frame, a typedef of the one record pc_frame, pc_yuv_frame.h) is ONE picture
 * of H x W luma samples with Hc x Wc chroma samples, Hc = ceil(H / sy), Wc = ceil(W / sx), as strided planes; the batch strides are
 * ignored.  y_row >= W, u_row >= 2*Wc (semi-planar) or Wc, v_row >= Wc.  A pointer needs the alignment of its element only.
 *
 * Geometry (pc_tiles.h).  Tile size T, a multiple of 64, at most 2048; overlap O, a multiple of 4 with 0 <= O <= T/2; stride
 * S = T - O.  Along an axis of length L there is 1 tile if L <= T, otherwise ceil((L - T) / S) + 1.  Tiles are numbered row-major
 * over the ny x nx grid.
 *
 * Footprint (the contract).  Along an axis of length L, with e = min(i*S + T, L), tile i reads
 *   luma positions      [i*S, e)
 *   chroma positions    [i*S, e - 1]                                                  where the axis is not subsampled (sx or sy = 1),
 *                       whatever the siting and the upsampling, and otherwise, with Lc = ceil(L / 2),
 *                       [max(i*S/2 - lo, 0), min(ceil(e/2) - 1 + hi, Lc - 1)]
 *                       hi = 1 for PC_CHC_LINEAR, else 0;  lo = 1 for PC_CHC_LINEAR and PC_CHC_CENTRE on that axis, else 0.
 * The centre-sited linear rule gives an even luma index the chroma sample before its own and an odd one the sample after it; the
 * co-sited rule gives an even luma index one tap and an odd one the sample after it, so it never reaches below i*S/2 (i*S is even);
 * nearest upsampling takes one sample.  The footprint of tile (i, j) is the product of the two axes' ranges, once in the luma plane
 * and once each in Cb and Cr (the same rectangle).  It is exactly the set of samples pc_chroma_tiles_cut reads with a non-zero
 * weight for the tile: every sample the cut reads lies in it, and every sample in it is read.  For centre-sited 4:2:0 it is
 * pc_clips.h's footprint.
 */
#ifndef PC_CHROMA_CLIPS_H
#define PC_CHROMA_CLIPS_H

#include "pcodec.h"
#include "pc_yuv_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PC_CHC_PLANAR = 0, PC_CHC_SEMIPLANAR = 1 };
enum { PC_CHC_LIMITED = PC_YUV_LIMITED, PC_CHC_FULL = PC_YUV_FULL };
enum { PC_CHC_NEAREST = PC_YUV_NEAREST, PC_CHC_LINEAR = PC_YUV_LINEAR };
enum { PC_CHC_CENTRE = 0, PC_CHC_COSITED = 1 };
enum { PC_CHC_CHANGES = 0, PC_CHC_CUT = 1 };

typedef pc_frame pc_chc_frame;      /* pc_yuv_frame.h; y_batch, u_batch, v_batch: ignored (one picture per record) */

/* Bytes of device workspace pc_chroma_clips_tile_changes needs: 24 bytes (three 64-bit counts) per block, T*T/(2048*sy) + 1 blocks
 * per tile: a work item is sy luma rows of one tile by eight tile-aligned luma columns with the 8 / sx chroma samples of its cells,
 * a block holds 256 of them, and one more block per tile takes the halo ring.  0 for arguments the call would refuse (T no multiple
 * of 64 or above 2048, sy neither 1 nor 2, n_tiles < 1, 2^31 blocks or more). */
PC_API size_t pc_chroma_clips_changes_workspace_size(int T, int sy, int n_tiles);

/* out[t][p], p = 0, 1, 2 for Y, Cb, Cr, of the tiles first_tile .. first_tile + n_tiles - 1 (a LINEAR range of the row-major grid):
 * the number of samples of plane p in the tile's footprint whose codes differ between cur and prev.  Exact integers: the result does
 * not depend on order, access path or tile range.
 *   cur, prev     two WHOLE H x W frames of the format; they may be pitched differently.
 *   hsite, vsite, upsample   the siting and the upsampling the tiles are to be cut with: they choose the footprint's halo.
 *   workspace     at least pc_chroma_clips_changes_workspace_size(T, sy, n_tiles) bytes, 8-byte aligned; PC_ERR_ARG if smaller.
 *                 Every partial is written, nothing after them.
 *   out           uint64 [n_tiles][3], 8-byte aligned; every element is written.
 * No atomics: thread, wave tree, the block's waves in order (into the workspace), then one wave per tile over its block partials.
 * Two launches. */
PC_API int pc_chroma_clips_tile_changes(const pc_chc_frame* cur, const pc_chc_frame* prev, int layout, int bits, int shift, int sx, int sy,
                                        int hsite, int vsite, int upsample, int H, int W, int T, int O, int first_tile, int n_tiles,
                                        void* workspace, size_t workspace_bytes, uint64_t* out, void* stream);

/* dst[m][0..2][r][q] = (R, G, B) of luma pixel (Y, X) = (ti*S + r, tj*S + q) of the frame, (ti, tj) = (tiles[m] / nx, tiles[m] % nx),
 * where that pixel lies inside H x W, and +0.0f elsewhere: bit for bit what pc_chroma_tiles_cut writes for the rectangle
 * (ti, tj, 1, 1) -- pc_chroma_tiles.h's arithmetic, its taps clamped at the FRAME's edges.
 *   src           the whole H x W frame.
 *   tiles         DEVICE array of n int32 tile indices, row-major in the WHOLE grid, in any order, repeats allowed; 4-byte aligned.
 *                 The host cannot check device memory, so the kernel does: an index outside [0, ny*nx) gives a tile of +0.0f and
 *                 never an access outside the frame.
 *   dst           contiguous float32 [n][3][T][T]; every element is written (no memset needed).  4-byte aligned.
 * One kernel. */
PC_API int pc_chroma_clips_cut_list(const pc_chc_frame* src, int layout, int bits, int shift, int sx, int sy, int hsite, int vsite, int range,
                                    int upsample, float a, float b, float c, float d, int H, int W, int T, int O, const int32_t* tiles, int n,
                                    float* dst, void* stream);

/* Host only, launches nothing: *wide = 1 where the call moves four elements of a plane per access (a 32-bit word of an 8-bit plane,
 * a 64-bit word of a 16-bit plane) and, for the cut, four floats per access (128 bits); 0 where it moves them one by one.  Both give
 * the same bits and the same counts.
 *   op = PC_CHC_CHANGES   pc_chroma_clips_tile_changes with frame = cur and other = prev; f32 is ignored.
 *   op = PC_CHC_CUT       pc_chroma_clips_cut_list with frame = src and f32 = dst; other is ignored.
 * The wide path needs: every plane pointer (of both frames for the changes) aligned to four elements and every row stride a
 * multiple of 4; at sx == 2 O a multiple of 8 (S is then one, a work item's first luma column a multiple of 8 in the frame and its
 * first chroma column a multiple of 4; with O = 4 a tile's first chroma column is 2 mod 4), at sx == 1 every O qualifies (a chroma
 * column is a luma column, and S is always a multiple of 4); for the cut the float pointer 16-byte aligned.  Items that straddle an
 * edge of the frame, and the halo ring of the changes, go element by element on either path.  The calls decide with the same code.
 * PC_ERR_ARG for an unknown op, layout, depth or sx, NULL pointers or O < 0. */
PC_API int pc_chroma_clips_plan(int op, int layout, int bits, int sx, const pc_chc_frame* frame, const pc_chc_frame* other, const void* f32,
                                int O, int* wide);

PC_API const char* pc_chroma_clips_strerror(int code);
PC_API int pc_chroma_clips_last_hip_error(void);

#ifdef __cplusplus
}
#endif

#endif /* PC_CHROMA_CLIPS_H */

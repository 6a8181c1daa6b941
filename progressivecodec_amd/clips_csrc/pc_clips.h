/* pc_clips.h -- C ABI of libpc_clips.so: what a CLIP of YUV 4:2:0 frames (NV12 / I420 / P010) needs beyond one frame, on gfx950.
 * pc_clips_tile_changes counts, per tile and plane, the samples of the tile's FOOTPRINT whose codes differ between two frames (a tile
 * whose three counts are zero would be cut, and so coded, to exactly the bytes it had in the previous frame); pc_clips_cut_list cuts
 * a LIST of tiles, scattered over the grid, into float32 RGB tiles in one launch (pc_frame_tiles_cut takes grid rectangles only).
 * on top of section 14 (pc_frame_tiles.h: the cut) and section 11 (pc_tiles.h: geometry).
 *
 * Kept apart from libpcodec.so and from the other image-side libraries (libpc_pixels.so, libpc_tiles.so, libpc_rate.so,
 * libpc_frames.so, libpc_frame_tiles.so, libpc_frame_rate.so): nothing here is part of the codec's numeric contract, byte strings or
 * profiles, and no library of the image domain links another (the device code this one shares with pc_frame_tiles.hip -- plane
 * loads, levels, the ingest arithmetic -- comes from the headers of image_csrc/).  Plain C, the conventions of
 * pc_frame_rate.h: device pointers, int64
 * strides in ELEMENTS, status codes PC_OK / PC_ERR_* (pcodec.h), `stream` is a hipStream_t passed as void* (NULL = default stream).
 * No call allocates device memory or synchronises the host: the caller passes the workspace, and every launch is ordered on
 * `stream`.  Every argument is checked before the first HIP call; a call that returns PC_ERR_ARG has launched nothing.  All offsets
 * are 64-bit.
 *
 * A frame (pc_cl_frame, a typedef of the one record pc_frame, pc_yuv_frame.h) is ONE picture of H x W luma samples with Hc x Wc
 * chroma samples, Hc = ceil(H/2), Wc = ceil(W/2), as strided planes; the batch strides are ignored.
 *   PC_CL_NV12  Y (r, q) at y[r*y_row + q];  Cb (i, j) at u[i*u_row + 2j], Cr one element after it;  v is ignored.  8-bit codes.
 *   PC_CL_I420  Y as above;  Cb at u[i*u_row + j], Cr at v[i*v_row + j].  8-bit codes.
 *   PC_CL_P010  the layout of NV12 in 16-bit words, code = word >> 6 (the low six bits are ignored: two frames that differ in them
 *               alone are equal).
 * y_row >= W, u_row >= 2*Wc (interleaved) or Wc, v_row >= Wc.  A pointer needs the alignment of its element only.
 *
 * Geometry (pc_tiles.h).  Tile size T, a multiple of 64, at most 2048; overlap O, a multiple of 4 with 0 <= O <= T/2; stride
 * S = T - O.  Along an axis of length L there is 1 tile if L <= T, otherwise ceil((L - T) / S) + 1.  Tiles are numbered row-major
 * over the ny x nx grid.
 *
 * Footprint.  With halo = 1 for PC_CL_LINEAR and 0 for PC_CL_NEAREST, along an axis of length L with Lc = ceil(L / 2), tile i reads
 *   luma positions    [i*S, e),  e = min(i*S + T, L)
 *   chroma positions  [max(i*S/2 - halo, 0), min(ceil(e/2) - 1 + halo, Lc - 1)]
 * and the footprint of tile (i, j) is the product of the two axes' ranges, once in the luma plane and once each in Cb and Cr (the
 * same rectangle).  The halo is the neighbouring chroma sample the linear upsampling of the cut takes: luma row i*S (even) takes
 * chroma row i*S/2 - 1, an odd last luma row the chroma row after it, the taps clamped at the frame's edges.  Every sample the cut
 * reads for a tile lies in its footprint.
 */
#ifndef PC_CLIPS_H
#define PC_CLIPS_H

#include "pcodec.h"
#include "pc_yuv_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PC_CL_NV12 = PC_YUV_NV12, PC_CL_I420 = PC_YUV_I420, PC_CL_P010 = PC_YUV_P010 };
enum { PC_CL_LIMITED = PC_YUV_LIMITED, PC_CL_FULL = PC_YUV_FULL };
enum { PC_CL_NEAREST = PC_YUV_NEAREST, PC_CL_LINEAR = PC_YUV_LINEAR };
enum { PC_CL_CHANGES = 0, PC_CL_CUT = 1 };

typedef pc_frame pc_cl_frame;       /* pc_yuv_frame.h; y_batch, u_batch, v_batch: ignored (one picture per record) */

/* Bytes of device workspace pc_clips_tile_changes needs: 24 bytes (three 64-bit counts) per block, T*T/4096 + 1 blocks per tile:
 * a work item is one row pair of one tile by eight tile-aligned luma columns with the four chroma sample pairs of its 2 x 2 cells, a
 * block holds 256 of them, and one more block per tile takes the halo ring.  0 for arguments the call would refuse (T no multiple of
 * 64 or above 2048, n_tiles < 1). */
PC_API size_t pc_clips_changes_workspace_size(int T, int n_tiles);

/* out[t][p], p = 0, 1, 2 for Y, Cb, Cr, of the tiles first_tile .. first_tile + n_tiles - 1 (a LINEAR range of the row-major grid):
 * the number of samples of plane p in the tile's footprint whose codes differ between cur and prev.  Exact integers: the result does
 * not depend on order, access path or tile range.
 *   cur, prev     two WHOLE H x W frames in `fmt`; they may be pitched differently.
 *   upsample      PC_CL_LINEAR (halo 1) or PC_CL_NEAREST (halo 0): the upsampling the tiles are to be cut with.
 *   workspace     at least pc_clips_changes_workspace_size(T, n_tiles) bytes, 8-byte aligned; PC_ERR_ARG if smaller.
 *   out           uint64 [n_tiles][3], 8-byte aligned; every element is written.
 * No atomics: thread, wave tree, the block's waves in order (into the workspace), then one wave per tile over its block partials.
 * Two launches. */
PC_API int pc_clips_tile_changes(const pc_cl_frame* cur, const pc_cl_frame* prev, int fmt, int upsample, int H, int W, int T, int O,
                                 int first_tile, int n_tiles, void* workspace, size_t workspace_bytes, uint64_t* out, void* stream);

/* dst[m][0..2][r][q] = (R, G, B) of luma pixel (Y, X) = (ti*S + r, tj*S + q) of the frame, (ti, tj) = (tiles[m] / nx, tiles[m] % nx),
 * where that pixel lies inside H x W, and +0.0f elsewhere: bit for bit what pc_frame_tiles_cut writes for the rectangle
 * (ti, tj, 1, 1) -- pc_frame_tiles.h's arithmetic.  With C the Cb or Cr plane of codes of the WHOLE frame:
 *   i0 = Y >> 1, i1 = i0 + 1 if Y is odd else i0 - 1, clamped to [0, Hc-1]; j0, j1 likewise from X and Wc;
 *   c16 = 9 C[i0,j0] + 3 C[i0,j1] + 3 C[i1,j0] + C[i1,j1]   (PC_CL_LINEAR)   or   16 C[i0,j0]   (PC_CL_NEAREST)  -- integers, exact;
 *   y' = float(Ycode - yo) / float(ys);  cb' = float(c16_b - 16 co) / float(16 cs);  cr' likewise;
 *   R = y' + (cr' * a);  G = (y' - (cb' * b)) - (cr' * c);  B = y' + (cb' * d);  each then fminf(fmaxf(v, 0), 1)
 * with the levels (n = 8 or 10 bits, s = 2^(n-8)) PC_CL_LIMITED yo = 16s, ys = 219s, co = 128s, cs = 224s and PC_CL_FULL yo = 0,
 * ys = 2^n-1, co = 128s, cs = 2^n-1; every product, sum and quotient is one IEEE float32 operation (-ffp-contract=off).
 *   src           the whole H x W frame.
 *   tiles         DEVICE array of n int32 tile indices, row-major in the WHOLE grid, in any order, repeats allowed; 4-byte aligned.
 *                 The host cannot check device memory, so the kernel does: an index outside [0, ny*nx) gives a tile of +0.0f and
 *                 never an access outside the frame.
 *   dst           contiguous float32 [n][3][T][T]; every element is written (no memset needed).  4-byte aligned.
 * One kernel. */
PC_API int pc_clips_cut_list(const pc_cl_frame* src, int fmt, int range, int upsample, float a, float b, float c, float d, int H, int W,
                             int T, int O, const int32_t* tiles, int n, float* dst, void* stream);

/* Host only, launches nothing: *wide = 1 where the call moves four elements of a plane per access (a 32-bit word of an 8-bit plane,
 * a 64-bit word of a 16-bit plane) and, for the cut, four floats per access (128 bits); 0 where it moves them one by one.  Both give
 * the same bits and the same counts.
 *   op = PC_CL_CHANGES   pc_clips_tile_changes with frame = cur and other = prev; f32 is ignored.
 *   op = PC_CL_CUT       pc_clips_cut_list with frame = src and f32 = dst; other is ignored.
 * The wide path needs: every plane pointer (of both frames for the changes) aligned to four elements and every row stride a
 * multiple of 4; O a multiple of 8 (S is then one, a work item's first luma column a multiple of 8 in the frame and its first
 * chroma column a multiple of 4; with O = 4 a tile's first chroma column is 2 mod 4); for the cut the float pointer 16-byte aligned.
 * Items that straddle an edge of the frame, and the halo ring of the changes, go element by element on either path.  The calls
 * decide with the same code.  PC_ERR_ARG for an unknown op or format, NULL pointers or O < 0. */
PC_API int pc_clips_plan(int op, int fmt, const pc_cl_frame* frame, const pc_cl_frame* other, const void* f32, int O, int* wide);

PC_API const char* pc_clips_strerror(int code);
PC_API int pc_clips_last_hip_error(void);

#ifdef __cplusplus
}
#endif

#endif /* PC_CLIPS_H */

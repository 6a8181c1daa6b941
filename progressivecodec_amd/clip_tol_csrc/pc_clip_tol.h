/* pc_clip_tol.h -- C ABI of libpc_clip_tol.so: the TOLERANT scan of a clip of YUV 4:2:0 frames (NV12 / I420 / P010) on gfx950.  For
 * every frame k >= 1 and every tile t it measures the tile's footprint in frame k against the frame the tile was LAST CODED in (its
 * anchor) -- how many codes differ, the sum of their squared differences, the largest absolute difference, per plane -- and decides,
 * on the device, whether the tile is close enough to be shown from its anchor's bytes once more.  Because the comparison is against
 * the anchor and never against the previous frame, the error of a reused tile against its source is bounded by the tolerance however
 * long the run (a fade of one code per frame is recoded every max_abs + 1 frames, not never).  DESIGN.md section 18, on top of
 * section 16 (pc_clips.h: geometry, footprint, the exact test this one widens) and section 17 (pc_clip_rate.h: the device frame
 * table).  The product is the source table of an ordinary PCS1 container (clips.py).
 *
 * Kept apart from libpcodec.so and from the other image-side libraries (libpc_pixels.so, libpc_tiles.so, libpc_rate.so,
 * libpc_frames.so, libpc_frame_tiles.so, libpc_frame_rate.so, libpc_clips.so, libpc_clip_rate.so): nothing here is part of the
 * codec's numeric contract, byte strings or profiles, and no library of the image domain links another (the device code this one
 * shares with pc_clips.hip -- plane loads, word >> 6 for P010, the item, the halo block -- comes from the headers of image_csrc/,
 * DESIGN.md section 19).  Plain C, the conventions of pc_clip_rate.h: device pointers, int64 strides in
 * ELEMENTS, status codes PC_OK / PC_ERR_* (pcodec.h), `stream` is a hipStream_t passed as void* (NULL = default stream).  No call
 * allocates device memory or synchronises the host: the caller passes the workspace, and every launch is ordered on `stream`.  Every
 * argument is checked before the first HIP call; a call that returns PC_ERR_ARG has launched nothing.  All offsets are 64-bit.
 *
 * A frame (pc_ct_frame, a typedef of the one record pc_frame, pc_yuv_frame.h) is ONE picture of H x W luma samples with Hc x Wc
 * chroma samples, Hc = ceil(H/2), Wc = ceil(W/2), as strided planes; the batch strides are ignored.
 *   PC_CT_NV12  Y (r, q) at y[r*y_row + q];  Cb (i, j) at u[i*u_row + 2j], Cr one element after it;  v is ignored.  8-bit codes.
 *   PC_CT_I420  Y as above;  Cb at u[i*u_row + j], Cr at v[i*v_row + j].  8-bit codes.
 *   PC_CT_P010  the layout of NV12 in 16-bit words, code = word >> 6 (the low six bits are ignored).  10-bit codes.
 * y_row >= W, u_row >= 2*Wc (interleaved) or Wc, v_row >= Wc.  A pointer needs the alignment of its element only.  Every frame of a
 * clip has the same H, W and format; each may be pitched in its own way.
 *
 * Geometry and footprint are pc_clips.h's, word for word.  Tile size T, a multiple of 64, at most 2048; overlap O, a multiple of 4
 * with 0 <= O <= T/2; stride S = T - O; along an axis of length L there is 1 tile if L <= T, otherwise ceil((L - T) / S) + 1; tiles
 * are numbered row-major over the ny x nx grid.  With halo = 1 for PC_CT_LINEAR and 0 for PC_CT_NEAREST, along an axis of length L
 * with Lc = ceil(L / 2), tile i reads luma positions [i*S, e), e = min(i*S + T, L), and chroma positions
 * [max(i*S/2 - halo, 0), min(ceil(e/2) - 1 + halo, Lc - 1)]; the footprint of tile (i, j) is the product of the two axes' ranges,
 * once in the luma plane and once each in Cb and Cr.  nsamp[p] is the number of samples of the footprint in plane p.
 *
 * Difference of tile t between frames a and b, per plane p = 0, 1, 2 (Y, Cb, Cr), every footprint sample taken exactly once:
 *   count   the samples whose codes differ (pc_clips_tile_changes' number)
 *   sse     the sum of (code_a - code_b)^2            <= 2048^2 * 1023^2 < 2^43
 *   maxabs  the largest |code_a - code_b|
 * Tolerance: max_abs[3], each in [0, 2^bits - 1]; mse_q10[3], each in [0, 2^30], in units of 1/1024 code^2 (1023^2 * 1024 < 2^30:
 * the value 2^30 never binds and stands for "no condition"); max_run >= 0, 0 for "unlimited".  A tile is CLOSE to its anchor iff for
 * every plane maxabs[p] <= max_abs[p] and 1024 * sse[p] <= mse_q10[p] * nsamp[p] (integers, cross-multiplied: no division, no
 * float; both sides fit 64 bits).
 *
 * The scan.  anchor[t] = 0 and source[0][t] = 0; stats[0] is all zeros.  For k = 1 .. F - 1 in order and every tile t:
 * stats[k][t] is the difference of frames k and anchor[t]; the tile is REUSED iff it is close and (max_run == 0 or
 * k - anchor[t] + 1 <= max_run), and then source[k][t] = anchor[t]; otherwise source[k][t] = k and anchor[t] = k.  stats[k][t] holds
 * the evidence in both cases.
 */
#ifndef PC_CLIP_TOL_H
#define PC_CLIP_TOL_H

#include "pcodec.h"
#include "pc_yuv_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PC_CT_NV12 = PC_YUV_NV12, PC_CT_I420 = PC_YUV_I420, PC_CT_P010 = PC_YUV_P010 };
enum { PC_CT_NEAREST = PC_YUV_NEAREST, PC_CT_LINEAR = PC_YUV_LINEAR };
enum { PC_CT_NO_MSE = 1 << 30 };

typedef pc_frame pc_ct_frame;       /* pc_yuv_frame.h; y_batch, u_batch, v_batch: ignored (one picture per record) */

/* Bytes of device workspace pc_clip_tol_scan needs for a grid of n_tiles tiles: 72 bytes (nine 64-bit numbers: count, sse, maxabs
 * of three planes) per block, T*T/4096 + 1 blocks per tile -- a work item is one row pair of one tile by eight tile-aligned luma
 * columns with the four chroma sample pairs of its 2 x 2 cells, a block holds 256 of them, and one more block per tile takes the halo
 * ring -- then 4 bytes per tile for the anchors, the sum rounded up to a multiple of 8.  0 for arguments the scan would refuse (T no
 * multiple of 64 or above 2048, n_tiles < 1). */
PC_API size_t pc_clip_tol_workspace_size(int T, int n_tiles);

/* The scan above over a clip of n_frames frames, n = ny*nx tiles.
 *   frames_host   n_frames pc_ct_frame records in HOST memory, each a WHOLE H x W frame in `fmt`: read for the argument checks and
 *                 for the access path, never passed to the device.
 *   frames_dev    the same table in DEVICE memory (the caller uploads it once per clip), 8-byte aligned.
 *   upsample      PC_CT_LINEAR (halo 1) or PC_CT_NEAREST (halo 0): the upsampling the tiles are to be cut with.
 *   max_abs       HOST array of three ints, each in [0, 2^bits - 1] (bits = 8, or 10 for PC_CT_P010)
 *   mse_q10       HOST array of three ints, each in [0, 2^30]
 *   max_run       >= 0
 *   workspace     at least pc_clip_tol_workspace_size(T, ny*nx) bytes, 8-byte aligned; PC_ERR_ARG if smaller.  Its contents on
 *                 entry do not matter; nothing past that size is written.
 *   source        int32 [n_frames][n], 4-byte aligned; every element is written, row 0 included.
 *   stats         uint64 [n_frames][n][3][3], the last axis (count, sse, maxabs), 8-byte aligned; every element is written.
 * One launch writes row 0 and zeroes the anchors; then n_frames - 1 launch pairs, all on `stream`, whose order makes step k + 1 see
 * step k's anchors.  The host never reads device memory: the decision is taken on the device.  An anchor is only ever written by this
 * call's own kernels, but the host cannot see device memory, so the first kernel of a step still checks it against [0, k): anything
 * else is "recode, stats zero", and no frame is touched for that tile.  No atomics: thread, wave tree, the block's waves in order
 * (into the workspace), then one wave per tile over its block partials, which also decides.  Exact integers throughout: the result
 * does not depend on order or access path.  n_frames = 1 writes row 0 and launches nothing else. */
PC_API int pc_clip_tol_scan(const pc_ct_frame* frames_host, const pc_ct_frame* frames_dev, int n_frames, int fmt, int upsample, int H,
                            int W, int T, int O, const int* max_abs, const int* mse_q10, int max_run, void* workspace,
                            size_t workspace_bytes, int32_t* source, uint64_t* stats, void* stream);

/* Host only, launches nothing: *wide = 1 where pc_clip_tol_scan with this table and overlap moves four elements of a plane per access
 * (a 32-bit word of an 8-bit plane, a 64-bit word of a 16-bit plane), 0 where it moves them one by one.  Both give the same numbers.
 * The wide path needs EVERY frame of the table with every plane pointer aligned to four elements and every row stride a multiple of
 * 4, and O a multiple of 8 (the path is decided once per call: one unaligned frame makes the whole call narrow).  Items that straddle
 * an edge of the frame, and the halo ring, go element by element on either path.  The scan decides with the same code.  PC_ERR_ARG
 * for an unknown format, NULL pointers, n_frames < 1 or O < 0. */
PC_API int pc_clip_tol_plan(int fmt, const pc_ct_frame* frames_host, int n_frames, int O, int* wide);

PC_API const char* pc_clip_tol_strerror(int code);
PC_API int pc_clip_tol_last_hip_error(void);

#ifdef __cplusplus
}
#endif

#endif /* PC_CLIP_TOL_H */

/* pc_chroma_clip_tol.h -- C ABI of libpc_chroma_clip_tol.so: the TOLERANT scan of a clip of YUV frames of any of pc_chroma.h's twelve
 * formats (4:2:0 / 4:2:2 / 4:4:4, planar or semi-planar, 8-bit or 10-bit) and three chroma sitings on gfx950.  For every frame k >= 1
 * and every tile t it measures the tile's footprint in frame k against the frame the tile was LAST CODED in (its anchor) -- how many
 * codes differ, the sum of their squared differences, the largest absolute difference, per plane -- and decides, on the device,
 * whether the tile is close enough to be shown from its anchor's bytes once more.  DESIGN.md section 29: what pc_clip_tol.h (section
 * 18) is for NV12 / I420 / P010 with centre-sited chroma, on top of section 25 (pc_chroma_clips.h: geometry, footprint, the exact
 * test this one widens) and section 17 (the device frame table).  The product is the source table of an ordinary PCL1 container
 * (chroma_clips.py).
 *
 * Kept apart from libpcodec.so and from the other image-side libraries; no library of the image domain links another (the device
 * code this one shares -- plane loads, the code of an element, the format checks, the reduction -- comes from the headers of
 * image_csrc/).  Plain C, the conventions of pc_clip_tol.h and pc_chroma_clips.h: device pointers, int64 strides in ELEMENTS, status
 * codes PC_OK / PC_ERR_* (pcodec.h), `stream` is a hipStream_t passed as void* (NULL = default stream).  No call allocates device
 * memory or synchronises the host: the caller passes the workspace, and every launch is ordered on `stream`.  Every argument is
 * checked before the first HIP call; a call that returns PC_ERR_ARG has launched nothing.  All offsets are 64-bit.
 *
 * A format is pc_chroma.h's five integers:
 *   layout  PC_CCT_PLANAR      Cb (i, j) at u[i*u_row + j], Cr at v[i*v_row + j]
 *           PC_CCT_SEMIPLANAR  Cb at u[i*u_row + 2j], Cr one element after it; v is ignored
 *   bits    8 (elements are bytes) or 10 (elements are little-endian 16-bit words)
 *   shift   the bits below the code in an element: 0 for bits = 8; 0 or 6 for bits = 10
 *   sx, sy  luma samples per chroma sample along a row and along a column: (2, 2) 4:2:0, (2, 1) 4:2:2, (1, 1) 4:4:4
 * and a siting is two values, one per axis: PC_CCT_CENTRE or PC_CCT_COSITED (chroma sample j lies on luma sample 2j); an axis that
 * is not subsampled ignores its value.  A frame (pc_cct_frame, a typedef of the one record pc_frame, pc_yuv_frame.h) is ONE picture
 * of H x W luma samples with Hc x Wc chroma samples, Hc = ceil(H / sy), Wc = ceil(W / sx), as strided planes; the batch strides are
 * ignored.  y_row >= W, u_row >= 2*Wc (semi-planar) or Wc, v_row >= Wc.  A pointer needs the alignment of its element only.  Every
 * frame of a clip has the same H, W and format; each may be pitched in its own way.
 *
 * Geometry and footprint are pc_chroma_clips.h's.  Tile size T, a multiple of 64, at most 2048; overlap O, a multiple of 4 with
 * 0 <= O <= T/2; stride S = T - O; along an axis of length L there is 1 tile if L <= T, otherwise ceil((L - T) / S) + 1; tiles are
 * numbered row-major over the ny x nx grid.  Along an axis of length L, with e = min(i*S + T, L), tile i reads
 *   luma positions      [i*S, e)
 *   chroma positions    [i*S, e - 1]                                                  where the axis is not subsampled (sx or sy = 1),
 *                       whatever the siting and the upsampling, and otherwise, with Lc = ceil(L / 2),
 *                       [max(i*S/2 - lo, 0), min(ceil(e/2) - 1 + hi, Lc - 1)]
 *                       hi = 1 for PC_CCT_LINEAR, else 0;  lo = 1 for PC_CCT_LINEAR and PC_CCT_CENTRE on that axis, else 0.
 * The footprint of tile (i, j) is the product of the two axes' ranges, once in the luma plane and once each in Cb and Cr (the same
 * rectangle).  nsamp[p] is the number of samples of the footprint in plane p: it depends on the format, the siting and the
 * upsampling, so the siting moves the MSE decision below as well as the halo.
 *
 * Codes are (element >> shift) & (2^bits - 1): the other bits of a word are ignored, and two frames that differ in them alone have an
 * all-zero difference.
 *
 * Difference of tile t between frames a and b, per plane p = 0, 1, 2 (Y, Cb, Cr), every footprint sample taken exactly once:
 *   count   the samples whose codes differ (pc_chroma_clips_tile_changes' number)
 *   sse     the sum of (code_a - code_b)^2      with T <= 2048 a 4:4:4 chroma footprint has at most T^2 samples, as the luma one:
 *                                               sse <= 2048^2 * 1023^2 < 2^43
 *   maxabs  the largest |code_a - code_b|
 * Tolerance: max_abs[3], each in [0, 2^bits - 1] of the FORMAT; mse_q10[3], each in [0, 2^30], in units of 1/1024 code^2
 * (1023^2 * 1024 < 2^30: the value 2^30 never binds and stands for "no condition"); max_run >= 0, 0 for "unlimited".  A tile is CLOSE
 * to its anchor iff for every plane maxabs[p] <= max_abs[p] and 1024 * sse[p] <= mse_q10[p] * nsamp[p] (integers, cross-multiplied:
 * no division, no float; both sides fit 64 bits).
 *
 * The scan.  anchor[t] = 0 and source[0][t] = 0; stats[0] is all zeros.  For k = 1 .. F - 1 in order and every tile t:
 * stats[k][t] is the difference of frames k and anchor[t]; the tile is REUSED iff it is close and (max_run == 0 or
 * k - anchor[t] + 1 <= max_run), and then source[k][t] = anchor[t]; otherwise source[k][t] = k and anchor[t] = k.  stats[k][t] holds
 * the evidence in both cases.
 */
#ifndef PC_CHROMA_CLIP_TOL_H
#define PC_CHROMA_CLIP_TOL_H

#include "pcodec.h"
#include "pc_yuv_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PC_CCT_PLANAR = 0, PC_CCT_SEMIPLANAR = 1 };
enum { PC_CCT_NEAREST = PC_YUV_NEAREST, PC_CCT_LINEAR = PC_YUV_LINEAR };
enum { PC_CCT_CENTRE = 0, PC_CCT_COSITED = 1 };
enum { PC_CCT_NO_MSE = 1 << 30 };

typedef pc_frame pc_cct_frame;      /* pc_yuv_frame.h; y_batch, u_batch, v_batch: ignored (one picture per record) */

/* Bytes of device workspace pc_chroma_clip_tol_scan needs for a grid of n_tiles tiles: 72 bytes (nine 64-bit numbers: count, sse,
 * maxabs of three planes) per block, T*T/(2048*sy) + 1 blocks per tile -- a work item is sy luma rows of one tile by eight
 * tile-aligned luma columns with the 8 / sx chroma samples of its cells, a block holds 256 of them, and one more block per tile takes
 * the halo ring -- then 4 bytes per tile for the anchors, the sum rounded up to a multiple of 8.  0 for arguments the scan would
 * refuse (T no multiple of 64 or above 2048, sy neither 1 nor 2, n_tiles < 1, 2^31 blocks or more). */
PC_API size_t pc_chroma_clip_tol_workspace_size(int T, int sy, int n_tiles);

/* The scan above over a clip of n_frames frames, n = ny*nx tiles.
 *   frames_host   n_frames pc_cct_frame records in HOST memory, each a WHOLE H x W frame of the format: read for the argument checks
 *                 and for the access path, never passed to the device.
 *   frames_dev    the same table in DEVICE memory (the caller uploads it once per clip), 8-byte aligned.
 *   hsite, vsite, upsample   the siting and the upsampling the tiles are to be cut with: they choose the footprint's halo and nsamp.
 *   max_abs       HOST array of three ints, each in [0, 2^bits - 1]
 *   mse_q10       HOST array of three ints, each in [0, 2^30]
 *   max_run       >= 0
 *   workspace     at least pc_chroma_clip_tol_workspace_size(T, sy, ny*nx) bytes, 8-byte aligned; PC_ERR_ARG if smaller.  Its
 *                 contents on entry do not matter; nothing past that size is written.
 *   source        int32 [n_frames][n], 4-byte aligned; every element is written, row 0 included.
 *   stats         uint64 [n_frames][n][3][3], the last axis (count, sse, maxabs), 8-byte aligned; every element is written.
 * One launch writes row 0 and zeroes the anchors; then n_frames - 1 launch pairs, all on `stream`, whose order makes step k + 1 see
 * step k's anchors.  The host never reads device memory: the decision is taken on the device.  An anchor is only ever written by this
 * call's own kernels, but the host cannot see device memory, so the first kernel of a step still checks it against [0, k): anything
 * else is "recode, stats zero", and no frame is touched for that tile.  No atomics: thread, wave tree, the block's waves in order
 * (into the workspace), then one wave per tile over its block partials, which also decides.  Exact integers throughout: the result
 * does not depend on order or access path.  n_frames = 1 writes row 0 and launches nothing else.  PC_ERR_ARG also for n * 9 above
 * INT32_MAX and for everything pc_chroma_clips_tile_changes refuses in a format, a siting, an upsampling, a geometry or a frame. */
PC_API int pc_chroma_clip_tol_scan(const pc_cct_frame* frames_host, const pc_cct_frame* frames_dev, int n_frames, int layout, int bits,
                                   int shift, int sx, int sy, int hsite, int vsite, int upsample, int H, int W, int T, int O,
                                   const int* max_abs, const int* mse_q10, int max_run, void* workspace, size_t workspace_bytes,
                                   int32_t* source, uint64_t* stats, void* stream);

/* Host only, launches nothing: *wide = 1 where pc_chroma_clip_tol_scan with this table and overlap moves four elements of a plane per
 * access (a 32-bit word of an 8-bit plane, a 64-bit word of a 16-bit plane), 0 where it moves them one by one.  Both give the same
 * numbers.  The wide path needs, for EVERY frame of the table, what pc_chroma_clips_plan(PC_CHC_CHANGES, ...) needs for a pair: every
 * plane pointer aligned to four elements and every row stride a multiple of 4, and at sx == 2 O a multiple of 8 (at sx == 1 every O
 * qualifies).  The path is decided once per call: one unaligned frame makes the whole call narrow.  Items that straddle an edge of
 * the frame, and the halo ring, go element by element on either path.  This is the one function that decides: the scan calls it.
 * PC_ERR_ARG for an unknown layout, depth or sx, NULL pointers, n_frames < 1 or O < 0. */
PC_API int pc_chroma_clip_tol_plan(int layout, int bits, int sx, const pc_cct_frame* frames_host, int n_frames, int O, int* wide);

PC_API const char* pc_chroma_clip_tol_strerror(int code);
PC_API int pc_chroma_clip_tol_last_hip_error(void);

#ifdef __cplusplus
}
#endif

#endif /* PC_CHROMA_CLIP_TOL_H */

/* pc_clip_rate.h -- C ABI of libpc_clip_rate.so: the per-plane weighted squared error of decoded float32 RGB tiles against the frames
 * of a CLIP of YUV 4:2:0 frames (NV12 / I420 / P010), for a LIST of (frame, tile) jobs scattered over the clip, measured in the
 * frames' own code domain, on gfx950.  DESIGN.md section 17: section 15's measure (pc_frame_rate.h: a linear range of tiles of ONE
 * frame) for the work list of section 16 (pc_clips.h: the coded tiles of a clip, a few per frame).  It is what rate-controlled coding
 * of clips (clip_rate.py) allocates bytes by.
 *
 * Kept apart from libpcodec.so and from the other image-side libraries (libpc_pixels.so, libpc_tiles.so, libpc_rate.so,
 * libpc_frames.so, libpc_frame_tiles.so, libpc_frame_rate.so, libpc_clips.so): nothing here is part of the codec's numeric contract,
 * byte strings or profiles, and no library of the image domain links another (the device code this one shares with
 * pc_frame_rate.hip -- plane loads, levels, the emit arithmetic, band numerators, the item, the reduction -- comes from the headers of
 * image_csrc/).
 * Plain C, the conventions of pc_frame_rate.h: device pointers, int64 strides in ELEMENTS, status codes PC_OK / PC_ERR_* (pcodec.h),
 * `stream` is a hipStream_t passed as void* (NULL = default stream).  No call allocates device memory or synchronises the host: the
 * caller passes the workspace, and every launch is ordered on `stream`.  Every argument is checked before the first HIP call; a call
 * that returns PC_ERR_ARG has launched nothing.  All offsets are 64-bit.
 *
 * A frame (pc_cr_frame: like pc_frame_rate.h's pc_fr_frame a typedef of the one record pc_frame, pc_yuv_frame.h) is ONE picture
 * of H x W luma samples with Hc x Wc chroma samples, Hc = ceil(H/2), Wc = ceil(W/2), as strided planes; the batch strides are ignored.
 *   PC_CR_NV12  Y (r, q) at y[r*y_row + q];  Cb (i, j) at u[i*u_row + 2j], Cr one element after it;  v is ignored.  8-bit codes.
 *   PC_CR_I420  Y as above;  Cb at u[i*u_row + j], Cr at v[i*v_row + j].  8-bit codes.
 *   PC_CR_P010  the layout of NV12 in 16-bit words, code = word >> 6 (the low six bits are ignored).
 * y_row >= W, u_row >= 2*Wc (interleaved) or Wc, v_row >= Wc.  A pointer needs the alignment of its element only.  Every frame of a
 * clip has the same H, W and format; each may be pitched in its own way.
 *
 * Levels, geometry, the emit and the weights are pc_frame_rate.h's, word for word: levels (n = 8 or 10 bits, s = 2^(n-8))
 * PC_CR_LIMITED yo = 16s, ys = 219s, co = 128s, cs = 224s and PC_CR_FULL yo = 0, ys = 2^n-1, co = 128s, cs = 2^n-1; tile size T, a
 * multiple of 64, at most 2048 (8-bit formats) or 1024 (PC_CR_P010); overlap O, a multiple of 4 with 0 <= O <= T/2; stride S = T - O;
 * along an axis of length L there is 1 tile if L <= T, otherwise ceil((L - T) / S) + 1; tiles are numbered row-major over the ny x nx
 * grid.  Every float product and sum is one IEEE float32 operation (the library is built with -ffp-contract=off); everything that
 * is accumulated is an integer.
 */
#ifndef PC_CLIP_RATE_H
#define PC_CLIP_RATE_H

#include "pcodec.h"
#include "pc_yuv_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PC_CR_NV12 = PC_YUV_NV12, PC_CR_I420 = PC_YUV_I420, PC_CR_P010 = PC_YUV_P010 };
enum { PC_CR_LIMITED = PC_YUV_LIMITED, PC_CR_FULL = PC_YUV_FULL };

typedef pc_frame pc_cr_frame;       /* pc_yuv_frame.h; y_batch, u_batch, v_batch: ignored (one picture per record) */

/* Bytes of device workspace pc_clip_rate_sse_jobs needs: 24 bytes (three 64-bit sums) per block of 256 work items; a work item is
 * one row pair of one tile by eight tile-aligned columns, so a job has T*T/16 of them and T*T/4096 blocks.  0 for arguments the call
 * would refuse (T no multiple of 64 or above 2048, n_jobs < 1). */
PC_API size_t pc_clip_rate_workspace_size(int T, int n_jobs);

/* out[m][p], p = 0, 1, 2 for Y, Cb, Cr, of job m = (slot, tile) = (jobs[m][0], jobs[m][1]): bit for bit what
 * pc_frame_rate_tile_sse writes for first_tile = tile, n_tiles = 1 against the frame frames[slot], the float tile being the one at
 * x + m*sxt -- the same emit, the same weights ay * ax and cy * cx, exact unsigned 64-bit integers (< 2^60), the same limits.
 *   x             float32 tile set: element (m, c, r, q) at x[m*sxt + c*sxc + r*sxh + q]; sxh >= T; 4-byte aligned.
 *   frames_host   n_frames pc_cr_frame records in HOST memory, each a WHOLE H x W frame in `fmt`: read for the argument checks and
 *                 for the access path, never passed to the device.
 *   frames_dev    the same table in DEVICE memory (the caller uploads it once per clip), 8-byte aligned.
 *   jobs          DEVICE array int32 [n_jobs][2] of (frame slot, tile index row-major in the WHOLE grid), in any order, repeats
 *                 allowed, from any mix of frames; 4-byte aligned.  The host cannot check device memory, so the kernel does: a job
 *                 whose slot lies outside [0, n_frames) or whose tile lies outside [0, ny*nx) gives 0, 0, 0 and never an access
 *                 outside a frame or the table.
 *   workspace     at least pc_clip_rate_workspace_size(T, n_jobs) bytes, 8-byte aligned; PC_ERR_ARG if smaller.
 *   out           uint64 [n_jobs][3], 8-byte aligned; every element is written.
 * No atomics: thread, wave tree, the block's waves in order (into the workspace), then one wave per job over its block partials.
 * Two launches. */
PC_API int pc_clip_rate_sse_jobs(const float* x, int64_t sxt, int64_t sxc, int64_t sxh, int H, int W, int T, int O, int fmt, int range,
                                 float kr, float kg, float kb, float ib, float ir, const pc_cr_frame* frames_host,
                                 const pc_cr_frame* frames_dev, int n_frames, const int32_t* jobs, int n_jobs, void* workspace,
                                 size_t workspace_bytes, uint64_t* out, void* stream);

/* Host only, launches nothing: *wide = 1 where pc_clip_rate_sse_jobs with these arguments moves four floats per access (128 bits)
 * and four elements of a plane per access (a 32-bit word of an 8-bit plane, a 64-bit word of a 16-bit plane), 0 where it moves them
 * one by one.  Both give the same bits.  The wide path needs: the float pointer 16-byte aligned and its strides multiples of 4;
 * O a multiple of 8; and EVERY frame of the table with every plane pointer aligned to four elements and every row stride a
 * multiple of 4 (the path is decided once per call, not per job).  Items that straddle an edge of the frame go element by element
 * on either path.  The call decides with the same code.  PC_ERR_ARG for an unknown format, NULL pointers, n_frames < 1 or O < 0. */
PC_API int pc_clip_rate_plan(const void* x, int64_t sxt, int64_t sxc, int64_t sxh, int O, int fmt, const pc_cr_frame* frames_host,
                             int n_frames, int* wide);

PC_API const char* pc_clip_rate_strerror(int code);
PC_API int pc_clip_rate_last_hip_error(void);

#ifdef __cplusplus
}
#endif

#endif /* PC_CLIP_RATE_H */

/* pc_chroma_clip_tol_rate.h -- C ABI of libpc_chroma_clip_tol_rate.so: the per-plane weighted squared error of decoded float32 RGB
 * tiles against EVERY frame of the run each is shown in, for a clip of YUV frames in any of pc_chroma.h's twelve formats (4:2:0 /
 * 4:2:2 / 4:4:4, planar or semi-planar, 8-bit or 10-bit) and three chroma sitings, measured in the frames' own code domain, on gfx950.
 * section 28's measure (pc_chroma_clip_rate.h: one (frame, tile) job per decoded tile) for the tolerant source
 * table of section 29 (pc_chroma_clip_tol.h), where a coded tile is shown in frames it is only CLOSE to, so that its error differs
 * from frame to frame and has to be measured against each.  A job is one decoded tile and a list of frame slots (its entries); the
 * tile is read and emitted once -- colour matrix, rounding, clamps, the horizontal and vertical chroma filters with their co-sited
 * halo -- and its codes are compared against each of them.  It is what tolerant rate-controlled coding of clips of those frames
 * (chroma_clip_tol_rate.py) allocates bytes by; what pc_clip_tol_rate.h (section 20) is for NV12 / I420 / P010 with centre-sited
 * chroma, and bit for bit that there.
 *
 * Kept apart from libpcodec.so and from the other image-side libraries; no library of the image domain links another (what this one
 * shares with them comes from the headers of image_csrc/, DESIGN.md sections 19 and 27).  Plain C, the conventions of
 * pc_clip_tol_rate.h and pc_chroma_clip_rate.h: device pointers, int64 strides in ELEMENTS, status codes PC_OK / PC_ERR_* (pcodec.h),
 * `stream` is a hipStream_t passed as void* (NULL = default stream).  No call allocates device memory or synchronises the host: the
 * caller passes the workspace, and every launch is ordered on `stream`.  Every argument is checked before the first HIP call; a call
 * that returns PC_ERR_ARG has launched nothing.  All offsets are 64-bit.
 *
 * A format (layout, bits, shift, sx, sy), a siting (one value per axis), a frame (pc_cctr_frame: a typedef of the one record
 * pc_frame, pc_yuv_frame.h), the levels, the geometry (tile size T, a multiple of 64, at most 2048 at bits = 8 or 1024 at bits = 10;
 * overlap O, a multiple of 4 with 0 <= O <= T/2; the row-major ny x nx grid), the emit, the chroma filter with its clamps at the
 * tile's in-frame part and the integer band weights are pc_chroma_clip_rate.h's, word for word.  Every float product and sum is one
 * IEEE float32 operation (the library is built with -ffp-contract=off); everything that is accumulated is an integer.
 */
#ifndef PC_CHROMA_CLIP_TOL_RATE_H
#define PC_CHROMA_CLIP_TOL_RATE_H

#include "pcodec.h"
#include "pc_yuv_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PC_CCTR_PLANAR = 0, PC_CCTR_SEMIPLANAR = 1 };
enum { PC_CCTR_LIMITED = PC_YUV_LIMITED, PC_CCTR_FULL = PC_YUV_FULL };
enum { PC_CCTR_CENTRE = 0, PC_CCTR_COSITED = 1 };

typedef pc_frame pc_cctr_frame;     /* pc_yuv_frame.h; y_batch, u_batch, v_batch: ignored (one picture per record) */

/* Bytes of device workspace pc_chroma_clip_tol_rate_sse_runs needs: 24 bytes (three 64-bit sums) per wave and entry; a work item is
 * sy rows of one tile by eight tile-aligned columns, a job has T*T/(2048*sy) blocks of four waves, and every wave writes one partial
 * per entry of its job: 96 * (T*T/(2048*sy)) * n_entries.  0 for arguments the call would refuse (T no multiple of 64 or above 2048,
 * sy not 1 or 2, n_entries < 1, more than 2^31 - 1 blocks times entries). */
PC_API size_t pc_chroma_clip_tol_rate_workspace_size(int T, int sy, int n_entries);

/* out[e][p], p = 0, 1, 2 for Y, Cb, Cr, of entry e of job m (offsets[m] <= e < offsets[m + 1]): bit for bit what
 * pc_chroma_clip_rate_sse_jobs writes for the job (slots[e], tiles[m]) with the float tile at x + m*sxt -- the same emit, the same
 * clamps at the tile's in-frame part, the same weights ay * ax and cy * cx, exact unsigned 64-bit integers (< 2^60), the same limits.
 *   x             float32 tile set: element (m, c, r, q) at x[m*sxt + c*sxc + r*sxh + q]; sxh >= T; 4-byte aligned.
 *   frames_host   n_frames pc_cctr_frame records in HOST memory, each a WHOLE H x W frame in the format: read for the argument
 *                 checks and for the access path, never passed to the device.
 *   frames_dev    the same table in DEVICE memory (the caller uploads it once per clip), 8-byte aligned.
 *   tiles         DEVICE array int32 [n_jobs]: job m's tile index, row-major in the WHOLE grid; repeats allowed; 4-byte aligned.
 *   offsets_host  int32 [n_jobs + 1] in HOST memory: PC_ERR_ARG unless it starts at 0, is strictly increasing (every job has at
 *                 least one entry) and ends at n_entries.
 *   offsets_dev   the same bytes in DEVICE memory, 4-byte aligned.
 *   slots         DEVICE array int32 [n_entries]: the frame slot of each entry in the table, in any order, repeats allowed.
 *   workspace     at least pc_chroma_clip_tol_rate_workspace_size(T, sy, n_entries) bytes, 8-byte aligned; PC_ERR_ARG if smaller.
 *   out           uint64 [n_entries][3], 8-byte aligned; every element is written.
 * The host cannot check device memory, so the kernel does: an entry whose slot lies outside [0, n_frames) gives 0, 0, 0, and a job
 * whose tile lies outside [0, ny*nx) gives 0, 0, 0 for all its entries; neither reads a frame.  What the kernel reads from
 * offsets_dev it clamps to [0, n_entries]: whatever the device tables hold, nothing is accessed outside x's n_jobs tiles, the
 * frames of the table, the workspace and out.
 * No atomics and no LDS: thread, wave tree, one partial per wave and entry (into the workspace), then one wave per entry over its
 * partials.  Two launches. */
PC_API int pc_chroma_clip_tol_rate_sse_runs(const float* x, int64_t sxt, int64_t sxc, int64_t sxh, int H, int W, int T, int O, int layout,
                                            int bits, int shift, int sx, int sy, int hsite, int vsite, int range, float kr, float kg,
                                            float kb, float ib, float ir, const pc_cctr_frame* frames_host,
                                            const pc_cctr_frame* frames_dev, int n_frames, const int32_t* tiles,
                                            const int32_t* offsets_host, const int32_t* offsets_dev, const int32_t* slots, int n_jobs,
                                            int n_entries, void* workspace, size_t workspace_bytes, uint64_t* out, void* stream);

/* Host only, launches nothing: *wide = 1 where pc_chroma_clip_tol_rate_sse_runs with these arguments moves four floats per access
 * (128 bits) and four elements of a plane per access (a 32-bit word of an 8-bit plane, a 64-bit word of a 16-bit plane), 0 where it
 * moves them one by one.  Both give the same bits.  The rule is pc_chroma_clip_rate_plan's, for EVERY frame of the table (the path
 * is decided once per call, not per entry): the float pointer 16-byte aligned and its strides multiples of 4; every plane pointer of
 * every frame aligned to four elements and every row stride a multiple of 4; at sx == 2, O a multiple of 8; at sx == 1 every O
 * qualifies.  Items that straddle an edge of the frame go element by element on either path.  The call decides with the same code.
 * PC_ERR_ARG for an unknown layout, depth or sx, NULL pointers, n_frames < 1 or O < 0. */
PC_API int pc_chroma_clip_tol_rate_plan(const void* x, int64_t sxt, int64_t sxc, int64_t sxh, int O, int layout, int bits, int sx,
                                        const pc_cctr_frame* frames_host, int n_frames, int* wide);

PC_API const char* pc_chroma_clip_tol_rate_strerror(int code);
PC_API int pc_chroma_clip_tol_rate_last_hip_error(void);

#ifdef __cplusplus
}
#endif

#endif /* PC_CHROMA_CLIP_TOL_RATE_H */

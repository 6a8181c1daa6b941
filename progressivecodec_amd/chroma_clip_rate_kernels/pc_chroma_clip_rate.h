/* pc_chroma_clip_rate.h -- C ABI of libpc_chroma_clip_rate.so: the per-plane weighted squared error of decoded float32 RGB tiles
 * against the frames of a CLIP of YUV frames in any of pc_chroma.h's twelve formats (4:2:0 / 4:2:2 / 4:4:4, planar or semi-planar,
 * 8-bit or 10-bit) and three chroma sitings, for a LIST of (frame, tile) jobs scattered over the clip, measured in the frames' own
 * code domain, on gfx950.  DESIGN.md section 28: section 24's measure (pc_chroma_rate.h: a linear range of tiles of ONE frame) for
 * the work list of section 25 (pc_chroma_clips.h: the coded tiles of a clip, a few per frame).  It is what rate-controlled coding of
 * clips of those frames (chroma_clip_rate.py) allocates bytes by; what pc_clip_rate.h (section 17) is for NV12 / I420 / P010 with
 * centre-sited chroma, and bit for bit that there.
 *
 * Kept apart from libpcodec.so and from the other image-side libraries; no library of the image domain links another (what this one
 * shares with them comes from the headers of image_csrc/, DESIGN.md sections 19 and 27; the item is image_csrc/pc_chroma_sse_item.h).
 * Plain C, the conventions of pc_clip_rate.h and pc_chroma_rate.h: device pointers, int64 strides in ELEMENTS, status codes PC_OK /
 * PC_ERR_* (pcodec.h), `stream` is a hipStream_t passed as void* (NULL = default stream).  No call allocates device memory or
 * synchronises the host: the caller passes the workspace, and every launch is ordered on `stream`.  Every argument is checked before
 * the first HIP call; a call that returns PC_ERR_ARG has launched nothing.  All offsets are 64-bit.
 *
 * A format is pc_chroma.h's five integers:
 *   layout  PC_CCR_PLANAR      Cb (i, j) at u[i*u_row + j], Cr at v[i*v_row + j]
 *           PC_CCR_SEMIPLANAR  Cb at u[i*u_row + 2j], Cr one element after it; v is ignored
 *   bits    8 (elements are bytes) or 10 (elements are little-endian 16-bit words)
 *   shift   the bits below the code in an element: 0 for bits = 8; 0 or 6 for bits = 10.  code = (element >> shift) & (2^bits - 1)
 *   sx, sy  luma samples per chroma sample along a row and along a column: (2, 2) 4:2:0, (2, 1) 4:2:2, (1, 1) 4:4:4
 * and a siting is two values, one per axis: PC_CCR_CENTRE or PC_CCR_COSITED; an axis that is not subsampled ignores its value.  A
 * frame (pc_ccr_frame, a typedef of the one record pc_frame, pc_yuv_frame.h) is ONE picture of H x W luma samples with Hc x Wc chroma
 * samples, Hc = ceil(H / sy), Wc = ceil(W / sx), as strided planes; the batch strides are ignored.  y_row >= W, u_row >= 2*Wc
 * (semi-planar) or Wc, v_row >= Wc.  A pointer needs the alignment of its element only.  Every frame of a clip has the same H, W,
 * format and siting; each may be pitched in its own way.
 *
 * Levels, geometry, the emit, the chroma filter with its clamps at the tile's in-frame part and the integer band weights are
 * pc_chroma_rate.h's, word for word: tile size T, a multiple of 64, at most 2048 (bits = 8) or 1024 (bits = 10); overlap O, a
 * multiple of 4 with 0 <= O <= T/2; stride S = T - O; tiles are numbered row-major over the ny x nx grid.  Every float product and sum
 * is one IEEE float32 operation (the library is built with -ffp-contract=off); everything that is accumulated is an integer.
 *
 * The reuse identity.  Of the original frame a job reads luma [i*S, e) per axis and chroma (i*S/sy + k, j*S/sx + m), k < ceil(hh/sy),
 * m < ceil(ww/sx): on every axis, for every siting and upsampling, a subset of pc_chroma_clips.h's footprint of the tile.  A tile
 * that section 25 calls unchanged between two frames therefore has the same three sums against either.
 */
#ifndef PC_CHROMA_CLIP_RATE_H
#define PC_CHROMA_CLIP_RATE_H

#include "pcodec.h"
#include "pc_yuv_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PC_CCR_PLANAR = 0, PC_CCR_SEMIPLANAR = 1 };
enum { PC_CCR_LIMITED = PC_YUV_LIMITED, PC_CCR_FULL = PC_YUV_FULL };
enum { PC_CCR_CENTRE = 0, PC_CCR_COSITED = 1 };

typedef pc_frame pc_ccr_frame;      /* pc_yuv_frame.h; y_batch, u_batch, v_batch: ignored (one picture per record) */

/* Bytes of device workspace pc_chroma_clip_rate_sse_jobs needs: 24 bytes (three 64-bit sums) per block of 256 work items; a work
 * item is sy rows of one tile by eight tile-aligned columns, so a job has T*T/(8*sy) of them (a multiple of 256 for every admissible
 * T) and T*T/(2048*sy) blocks.  0 for arguments the call would refuse (T no multiple of 64 or above 2048, sy not 1 or 2, n_jobs < 1). */
PC_API size_t pc_chroma_clip_rate_workspace_size(int T, int sy, int n_jobs);

/* out[m][p], p = 0, 1, 2 for Y, Cb, Cr, of job m = (slot, tile) = (jobs[m][0], jobs[m][1]): bit for bit what
 * pc_chroma_rate_tile_sse writes for first_tile = tile, n_tiles = 1 against the frame frames[slot], the float tile being the one at
 * x + m*sxt -- the same emit, the same clamps at the tile's in-frame part, the same weights ay * ax and cy * cx, exact unsigned
 * 64-bit integers (< 2^60), the same limits.
 *   x             float32 tile set: element (m, c, r, q) at x[m*sxt + c*sxc + r*sxh + q]; sxh >= T; 4-byte aligned.
 *   frames_host   n_frames pc_ccr_frame records in HOST memory, each a WHOLE H x W frame in the format: read for the argument checks
 *                 and for the access path, never passed to the device.
 *   frames_dev    the same table in DEVICE memory (the caller uploads it once per clip), 8-byte aligned.
 *   jobs          DEVICE array int32 [n_jobs][2] of (frame slot, tile index row-major in the WHOLE grid), in any order, repeats
 *                 allowed, from any mix of frames; 4-byte aligned.  The host cannot check device memory, so the kernel does: a job
 *                 whose slot lies outside [0, n_frames) or whose tile lies outside [0, ny*nx) gives 0, 0, 0 and never an access
 *                 outside a frame or the table.
 *   workspace     at least pc_chroma_clip_rate_workspace_size(T, sy, n_jobs) bytes, 8-byte aligned; PC_ERR_ARG if smaller.
 *   out           uint64 [n_jobs][3], 8-byte aligned; every element is written.
 * No atomics: thread, wave tree, the block's waves in order (into the workspace), then one wave per job over its block partials.
 * Two launches. */
PC_API int pc_chroma_clip_rate_sse_jobs(const float* x, int64_t sxt, int64_t sxc, int64_t sxh, int H, int W, int T, int O, int layout,
                                        int bits, int shift, int sx, int sy, int hsite, int vsite, int range, float kr, float kg, float kb,
                                        float ib, float ir, const pc_ccr_frame* frames_host, const pc_ccr_frame* frames_dev, int n_frames,
                                        const int32_t* jobs, int n_jobs, void* workspace, size_t workspace_bytes, uint64_t* out,
                                        void* stream);

/* Host only, launches nothing: *wide = 1 where pc_chroma_clip_rate_sse_jobs with these arguments moves four floats per access (128
 * bits) and four elements of a plane per access (a 32-bit word of an 8-bit plane, a 64-bit word of a 16-bit plane), 0 where it moves
 * them one by one.  Both give the same bits.  The wide path needs pc_chroma_rate_plan's conditions for EVERY frame of the table (the
 * path is decided once per call, not per job): the float pointer 16-byte aligned and its strides multiples of 4; every plane pointer
 * of every frame aligned to four elements and every row stride a multiple of 4; at sx == 2, O a multiple of 8; at sx == 1 every O
 * qualifies.  Items that straddle an edge of the frame go element by element on either path.  The call decides with the same code.
 * PC_ERR_ARG for an unknown layout, depth or sx, NULL pointers, n_frames < 1 or O < 0. */
PC_API int pc_chroma_clip_rate_plan(const void* x, int64_t sxt, int64_t sxc, int64_t sxh, int O, int layout, int bits, int sx,
                                    const pc_ccr_frame* frames_host, int n_frames, int* wide);

PC_API const char* pc_chroma_clip_rate_strerror(int code);
PC_API int pc_chroma_clip_rate_last_hip_error(void);

#ifdef __cplusplus
}
#endif

#endif /* PC_CHROMA_CLIP_RATE_H */

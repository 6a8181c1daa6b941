/* pc_frame_rate.h -- C ABI of libpc_frame_rate.so: the per-tile, per-plane weighted squared error of decoded float32 RGB tiles against
 * the original YUV 4:2:0 frame (NV12 / I420 / P010), measured in the frame's own code domain (Y, Cb and Cr codes at the format's bit
 * depth, 4:2:0 chroma), on gfx950.  DESIGN.md section 15: the composition of section 13's emit (pc_frames.h), section 11's geometry
 * (pc_tiles.h) and section 12's integer band weights (pc_rate.h).  It is what rate-controlled tiled coding of frames
 * (frame_rate.py) allocates bytes by.
 *
 * Kept apart from libpcodec.so and from the other image-side libraries (libpc_pixels.so, libpc_tiles.so, libpc_rate.so,
 * libpc_frames.so, libpc_frame_tiles.so): nothing here is part of the codec's numeric contract, byte strings or profiles, and no
 * library of the image domain links another (the device code this one shares with pc_frame_tiles.hip and pc_rate.hip comes from the
 * headers of image_csrc/).  Plain C, the conventions of pc_frame_tiles.h: device pointers, int64 strides in
 * ELEMENTS, status codes PC_OK / PC_ERR_*
 * (pcodec.h), `stream` is a hipStream_t passed as void* (NULL = default stream).  No call allocates device memory or synchronises the
 * host: the caller passes the workspace, and every launch is ordered on `stream`.  Every argument is checked before the first HIP
 * call; a call that returns PC_ERR_ARG has launched nothing.  All offsets are 64-bit.
 *
 * A frame (pc_fr_frame, a typedef of the one record pc_frame, pc_yuv_frame.h) is ONE picture of H x W luma samples with Hc x Wc
 * chroma samples, Hc = ceil(H/2), Wc = ceil(W/2), as strided planes; the batch strides are ignored.
 *   PC_FR_NV12  Y (r, q) at y[r*y_row + q];  Cb (i, j) at u[i*u_row + 2j], Cr one element after it;  v is ignored.  8-bit codes.
 *   PC_FR_I420  Y as above;  Cb at u[i*u_row + j], Cr at v[i*v_row + j].  8-bit codes.
 *   PC_FR_P010  the layout of NV12 in 16-bit words, code = word >> 6 (the low six bits are ignored).
 * y_row >= W, u_row >= 2*Wc (interleaved) or Wc, v_row >= Wc.  A pointer needs the alignment of its element only.
 *
 * Levels (n = 8 or 10 bits, s = 2^(n-8)):   PC_FR_LIMITED  yo = 16s, ys = 219s, co = 128s, cs = 224s
 *                                           PC_FR_FULL     yo = 0,   ys = 2^n-1, co = 128s, cs = 2^n-1
 * The colour coefficients are plain float arguments, computed by the caller.  Every float product and sum below is one IEEE float32
 * operation (the library is built with -ffp-contract=off); everything that is accumulated is an integer.
 *
 * Geometry (pc_tiles.h).  Tile size T, a multiple of 64, at most 2048 (8-bit formats) or 1024 (PC_FR_P010); overlap O, a multiple
 * of 4 with 0 <= O <= T/2; stride S = T - O.  Along an axis of length L there is 1 tile if L <= T, otherwise ceil((L - T) / S) + 1.
 * Tiles are numbered row-major over the ny x nx grid; tile (i, j) covers rows [i*S, i*S + T) and columns [j*S, j*S + T) of the
 * frame, of which hh = min(T, H - i*S) rows and ww = min(T, W - j*S) columns lie inside it.
 */
#ifndef PC_FRAME_RATE_H
#define PC_FRAME_RATE_H

#include "pcodec.h"
#include "pc_yuv_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PC_FR_NV12 = PC_YUV_NV12, PC_FR_I420 = PC_YUV_I420, PC_FR_P010 = PC_YUV_P010 };
enum { PC_FR_LIMITED = PC_YUV_LIMITED, PC_FR_FULL = PC_YUV_FULL };

typedef pc_frame pc_fr_frame;       /* pc_yuv_frame.h; y_batch, u_batch, v_batch: ignored (one picture per record) */

/* Bytes of device workspace pc_frame_rate_tile_sse needs: 24 bytes (three 64-bit sums) per block of 256 work items; a work item is
 * one row pair of one tile by eight tile-aligned columns, so a tile has T*T/16 of them and T*T/4096 blocks.  0 for arguments the
 * call would refuse (T no multiple of 64 or above 2048, n_tiles < 1). */
PC_API size_t pc_frame_rate_workspace_size(int T, int n_tiles);

/* out[t][p], p = 0, 1, 2 for Y, Cb, Cr, of the tiles first_tile .. first_tile + n_tiles - 1 (a LINEAR range of the row-major grid,
 * tile first_tile + t at x + t*sxt).  A tile is judged by its own rendering, its in-frame part hh x ww being the picture:
 *   (R, G, B) = fminf(fmaxf(v, 0), 1) (NaN -> 0);  Y' = ((kr * R) + (kg * G)) + (kb * B);  Cb' = (B - Y') * ib;  Cr' = (R - Y') * ir;
 *   Ycode(r, q) = clampi(rintf((Y' * float(ys)) + float(yo)), 0, 2^n-1)                                     r < hh, q < ww
 *   Cbcode(k, m) = clampi(rintf(((u00 + u01) + (u10 + u11)) * 0.25f + float(co)), 0, 2^n-1), u = Cb' * float(cs) at rows 2k and
 *   min(2k+1, hh-1), columns 2m and min(2m+1, ww-1) (subscripts: row, column);  Cr likewise                 2k < hh, 2m < ww
 * and compared with the original's codes: luma at frame position (i*S + r, j*S + q), chroma at (i*S/2 + k, j*S/2 + m).
 * With ay(r), ax(q) the integer numerators of the band weights over den = 2*O (den = 1 for O = 0; pc_rate.h):
 *   2u + 1 where the tile is not the first along the axis and u < O; 2(O - 1 - (u - S)) + 1 where it is not the last and u >= S; den
 *   elsewhere; and cy(k) = (ay(2k) + ay(2k+1)) / 2, cx(m) likewise (integers: O and S are even):
 *   out[t][0] = sum ay(r) ax(q) e^2,   out[t][1], out[t][2] = sum cy(k) cx(m) e^2      in unsigned 64-bit integers, exact (< 2^60).
 *   x             float32 tile set: element (t, c, r, q) at x[t*sxt + c*sxc + r*sxh + q]; sxh >= T; 4-byte aligned.
 *   ref           the WHOLE original H x W frame in `fmt`.
 *   workspace     at least pc_frame_rate_workspace_size(T, n_tiles) bytes, 8-byte aligned; PC_ERR_ARG if smaller.
 *   out           uint64 [n_tiles][3], 8-byte aligned; every element is written.
 * No atomics: thread, wave tree, the block's waves in order (into the workspace), then one wave per tile over its block partials.
 * Two launches. */
PC_API int pc_frame_rate_tile_sse(const float* x, int64_t sxt, int64_t sxc, int64_t sxh, int H, int W, int T, int O, int first_tile,
                                  int n_tiles, int fmt, int range, float kr, float kg, float kb, float ib, float ir,
                                  const pc_fr_frame* ref, void* workspace, size_t workspace_bytes, uint64_t* out, void* stream);

/* Host only, launches nothing: *wide = 1 where pc_frame_rate_tile_sse with these arguments moves four floats per access (128 bits)
 * and four elements of a plane per access (a 32-bit word of an 8-bit plane, a 64-bit word of a 16-bit plane), 0 where it moves them
 * one by one.  Both give the same bits.  The wide path needs: the float pointer 16-byte aligned and its strides multiples of 4;
 * every plane pointer of ref aligned to four elements and every row stride a multiple of 4; O a multiple of 8 (S is then one, a
 * work item's first luma column a multiple of 8 in the frame and its first chroma column a multiple of 4).  Items that straddle an
 * edge of the frame go element by element on either path.  The call decides with the same code.  PC_ERR_ARG for an unknown format,
 * NULL pointers or O < 0. */
PC_API int pc_frame_rate_plan(const void* x, int64_t sxt, int64_t sxc, int64_t sxh, int O, int fmt, const pc_fr_frame* ref, int* wide);

PC_API const char* pc_frame_rate_strerror(int code);
PC_API int pc_frame_rate_last_hip_error(void);

#ifdef __cplusplus
}
#endif

#endif /* PC_FRAME_RATE_H */

/* pc_frames.h -- C ABI of libpc_frames.so: the YUV 4:2:0 front and back end of the codec on gfx950.  An NV12 / I420 / P010 frame in,
 * the float32 RGB planes the encoder takes out (pc_frames_ingest); the decoder's float32 planes in, a frame of the chosen format and
 * the per-plane distortion sums out (pc_frames_emit).  DESIGN.md section 13.
 *
 * Kept apart from libpcodec.so and from the other image-side libraries (libpc_pixels.so, libpc_tiles.so, libpc_rate.so): nothing here is
 * part of the codec's numeric contract, byte strings or profiles, and no library of the image domain links another.  Plain C, the
 * conventions of pc_pixels.h: device pointers, int64 strides, status codes PC_OK / PC_ERR_* (pcodec.h), `stream` is a hipStream_t
 * passed as void* (NULL = default stream).  No call allocates device memory or synchronises the host: the caller passes the
 * workspace, and every launch is ordered on `stream`.  Every argument is checked before the first HIP call; a call that returns
 * PC_ERR_ARG has launched nothing.  All offsets are 64-bit.
 *
 * A frame (pc_frame) is B pictures of H x W luma samples with Hc x Wc chroma samples, Hc = ceil(H/2), Wc = ceil(W/2), as strided
 * planes.  Strides are in ELEMENTS: bytes for the 8-bit formats, little-endian 16-bit words for PC_FRAMES_P010.
 *   PC_FRAMES_NV12  Y (b, r, q) at y[b*y_batch + r*y_row + q];  Cb (b, i, j) at u[b*u_batch + i*u_row + 2j], Cr one element after it;
 *                   v is ignored.  8-bit codes.
 *   PC_FRAMES_I420  Y as above;  Cb at u[b*u_batch + i*u_row + j], Cr at v[b*v_batch + i*v_row + j].  8-bit codes.
 *   PC_FRAMES_P010  the layout of NV12 in 16-bit words with the 10-bit code in the upper bits: code = word >> 6 on input (the low six
 *                   bits are ignored), word = code << 6 on output.
 * y_row >= W, u_row >= 2*Wc (interleaved) or Wc, v_row >= Wc; batch strides >= 1.  A pointer needs the alignment of its element only.
 * The planes of a destination must be nested rows-in-pictures (with B > 1, batch stride >= (rows - 1)*row stride + row length) and
 * must not overlap each other (the first is checked, the second is the caller's to keep).
 *
 * A float32 plane set is a pointer and batch, channel and row strides in ELEMENTS, unit stride along W.
 *
 * Levels (n = 8 or 10 bits, s = 2^(n-8)):   PC_FRAMES_LIMITED  yo = 16s, ys = 219s, co = 128s, cs = 224s
 *                                           PC_FRAMES_FULL     yo = 0,   ys = 2^n-1, co = 128s, cs = 2^n-1
 * The colour coefficients are plain float arguments, computed by the caller (float64 from Kr and Kb, rounded once): the library holds
 * no colour table.  Every product, sum and quotient below is one IEEE float32 operation (the library is built with -ffp-contract=off).
 */
#ifndef PC_FRAMES_H
#define PC_FRAMES_H

#include "pcodec.h"
#include "pc_yuv_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PC_FRAMES_NV12 = PC_YUV_NV12, PC_FRAMES_I420 = PC_YUV_I420, PC_FRAMES_P010 = PC_YUV_P010 };
enum { PC_FRAMES_LIMITED = PC_YUV_LIMITED, PC_FRAMES_FULL = PC_YUV_FULL };
enum { PC_FRAMES_NEAREST = PC_YUV_NEAREST, PC_FRAMES_LINEAR = PC_YUV_LINEAR };
enum { PC_FRAMES_INGEST = 0, PC_FRAMES_EMIT = 1 };

/* pc_frame: pc_yuv_frame.h, the record every YUV library shares; here all nine members are read */

/* dst[b][0..2][top + r][left + q] = (R, G, B) of luma pixel (r, q), and +0.0f everywhere else.  With C the Cb or Cr plane of codes:
 *   i0 = r >> 1, i1 = i0 + 1 if r is odd else i0 - 1, clamped to [0, Hc-1]; j0, j1 likewise from q;
 *   c16 = 9 C[i0,j0] + 3 C[i0,j1] + 3 C[i1,j0] + C[i1,j1]   (PC_FRAMES_LINEAR: centre-sited bilinear, edge clamp)
 *   c16 = 16 C[i0,j0]                                        (PC_FRAMES_NEAREST)                     -- integers, exact;
 *   y' = float(Y - yo) / float(ys);  cb' = float(c16_b - 16 co) / float(16 cs);  cr' likewise;
 *   R = y' + (cr' * a);  G = (y' - (cb' * b)) - (cr' * c);  B = y' + (cb' * d);  each then fminf(fmaxf(v, 0), 1).
 *   src           frame of B pictures of H x W.
 *   dst           contiguous float32 [B][3][Hp][Wp]; every element is written (no memset needed).  4-byte aligned.
 *   top, left     >= 0, top + H <= Hp, left + W <= Wp. */
PC_API int pc_frames_ingest(const pc_frame* src, int fmt, int range, int upsample, float a, float b, float c, float d, int B, int H,
                            int W, float* dst, int Hp, int Wp, int top, int left, void* stream);

/* Bytes of device workspace pc_frames_emit needs when it is given `ref` for B pictures of H x W (24 bytes, three 64-bit sums, per
 * block; a block is 256 consecutive work items of one picture, a work item two rows by eight luma columns); 0 for arguments the call
 * would refuse. */
PC_API size_t pc_frames_emit_workspace_size(int B, int H, int W);

/* For every luma pixel of the window (top, left, H, W) of x:  (R, G, B) = fminf(fmaxf(v, 0), 1) of the three planes (NaN -> 0);
 *   Y' = ((kr * R) + (kg * G)) + (kb * B);  Cb' = (B - Y') * ib;  Cr' = (R - Y') * ir;
 *   Ycode = clampi(rintf((Y' * float(ys)) + float(yo)), 0, 2^n-1);
 * and for chroma sample (i, j), with the luma rows 2i and min(2i+1, H-1) and columns 2j and min(2j+1, W-1) and u = Cb' * float(cs):
 *   code = clampi(rintf(((u00 + u01) + (u10 + u11)) * 0.25f + float(co)), 0, 2^n-1)   (subscripts: row, column); Cr likewise.
 *   x             float32, element (b, c, y, x) at x[b*sxb + c*sxc + y*sxh + x]; the planes are Hp x Wp (sxh >= Wp); 4-byte aligned.
 *   dst           frame in `fmt`; elements outside its H x W / Hc x Wc samples are not touched.  NULL with ref: the sums only.
 *   ref           optional frame in `fmt`.  With it (then workspace and sse are required):
 *     sse[b][p]   p = 0, 1, 2 for Y, Cb, Cr: the sum over the plane of (code - refcode)^2 in unsigned 64-bit integers, exact.  No
 *                 atomics: thread, wave tree, block (into the workspace), then one reduction launch per call.  Every element is
 *                 written.
 *   workspace     at least pc_frames_emit_workspace_size(B, H, W) bytes; PC_ERR_ARG if smaller.  Unused without ref.  workspace and
 *                 sse are 8-byte aligned. */
PC_API int pc_frames_emit(const float* x, int64_t sxb, int64_t sxc, int64_t sxh, int Hp, int Wp, int top, int left, int B, int H, int W,
                          int fmt, int range, float kr, float kg, float kb, float ib, float ir, const pc_frame* dst,
                          const pc_frame* ref, void* workspace, size_t workspace_bytes, uint64_t* sse, void* stream);

/* Host only, launches nothing: *wide = 1 where the ingest (op = PC_FRAMES_INGEST: frame is src, f32 is dst with strides 3*Hp*Wp,
 * Hp*Wp, Wp) or the emit (op = PC_FRAMES_EMIT: frame is dst, f32 is x) with these arguments moves four elements of a plane per access
 * (a 32-bit word of an 8-bit plane, a 64-bit word of a 16-bit plane) and four floats per access (128 bits), 0 where it moves them one
 * by one.  Both give the same bits, sums included.  A work item is eight consecutive columns -- of one padded row for the ingest, of
 * one row pair of the window for the emit -- so the wide path needs: the f32 pointer 16-byte aligned and its strides multiples of 4;
 * for the ingest Wp (fh) and left multiples of 8 (no partial last item; an item's first luma column is then a multiple of 8 in the
 * picture and its chroma column a multiple of 4), for the emit left a multiple of 4; every plane pointer of every frame aligned to
 * four elements and every plane stride a multiple of 4.  Items that straddle an edge of the picture go element by element on either
 * path.
 * `ref` may be NULL; for the emit `frame` may be NULL when `ref` is not (sums only).  The calls decide with the same code.
 * PC_ERR_ARG for an unknown op or format, NULL pointers or left < 0. */
PC_API int pc_frames_plan(int op, int fmt, const pc_frame* frame, const void* f32, int64_t fb, int64_t fc, int64_t fh, int left,
                          const pc_frame* ref, int* wide);

PC_API const char* pc_frames_strerror(int code);
PC_API int pc_frames_last_hip_error(void);

#ifdef __cplusplus
}
#endif

#endif /* PC_FRAMES_H */

/* pc_pixels.h -- C ABI of libpc_pixels.so: the image-domain front and back end of the codec on gfx950.  8-bit pixels in, the float32
 * planes the encoder takes out (pc_pixels_ingest_u8); the decoder's float32 planes in, 8-bit pixels and the distortion sums out
 * (pc_pixels_emit_u8).  DESIGN.md section 10.
 *
 * Kept apart from libpcodec.so: the codec's numeric contract, byte strings and profiles do not depend on anything here.
 * Plain C, the conventions of pc_metrics.h: device pointers, int64 strides, status codes PC_OK / PC_ERR_* (pcodec.h), `stream` is a
 * hipStream_t passed as void* (NULL = default stream).  No call allocates device memory or synchronises the host: the caller passes
 * the workspace, and every launch is ordered on `stream`.  Every argument is checked before the first HIP call; a call that returns
 * PC_ERR_ARG has launched nothing.
 *
 * An 8-bit image ("u8 view") is a pointer, a layout and three strides in BYTES:
 *   PC_PIXELS_HWC  [B,H,W,3] interleaved: byte (b, y, x, c) at p[b*s_batch + y*s_row + 3*x + c]; s_plane is ignored.
 *   PC_PIXELS_CHW  [B,3,H,W] planar:      byte (b, c, y, x) at p[b*s_batch + c*s_plane + y*s_row + x].
 * s_row >= the bytes of a row (3*W or W), s_batch >= 1, s_plane >= 1 (planar).  The pointer needs no alignment.  A destination view
 * must be nested rows-in-planes-in-images, so that no byte is written twice (checked; other non-overlapping orders, such as
 * [B,H,3,W] memory, are refused): with span = (H-1)*s_row + the bytes of a row, interleaved s_batch >= span (B > 1); planar
 * s_plane >= span and s_batch >= 2*s_plane + span (B > 1).
 *
 * A float32 plane set is a pointer and batch, channel and row strides in ELEMENTS, unit stride along W.
 */
#ifndef PC_PIXELS_H
#define PC_PIXELS_H

#include "pcodec.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PC_PIXELS_HWC = 0, PC_PIXELS_CHW = 1 };
enum { PC_PIXELS_NEAREST = 0, PC_PIXELS_TRUNC = 1 };
enum { PC_PIXELS_INGEST = 0, PC_PIXELS_EMIT = 1 };

/* dst[b][c][top + y][left + x] = (float)src(b, y, x, c) / 255.0f, the correctly rounded float32 quotient (bitwise torch's
 * u8.float().div(255) and ToTensor; the values come from a 256-entry table of host-computed quotients), and +0.0f everywhere else.
 *   src           u8 view of B images of H x W pixels.
 *   dst           contiguous float32 [B][3][Hp][Wp]; every element is written (no memset needed).  4-byte aligned.
 *   top, left     >= 0, top + H <= Hp, left + W <= Wp. */
PC_API int pc_pixels_ingest_u8(const uint8_t* src, int layout, int64_t s_batch, int64_t s_plane, int64_t s_row, int B, int H, int W,
                               float* dst, int Hp, int Wp, int top, int left, void* stream);

/* Bytes of device workspace pc_pixels_emit_u8 needs when it is given `ref` for B images of H x W pixels (the per-block partial sums:
 * 48 bytes per block; a block is 1024 consecutive four-column groups of one image's rows); 0 for arguments the call would refuse. */
PC_API size_t pc_pixels_emit_workspace_size(int B, int H, int W);

/* For the window (top, left, H, W) of every plane of x: c = fminf(fmaxf(v, 0), 1) (NaN -> 0), q = rintf(c * 255.0f)
 * (PC_PIXELS_NEAREST, half to even) or truncf(c * 255.0f) (PC_PIXELS_TRUNC: mul(255).byte() of a clamped tensor), stored to dst.
 *   x             float32, element (b, c, y, x) of the plane at x[b*sxb + c*sxc + y*sxh + x]; the planes are Hp x Wp (sxh >= Wp);
 *                 4-byte aligned.
 *   dst           u8 view; bytes outside the H x W window of the view are not touched.  NULL with ref: the sums only, no image.
 *   ref           optional u8 view of the original image.  With it (and then workspace, sse_u8 and sse_f are required):
 *     sse_u8[b][c]  sum over the window of (q - ref)^2, in integers (exact).
 *     sse_f[b][c]   sum over the window of (x_ref - c)^2 with x_ref = ref / 255.0f as pc_pixels_ingest_u8 gives it: the difference in
 *                   float32, its square in float64 (exact), accumulated in float64 in a fixed order (per thread, per block into the
 *                   workspace, then one ordered reduction per image).  No atomics: per image the sums depend on that image's pixels
 *                   only and are bitwise the same alone, inside any batch, from run to run and on either access path.
 *   workspace     at least pc_pixels_emit_workspace_size(B, H, W) bytes; PC_ERR_ARG if smaller.  Unused without ref.
 *                 workspace, sse_u8 and sse_f are 8-byte aligned.
 */
PC_API int pc_pixels_emit_u8(const float* x, int64_t sxb, int64_t sxc, int64_t sxh, int Hp, int Wp, int top, int left, int B, int H,
                             int W, int rounding, uint8_t* dst, int dst_layout, int64_t d_batch, int64_t d_plane, int64_t d_row,
                             const uint8_t* ref, int ref_layout, int64_t r_batch, int64_t r_plane, int64_t r_row, void* workspace,
                             size_t workspace_bytes, uint64_t* sse_u8, double* sse_f, void* stream);

/* Host only, launches nothing: *wide = 1 where the ingest (op = PC_PIXELS_INGEST: u8 is src, f32 is dst with strides 3*Hp*Wp, Hp*Wp,
 * Wp) or the emit (op = PC_PIXELS_EMIT: u8 is dst, f32 is x) with these arguments moves four pixels per access (a 32-bit word of
 * bytes, a 128-bit word of floats), 0 where it moves them byte by byte and float by float.  Both give the same bits, sums included.
 * A work item is four consecutive columns of one row -- of the padded row for the ingest, of the window for the emit -- so the wide
 * path needs: the f32 pointer 16-byte aligned and its strides multiples of 4 (emit: left too); every u8 view's strides multiples of 4
 * (s_plane: planar only) and its pointer 4-byte aligned (ingest: the address of padded column 0, src - 3*left or src - left).
 * `ref` may be NULL; for the emit `u8` may be NULL when `ref` is not (sums only).  The calls decide with the same code.  PC_ERR_ARG for an unknown op or layout, NULL pointers or B, H, W < 1. */
PC_API int pc_pixels_plan(int op, const void* u8, int layout, int64_t s_batch, int64_t s_plane, int64_t s_row, const void* f32,
                          int64_t fb, int64_t fc, int64_t fh, int top, int left, int B, int H, int W, const void* ref, int ref_layout,
                          int64_t r_batch, int64_t r_plane, int64_t r_row, int* wide);

PC_API const char* pc_pixels_strerror(int code);
PC_API int pc_pixels_last_hip_error(void);

#ifdef __cplusplus
}
#endif

#endif /* PC_PIXELS_H */

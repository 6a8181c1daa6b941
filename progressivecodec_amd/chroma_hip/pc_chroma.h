/* pc_chroma.h -- C ABI of libpc_chroma.so: YUV frames of any of three chroma subsamplings (4:2:0, 4:2:2, 4:4:4), two layouts, two
 * depths and three chroma sitings in, the float32 RGB planes the encoder takes out (pc_chroma_ingest); the decoder's float32 planes
 * in, a frame of the chosen format and siting and the per-plane distortion sums out (pc_chroma_emit).  DESIGN.md section 21; for
 * 4:2:0 with centre siting both calls compute what pc_frames.h's compute, bit for bit.
 *
 * Kept apart from libpcodec.so and from the other image-side libraries; no library of the image domain links another.  Plain C, the
 * conventions of pc_frames.h: device pointers, int64 strides, status codes PC_OK / PC_ERR_* (pcodec.h), `stream` is a hipStream_t
 * passed as void* (NULL = default stream).  No call allocates device memory or synchronises the host: the caller passes the
 * workspace, and every launch is ordered on `stream`.  Every argument is checked before the first HIP call; a call that returns
 * PC_ERR_ARG has launched nothing.  All offsets are 64-bit.
 *
 * A format is five integers:
 *   layout  PC_CH_PLANAR      Cb (b, i, j) at u[b*u_batch + i*u_row + j], Cr at v[b*v_batch + i*v_row + j]
 *           PC_CH_SEMIPLANAR  Cb at u[b*u_batch + i*u_row + 2j], Cr one element after it; v is ignored
 *   bits    8 (elements are bytes) or 10 (elements are little-endian 16-bit words)
 *   shift   the bits below the code in an element: 0 for bits = 8; 0 or 6 for bits = 10.  code = (element >> shift) & (2^bits - 1)
 *           on input (the other bits of a word are ignored), element = code << shift on output
 *   sx, sy  luma samples per chroma sample along a row and along a column: (2, 2) 4:2:0, (2, 1) 4:2:2, (1, 1) 4:4:4
 * so that i420 / i422 / i444 are (PLANAR, 8, 0), nv12 / nv16 / nv24 (SEMIPLANAR, 8, 0), p010 / p210 / p410 (SEMIPLANAR, 10, 6) and
 * yuv420p10 / yuv422p10 / yuv444p10 (PLANAR, 10, 0).  A frame (pc_ch_frame) is B pictures of H x W luma samples (Y (b, r, q) at
 * y[b*y_batch + r*y_row + q]) with Hc x Wc chroma samples, Hc = ceil(H / sy), Wc = ceil(W / sx), as strided planes; strides in
 * ELEMENTS.  y_row >= W, u_row >= 2*Wc (semi-planar) or Wc, v_row >= Wc; batch strides >= 1.  A pointer needs the alignment of its
 * element only.  The planes of a destination must be nested rows-in-pictures (with B > 1, batch stride >= (rows - 1)*row stride + row
 * length) and must not overlap each other (the first is checked, the second is the caller's to keep).
 *
 * Siting is two values, one per axis: PC_CH_CENTRE (the chroma sample lies in the middle of its sx or sy luma samples) or
 * PC_CH_COSITED (chroma sample j lies on luma sample 2j).  An axis that is not subsampled ignores its value.
 *
 * A float32 plane set is a pointer and batch, channel and row strides in ELEMENTS, unit stride along W.
 * Levels (n = bits, s = 2^(n-8)):   PC_CH_LIMITED  yo = 16s, ys = 219s, co = 128s, cs = 224s
 *                                   PC_CH_FULL     yo = 0,   ys = 2^n-1, co = 128s, cs = 2^n-1
 * The colour coefficients are plain float arguments, computed by the caller (float64 from Kr and Kb, rounded once): the library holds
 * no colour table.  Every product, sum and quotient below is one IEEE float32 operation (the library is built with -ffp-contract=off).
 */
#ifndef PC_CHROMA_H
#define PC_CHROMA_H

#include "pcodec.h"
#include "pc_yuv_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PC_CH_PLANAR = 0, PC_CH_SEMIPLANAR = 1 };
enum { PC_CH_LIMITED = PC_YUV_LIMITED, PC_CH_FULL = PC_YUV_FULL };
enum { PC_CH_NEAREST = PC_YUV_NEAREST, PC_CH_LINEAR = PC_YUV_LINEAR };
enum { PC_CH_CENTRE = 0, PC_CH_COSITED = 1 };
enum { PC_CH_INGEST = 0, PC_CH_EMIT = 1 };

typedef pc_frame pc_ch_frame;   /* pc_yuv_frame.h, the record every YUV library shares; here all nine members are read */

/* dst[b][0..2][top + r][left + q] = (R, G, B) of luma pixel (r, q), and +0.0f everywhere else.  Per axis, luma index r against n
 * chroma samples gives two taps (i0, w0), (i1, w1), w0 + w1 = 4:
 *   axis not subsampled                i0 = r,      (4, 0)
 *   subsampled, PC_CH_NEAREST          i0 = r >> 1, (4, 0), for either siting
 *   subsampled, linear, PC_CH_CENTRE   i0 = r >> 1; i1 = i0 + 1 if r is odd else i0 - 1, clamped to [0, n-1]; (3, 1)
 *   subsampled, linear, PC_CH_COSITED  i0 = r >> 1; r even: (4, 0); r odd: i1 = min(i0 + 1, n-1), (2, 2)
 * With C the Cb or Cr plane of codes:  c16 = sum over a, b of wy_a * wx_b * C[i_a, j_b]   -- integers, exact;
 *   y' = float(Y - yo) / float(ys);  cb' = float(c16_b - 16 co) / float(16 cs);  cr' likewise;
 *   R = y' + (cr' * a);  G = (y' - (cb' * b)) - (cr' * c);  B = y' + (cb' * d);  each then fminf(fmaxf(v, 0), 1).
 *   src           frame of B pictures of H x W.
 *   dst           contiguous float32 [B][3][Hp][Wp]; every element is written (no memset needed).  4-byte aligned.
 *   top, left     >= 0, top + H <= Hp, left + W <= Wp. */
PC_API int pc_chroma_ingest(const pc_ch_frame* src, int layout, int bits, int shift, int sx, int sy, int hsite, int vsite, int range,
                            int upsample, float a, float b, float c, float d, int B, int H, int W, float* dst, int Hp, int Wp, int top,
                            int left, void* stream);

/* Bytes of device workspace pc_chroma_emit needs when it is given `ref` for B pictures of H x W (24 bytes, three 64-bit sums, per
 * block; a block is 256 consecutive work items of one picture, a work item sy rows by eight luma columns); 0 for arguments the call
 * would refuse. */
PC_API size_t pc_chroma_emit_workspace_size(int B, int H, int W, int sy);

/* For every luma pixel of the window (top, left, H, W) of x:  (R, G, B) = fminf(fmaxf(v, 0), 1) of the three planes (NaN -> 0);
 *   Y' = ((kr * R) + (kg * G)) + (kb * B);  Cb' = (B - Y') * ib;  Cr' = (R - Y') * ir;
 *   Ycode = clampi(rintf((Y' * float(ys)) + float(yo)), 0, 2^n-1);  u = Cb' * float(cs)  (Cr likewise).
 * A chroma sample filters the u values along rows first, then along columns, by one rule per axis for chroma index j against N
 * luma samples p[0 .. N-1]:
 *   axis not subsampled   h = p[j],                                                                  scale 1
 *   PC_CH_CENTRE          h = p[2j] + p[min(2j+1, N-1)],                                              scale 2
 *   PC_CH_COSITED         a = p[max(2j-1, 0)], b = p[2j], c = p[min(2j+1, N-1)]; h = (a + c) + (b + b),  scale 4
 * (horizontally on every luma row the vertical rule needs, then the same rule on the h values), and
 *   code = clampi(rintf(v * s + float(co)), 0, 2^n-1),  s = 1 / (scale_h * scale_v), a power of two.
 *   x             float32, element (b, c, y, x) at x[b*sxb + c*sxc + y*sxh + x]; the planes are Hp x Wp (sxh >= Wp); 4-byte aligned.
 *   dst           frame; elements outside its H x W / Hc x Wc samples are not touched.  NULL with ref: the sums only.
 *   ref           optional frame of the same format.  With it (then workspace and sse are required):
 *     sse[b][p]   p = 0, 1, 2 for Y, Cb, Cr: the sum over the plane of (code - refcode)^2 in unsigned 64-bit integers, exact.  No
 *                 atomics: thread, wave tree, block (into the workspace), then one reduction launch per call.  Every element is
 *                 written.
 *   workspace     at least pc_chroma_emit_workspace_size(B, H, W, sy) bytes; PC_ERR_ARG if smaller.  Unused without ref.  workspace
 *                 and sse are 8-byte aligned. */
PC_API int pc_chroma_emit(const float* x, int64_t sxb, int64_t sxc, int64_t sxh, int Hp, int Wp, int top, int left, int B, int H, int W,
                          int layout, int bits, int shift, int sx, int sy, int hsite, int vsite, int range, float kr, float kg,
                          float kb, float ib, float ir, const pc_ch_frame* dst, const pc_ch_frame* ref, void* workspace,
                          size_t workspace_bytes, uint64_t* sse, void* stream);

/* Host only, launches nothing: *wide = 1 where the ingest (op = PC_CH_INGEST: frame is src, f32 is dst with strides 3*Hp*Wp, Hp*Wp,
 * Wp) or the emit (op = PC_CH_EMIT: frame is dst, f32 is x) with these arguments moves four elements of a plane per access (a 32-bit
 * word of an 8-bit plane, a 64-bit word of a 16-bit plane) and four floats per access (128 bits), 0 where it moves them one by one.
 * Both give the same bits, sums included.  A work item is eight consecutive luma columns -- of one padded row for the ingest, of sy
 * rows of the window for the emit -- so the wide path needs: the f32 pointer 16-byte aligned and its strides multiples of 4; for the
 * ingest Wp (fh) and left multiples of 8, for the emit left a multiple of 4; every plane pointer of every frame aligned to four
 * elements and every plane stride a multiple of 4.  Neither the subsampling nor the siting enters: an item's first chroma element is
 * a multiple of four elements in every format.  Items that straddle an edge of the picture go element by element on either path.
 * `ref` may be NULL; for the emit `frame` may be NULL when `ref` is not (sums only).  The calls decide with the same code.
 * PC_ERR_ARG for an unknown op, layout or depth, NULL pointers or left < 0. */
PC_API int pc_chroma_plan(int op, int layout, int bits, const pc_ch_frame* frame, const void* f32, int64_t fb, int64_t fc, int64_t fh,
                          int left, const pc_ch_frame* ref, int* wide);

PC_API const char* pc_chroma_strerror(int code);
PC_API int pc_chroma_last_hip_error(void);

#ifdef __cplusplus
}
#endif

#endif /* PC_CHROMA_H */

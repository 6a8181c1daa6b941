/* pc_yuv_frame.h -- the one YUV 4:2:0 frame record and the one set of format, range and upsampling values of the image-side
 * libraries (libpc_frames.so, libpc_frame_tiles.so, libpc_frame_rate.so, libpc_clips.so, libpc_clip_rate.so, libpc_clip_tol.so).
 * Plain C.  Each library's public header includes this one and keeps its own names (pc_ft_frame, PC_FT_NV12, ...) as typedefs and
 * enumerators of these: one record, one set of values, no ABI name changed.  The header lives beside the libraries' sources and not
 * under include/: the codec's source hash (bench.source_hash) covers the headers of include/, and nothing of the image side is part of it.
 *
 * A frame is strided planes of luma (y) and chroma (u, v) samples with strides in ELEMENTS: bytes for the 8-bit formats,
 * little-endian 16-bit words for P010.  What the batch strides mean, and whether they are read at all, is each library's to say.
 *   NV12  Cb at u[.. + 2j], Cr one element after it; v is ignored.  8-bit codes.
 *   I420  Cb in u, Cr in v.  8-bit codes.
 *   P010  the layout of NV12 in 16-bit words, code = word >> 6. */
#ifndef PC_YUV_FRAME_H
#define PC_YUV_FRAME_H

#include <stdint.h>

enum { PC_YUV_NV12 = 0, PC_YUV_I420 = 1, PC_YUV_P010 = 2 };
enum { PC_YUV_LIMITED = 0, PC_YUV_FULL = 1 };
enum { PC_YUV_NEAREST = 0, PC_YUV_LINEAR = 1 };

typedef struct pc_frame {
    void* y;
    int64_t y_batch, y_row;
    void* u;                    /* NV12 / P010: the interleaved CbCr plane */
    int64_t u_batch, u_row;
    void* v;                    /* I420 only */
    int64_t v_batch, v_row;
} pc_frame;

#endif /* PC_YUV_FRAME_H */

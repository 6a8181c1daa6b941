// pc_yuv_device.h -- what the YUV 4:2:0 libraries (frames, frame_tiles, frame_rate, clips, clip_rate, clip_tol) share on the device
// and in their argument checks: typed planes, the four-element loads and stores, the levels, the colour arithmetic of the ingest
// (to_rgb) and of the emit (emit_px, emit_chroma), and the host checks of a single-picture frame.  Every float
// operation is written out and parenthesised as the contracts state it; the libraries are built with -ffp-contract=off.  Include after
// pc_image_host.h.
#ifndef PC_YUV_DEVICE_H
#define PC_YUV_DEVICE_H

#include "pc_yuv_frame.h"

namespace {

constexpr int COLS = 8;                  // luma columns per work item

template <class T>
struct Planes {                          // one picture of a pc_frame with typed pointers; row strides in elements
    T* y;
    int64_t yr;
    T* u;
    int64_t ur;
    T* v;
    int64_t vr;
};

template <class T>
__host__ __device__ __forceinline__ Planes<T> planes_of(const pc_frame* f)
{
    return Planes<T>{static_cast<T*>(f->y), f->y_row, static_cast<T*>(f->u), f->u_row, static_cast<T*>(f->v), f->v_row};
}

struct Levels {
    int yo, ys, co, cs, maxv;
};

struct IngestCoef {
    float a, b, c, d;
};

struct EmitCoef {
    float kr, kg, kb, ib, ir;
};

// four consecutive elements of a plane in one access: a 32-bit word of bytes, a 64-bit word of 16-bit words
__device__ __forceinline__ void load4(const uint8_t* p, unsigned v[4])
{
    const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
    v[0] = w & 255u; v[1] = (w >> 8) & 255u; v[2] = (w >> 16) & 255u; v[3] = w >> 24;
}

__device__ __forceinline__ void load4(const uint16_t* p, unsigned v[4])
{
    const uint2 w = *reinterpret_cast<const uint2*>(p);
    v[0] = w.x & 0xffffu; v[1] = w.x >> 16; v[2] = w.y & 0xffffu; v[3] = w.y >> 16;
}

__device__ __forceinline__ void store4(uint8_t* p, const unsigned v[4])
{
    *reinterpret_cast<uint32_t*>(p) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
}

__device__ __forceinline__ void store4(uint16_t* p, const unsigned v[4])
{
    *reinterpret_cast<uint2*>(p) = make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// One luma pixel of the ingest: its code and the two 16-fold chroma sums -> R, G, B.
__device__ __forceinline__ void to_rgb(int Y, int cb16, int cr16, const Levels& lv, const IngestCoef& k, float& R, float& G, float& B)
{
    const float y = (float)(Y - lv.yo) / (float)lv.ys;
    const float cb = (float)(cb16 - 16 * lv.co) / (float)(16 * lv.cs);
    const float cr = (float)(cr16 - 16 * lv.co) / (float)(16 * lv.cs);
    R = clamp01(y + cr * k.a);
    G = clamp01((y - cb * k.b) - cr * k.c);
    B = clamp01(y + cb * k.d);
}

// One luma pixel of the emit: the three floats -> its luma code and its scaled chroma differences Cb' * cs, Cr' * cs.
__device__ __forceinline__ void emit_px(float r, float g, float b, const Levels& lv, const EmitCoef& k, unsigned& yq, float& ub, float& ur)
{
    const float R = clamp01(r), Gc = clamp01(g), Bc = clamp01(b);
    const float Yf = (k.kr * R + k.kg * Gc) + k.kb * Bc;
    const float Cb = (Bc - Yf) * k.ib, Cr = (R - Yf) * k.ir;
    yq = (unsigned)clampi((int)rintf(Yf * (float)lv.ys + (float)lv.yo), 0, lv.maxv);
    ub = Cb * (float)lv.cs;
    ur = Cr * (float)lv.cs;
}

// One chroma sample of the emit: the code of the mean of a 2 x 2 cell's scaled differences (subscripts: row, column).
__device__ __forceinline__ int emit_chroma(float u00, float u01, float u10, float u11, const Levels& lv)
{
    return clampi((int)rintf(((u00 + u01) + (u10 + u11)) * 0.25f + (float)lv.co), 0, lv.maxv);
}

// -- host ----------------------------------------------------------------------------------------------------------------------------

bool fmt_ok(int fmt) { return fmt == PC_YUV_NV12 || fmt == PC_YUV_I420 || fmt == PC_YUV_P010; }
bool interleaved(int fmt) { return fmt != PC_YUV_I420; }
int elem_bytes(int fmt) { return fmt == PC_YUV_P010 ? 2 : 1; }
bool upsample_ok(int u) { return u == PC_YUV_NEAREST || u == PC_YUV_LINEAR; }

bool levels_of(int fmt, int range, Levels& lv)
{
    const int n = fmt == PC_YUV_P010 ? 10 : 8, s = 1 << (n - 8), maxv = (1 << n) - 1;
    if (range == PC_YUV_LIMITED) lv = Levels{16 * s, 219 * s, 128 * s, 224 * s, maxv};
    else if (range == PC_YUV_FULL) lv = Levels{0, maxv, 128 * s, maxv, maxv};
    else return false;
    return true;
}

// every plane pointer the format reads is there
bool planes_set(int fmt, const pc_frame* f) { return f->y && f->u && (interleaved(fmt) || f->v); }

// One plane of rows of `len` elements: pointer aligned to its element, the row stride at least the row.
bool plane_ok(const void* p, int64_t sr, int es, int64_t len) { return p && reinterpret_cast<uintptr_t>(p) % es == 0 && sr >= len; }

// One picture of W luma columns; the batch strides are not looked at.
bool frame_ok(int fmt, const pc_frame* f, int W)
{
    if (!f || !fmt_ok(fmt)) return false;
    const int es = elem_bytes(fmt);
    const int64_t Wc = cdiv(W, 2);
    if (!plane_ok(f->y, f->y_row, es, W)) return false;
    if (interleaved(fmt)) return plane_ok(f->u, f->u_row, es, 2 * Wc);
    return plane_ok(f->u, f->u_row, es, Wc) && plane_ok(f->v, f->v_row, es, Wc);
}

// One plane, and one picture, as the wide path needs them: the pointer on four elements, the row stride a multiple of 4.
bool plane_wide(const void* p, int64_t sr, int es) { return reinterpret_cast<uintptr_t>(p) % (4 * es) == 0 && mult4(sr); }

bool frame_wide(int fmt, const pc_frame* f)
{
    const int es = elem_bytes(fmt);
    if (!plane_wide(f->y, f->y_row, es) || !plane_wide(f->u, f->u_row, es)) return false;
    return interleaved(fmt) || plane_wide(f->v, f->v_row, es);
}

}  // namespace

#endif  // PC_YUV_DEVICE_H

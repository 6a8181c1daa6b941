// pc_pixels.hip -- 8-bit pixels <-> the codec's float32 planes on gfx950 (pc_pixels.h).  Definition: DESIGN.md section 10.
//
// Both kernels share one decomposition: a work item is four consecutive columns of one row, all three channels (12 bytes on the 8-bit
// side, three runs of four floats on the float side); a thread takes ITEMS items NT apart, a block ITEMS * NT consecutive items of ONE
// image.  The access path (WIDE: a 32-bit word of bytes, a 128-bit word of floats; else byte by byte and float by float) only changes
// the load and store instructions, never which thread handles which pixel or in which order it adds: the bits are the same on both.
// The distortion sums run in a fixed order (thread, wave tree, waves in order, then emit_final over the block partials), no atomics.
#include "pc_image_host.h"

#include "pc_pixels.h"

namespace {

constexpr int NT = 256;                  // threads per block (4 waves)
constexpr int ITEMS = 4;                 // work items per thread
constexpr int BLOCK_ITEMS = NT * ITEMS;

// float(v) / 255.0f for every byte value, divided on the host (IEEE, correctly rounded); a kernel argument, staged into LDS.
struct Lut {
    float v[256];
};

struct U8 {                              // a u8 view (pc_pixels.h), strides in bytes
    const uint8_t* p;
    int layout;
    int64_t sb, sp, sr;
};

struct F32 {                             // float planes, strides in elements
    const float* p;
    int64_t sb, sc, sh;
};

struct Partial {                         // one block's sums per channel
    double f[3];
    unsigned long long u[3];
};

// The 12 bytes of pixels x0 .. x0+3 of row y of image b: v[c][i].  n < 4: only pixels 0 .. n-1 exist (the others read as 0).
template <bool WIDE>
__device__ __forceinline__ void load_px(const U8& s, int b, int y, int x0, int n, unsigned v[3][4])
{
    if (s.layout == PC_PIXELS_HWC) {
        const uint8_t* q = s.p + b * s.sb + y * s.sr + 3 * (int64_t)x0;
        if (WIDE && n == 4) {
            const uint32_t* w = reinterpret_cast<const uint32_t*>(q);
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
            v[0][0] = w0 & 255u; v[1][0] = (w0 >> 8) & 255u; v[2][0] = (w0 >> 16) & 255u;
            v[0][1] = w0 >> 24;  v[1][1] = w1 & 255u;        v[2][1] = (w1 >> 8) & 255u;
            v[0][2] = (w1 >> 16) & 255u; v[1][2] = w1 >> 24; v[2][2] = w2 & 255u;
            v[0][3] = (w2 >> 8) & 255u;  v[1][3] = (w2 >> 16) & 255u; v[2][3] = w2 >> 24;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][i] = i < n ? q[3 * i + c] : 0u;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint8_t* q = s.p + b * s.sb + c * s.sp + y * s.sr + x0;
            if (WIDE && n == 4) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(q);
                v[c][0] = w & 255u; v[c][1] = (w >> 8) & 255u; v[c][2] = (w >> 16) & 255u; v[c][3] = w >> 24;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[c][i] = i < n ? q[i] : 0u;
            }
        }
    }
}

template <bool WIDE>
__device__ __forceinline__ void store_px(uint8_t* p, int layout, int64_t sb, int64_t sp, int64_t sr, int b, int y, int x0, int n,
                                         const unsigned v[3][4])
{
    if (layout == PC_PIXELS_HWC) {
        uint8_t* q = p + b * sb + y * sr + 3 * (int64_t)x0;
        if (WIDE && n == 4) {
            uint32_t* w = reinterpret_cast<uint32_t*>(q);
            w[0] = v[0][0] | (v[1][0] << 8) | (v[2][0] << 16) | (v[0][1] << 24);
            w[1] = v[1][1] | (v[2][1] << 8) | (v[0][2] << 16) | (v[1][2] << 24);
            w[2] = v[2][2] | (v[0][3] << 8) | (v[1][3] << 16) | (v[2][3] << 24);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (i < n) q[3 * i + c] = (uint8_t)v[c][i];
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uint8_t* q = p + b * sb + c * sp + y * sr + x0;
            if (WIDE && n == 4) {
                *reinterpret_cast<uint32_t*>(q) = v[c][0] | (v[c][1] << 8) | (v[c][2] << 16) | (v[c][3] << 24);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < n) q[i] = (uint8_t)v[c][i];
            }
        }
    }
}

// Items are the four-column groups of the PADDED rows: item -> (yp, g), columns 4g .. 4g+3 of row yp of dst.  G = ceil(Wp / 4),
// items = Hp * G per image, blocks = ceil(items / BLOCK_ITEMS) per image.
template <bool WIDE>
__global__ __launch_bounds__(NT) void ingest_kernel(U8 src, int H, int W, float* __restrict__ dst, int Hp, int Wp, int top, int left,
                                                    int G, int items, int blocks, Lut lut)
{
    __shared__ float tab[256];
    tab[threadIdx.x] = lut.v[threadIdx.x];
    __syncthreads();
    const int b = blockIdx.x / blocks, blk = blockIdx.x - b * blocks;
    const int64_t plane = (int64_t)Hp * Wp;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int item = blk * BLOCK_ITEMS + k * NT + threadIdx.x;
        if (item >= items) break;
        const int yp = item / G, g = item - yp * G;
        const int xp0 = 4 * g, n = min(4, Wp - xp0);              // n columns of dst exist
        const int y = yp - top, x0 = xp0 - left;                  // image coordinates of the first column
        float o[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) o[c][i] = 0.f;
        if (y >= 0 && y < H && x0 + 3 >= 0 && x0 < W) {
            unsigned v[3][4];
            if (x0 >= 0 && x0 + 3 < W) {
                load_px<WIDE>(src, b, y, x0, 4, v);
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int i = 0; i < 4; ++i) o[c][i] = tab[v[c][i]];
            } else {                                              // the group straddles the image's left or right edge
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int x = x0 + i;
                    if (x >= 0 && x < W) {
                        unsigned one[3][4];
                        load_px<false>(src, b, y, x, 1, one);
#pragma unroll
                        for (int c = 0; c < 3; ++c) o[c][i] = tab[one[c][0]];
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* d = dst + (b * (int64_t)3 + c) * plane + (int64_t)yp * Wp + xp0;
            if (WIDE) {                                           // Wp % 4 == 0: n == 4
                *reinterpret_cast<float4*>(d) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < n) d[i] = o[c][i];
            }
        }
    }
}

// Items are the four-column groups of the WINDOW's rows: item -> (y, g), columns 4g .. 4g+3 of row y of the image.
template <bool WIDE, bool HAS_REF>
__global__ __launch_bounds__(NT) void emit_kernel(F32 x, int top, int left, int H, int W, int trunc, uint8_t* __restrict__ dst,
                                                  int dst_layout, int64_t db, int64_t dp, int64_t dr, U8 ref, int G, int items,
                                                  int blocks, Lut lut, Partial* __restrict__ partials)
{
    __shared__ float tab[256];
    __shared__ Partial red[NT / 64];
    if (HAS_REF) {
        tab[threadIdx.x] = lut.v[threadIdx.x];
        __syncthreads();
    }
    const int b = blockIdx.x / blocks, blk = blockIdx.x - b * blocks;
    double sf[3] = {0.0, 0.0, 0.0};
    unsigned long long su[3] = {0ull, 0ull, 0ull};
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int item = blk * BLOCK_ITEMS + k * NT + threadIdx.x;
        if (item >= items) break;
        const int y = item / G, g = item - y * G;
        const int x0 = 4 * g, n = min(4, W - x0);
        float c[3][4];
        unsigned q[3][4];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float* s = x.p + b * x.sb + ch * x.sc + (int64_t)(top + y) * x.sh + left + x0;
            if (WIDE && n == 4) {
                const float4 f = *reinterpret_cast<const float4*>(s);
                c[ch][0] = f.x; c[ch][1] = f.y; c[ch][2] = f.z; c[ch][3] = f.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) c[ch][i] = i < n ? s[i] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                c[ch][i] = fminf(fmaxf(c[ch][i], 0.f), 1.f);
                const float s255 = c[ch][i] * 255.0f;
                q[ch][i] = (unsigned)(int)(trunc ? truncf(s255) : rintf(s255));
            }
        }
        if (dst) store_px<WIDE>(dst, dst_layout, db, dp, dr, b, y, x0, n, q);
        if (HAS_REF) {
            unsigned r[3][4];
            load_px<WIDE>(ref, b, y, x0, n, r);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (i < n) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const float d = tab[r[ch][i]] - c[ch][i];
                        sf[ch] += (double)d * (double)d;
                        const int e = (int)q[ch][i] - (int)r[ch][i];
                        su[ch] += (unsigned long long)(e * e);
                    }
                }
            }
        }
    }
    if (HAS_REF) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                sf[ch] += __shfl_down(sf[ch], off, 64);
                su[ch] += __shfl_down(su[ch], off, 64);
            }
        }
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                red[threadIdx.x >> 6].f[ch] = sf[ch];
                red[threadIdx.x >> 6].u[ch] = su[ch];
            }
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            const int ch = threadIdx.x;
            double a = red[0].f[ch];
            unsigned long long u = red[0].u[ch];
            for (int wv = 1; wv < NT / 64; ++wv) {
                a += red[wv].f[ch];
                u += red[wv].u[ch];
            }
            partials[blockIdx.x].f[ch] = a;
            partials[blockIdx.x].u[ch] = u;
        }
    }
}

// One block per image: its block partials in a fixed order (thread t takes t, t + NT, ...; wave tree; waves in order).
__global__ __launch_bounds__(NT) void emit_final_kernel(const Partial* __restrict__ partials, int blocks,
                                                        unsigned long long* __restrict__ sse_u8, double* __restrict__ sse_f)
{
    __shared__ Partial red[NT / 64];
    const int b = blockIdx.x;
    const Partial* p = partials + (int64_t)b * blocks;
    double sf[3] = {0.0, 0.0, 0.0};
    unsigned long long su[3] = {0ull, 0ull, 0ull};
    for (int t = threadIdx.x; t < blocks; t += NT) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            sf[ch] += p[t].f[ch];
            su[ch] += p[t].u[ch];
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            sf[ch] += __shfl_down(sf[ch], off, 64);
            su[ch] += __shfl_down(su[ch], off, 64);
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            red[threadIdx.x >> 6].f[ch] = sf[ch];
            red[threadIdx.x >> 6].u[ch] = su[ch];
        }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int ch = threadIdx.x;
        double a = red[0].f[ch];
        unsigned long long u = red[0].u[ch];
        for (int wv = 1; wv < NT / 64; ++wv) {
            a += red[wv].f[ch];
            u += red[wv].u[ch];
        }
        sse_f[b * 3 + ch] = a;
        sse_u8[b * 3 + ch] = u;
    }
}

const Lut& lut()
{
    static const Lut t = [] {
        Lut l;
        for (int i = 0; i < 256; ++i) l.v[i] = (float)i / 255.0f;
        return l;
    }();
    return t;
}

bool layout_ok(int layout) { return layout == PC_PIXELS_HWC || layout == PC_PIXELS_CHW; }

// A u8 view of B images of H x W pixels: strides in range; `disjoint` (destinations): rows inside planes inside images, each
// level's stride at least the bytes the level below spans, which is sufficient (not necessary) for no byte to be written twice.
bool view_ok(const void* p, int layout, int64_t sb, int64_t sp, int64_t sr, int B, int H, int W, bool disjoint)
{
    if (!p || !layout_ok(layout)) return false;
    const bool chw = layout == PC_PIXELS_CHW;
    const int64_t row = chw ? (int64_t)W : 3 * (int64_t)W;
    if (sr < row || sb < 1 || (chw && sp < 1)) return false;
    if (disjoint) {
        const int64_t plane = (int64_t)(H - 1) * sr + row;                  // bytes spanned by the rows of one plane (or HWC image)
        if (chw && sp < plane) return false;
        const int64_t image = chw ? 2 * sp + plane : plane;
        if (B > 1 && sb < image) return false;
    }
    return true;
}

// Sizes every call shares: B, H, W >= 1 and the block count of an item space of rows x ceil(cols / 4) per image within 32 bits.
struct Grid {
    int G, items, blocks;
};

bool grid_of(int B, int rows, int cols, Grid& g)
{
    if (B < 1 || rows < 1 || cols < 1) return false;
    const int64_t G = cdiv(cols, 4), items = (int64_t)rows * G;
    if (items > INT32_MAX - BLOCK_ITEMS) return false;
    const int64_t blocks = cdiv(items, BLOCK_ITEMS);
    if ((int64_t)B * blocks > INT32_MAX) return false;
    g.G = (int)G;
    g.items = (int)items;
    g.blocks = (int)blocks;
    return true;
}

// The alignment of a u8 view as the wide path needs it; `shift`: bytes from the pointer back to the first work item's column 0.
bool u8_wide(const void* p, int layout, int64_t sb, int64_t sp, int64_t sr, int64_t shift)
{
    const int64_t a = (int64_t)(reinterpret_cast<uintptr_t>(p) % 4) - shift % 4;
    return mult4(a) && mult4(sb) && mult4(sr) && (layout == PC_PIXELS_HWC || mult4(sp));
}

bool f32_wide(const void* p, int64_t fb, int64_t fc, int64_t fh, int64_t shift)
{
    return aligned(p, 16) && mult4(fb) && mult4(fc) && mult4(fh) && mult4(shift);
}

// The one place that decides the access path: the calls launch from it, pc_pixels_plan reports it.
bool wide_path(int op, const void* u8, int layout, int64_t sb, int64_t sp, int64_t sr, const void* f32, int64_t fb, int64_t fc,
               int64_t fh, int left, const void* ref, int ref_layout, int64_t rb, int64_t rp, int64_t rr)
{
    if (op == PC_PIXELS_INGEST)
        return f32_wide(f32, fb, fc, fh, 0) && u8_wide(u8, layout, sb, sp, sr, (layout == PC_PIXELS_HWC ? 3 : 1) * (int64_t)left);
    return f32_wide(f32, fb, fc, fh, left) && (!u8 || u8_wide(u8, layout, sb, sp, sr, 0)) &&
           (!ref || u8_wide(ref, ref_layout, rb, rp, rr, 0));
}

bool ingest_args_ok(const void* src, int layout, int64_t sb, int64_t sp, int64_t sr, int B, int H, int W, const void* dst, int Hp,
                    int Wp, int top, int left, Grid& g)
{
    if (!dst || !aligned(dst, 4) || B < 1 || H < 1 || W < 1) return false;
    if (top < 0 || left < 0 || Hp < 1 || Wp < 1 || (int64_t)top + H > Hp || (int64_t)left + W > Wp) return false;
    return view_ok(src, layout, sb, sp, sr, B, H, W, false) && grid_of(B, Hp, Wp, g);
}

bool emit_args_ok(const void* x, int64_t sxb, int64_t sxc, int64_t sxh, int Hp, int Wp, int top, int left, int B, int H, int W,
                  const void* dst, int dst_layout, int64_t db, int64_t dp, int64_t dr, const void* ref, int ref_layout, int64_t rb,
                  int64_t rp, int64_t rr, Grid& g)
{
    if (!x || !aligned(x, 4) || B < 1 || H < 1 || W < 1) return false;
    if (top < 0 || left < 0 || Hp < 1 || Wp < 1 || (int64_t)top + H > Hp || (int64_t)left + W > Wp) return false;
    if (sxh < Wp || sxc < 1 || sxb < 1) return false;
    if (dst ? !view_ok(dst, dst_layout, db, dp, dr, B, H, W, true) : !ref) return false;        // sums only: no image is written
    if (ref && !view_ok(ref, ref_layout, rb, rp, rr, B, H, W, false)) return false;
    return grid_of(B, H, W, g);
}

}  // namespace

extern "C" int pc_pixels_plan(int op, const void* u8, int layout, int64_t s_batch, int64_t s_plane, int64_t s_row, const void* f32,
                              int64_t fb, int64_t fc, int64_t fh, int top, int left, int B, int H, int W, const void* ref,
                              int ref_layout, int64_t r_batch, int64_t r_plane, int64_t r_row, int* wide)
{
    if ((op != PC_PIXELS_INGEST && op != PC_PIXELS_EMIT) || !f32 || !wide) return PC_ERR_ARG;
    if (u8 ? !layout_ok(layout) : (op != PC_PIXELS_EMIT || !ref)) return PC_ERR_ARG;
    if (B < 1 || H < 1 || W < 1 || top < 0 || left < 0) return PC_ERR_ARG;
    if (op == PC_PIXELS_INGEST) ref = nullptr;
    if (ref && !layout_ok(ref_layout)) return PC_ERR_ARG;
    *wide = wide_path(op, u8, layout, s_batch, s_plane, s_row, f32, fb, fc, fh, left, ref, ref_layout, r_batch, r_plane, r_row) ? 1 : 0;
    return PC_OK;
}

extern "C" int pc_pixels_ingest_u8(const uint8_t* src, int layout, int64_t s_batch, int64_t s_plane, int64_t s_row, int B, int H, int W,
                                   float* dst, int Hp, int Wp, int top, int left, void* stream)
{
    Grid g;
    if (!ingest_args_ok(src, layout, s_batch, s_plane, s_row, B, H, W, dst, Hp, Wp, top, left, g)) return PC_ERR_ARG;
    const int64_t plane = (int64_t)Hp * Wp;
    const bool wide = wide_path(PC_PIXELS_INGEST, src, layout, s_batch, s_plane, s_row, dst, 3 * plane, plane, Wp, left, nullptr, 0, 0,
                                0, 0);
    const U8 s{src, layout, s_batch, s_plane, s_row};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(B * g.blocks)), block(NT);
    if (wide)
        hipLaunchKernelGGL(ingest_kernel<true>, grid, block, 0, st, s, H, W, dst, Hp, Wp, top, left, g.G, g.items, g.blocks, lut());
    else
        hipLaunchKernelGGL(ingest_kernel<false>, grid, block, 0, st, s, H, W, dst, Hp, Wp, top, left, g.G, g.items, g.blocks, lut());
    HIPCHK(hipGetLastError());
    return PC_OK;
}

extern "C" size_t pc_pixels_emit_workspace_size(int B, int H, int W)
{
    Grid g;
    return grid_of(B, H, W, g) ? (size_t)B * g.blocks * sizeof(Partial) : 0;
}

extern "C" int pc_pixels_emit_u8(const float* x, int64_t sxb, int64_t sxc, int64_t sxh, int Hp, int Wp, int top, int left, int B, int H,
                                 int W, int rounding, uint8_t* dst, int dst_layout, int64_t d_batch, int64_t d_plane, int64_t d_row,
                                 const uint8_t* ref, int ref_layout, int64_t r_batch, int64_t r_plane, int64_t r_row, void* workspace,
                                 size_t workspace_bytes, uint64_t* sse_u8, double* sse_f, void* stream)
{
    Grid g;
    if (!emit_args_ok(x, sxb, sxc, sxh, Hp, Wp, top, left, B, H, W, dst, dst_layout, d_batch, d_plane, d_row, ref, ref_layout, r_batch,
                      r_plane, r_row, g))
        return PC_ERR_ARG;
    if (rounding != PC_PIXELS_NEAREST && rounding != PC_PIXELS_TRUNC) return PC_ERR_ARG;
    if (ref) {
        if (!workspace || !aligned(workspace, 8)) return PC_ERR_ARG;
        if (!sse_u8 || !aligned(sse_u8, 8) || !sse_f || !aligned(sse_f, 8)) return PC_ERR_ARG;
        if (workspace_bytes < (size_t)B * g.blocks * sizeof(Partial)) return PC_ERR_ARG;
    }
    const bool wide = wide_path(PC_PIXELS_EMIT, dst, dst_layout, d_batch, d_plane, d_row, x, sxb, sxc, sxh, left, ref, ref_layout,
                                r_batch, r_plane, r_row);
    const F32 xv{x, sxb, sxc, sxh};
    const U8 rv{ref, ref_layout, r_batch, r_plane, r_row};
    const int trunc = rounding == PC_PIXELS_TRUNC;
    Partial* part = static_cast<Partial*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(B * g.blocks)), block(NT);
#define PC_EMIT(WIDE, REF)                                                                                                            \
    hipLaunchKernelGGL((emit_kernel<WIDE, REF>), grid, block, 0, st, xv, top, left, H, W, trunc, dst, dst_layout, d_batch, d_plane,  \
                       d_row, rv, g.G, g.items, g.blocks, lut(), part)
    if (ref) {
        if (wide) PC_EMIT(true, true); else PC_EMIT(false, true);
    } else {
        if (wide) PC_EMIT(true, false); else PC_EMIT(false, false);
    }
#undef PC_EMIT
    HIPCHK(hipGetLastError());
    if (ref) {
        hipLaunchKernelGGL(emit_final_kernel, dim3((unsigned)B), block, 0, st, part, g.blocks,
                           reinterpret_cast<unsigned long long*>(sse_u8), sse_f);
        HIPCHK(hipGetLastError());
    }
    return PC_OK;
}

extern "C" const char* pc_pixels_strerror(int code)
{
    switch (code) {
    case PC_OK: return "ok";
    case PC_ERR_ARG: return "invalid argument, unsupported shape or workspace too small (pc_pixels_emit_workspace_size)";
    case PC_ERR_HIP: return "HIP runtime error";
    default: return "unknown error";
    }
}

extern "C" int pc_pixels_last_hip_error(void) { return g_last_hip.load(); }

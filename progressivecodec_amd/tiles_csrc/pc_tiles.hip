// pc_tiles.hip -- one 8-bit image <-> independent tiles of float32 planes on gfx950 (pc_tiles.h).  Definition: DESIGN.md section 11.
//
// The decomposition is pc_pixels.hip's: a work item is four consecutive columns of one row, all three channels (12 bytes on the 8-bit
// side, three runs of four floats per tile on the float side); a thread takes ITEMS items NT apart, a block ITEMS * NT consecutive
// items.  The groups are aligned to multiples of 4 in tile columns (cut) and in image columns (stitch); the stride S = T - O is a
// multiple of 4, so a group never straddles a tile edge or a band edge: it has ONE set of covering tiles, and the float side is the
// aligned one.  The access path (WIDE: a 32-bit word of bytes, a 128-bit word of floats; else byte by byte and float by float) only
// changes the load and store instructions, never which thread handles which pixel or in which order it adds: the bits are the same
// on both.  The distortion sums run in a fixed order (thread, wave tree, waves in order, then final_kernel over the block partials),
// no atomics.
#include "pc_image_host.h"
#include "pc_tile_grid.h"

#include "pc_tiles.h"

namespace {

constexpr int NT = 256;                  // threads per block (4 waves)
constexpr int ITEMS = 4;                 // work items per thread
constexpr int BLOCK_ITEMS = NT * ITEMS;

// float(v) / 255.0f for every byte value, divided on the host (IEEE, correctly rounded); a kernel argument, staged into LDS.
struct Lut {
    float v[256];
};

struct U8 {                              // a u8 view (pc_tiles.h), strides in bytes
    const uint8_t* p;
    int layout;
    int64_t sp, sr;
};

struct Partial {                         // one block's sums per channel
    double f[3];
    unsigned long long u[3];
};

// The bytes of pixels x0 + lo .. x0 + hi - 1 of row y: v[c][i]; the other lanes read as 0.  x0 may lie up to three pixels before the
// view's first column (then lo > 0): only the lanes lo .. hi - 1 are addressed.
template <bool WIDE>
__device__ __forceinline__ void load_px(const U8& s, int64_t y, int64_t x0, int lo, int hi, unsigned v[3][4])
{
    if (s.layout == PC_TILES_HWC) {
        const uint8_t* q = s.p + y * s.sr + 3 * x0;
        if (WIDE && lo == 0 && hi == 4) {
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
                for (int c = 0; c < 3; ++c) v[c][i] = (i >= lo && i < hi) ? q[3 * i + c] : 0u;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint8_t* q = s.p + c * s.sp + y * s.sr + x0;
            if (WIDE && lo == 0 && hi == 4) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(q);
                v[c][0] = w & 255u; v[c][1] = (w >> 8) & 255u; v[c][2] = (w >> 16) & 255u; v[c][3] = w >> 24;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[c][i] = (i >= lo && i < hi) ? q[i] : 0u;
            }
        }
    }
}

template <bool WIDE>
__device__ __forceinline__ void store_px(uint8_t* p, int layout, int64_t sp, int64_t sr, int64_t y, int64_t x0, int lo, int hi,
                                         const unsigned v[3][4])
{
    if (layout == PC_TILES_HWC) {
        uint8_t* q = p + y * sr + 3 * x0;
        if (WIDE && lo == 0 && hi == 4) {
            uint32_t* w = reinterpret_cast<uint32_t*>(q);
            w[0] = v[0][0] | (v[1][0] << 8) | (v[2][0] << 16) | (v[0][1] << 24);
            w[1] = v[1][1] | (v[2][1] << 8) | (v[0][2] << 16) | (v[1][2] << 24);
            w[2] = v[2][2] | (v[0][3] << 8) | (v[1][3] << 16) | (v[2][3] << 24);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (i >= lo && i < hi) q[3 * i + c] = (uint8_t)v[c][i];
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uint8_t* q = p + c * sp + y * sr + x0;
            if (WIDE && lo == 0 && hi == 4) {
                *reinterpret_cast<uint32_t*>(q) = v[c][0] | (v[c][1] << 8) | (v[c][2] << 16) | (v[c][3] << 24);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i >= lo && i < hi) q[i] = (uint8_t)v[c][i];
            }
        }
    }
}

// Items are the four-column groups of the tiles' rows: item -> (tile t of the rectangle, row r, group g), tile columns 4g .. 4g+3.
// G4 = T / 4, tile_items = T * G4, items = nty * ntx * tile_items.
template <bool WIDE>
__global__ __launch_bounds__(NT) void cut_kernel(U8 src, int H, int W, int T, int S, int ty0, int tx0, int ntx, float* __restrict__ dst,
                                                 int G4, int tile_items, int64_t items, Lut lut)
{
    __shared__ float tab[256];
    tab[threadIdx.x] = lut.v[threadIdx.x];
    __syncthreads();
    const int64_t plane = (int64_t)T * T;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int64_t item = (int64_t)blockIdx.x * BLOCK_ITEMS + k * NT + threadIdx.x;
        if (item >= items) break;
        const int t = (int)(item / tile_items), rem = (int)(item - (int64_t)t * tile_items);
        const int r = rem / G4, g = rem - r * G4;
        const int a = t / ntx, b = t - a * ntx;
        const int64_t Y = (int64_t)(ty0 + a) * S + r, X0 = (int64_t)(tx0 + b) * S + 4 * g;      // image coordinates of the first column
        float o[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) o[c][i] = 0.f;
        if (Y < H && X0 < W) {
            unsigned v[3][4];
            const int n = (int)(W - X0 < 4 ? W - X0 : 4);                                     // n < 4: the group straddles the right edge
            load_px<WIDE>(src, Y, X0, 0, n, v);
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int i = 0; i < 4; ++i) o[c][i] = i < n ? tab[v[c][i]] : 0.f;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* d = dst + ((int64_t)t * 3 + c) * plane + (int64_t)r * T + 4 * g;
            if (WIDE) {
                *reinterpret_cast<float4*>(d) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) d[i] = o[c][i];
            }
        }
    }
}

// num / den for two small integers as the correctly rounded float32 quotient: both are exact doubles, the double quotient carries
// 53 >= 2 * 24 + 2 bits, so rounding it to float32 rounds the exact quotient once.
__device__ __forceinline__ float quotient(int num, int den) { return (float)((double)num / (double)den); }

// Items are the four-column groups of the WINDOW's rows, aligned in image columns: item -> (y, g), image columns X0 .. X0+3 with
// X0 = 4 * (x0 / 4 + g) of image row y0 + y; the lanes lo .. hi-1 of a group lie inside the window.  G groups per row.
template <bool WIDE, bool HAS_REF>
__global__ __launch_bounds__(NT) void stitch_kernel(F32 x, int T, int S, int O, int ny, int nx, int ty0, int tx0, int ntx, int y0, int x0,
                                                    int w, int trunc, uint8_t* __restrict__ dst, int dst_layout, int64_t dp, int64_t dr,
                                                    U8 ref, int G, int64_t items, Lut lut, Partial* __restrict__ partials)
{
    __shared__ float tab[256];
    __shared__ Partial red[NT / 64];
    if (HAS_REF) {
        tab[threadIdx.x] = lut.v[threadIdx.x];
        __syncthreads();
    }
    double sf[3] = {0.0, 0.0, 0.0};
    unsigned long long su[3] = {0ull, 0ull, 0ull};
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int64_t item = (int64_t)blockIdx.x * BLOCK_ITEMS + k * NT + threadIdx.x;
        if (item >= items) break;
        const int y = (int)(item / G), g = (int)(item - (int64_t)y * G);
        const int Y = y0 + y, X0 = 4 * (x0 / 4 + g);
        const int lo = x0 > X0 ? x0 - X0 : 0, hi = x0 + w - X0 < 4 ? x0 + w - X0 : 4;
        // the covering tiles per axis, in ascending order: tile index, row / first column inside it, weight(s)
        int ty[2], row[2], tx[2], col[2], nyc = 0, nxc = 0;
        float wy[2], wx[2][4];
        {
            const int i = Y / S < ny - 1 ? Y / S : ny - 1, u = Y - i * S;
            if (i > 0 && u < O) {
                ty[0] = i - 1; row[0] = u + S; wy[0] = quotient(2 * (O - 1 - u) + 1, 2 * O);
                ty[1] = i;     row[1] = u;     wy[1] = quotient(2 * u + 1, 2 * O);
                nyc = 2;
            } else {
                ty[0] = i; row[0] = u; wy[0] = 1.0f;
                nyc = 1;
            }
        }
        {
            const int i = X0 / S < nx - 1 ? X0 / S : nx - 1, u = X0 - i * S;
            if (i > 0 && u < O) {                                   // O and S are multiples of 4: all four columns are in the band
                tx[0] = i - 1; col[0] = u + S;
                tx[1] = i;     col[1] = u;
#pragma unroll
                for (int l = 0; l < 4; ++l) {
                    wx[0][l] = quotient(2 * (O - 1 - (u + l)) + 1, 2 * O);
                    wx[1][l] = quotient(2 * (u + l) + 1, 2 * O);
                }
                nxc = 2;
            } else {
                tx[0] = i; col[0] = u;
#pragma unroll
                for (int l = 0; l < 4; ++l) wx[0][l] = 1.0f;
                nxc = 1;
            }
        }
        float m[3][4];
        unsigned q[3][4];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
            for (int l = 0; l < 4; ++l) m[ch][l] = 0.f;
        for (int a = 0; a < nyc; ++a) {
            for (int b = 0; b < nxc; ++b) {
                const int64_t tl = (int64_t)(ty[a] - ty0) * ntx + (tx[b] - tx0);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    // col + 3 < T for every group that starts inside the image, so the whole group lies inside the tile's row
                    const float* s = x.p + tl * x.st + ch * x.sc + (int64_t)row[a] * x.sh + col[b];
                    float v[4];
                    if (WIDE) {
                        const float4 f = *reinterpret_cast<const float4*>(s);
                        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
                    } else {
#pragma unroll
                        for (int l = 0; l < 4; ++l) v[l] = (l >= lo && l < hi) ? s[l] : 0.f;
                    }
#pragma unroll
                    for (int l = 0; l < 4; ++l) {
                        const float c = fminf(fmaxf(v[l], 0.f), 1.f);
                        m[ch][l] = fmaf(wy[a] * wx[b][l], c, m[ch][l]);
                    }
                }
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                const float s255 = m[ch][l] * 255.0f;
                q[ch][l] = (unsigned)(int)(trunc ? truncf(s255) : rintf(s255));
            }
        const int64_t xw = (int64_t)X0 - x0;                        // the group's first column relative to the window: -3 .. w-1
        if (dst) store_px<WIDE>(dst, dst_layout, dp, dr, y, xw, lo, hi, q);
        if (HAS_REF) {
            unsigned r[3][4];
            load_px<WIDE>(ref, y, xw, lo, hi, r);
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                if (l >= lo && l < hi) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const float d = tab[r[ch][l]] - m[ch][l];
                        sf[ch] += (double)d * (double)d;
                        const int e = (int)q[ch][l] - (int)r[ch][l];
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

// One block: the block partials in a fixed order (thread t takes t, t + NT, ...; wave tree; waves in order).
__global__ __launch_bounds__(NT) void final_kernel(const Partial* __restrict__ p, int blocks, unsigned long long* __restrict__ sse_u8,
                                                   double* __restrict__ sse_f)
{
    __shared__ Partial red[NT / 64];
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
        sse_f[ch] = a;
        sse_u8[ch] = u;
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

bool layout_ok(int layout) { return layout == PC_TILES_HWC || layout == PC_TILES_CHW; }

// A u8 view of h x w pixels: strides in range; `disjoint` (destinations): rows inside planes, the plane stride at least the bytes the
// rows of a plane span, which is sufficient (not necessary) for no byte to be written twice.
bool view_ok(const void* p, int layout, int64_t sp, int64_t sr, int h, int w, bool disjoint)
{
    if (!p || !layout_ok(layout)) return false;
    const bool chw = layout == PC_TILES_CHW;
    const int64_t row = chw ? (int64_t)w : 3 * (int64_t)w;
    if (sr < row || (chw && sp < 1)) return false;
    if (disjoint && chw && sp < (int64_t)(h - 1) * sr + row) return false;
    return true;
}

// The item space of a stitch: rows x the image-aligned four-column groups that meet [x0, x0 + w).
struct Items {
    int G, blocks;
    int64_t items;
};

bool items_of(int x0, int h, int w, Items& it)
{
    if (x0 < 0 || h < 1 || w < 1 || (int64_t)x0 + w > INT32_MAX) return false;
    const int64_t G = cdiv((int64_t)x0 + w, 4) - x0 / 4, items = (int64_t)h * G, blocks = cdiv(items, BLOCK_ITEMS);
    if (blocks > INT32_MAX) return false;
    it.G = (int)G;
    it.items = items;
    it.blocks = (int)blocks;
    return true;
}

// The alignment of a u8 view as the wide path needs it; `shift`: bytes from the pointer back to the first work item's column 0.
bool u8_wide(const void* p, int layout, int64_t sp, int64_t sr, int64_t shift)
{
    const int64_t a = (int64_t)(reinterpret_cast<uintptr_t>(p) % 4) - shift % 4;
    return mult4(a) && mult4(sr) && (layout == PC_TILES_HWC || mult4(sp));
}

// The one place that decides the access path: the calls launch from it, pc_tiles_plan reports it.
bool wide_path(int op, const void* u8, int layout, int64_t sp, int64_t sr, const void* f32, int64_t ft, int64_t fc, int64_t fh, int x0,
               const void* ref, int ref_layout, int64_t rp, int64_t rr)
{
    if (op == PC_TILES_CUT) return f32_wide(f32, ft, fc, fh) && u8_wide(u8, layout, sp, sr, 0);
    const int back = x0 % 4;
    return f32_wide(f32, ft, fc, fh) && (!u8 || u8_wide(u8, layout, sp, sr, (layout == PC_TILES_HWC ? 3 : 1) * back)) &&
           (!ref || u8_wide(ref, ref_layout, rp, rr, (ref_layout == PC_TILES_HWC ? 3 : 1) * back));
}

}  // namespace

extern "C" int pc_tiles_grid(int H, int W, int T, int O, int* ny, int* nx)
{
    Geo g;
    if (!ny || !nx || !geo_of(H, W, T, O, INT_MAX, g)) return PC_ERR_ARG;
    *ny = g.ny;
    *nx = g.nx;
    return PC_OK;
}

extern "C" int pc_tiles_plan(int op, const void* u8, int layout, int64_t s_plane, int64_t s_row, const void* f32, int64_t ft, int64_t fc,
                             int64_t fh, int x0, const void* ref, int ref_layout, int64_t r_plane, int64_t r_row, int* wide)
{
    if ((op != PC_TILES_CUT && op != PC_TILES_STITCH) || !f32 || !wide) return PC_ERR_ARG;
    if (u8 ? !layout_ok(layout) : (op != PC_TILES_STITCH || !ref)) return PC_ERR_ARG;
    if (op == PC_TILES_CUT) {
        ref = nullptr;
        x0 = 0;
    }
    if (x0 < 0 || (ref && !layout_ok(ref_layout))) return PC_ERR_ARG;
    *wide = wide_path(op, u8, layout, s_plane, s_row, f32, ft, fc, fh, x0, ref, ref_layout, r_plane, r_row) ? 1 : 0;
    return PC_OK;
}

extern "C" int pc_tiles_cut_u8(const uint8_t* src, int layout, int64_t s_plane, int64_t s_row, int H, int W, int T, int O, int ty0, int tx0,
                               int nty, int ntx, float* dst, void* stream)
{
    Geo g;
    if (!geo_of(H, W, T, O, INT_MAX, g) || !rect_ok(g, ty0, tx0, nty, ntx)) return PC_ERR_ARG;
    if (!dst || !aligned(dst, 4) || !view_ok(src, layout, s_plane, s_row, H, W, false)) return PC_ERR_ARG;
    const int G4 = T / 4;
    const int64_t tile_items = (int64_t)T * G4, tiles = (int64_t)nty * ntx;
    if (tile_items > INT32_MAX || tiles > INT32_MAX / 3) return PC_ERR_ARG;
    const int64_t items = tiles * tile_items, blocks = cdiv(items, BLOCK_ITEMS);
    if (blocks > INT32_MAX) return PC_ERR_ARG;
    const int64_t plane = (int64_t)T * T;
    const bool wide = wide_path(PC_TILES_CUT, src, layout, s_plane, s_row, dst, 3 * plane, plane, T, 0, nullptr, 0, 0, 0);
    const U8 s{src, layout, s_plane, s_row};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks), block(NT);
    if (wide)
        hipLaunchKernelGGL(cut_kernel<true>, grid, block, 0, st, s, H, W, T, g.S, ty0, tx0, ntx, dst, G4, (int)tile_items, items, lut());
    else
        hipLaunchKernelGGL(cut_kernel<false>, grid, block, 0, st, s, H, W, T, g.S, ty0, tx0, ntx, dst, G4, (int)tile_items, items, lut());
    HIPCHK(hipGetLastError());
    return PC_OK;
}

extern "C" size_t pc_tiles_stitch_workspace_size(int x0, int h, int w)
{
    Items it;
    return items_of(x0, h, w, it) ? (size_t)it.blocks * sizeof(Partial) : 0;
}

extern "C" int pc_tiles_stitch_u8(const float* x, int64_t sxt, int64_t sxc, int64_t sxh, int H, int W, int T, int O, int ty0, int tx0,
                                  int nty, int ntx, int y0, int x0, int h, int w, int rounding, uint8_t* dst, int dst_layout,
                                  int64_t d_plane, int64_t d_row, const uint8_t* ref, int ref_layout, int64_t r_plane, int64_t r_row,
                                  void* workspace, size_t workspace_bytes, uint64_t* sse_u8, double* sse_f, void* stream)
{
    Geo g;
    Items it;
    if (!geo_of(H, W, T, O, INT_MAX, g) || !rect_ok(g, ty0, tx0, nty, ntx)) return PC_ERR_ARG;
    if (!x || !aligned(x, 4) || sxh < T || sxc < 1 || sxt < 1) return PC_ERR_ARG;
    if (y0 < 0 || x0 < 0 || h < 1 || w < 1 || (int64_t)y0 + h > H || (int64_t)x0 + w > W || !items_of(x0, h, w, it)) return PC_ERR_ARG;
    // every tile that covers a pixel of the window lies in the rectangle
    if (first_tile(y0, g.S, O, g.ny) < ty0 || last_tile(y0 + h - 1, g.S, g.ny) >= ty0 + nty) return PC_ERR_ARG;
    if (first_tile(x0, g.S, O, g.nx) < tx0 || last_tile(x0 + w - 1, g.S, g.nx) >= tx0 + ntx) return PC_ERR_ARG;
    if (rounding != PC_TILES_NEAREST && rounding != PC_TILES_TRUNC) return PC_ERR_ARG;
    if (dst ? !view_ok(dst, dst_layout, d_plane, d_row, h, w, true) : !ref) return PC_ERR_ARG;          // sums only: no image is written
    if (ref) {
        if (!view_ok(ref, ref_layout, r_plane, r_row, h, w, false)) return PC_ERR_ARG;
        if (!workspace || !aligned(workspace, 8)) return PC_ERR_ARG;
        if (!sse_u8 || !aligned(sse_u8, 8) || !sse_f || !aligned(sse_f, 8)) return PC_ERR_ARG;
        if (workspace_bytes < (size_t)it.blocks * sizeof(Partial)) return PC_ERR_ARG;
    }
    const bool wide = wide_path(PC_TILES_STITCH, dst, dst_layout, d_plane, d_row, x, sxt, sxc, sxh, x0, ref, ref_layout, r_plane, r_row);
    const F32 xv{x, sxt, sxc, sxh};
    const U8 rv{ref, ref_layout, r_plane, r_row};
    const int trunc = rounding == PC_TILES_TRUNC;
    Partial* part = static_cast<Partial*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)it.blocks), block(NT);
#define PC_STITCH(WIDE, REF)                                                                                                          \
    hipLaunchKernelGGL((stitch_kernel<WIDE, REF>), grid, block, 0, st, xv, T, g.S, O, g.ny, g.nx, ty0, tx0, ntx, y0, x0, w, trunc, dst,  \
                       dst_layout, d_plane, d_row, rv, it.G, it.items, lut(), part)
    if (ref) {
        if (wide) PC_STITCH(true, true); else PC_STITCH(false, true);
    } else {
        if (wide) PC_STITCH(true, false); else PC_STITCH(false, false);
    }
#undef PC_STITCH
    HIPCHK(hipGetLastError());
    if (ref) {
        hipLaunchKernelGGL(final_kernel, dim3(1), block, 0, st, part, it.blocks, reinterpret_cast<unsigned long long*>(sse_u8), sse_f);
        HIPCHK(hipGetLastError());
    }
    return PC_OK;
}

extern "C" const char* pc_tiles_strerror(int code)
{
    switch (code) {
    case PC_OK: return "ok";
    case PC_ERR_ARG: return "invalid argument, geometry outside pc_tiles.h, tiles missing from the rectangle or workspace too small";
    case PC_ERR_HIP: return "HIP runtime error";
    default: return "unknown error";
    }
}

extern "C" int pc_tiles_last_hip_error(void) { return g_last_hip.load(); }

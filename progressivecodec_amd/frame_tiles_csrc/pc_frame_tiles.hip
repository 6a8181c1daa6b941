// pc_frame_tiles.hip -- one YUV 4:2:0 frame (NV12 / I420 / P010) <-> independent tiles of float32 RGB planes on gfx950
// (pc_frame_tiles.h).  Definition: DESIGN.md section 14, the composition of sections 13 and 11; the cut is cut_item of
// image_csrc/pc_yuv_items.h, as in pc_frames.hip and pc_clips.hip; loads, levels and the emit arithmetic are
// image_csrc/pc_yuv_device.h's, the geometry image_csrc/pc_tile_grid.h's, the reduction image_csrc/pc_reduce.h's.
//
// A work item is eight consecutive luma columns: of ONE tile row for the cut (aligned in tile columns; its two chroma rows are chosen
// per luma row), of one ROW PAIR of the window for the stitch (aligned to a multiple of 8 in FRAME columns; four chroma samples, each
// the mean of 2 x 2 blended luma positions the thread holds).  A thread takes one item, a block NT consecutive items.  S = T - O is a
// multiple of 4, so each four-column half of a stitch item has ONE set of covering tiles and its tile-local column is a multiple of 4
// (the float side is the aligned one); a band edge may fall between the halves, so tiles and weights are per half and per column.  S is
// even and the window's first row is even, so the two rows of a pair have the same covering tiles and differ in wy only.  The access
// path (WIDE: four elements of a plane and four floats per access; else one by one) only changes the load and store instructions,
// never which thread handles which sample or in which order it adds: the bits are the same on both.  No LDS on the data path; the
// sums go thread, wave tree, waves in order (12 words of LDS), then final_kernel over the block partials, no atomics.
#include <climits>

#include "pc_image_host.h"
#include "pc_reduce.h"
#include "pc_tile_grid.h"
#include "pc_yuv_device.h"
#include "pc_yuv_items.h"

#include "pc_frame_tiles.h"

namespace {

struct Tiling {                          // the grid and the rectangle a tile set holds
    int T, S, O, ny, nx, ty0, tx0, ntx;
};

// Items are the eight-column groups of the tiles' rows: item -> (tile t of the rectangle, row r, group g), tile columns 8g .. 8g+7.
// G8 = T / 8, tile_items = T * G8, items = nty * ntx * tile_items.  SH: the bits below the code in an element (P010: 6).  The chroma
// taps are clamped at the FRAME's edges Hc - 1, Wc - 1.  WIDE needs S a multiple of 8: X0 is then one, and X0 / 2 a multiple of 4.
template <class T, bool IL, bool WIDE>
__global__ __launch_bounds__(NT) void cut_kernel(Planes<const T> s, int H, int W, int Hc, int Wc, Tiling tg, float* __restrict__ dst, int G8,
                                                 int tile_items, int64_t items, int linear, Levels lv, IngestCoef k)
{
    const int64_t item = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (item >= items) return;
    const int t = (int)(item / tile_items), rem = (int)(item - (int64_t)t * tile_items);
    const int r = rem / G8, g = rem - r * G8;
    const int ta = t / tg.ntx, tb = t - ta * tg.ntx;
    const int64_t Y64 = (int64_t)(tg.ty0 + ta) * tg.S + r, X64 = (int64_t)(tg.tx0 + tb) * tg.S + COLS * g;      // frame coordinates
    float o[3][COLS];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < COLS; ++i) o[c][i] = 0.f;
    if (Y64 < H && X64 < W) cut_item<T, IL, WIDE, false>(s, W, Hc, Wc, (int)Y64, (int)X64, linear, lv, k, o);
    const int64_t plane = (int64_t)tg.T * tg.T;
#pragma unroll
    for (int c = 0; c < 3; ++c) store8<WIDE>(dst + ((int64_t)t * 3 + c) * plane + (int64_t)r * tg.T + COLS * g, o[c], COLS);
}

// num / den for two small integers as the correctly rounded float32 quotient: both are exact doubles, the double quotient carries
// 53 >= 2 * 24 + 2 bits, so rounding it to float32 rounds the exact quotient once.
__device__ __forceinline__ float quotient(int num, int den) { return (float)((double)num / (double)den); }

// One item of the stitch: frame rows Y0 and Y0 + dy (dy = 0 where the window's odd last row stands in for the one below it), frame
// columns X0 .. X0+7 of which the lanes lo .. hi-1 lie in the window (lo even); yw, xw: the first row and column relative to the
// window (xw may be negative, down to -6).  FULL: lo == 0, hi == 8 and every plane access is wide; else element by element.  The
// whole item is compiled twice, so that the two kinds of access never meet in one basic block.
template <class T, bool IL, bool WIDE, bool FULL, bool HAS_REF>
__device__ __forceinline__ void stitch_item(const F32& x, const Tiling& tg, int Y0, int dy, int X0, int lo, int hi, int yw, int xw,
                                            const Planes<T>& dst, const Planes<const T>& ref, const Levels& lv, const EmitCoef& k,
                                            unsigned long long su[3])
{
    constexpr int SH = sizeof(T) == 2 ? 6 : 0;
    constexpr int CS = IL ? 2 : 1;
    const int S = tg.S, O = tg.O;
    // the covering tiles along y, ascending: tile index, the row of Y0 inside it, the weights of the two rows
    int ty[2] = {0, 0}, row[2] = {0, 0}, nyc;
    float wy[2][2] = {{1.0f, 0.f}, {1.0f, 0.f}};                  // [row of the pair][covering tile]
    {
        const int i = Y0 / S < tg.ny - 1 ? Y0 / S : tg.ny - 1, u = Y0 - i * S;
        if (i > 0 && u < O) {                                      // u is even and O a multiple of 4: u + dy < O as well
            ty[0] = i - 1; row[0] = u + S;
            ty[1] = i;     row[1] = u;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int ur = u + r * dy;
                wy[r][0] = quotient(2 * (O - 1 - ur) + 1, 2 * O);
                wy[r][1] = quotient(2 * ur + 1, 2 * O);
            }
            nyc = 2;
        } else {
            ty[0] = i; row[0] = u;
            nyc = 1;
        }
    }
    float m[2][3][COLS];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
            for (int q = 0; q < COLS; ++q) m[r][ch][q] = 0.f;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        if (FULL || (lo < 4 * hf + 4 && hi > 4 * hf)) {            // the half meets the window: it starts inside the frame
            const int c0 = X0 + 4 * hf;
            int tx[2] = {0, 0}, col[2] = {0, 0}, nxc;
            float wx[2][4];
            const int i = c0 / S < tg.nx - 1 ? c0 / S : tg.nx - 1, u = c0 - i * S;
            if (i > 0 && u < O) {                                  // O and S are multiples of 4: all four columns are in the band
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
                for (int l = 0; l < 4; ++l) { wx[0][l] = 1.0f; wx[1][l] = 0.f; }
                nxc = 1;
            }
            for (int a = 0; a < nyc; ++a) {
                for (int b = 0; b < nxc; ++b) {
                    const int64_t tl = (int64_t)(ty[a] - tg.ty0) * tg.ntx + (tx[b] - tg.tx0);
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) {
                            // col + 3 < T for every half that starts inside the frame: the four floats lie inside the tile's row
                            const float* s = x.p + tl * x.st + ch * x.sc + (int64_t)(row[a] + r * dy) * x.sh + col[b];
                            float v[4];
                            if (WIDE) {
                                const float4 f = *reinterpret_cast<const float4*>(s);
                                v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
                            } else {
#pragma unroll
                                for (int l = 0; l < 4; ++l) v[l] = (FULL || (4 * hf + l >= lo && 4 * hf + l < hi)) ? s[l] : 0.f;
                            }
#pragma unroll
                            for (int l = 0; l < 4; ++l)
                                m[r][ch][4 * hf + l] = fmaf(wy[r][a] * wx[b][l], clamp01(v[l]), m[r][ch][4 * hf + l]);
                        }
                    }
                }
            }
        }
    }
    // section 13's emit on m
    const int rows = dy + 1;
    unsigned yq[2][COLS], cq[2][4];
    float ub[2][COLS], ur[2][COLS];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int q = 0; q < COLS; ++q) emit_px(m[r][0][q], m[r][1][q], m[r][2][q], lv, k, yq[r][q], ub[r][q], ur[r][q]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool two = FULL || 2 * j + 1 < hi;                   // else the window's odd last column stands in for the one right of it
        const float b01 = two ? ub[0][2 * j + 1] : ub[0][2 * j], b11 = two ? ub[1][2 * j + 1] : ub[1][2 * j];
        const float r01 = two ? ur[0][2 * j + 1] : ur[0][2 * j], r11 = two ? ur[1][2 * j + 1] : ur[1][2 * j];
        cq[0][j] = (unsigned)emit_chroma(ub[0][2 * j], b01, ub[1][2 * j], b11, lv);
        cq[1][j] = (unsigned)emit_chroma(ur[0][2 * j], r01, ur[1][2 * j], r11, lv);
    }
    const int64_t ci = yw >> 1, cx = xw >> 1;                      // the window's chroma row, and first chroma column (xw is even)
    if (dst.y) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r < rows) {
                const int64_t base = (int64_t)(yw + r) * dst.yr + xw;
                if (FULL) {
                    unsigned w[COLS];
#pragma unroll
                    for (int q = 0; q < COLS; ++q) w[q] = yq[r][q] << SH;
                    store4(dst.y + base, w);
                    store4(dst.y + base + 4, w + 4);
                } else {
#pragma unroll
                    for (int q = 0; q < COLS; ++q)
                        if (q >= lo && q < hi) dst.y[base + q] = (T)(yq[r][q] << SH);
                }
            }
        }
        const int64_t bu = ci * dst.ur + CS * cx, bv = IL ? bu + 1 : ci * dst.vr + cx;
        T* pv = IL ? dst.u : dst.v;
        if (FULL) {
            if (IL) {
                unsigned w[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) { w[2 * j] = cq[0][j] << SH; w[2 * j + 1] = cq[1][j] << SH; }
                store4(dst.u + bu, w);
                store4(dst.u + bu + 4, w + 4);
            } else {
                unsigned w[2][4];
#pragma unroll
                for (int j = 0; j < 4; ++j) { w[0][j] = cq[0][j] << SH; w[1][j] = cq[1][j] << SH; }
                store4(dst.u + bu, w[0]);
                store4(pv + bv, w[1]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (2 * j >= lo && 2 * j < hi) { dst.u[bu + CS * j] = (T)(cq[0][j] << SH); pv[bv + CS * j] = (T)(cq[1][j] << SH); }
        }
    }
    if (HAS_REF) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r < rows) {
                const int64_t base = (int64_t)(yw + r) * ref.yr + xw;
                unsigned w[COLS];
                if (FULL) {
                    load4(ref.y + base, w);
                    load4(ref.y + base + 4, w + 4);
                } else {
#pragma unroll
                    for (int q = 0; q < COLS; ++q) w[q] = (q >= lo && q < hi) ? (unsigned)ref.y[base + q] : 0u;
                }
#pragma unroll
                for (int q = 0; q < COLS; ++q) {
                    if (FULL || (q >= lo && q < hi)) {
                        const int e = (int)yq[r][q] - (int)(w[q] >> SH);
                        su[0] += (unsigned long long)(e * e);
                    }
                }
            }
        }
        const int64_t bu = ci * ref.ur + CS * cx, bv = IL ? bu + 1 : ci * ref.vr + cx;
        const T* pv = IL ? ref.u : ref.v;
        unsigned w[2][4];
        if (FULL) {
            if (IL) {
                unsigned e[8];
                load4(ref.u + bu, e);
                load4(ref.u + bu + 4, e + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) { w[0][j] = e[2 * j]; w[1][j] = e[2 * j + 1]; }
            } else {
                load4(ref.u + bu, w[0]);
                load4(pv + bv, w[1]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in = 2 * j >= lo && 2 * j < hi;
                w[0][j] = in ? (unsigned)ref.u[bu + CS * j] : 0u;
                w[1][j] = in ? (unsigned)pv[bv + CS * j] : 0u;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (FULL || (2 * j >= lo && 2 * j < hi)) {
                const int eb = (int)cq[0][j] - (int)(w[0][j] >> SH), er = (int)cq[1][j] - (int)(w[1][j] >> SH);
                su[1] += (unsigned long long)(eb * eb);
                su[2] += (unsigned long long)(er * er);
            }
        }
    }
}

// Items are the eight-column groups, aligned in frame columns, of the WINDOW's row pairs: item -> (i, g), frame rows y0 + 2i and
// y0 + 2i + 1, frame columns X0 .. X0+7 with X0 = 8 * (x0 / 8 + g).  G groups per row pair, items = ceil(h / 2) * G.
// partials: [gridDim.x][3].
template <class T, bool IL, bool WIDE, bool HAS_REF>
__global__ __launch_bounds__(NT) void stitch_kernel(F32 x, Tiling tg, int y0, int x0, int h, int w, Planes<T> dst, Planes<const T> ref,
                                                    int G, int items, Levels lv, EmitCoef k, unsigned long long* __restrict__ partials)
{
    const int item = blockIdx.x * NT + threadIdx.x;
    unsigned long long su[3] = {0ull, 0ull, 0ull};
    if (item < items) {
        const int i = item / G, g = item - i * G;
        const int X0 = COLS * (x0 / COLS + g);
        const int lo = x0 > X0 ? x0 - X0 : 0, hi = x0 + w - X0 < COLS ? x0 + w - X0 : COLS;
        const int dy = 2 * i + 1 < h ? 1 : 0;
        if (WIDE && lo == 0 && hi == COLS)
            stitch_item<T, IL, WIDE, true, HAS_REF>(x, tg, y0 + 2 * i, dy, X0, lo, hi, 2 * i, X0 - x0, dst, ref, lv, k, su);
        else
            stitch_item<T, IL, WIDE, false, HAS_REF>(x, tg, y0 + 2 * i, dy, X0, lo, hi, 2 * i, X0 - x0, dst, ref, lv, k, su);
    }
    if (HAS_REF) block_reduce<Sum>(su, partials + (int64_t)blockIdx.x * 3);
}

// One block: the block partials in a fixed order (thread t takes t, t + NT, ...; wave tree; waves in order).
__global__ __launch_bounds__(NT) void final_kernel(const unsigned long long* __restrict__ partials, int blocks,
                                                   unsigned long long* __restrict__ sse)
{
    unsigned long long su[3] = {0ull, 0ull, 0ull};
    gather_partials<Sum>(partials, 0, blocks, (int)threadIdx.x, NT, su);
    block_reduce<Sum>(su, sse);
}

// The item space of a stitch: row pairs x the frame-aligned eight-column groups that meet [x0, x0 + w).
struct Items {
    int G, items, blocks;
};

bool items_of(int x0, int h, int w, Items& it)
{
    if (x0 < 0 || h < 1 || w < 1 || (int64_t)x0 + w > INT32_MAX) return false;
    const int64_t G = cdiv((int64_t)x0 + w, COLS) - x0 / COLS, items = cdiv(h, 2) * G;
    if (items > INT32_MAX - NT) return false;
    it.G = (int)G;
    it.items = (int)items;
    it.blocks = (int)cdiv(items, NT);
    return true;
}

// y0 and x0 even; h even or the window ends on the frame's last row; w likewise: the window's chroma samples are the frame's.
bool admissible(int H, int W, int y0, int x0, int h, int w)
{
    return y0 % 2 == 0 && x0 % 2 == 0 && (h % 2 == 0 || (int64_t)y0 + h == H) && (w % 2 == 0 || (int64_t)x0 + w == W);
}

// One plane as the wide path needs it; `back`: elements from the pointer back to the first work item's column 0.
bool plane_wide(const void* p, int64_t sr, int es, int64_t back)
{
    return (reinterpret_cast<uintptr_t>(p) / es + 4 - back % 4) % 4 == 0 && mult4(sr);
}

bool frame_wide(int fmt, const pc_ft_frame* f, int back)
{
    const int es = elem_bytes(fmt);
    if (!plane_wide(f->y, f->y_row, es, back)) return false;
    if (interleaved(fmt)) return plane_wide(f->u, f->u_row, es, back);
    return plane_wide(f->u, f->u_row, es, back / 2) && plane_wide(f->v, f->v_row, es, back / 2);
}

// The one place that decides the access path: the calls launch from it, pc_frame_tiles_plan reports it.
bool wide_path(int op, int fmt, const pc_ft_frame* frame, const void* f32, int64_t ft, int64_t fc, int64_t fh, int O, int x0,
               const pc_ft_frame* ref)
{
    if (!f32_wide(f32, ft, fc, fh)) return false;
    if (op == PC_FT_CUT) return O % 8 == 0 && frame_wide(fmt, frame, 0);
    const int back = x0 % COLS;
    return (!frame || frame_wide(fmt, frame, back)) && (!ref || frame_wide(fmt, ref, back));
}

// a frame the call may go without: all zero then
template <class T>
Planes<T> planes_or_none(const pc_ft_frame* f)
{
    return f ? planes_of<T>(f) : Planes<T>{nullptr, 0, nullptr, 0, nullptr, 0};
}

template <class T, bool IL>
void launch_cut(bool wide, dim3 grid, hipStream_t st, const pc_ft_frame* src, int H, int W, const Tiling& tg, float* dst, int G8,
                int tile_items, int64_t items, int linear, const Levels& lv, const IngestCoef& k)
{
    const Planes<const T> s = planes_of<const T>(src);
    const int Hc = (int)cdiv(H, 2), Wc = (int)cdiv(W, 2);
    if (wide)
        hipLaunchKernelGGL((cut_kernel<T, IL, true>), grid, dim3(NT), 0, st, s, H, W, Hc, Wc, tg, dst, G8, tile_items, items, linear, lv, k);
    else
        hipLaunchKernelGGL((cut_kernel<T, IL, false>), grid, dim3(NT), 0, st, s, H, W, Hc, Wc, tg, dst, G8, tile_items, items, linear, lv, k);
}

template <class T, bool IL>
void launch_stitch(bool wide, bool has_ref, dim3 grid, hipStream_t st, const F32& x, const Tiling& tg, int y0, int x0, int h, int w,
                   const pc_ft_frame* dst, const pc_ft_frame* ref, const Items& it, const Levels& lv, const EmitCoef& k,
                   unsigned long long* part)
{
    const Planes<T> d = planes_or_none<T>(dst);
    const Planes<const T> r = planes_or_none<const T>(ref);
#define PC_STITCH(WIDE, REF)                                                                                                          \
    hipLaunchKernelGGL((stitch_kernel<T, IL, WIDE, REF>), grid, dim3(NT), 0, st, x, tg, y0, x0, h, w, d, r, it.G, it.items, lv, k, part)
    if (has_ref) {
        if (wide) PC_STITCH(true, true); else PC_STITCH(false, true);
    } else {
        if (wide) PC_STITCH(true, false); else PC_STITCH(false, false);
    }
#undef PC_STITCH
}

}  // namespace

extern "C" int pc_frame_tiles_plan(int op, int fmt, const pc_ft_frame* frame, const void* f32, int64_t ft, int64_t fc, int64_t fh, int O,
                                   int x0, const pc_ft_frame* ref, int* wide)
{
    if ((op != PC_FT_CUT && op != PC_FT_STITCH) || !fmt_ok(fmt) || !f32 || !wide) return PC_ERR_ARG;
    if (op == PC_FT_CUT) {
        ref = nullptr;
        x0 = 0;
        if (O < 0) return PC_ERR_ARG;
    }
    if (x0 < 0 || x0 % 2) return PC_ERR_ARG;
    if (!frame && (op != PC_FT_STITCH || !ref)) return PC_ERR_ARG;
    for (const pc_ft_frame* f : {frame, ref})
        if (f && !planes_set(fmt, f)) return PC_ERR_ARG;
    *wide = wide_path(op, fmt, frame, f32, ft, fc, fh, O, x0, ref) ? 1 : 0;
    return PC_OK;
}

extern "C" int pc_frame_tiles_cut(const pc_ft_frame* src, int fmt, int range, int upsample, float a, float b, float c, float d, int H,
                                  int W, int T, int O, int ty0, int tx0, int nty, int ntx, float* dst, void* stream)
{
    Geo g;
    Levels lv;
    if (!geo_of(H, W, T, O, INT_MAX, g) || !rect_ok(g, ty0, tx0, nty, ntx)) return PC_ERR_ARG;
    if (!dst || !aligned(dst, 4) || !frame_ok(fmt, src, W) || !levels_of(fmt, range, lv)) return PC_ERR_ARG;
    if (!upsample_ok(upsample)) return PC_ERR_ARG;
    const int G8 = T / COLS;
    const int64_t tile_items = (int64_t)T * G8, tiles = (int64_t)nty * ntx;
    if (tile_items > INT32_MAX || tiles > INT32_MAX / 3) return PC_ERR_ARG;
    const int64_t items = tiles * tile_items, blocks = cdiv(items, NT);
    if (blocks > INT32_MAX) return PC_ERR_ARG;
    const int64_t plane = (int64_t)T * T;
    const bool wide = wide_path(PC_FT_CUT, fmt, src, dst, 3 * plane, plane, T, O, 0, nullptr);
    const Tiling tg{T, g.S, O, g.ny, g.nx, ty0, tx0, ntx};
    const IngestCoef k{a, b, c, d};
    const int linear = upsample == PC_FT_LINEAR;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks);
    if (fmt == PC_FT_NV12) launch_cut<uint8_t, true>(wide, grid, st, src, H, W, tg, dst, G8, (int)tile_items, items, linear, lv, k);
    else if (fmt == PC_FT_I420) launch_cut<uint8_t, false>(wide, grid, st, src, H, W, tg, dst, G8, (int)tile_items, items, linear, lv, k);
    else launch_cut<uint16_t, true>(wide, grid, st, src, H, W, tg, dst, G8, (int)tile_items, items, linear, lv, k);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

extern "C" size_t pc_frame_tiles_stitch_workspace_size(int x0, int h, int w)
{
    Items it;
    return items_of(x0, h, w, it) ? (size_t)it.blocks * 3 * sizeof(unsigned long long) : 0;
}

extern "C" int pc_frame_tiles_stitch(const float* x, int64_t sxt, int64_t sxc, int64_t sxh, int H, int W, int T, int O, int ty0, int tx0,
                                     int nty, int ntx, int y0, int x0, int h, int w, int fmt, int range, float kr, float kg, float kb,
                                     float ib, float ir, const pc_ft_frame* dst, const pc_ft_frame* ref, void* workspace,
                                     size_t workspace_bytes, uint64_t* sse, void* stream)
{
    Geo g;
    Items it;
    Levels lv;
    if (!geo_of(H, W, T, O, INT_MAX, g) || !rect_ok(g, ty0, tx0, nty, ntx)) return PC_ERR_ARG;
    if (!x || !aligned(x, 4) || sxh < T || sxc < 1 || sxt < 1) return PC_ERR_ARG;
    if (y0 < 0 || x0 < 0 || h < 1 || w < 1 || (int64_t)y0 + h > H || (int64_t)x0 + w > W || !items_of(x0, h, w, it)) return PC_ERR_ARG;
    if (!admissible(H, W, y0, x0, h, w)) return PC_ERR_ARG;
    // every tile that covers a pixel of the window lies in the rectangle
    if (first_tile(y0, g.S, O, g.ny) < ty0 || last_tile(y0 + h - 1, g.S, g.ny) >= ty0 + nty) return PC_ERR_ARG;
    if (first_tile(x0, g.S, O, g.nx) < tx0 || last_tile(x0 + w - 1, g.S, g.nx) >= tx0 + ntx) return PC_ERR_ARG;
    if (!fmt_ok(fmt) || !levels_of(fmt, range, lv)) return PC_ERR_ARG;
    if (!dst && !ref) return PC_ERR_ARG;
    if (dst && !frame_ok(fmt, dst, w)) return PC_ERR_ARG;
    if (ref) {
        if (!frame_ok(fmt, ref, w)) return PC_ERR_ARG;
        if (!workspace || !aligned(workspace, 8) || !sse || !aligned(sse, 8)) return PC_ERR_ARG;
        if (workspace_bytes < (size_t)it.blocks * 3 * sizeof(unsigned long long)) return PC_ERR_ARG;
    }
    const bool wide = wide_path(PC_FT_STITCH, fmt, dst, x, sxt, sxc, sxh, O, x0, ref);
    const F32 xv{x, sxt, sxc, sxh};
    const Tiling tg{T, g.S, O, g.ny, g.nx, ty0, tx0, ntx};
    const EmitCoef k{kr, kg, kb, ib, ir};
    unsigned long long* part = static_cast<unsigned long long*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)it.blocks);
    if (fmt == PC_FT_NV12) launch_stitch<uint8_t, true>(wide, ref != nullptr, grid, st, xv, tg, y0, x0, h, w, dst, ref, it, lv, k, part);
    else if (fmt == PC_FT_I420) launch_stitch<uint8_t, false>(wide, ref != nullptr, grid, st, xv, tg, y0, x0, h, w, dst, ref, it, lv, k, part);
    else launch_stitch<uint16_t, true>(wide, ref != nullptr, grid, st, xv, tg, y0, x0, h, w, dst, ref, it, lv, k, part);
    HIPCHK(hipGetLastError());
    if (ref) {
        hipLaunchKernelGGL(final_kernel, dim3(1), dim3(NT), 0, st, part, it.blocks, reinterpret_cast<unsigned long long*>(sse));
        HIPCHK(hipGetLastError());
    }
    return PC_OK;
}

extern "C" const char* pc_frame_tiles_strerror(int code)
{
    switch (code) {
    case PC_OK: return "ok";
    case PC_ERR_ARG:
        return "invalid argument, unknown format, geometry outside pc_frame_tiles.h, inadmissible window, tiles missing from the rectangle "
               "or workspace too small (pc_frame_tiles_stitch_workspace_size)";
    case PC_ERR_HIP: return "HIP runtime error";
    default: return "unknown error";
    }
}

extern "C" int pc_frame_tiles_last_hip_error(void) { return g_last_hip.load(); }

// pc_chroma_tiles.hip -- one YUV frame of any of pc_chroma.h's twelve formats and three chroma sitings <-> independent tiles of float32
// RGB planes on gfx950 (pc_chroma_tiles.h).  Definition: DESIGN.md section 23, the composition of sections 21 and 11.  Loads, levels
// and the per-pixel colour arithmetic are image_csrc/pc_yuv_device.h's, the geometry image_csrc/pc_tile_grid.h's, the reduction
// image_csrc/pc_reduce.h's, the ingest item and the format checks image_csrc/pc_chroma_items.h's.
//
// A work item is eight consecutive luma columns: of ONE tile row for the cut (aligned in tile columns; its chroma taps are chosen by
// the frame position and clamp at the frame's edges), of SY rows of the window for the stitch (a row pair at 4:2:0, one row at 4:2:2
// and 4:4:4; aligned to a multiple of 8 in FRAME columns) with the 8 / SX chroma samples of those columns.  A thread takes one item, a
// block NT consecutive items.  S = T - O is a multiple of 4, so each four-column half of a stitch item has ONE set of covering tiles
// and its tile-local column is a multiple of 4; a band edge may fall between the halves, so tiles and weights are per half and per
// column.  Rows are worked one at a time -- blend, emit_px, keep the luma codes and the row's horizontally filtered chroma
// differences, drop the floats -- and each row finds its own covering tiles: a tile origin or a band edge can fall between row 2i - 1
// and row 2i.
//
// The co-sited filter [1, 2, 1] reaches one luma column left of the item (or of the window's first column, when the window starts
// inside the item) and, vertically, one luma row above it.  The item blends those halo pixels itself, from their own covering tiles
// and weights by the same fmaf chain as the item that owns them, and passes them through the same emit_px: both hold the same bits
// and no item waits for another: no LDS, no cross-lane traffic on the data path.
//
// The access path (WIDE: four elements of a plane and four floats per access; else one by one) only changes the load and store
// instructions, never which thread handles which sample or in which order it adds.  Template parameters are what changes the shape of
// an item (element type, interleave, SX, SY, the access path, whether sums are taken and, at SY = 2, whether the row above is read);
// the depth shift, the tap weights of the cut, the horizontal siting of the stitch and its scale are wave-uniform kernel arguments.
// 24 cut kernels, 64 stitch kernels and the final.  The sums go thread, wave tree, waves in order (12 words of LDS), then final_kernel
// over the block partials, no atomics (image_csrc/pc_reduce.h).
#include "pc_image_host.h"
#include "pc_reduce.h"
#include "pc_tile_grid.h"
#include "pc_yuv_device.h"
#include "pc_yuv_items.h"
#include "pc_chroma_items.h"

#include "pc_chroma_tiles.h"

namespace {

static_assert(PC_CHT_PLANAR == LAYOUT_PLANAR && PC_CHT_SEMIPLANAR == LAYOUT_SEMIPLANAR, "pc_chroma_items.h's layouts are pc_chroma_tiles.h's");
static_assert(PC_CHT_CENTRE == SITE_CENTRE && PC_CHT_COSITED == SITE_COSITED, "pc_chroma_items.h's sitings are pc_chroma_tiles.h's");

struct Tiling {                          // the grid and the rectangle a tile set holds
    int T, S, O, ny, nx, ty0, tx0, ntx;
};

// What the stitch takes of it.  Its tile set's pointer is that of the GRID's tile (0, 0) in the rectangle's numbering -- tile (ty, tx)
// is entry ty * ntx + tx from there; only the rectangle's tiles are ever read -- and a window's frame has 32-bit row strides (the
// call refuses larger ones): two wave-uniform values less per tile set and three per frame, which is what keeps the widest
// instantiations clear of the scalar register file's end.
struct Tiles {
    int S, O, ny, nx, ntx;
};

template <class T>
struct Rows {                            // Planes with 32-bit row strides
    T* y;
    T* u;
    T* v;
    int yr, ur, vr;
};

// The stitch's siting: co-sited along x (0 where the axis is not subsampled), s = 1 / (scale_h * scale_v), and the depth shift.  The
// vertical siting chooses the kernel (its template parameter VCO) on the host.
struct Site {
    int hco;
    float s;
    int sh;
};

// -- cut -----------------------------------------------------------------------------------------------------------------------------

// Items are the eight-column groups of the tiles' rows: item -> (tile t of the rectangle, row r, group g), tile columns 8g .. 8g+7.
// G8 = T / 8, tile_items = T * G8, items = nty * ntx * tile_items.  The chroma taps are clamped at the FRAME's edges Hc - 1, Wc - 1.
// WIDE needs S a multiple of 8 at SX = 2 (X is then one, and X / 2 a multiple of 4); at SX = 1 S is a multiple of 4, which is enough.
template <class T, bool IL, int SX, int SY, bool WIDE>
__global__ __launch_bounds__(NT) void cut_kernel(Planes<const T> s, int H, int W, int Hc, int Wc, Tiling tg, float* __restrict__ dst, int G8,
                                                 int tile_items, int64_t items, Taps t, Levels lv, IngestCoef k)
{
    const int64_t item = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (item >= items) return;
    const int tl = (int)(item / tile_items), rem = (int)(item - (int64_t)tl * tile_items);
    const int r = rem / G8, g = rem - r * G8;
    const int ta = tl / tg.ntx, tb = tl - ta * tg.ntx;
    const int64_t Y64 = (int64_t)(tg.ty0 + ta) * tg.S + r, X64 = (int64_t)(tg.tx0 + tb) * tg.S + COLS * g;      // frame coordinates
    float o[3][COLS];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < COLS; ++i) o[c][i] = 0.f;
    if (Y64 < H && X64 < W) ingest_item<T, IL, SX, SY, WIDE>(s, W, Hc, Wc, (int)Y64, (int)X64, t, lv, k, o);
    const int64_t plane = (int64_t)tg.T * tg.T;
#pragma unroll
    for (int c = 0; c < 3; ++c) store8<WIDE>(dst + ((int64_t)tl * 3 + c) * plane + (int64_t)r * tg.T + COLS * g, o[c], COLS);
}

// -- stitch --------------------------------------------------------------------------------------------------------------------------

// num / den for two small integers as the correctly rounded float32 quotient: both are exact floats (at most 2 O <= T), and the
// float32 division is one IEEE operation, as in to_rgb.  pc_frame_tiles.hip and pc_tiles.hip round the double quotient instead (53 >=
// 2 * 24 + 2 bits: one rounding of the exact quotient as well); the bits are the same, the register pairs are not needed here.
__device__ __forceinline__ float quotient(int num, int den) { return (float)num / (float)den; }

// The tiles of an axis of n that cover coordinate c, ascending: tile index t[], the coordinate inside each p[], how many.  In a band
// (two tiles) u is the coordinate inside the later one.
struct Cover {
    int t[2], p[2], n, u;
};

__device__ __forceinline__ Cover cover_of(int c, int S, int O, int n)
{
    Cover cv;
    const int i = c / S < n - 1 ? c / S : n - 1, u = c - i * S;
    cv.u = u;
    if (i > 0 && u < O) {
        cv.t[0] = i - 1; cv.p[0] = u + S;
        cv.t[1] = i;     cv.p[1] = u;
        cv.n = 2;
    } else {
        cv.t[0] = i; cv.p[0] = u;
        cv.t[1] = i; cv.p[1] = u;
        cv.n = 1;
    }
    return cv;
}

// the weight of the earlier (a = 0) and of the later (a = 1) tile of a band at coordinate u inside the later one
__device__ __forceinline__ float band_weight(int a, int u, int O) { return a ? quotient(2 * u + 1, 2 * O) : quotient(2 * (O - 1 - u) + 1, 2 * O); }

// m of frame row Y at the frame columns X0 + q, lb <= q < hi (the other lanes: +0.0f, or on the wide path whatever their half's tiles
// hold there; nobody reads them).  FULL: every lane.
template <bool WIDE, bool FULL>
__device__ __forceinline__ void blend_row(const F32& x, const Tiles& tg, int Y, int X0, int lb, int hi, float (&m)[3][COLS])
{
    const int S = tg.S, O = tg.O;
    const Cover cy = cover_of(Y, S, O, tg.ny);
    float wy[2] = {1.0f, 0.f};
    if (cy.n == 2) { wy[0] = band_weight(0, cy.u, O); wy[1] = band_weight(1, cy.u, O); }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
#pragma unroll
        for (int q = 0; q < COLS; ++q) m[ch][q] = 0.f;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        if (FULL || (lb < 4 * hf + 4 && hi > 4 * hf)) {            // the half holds a pixel that is wanted: it starts inside the frame
            const Cover cx = cover_of(X0 + 4 * hf, S, O, tg.nx);   // O and S are multiples of 4: all four columns share the tiles
            float wx[2][4];
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                wx[0][l] = cx.n == 2 ? band_weight(0, cx.u + l, O) : 1.0f;
                wx[1][l] = cx.n == 2 ? band_weight(1, cx.u + l, O) : 0.f;
            }
#pragma unroll
            for (int a = 0; a < 2; ++a) {
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    if (a >= cy.n || b >= cx.n) continue;          // unrolled and predicated: every index is a constant
                    const int64_t tl = (int64_t)cy.t[a] * tg.ntx + cx.t[b];
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        // p + 3 < T for every half that starts inside the frame: the four floats lie inside the tile's row
                        const float* s = x.p + tl * x.st + ch * x.sc + (int64_t)cy.p[a] * x.sh + cx.p[b];
                        float v[4];
                        if (WIDE) {
                            const float4 f = *reinterpret_cast<const float4*>(s);
                            v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
                        } else {
#pragma unroll
                            for (int l = 0; l < 4; ++l) v[l] = (FULL || (4 * hf + l >= lb && 4 * hf + l < hi)) ? s[l] : 0.f;
                        }
#pragma unroll
                        for (int l = 0; l < 4; ++l) m[ch][4 * hf + l] = fmaf(wy[a] * wx[b][l], clamp01(v[l]), m[ch][4 * hf + l]);
                    }
                }
            }
        }
    }
}

// m of ONE frame pixel (a halo pixel): its own covering tiles and weights, the chain of blend_row on the same inputs.
__device__ __forceinline__ void blend_px(const F32& x, const Tiles& tg, int Y, int X, float (&m)[3])
{
    const int S = tg.S, O = tg.O;
    const Cover cy = cover_of(Y, S, O, tg.ny), cx = cover_of(X, S, O, tg.nx);
    float wy[2] = {1.0f, 0.f}, wx[2] = {1.0f, 0.f};
    if (cy.n == 2) { wy[0] = band_weight(0, cy.u, O); wy[1] = band_weight(1, cy.u, O); }
    if (cx.n == 2) { wx[0] = band_weight(0, cx.u, O); wx[1] = band_weight(1, cx.u, O); }
    m[0] = m[1] = m[2] = 0.f;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            if (a >= cy.n || b >= cx.n) continue;
            const int64_t tl = (int64_t)cy.t[a] * tg.ntx + cx.t[b];
            const float* s = x.p + tl * x.st + (int64_t)cy.p[a] * x.sh + cx.p[b];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) m[ch] = fmaf(wy[a] * wx[b], clamp01(s[ch * x.sc]), m[ch]);
        }
    }
}

// One luma row of an item: frame row Y, frame columns X0 .. X0+7 of which the lanes lo .. hi-1 lie in the window -> their luma codes
// (written to dy and compared with ry where the item owns the row and the pointers are set; both point at lane 0) and the row's
// horizontally filtered chroma differences h[Cb, Cr][8 / SX].  The filter's indices clamp at the FRAME's edges: a lane right of hi - 1
// that a sample of the window needs lies beyond the frame (the window is admissible), and the last column stands in for it; the
// co-sited filter's column left of a sample is lane 2j - 1 (blended here even where it lies left of the window), the halo pixel
// X0 - 1 for the item's first sample, and column 0 itself at the frame's left edge.
template <class T, int SX, bool WIDE, bool FULL, bool HAS_REF>
__device__ __forceinline__ void stitch_row(const F32& x, const Tiles& tg, int Y, int X0, int lo, int hi, bool own, T* dy, const T* ry,
                                           const Site& st, const Levels& lv, const EmitCoef& k, float (&h)[2][COLS / SX], u64& su)
{
    unsigned yq[COLS];
    float ub[COLS], ur[COLS];
    {
        float m[3][COLS];
        blend_row<WIDE, FULL>(x, tg, Y, X0, (SX == 2 && st.hco && lo > 0) ? lo - 1 : lo, hi, m);
#pragma unroll
        for (int q = 0; q < COLS; ++q) emit_px(m[0][q], m[1][q], m[2][q], lv, k, yq[q], ub[q], ur[q]);
    }
    if (SX == 1) {
#pragma unroll
        for (int q = 0; q < COLS; ++q) { h[0][q] = ub[q]; h[1][q] = ur[q]; }
    } else if (st.hco) {
        float bl = ub[0], rl = ur[0];                             // frame column 0 stands in for the one left of it
        if (X0 > 0 && lo == 0) {
            float px[3];
            unsigned yl;
            blend_px(x, tg, Y, X0 - 1, px);
            emit_px(px[0], px[1], px[2], lv, k, yl, bl, rl);
        }
#pragma unroll
        for (int j = 0; j < COLS / 2; ++j) {
            const bool two = FULL || 2 * j + 1 < hi;
            const float cb = two ? ub[2 * j + 1] : ub[2 * j], cr = two ? ur[2 * j + 1] : ur[2 * j];
            h[0][j] = ((j ? ub[2 * j - 1] : bl) + cb) + (ub[2 * j] + ub[2 * j]);
            h[1][j] = ((j ? ur[2 * j - 1] : rl) + cr) + (ur[2 * j] + ur[2 * j]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < COLS / 2; ++j) {
            const bool two = FULL || 2 * j + 1 < hi;
            h[0][j] = ub[2 * j] + (two ? ub[2 * j + 1] : ub[2 * j]);
            h[1][j] = ur[2 * j] + (two ? ur[2 * j + 1] : ur[2 * j]);
        }
    }
    if (!own) return;
    if (dy) {
        if (FULL) {
            unsigned w[COLS];
#pragma unroll
            for (int q = 0; q < COLS; ++q) w[q] = word_of<T>(yq[q], st.sh);
            store4(dy, w);
            store4(dy + 4, w + 4);
        } else {
#pragma unroll
            for (int q = 0; q < COLS; ++q)
                if (q >= lo && q < hi) dy[q] = (T)word_of<T>(yq[q], st.sh);
        }
    }
    if (HAS_REF) {
        unsigned w[COLS];
        if (FULL) {
            load4(ry, w);
            load4(ry + 4, w + 4);
        } else {
#pragma unroll
            for (int q = 0; q < COLS; ++q) w[q] = (q >= lo && q < hi) ? (unsigned)ry[q] : 0u;
        }
#pragma unroll
        for (int q = 0; q < COLS; ++q) {
            if (FULL || (q >= lo && q < hi)) {
                const int e = (int)yq[q] - (int)code_of<T>(w[q], st.sh, (unsigned)lv.maxv);
                su += (u64)(e * e);
            }
        }
    }
}

// One item of the stitch: frame rows Y0 .. Y0 + SY - 1 (the last may be missing at the frame's odd last row), frame columns
// X0 .. X0+7 of which the lanes lo .. hi-1 lie in the window (lo a multiple of SX); yw, xw: the first row and column relative to the
// window (xw may be negative, down to -7).  FULL: lo == 0, hi == 8 and every access is wide; else plane accesses go element by
// element.  The whole item is compiled twice, so that the two kinds of access never meet in one basic block.
template <class T, bool IL, int SX, int SY, bool VCO, bool WIDE, bool FULL, bool HAS_REF>
__device__ __forceinline__ void stitch_item(const F32& x, const Tiles& tg, int H, int Y0, int X0, int lo, int hi, int yw, int xw,
                                            const Rows<T>& dst, const Rows<const T>& ref, const Site& st, const Levels& lv,
                                            const EmitCoef& k, u64 su[3])
{
    constexpr int CS = IL ? 2 : 1;
    constexpr int NC = COLS / SX;                                 // chroma samples of the item
    float v[2][NC];
    // every address of the item up front, as the thread's own values: the two frame records are not needed after this
    const int64_t ci = SY == 2 ? yw >> 1 : yw, cx = SX == 2 ? xw >> 1 : xw;   // the window's chroma row and first chroma column
    T* py[2] = {nullptr, nullptr};                                // lane 0 of the item's luma rows in dst, in ref
    const T* pr[2] = {nullptr, nullptr};
    T* du = nullptr;
    T* dv = nullptr;
    const T* ru = nullptr;
    const T* rv = nullptr;
    if (dst.y) {
        py[0] = dst.y + (int64_t)yw * dst.yr + xw;
        py[1] = py[0] + dst.yr;
        du = dst.u + ci * dst.ur + CS * cx;
        dv = IL ? du + 1 : dst.v + ci * dst.vr + cx;
    }
    if (HAS_REF) {
        pr[0] = ref.y + (int64_t)yw * ref.yr + xw;
        pr[1] = pr[0] + ref.yr;
        ru = ref.u + ci * ref.ur + CS * cx;
        rv = IL ? ru + 1 : ref.v + ci * ref.vr + cx;
    }
    if (SY == 1) {
        stitch_row<T, SX, WIDE, FULL, HAS_REF>(x, tg, Y0, X0, lo, hi, true, py[0], pr[0], st, lv, k, v, su[0]);
    } else {
        // A row at a time (blend, emit_px, keep the codes and the h values, drop the floats), in the order the vertical rule adds
        // them: the row above (a, co-sited only; row 0 itself at the frame's top edge), the row below (c; the frame's last row stands
        // in for a missing one), then the item's first row (b): (a + c) + (b + b), or b + c.
        const bool second = Y0 + 1 < H;
        float acc[2][NC], t[2][NC];
        if (VCO) {
            stitch_row<T, SX, WIDE, FULL, false>(x, tg, max(Y0 - 1, 0), X0, lo, hi, false, nullptr, nullptr, st, lv, k, acc, su[0]);
            stitch_row<T, SX, WIDE, FULL, HAS_REF>(x, tg, second ? Y0 + 1 : Y0, X0, lo, hi, second, py[1], pr[1], st, lv, k, t, su[0]);
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int j = 0; j < NC; ++j) acc[p][j] = acc[p][j] + t[p][j];
        } else {
            stitch_row<T, SX, WIDE, FULL, HAS_REF>(x, tg, second ? Y0 + 1 : Y0, X0, lo, hi, second, py[1], pr[1], st, lv, k, acc, su[0]);
        }
        stitch_row<T, SX, WIDE, FULL, HAS_REF>(x, tg, Y0, X0, lo, hi, true, py[0], pr[0], st, lv, k, t, su[0]);
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int j = 0; j < NC; ++j) v[p][j] = VCO ? acc[p][j] + (t[p][j] + t[p][j]) : t[p][j] + acc[p][j];
    }
    unsigned cq[2][NC];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int j = 0; j < NC; ++j) cq[p][j] = (unsigned)clampi((int)rintf(v[p][j] * st.s + (float)lv.co), 0, lv.maxv);
    if (du) {
        if (FULL) {
            if (IL) {
                unsigned w[2 * NC];
#pragma unroll
                for (int j = 0; j < NC; ++j) { w[2 * j] = word_of<T>(cq[0][j], st.sh); w[2 * j + 1] = word_of<T>(cq[1][j], st.sh); }
#pragma unroll
                for (int m = 0; m < 2 * NC; m += 4) store4(du + m, w + m);
            } else {
                unsigned w[2][NC];
#pragma unroll
                for (int j = 0; j < NC; ++j) { w[0][j] = word_of<T>(cq[0][j], st.sh); w[1][j] = word_of<T>(cq[1][j], st.sh); }
#pragma unroll
                for (int m = 0; m < NC; m += 4) { store4(du + m, w[0] + m); store4(dv + m, w[1] + m); }
            }
        } else {
#pragma unroll
            for (int j = 0; j < NC; ++j)
                if (SX * j >= lo && SX * j < hi) { du[CS * j] = (T)word_of<T>(cq[0][j], st.sh); dv[CS * j] = (T)word_of<T>(cq[1][j], st.sh); }
        }
    }
    if (HAS_REF) {
        unsigned w[2][NC];
        if (FULL) {
            if (IL) {
                unsigned e[2 * NC];
#pragma unroll
                for (int m = 0; m < 2 * NC; m += 4) load4(ru + m, e + m);
#pragma unroll
                for (int j = 0; j < NC; ++j) { w[0][j] = e[2 * j]; w[1][j] = e[2 * j + 1]; }
            } else {
#pragma unroll
                for (int m = 0; m < NC; m += 4) { load4(ru + m, w[0] + m); load4(rv + m, w[1] + m); }
            }
        } else {
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const bool in = SX * j >= lo && SX * j < hi;
                w[0][j] = in ? (unsigned)ru[CS * j] : 0u;
                w[1][j] = in ? (unsigned)rv[CS * j] : 0u;
            }
        }
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            if (FULL || (SX * j >= lo && SX * j < hi)) {
                const int eb = (int)cq[0][j] - (int)code_of<T>(w[0][j], st.sh, (unsigned)lv.maxv);
                const int er = (int)cq[1][j] - (int)code_of<T>(w[1][j], st.sh, (unsigned)lv.maxv);
                su[1] += (u64)(eb * eb);
                su[2] += (u64)(er * er);
            }
        }
    }
}

// Items are the eight-column groups, aligned in frame columns, of the WINDOW's chroma rows: item -> (i, g), frame rows y0 + SY i ..,
// frame columns X0 .. X0+7 with X0 = 8 * (x0 / 8 + g).  G groups per chroma row, items = ceil(h / SY) * G.  partials: [gridDim.x][3].
template <class T, bool IL, int SX, int SY, bool VCO, bool WIDE, bool HAS_REF>
__global__ __launch_bounds__(NT) void stitch_kernel(F32 x, Tiles tg, int H, int y0, int x0, int w, Rows<T> dst, Rows<const T> ref, int G,
                                                    int items, Site st, Levels lv, EmitCoef k, u64* __restrict__ partials)
{
    const int item = blockIdx.x * NT + threadIdx.x;
    u64 su[3] = {0ull, 0ull, 0ull};
    if (item < items) {
        const int i = item / G, g = item - i * G;
        const int X0 = COLS * (x0 / COLS + g);
        const int lo = x0 > X0 ? x0 - X0 : 0, hi = x0 + w - X0 < COLS ? x0 + w - X0 : COLS;
        if (WIDE && lo == 0 && hi == COLS)
            stitch_item<T, IL, SX, SY, VCO, WIDE, true, HAS_REF>(x, tg, H, y0 + SY * i, X0, lo, hi, SY * i, X0 - x0, dst, ref, st, lv, k, su);
        else
            stitch_item<T, IL, SX, SY, VCO, WIDE, false, HAS_REF>(x, tg, H, y0 + SY * i, X0, lo, hi, SY * i, X0 - x0, dst, ref, st, lv, k, su);
    }
    if (HAS_REF) block_reduce<Sum>(su, partials + (int64_t)blockIdx.x * 3);
}

// One block: the block partials in a fixed order (thread t takes t, t + NT, ...; wave tree; waves in order).
__global__ __launch_bounds__(NT) void final_kernel(const u64* __restrict__ partials, int blocks, u64* __restrict__ sse)
{
    u64 su[3] = {0ull, 0ull, 0ull};
    gather_partials<Sum>(partials, 0, blocks, (int)threadIdx.x, NT, su);
    block_reduce<Sum>(su, sse);
}

// -- host ----------------------------------------------------------------------------------------------------------------------------

// The item space of a stitch: chroma rows x the frame-aligned eight-column groups that meet [x0, x0 + w).
struct Items {
    int G, items, blocks;
};

bool items_of(int x0, int h, int w, int sy, Items& it)
{
    if (x0 < 0 || h < 1 || w < 1 || (sy != 1 && sy != 2) || (int64_t)x0 + w > INT32_MAX) return false;
    const int64_t G = cdiv((int64_t)x0 + w, COLS) - x0 / COLS, items = cdiv(h, sy) * G;
    if (items > INT32_MAX - NT) return false;
    it.G = (int)G;
    it.items = (int)items;
    it.blocks = (int)cdiv(items, NT);
    return true;
}

// y0 % sy == 0 and x0 % sx == 0; h % sy == 0 or the window ends on the frame's last row; w likewise: the window's chroma samples are
// the frame's.
bool admissible(int H, int W, int sx, int sy, int y0, int x0, int h, int w)
{
    return y0 % sy == 0 && x0 % sx == 0 && (h % sy == 0 || (int64_t)y0 + h == H) && (w % sx == 0 || (int64_t)x0 + w == W);
}

// One plane as the wide path needs it when the first work item's column 0 lies `back` elements before the pointer.
bool plane_wide_back(const void* p, int64_t sr, int es, int64_t back)
{
    return plane_wide(reinterpret_cast<const char*>(p) - (back % 4) * es, sr, es);
}

// back: luma columns from the first item's column 0 to the frame's first sample (0 for the cut, x0 % 8 for the stitch)
bool picture_wide(bool il, int es, int sx, const pc_cht_frame* f, int back)
{
    if (!plane_wide_back(f->y, f->y_row, es, back)) return false;
    if (il) return plane_wide_back(f->u, f->u_row, es, 2 * back / sx);
    return plane_wide_back(f->u, f->u_row, es, back / sx) && plane_wide_back(f->v, f->v_row, es, back / sx);
}

// The one place that decides the access path: the calls launch from it, pc_chroma_tiles_plan reports it.
bool wide_path(int op, bool il, int es, int sx, const pc_cht_frame* frame, const void* f32, int64_t ft, int64_t fc, int64_t fh, int O, int x0,
               const pc_cht_frame* ref)
{
    if (!f32_wide(f32, ft, fc, fh)) return false;
    if (op == PC_CHT_CUT) return (sx == 1 || O % 8 == 0) && picture_wide(il, es, sx, frame, 0);
    const int back = x0 % COLS;
    return (!frame || picture_wide(il, es, sx, frame, back)) && (!ref || picture_wide(il, es, sx, ref, back));
}

// a frame the stitch may go without: all zero then
template <class T>
Rows<T> rows_or_none(const pc_cht_frame* f)
{
    if (!f) return Rows<T>{nullptr, nullptr, nullptr, 0, 0, 0};
    return Rows<T>{static_cast<T*>(f->y), static_cast<T*>(f->u), static_cast<T*>(f->v), (int)f->y_row, (int)f->u_row, (int)f->v_row};
}

// the row strides the stitch reads fit 32 bits
bool rows_fit(bool il, const pc_cht_frame* f) { return f->y_row <= INT32_MAX && f->u_row <= INT32_MAX && (il || f->v_row <= INT32_MAX); }

}  // namespace

extern "C" int pc_chroma_tiles_plan(int op, int layout, int bits, int sx, const pc_cht_frame* frame, const void* f32, int64_t ft, int64_t fc,
                                    int64_t fh, int O, int x0, const pc_cht_frame* ref, int* wide)
{
    Fmt fm;
    if ((op != PC_CHT_CUT && op != PC_CHT_STITCH) || !format_of(layout, bits, 0, sx, 1, fm) || !f32 || !wide) return PC_ERR_ARG;
    if (op == PC_CHT_CUT) {
        ref = nullptr;
        x0 = 0;
        if (O < 0) return PC_ERR_ARG;
    }
    if (x0 < 0 || x0 % sx) return PC_ERR_ARG;
    if (!frame && (op != PC_CHT_STITCH || !ref)) return PC_ERR_ARG;
    for (const pc_cht_frame* f : {frame, ref})
        if (f && !(f->y && f->u && (fm.il || f->v))) return PC_ERR_ARG;
    *wide = wide_path(op, fm.il, bits == 10 ? 2 : 1, sx, frame, f32, ft, fc, fh, O, x0, ref) ? 1 : 0;
    return PC_OK;
}

extern "C" int pc_chroma_tiles_cut(const pc_cht_frame* src, int layout, int bits, int shift, int sx, int sy, int hsite, int vsite, int range,
                                   int upsample, float a, float b, float c, float d, int H, int W, int T, int O, int ty0, int tx0, int nty,
                                   int ntx, float* dst, void* stream)
{
    Geo g;
    Levels lv;
    Fmt fm;
    if (!geo_of(H, W, T, O, INT_MAX, g) || !rect_ok(g, ty0, tx0, nty, ntx)) return PC_ERR_ARG;
    if (!format_of(layout, bits, shift, sx, sy, fm) || !site_ok(hsite) || !site_ok(vsite) || !upsample_ok(upsample)) return PC_ERR_ARG;
    if (!dst || !aligned(dst, 4) || !picture_ok(fm, src, W) || !depth_levels(bits, range, lv)) return PC_ERR_ARG;
    const int G8 = T / COLS;
    const int64_t tile_items = (int64_t)T * G8, tiles = (int64_t)nty * ntx;
    if (tile_items > INT32_MAX || tiles > INT32_MAX / 3) return PC_ERR_ARG;
    const int64_t items = tiles * tile_items, blocks = cdiv(items, NT);
    if (blocks > INT32_MAX) return PC_ERR_ARG;
    const int64_t plane = (int64_t)T * T;
    const bool wide = wide_path(PC_CHT_CUT, fm.il, bits == 10 ? 2 : 1, sx, src, dst, 3 * plane, plane, T, O, 0, nullptr);
    const Tiling tg{T, g.S, O, g.ny, g.nx, ty0, tx0, ntx};
    const IngestCoef k{a, b, c, d};
    const Taps t = taps_of(sx, sy, hsite, vsite, upsample == PC_CHT_LINEAR, shift);
    const int Hc = (int)cdiv(H, sy), Wc = (int)cdiv(W, sx);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks);
    with_format(fm, [&](auto el, auto il, auto SX, auto SY) {
        using T_ = decltype(el);
        const Planes<const T_> s = planes_of<const T_>(src);
        if (wide)
            hipLaunchKernelGGL((cut_kernel<T_, il.value, SX.value, SY.value, true>), grid, dim3(NT), 0, st, s, H, W, Hc, Wc, tg, dst, G8,
                               (int)tile_items, items, t, lv, k);
        else
            hipLaunchKernelGGL((cut_kernel<T_, il.value, SX.value, SY.value, false>), grid, dim3(NT), 0, st, s, H, W, Hc, Wc, tg, dst, G8,
                               (int)tile_items, items, t, lv, k);
    });
    HIPCHK(hipGetLastError());
    return PC_OK;
}

extern "C" size_t pc_chroma_tiles_stitch_workspace_size(int x0, int h, int w, int sy)
{
    Items it;
    return items_of(x0, h, w, sy, it) ? (size_t)it.blocks * 3 * sizeof(u64) : 0;
}

extern "C" int pc_chroma_tiles_stitch(const float* x, int64_t sxt, int64_t sxc, int64_t sxh, int H, int W, int T, int O, int ty0, int tx0,
                                      int nty, int ntx, int y0, int x0, int h, int w, int layout, int bits, int shift, int sx, int sy,
                                      int hsite, int vsite, int range, float kr, float kg, float kb, float ib, float ir,
                                      const pc_cht_frame* dst, const pc_cht_frame* ref, void* workspace, size_t workspace_bytes,
                                      uint64_t* sse, void* stream)
{
    Geo g;
    Items it;
    Levels lv;
    Fmt fm;
    if (!geo_of(H, W, T, O, INT_MAX, g) || !rect_ok(g, ty0, tx0, nty, ntx)) return PC_ERR_ARG;
    if (!x || !aligned(x, 4) || sxh < T || sxc < 1 || sxt < 1) return PC_ERR_ARG;
    if (!format_of(layout, bits, shift, sx, sy, fm) || !site_ok(hsite) || !site_ok(vsite) || !depth_levels(bits, range, lv)) return PC_ERR_ARG;
    if (y0 < 0 || x0 < 0 || h < 1 || w < 1 || (int64_t)y0 + h > H || (int64_t)x0 + w > W || !items_of(x0, h, w, sy, it)) return PC_ERR_ARG;
    if (!admissible(H, W, sx, sy, y0, x0, h, w)) return PC_ERR_ARG;
    const bool hco = sx == 2 && hsite == PC_CHT_COSITED, vco = sy == 2 && vsite == PC_CHT_COSITED;
    // every tile that covers a pixel of the window extended by its halo lies in the rectangle
    const int ya = vco && y0 > 0 ? y0 - 1 : y0, xa = hco && x0 > 0 ? x0 - 1 : x0;
    if (first_tile(ya, g.S, O, g.ny) < ty0 || last_tile(y0 + h - 1, g.S, g.ny) >= ty0 + nty) return PC_ERR_ARG;
    if (first_tile(xa, g.S, O, g.nx) < tx0 || last_tile(x0 + w - 1, g.S, g.nx) >= tx0 + ntx) return PC_ERR_ARG;
    if (!dst && !ref) return PC_ERR_ARG;
    if (dst && !(picture_ok(fm, dst, w) && rows_fit(fm.il, dst))) return PC_ERR_ARG;
    if (ref) {
        if (!picture_ok(fm, ref, w) || !rows_fit(fm.il, ref)) return PC_ERR_ARG;
        if (!workspace || !aligned(workspace, 8) || !sse || !aligned(sse, 8)) return PC_ERR_ARG;
        if (workspace_bytes < (size_t)it.blocks * 3 * sizeof(u64)) return PC_ERR_ARG;
    }
    const bool wide = wide_path(PC_CHT_STITCH, fm.il, bits == 10 ? 2 : 1, sx, dst, x, sxt, sxc, sxh, O, x0, ref);
    // the tile set seen from the grid's tile (0, 0); the address is formed in integers, nothing is read before the rectangle
    const intptr_t origin = reinterpret_cast<intptr_t>(x) - (intptr_t)(((int64_t)ty0 * ntx + tx0) * sxt * (int64_t)sizeof(float));
    const F32 xv{reinterpret_cast<const float*>(origin), sxt, sxc, sxh};
    const Tiles tg{g.S, O, g.ny, g.nx, ntx};
    const EmitCoef k{kr, kg, kb, ib, ir};
    const Site site{hco ? 1 : 0, 1.f / (float)((sx == 2 ? (hco ? 4 : 2) : 1) * (sy == 2 ? (vco ? 4 : 2) : 1)), shift};
    u64* part = static_cast<u64*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)it.blocks);
    with_format(fm, [&](auto el, auto il, auto SX, auto SY) {
        using T_ = decltype(el);
        const Rows<T_> d = rows_or_none<T_>(dst);
        const Rows<const T_> r = rows_or_none<const T_>(ref);
#define PC_STITCH(VCO, WIDE, REF)                                                                                                          \
    hipLaunchKernelGGL((stitch_kernel<T_, il.value, SX.value, SY.value, VCO, WIDE, REF>), grid, dim3(NT), 0, st, xv, tg, H, y0, x0, w, d, r, \
                       it.G, it.items, site, lv, k, part)
    // VCO is instantiated for SY = 2 alone: at SY = 1 both branches below name the same kernel
#define PC_STITCH_V(WIDE, REF)                                                                                                             \
    do {                                                                                                                                   \
        if (SY.value == 2 && vco) PC_STITCH((SY.value == 2), WIDE, REF); else PC_STITCH(false, WIDE, REF);                                 \
    } while (0)
        if (ref) {
            if (wide) PC_STITCH_V(true, true); else PC_STITCH_V(false, true);
        } else {
            if (wide) PC_STITCH_V(true, false); else PC_STITCH_V(false, false);
        }
#undef PC_STITCH_V
#undef PC_STITCH
    });
    HIPCHK(hipGetLastError());
    if (ref) {
        hipLaunchKernelGGL(final_kernel, dim3(1), dim3(NT), 0, st, part, it.blocks, reinterpret_cast<u64*>(sse));
        HIPCHK(hipGetLastError());
    }
    return PC_OK;
}

extern "C" const char* pc_chroma_tiles_strerror(int code)
{
    switch (code) {
    case PC_OK: return "ok";
    case PC_ERR_ARG:
        return "invalid argument, unknown layout, depth, shift, subsampling, siting, range or upsampler, geometry outside pc_chroma_tiles.h, "
               "inadmissible window, tiles missing from the rectangle (the halo of a co-sited axis included) or workspace too small "
               "(pc_chroma_tiles_stitch_workspace_size)";
    case PC_ERR_HIP: return "HIP runtime error";
    default: return "unknown error";
    }
}

extern "C" int pc_chroma_tiles_last_hip_error(void) { return g_last_hip.load(); }

// pc_chroma_rate.hip -- the per-tile, per-plane weighted squared error of decoded float tiles against the original YUV frame in any
// of pc_chroma.h's twelve formats and three chroma sitings, in the frame's own codes, on gfx950 (pc_chroma_rate.h).  Definition:
// DESIGN.md section 24, the composition of sections 21 (the emit), 11 (geometry) and 12 (integer band weights).  Loads, levels and
// the per-pixel colour arithmetic are image_csrc/pc_yuv_device.h's, the geometry and the band numerators image_csrc/pc_tile_grid.h's,
// the reduction image_csrc/pc_reduce.h's, the code of an element and the format checks image_csrc/pc_chroma_items.h's.
//
// A work item is SY rows of one tile (a row pair at 4:2:0, one row at 4:2:2 and 4:4:4) by eight tile-aligned columns, with the
// 8 / SX chroma samples of those columns.  A thread takes one item, a block NT consecutive items of ONE tile (T * T / (8 SY) is a
// multiple of 256 for every T that is a multiple of 64: no block straddles two tiles and none has a tail).  S is a multiple of 4, so
// a tile's chroma cells are the frame's.  Rows are worked one at a time -- load, emit_px, compare and weigh the luma codes, keep the
// row's horizontally filtered chroma differences, drop the floats.
//
// The co-sited filter [1, 2, 1] reaches one tile column left of the item and, vertically, one tile row above it.  The item computes
// the halo pixel itself from tile column max(q0 - 1, 0) and, under VCO, takes the halo row max(r0 - 1, 0) through the same code as a
// third row: the thread that owns those pixels holds the same bits, and no item waits for another.  Every clamp is at the tile's
// in-frame part: a tile never reads another tile.
//
// An item whose rows and columns all lie inside the frame and whose accesses are all wide is compiled on its own (FULL); every other
// item goes element by element.  The access path only changes the load instructions, never which thread holds which sample or in
// which order it adds: the sums are the same bits on both.  Template parameters are what changes the shape of an item (element type,
// interleave, SX, SY, whether the row above is read, the access path); the depth shift, the horizontal siting and the scale are
// wave-uniform kernel arguments.  32 sse kernels and the final.  Everything that is added is an integer: a thread's sums, the wave
// tree, the waves of a block in order, then final_kernel over a tile's block partials (image_csrc/pc_reduce.h).
#include "pc_image_host.h"
#include "pc_reduce.h"
#include "pc_tile_grid.h"
#include "pc_yuv_device.h"
#include "pc_chroma_items.h"

#include "pc_chroma_rate.h"

namespace {

static_assert(PC_CHR_PLANAR == LAYOUT_PLANAR && PC_CHR_SEMIPLANAR == LAYOUT_SEMIPLANAR, "pc_chroma_items.h's layouts are pc_chroma_rate.h's");
static_assert(PC_CHR_CENTRE == SITE_CENTRE && PC_CHR_COSITED == SITE_COSITED, "pc_chroma_items.h's sitings are pc_chroma_rate.h's");

constexpr int T_MAX8 = 2048;             // T^4 * 255^2 < 2^60
constexpr int T_MAX10 = 1024;            // T^4 * 1023^2 < 2^60

struct RangeGrid : Grid {                // the frame, the grid and the linear range of the call
    int first_tile;
};

// What the measurement takes of the siting and the depth: co-sited along x (0 where the axis is not subsampled), s = 1 / (scale_h *
// scale_v), and the depth shift.  The vertical siting chooses the kernel (its template parameter VCO) on the host.
struct Measure {
    int hco;
    float s;
    int sh;
};

// One row of an item: the floats of tile columns q0 .. q0+7 at xr (channel stride sc; xr is column 0 of the tile's row), of which
// the lanes 0 .. hi-1 lie inside the frame -> the row's horizontally filtered chroma differences h[Cb, Cr][8 / SX] and, where the
// item owns the row (ry: lane 0 of the original's luma row), its weighted luma error ay * sum ax(q) e^2 into su.  A column right of
// hi - 1 is column hi - 1 (p[min(2m+1, N-1)]); the co-sited filter's column q0 - 1 is the halo pixel, column 0 at the tile's left
// edge (p[max(2m-1, 0)]).
template <class T, int SX, bool FULL>
__device__ __forceinline__ void weighted_row(const float* xr, int64_t sc, int q0, int hi, const T* ry, unsigned ay, const unsigned (&ax)[COLS],
                                             const Measure& ms, const Levels& lv, const EmitCoef& k, float (&h)[2][COLS / SX], u64& su)
{
    unsigned yq[COLS];
    float ub[COLS], ur[COLS];
    {
        float c[3][COLS];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float* s = xr + ch * sc + q0;                   // q0 + 7 < T <= the row stride: inside the tile's row
            if (FULL) {
                const float4 f0 = *reinterpret_cast<const float4*>(s), f1 = *reinterpret_cast<const float4*>(s + 4);
                c[ch][0] = f0.x; c[ch][1] = f0.y; c[ch][2] = f0.z; c[ch][3] = f0.w;
                c[ch][4] = f1.x; c[ch][5] = f1.y; c[ch][6] = f1.z; c[ch][7] = f1.w;
            } else {
#pragma unroll
                for (int q = 0; q < COLS; ++q) c[ch][q] = s[min(q, hi - 1)];
            }
        }
#pragma unroll
        for (int q = 0; q < COLS; ++q) emit_px(c[0][q], c[1][q], c[2][q], lv, k, yq[q], ub[q], ur[q]);
    }
    if (SX == 1) {
#pragma unroll
        for (int q = 0; q < COLS; ++q) { h[0][q] = ub[q]; h[1][q] = ur[q]; }
    } else if (ms.hco) {
        const int ql = max(q0 - 1, 0);
        unsigned yl;
        float bl, rl;
        emit_px(xr[ql], xr[sc + ql], xr[2 * sc + ql], lv, k, yl, bl, rl);
#pragma unroll
        for (int j = 0; j < COLS / 2; ++j) {
            h[0][j] = ((j ? ub[2 * j - 1] : bl) + ub[2 * j + 1]) + (ub[2 * j] + ub[2 * j]);
            h[1][j] = ((j ? ur[2 * j - 1] : rl) + ur[2 * j + 1]) + (ur[2 * j] + ur[2 * j]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < COLS / 2; ++j) {
            h[0][j] = ub[2 * j] + ub[2 * j + 1];
            h[1][j] = ur[2 * j] + ur[2 * j + 1];
        }
    }
    if (!ry) return;
    unsigned w[COLS];
    if (FULL) {
        load4(ry, w);
        load4(ry + 4, w + 4);
    } else {
#pragma unroll
        for (int q = 0; q < COLS; ++q) w[q] = q < hi ? (unsigned)ry[q] : 0u;
    }
    u64 row = 0ull;                                               // each term < 2^11 * 2^16 (8 bits), 2^10 * 2^20 (10 bits)
#pragma unroll
    for (int q = 0; q < COLS; ++q) {
        if (FULL || q < hi) {
            const int e = (int)yq[q] - (int)code_of<T>(w[q], ms.sh, (unsigned)lv.maxv);
            row += (u64)(ax[q] * (unsigned)(e * e));
        }
    }
    su += (u64)ay * row;
}

// One item: tile rows r0 .. r0 + SY - 1 and tile columns q0 .. q0+7 of the tile at xt, of which `rows` rows and the lanes 0 .. hi-1
// lie inside the frame (1 <= rows <= SY, 1 <= hi <= 8); Y, X: the frame position of (r0, q0), multiples of SY and of 8 / 4.  FULL:
// rows == SY, hi == 8 and every access is wide; else element by element.  ay[SY], ax[8]: the band numerators of the item's rows and
// columns, whether inside the frame or not.  The whole item is compiled twice, so that the two kinds of access never meet in one
// basic block.
template <class T, bool IL, int SX, int SY, bool VCO, bool FULL>
__device__ __forceinline__ void sse_item(const float* xt, int64_t sc, int64_t sh, int r0, int q0, int rows, int hi, const Planes<const T>& ref,
                                         int64_t Y, int64_t X, const Measure& ms, const Levels& lv, const EmitCoef& k,
                                         const unsigned (&ay)[SY], const unsigned (&ax)[COLS], u64 su[3])
{
    constexpr int CS = IL ? 2 : 1;                                // elements from one Cb (Cr) sample to the next
    constexpr int NC = COLS / SX;                                 // chroma samples of the item
    const int nc = SX == 2 ? (hi + 1) >> 1 : hi;
    const T* ry = ref.y + Y * ref.yr + X;
    float v[2][NC];
    if (SY == 1) {
        weighted_row<T, SX, FULL>(xt + (int64_t)r0 * sh, sc, q0, hi, ry, ay[0], ax, ms, lv, k, v, su[0]);
    } else {
        // In the order the vertical rule adds them: the row above (a, co-sited only; row 0 itself at the tile's top edge), the row
        // below (c; the last row inside the frame stands in for a missing one), then the item's first row (b): (a + c) + (b + b), or
        // b + c.
        const bool second = FULL || rows == 2;
        float acc[2][NC], t[2][NC];
        if (VCO) {
            weighted_row<T, SX, FULL>(xt + (int64_t)max(r0 - 1, 0) * sh, sc, q0, hi, nullptr, 0u, ax, ms, lv, k, acc, su[0]);
            weighted_row<T, SX, FULL>(xt + (int64_t)(second ? r0 + 1 : r0) * sh, sc, q0, hi, second ? ry + ref.yr : nullptr, ay[SY - 1], ax, ms,
                                      lv, k, t, su[0]);
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int j = 0; j < NC; ++j) acc[p][j] = acc[p][j] + t[p][j];
        } else {
            weighted_row<T, SX, FULL>(xt + (int64_t)(second ? r0 + 1 : r0) * sh, sc, q0, hi, second ? ry + ref.yr : nullptr, ay[SY - 1], ax, ms,
                                      lv, k, acc, su[0]);
        }
        weighted_row<T, SX, FULL>(xt + (int64_t)r0 * sh, sc, q0, hi, ry, ay[0], ax, ms, lv, k, t, su[0]);
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int j = 0; j < NC; ++j) v[p][j] = VCO ? acc[p][j] + (t[p][j] + t[p][j]) : t[p][j] + acc[p][j];
    }
    // chroma: the frame's sample (Y / SY, X / SX + m) is the tile's sample (r0 / SY, q0 / SX + m)
    const int64_t ci = SY == 2 ? Y >> 1 : Y, cx0 = SX == 2 ? X >> 1 : X;
    const T* ru = ref.u + ci * ref.ur + CS * cx0;
    const T* rv = IL ? ru + 1 : ref.v + ci * ref.vr + cx0;
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
            w[0][j] = j < nc ? (unsigned)ru[CS * j] : 0u;
            w[1][j] = j < nc ? (unsigned)rv[CS * j] : 0u;
        }
    }
    const u64 cy = (u64)(SY == 2 ? (ay[0] + ay[SY - 1]) >> 1 : ay[0]);
    u64 sb = 0ull, sr = 0ull;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        if (FULL || j < nc) {
            const int eb = clampi((int)rintf(v[0][j] * ms.s + (float)lv.co), 0, lv.maxv) - (int)code_of<T>(w[0][j], ms.sh, (unsigned)lv.maxv);
            const int er = clampi((int)rintf(v[1][j] * ms.s + (float)lv.co), 0, lv.maxv) - (int)code_of<T>(w[1][j], ms.sh, (unsigned)lv.maxv);
            const unsigned cx = SX == 2 ? (ax[SX * j] + ax[SX * j + SX - 1]) >> 1 : ax[j];
            sb += (u64)(cx * (unsigned)(eb * eb));
            sr += (u64)(cx * (unsigned)(er * er));
        }
    }
    su[1] += cy * sb;
    su[2] += cy * sr;
}

// Block b of tile t is block t * bpt + b: the items b * NT .. of the tile, item -> (chroma row kp, group g), tile rows SY kp ..,
// tile columns 8g .. 8g+7 (G8 = T / 8).  partials[(t * bpt + b) * 3 + p].
template <class T, bool IL, int SX, int SY, bool VCO, bool WIDE>
__global__ __launch_bounds__(NT) void sse_kernel(F32 x, Planes<const T> ref, RangeGrid gr, int G8, int bpt, Measure ms, Levels lv, EmitCoef k,
                                                 u64* __restrict__ partials)
{
    const int t = (int)(blockIdx.x / (unsigned)bpt), b = (int)(blockIdx.x - (unsigned)t * (unsigned)bpt);
    u64 su[3] = {0ull, 0ull, 0ull};
    const int tile = gr.first_tile + t;
    const int i = tile / gr.nx, j = tile - i * gr.nx;
    const int S = gr.S, O = gr.O, den = O > 0 ? 2 * O : 1;
    const int Yt = i * S, Xt = j * S;                             // the tile's first row and column in the frame: < H, < W
    const int hh = min(gr.T, gr.H - Yt), ww = min(gr.T, gr.W - Xt);
    const int rem = b * NT + (int)threadIdx.x;                    // < T * T / 8 <= 2^19
    const int kp = rem / G8, r0 = SY * kp, q0 = COLS * (rem - kp * G8);
    if (r0 < hh && q0 < ww) {
        const int rows = min(SY, hh - r0), hi = min(COLS, ww - q0);
        unsigned ay[SY], ax[COLS];
#pragma unroll
        for (int r = 0; r < SY; ++r) ay[r] = axis_weight(i, gr.ny, r0 + r, S, O, den);
#pragma unroll
        for (int q = 0; q < COLS; ++q) ax[q] = axis_weight(j, gr.nx, q0 + q, S, O, den);
        const float* xt = x.p + (int64_t)t * x.st;
        if (WIDE && rows == SY && hi == COLS)
            sse_item<T, IL, SX, SY, VCO, true>(xt, x.sc, x.sh, r0, q0, rows, hi, ref, (int64_t)Yt + r0, (int64_t)Xt + q0, ms, lv, k, ay, ax, su);
        else
            sse_item<T, IL, SX, SY, VCO, false>(xt, x.sc, x.sh, r0, q0, rows, hi, ref, (int64_t)Yt + r0, (int64_t)Xt + q0, ms, lv, k, ay, ax, su);
    }
    block_reduce<Sum>(su, partials + (int64_t)blockIdx.x * 3);
}

// One wave per tile: its bpt block partials, lane l taking l, l + 64, ..., then the wave tree.
__global__ __launch_bounds__(64) void final_kernel(const u64* __restrict__ p, int bpt, u64* __restrict__ out)
{
    row_final<Sum, 3>(p, bpt, out);
}

// -- host ----------------------------------------------------------------------------------------------------------------------------

// The item space: SY rows by eight columns, T * T / (8 SY) items to a tile, NT to a block.  Blocks per tile and blocks in all;
// false for what the calls refuse.
bool item_blocks_of(int T, int sy, int n_tiles, int t_max, int& bpt, int64_t& blocks)
{
    if (T < 64 || T % 64 || T > t_max || (sy != 1 && sy != 2) || n_tiles < 1) return false;
    bpt = (int)((int64_t)T * T / ((int64_t)sy * COLS * NT));
    blocks = (int64_t)n_tiles * bpt;
    return blocks <= INT32_MAX;
}

// The one place that decides the access path: the call launches from it, pc_chroma_rate_plan reports it.
bool wide_path(const void* x, int64_t st, int64_t sc, int64_t sh, int O, bool il, int es, int sx, const pc_chr_frame* ref)
{
    if (!f32_wide(x, st, sc, sh) || (sx == 2 && O % 8 != 0)) return false;
    if (!plane_wide(ref->y, ref->y_row, es) || !plane_wide(ref->u, ref->u_row, es)) return false;
    return il || plane_wide(ref->v, ref->v_row, es);
}

}  // namespace

extern "C" size_t pc_chroma_rate_workspace_size(int T, int sy, int n_tiles)
{
    int bpt;
    int64_t blocks;
    return item_blocks_of(T, sy, n_tiles, T_MAX8, bpt, blocks) ? (size_t)blocks * 3 * sizeof(u64) : 0;
}

extern "C" int pc_chroma_rate_plan(const void* x, int64_t sxt, int64_t sxc, int64_t sxh, int O, int layout, int bits, int sx,
                                   const pc_chr_frame* ref, int* wide)
{
    Fmt fm;
    if (!x || !wide || !format_of(layout, bits, 0, sx, 1, fm) || O < 0 || !ref) return PC_ERR_ARG;
    if (!(ref->y && ref->u && (fm.il || ref->v))) return PC_ERR_ARG;
    *wide = wide_path(x, sxt, sxc, sxh, O, fm.il, bits == 10 ? 2 : 1, sx, ref) ? 1 : 0;
    return PC_OK;
}

extern "C" int pc_chroma_rate_tile_sse(const float* x, int64_t sxt, int64_t sxc, int64_t sxh, int H, int W, int T, int O, int first_tile,
                                       int n_tiles, int layout, int bits, int shift, int sx, int sy, int hsite, int vsite, int range,
                                       float kr, float kg, float kb, float ib, float ir, const pc_chr_frame* ref, void* workspace,
                                       size_t workspace_bytes, uint64_t* out, void* stream)
{
    Geo g;
    Levels lv;
    Fmt fm;
    int bpt;
    int64_t blocks;
    if (!format_of(layout, bits, shift, sx, sy, fm) || !site_ok(hsite) || !site_ok(vsite) || !depth_levels(bits, range, lv)) return PC_ERR_ARG;
    if (!geo_of(H, W, T, O, bits == 10 ? T_MAX10 : T_MAX8, g) || !item_blocks_of(T, sy, n_tiles, T_MAX8, bpt, blocks)) return PC_ERR_ARG;
    if (first_tile < 0 || (int64_t)first_tile + n_tiles > (int64_t)g.ny * g.nx) return PC_ERR_ARG;
    if (!x || !aligned(x, 4) || sxh < T || sxc < 1 || sxt < 1) return PC_ERR_ARG;
    if (!picture_ok(fm, ref, W)) return PC_ERR_ARG;
    if (!workspace || !aligned(workspace, 8) || !out || !aligned(out, 8)) return PC_ERR_ARG;
    if (workspace_bytes < (size_t)blocks * 3 * sizeof(u64)) return PC_ERR_ARG;
    const bool hco = sx == 2 && hsite == PC_CHR_COSITED, vco = sy == 2 && vsite == PC_CHR_COSITED;
    const bool wide = wide_path(x, sxt, sxc, sxh, O, fm.il, bits == 10 ? 2 : 1, sx, ref);
    const F32 xv{x, sxt, sxc, sxh};
    const RangeGrid gr{{H, W, T, g.S, O, g.ny, g.nx}, first_tile};
    const EmitCoef k{kr, kg, kb, ib, ir};
    const Measure ms{hco ? 1 : 0, 1.f / (float)((sx == 2 ? (hco ? 4 : 2) : 1) * (sy == 2 ? (vco ? 4 : 2) : 1)), shift};
    u64* part = static_cast<u64*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks);
    with_format(fm, [&](auto el, auto il, auto SX, auto SY) {
        using T_ = decltype(el);
        const Planes<const T_> r = planes_of<const T_>(ref);
#define PC_SSE(VCO, WIDE)                                                                                                                   \
    hipLaunchKernelGGL((sse_kernel<T_, il.value, SX.value, SY.value, VCO, WIDE>), grid, dim3(NT), 0, st, xv, r, gr, T / COLS, bpt, ms, lv, k, part)
        // VCO is instantiated for SY = 2 alone: at SY = 1 both branches below name the same kernel
        if (wide) {
            if (SY.value == 2 && vco) PC_SSE((SY.value == 2), true); else PC_SSE(false, true);
        } else {
            if (SY.value == 2 && vco) PC_SSE((SY.value == 2), false); else PC_SSE(false, false);
        }
#undef PC_SSE
    });
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(final_kernel, dim3((unsigned)n_tiles), dim3(64), 0, st, part, bpt, reinterpret_cast<u64*>(out));
    HIPCHK(hipGetLastError());
    return PC_OK;
}

extern "C" const char* pc_chroma_rate_strerror(int code)
{
    switch (code) {
    case PC_OK: return "ok";
    case PC_ERR_ARG:
        return "invalid argument, unknown layout, depth, shift, subsampling, siting or range, geometry outside pc_chroma_rate.h, tile range "
               "outside the grid or workspace too small (pc_chroma_rate_workspace_size)";
    case PC_ERR_HIP: return "HIP runtime error";
    default: return "unknown error";
    }
}

extern "C" int pc_chroma_rate_last_hip_error(void) { return g_last_hip.load(); }

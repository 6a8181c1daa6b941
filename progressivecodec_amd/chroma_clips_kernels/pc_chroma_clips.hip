// pc_chroma_clips.hip -- clips of YUV frames of any of pc_chroma.h's twelve formats and three chroma sitings on gfx950
// (pc_chroma_clips.h): which tiles of a frame changed since the previous one, counted exactly over each tile's footprint, and the cut
// of a LIST of tiles into float32 RGB.  Definition: DESIGN.md section 25, on top of sections 23 (the cut) and 11 (geometry); what
// pc_clips.hip (section 16) is for NV12 / I420 / P010 with centre-sited chroma.  Loads, levels and the per-pixel colour arithmetic are
// image_csrc/pc_yuv_device.h's, the geometry image_csrc/pc_tile_grid.h's, the reduction image_csrc/pc_reduce.h's, the ingest item
// and the format checks image_csrc/pc_chroma_items.h's.
//
// Changes.  A work item is SY luma rows of one tile (a row pair at 4:2:0, one row at 4:2:2 and 4:4:4) by eight tile-aligned luma
// columns, with the 8 / SX chroma samples of its cells, in both frames.  A thread takes one item, a block NT consecutive items of ONE
// tile (T * T / (8 SY) is a multiple of 256 for every T that is a multiple of 64: no block straddles two tiles and none has a tail).
// S and T are multiples of 4, so a tile's cells are the frame's: the items cover the tile's luma and the chroma rectangle WITHOUT the
// halo exactly once.  One more block per tile takes the halo ring -- the chroma row above or below and the column left or right of
// that rectangle -- element by element (2 T + 4 samples at most); a side is taken only where the footprint rule of pc_chroma_clips.h
// has a halo on it (four wave-uniform flags, computed on the host from the format, the siting and the upsampling) and the frame has
// the samples.  An item whose rows and columns all lie inside the frame and whose accesses are all wide is compiled on its own
// (FULL); every other item goes element by element.  The access path only changes the load instructions, never which thread holds
// which sample; and what is added are integers: thread, wave tree, the waves of a block in order (12 words of LDS), then final_kernel
// over a tile's block partials.  No atomics, no LDS on the data path.  Template parameters are what changes an item's shape: element
// type, interleave, (SX, SY) and the access path; the depth shift and the halo flags are wave-uniform kernel arguments.
// 24 changes kernels, 24 cut kernels and the final.
//
// Cut.  pc_chroma_tiles.hip's cut_kernel with the tile taken from a device array: a work item is eight consecutive luma columns of
// one tile row, aligned in tile columns; an index outside the grid is checked by the kernel and leaves the item's floats +0.0f.
#include "pc_image_host.h"
#include "pc_reduce.h"
#include "pc_tile_grid.h"
#include "pc_yuv_device.h"
#include "pc_yuv_items.h"
#include "pc_chroma_items.h"

#include "pc_chroma_clips.h"

namespace {

static_assert(PC_CHC_PLANAR == LAYOUT_PLANAR && PC_CHC_SEMIPLANAR == LAYOUT_SEMIPLANAR, "pc_chroma_items.h's layouts are pc_chroma_clips.h's");
static_assert(PC_CHC_CENTRE == SITE_CENTRE && PC_CHC_COSITED == SITE_COSITED, "pc_chroma_items.h's sitings are pc_chroma_clips.h's");

constexpr int T_MAX = 2048;

struct RangeGrid : Grid {                // the frame, the grid and the linear range of the call
    int first_tile;
};

// The footprint's halo: whether the rule reaches one chroma sample below the items' rectangle (lo) and above it (hi) along y and
// along x, the depth shift and the code mask.
struct Rule {
    int ylo, yhi, xlo, xhi, sh;
    unsigned mask;
};

// -- changes -------------------------------------------------------------------------------------------------------------------------

// one sample pair of plane p: elements a and b of the two frames
template <class T>
__device__ __forceinline__ void take(unsigned a, unsigned b, int p, const Rule& ru, unsigned (&su)[3])
{
    su[p] += code_of<T>(a, ru.sh, ru.mask) != code_of<T>(b, ru.sh, ru.mask) ? 1u : 0u;
}

// One item: luma rows Y .. Y + SY - 1 and columns X .. X+7 of the frame (multiples of SY and SX), of which `rows` rows and the lanes
// 0 .. hi-1 lie inside the tile's part of the frame (1 <= rows <= SY, 1 <= hi <= 8), and the chroma samples (Y / SY, X / SX + m),
// SX m < hi.  FULL: rows == SY, hi == 8 and every access is wide; else element by element.  A lane outside is 0 in both frames: it
// adds nothing.
template <class T, bool IL, int SX, int SY, bool FULL>
__device__ __forceinline__ void changes_item(const Planes<const T>& a, const Planes<const T>& b, int64_t Y, int64_t X, int rows, int hi,
                                             const Rule& ru, unsigned (&su)[3])
{
    constexpr int CS = IL ? 2 : 1;                                // elements from one Cb (Cr) sample to the next
    constexpr int NC = COLS / SX;                                 // chroma samples of the item
#pragma unroll
    for (int r = 0; r < SY; ++r) {
        if (FULL || r < rows) {
            const T* pa = a.y + (Y + r) * a.yr + X;
            const T* pb = b.y + (Y + r) * b.yr + X;
            unsigned wa[COLS], wb[COLS];
            if (FULL) {
                load4(pa, wa);
                load4(pa + 4, wa + 4);
                load4(pb, wb);
                load4(pb + 4, wb + 4);
            } else {
#pragma unroll
                for (int q = 0; q < COLS; ++q) {
                    wa[q] = q < hi ? (unsigned)pa[q] : 0u;
                    wb[q] = q < hi ? (unsigned)pb[q] : 0u;
                }
            }
#pragma unroll
            for (int q = 0; q < COLS; ++q) take<T>(wa[q], wb[q], 0, ru, su);
        }
    }
    const int64_t ci = SY == 2 ? Y >> 1 : Y, cx0 = SX == 2 ? X >> 1 : X;
    const T* ua = a.u + ci * a.ur + CS * cx0;
    const T* va = IL ? ua + 1 : a.v + ci * a.vr + cx0;
    const T* ub = b.u + ci * b.ur + CS * cx0;
    const T* vb = IL ? ub + 1 : b.v + ci * b.vr + cx0;
    unsigned ca[2][NC], cb[2][NC];                                // [Cb, Cr][sample]
    if (FULL) {
        if (IL) {
            unsigned ea[2 * NC], eb[2 * NC];
#pragma unroll
            for (int m = 0; m < 2 * NC; m += 4) {
                load4(ua + m, ea + m);
                load4(ub + m, eb + m);
            }
#pragma unroll
            for (int m = 0; m < NC; ++m) {
                ca[0][m] = ea[2 * m]; ca[1][m] = ea[2 * m + 1];
                cb[0][m] = eb[2 * m]; cb[1][m] = eb[2 * m + 1];
            }
        } else {
#pragma unroll
            for (int m = 0; m < NC; m += 4) {
                load4(ua + m, ca[0] + m);
                load4(va + m, ca[1] + m);
                load4(ub + m, cb[0] + m);
                load4(vb + m, cb[1] + m);
            }
        }
    } else {
#pragma unroll
        for (int m = 0; m < NC; ++m) {
            const bool in = SX * m < hi;
            ca[0][m] = in ? (unsigned)ua[CS * m] : 0u;
            ca[1][m] = in ? (unsigned)va[CS * m] : 0u;
            cb[0][m] = in ? (unsigned)ub[CS * m] : 0u;
            cb[1][m] = in ? (unsigned)vb[CS * m] : 0u;
        }
    }
#pragma unroll
    for (int m = 0; m < NC; ++m) {
        take<T>(ca[0][m], cb[0][m], 1, ru, su);
        take<T>(ca[1][m], cb[1][m], 2, ru, su);
    }
}

// Blocks t * (bpt + 1) .. + bpt - 1 hold the items of tile t: item -> (chroma row kp, group g), tile rows SY kp .. SY kp + SY - 1,
// tile columns 8g .. 8g+7 (G8 = T / 8); block t * (bpt + 1) + bpt holds its halo ring -- the chroma row above and below and the column
// left and right of the rectangle the items covered, where the rule has a halo on that side and the frame has the samples.
// partials[blockIdx.x * 3 + p].
template <class T, bool IL, int SX, int SY, bool WIDE>
__global__ __launch_bounds__(NT) void changes_kernel(Planes<const T> a, Planes<const T> b, RangeGrid gr, int G8, int bpt, Rule ru,
                                                     u64* __restrict__ partials)
{
    constexpr int CS = IL ? 2 : 1;
    const int bpt1 = bpt + 1;
    const int t = (int)(blockIdx.x / (unsigned)bpt1), bl = (int)(blockIdx.x - (unsigned)t * (unsigned)bpt1);
    const int tile = gr.first_tile + t;
    const int i = tile / gr.nx, j = tile - i * gr.nx;
    const int Yt = i * gr.S, Xt = j * gr.S;                       // the tile's first row and column in the frame: < H, < W
    const int hh = min(gr.T, gr.H - Yt), ww = min(gr.T, gr.W - Xt);
    unsigned su[3] = {0u, 0u, 0u};
    if (bl < bpt) {
        const int rem = bl * NT + (int)threadIdx.x;               // < T * T / 8 <= 2^19
        const int kp = rem / G8, r0 = SY * kp, q0 = COLS * (rem - kp * G8);
        if (r0 < hh && q0 < ww) {
            const int rows = min(SY, hh - r0), hi = min(COLS, ww - q0);
            if (WIDE && rows == SY && hi == COLS)
                changes_item<T, IL, SX, SY, true>(a, b, (int64_t)Yt + r0, (int64_t)Xt + q0, rows, hi, ru, su);
            else
                changes_item<T, IL, SX, SY, false>(a, b, (int64_t)Yt + r0, (int64_t)Xt + q0, rows, hi, ru, su);
        }
    } else {
        // the chroma rectangle the items covered: rows r0c .. r1c, columns c0c .. c1c; the ring around it where the rule and the frame
        // have it
        const int Hc = (gr.H + SY - 1) / SY, Wc = (gr.W + SX - 1) / SX;
        const int r0c = Yt / SY, r1c = r0c + (hh + SY - 1) / SY - 1, c0c = Xt / SX, c1c = c0c + (ww + SX - 1) / SX - 1;
        const bool top = ru.ylo && r0c > 0, bottom = ru.yhi && r1c < Hc - 1, left = ru.xlo && c0c > 0, right = ru.xhi && c1c < Wc - 1;
        const int cf = c0c - (left ? 1 : 0), nw = c1c + (right ? 1 : 0) - cf + 1, nh = r1c - r0c + 1;
        for (int idx = (int)threadIdx.x; idx < 2 * nw + 2 * nh; idx += NT) {
            int row, col;
            bool on;
            if (idx < nw) { row = r0c - 1; col = cf + idx; on = top; }
            else if (idx < 2 * nw) { row = r1c + 1; col = cf + idx - nw; on = bottom; }
            else if (idx < 2 * nw + nh) { row = r0c + idx - 2 * nw; col = c0c - 1; on = left; }
            else { row = r0c + idx - 2 * nw - nh; col = c1c + 1; on = right; }
            if (on) {                                              // 0 <= row < Hc and 0 <= col < Wc
                const int64_t oa = (int64_t)row * a.ur + CS * (int64_t)col, ob = (int64_t)row * b.ur + CS * (int64_t)col;
                const T* va = IL ? a.u + oa + 1 : a.v + (int64_t)row * a.vr + col;
                const T* vb = IL ? b.u + ob + 1 : b.v + (int64_t)row * b.vr + col;
                take<T>((unsigned)a.u[oa], (unsigned)b.u[ob], 1, ru, su);
                take<T>((unsigned)*va, (unsigned)*vb, 2, ru, su);
            }
        }
    }
    block_reduce<Sum>(su, partials + (int64_t)blockIdx.x * 3);
}

// One wave per tile: its nb block partials, lane l taking l, l + 64, ..., then the wave tree.
__global__ __launch_bounds__(64) void final_kernel(const u64* __restrict__ p, int nb, u64* __restrict__ out)
{
    row_final<Sum, 3>(p, nb, out);
}

// -- cut -----------------------------------------------------------------------------------------------------------------------------

// Items are the eight-column groups of the listed tiles' rows: item -> (entry m of the list, row r, group g), tile columns 8g .. 8g+7.
// G8 = T / 8, tile_items = T * G8, items = n * tile_items.  The chroma taps are clamped at the FRAME's edges Hc - 1, Wc - 1.  WIDE
// needs S a multiple of 8 at SX = 2 (X is then one, and X / 2 a multiple of 4); at SX = 1 S is a multiple of 4, which is enough.
template <class T, bool IL, int SX, int SY, bool WIDE>
__global__ __launch_bounds__(NT) void cut_list_kernel(Planes<const T> s, int H, int W, int Hc, int Wc, int TT, int S, int ny, int nx,
                                                      const int32_t* __restrict__ tiles, float* __restrict__ dst, int G8, int tile_items,
                                                      int64_t items, Taps t, Levels lv, IngestCoef k)
{
    const int64_t item = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (item >= items) return;
    const int m = (int)(item / tile_items), rem = (int)(item - (int64_t)m * tile_items);
    const int r = rem / G8, g = rem - r * G8;
    const int idx = tiles[m];
    const bool listed = idx >= 0 && (int64_t)idx < (int64_t)ny * nx;
    const int ti = listed ? idx / nx : 0, tj = listed ? idx - ti * nx : 0;
    const int64_t Y64 = (int64_t)ti * S + r, X64 = (int64_t)tj * S + COLS * g;                                   // frame coordinates
    float o[3][COLS];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < COLS; ++i) o[c][i] = 0.f;
    if (listed && Y64 < H && X64 < W) ingest_item<T, IL, SX, SY, WIDE>(s, W, Hc, Wc, (int)Y64, (int)X64, t, lv, k, o);
    const int64_t plane = (int64_t)TT * TT;
#pragma unroll
    for (int c = 0; c < 3; ++c) store8<WIDE>(dst + ((int64_t)m * 3 + c) * plane + (int64_t)r * TT + COLS * g, o[c], COLS);
}

// -- host ----------------------------------------------------------------------------------------------------------------------------

// every plane pointer on four elements, every row stride a multiple of 4
bool picture_wide(bool il, int es, const pc_chc_frame* f)
{
    if (!plane_wide(f->y, f->y_row, es) || !plane_wide(f->u, f->u_row, es)) return false;
    return il || plane_wide(f->v, f->v_row, es);
}

// The one place that decides the access path: the calls launch from it, pc_chroma_clips_plan reports it.
bool wide_path(int op, bool il, int es, int sx, const pc_chc_frame* frame, const pc_chc_frame* other, const void* f32, int O)
{
    if ((sx == 2 && O % 8) || !picture_wide(il, es, frame)) return false;
    if (op == PC_CHC_CHANGES) return picture_wide(il, es, other);
    return aligned(f32, 16);             // the strides 3*T*T, T*T and T are multiples of 4
}

// The item space of a tile taken sy rows by eight columns: T * T / (8 sy) items, NT to a block, and one more block per tile (the halo
// ring's).  Blocks per tile without the ring's and blocks in all; false for what the calls refuse.
bool item_blocks_of(int T, int sy, int n_tiles, int& bpt, int64_t& blocks)
{
    if (T < 64 || T % 64 || T > T_MAX || (sy != 1 && sy != 2) || n_tiles < 1) return false;
    bpt = (int)((int64_t)T * T / ((int64_t)sy * COLS * NT));
    blocks = (int64_t)n_tiles * (bpt + 1);
    return blocks <= INT32_MAX;
}

}  // namespace

extern "C" size_t pc_chroma_clips_changes_workspace_size(int T, int sy, int n_tiles)
{
    int bpt;
    int64_t blocks;
    return item_blocks_of(T, sy, n_tiles, bpt, blocks) ? (size_t)blocks * 3 * sizeof(u64) : 0;
}

extern "C" int pc_chroma_clips_plan(int op, int layout, int bits, int sx, const pc_chc_frame* frame, const pc_chc_frame* other, const void* f32,
                                    int O, int* wide)
{
    Fmt fm;
    if ((op != PC_CHC_CHANGES && op != PC_CHC_CUT) || !format_of(layout, bits, 0, sx, 1, fm) || !wide || O < 0) return PC_ERR_ARG;
    if (op == PC_CHC_CUT) other = nullptr;
    if (!frame || (op == PC_CHC_CHANGES && !other) || (op == PC_CHC_CUT && !f32)) return PC_ERR_ARG;
    for (const pc_chc_frame* f : {frame, other})
        if (f && !(f->y && f->u && (fm.il || f->v))) return PC_ERR_ARG;
    *wide = wide_path(op, fm.il, bits == 10 ? 2 : 1, sx, frame, other, f32, O) ? 1 : 0;
    return PC_OK;
}

extern "C" int pc_chroma_clips_tile_changes(const pc_chc_frame* cur, const pc_chc_frame* prev, int layout, int bits, int shift, int sx, int sy,
                                            int hsite, int vsite, int upsample, int H, int W, int T, int O, int first_tile, int n_tiles,
                                            void* workspace, size_t workspace_bytes, uint64_t* out, void* stream)
{
    Geo g;
    Fmt fm;
    int bpt;
    int64_t blocks;
    if (!format_of(layout, bits, shift, sx, sy, fm) || !site_ok(hsite) || !site_ok(vsite) || !upsample_ok(upsample)) return PC_ERR_ARG;
    if (!geo_of(H, W, T, O, T_MAX, g) || !item_blocks_of(T, sy, n_tiles, bpt, blocks)) return PC_ERR_ARG;
    if (first_tile < 0 || (int64_t)first_tile + n_tiles > (int64_t)g.ny * g.nx) return PC_ERR_ARG;
    if (!picture_ok(fm, cur, W) || !picture_ok(fm, prev, W)) return PC_ERR_ARG;
    if (!workspace || !aligned(workspace, 8) || !out || !aligned(out, 8)) return PC_ERR_ARG;
    if (workspace_bytes < (size_t)blocks * 3 * sizeof(u64)) return PC_ERR_ARG;
    const bool wide = wide_path(PC_CHC_CHANGES, fm.il, bits == 10 ? 2 : 1, sx, cur, prev, nullptr, O);
    const RangeGrid gr{{H, W, T, g.S, O, g.ny, g.nx}, first_tile};
    const bool linear = upsample == PC_CHC_LINEAR;
    const Rule ru{sy == 2 && linear && vsite == PC_CHC_CENTRE, sy == 2 && linear, sx == 2 && linear && hsite == PC_CHC_CENTRE,
                  sx == 2 && linear, shift, (1u << bits) - 1u};
    u64* part = static_cast<u64*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks);
    with_format(fm, [&](auto el, auto il, auto SX, auto SY) {
        using T_ = decltype(el);
        const Planes<const T_> a = planes_of<const T_>(cur), b = planes_of<const T_>(prev);
        if (wide)
            hipLaunchKernelGGL((changes_kernel<T_, il.value, SX.value, SY.value, true>), grid, dim3(NT), 0, st, a, b, gr, T / COLS, bpt, ru, part);
        else
            hipLaunchKernelGGL((changes_kernel<T_, il.value, SX.value, SY.value, false>), grid, dim3(NT), 0, st, a, b, gr, T / COLS, bpt, ru, part);
    });
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(final_kernel, dim3((unsigned)n_tiles), dim3(64), 0, st, part, bpt + 1, reinterpret_cast<u64*>(out));
    HIPCHK(hipGetLastError());
    return PC_OK;
}

extern "C" int pc_chroma_clips_cut_list(const pc_chc_frame* src, int layout, int bits, int shift, int sx, int sy, int hsite, int vsite, int range,
                                        int upsample, float a, float b, float c, float d, int H, int W, int T, int O, const int32_t* tiles,
                                        int n, float* dst, void* stream)
{
    Geo g;
    Levels lv;
    Fmt fm;
    if (!geo_of(H, W, T, O, T_MAX, g) || !upsample_ok(upsample)) return PC_ERR_ARG;
    if (!format_of(layout, bits, shift, sx, sy, fm) || !site_ok(hsite) || !site_ok(vsite)) return PC_ERR_ARG;
    if (!dst || !aligned(dst, 4) || !picture_ok(fm, src, W) || !depth_levels(bits, range, lv)) return PC_ERR_ARG;
    if (!tiles || !aligned(tiles, 4) || n < 1 || n > INT32_MAX / 3) return PC_ERR_ARG;
    const int G8 = T / COLS;
    const int64_t tile_items = (int64_t)T * G8;                    // <= 2^19
    const int64_t items = (int64_t)n * tile_items, blocks = cdiv(items, NT);
    if (blocks > INT32_MAX) return PC_ERR_ARG;
    const bool wide = wide_path(PC_CHC_CUT, fm.il, bits == 10 ? 2 : 1, sx, src, nullptr, dst, O);
    const IngestCoef k{a, b, c, d};
    const Taps t = taps_of(sx, sy, hsite, vsite, upsample == PC_CHC_LINEAR, shift);
    const int Hc = (int)cdiv(H, sy), Wc = (int)cdiv(W, sx);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks);
    with_format(fm, [&](auto el, auto il, auto SX, auto SY) {
        using T_ = decltype(el);
        const Planes<const T_> s = planes_of<const T_>(src);
        if (wide)
            hipLaunchKernelGGL((cut_list_kernel<T_, il.value, SX.value, SY.value, true>), grid, dim3(NT), 0, st, s, H, W, Hc, Wc, T, g.S, g.ny,
                               g.nx, tiles, dst, G8, (int)tile_items, items, t, lv, k);
        else
            hipLaunchKernelGGL((cut_list_kernel<T_, il.value, SX.value, SY.value, false>), grid, dim3(NT), 0, st, s, H, W, Hc, Wc, T, g.S, g.ny,
                               g.nx, tiles, dst, G8, (int)tile_items, items, t, lv, k);
    });
    HIPCHK(hipGetLastError());
    return PC_OK;
}

extern "C" const char* pc_chroma_clips_strerror(int code)
{
    switch (code) {
    case PC_OK: return "ok";
    case PC_ERR_ARG:
        return "invalid argument, unknown layout, depth, shift, subsampling, siting, range or upsampler, geometry outside "
               "pc_chroma_clips.h, tile range outside the grid, empty tile list or workspace too small "
               "(pc_chroma_clips_changes_workspace_size)";
    case PC_ERR_HIP: return "HIP runtime error";
    default: return "unknown error";
    }
}

extern "C" int pc_chroma_clips_last_hip_error(void) { return g_last_hip.load(); }

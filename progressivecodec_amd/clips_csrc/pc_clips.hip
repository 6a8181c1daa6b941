// pc_clips.hip -- clips of YUV 4:2:0 frames (NV12 / I420 / P010) on gfx950 (pc_clips.h): which tiles of a frame changed since the
// previous one, counted exactly over each tile's footprint, and the cut of a LIST of tiles into float32 RGB.  Definition: DESIGN.md
// section 16, on top of sections 14 (the cut) and 11 (geometry); the cut is cut_item of image_csrc/pc_yuv_items.h, as in
// pc_frame_tiles.hip; the compare is its compare_tile with this library's accumulate policy (Count), as in pc_clip_tol.hip; the
// reduction is image_csrc/pc_reduce.h's.
//
// Changes.  A work item is one ROW PAIR (2k, 2k+1) of one tile by eight tile-aligned luma columns: sixteen luma samples and the four
// Cb and four Cr samples of the 2 x 2 cells the thread holds, in both frames.  A thread takes one item, a block NT consecutive items
// of ONE tile (T * T / 16 is a multiple of 256 for every T that is a multiple of 64: no block straddles two tiles and none has a
// tail).  S and T are even, so a tile's cells are the frame's: the items cover the tile's luma and the chroma rectangle WITHOUT the
// halo exactly once.  One more block per tile takes the halo ring -- the chroma row above and below and the column left and right of
// that rectangle, where the frame has them and the upsampling is linear -- element by element (2 T + 4 samples at most).  An item
// whose rows and columns all lie inside the frame and whose accesses are all wide is compiled on its own (FULL); every other item
// goes element by element.  The access path only changes the load instructions, never which thread holds which sample; and what is
// added are integers: thread, wave tree, the waves of a block in order (12 words of LDS), then final_kernel over a tile's block
// partials.  No atomics, no LDS on the data path.
//
// Cut.  pc_frame_tiles.hip's cut_kernel with the tile taken from a device array: a work item is eight consecutive luma columns of
// one tile row, aligned in tile columns; an index outside the grid is checked by the kernel and leaves the item's floats +0.0f.
#include "pc_image_host.h"
#include "pc_reduce.h"
#include "pc_tile_grid.h"
#include "pc_yuv_device.h"
#include "pc_yuv_items.h"

#include "pc_clips.h"

namespace {

constexpr int T_MAX = 2048;

struct RangeGrid : Grid {                // the frame, the grid and the linear range of the call
    int first_tile;
};

// -- changes -------------------------------------------------------------------------------------------------------------------------

// compare_tile's policy: the samples of plane p whose codes differ
struct Count {
    static constexpr int N = 3;
    template <int SH>
    static __device__ __forceinline__ void take(unsigned a, unsigned b, int p, unsigned (&su)[3])
    {
        su[p] += (a >> SH) != (b >> SH) ? 1u : 0u;
    }
};

// Blocks t * (bpt + 1) .. + bpt - 1 hold the items of tile t: item -> (row pair k, group g), tile rows 2k and 2k + 1, tile columns
// 8g .. 8g+7; block t * (bpt + 1) + bpt holds its halo ring.  partials[blockIdx.x * 3 + p].
template <class T, bool IL, bool WIDE>
__global__ __launch_bounds__(NT) void changes_kernel(Planes<const T> a, Planes<const T> b, RangeGrid gr, int G8, int bpt, int halo,
                                                     u64* __restrict__ partials)
{
    const int bpt1 = bpt + 1;
    const int t = (int)(blockIdx.x / (unsigned)bpt1), bl = (int)(blockIdx.x - (unsigned)t * (unsigned)bpt1);
    unsigned su[3] = {0u, 0u, 0u};
    compare_tile<T, IL, WIDE, Count>(a, b, gr, gr.first_tile + t, bl, bpt, G8, halo, su);
    block_reduce<Sum>(su, partials + (int64_t)blockIdx.x * 3);
}

// One wave per tile: its nb block partials, lane l taking l, l + 64, ..., then the wave tree.
__global__ __launch_bounds__(64) void final_kernel(const u64* __restrict__ p, int nb, u64* __restrict__ out)
{
    row_final<Sum, 3>(p, nb, out);
}

// -- cut -----------------------------------------------------------------------------------------------------------------------------

// Items are the eight-column groups of the listed tiles' rows: item -> (entry m of the list, row r, group g), tile columns 8g .. 8g+7.
// G8 = T / 8, tile_items = T * G8, items = n * tile_items.  SH: the bits below the code in an element (P010: 6).  The chroma taps are
// clamped at the FRAME's edges Hc - 1, Wc - 1.  WIDE needs S a multiple of 8: X0 is then one, and X0 / 2 a multiple of 4.
template <class T, bool IL, bool WIDE>
__global__ __launch_bounds__(NT) void cut_list_kernel(Planes<const T> s, int H, int W, int Hc, int Wc, int TT, int S, int ny, int nx,
                                                      const int32_t* __restrict__ tiles, float* __restrict__ dst, int G8, int tile_items,
                                                      int64_t items, int linear, Levels lv, IngestCoef k)
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
    if (listed && Y64 < H && X64 < W) cut_item<T, IL, WIDE, false>(s, W, Hc, Wc, (int)Y64, (int)X64, linear, lv, k, o);
    const int64_t plane = (int64_t)TT * TT;
#pragma unroll
    for (int c = 0; c < 3; ++c) store8<WIDE>(dst + ((int64_t)m * 3 + c) * plane + (int64_t)r * TT + COLS * g, o[c], COLS);
}

// -- host ----------------------------------------------------------------------------------------------------------------------------

// The one place that decides the access path: the calls launch from it, pc_clips_plan reports it.
bool wide_path(int op, int fmt, const pc_cl_frame* frame, const pc_cl_frame* other, const void* f32, int O)
{
    if (O % 8 || !frame_wide(fmt, frame)) return false;
    if (op == PC_CL_CHANGES) return frame_wide(fmt, other);
    return aligned(f32, 16);             // the strides 3*T*T, T*T and T are multiples of 4
}

template <class T, bool IL>
void launch_changes(bool wide, dim3 grid, hipStream_t st, const pc_cl_frame* cur, const pc_cl_frame* prev, const RangeGrid& gr, int bpt,
                    int halo, u64* part)
{
    const Planes<const T> a = planes_of<const T>(cur), b = planes_of<const T>(prev);
    if (wide)
        hipLaunchKernelGGL((changes_kernel<T, IL, true>), grid, dim3(NT), 0, st, a, b, gr, gr.T / COLS, bpt, halo, part);
    else
        hipLaunchKernelGGL((changes_kernel<T, IL, false>), grid, dim3(NT), 0, st, a, b, gr, gr.T / COLS, bpt, halo, part);
}

template <class T, bool IL>
void launch_cut(bool wide, dim3 grid, hipStream_t st, const pc_cl_frame* src, int H, int W, int T_, const Geo& g, const int32_t* tiles,
                float* dst, int G8, int tile_items, int64_t items, int linear, const Levels& lv, const IngestCoef& k)
{
    const Planes<const T> s = planes_of<const T>(src);
    const int Hc = (int)cdiv(H, 2), Wc = (int)cdiv(W, 2);
    if (wide)
        hipLaunchKernelGGL((cut_list_kernel<T, IL, true>), grid, dim3(NT), 0, st, s, H, W, Hc, Wc, T_, g.S, g.ny, g.nx, tiles, dst, G8,
                           tile_items, items, linear, lv, k);
    else
        hipLaunchKernelGGL((cut_list_kernel<T, IL, false>), grid, dim3(NT), 0, st, s, H, W, Hc, Wc, T_, g.S, g.ny, g.nx, tiles, dst, G8,
                           tile_items, items, linear, lv, k);
}

}  // namespace

extern "C" size_t pc_clips_changes_workspace_size(int T, int n_tiles)
{
    int bpt;
    int64_t blocks;
    return pair_blocks_of(T, n_tiles, T_MAX, 1, bpt, blocks) ? (size_t)blocks * 3 * sizeof(u64) : 0;
}

extern "C" int pc_clips_plan(int op, int fmt, const pc_cl_frame* frame, const pc_cl_frame* other, const void* f32, int O, int* wide)
{
    if ((op != PC_CL_CHANGES && op != PC_CL_CUT) || !fmt_ok(fmt) || !wide || O < 0) return PC_ERR_ARG;
    if (op == PC_CL_CUT) other = nullptr;
    if (!frame || (op == PC_CL_CHANGES && !other) || (op == PC_CL_CUT && !f32)) return PC_ERR_ARG;
    for (const pc_cl_frame* f : {frame, other})
        if (f && !planes_set(fmt, f)) return PC_ERR_ARG;
    *wide = wide_path(op, fmt, frame, other, f32, O) ? 1 : 0;
    return PC_OK;
}

extern "C" int pc_clips_tile_changes(const pc_cl_frame* cur, const pc_cl_frame* prev, int fmt, int upsample, int H, int W, int T, int O,
                                     int first_tile, int n_tiles, void* workspace, size_t workspace_bytes, uint64_t* out, void* stream)
{
    Geo g;
    int bpt;
    int64_t blocks;
    if (!fmt_ok(fmt) || !upsample_ok(upsample)) return PC_ERR_ARG;
    if (!geo_of(H, W, T, O, T_MAX, g) || !pair_blocks_of(T, n_tiles, T_MAX, 1, bpt, blocks)) return PC_ERR_ARG;
    if (first_tile < 0 || (int64_t)first_tile + n_tiles > (int64_t)g.ny * g.nx) return PC_ERR_ARG;
    if (!frame_ok(fmt, cur, W) || !frame_ok(fmt, prev, W)) return PC_ERR_ARG;
    if (!workspace || !aligned(workspace, 8) || !out || !aligned(out, 8)) return PC_ERR_ARG;
    if (workspace_bytes < (size_t)blocks * 3 * sizeof(u64)) return PC_ERR_ARG;
    const bool wide = wide_path(PC_CL_CHANGES, fmt, cur, prev, nullptr, O);
    const RangeGrid gr{{H, W, T, g.S, O, g.ny, g.nx}, first_tile};
    const int halo = upsample == PC_CL_LINEAR ? 1 : 0;
    u64* part = static_cast<u64*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks);
    if (fmt == PC_CL_NV12) launch_changes<uint8_t, true>(wide, grid, st, cur, prev, gr, bpt, halo, part);
    else if (fmt == PC_CL_I420) launch_changes<uint8_t, false>(wide, grid, st, cur, prev, gr, bpt, halo, part);
    else launch_changes<uint16_t, true>(wide, grid, st, cur, prev, gr, bpt, halo, part);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(final_kernel, dim3((unsigned)n_tiles), dim3(64), 0, st, part, bpt + 1, reinterpret_cast<u64*>(out));
    HIPCHK(hipGetLastError());
    return PC_OK;
}

extern "C" int pc_clips_cut_list(const pc_cl_frame* src, int fmt, int range, int upsample, float a, float b, float c, float d, int H,
                                 int W, int T, int O, const int32_t* tiles, int n, float* dst, void* stream)
{
    Geo g;
    Levels lv;
    if (!geo_of(H, W, T, O, T_MAX, g) || !upsample_ok(upsample)) return PC_ERR_ARG;
    if (!dst || !aligned(dst, 4) || !frame_ok(fmt, src, W) || !levels_of(fmt, range, lv)) return PC_ERR_ARG;
    if (!tiles || !aligned(tiles, 4) || n < 1 || n > INT32_MAX / 3) return PC_ERR_ARG;
    const int G8 = T / COLS;
    const int64_t tile_items = (int64_t)T * G8;                    // <= 2^19
    const int64_t items = (int64_t)n * tile_items, blocks = cdiv(items, NT);
    if (blocks > INT32_MAX) return PC_ERR_ARG;
    const bool wide = wide_path(PC_CL_CUT, fmt, src, nullptr, dst, O);
    const IngestCoef k{a, b, c, d};
    const int linear = upsample == PC_CL_LINEAR;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks);
    if (fmt == PC_CL_NV12) launch_cut<uint8_t, true>(wide, grid, st, src, H, W, T, g, tiles, dst, G8, (int)tile_items, items, linear, lv, k);
    else if (fmt == PC_CL_I420) launch_cut<uint8_t, false>(wide, grid, st, src, H, W, T, g, tiles, dst, G8, (int)tile_items, items, linear, lv, k);
    else launch_cut<uint16_t, true>(wide, grid, st, src, H, W, T, g, tiles, dst, G8, (int)tile_items, items, linear, lv, k);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

extern "C" const char* pc_clips_strerror(int code)
{
    switch (code) {
    case PC_OK: return "ok";
    case PC_ERR_ARG:
        return "invalid argument, unknown format, range or upsampling, geometry outside pc_clips.h, tile range outside the grid, empty "
               "tile list or workspace too small (pc_clips_changes_workspace_size)";
    case PC_ERR_HIP: return "HIP runtime error";
    default: return "unknown error";
    }
}

extern "C" int pc_clips_last_hip_error(void) { return g_last_hip.load(); }

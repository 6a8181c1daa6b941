// pc_chroma_clip_rate.hip -- the per-plane weighted squared error of decoded float tiles against the frames of a clip of YUV frames in
// any of pc_chroma.h's twelve formats and three chroma sitings, for a list of (frame slot, tile) jobs, in the frames' own codes, on
// gfx950 (pc_chroma_clip_rate.h).  Definition: DESIGN.md section 28: section 24's measure over section 25's work list.  The item is
// sse_item of image_csrc/pc_chroma_sse_item.h (the text of pc_chroma_rate.hip's); loads, levels and the per-pixel colour arithmetic
// are image_csrc/pc_yuv_device.h's, the geometry and the band numerators image_csrc/pc_tile_grid.h's, the reduction
// image_csrc/pc_reduce.h's, the code of an element and the format checks image_csrc/pc_chroma_items.h's.
//
// A work item is SY rows of one job's tile (a row pair at 4:2:0, one row at 4:2:2 and 4:4:4) by eight tile-aligned columns, with the
// 8 / SX chroma samples of those columns.  A thread takes one item, a block NT consecutive items of ONE job (T * T / (8 SY) is a
// multiple of 256 for every T that is a multiple of 64: no block straddles two jobs and none has a tail).  The block reads its job
// (slot, tile) and, where both are in range, the frame record frames[slot] from the device table: the index depends on blockIdx
// alone, so the loads are wave-uniform.  A job out of range adds nothing and reads nothing but its own two words.  An item whose rows
// and columns all lie inside the frame and whose accesses are all wide is compiled on its own (FULL); every other item goes element
// by element.  The access path only changes the load instructions, never which thread holds which sample or in which order it adds:
// the sums are the same bits on both.  Template parameters are what changes the shape of an item (element type, interleave, SX, SY,
// whether the row above is read, the access path); the depth shift, the horizontal siting and the scale are wave-uniform kernel
// arguments.  32 sse_jobs kernels and the final.  Everything that is added is an integer: a thread's sums, the wave tree, the waves of
// a block in order (12 words of LDS), then final_kernel over a job's block partials.  No atomics, no LDS on the data path.
#include "pc_image_host.h"
#include "pc_reduce.h"
#include "pc_tile_grid.h"
#include "pc_yuv_device.h"
#include "pc_chroma_items.h"
#include "pc_chroma_sse_item.h"

#include "pc_chroma_clip_rate.h"

namespace {

static_assert(PC_CCR_PLANAR == LAYOUT_PLANAR && PC_CCR_SEMIPLANAR == LAYOUT_SEMIPLANAR, "pc_chroma_items.h's layouts are pc_chroma_clip_rate.h's");
static_assert(PC_CCR_CENTRE == SITE_CENTRE && PC_CCR_COSITED == SITE_COSITED, "pc_chroma_items.h's sitings are pc_chroma_clip_rate.h's");

constexpr int T_MAX8 = 2048;             // T^4 * 255^2 < 2^60
constexpr int T_MAX10 = 1024;            // T^4 * 1023^2 < 2^60

// Block b of job m is block m * bpt + b: the items b * NT .. of the job's tile, item -> (chroma row kp, group g), tile rows SY kp ..,
// tile columns 8g .. 8g+7 (G8 = T / 8).  partials[(m * bpt + b) * 3 + p]; every block writes its three, zeros for a job out of range.
template <class T, bool IL, int SX, int SY, bool VCO, bool WIDE>
__global__ __launch_bounds__(NT) void sse_jobs_kernel(F32 x, const pc_ccr_frame* __restrict__ frames, int n_frames,
                                                      const int32_t* __restrict__ jobs, Grid gr, int G8, int bpt, Measure ms, Levels lv,
                                                      EmitCoef k, u64* __restrict__ partials)
{
    const int m = (int)(blockIdx.x / (unsigned)bpt), b = (int)(blockIdx.x - (unsigned)m * (unsigned)bpt);
    const int slot = jobs[2 * (int64_t)m], tile = jobs[2 * (int64_t)m + 1];
    u64 su[3] = {0ull, 0ull, 0ull};
    if (slot >= 0 && slot < n_frames && tile >= 0 && tile < gr.ny * gr.nx) {  // block-uniform: the barrier of the reduction is outside
        const Planes<const T> ref = planes_of<const T>(frames + slot);
        const int i = tile / gr.nx, j = tile - i * gr.nx;
        const int S = gr.S, O = gr.O, den = O > 0 ? 2 * O : 1;
        const int Yt = i * S, Xt = j * S;                         // the tile's first row and column in the frame: < H, < W
        const int hh = min(gr.T, gr.H - Yt), ww = min(gr.T, gr.W - Xt);
        const int rem = b * NT + (int)threadIdx.x;                // < T * T / 8 <= 2^19
        const int kp = rem / G8, r0 = SY * kp, q0 = COLS * (rem - kp * G8);
        if (r0 < hh && q0 < ww) {
            const int rows = min(SY, hh - r0), hi = min(COLS, ww - q0);
            unsigned ay[SY], ax[COLS];
#pragma unroll
            for (int r = 0; r < SY; ++r) ay[r] = axis_weight(i, gr.ny, r0 + r, S, O, den);
#pragma unroll
            for (int q = 0; q < COLS; ++q) ax[q] = axis_weight(j, gr.nx, q0 + q, S, O, den);
            const float* xt = x.p + (int64_t)m * x.st;
            if (WIDE && rows == SY && hi == COLS)
                sse_item<T, IL, SX, SY, VCO, true>(xt, x.sc, x.sh, r0, q0, rows, hi, ref, (int64_t)Yt + r0, (int64_t)Xt + q0, ms, lv, k, ay, ax, su);
            else
                sse_item<T, IL, SX, SY, VCO, false>(xt, x.sc, x.sh, r0, q0, rows, hi, ref, (int64_t)Yt + r0, (int64_t)Xt + q0, ms, lv, k, ay, ax, su);
        }
    }
    block_reduce<Sum>(su, partials + (int64_t)blockIdx.x * 3);
}

// One wave per job: its bpt block partials, lane l taking l, l + 64, ..., then the wave tree.
__global__ __launch_bounds__(64) void final_kernel(const u64* __restrict__ p, int bpt, u64* __restrict__ out)
{
    row_final<Sum, 3>(p, bpt, out);
}

// -- host ----------------------------------------------------------------------------------------------------------------------------

// The item space: SY rows by eight columns, T * T / (8 SY) items to a job, NT to a block.  Blocks per job and blocks in all; false
// for what the calls refuse.
bool item_blocks_of(int T, int sy, int n_jobs, int t_max, int& bpt, int64_t& blocks)
{
    if (T < 64 || T % 64 || T > t_max || (sy != 1 && sy != 2) || n_jobs < 1) return false;
    bpt = (int)((int64_t)T * T / ((int64_t)sy * COLS * NT));
    blocks = (int64_t)n_jobs * bpt;
    return blocks <= INT32_MAX;
}

// The one place that decides the access path: the call launches from it, pc_chroma_clip_rate_plan reports it.  Once per call: every
// frame of the table has to allow it, whichever the jobs name.
bool wide_path(const void* x, int64_t st, int64_t sc, int64_t sh, int O, bool il, int es, int sx, const pc_ccr_frame* frames, int n_frames)
{
    if (!f32_wide(x, st, sc, sh) || (sx == 2 && O % 8 != 0)) return false;
    for (int f = 0; f < n_frames; ++f) {
        const pc_ccr_frame* ref = frames + f;
        if (!plane_wide(ref->y, ref->y_row, es) || !plane_wide(ref->u, ref->u_row, es)) return false;
        if (!il && !plane_wide(ref->v, ref->v_row, es)) return false;
    }
    return true;
}

}  // namespace

extern "C" size_t pc_chroma_clip_rate_workspace_size(int T, int sy, int n_jobs)
{
    int bpt;
    int64_t blocks;
    return item_blocks_of(T, sy, n_jobs, T_MAX8, bpt, blocks) ? (size_t)blocks * 3 * sizeof(u64) : 0;
}

extern "C" int pc_chroma_clip_rate_plan(const void* x, int64_t sxt, int64_t sxc, int64_t sxh, int O, int layout, int bits, int sx,
                                        const pc_ccr_frame* frames_host, int n_frames, int* wide)
{
    Fmt fm;
    if (!x || !wide || !format_of(layout, bits, 0, sx, 1, fm) || O < 0 || !frames_host || n_frames < 1) return PC_ERR_ARG;
    for (int f = 0; f < n_frames; ++f)
        if (!(frames_host[f].y && frames_host[f].u && (fm.il || frames_host[f].v))) return PC_ERR_ARG;
    *wide = wide_path(x, sxt, sxc, sxh, O, fm.il, bits == 10 ? 2 : 1, sx, frames_host, n_frames) ? 1 : 0;
    return PC_OK;
}

extern "C" int pc_chroma_clip_rate_sse_jobs(const float* x, int64_t sxt, int64_t sxc, int64_t sxh, int H, int W, int T, int O, int layout,
                                            int bits, int shift, int sx, int sy, int hsite, int vsite, int range, float kr, float kg,
                                            float kb, float ib, float ir, const pc_ccr_frame* frames_host, const pc_ccr_frame* frames_dev,
                                            int n_frames, const int32_t* jobs, int n_jobs, void* workspace, size_t workspace_bytes,
                                            uint64_t* out, void* stream)
{
    Geo g;
    Levels lv;
    Fmt fm;
    int bpt;
    int64_t blocks;
    if (!format_of(layout, bits, shift, sx, sy, fm) || !site_ok(hsite) || !site_ok(vsite) || !depth_levels(bits, range, lv)) return PC_ERR_ARG;
    if (!geo_of(H, W, T, O, bits == 10 ? T_MAX10 : T_MAX8, g) || !item_blocks_of(T, sy, n_jobs, T_MAX8, bpt, blocks)) return PC_ERR_ARG;
    if (!x || !aligned(x, 4) || sxh < T || sxc < 1 || sxt < 1) return PC_ERR_ARG;
    if (!frames_host || !frames_dev || !aligned(frames_dev, 8) || n_frames < 1) return PC_ERR_ARG;
    for (int f = 0; f < n_frames; ++f)
        if (!picture_ok(fm, frames_host + f, W)) return PC_ERR_ARG;
    if (!jobs || !aligned(jobs, 4)) return PC_ERR_ARG;
    if (!workspace || !aligned(workspace, 8) || !out || !aligned(out, 8)) return PC_ERR_ARG;
    if (workspace_bytes < (size_t)blocks * 3 * sizeof(u64)) return PC_ERR_ARG;
    const bool hco = sx == 2 && hsite == PC_CCR_COSITED, vco = sy == 2 && vsite == PC_CCR_COSITED;
    const bool wide = wide_path(x, sxt, sxc, sxh, O, fm.il, bits == 10 ? 2 : 1, sx, frames_host, n_frames);
    const F32 xv{x, sxt, sxc, sxh};
    const Grid gr{H, W, T, g.S, O, g.ny, g.nx};
    const EmitCoef k{kr, kg, kb, ib, ir};
    const Measure ms{hco ? 1 : 0, 1.f / (float)((sx == 2 ? (hco ? 4 : 2) : 1) * (sy == 2 ? (vco ? 4 : 2) : 1)), shift};
    u64* part = static_cast<u64*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks);
    with_format(fm, [&](auto el, auto il, auto SX, auto SY) {
        using T_ = decltype(el);
#define PC_SSE(VCO, WIDE)                                                                                                                   \
    hipLaunchKernelGGL((sse_jobs_kernel<T_, il.value, SX.value, SY.value, VCO, WIDE>), grid, dim3(NT), 0, st, xv, frames_dev, n_frames, jobs, gr, \
                       T / COLS, bpt, ms, lv, k, part)
        // VCO is instantiated for SY = 2 alone: at SY = 1 both branches below name the same kernel
        if (wide) {
            if (SY.value == 2 && vco) PC_SSE((SY.value == 2), true); else PC_SSE(false, true);
        } else {
            if (SY.value == 2 && vco) PC_SSE((SY.value == 2), false); else PC_SSE(false, false);
        }
#undef PC_SSE
    });
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(final_kernel, dim3((unsigned)n_jobs), dim3(64), 0, st, part, bpt, reinterpret_cast<u64*>(out));
    HIPCHK(hipGetLastError());
    return PC_OK;
}

extern "C" const char* pc_chroma_clip_rate_strerror(int code)
{
    switch (code) {
    case PC_OK: return "ok";
    case PC_ERR_ARG:
        return "invalid argument, unknown layout, depth, shift, subsampling, siting or range, geometry outside pc_chroma_clip_rate.h, an "
               "empty frame table or job list or workspace too small (pc_chroma_clip_rate_workspace_size)";
    case PC_ERR_HIP: return "HIP runtime error";
    default: return "unknown error";
    }
}

extern "C" int pc_chroma_clip_rate_last_hip_error(void) { return g_last_hip.load(); }

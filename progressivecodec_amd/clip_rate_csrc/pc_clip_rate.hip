// pc_clip_rate.hip -- the per-plane weighted squared error of decoded float tiles against the frames of a clip of YUV 4:2:0 frames
// (NV12 / I420 / P010), for a list of (frame slot, tile) jobs, in the frames' own codes, on gfx950 (pc_clip_rate.h).  Definition:
// section 15's measure over section 16's work list; the item is sse_tile of image_csrc/pc_yuv_items.h, as in pc_frame_rate.hip; the
// reduction is image_csrc/pc_reduce.h's.
//
// A work item is one ROW PAIR (2k, 2k+1) of one job's tile by eight tile-aligned columns: sixteen luma codes and the four chroma pairs
// that are the means of the 2 x 2 cells the thread holds.  A thread takes one item, a block NT consecutive items of ONE job
// (T * T / 16 is a multiple of 256 for every T that is a multiple of 64: no block straddles two jobs and none has a tail).  The block
// reads its job (slot, tile) and, where both are in range, the frame record frames[slot] from the device table: the index depends
// on blockIdx alone, so the loads are wave-uniform.  A job out of range adds nothing and reads nothing but its own two words.  An
// item whose rows and columns all lie inside the frame and whose accesses are all wide is compiled on its own (FULL); every other
// item goes element by element, its edge cells clamped as the contract says.  The access path only changes the load instructions,
// never which thread holds which sample: the sums are the same bits on both.  Everything that is added is an integer: a thread's
// sums, the wave tree, the waves of a block in order (12 words of LDS), then final_kernel over a job's block partials.  No atomics,
// no LDS on the data path.
#include "pc_image_host.h"
#include "pc_reduce.h"
#include "pc_tile_grid.h"
#include "pc_yuv_device.h"
#include "pc_yuv_items.h"

#include "pc_clip_rate.h"

namespace {

constexpr int T_MAX8 = 2048;             // T^4 * 255^2 < 2^60
constexpr int T_MAX10 = 1024;            // T^4 * 1023^2 < 2^60

// Block b of job m is block m * bpt + b: the items b * NT .. of the job's tile, item -> (row pair k, group g), tile rows 2k and
// 2k + 1, tile columns 8g .. 8g+7.  partials[(m * bpt + b) * 3 + p]; every block writes its three, zeros for a job out of range.
template <class T, bool IL, bool WIDE>
__global__ __launch_bounds__(NT) void sse_jobs_kernel(F32 x, const pc_cr_frame* __restrict__ frames, int n_frames,
                                                      const int32_t* __restrict__ jobs, Grid gr, int G8, int bpt, Levels lv, EmitCoef k,
                                                      u64* __restrict__ partials)
{
    const int m = (int)(blockIdx.x / (unsigned)bpt), b = (int)(blockIdx.x - (unsigned)m * (unsigned)bpt);
    const int slot = jobs[2 * (int64_t)m], tg = jobs[2 * (int64_t)m + 1];
    u64 su[3] = {0ull, 0ull, 0ull};
    if (slot >= 0 && slot < n_frames && tg >= 0 && tg < gr.ny * gr.nx)        // block-uniform: the barrier of the reduction is outside
        sse_tile<T, IL, WIDE>(x.p + (int64_t)m * x.st, x.sc, x.sh, planes_of<const T>(frames + slot), gr, tg, b, G8, lv, k, su);
    block_reduce<Sum>(su, partials + (int64_t)blockIdx.x * 3);
}

// One wave per job: its bpt block partials, lane l taking l, l + 64, ..., then the wave tree.
__global__ __launch_bounds__(64) void final_kernel(const u64* __restrict__ p, int bpt, u64* __restrict__ out)
{
    row_final<Sum, 3>(p, bpt, out);
}

// The one place that decides the access path: the call launches from it, pc_clip_rate_plan reports it.  Once per call: every frame
// of the table has to allow it, whichever the jobs name.
bool wide_path(const void* x, int64_t st, int64_t sc, int64_t sh, int O, int fmt, const pc_cr_frame* frames, int n_frames)
{
    if (!f32_wide(x, st, sc, sh) || O % 8) return false;
    for (int f = 0; f < n_frames; ++f)
        if (!frame_wide(fmt, frames + f)) return false;
    return true;
}

template <class T, bool IL>
void launch(bool wide, dim3 grid, hipStream_t st, const F32& x, const pc_cr_frame* frames, int n_frames, const int32_t* jobs, const Grid& gr,
            int bpt, const Levels& lv, const EmitCoef& k, u64* part)
{
    if (wide)
        hipLaunchKernelGGL((sse_jobs_kernel<T, IL, true>), grid, dim3(NT), 0, st, x, frames, n_frames, jobs, gr, gr.T / COLS, bpt, lv, k, part);
    else
        hipLaunchKernelGGL((sse_jobs_kernel<T, IL, false>), grid, dim3(NT), 0, st, x, frames, n_frames, jobs, gr, gr.T / COLS, bpt, lv, k, part);
}

}  // namespace

extern "C" size_t pc_clip_rate_workspace_size(int T, int n_jobs)
{
    int bpt;
    int64_t blocks;
    return pair_blocks_of(T, n_jobs, T_MAX8, 0, bpt, blocks) ? (size_t)blocks * 3 * sizeof(u64) : 0;
}

extern "C" int pc_clip_rate_plan(const void* x, int64_t sxt, int64_t sxc, int64_t sxh, int O, int fmt, const pc_cr_frame* frames_host,
                                 int n_frames, int* wide)
{
    if (!x || !wide || !fmt_ok(fmt) || O < 0 || !frames_host || n_frames < 1) return PC_ERR_ARG;
    for (int f = 0; f < n_frames; ++f)
        if (!planes_set(fmt, frames_host + f)) return PC_ERR_ARG;
    *wide = wide_path(x, sxt, sxc, sxh, O, fmt, frames_host, n_frames) ? 1 : 0;
    return PC_OK;
}

extern "C" int pc_clip_rate_sse_jobs(const float* x, int64_t sxt, int64_t sxc, int64_t sxh, int H, int W, int T, int O, int fmt, int range,
                                     float kr, float kg, float kb, float ib, float ir, const pc_cr_frame* frames_host,
                                     const pc_cr_frame* frames_dev, int n_frames, const int32_t* jobs, int n_jobs, void* workspace,
                                     size_t workspace_bytes, uint64_t* out, void* stream)
{
    Geo g;
    Levels lv;
    int bpt;
    int64_t blocks;
    if (!fmt_ok(fmt) || !levels_of(fmt, range, lv)) return PC_ERR_ARG;
    if (!geo_of(H, W, T, O, fmt == PC_CR_P010 ? T_MAX10 : T_MAX8, g) || !pair_blocks_of(T, n_jobs, T_MAX8, 0, bpt, blocks)) return PC_ERR_ARG;
    if (!x || !aligned(x, 4) || sxh < T || sxc < 1 || sxt < 1) return PC_ERR_ARG;
    if (!frames_host || !frames_dev || !aligned(frames_dev, 8) || n_frames < 1) return PC_ERR_ARG;
    for (int f = 0; f < n_frames; ++f)
        if (!frame_ok(fmt, frames_host + f, W)) return PC_ERR_ARG;
    if (!jobs || !aligned(jobs, 4)) return PC_ERR_ARG;
    if (!workspace || !aligned(workspace, 8) || !out || !aligned(out, 8)) return PC_ERR_ARG;
    if (workspace_bytes < (size_t)blocks * 3 * sizeof(u64)) return PC_ERR_ARG;
    const bool wide = wide_path(x, sxt, sxc, sxh, O, fmt, frames_host, n_frames);
    const F32 xv{x, sxt, sxc, sxh};
    const Grid gr{H, W, T, g.S, O, g.ny, g.nx};
    const EmitCoef k{kr, kg, kb, ib, ir};
    u64* part = static_cast<u64*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks);
    if (fmt == PC_CR_NV12) launch<uint8_t, true>(wide, grid, st, xv, frames_dev, n_frames, jobs, gr, bpt, lv, k, part);
    else if (fmt == PC_CR_I420) launch<uint8_t, false>(wide, grid, st, xv, frames_dev, n_frames, jobs, gr, bpt, lv, k, part);
    else launch<uint16_t, true>(wide, grid, st, xv, frames_dev, n_frames, jobs, gr, bpt, lv, k, part);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(final_kernel, dim3((unsigned)n_jobs), dim3(64), 0, st, part, bpt, reinterpret_cast<u64*>(out));
    HIPCHK(hipGetLastError());
    return PC_OK;
}

extern "C" const char* pc_clip_rate_strerror(int code)
{
    switch (code) {
    case PC_OK: return "ok";
    case PC_ERR_ARG:
        return "invalid argument, unknown format or range, geometry outside pc_clip_rate.h, an empty frame table or job list or workspace "
               "too small (pc_clip_rate_workspace_size)";
    case PC_ERR_HIP: return "HIP runtime error";
    default: return "unknown error";
    }
}

extern "C" int pc_clip_rate_last_hip_error(void) { return g_last_hip.load(); }

// pc_chroma_clip_tol.hip -- the tolerant scan of a clip of YUV frames of any of pc_chroma.h's twelve formats and three chroma sitings
// on gfx950 (pc_chroma_clip_tol.h): per frame and tile the difference of the tile's footprint against the frame the tile was last
// coded in (count, sum of squared differences, largest absolute difference, per plane), and the decision to reuse or recode, taken on
// the device.  Definition: DESIGN.md section 29, on top of sections 18 (the tolerance, closeness, the scan), 25 (geometry, footprint)
// and 17 (the device frame table); what pc_clip_tol.hip is for NV12 / I420 / P010 with centre-sited chroma.  The item and the halo
// block are compare_chroma_tile of image_csrc/pc_chroma_compare.h with this library's accumulate policy (Stats), the reduction is
// image_csrc/pc_reduce.h's, the code of an element and the format checks image_csrc/pc_chroma_items.h's.
//
// Step k is two launches.  diff_kernel: a work item is SY luma rows of one tile (a row pair at 4:2:0, one row at 4:2:2 and 4:4:4) by
// eight tile-aligned luma columns, with the 8 / SX chroma samples of its cells, in frame k and in the tile's anchor.  A thread takes
// one item, a block NT consecutive items of ONE tile (T * T / (8 SY) is a multiple of 256 for every T that is a multiple of 64: no
// block straddles two tiles and none has a tail).  The block reads anchor[t] and, where it lies in [0, k), the two frame records
// frames[k] and frames[anchor[t]]: the indices depend on blockIdx alone, so the loads are wave-uniform.  One more block per tile
// takes the halo ring element by element, a side only where the footprint rule has a halo on it (four wave-uniform flags, computed on
// the host from the format, the siting and the upsampling) and the frame has the samples.  An item whose rows and columns all lie
// inside the frame and whose accesses are all wide is compiled on its own (FULL); every other item goes element by element.  A thread
// carries nine accumulators (count, sse, maxabs of three planes); they go thread -> wave tree -> the block's four waves in order (36
// words of LDS, inside pc_reduce.h) -> one 72-byte partial per block, by sum, sum and max.  decide_kernel: one wave per tile over its
// partials; lane 0 writes stats[k][t], computes nsamp from the per-axis rule, applies the rule and writes source[k][t] and
// anchor[t].  Stream order makes step k + 1 see step k's anchors.  Everything is an integer: the result depends neither on order nor
// on access path.  No atomics, no LDS on the data path.  Template parameters are what changes an item's shape: element type,
// interleave, (SX, SY) and the access path; the depth shift and the halo flags are wave-uniform kernel arguments.
// 24 diff kernels, the decide kernel and the init kernel.
#include "pc_image_host.h"
#include "pc_reduce.h"
#include "pc_tile_grid.h"
#include "pc_yuv_device.h"
#include "pc_chroma_items.h"
#include "pc_chroma_compare.h"

#include "pc_chroma_clip_tol.h"

namespace {

static_assert(PC_CCT_PLANAR == LAYOUT_PLANAR && PC_CCT_SEMIPLANAR == LAYOUT_SEMIPLANAR, "pc_chroma_items.h's layouts are pc_chroma_clip_tol.h's");
static_assert(PC_CCT_CENTRE == SITE_CENTRE && PC_CCT_COSITED == SITE_COSITED, "pc_chroma_items.h's sitings are pc_chroma_clip_tol.h's");

constexpr int T_MAX = 2048;              // T^2 * 1023^2 < 2^43: a 4:4:4 chroma footprint has at most T^2 samples, as the luma one
constexpr int NACC = 9;                  // [plane][count, sse, maxabs]

struct Tol {
    unsigned max_abs[3], mse_q10[3];
    int max_run;
};

// compare_chroma_tile's policy.  One sample of plane p into a thread's accumulators: ac[3p] count, ac[3p + 1] sse, ac[3p + 2] maxabs.
// A thread holds at most 16 samples of a plane in an item (SY * 8 of luma: 16 at 4:2:0, 8 otherwise; 8 / SX of Cb and of Cr), or 17
// of a halo ring (4:2:0: 2 * 1026 + 2 * 1024 samples over 256 threads; 4:2:2: one run of 2 * 2048): 17 * 1023^2 < 2^25.
static_assert(17ull * 1023 * 1023 < (1ull << 25), "a thread's sums");
static_assert(2 * (T_MAX / 2 + 2) + 2 * (T_MAX / 2) <= 17 * NT && 2 * T_MAX <= 16 * NT && 2 * COLS <= 17, "at most 17 samples of a plane per thread");
struct Stats {
    static constexpr int N = NACC;
    template <class T>
    static __device__ __forceinline__ void take(unsigned a, unsigned b, int p, const Halo& ha, unsigned (&ac)[NACC])
    {
        const int e = (int)code_of<T>(a, ha.sh, ha.mask) - (int)code_of<T>(b, ha.sh, ha.mask);
        const unsigned d = (unsigned)(e < 0 ? -e : e);
        ac[3 * p] += d ? 1u : 0u;
        ac[3 * p + 1] += d * d;
        ac[3 * p + 2] = max(ac[3 * p + 2], d);
    }
    template <class V>
    static __device__ __forceinline__ V op(int c, V a, V b) { return c % 3 == 2 ? max(a, b) : a + b; }   // sum, sum, max
};

// The first launch of step k.  Blocks t * (bpt + 1) .. + bpt - 1 hold the items of tile t: item -> (chroma row kp, group g), tile
// rows SY kp .. SY kp + SY - 1, tile columns 8g .. 8g+7; block t * (bpt + 1) + bpt holds its halo ring.
// partials[blockIdx.x * 9 + 3p + c]; every block writes its nine, zeros where the anchor lies outside [0, k).
template <class T, bool IL, int SX, int SY, bool WIDE>
__global__ __launch_bounds__(NT) void diff_kernel(const pc_cct_frame* __restrict__ frames, int k, const int32_t* __restrict__ anchor, Grid gr,
                                                  int G8, int bpt, Halo ha, u64* __restrict__ partials)
{
    const int bpt1 = bpt + 1;
    const int t = (int)(blockIdx.x / (unsigned)bpt1), bl = (int)(blockIdx.x - (unsigned)t * (unsigned)bpt1);
    const int an = anchor[t];
    unsigned ac[NACC];
#pragma unroll
    for (int c = 0; c < NACC; ++c) ac[c] = 0u;
    if (an >= 0 && an < k)                                        // block-uniform: the barrier of the reduction is outside
        compare_chroma_tile<T, IL, SX, SY, WIDE, Stats>(planes_of<const T>(frames + k), planes_of<const T>(frames + an), gr, t, bl, bpt, G8, ha, ac);
    // a wave holds at most 64 * 17 samples of a plane: 64 * 2^25 = 2^31; 64-bit from the block on
    block_reduce<Stats>(ac, partials + (int64_t)blockIdx.x * NACC);
}

// samples of tile i's footprint along an axis: (luma, chroma); sub: the axis is subsampled, lo and hi its halo flags
__device__ __forceinline__ void axis_samples(int i, int L, int T, int S, bool sub, int lo, int hi, int& nl, int& nc)
{
    const int y0 = i * S, e = min(y0 + T, L), Lc = (L + 1) >> 1;
    const int c0 = max((y0 >> 1) - lo, 0), c1 = min(((e + 1) >> 1) - 1 + hi, Lc - 1);
    nl = e - y0;
    nc = sub ? c1 - c0 + 1 : nl;
}

// The second launch of step k.  One wave per tile: its nb block partials, lane l taking l, l + 64, ..., then the wave tree; lane 0
// writes the tile's nine numbers, decides, and writes source[k][t] and anchor[t].  src and st: row k of source and stats.
__global__ __launch_bounds__(64) void decide_kernel(const u64* __restrict__ p, int nb, int k, Grid gr, int subx, int suby, Halo ha, Tol tol,
                                                    int32_t* __restrict__ anchor, int32_t* __restrict__ src, u64* __restrict__ st)
{
    const int64_t t = blockIdx.x;
    u64 ac[NACC];
#pragma unroll
    for (int c = 0; c < NACC; ++c) ac[c] = 0ull;
    gather_partials<Stats>(p, t, nb, (int)threadIdx.x, 64, ac);
    wave_reduce<Stats>(ac);
    if (threadIdx.x == 0) {
        const int an = anchor[t];
        bool reuse = an >= 0 && an < k;                           // outside: the first launch added nothing, the nine are zero
#pragma unroll
        for (int c = 0; c < NACC; ++c) st[t * NACC + c] = ac[c];
        const int i = (int)t / gr.nx, j = (int)t - i * gr.nx;
        int hl, hc, wl, wc;
        axis_samples(i, gr.H, gr.T, gr.S, suby != 0, ha.ylo, ha.yhi, hl, hc);
        axis_samples(j, gr.W, gr.T, gr.S, subx != 0, ha.xlo, ha.xhi, wl, wc);
        const u64 nsamp[3] = {(u64)hl * (u64)wl, (u64)hc * (u64)wc, (u64)hc * (u64)wc};
#pragma unroll
        for (int q = 0; q < 3; ++q)                               // 1024 * sse < 2^53, mse_q10 * nsamp <= 2^30 * 2^22
            reuse = reuse && ac[3 * q + 2] <= (u64)tol.max_abs[q] && 1024ull * ac[3 * q + 1] <= (u64)tol.mse_q10[q] * nsamp[q];
        reuse = reuse && (tol.max_run == 0 || k - an + 1 <= tol.max_run);
        src[t] = reuse ? an : k;
        if (!reuse) anchor[t] = k;
    }
}

// Row 0 and the anchors: source[0][t] = 0, stats[0][t] = 0, anchor[t] = 0.
__global__ __launch_bounds__(NT) void init_kernel(int n, int32_t* __restrict__ anchor, int32_t* __restrict__ src, u64* __restrict__ st)
{
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i < n) {
        anchor[i] = 0;
        src[i] = 0;
    }
    if (i < (int64_t)n * NACC) st[i] = 0ull;
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

// the partials, then the anchors
size_t workspace_of(int64_t blocks, int n_tiles)
{
    return (size_t)((blocks * NACC * (int64_t)sizeof(u64) + (int64_t)n_tiles * 4 + 7) / 8 * 8);
}

bool planes_given(bool il, const pc_cct_frame* f) { return f->y && f->u && (il || f->v); }

// every plane pointer on four elements, every row stride a multiple of 4
bool picture_wide(bool il, int es, const pc_cct_frame* f)
{
    if (!plane_wide(f->y, f->y_row, es) || !plane_wide(f->u, f->u_row, es)) return false;
    return il || plane_wide(f->v, f->v_row, es);
}

}  // namespace

extern "C" size_t pc_chroma_clip_tol_workspace_size(int T, int sy, int n_tiles)
{
    int bpt;
    int64_t blocks;
    return item_blocks_of(T, sy, n_tiles, bpt, blocks) ? workspace_of(blocks, n_tiles) : 0;
}

// The one place that decides the access path: the scan launches from it.  Once per call: every frame of the table has to allow it.
extern "C" int pc_chroma_clip_tol_plan(int layout, int bits, int sx, const pc_cct_frame* frames_host, int n_frames, int O, int* wide)
{
    Fmt fm;
    if (!format_of(layout, bits, 0, sx, 1, fm) || !wide || O < 0 || !frames_host || n_frames < 1) return PC_ERR_ARG;
    for (int f = 0; f < n_frames; ++f)
        if (!planes_given(fm.il, frames_host + f)) return PC_ERR_ARG;
    int w = (sx == 2 && O % 8) ? 0 : 1;
    for (int f = 0; f < n_frames && w; ++f)
        if (!picture_wide(fm.il, bits == 10 ? 2 : 1, frames_host + f)) w = 0;
    *wide = w;
    return PC_OK;
}

extern "C" int pc_chroma_clip_tol_scan(const pc_cct_frame* frames_host, const pc_cct_frame* frames_dev, int n_frames, int layout, int bits,
                                       int shift, int sx, int sy, int hsite, int vsite, int upsample, int H, int W, int T, int O,
                                       const int* max_abs, const int* mse_q10, int max_run, void* workspace, size_t workspace_bytes,
                                       int32_t* source, uint64_t* stats, void* stream)
{
    Geo g;
    Fmt fm;
    int bpt;
    int64_t blocks;
    if (!format_of(layout, bits, shift, sx, sy, fm) || !site_ok(hsite) || !site_ok(vsite) || !upsample_ok(upsample)) return PC_ERR_ARG;
    if (!geo_of(H, W, T, O, T_MAX, g)) return PC_ERR_ARG;
    const int n = g.ny * g.nx;
    if (!item_blocks_of(T, sy, n, bpt, blocks)) return PC_ERR_ARG;         // one more block per tile: the halo ring
    if (!frames_host || !frames_dev || !aligned(frames_dev, 8) || n_frames < 1) return PC_ERR_ARG;
    for (int f = 0; f < n_frames; ++f)
        if (!picture_ok(fm, frames_host + f, W)) return PC_ERR_ARG;
    if (!max_abs || !mse_q10 || max_run < 0) return PC_ERR_ARG;
    const int top = (1 << bits) - 1;
    Tol tol;
    for (int p = 0; p < 3; ++p) {
        if (max_abs[p] < 0 || max_abs[p] > top || mse_q10[p] < 0 || mse_q10[p] > PC_CCT_NO_MSE) return PC_ERR_ARG;
        tol.max_abs[p] = (unsigned)max_abs[p];
        tol.mse_q10[p] = (unsigned)mse_q10[p];
    }
    tol.max_run = max_run;
    if (!workspace || !aligned(workspace, 8) || workspace_bytes < workspace_of(blocks, n)) return PC_ERR_ARG;
    if (!source || !aligned(source, 4) || !stats || !aligned(stats, 8)) return PC_ERR_ARG;
    if ((int64_t)n * NACC > INT32_MAX) return PC_ERR_ARG;
    int w = 0;
    if (pc_chroma_clip_tol_plan(layout, bits, sx, frames_host, n_frames, O, &w) != PC_OK) return PC_ERR_ARG;
    const bool wide = w != 0;
    const Grid gr{H, W, T, g.S, O, g.ny, g.nx};
    const Halo ha = halo_of(sx, sy, hsite == PC_CCT_CENTRE, vsite == PC_CCT_CENTRE, upsample == PC_CCT_LINEAR, shift, bits);
    u64* part = static_cast<u64*>(workspace);
    int32_t* anchor = reinterpret_cast<int32_t*>(part + blocks * NACC);
    u64* st64 = reinterpret_cast<u64*>(stats);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(init_kernel, dim3((unsigned)cdiv((int64_t)n * NACC, NT)), dim3(NT), 0, st, n, anchor, source, st64);
    HIPCHK(hipGetLastError());
    const dim3 grid((unsigned)blocks);
    for (int k = 1; k < n_frames; ++k) {
        with_format(fm, [&](auto el, auto il, auto SX, auto SY) {
            using T_ = decltype(el);
            if (wide)
                hipLaunchKernelGGL((diff_kernel<T_, il.value, SX.value, SY.value, true>), grid, dim3(NT), 0, st, frames_dev, k, anchor, gr, T / COLS,
                                   bpt, ha, part);
            else
                hipLaunchKernelGGL((diff_kernel<T_, il.value, SX.value, SY.value, false>), grid, dim3(NT), 0, st, frames_dev, k, anchor, gr, T / COLS,
                                   bpt, ha, part);
        });
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(decide_kernel, dim3((unsigned)n), dim3(64), 0, st, part, bpt + 1, k, gr, sx == 2 ? 1 : 0, sy == 2 ? 1 : 0, ha, tol, anchor,
                           source + (int64_t)k * n, st64 + (int64_t)k * n * NACC);
        HIPCHK(hipGetLastError());
    }
    return PC_OK;
}

extern "C" const char* pc_chroma_clip_tol_strerror(int code)
{
    switch (code) {
    case PC_OK: return "ok";
    case PC_ERR_ARG:
        return "invalid argument, unknown layout, depth, shift, subsampling, siting or upsampler, geometry outside pc_chroma_clip_tol.h, an "
               "empty frame table, a tolerance outside its ranges or workspace too small (pc_chroma_clip_tol_workspace_size)";
    case PC_ERR_HIP: return "HIP runtime error";
    default: return "unknown error";
    }
}

extern "C" int pc_chroma_clip_tol_last_hip_error(void) { return g_last_hip.load(); }

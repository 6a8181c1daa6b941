// pc_clip_tol_rate.hip -- the per-plane weighted squared error of decoded float tiles against EVERY frame of the run each is shown in,
// for a clip of YUV 4:2:0 frames (NV12 / I420 / P010), in the frames' own codes, on gfx950 (pc_clip_tol_rate.h).  Definition: DESIGN.md
// section 20: section 17's measure, entry by entry, for the runs of section 18's source table.  The shared pieces -- plane loads,
// levels, emit_px, emit_chroma, band numerators, wave tree, the final -- are image_csrc's; the run item has one user and lives here.
//
// A work item is sse_tile's (image_csrc/pc_yuv_items.h): one ROW PAIR (2k, 2k+1) of one job's tile by eight tile-aligned columns, sixteen
// luma codes and the four chroma pairs that are the means of the 2 x 2 cells the thread holds.  A thread takes one item, a block NT
// consecutive items of ONE job.  The item has two halves:
//   emit     once per job: the 3 x 2 x 8 floats -> 16 luma codes and 4 + 4 chroma codes, the same single IEEE operations in the same
//            order as sse_item, and the band numerators ay, ax.  All of it stays in registers, the codes two to a register.
//   compare  once per entry of the job: the frame's 16 luma and 8 chroma codes against the held ones, the three weighted sums formed
//            as sse_item forms them (the same integer types, the same clamped edge cells), the wave tree, and lane 0 of each wave
//            writes the wave's three sums: partials[(e * bpt + b) * 4 + wave][3].
// The block reads its job's tile and entry range, and per entry the slot and the frame record, by indices that depend on blockIdx and
// the loop counter alone: wave-uniform loads.  A job whose tile is out of range and an entry whose slot is out of range write zeros
// and read no frame, so every partial of every entry is written.  The loop has no barrier and the kernel no LDS.  An item whose rows
// and columns all lie inside the frame and whose accesses are all wide is compiled on its own (FULL), in both halves; every other
// item goes element by element.  The access path only changes the load instructions, never the sums.  Everything that is added is an
// integer.  No atomics.
#include "pc_image_host.h"
#include "pc_reduce.h"
#include "pc_tile_grid.h"
#include "pc_yuv_device.h"
#include "pc_yuv_items.h"

#include "pc_clip_tol_rate.h"

namespace {

constexpr int T_MAX8 = 2048;             // T^4 * 255^2 < 2^60
constexpr int T_MAX10 = 1024;            // T^4 * 1023^2 < 2^60
constexpr int WAVES = NT / 64;

// What an item holds across the entries of its job: codes two to a register (each fits 10 bits), low half first.
struct Held {
    unsigned yq[2][COLS / 2];            // [row][column pair]
    unsigned cb[2], cr[2];               // [sample pair]
    unsigned ay[2], ax[COLS];
};

// The emit half: rows r0, r0 + 1 and columns q0 .. q0+7 of the tile at xt, of which `rows` rows and the lanes 0 .. hi-1 lie inside
// the frame; a row or column beyond the frame stands in as the last one inside it, as in sse_item.  FULL: rows == 2, hi == 8 and
// every access is wide.
template <bool FULL>
__device__ __forceinline__ void run_emit(const float* xt, int64_t sc, int64_t sh, int r0, int q0, int rows, int hi, const Levels& lv,
                                         const EmitCoef& k, Held& h)
{
    unsigned yq[2][COLS];
    float ub[2][COLS], ur[2][COLS];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        float v[3][COLS];
        const int rr = FULL ? r : min(r, rows - 1);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            // r0 + 1 < T <= sh and q0 + 7 < T: the row pair and the eight floats lie inside the tile whatever the frame's edge
            const float* s = xt + ch * sc + (int64_t)(r0 + rr) * sh + q0;
            if (FULL) {
                const float4 f0 = *reinterpret_cast<const float4*>(s), f1 = *reinterpret_cast<const float4*>(s + 4);
                v[ch][0] = f0.x; v[ch][1] = f0.y; v[ch][2] = f0.z; v[ch][3] = f0.w;
                v[ch][4] = f1.x; v[ch][5] = f1.y; v[ch][6] = f1.z; v[ch][7] = f1.w;
            } else {
#pragma unroll
                for (int q = 0; q < COLS; ++q) v[ch][q] = s[min(q, hi - 1)];
            }
        }
#pragma unroll
        for (int q = 0; q < COLS; ++q) emit_px(v[0][q], v[1][q], v[2][q], lv, k, yq[r][q], ub[r][q], ur[r][q]);
#pragma unroll
        for (int m = 0; m < COLS / 2; ++m) h.yq[r][m] = yq[r][2 * m] | (yq[r][2 * m + 1] << 16);
    }
    unsigned cb[4], cr[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        cb[m] = (unsigned)emit_chroma(ub[0][2 * m], ub[0][2 * m + 1], ub[1][2 * m], ub[1][2 * m + 1], lv);
        cr[m] = (unsigned)emit_chroma(ur[0][2 * m], ur[0][2 * m + 1], ur[1][2 * m], ur[1][2 * m + 1], lv);
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        h.cb[m] = cb[2 * m] | (cb[2 * m + 1] << 16);
        h.cr[m] = cr[2 * m] | (cr[2 * m + 1] << 16);
    }
}

__device__ __forceinline__ int held_code(unsigned pair, int odd) { return (int)(odd ? pair >> 16 : pair & 0xffffu); }

// The compare half: the held codes against the frame ref at (Y, X), the frame position of the item's first row and column (both
// even); adds the item's three weighted sums to su exactly as sse_item does.
template <class T, bool IL, bool FULL>
__device__ __forceinline__ void run_compare(const Held& h, int rows, int hi, const Planes<const T>& ref, int64_t Y, int64_t X, u64 su[3])
{
    constexpr int SH = sizeof(T) == 2 ? 6 : 0;
    constexpr int CS = IL ? 2 : 1;                                // elements from one Cb (Cr) sample to the next
    // luma
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (FULL || r < rows) {
            const T* p = ref.y + (Y + r) * ref.yr + X;
            unsigned w[COLS];
            if (FULL) {
                load4(p, w);
                load4(p + 4, w + 4);
            } else {
#pragma unroll
                for (int q = 0; q < COLS; ++q) w[q] = q < hi ? (unsigned)p[q] : 0u;
            }
            u64 row = 0ull;                                        // each term < 2^11 * 2^20
#pragma unroll
            for (int q = 0; q < COLS; ++q) {
                if (FULL || q < hi) {
                    const int e = held_code(h.yq[r][q >> 1], q & 1) - (int)(w[q] >> SH);
                    row += (u64)(h.ax[q] * (unsigned)(e * e));
                }
            }
            su[0] += (u64)h.ay[r] * row;
        }
    }
    // chroma: the frame's sample (Y / 2, X / 2 + m) against the code of the tile's cell (r0 / 2, q0 / 2 + m)
    const int64_t ci = Y >> 1, cx0 = X >> 1;
    const T* pu = ref.u + ci * ref.ur + CS * cx0;
    const T* pv = IL ? pu + 1 : ref.v + ci * ref.vr + cx0;
    unsigned w[2][4];
    if (FULL) {
        if (IL) {
            unsigned e[8];
            load4(pu, e);
            load4(pu + 4, e + 4);
#pragma unroll
            for (int m = 0; m < 4; ++m) { w[0][m] = e[2 * m]; w[1][m] = e[2 * m + 1]; }
        } else {
            load4(pu, w[0]);
            load4(pv, w[1]);
        }
    } else {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const bool in = 2 * m < hi;
            w[0][m] = in ? (unsigned)pu[CS * m] : 0u;
            w[1][m] = in ? (unsigned)pv[CS * m] : 0u;
        }
    }
    const u64 cy = (u64)((h.ay[0] + h.ay[1]) >> 1);
    u64 sb = 0ull, sr = 0ull;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (FULL || 2 * m < hi) {
            const int eb = held_code(h.cb[m >> 1], m & 1) - (int)(w[0][m] >> SH);
            const int er = held_code(h.cr[m >> 1], m & 1) - (int)(w[1][m] >> SH);
            const unsigned cx = (h.ax[2 * m] + h.ax[2 * m + 1]) >> 1;
            sb += (u64)(cx * (unsigned)(eb * eb));
            sr += (u64)(cx * (unsigned)(er * er));
        }
    }
    su[1] += cy * sb;
    su[2] += cy * sr;
}

// Block b of job m is block m * bpt + b: the items b * NT .. of the job's tile, item -> (row pair kp, group g), tile rows 2 kp and
// 2 kp + 1, tile columns 8g .. 8g+7 (G8 = T / 8): sse_tile's map.
template <class T, bool IL, bool WIDE>
__global__ __launch_bounds__(NT) void sse_runs_kernel(F32 x, const pc_ctr_frame* __restrict__ frames, int n_frames,
                                                      const int32_t* __restrict__ tiles, const int32_t* __restrict__ offsets,
                                                      const int32_t* __restrict__ slots, int n_entries, Grid gr, int G8, int bpt, Levels lv,
                                                      EmitCoef k, u64* __restrict__ partials)
{
    const int m = (int)(blockIdx.x / (unsigned)bpt), b = (int)(blockIdx.x - (unsigned)m * (unsigned)bpt);
    const int tg = tiles[m];
    const int e0 = clampi(offsets[m], 0, n_entries), e1 = clampi(offsets[(int64_t)m + 1], 0, n_entries);
    const bool tile_in = tg >= 0 && tg < gr.ny * gr.nx;           // block-uniform
    Held h;
    bool active = false, full = false;
    int rows = 0, hi = 0;
    int64_t Y = 0, X = 0;
    if (tile_in) {
        const int i = tg / gr.nx, j = tg - i * gr.nx;
        const int S = gr.S, O = gr.O, den = O > 0 ? 2 * O : 1;
        const int Yt = i * S, Xt = j * S;                         // the tile's first row and column in the frame: < H, < W
        const int hh = min(gr.T, gr.H - Yt), ww = min(gr.T, gr.W - Xt);
        const int rem = b * NT + (int)threadIdx.x;                // < T * T / 16 <= 2^18
        const int kp = rem / G8, r0 = 2 * kp, q0 = COLS * (rem - kp * G8);
        if (r0 < hh && q0 < ww) {
            active = true;
            rows = r0 + 1 < hh ? 2 : 1;
            hi = min(COLS, ww - q0);
            full = WIDE && rows == 2 && hi == COLS;
            Y = (int64_t)Yt + r0;
            X = (int64_t)Xt + q0;
#pragma unroll
            for (int r = 0; r < 2; ++r) h.ay[r] = axis_weight(i, gr.ny, r0 + r, S, O, den);
#pragma unroll
            for (int q = 0; q < COLS; ++q) h.ax[q] = axis_weight(j, gr.nx, q0 + q, S, O, den);
            const float* xt = x.p + (int64_t)m * x.st;
            if (full) run_emit<true>(xt, x.sc, x.sh, r0, q0, rows, hi, lv, k, h);
            else run_emit<false>(xt, x.sc, x.sh, r0, q0, rows, hi, lv, k, h);
        }
    }
    const int wave = (int)(threadIdx.x >> 6);
    for (int e = e0; e < e1; ++e) {
        u64 su[3] = {0ull, 0ull, 0ull};
        if (tile_in) {
            const int slot = slots[e];                            // wave-uniform, as the frame record is
            if (slot >= 0 && slot < n_frames && active) {
                const Planes<const T> ref = planes_of<const T>(frames + slot);
                if (full) run_compare<T, IL, true>(h, rows, hi, ref, Y, X, su);
                else run_compare<T, IL, false>(h, rows, hi, ref, Y, X, su);
            }
        }
        wave_reduce<Sum>(su);                                      // every lane of the wave is here: no branch above leaves the loop
        if ((threadIdx.x & 63) == 0) {
            u64* d = partials + (((int64_t)e * bpt + b) * WAVES + wave) * 3;
            d[0] = su[0];
            d[1] = su[1];
            d[2] = su[2];
        }
    }
}

// One wave per entry: its 4 * bpt wave partials, lane l taking l, l + 64, ..., then the wave tree.
__global__ __launch_bounds__(64) void final_kernel(const u64* __restrict__ p, int n, u64* __restrict__ out)
{
    row_final<Sum, 3>(p, n, out);
}

// The one place that decides the access path: the call launches from it, pc_clip_tol_rate_plan reports it.  pc_clip_rate.hip's
// rule, once per call: every frame of the table has to allow it, whichever the entries name.
bool wide_path(const void* x, int64_t st, int64_t sc, int64_t sh, int O, int fmt, const pc_ctr_frame* frames, int n_frames)
{
    if (!f32_wide(x, st, sc, sh) || O % 8) return false;
    for (int f = 0; f < n_frames; ++f)
        if (!frame_wide(fmt, frames + f)) return false;
    return true;
}

struct Tables {
    const pc_ctr_frame* frames;
    int n_frames;
    const int32_t *tiles, *offsets, *slots;
    int n_entries;
};

template <class T, bool IL>
void launch(bool wide, dim3 grid, hipStream_t st, const F32& x, const Tables& t, const Grid& gr, int bpt, const Levels& lv, const EmitCoef& k,
            u64* part)
{
    if (wide)
        hipLaunchKernelGGL((sse_runs_kernel<T, IL, true>), grid, dim3(NT), 0, st, x, t.frames, t.n_frames, t.tiles, t.offsets, t.slots,
                           t.n_entries, gr, gr.T / COLS, bpt, lv, k, part);
    else
        hipLaunchKernelGGL((sse_runs_kernel<T, IL, false>), grid, dim3(NT), 0, st, x, t.frames, t.n_frames, t.tiles, t.offsets, t.slots,
                           t.n_entries, gr, gr.T / COLS, bpt, lv, k, part);
}

// bytes of the wave partials of n_entries entries; 0 for what the call refuses
size_t partial_bytes(int T, int n_entries)
{
    int bpt;
    int64_t blocks;
    return pair_blocks_of(T, n_entries, T_MAX8, 0, bpt, blocks) ? (size_t)blocks * WAVES * 3 * sizeof(u64) : 0;
}

}  // namespace

extern "C" size_t pc_clip_tol_rate_workspace_size(int T, int n_entries) { return partial_bytes(T, n_entries); }

extern "C" int pc_clip_tol_rate_plan(const void* x, int64_t sxt, int64_t sxc, int64_t sxh, int O, int fmt, const pc_ctr_frame* frames_host,
                                     int n_frames, int* wide)
{
    if (!x || !wide || !fmt_ok(fmt) || O < 0 || !frames_host || n_frames < 1) return PC_ERR_ARG;
    for (int f = 0; f < n_frames; ++f)
        if (!planes_set(fmt, frames_host + f)) return PC_ERR_ARG;
    *wide = wide_path(x, sxt, sxc, sxh, O, fmt, frames_host, n_frames) ? 1 : 0;
    return PC_OK;
}

extern "C" int pc_clip_tol_rate_sse_runs(const float* x, int64_t sxt, int64_t sxc, int64_t sxh, int H, int W, int T, int O, int fmt, int range,
                                         float kr, float kg, float kb, float ib, float ir, const pc_ctr_frame* frames_host,
                                         const pc_ctr_frame* frames_dev, int n_frames, const int32_t* tiles, const int32_t* offsets_host,
                                         const int32_t* offsets_dev, const int32_t* slots, int n_jobs, int n_entries, void* workspace,
                                         size_t workspace_bytes, uint64_t* out, void* stream)
{
    Geo g;
    Levels lv;
    int bpt;
    int64_t blocks;
    if (!fmt_ok(fmt) || !levels_of(fmt, range, lv)) return PC_ERR_ARG;
    if (!geo_of(H, W, T, O, fmt == PC_CTR_P010 ? T_MAX10 : T_MAX8, g) || !pair_blocks_of(T, n_jobs, T_MAX8, 0, bpt, blocks)) return PC_ERR_ARG;
    if (n_entries < n_jobs || !partial_bytes(T, n_entries)) return PC_ERR_ARG;
    if (!x || !aligned(x, 4) || sxh < T || sxc < 1 || sxt < 1) return PC_ERR_ARG;
    if (!frames_host || !frames_dev || !aligned(frames_dev, 8) || n_frames < 1) return PC_ERR_ARG;
    for (int f = 0; f < n_frames; ++f)
        if (!frame_ok(fmt, frames_host + f, W)) return PC_ERR_ARG;
    if (!tiles || !aligned(tiles, 4) || !offsets_host || !offsets_dev || !aligned(offsets_dev, 4) || !slots || !aligned(slots, 4)) return PC_ERR_ARG;
    if (offsets_host[0] != 0 || offsets_host[n_jobs] != n_entries) return PC_ERR_ARG;
    for (int m = 0; m < n_jobs; ++m)
        if (offsets_host[m + 1] <= offsets_host[m]) return PC_ERR_ARG;
    if (!workspace || !aligned(workspace, 8) || !out || !aligned(out, 8)) return PC_ERR_ARG;
    if (workspace_bytes < partial_bytes(T, n_entries)) return PC_ERR_ARG;
    const bool wide = wide_path(x, sxt, sxc, sxh, O, fmt, frames_host, n_frames);
    const F32 xv{x, sxt, sxc, sxh};
    const Grid gr{H, W, T, g.S, O, g.ny, g.nx};
    const EmitCoef k{kr, kg, kb, ib, ir};
    const Tables tb{frames_dev, n_frames, tiles, offsets_dev, slots, n_entries};
    u64* part = static_cast<u64*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks);
    if (fmt == PC_CTR_NV12) launch<uint8_t, true>(wide, grid, st, xv, tb, gr, bpt, lv, k, part);
    else if (fmt == PC_CTR_I420) launch<uint8_t, false>(wide, grid, st, xv, tb, gr, bpt, lv, k, part);
    else launch<uint16_t, true>(wide, grid, st, xv, tb, gr, bpt, lv, k, part);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(final_kernel, dim3((unsigned)n_entries), dim3(64), 0, st, part, WAVES * bpt, reinterpret_cast<u64*>(out));
    HIPCHK(hipGetLastError());
    return PC_OK;
}

extern "C" const char* pc_clip_tol_rate_strerror(int code)
{
    switch (code) {
    case PC_OK: return "ok";
    case PC_ERR_ARG:
        return "invalid argument, unknown format or range, geometry outside pc_clip_tol_rate.h, an empty frame table or job list, offsets "
               "that do not start at 0, rise strictly and end at n_entries, or workspace too small (pc_clip_tol_rate_workspace_size)";
    case PC_ERR_HIP: return "HIP runtime error";
    default: return "unknown error";
    }
}

extern "C" int pc_clip_tol_rate_last_hip_error(void) { return g_last_hip.load(); }

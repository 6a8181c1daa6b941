// pc_chroma_clip_tol_rate.hip -- the per-plane weighted squared error of decoded float tiles against EVERY frame of the run each is
// shown in, for a clip of YUV frames in any of pc_chroma.h's twelve formats and three chroma sitings, in the frames' own codes, on
// gfx950 (pc_chroma_clip_tol_rate.h).  Definition: DESIGN.md section 30: section 28's measure, entry by entry, for the runs of section
// 29's source table; section 20 with section 28's item.  The shared pieces -- plane loads, levels, emit_px, the code of an element,
// band numerators, the format checks, the wave tree, the final -- are image_csrc's; the run item has one user and lives here.
//
// A work item is sse_item's (image_csrc/pc_chroma_sse_item.h): SY rows of one job's tile (a row pair at 4:2:0, one row at 4:2:2 and
// 4:4:4) by eight tile-aligned columns, with the 8 / SX chroma samples of those columns.  A thread takes one item, a block NT
// consecutive items of ONE job.  The item has two halves:
//   emit     once per job: the floats of the item's rows (and, co-sited, of the row above and the halo pixel) -> SY * 8 luma codes
//            and 8 / SX + 8 / SX chroma codes, the same single IEEE operations in the same order as weighted_row / sse_item, and the
//            band numerators ay, ax.  All of it stays in registers, the codes two to a register.
//   compare  once per entry of the job: the frame's luma and chroma codes against the held ones, the three weighted sums formed as
//            sse_item forms them (the same integer types, the same clamped edge cells), the wave tree, and lane 0 of each wave
//            writes the wave's three sums: partials[(e * bpt + b) * 4 + wave][3].
// The block reads its job's tile and entry range, and per entry the slot and the frame record, by indices that depend on blockIdx and
// the loop counter alone: wave-uniform loads.  A job whose tile is out of range and an entry whose slot is out of range write zeros
// and read no frame, so every partial of every entry is written.  The loop has no barrier and the kernel no LDS.  An item whose rows
// and columns all lie inside the frame and whose accesses are all wide is compiled on its own (FULL), in both halves; every other
// item goes element by element.  The access path only changes the load instructions, never the sums.  Template parameters are what
// changes the shape of an item (element type, interleave, SX, SY, whether the row above is read, the access path); the depth shift,
// the horizontal siting and the scale are wave-uniform kernel arguments.  32 sse_runs kernels and the final.  Everything that is added
// is an integer.  No atomics.
#include "pc_image_host.h"
#include "pc_reduce.h"
#include "pc_tile_grid.h"
#include "pc_yuv_device.h"
#include "pc_chroma_items.h"
#include "pc_chroma_sse_item.h"

#include "pc_chroma_clip_tol_rate.h"

namespace {

static_assert(PC_CCTR_PLANAR == LAYOUT_PLANAR && PC_CCTR_SEMIPLANAR == LAYOUT_SEMIPLANAR, "pc_chroma_items.h's layouts are pc_chroma_clip_tol_rate.h's");
static_assert(PC_CCTR_CENTRE == SITE_CENTRE && PC_CCTR_COSITED == SITE_COSITED, "pc_chroma_items.h's sitings are pc_chroma_clip_tol_rate.h's");

constexpr int T_MAX8 = 2048;             // T^4 * 255^2 < 2^60
constexpr int T_MAX10 = 1024;            // T^4 * 1023^2 < 2^60
constexpr int WAVES = NT / 64;

// What an item holds across the entries of its job: codes two to a register (each fits 10 bits), low half first, and the band
// numerators ay, ax.  The chroma weights cy, cx are NOT held: each is one add and one shift of two of those ((ay[0] + ay[1]) >> 1,
// (ax[2j] + ax[2j + 1]) >> 1, or ay[0], ax[j] on an axis that is not subsampled), formed in run_compare with sse_item's own
// expressions, so the bits are the same; holding them would cost up to nine more registers across the loop, where the 4:2:0 kernels
// already sit at 5 waves per SIMD.
template <int SX, int SY>
struct Held {
    unsigned yq[SY][COLS / 2];           // [row][column pair]
    unsigned cb[COLS / SX / 2], cr[COLS / SX / 2];  // [sample pair]
    unsigned ay[SY], ax[COLS];
};

// One row of the emit half: the floats of tile columns q0 .. q0+7 at xr (channel stride sc; xr is column 0 of the tile's row), of
// which the lanes 0 .. hi-1 lie inside the frame -> the row's luma codes yq[8] and its horizontally filtered chroma differences
// h[Cb, Cr][8 / SX]: weighted_row's operations up to there.  A column right of hi - 1 is column hi - 1; the co-sited filter's column
// q0 - 1 is the halo pixel, column 0 at the tile's left edge.
template <int SX, bool FULL>
__device__ __forceinline__ void run_row(const float* xr, int64_t sc, int q0, int hi, int hco, const Levels& lv, const EmitCoef& k,
                                        unsigned (&yq)[COLS], float (&h)[2][COLS / SX])
{
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
    } else if (hco) {
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
}

// The emit half: tile rows r0 .. r0 + SY - 1 and columns q0 .. q0+7 of the tile at xt, of which `rows` rows and the lanes 0 .. hi-1
// lie inside the frame; a row or column beyond the frame stands in as the last one inside it, as in sse_item.  FULL: rows == SY,
// hi == 8 and every access is wide.  The vertical rule adds in sse_item's order: the row above (a, co-sited only; row 0 itself at the
// tile's top edge), the row below (c), then the item's first row (b): (a + c) + (b + b), or b + c; a sample is
// clampi(rintf(v * s + co), 0, maxv).
template <int SX, int SY, bool VCO, bool FULL>
__device__ __forceinline__ void run_emit(const float* xt, int64_t sc, int64_t sh, int r0, int q0, int rows, int hi, const Measure& ms,
                                         const Levels& lv, const EmitCoef& k, Held<SX, SY>& hd)
{
    constexpr int NC = COLS / SX;                                 // chroma samples of the item
    unsigned yq[SY][COLS];
    float v[2][NC];
    if (SY == 1) {
        run_row<SX, FULL>(xt + (int64_t)r0 * sh, sc, q0, hi, ms.hco, lv, k, yq[0], v);
    } else {
        const bool second = FULL || rows == 2;
        float acc[2][NC], t[2][NC];
        if (VCO) {
            unsigned ya[COLS];                                     // the row above belongs to another item: its luma codes go
            run_row<SX, FULL>(xt + (int64_t)max(r0 - 1, 0) * sh, sc, q0, hi, ms.hco, lv, k, ya, acc);
            run_row<SX, FULL>(xt + (int64_t)(second ? r0 + 1 : r0) * sh, sc, q0, hi, ms.hco, lv, k, yq[SY - 1], t);
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int j = 0; j < NC; ++j) acc[p][j] = acc[p][j] + t[p][j];
        } else {
            run_row<SX, FULL>(xt + (int64_t)(second ? r0 + 1 : r0) * sh, sc, q0, hi, ms.hco, lv, k, yq[SY - 1], acc);
        }
        run_row<SX, FULL>(xt + (int64_t)r0 * sh, sc, q0, hi, ms.hco, lv, k, yq[0], t);
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int j = 0; j < NC; ++j) v[p][j] = VCO ? acc[p][j] + (t[p][j] + t[p][j]) : t[p][j] + acc[p][j];
    }
#pragma unroll
    for (int r = 0; r < SY; ++r)
#pragma unroll
        for (int m = 0; m < COLS / 2; ++m) hd.yq[r][m] = yq[r][2 * m] | (yq[r][2 * m + 1] << 16);
    unsigned cb[NC], cr[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        cb[j] = (unsigned)clampi((int)rintf(v[0][j] * ms.s + (float)lv.co), 0, lv.maxv);
        cr[j] = (unsigned)clampi((int)rintf(v[1][j] * ms.s + (float)lv.co), 0, lv.maxv);
    }
#pragma unroll
    for (int m = 0; m < NC / 2; ++m) {
        hd.cb[m] = cb[2 * m] | (cb[2 * m + 1] << 16);
        hd.cr[m] = cr[2 * m] | (cr[2 * m + 1] << 16);
    }
}

__device__ __forceinline__ int held_code(unsigned pair, int odd) { return (int)(odd ? pair >> 16 : pair & 0xffffu); }

// The compare half: the held codes against the frame ref at (Y, X), the frame position of the item's first row and column
// (multiples of SY and of 8 / 4); adds the item's three weighted sums to su exactly as sse_item does.
template <class T, bool IL, int SX, int SY, bool FULL>
__device__ __forceinline__ void run_compare(const Held<SX, SY>& hd, int rows, int hi, const Planes<const T>& ref, int64_t Y, int64_t X, int sh,
                                            unsigned maxv, u64 su[3])
{
    constexpr int CS = IL ? 2 : 1;                                // elements from one Cb (Cr) sample to the next
    constexpr int NC = COLS / SX;                                 // chroma samples of the item
    const int nc = SX == 2 ? (hi + 1) >> 1 : hi;
    // luma
#pragma unroll
    for (int r = 0; r < SY; ++r) {
        if (FULL || r < rows) {
            const T* ry = ref.y + (Y + r) * ref.yr + X;
            unsigned w[COLS];
            if (FULL) {
                load4(ry, w);
                load4(ry + 4, w + 4);
            } else {
#pragma unroll
                for (int q = 0; q < COLS; ++q) w[q] = q < hi ? (unsigned)ry[q] : 0u;
            }
            u64 row = 0ull;                                        // each term < 2^11 * 2^16 (8 bits), 2^10 * 2^20 (10 bits)
#pragma unroll
            for (int q = 0; q < COLS; ++q) {
                if (FULL || q < hi) {
                    const int e = held_code(hd.yq[r][q >> 1], q & 1) - (int)code_of<T>(w[q], sh, maxv);
                    row += (u64)(hd.ax[q] * (unsigned)(e * e));
                }
            }
            su[0] += (u64)hd.ay[r] * row;
        }
    }
    // chroma: the frame's sample (Y / SY, X / SX + m) against the code of the tile's sample (r0 / SY, q0 / SX + m)
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
    const u64 cy = (u64)(SY == 2 ? (hd.ay[0] + hd.ay[SY - 1]) >> 1 : hd.ay[0]);
    u64 sb = 0ull, sr = 0ull;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        if (FULL || j < nc) {
            const int eb = held_code(hd.cb[j >> 1], j & 1) - (int)code_of<T>(w[0][j], sh, maxv);
            const int er = held_code(hd.cr[j >> 1], j & 1) - (int)code_of<T>(w[1][j], sh, maxv);
            const unsigned cx = SX == 2 ? (hd.ax[SX * j] + hd.ax[SX * j + SX - 1]) >> 1 : hd.ax[j];
            sb += (u64)(cx * (unsigned)(eb * eb));
            sr += (u64)(cx * (unsigned)(er * er));
        }
    }
    su[1] += cy * sb;
    su[2] += cy * sr;
}

struct Tables {
    const pc_cctr_frame* frames;
    int n_frames;
    const int32_t *tiles, *offsets, *slots;
    int n_entries;
};

// Block b of job m is block m * bpt + b: the items b * NT .. of the job's tile, item -> (chroma row kp, group g), tile rows SY kp ..,
// tile columns 8g .. 8g+7 (G8 = T / 8): sse_jobs_kernel's map.  A thread's sums stay below 2^60 with the tile's (T^4 * maxv^2).
template <class T, bool IL, int SX, int SY, bool VCO, bool WIDE>
__global__ __launch_bounds__(NT) void sse_runs_kernel(F32 x, Tables tb, Grid gr, int G8, int bpt, Measure ms, Levels lv, EmitCoef k,
                                                      u64* __restrict__ partials)
{
    const int m = (int)(blockIdx.x / (unsigned)bpt), b = (int)(blockIdx.x - (unsigned)m * (unsigned)bpt);
    const int tg = tb.tiles[m];
    const int e0 = clampi(tb.offsets[m], 0, tb.n_entries), e1 = clampi(tb.offsets[(int64_t)m + 1], 0, tb.n_entries);
    const bool tile_in = tg >= 0 && tg < gr.ny * gr.nx;           // block-uniform
    Held<SX, SY> hd;
    bool active = false, full = false;
    int rows = 0, hi = 0;
    int64_t Y = 0, X = 0;
    if (tile_in) {
        const int i = tg / gr.nx, j = tg - i * gr.nx;
        const int S = gr.S, O = gr.O, den = O > 0 ? 2 * O : 1;
        const int Yt = i * S, Xt = j * S;                         // the tile's first row and column in the frame: < H, < W
        const int hh = min(gr.T, gr.H - Yt), ww = min(gr.T, gr.W - Xt);
        const int rem = b * NT + (int)threadIdx.x;                // < T * T / 8 <= 2^19
        const int kp = rem / G8, r0 = SY * kp, q0 = COLS * (rem - kp * G8);
        if (r0 < hh && q0 < ww) {
            active = true;
            rows = min(SY, hh - r0);
            hi = min(COLS, ww - q0);
            full = WIDE && rows == SY && hi == COLS;
            Y = (int64_t)Yt + r0;
            X = (int64_t)Xt + q0;
#pragma unroll
            for (int r = 0; r < SY; ++r) hd.ay[r] = axis_weight(i, gr.ny, r0 + r, S, O, den);
#pragma unroll
            for (int q = 0; q < COLS; ++q) hd.ax[q] = axis_weight(j, gr.nx, q0 + q, S, O, den);
            const float* xt = x.p + (int64_t)m * x.st;
            if (full) run_emit<SX, SY, VCO, true>(xt, x.sc, x.sh, r0, q0, rows, hi, ms, lv, k, hd);
            else run_emit<SX, SY, VCO, false>(xt, x.sc, x.sh, r0, q0, rows, hi, ms, lv, k, hd);
        }
    }
    const int wave = (int)(threadIdx.x >> 6);
    for (int e = e0; e < e1; ++e) {
        u64 su[3] = {0ull, 0ull, 0ull};
        if (tile_in) {
            const int slot = tb.slots[e];                         // wave-uniform, as the frame record is
            if (slot >= 0 && slot < tb.n_frames && active) {
                const Planes<const T> ref = planes_of<const T>(tb.frames + slot);
                if (full) run_compare<T, IL, SX, SY, true>(hd, rows, hi, ref, Y, X, ms.sh, (unsigned)lv.maxv, su);
                else run_compare<T, IL, SX, SY, false>(hd, rows, hi, ref, Y, X, ms.sh, (unsigned)lv.maxv, su);
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

// -- host ----------------------------------------------------------------------------------------------------------------------------

// The item space: SY rows by eight columns, T * T / (8 SY) items to a job, NT to a block.  Blocks per job and blocks of n jobs (or
// entries); false for what the calls refuse.
bool run_blocks_of(int T, int sy, int n, int t_max, int& bpt, int64_t& blocks)
{
    if (T < 64 || T % 64 || T > t_max || (sy != 1 && sy != 2) || n < 1) return false;
    bpt = (int)((int64_t)T * T / ((int64_t)sy * COLS * NT));
    blocks = (int64_t)n * bpt;
    return blocks <= INT32_MAX;
}

// bytes of the wave partials of n_entries entries; 0 for what the call refuses
size_t partial_bytes(int T, int sy, int n_entries)
{
    int bpt;
    int64_t blocks;
    return run_blocks_of(T, sy, n_entries, T_MAX8, bpt, blocks) ? (size_t)blocks * WAVES * 3 * sizeof(u64) : 0;
}

// The one place that decides the access path: the call launches from it, pc_chroma_clip_tol_rate_plan reports it.
// pc_chroma_clip_rate.hip's rule, once per call: every frame of the table has to allow it, whichever the entries name.
bool wide_path(const void* x, int64_t st, int64_t sc, int64_t sh, int O, bool il, int es, int sx, const pc_cctr_frame* frames, int n_frames)
{
    if (!f32_wide(x, st, sc, sh) || (sx == 2 && O % 8 != 0)) return false;
    for (int f = 0; f < n_frames; ++f) {
        const pc_cctr_frame* ref = frames + f;
        if (!plane_wide(ref->y, ref->y_row, es) || !plane_wide(ref->u, ref->u_row, es)) return false;
        if (!il && !plane_wide(ref->v, ref->v_row, es)) return false;
    }
    return true;
}

}  // namespace

extern "C" size_t pc_chroma_clip_tol_rate_workspace_size(int T, int sy, int n_entries) { return partial_bytes(T, sy, n_entries); }

extern "C" int pc_chroma_clip_tol_rate_plan(const void* x, int64_t sxt, int64_t sxc, int64_t sxh, int O, int layout, int bits, int sx,
                                            const pc_cctr_frame* frames_host, int n_frames, int* wide)
{
    Fmt fm;
    if (!x || !wide || !format_of(layout, bits, 0, sx, 1, fm) || O < 0 || !frames_host || n_frames < 1) return PC_ERR_ARG;
    for (int f = 0; f < n_frames; ++f)
        if (!(frames_host[f].y && frames_host[f].u && (fm.il || frames_host[f].v))) return PC_ERR_ARG;
    *wide = wide_path(x, sxt, sxc, sxh, O, fm.il, bits == 10 ? 2 : 1, sx, frames_host, n_frames) ? 1 : 0;
    return PC_OK;
}

extern "C" int pc_chroma_clip_tol_rate_sse_runs(const float* x, int64_t sxt, int64_t sxc, int64_t sxh, int H, int W, int T, int O, int layout,
                                                int bits, int shift, int sx, int sy, int hsite, int vsite, int range, float kr, float kg,
                                                float kb, float ib, float ir, const pc_cctr_frame* frames_host,
                                                const pc_cctr_frame* frames_dev, int n_frames, const int32_t* tiles,
                                                const int32_t* offsets_host, const int32_t* offsets_dev, const int32_t* slots, int n_jobs,
                                                int n_entries, void* workspace, size_t workspace_bytes, uint64_t* out, void* stream)
{
    Geo g;
    Levels lv;
    Fmt fm;
    int bpt;
    int64_t blocks;
    if (!format_of(layout, bits, shift, sx, sy, fm) || !site_ok(hsite) || !site_ok(vsite) || !depth_levels(bits, range, lv)) return PC_ERR_ARG;
    if (!geo_of(H, W, T, O, bits == 10 ? T_MAX10 : T_MAX8, g) || !run_blocks_of(T, sy, n_jobs, T_MAX8, bpt, blocks)) return PC_ERR_ARG;
    // n_entries >= n_jobs follows from offsets that rise strictly from 0 to n_entries; it is asked first so that a caller whose
    // n_jobs does not fit its offsets is refused before offsets_host[n_jobs] is read
    if (n_entries < n_jobs || !partial_bytes(T, sy, n_entries)) return PC_ERR_ARG;
    if (!x || !aligned(x, 4) || sxh < T || sxc < 1 || sxt < 1) return PC_ERR_ARG;
    if (!frames_host || !frames_dev || !aligned(frames_dev, 8) || n_frames < 1) return PC_ERR_ARG;
    for (int f = 0; f < n_frames; ++f)
        if (!picture_ok(fm, frames_host + f, W)) return PC_ERR_ARG;
    if (!tiles || !aligned(tiles, 4) || !offsets_host || !offsets_dev || !aligned(offsets_dev, 4) || !slots || !aligned(slots, 4)) return PC_ERR_ARG;
    if (offsets_host[0] != 0 || offsets_host[n_jobs] != n_entries) return PC_ERR_ARG;
    for (int m = 0; m < n_jobs; ++m)
        if (offsets_host[m + 1] <= offsets_host[m]) return PC_ERR_ARG;
    if (!workspace || !aligned(workspace, 8) || !out || !aligned(out, 8)) return PC_ERR_ARG;
    if (workspace_bytes < partial_bytes(T, sy, n_entries)) return PC_ERR_ARG;
    const bool hco = sx == 2 && hsite == PC_CCTR_COSITED, vco = sy == 2 && vsite == PC_CCTR_COSITED;
    const bool wide = wide_path(x, sxt, sxc, sxh, O, fm.il, bits == 10 ? 2 : 1, sx, frames_host, n_frames);
    const F32 xv{x, sxt, sxc, sxh};
    const Grid gr{H, W, T, g.S, O, g.ny, g.nx};
    const EmitCoef k{kr, kg, kb, ib, ir};
    const Measure ms{hco ? 1 : 0, 1.f / (float)((sx == 2 ? (hco ? 4 : 2) : 1) * (sy == 2 ? (vco ? 4 : 2) : 1)), shift};
    const Tables tb{frames_dev, n_frames, tiles, offsets_dev, slots, n_entries};
    u64* part = static_cast<u64*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks);
    with_format(fm, [&](auto el, auto il, auto SX, auto SY) {
        using T_ = decltype(el);
        auto launch = [&](auto VCO, auto WIDE) {
            hipLaunchKernelGGL((sse_runs_kernel<T_, il.value, SX.value, SY.value, VCO.value, WIDE.value>), grid, dim3(NT), 0, st, xv, tb, gr,
                               T / COLS, bpt, ms, lv, k, part);
        };
        // VCO is instantiated for SY = 2 alone: at SY = 1 both branches below name the same kernel
        constexpr bool V = SY.value == 2;
        if (wide) {
            if (V && vco) launch(std::integral_constant<bool, V>{}, std::true_type{}); else launch(std::false_type{}, std::true_type{});
        } else {
            if (V && vco) launch(std::integral_constant<bool, V>{}, std::false_type{}); else launch(std::false_type{}, std::false_type{});
        }
    });
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(final_kernel, dim3((unsigned)n_entries), dim3(64), 0, st, part, WAVES * bpt, reinterpret_cast<u64*>(out));
    HIPCHK(hipGetLastError());
    return PC_OK;
}

extern "C" const char* pc_chroma_clip_tol_rate_strerror(int code)
{
    switch (code) {
    case PC_OK: return "ok";
    case PC_ERR_ARG:
        return "invalid argument, unknown layout, depth, shift, subsampling, siting or range, geometry outside pc_chroma_clip_tol_rate.h, an "
               "empty frame table or job list, offsets that do not start at 0, rise strictly and end at n_entries, or workspace too small "
               "(pc_chroma_clip_tol_rate_workspace_size)";
    case PC_ERR_HIP: return "HIP runtime error";
    default: return "unknown error";
    }
}

extern "C" int pc_chroma_clip_tol_rate_last_hip_error(void) { return g_last_hip.load(); }

// pc_clip_tol.hip -- the tolerant scan of a clip of YUV 4:2:0 frames (NV12 / I420 / P010) on gfx950 (pc_clip_tol.h): per frame and
// tile the difference of the tile's footprint against the frame the tile was last coded in (count, sum of squared differences,
// largest absolute difference, per plane), and the decision to reuse or recode, taken on the device.  Definition: DESIGN.md section
// 18, on top of sections 16 (geometry, footprint) and 17 (the device frame table); the device code shared with pc_clips.hip (plane
// loads, word >> 6, the footprint, the item, the halo block) and pc_clip_rate.hip (reading a frame record of the table by a
// block-uniform index) is restated here.
//
// Step k is two launches.  diff_kernel: a work item is one ROW PAIR (2r, 2r+1) of one tile by eight tile-aligned luma columns:
// sixteen luma samples and the four Cb and four Cr samples of the 2 x 2 cells the thread holds, in frame k and in the tile's anchor.
// A thread takes one item, a block NT consecutive items of ONE tile (T * T / 16 is a multiple of 256 for every T that is a multiple of
// 64: no block straddles two tiles and none has a tail).  The block reads anchor[t] and, where it lies in [0, k), the two frame
// records frames[k] and frames[anchor[t]]: the indices depend on blockIdx alone, so the loads are wave-uniform.  One more block per
// tile takes the halo ring element by element.  An item whose rows and columns all lie inside the frame and whose accesses are all
// wide is compiled on its own (FULL); every other item goes element by element.  A thread carries nine accumulators (count, sse,
// maxabs of three planes); they go thread -> wave tree -> the block's four waves in order (36 words of LDS) -> one 72-byte partial per
// block, by sum, sum and max.  decide_kernel: one wave per tile over its partials; lane 0 writes stats[k][t], applies the rule and
// writes source[k][t] and anchor[t].  Stream order makes step k + 1 see step k's anchors.  Everything is an integer: the result
// depends neither on order nor on access path.  No atomics, no LDS on the data path.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "pc_clip_tol.h"

static std::atomic<int> g_last_hip{0};
#define HIPCHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { g_last_hip = (int)_e; return PC_ERR_HIP; } } while (0)

namespace {

constexpr int NT = 256;                  // threads per block (4 waves), one work item each
constexpr int COLS = 8;                  // luma columns per work item
constexpr int T_MAX = 2048;              // T^2 * 1023^2 < 2^43
constexpr int NACC = 9;                  // [plane][count, sse, maxabs]

typedef unsigned long long u64;

template <class T>
struct Planes {                          // pc_ct_frame with typed pointers; row strides in elements
    const T* y;
    int64_t yr;
    const T* u;
    int64_t ur;
    const T* v;
    int64_t vr;
};

struct Grid {                            // the frame and the grid
    int H, W, T, S, O, ny, nx;
};

struct Tol {
    unsigned max_abs[3], mse_q10[3];
    int max_run;
};

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// four consecutive elements of a plane in one access: a 32-bit word of bytes, a 64-bit word of 16-bit words
__device__ __forceinline__ void load4(const uint8_t* p, unsigned v[4])
{
    const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
    v[0] = w & 255u; v[1] = (w >> 8) & 255u; v[2] = (w >> 16) & 255u; v[3] = w >> 24;
}

__device__ __forceinline__ void load4(const uint16_t* p, unsigned v[4])
{
    const uint2 w = *reinterpret_cast<const uint2*>(p);
    v[0] = w.x & 0xffffu; v[1] = w.x >> 16; v[2] = w.y & 0xffffu; v[3] = w.y >> 16;
}

// one sample of plane p into a thread's accumulators: ac[3p] count, ac[3p + 1] sse, ac[3p + 2] maxabs.  A thread holds at most 16
// luma samples, or 17 of a halo ring (2 * 1026 + 2 * 1024 samples over 256 threads): 17 * 1023^2 < 2^25.
template <int SH>
__device__ __forceinline__ void take(unsigned a, unsigned b, int p, unsigned ac[NACC])
{
    const int e = (int)(a >> SH) - (int)(b >> SH);
    const unsigned d = (unsigned)(e < 0 ? -e : e);
    ac[3 * p] += d ? 1u : 0u;
    ac[3 * p + 1] += d * d;
    ac[3 * p + 2] = max(ac[3 * p + 2], d);
}

// One item: luma rows Y, Y + 1 and columns X .. X+7 of the frame (both even), of which `rows` rows and the lanes 0 .. hi-1 lie
// inside the tile's part of the frame (rows is 1 or 2, 1 <= hi <= 8), and the chroma samples (Y / 2, X / 2 + m), 2m < hi.
// FULL: rows == 2, hi == 8 and every access is wide; else element by element.  A lane outside is 0 in both frames: it adds nothing.
template <class T, bool IL, bool FULL>
__device__ __forceinline__ void diff_item(const Planes<T>& a, const Planes<T>& b, int64_t Y, int64_t X, int rows, int hi, unsigned ac[NACC])
{
    constexpr int SH = sizeof(T) == 2 ? 6 : 0;
    constexpr int CS = IL ? 2 : 1;                                // elements from one Cb (Cr) sample to the next
#pragma unroll
    for (int r = 0; r < 2; ++r) {
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
            for (int q = 0; q < COLS; ++q) take<SH>(wa[q], wb[q], 0, ac);
        }
    }
    const int64_t ci = Y >> 1, cx0 = X >> 1;
    const T* ua = a.u + ci * a.ur + CS * cx0;
    const T* va = IL ? ua + 1 : a.v + ci * a.vr + cx0;
    const T* ub = b.u + ci * b.ur + CS * cx0;
    const T* vb = IL ? ub + 1 : b.v + ci * b.vr + cx0;
    unsigned ca[2][4], cb[2][4];                                  // [Cb, Cr][sample]
    if (FULL) {
        if (IL) {
            unsigned ea[8], eb[8];
            load4(ua, ea);
            load4(ua + 4, ea + 4);
            load4(ub, eb);
            load4(ub + 4, eb + 4);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                ca[0][m] = ea[2 * m]; ca[1][m] = ea[2 * m + 1];
                cb[0][m] = eb[2 * m]; cb[1][m] = eb[2 * m + 1];
            }
        } else {
            load4(ua, ca[0]);
            load4(va, ca[1]);
            load4(ub, cb[0]);
            load4(vb, cb[1]);
        }
    } else {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const bool in = 2 * m < hi;
            ca[0][m] = in ? (unsigned)ua[CS * m] : 0u;
            ca[1][m] = in ? (unsigned)va[CS * m] : 0u;
            cb[0][m] = in ? (unsigned)ub[CS * m] : 0u;
            cb[1][m] = in ? (unsigned)vb[CS * m] : 0u;
        }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        take<SH>(ca[0][m], cb[0][m], 1, ac);
        take<SH>(ca[1][m], cb[1][m], 2, ac);
    }
}

template <class T>
__device__ __forceinline__ Planes<T> planes_of(const pc_ct_frame* f)
{
    return Planes<T>{static_cast<const T*>(f->y), f->y_row, static_cast<const T*>(f->u), f->u_row, static_cast<const T*>(f->v), f->v_row};
}

// The first launch of step k.  Blocks t * (bpt + 1) .. + bpt - 1 hold the items of tile t: item -> (row pair r, group g), tile rows
// 2r and 2r + 1, tile columns 8g .. 8g+7; block t * (bpt + 1) + bpt holds its halo ring.  partials[blockIdx.x * 9 + 3p + c]; every
// block writes its nine, zeros where the anchor lies outside [0, k).
template <class T, bool IL, bool WIDE>
__global__ __launch_bounds__(NT) void diff_kernel(const pc_ct_frame* __restrict__ frames, int k, const int32_t* __restrict__ anchor, Grid gr,
                                                  int G8, int bpt, int halo, u64* __restrict__ partials)
{
    constexpr int SH = sizeof(T) == 2 ? 6 : 0;
    constexpr int CS = IL ? 2 : 1;
    __shared__ unsigned red[NT / 64][NACC];
    const int bpt1 = bpt + 1;
    const int t = (int)(blockIdx.x / (unsigned)bpt1), bl = (int)(blockIdx.x - (unsigned)t * (unsigned)bpt1);
    const int an = anchor[t];
    unsigned ac[NACC];
#pragma unroll
    for (int c = 0; c < NACC; ++c) ac[c] = 0u;
    if (an >= 0 && an < k) {                                      // block-uniform: the barrier below is outside
        const Planes<T> a = planes_of<T>(frames + k), b = planes_of<T>(frames + an);
        const int i = t / gr.nx, j = t - i * gr.nx;
        const int Yt = i * gr.S, Xt = j * gr.S;                   // the tile's first row and column in the frame: < H, < W
        const int hh = min(gr.T, gr.H - Yt), ww = min(gr.T, gr.W - Xt);
        if (bl < bpt) {
            const int rem = bl * NT + (int)threadIdx.x;           // < T * T / 16 <= 2^18
            const int kp = rem / G8, r0 = 2 * kp, q0 = COLS * (rem - kp * G8);
            if (r0 < hh && q0 < ww) {
                const int rows = r0 + 1 < hh ? 2 : 1, hi = min(COLS, ww - q0);
                if (WIDE && rows == 2 && hi == COLS)
                    diff_item<T, IL, true>(a, b, (int64_t)Yt + r0, (int64_t)Xt + q0, rows, hi, ac);
                else
                    diff_item<T, IL, false>(a, b, (int64_t)Yt + r0, (int64_t)Xt + q0, rows, hi, ac);
            }
        } else if (halo) {
            // the chroma rectangle the items covered: rows r0c .. r1c, columns c0c .. c1c; the ring around it where the frame has it
            const int Hc = (gr.H + 1) >> 1, Wc = (gr.W + 1) >> 1;
            const int r0c = Yt >> 1, r1c = r0c + ((hh + 1) >> 1) - 1, c0c = Xt >> 1, c1c = c0c + ((ww + 1) >> 1) - 1;
            const bool top = r0c > 0, bottom = r1c < Hc - 1, left = c0c > 0, right = c1c < Wc - 1;
            const int cf = c0c - (left ? 1 : 0), nw = c1c + (right ? 1 : 0) - cf + 1, nh = r1c - r0c + 1;
            for (int idx = (int)threadIdx.x; idx < 2 * nw + 2 * nh; idx += NT) {
                int row, col;
                bool on;
                if (idx < nw) { row = r0c - 1; col = cf + idx; on = top; }
                else if (idx < 2 * nw) { row = r1c + 1; col = cf + idx - nw; on = bottom; }
                else if (idx < 2 * nw + nh) { row = r0c + idx - 2 * nw; col = c0c - 1; on = left; }
                else { row = r0c + idx - 2 * nw - nh; col = c1c + 1; on = right; }
                if (on) {                                          // 0 <= row < Hc and 0 <= col < Wc
                    const int64_t oa = (int64_t)row * a.ur + CS * (int64_t)col, ob = (int64_t)row * b.ur + CS * (int64_t)col;
                    const T* va = IL ? a.u + oa + 1 : a.v + (int64_t)row * a.vr + col;
                    const T* vb = IL ? b.u + ob + 1 : b.v + (int64_t)row * b.vr + col;
                    take<SH>((unsigned)a.u[oa], (unsigned)b.u[ob], 1, ac);
                    take<SH>((unsigned)*va, (unsigned)*vb, 2, ac);
                }
            }
        }
    }
    // a wave holds at most 64 * 17 samples of a plane: 64 * 2^25 = 2^31
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int c = 0; c < NACC; ++c) {
            const unsigned o = __shfl_down(ac[c], off, 64);
            ac[c] = c % 3 == 2 ? max(ac[c], o) : ac[c] + o;
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < NACC; ++c) red[threadIdx.x >> 6][c] = ac[c];
    }
    __syncthreads();
    if (threadIdx.x < NACC) {
        const int c = threadIdx.x;
        u64 s = red[0][c];
        for (int wv = 1; wv < NT / 64; ++wv) s = c % 3 == 2 ? max(s, (u64)red[wv][c]) : s + red[wv][c];
        partials[(int64_t)blockIdx.x * NACC + c] = s;
    }
}

// samples of tile i's footprint along an axis: (luma, chroma)
__device__ __forceinline__ void axis_samples(int i, int L, int T, int S, int halo, int& nl, int& nc)
{
    const int y0 = i * S, e = min(y0 + T, L), Lc = (L + 1) >> 1;
    const int c0 = max((y0 >> 1) - halo, 0), c1 = min(((e + 1) >> 1) - 1 + halo, Lc - 1);
    nl = e - y0;
    nc = c1 - c0 + 1;
}

// The second launch of step k.  One wave per tile: its nb block partials, lane l taking l, l + 64, ..., then the wave tree; lane 0
// writes the tile's nine numbers, decides, and writes source[k][t] and anchor[t].  src and st: row k of source and stats.
__global__ __launch_bounds__(64) void decide_kernel(const u64* __restrict__ p, int nb, int k, Grid gr, int halo, Tol tol, int32_t* __restrict__ anchor,
                                                    int32_t* __restrict__ src, u64* __restrict__ st)
{
    const int64_t t = blockIdx.x;
    u64 ac[NACC];
#pragma unroll
    for (int c = 0; c < NACC; ++c) ac[c] = 0ull;
    for (int b = threadIdx.x; b < nb; b += 64) {
#pragma unroll
        for (int c = 0; c < NACC; ++c) {
            const u64 v = p[(t * nb + b) * NACC + c];
            ac[c] = c % 3 == 2 ? max(ac[c], v) : ac[c] + v;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int c = 0; c < NACC; ++c) {
            const u64 o = __shfl_down(ac[c], off, 64);
            ac[c] = c % 3 == 2 ? max(ac[c], o) : ac[c] + o;
        }
    }
    if (threadIdx.x == 0) {
        const int an = anchor[t];
        bool reuse = an >= 0 && an < k;                           // outside: the first launch added nothing, the nine are zero
#pragma unroll
        for (int c = 0; c < NACC; ++c) st[t * NACC + c] = ac[c];
        const int i = (int)t / gr.nx, j = (int)t - i * gr.nx;
        int hl, hc, wl, wc;
        axis_samples(i, gr.H, gr.T, gr.S, halo, hl, hc);
        axis_samples(j, gr.W, gr.T, gr.S, halo, wl, wc);
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

bool fmt_ok(int fmt) { return fmt == PC_CT_NV12 || fmt == PC_CT_I420 || fmt == PC_CT_P010; }
bool interleaved(int fmt) { return fmt != PC_CT_I420; }
int elem_bytes(int fmt) { return fmt == PC_CT_P010 ? 2 : 1; }
bool upsample_ok(int u) { return u == PC_CT_NEAREST || u == PC_CT_LINEAR; }

// One plane of rows of `len` elements: pointer aligned to its element, the row stride at least the row.
bool plane_ok(const void* p, int64_t sr, int es, int64_t len) { return p && reinterpret_cast<uintptr_t>(p) % es == 0 && sr >= len; }

bool frame_ok(int fmt, const pc_ct_frame* f, int W)
{
    if (!f || !fmt_ok(fmt)) return false;
    const int es = elem_bytes(fmt);
    const int64_t Wc = cdiv(W, 2);
    if (!plane_ok(f->y, f->y_row, es, W)) return false;
    if (interleaved(fmt)) return plane_ok(f->u, f->u_row, es, 2 * Wc);
    return plane_ok(f->u, f->u_row, es, Wc) && plane_ok(f->v, f->v_row, es, Wc);
}

int64_t axis_tiles(int L, int T, int S) { return L <= T ? 1 : cdiv((int64_t)L - T, S) + 1; }

struct Geo {
    int S, ny, nx;
};

// pc_tiles.h's geometry, with T <= T_MAX
bool geo_of(int H, int W, int T, int O, Geo& g)
{
    if (H < 1 || W < 1 || T < 64 || T % 64 || T > T_MAX || O < 0 || O % 4 || O > T / 2) return false;
    const int S = T - O;
    const int64_t ny = axis_tiles(H, T, S), nx = axis_tiles(W, T, S);
    if (ny * nx > INT32_MAX) return false;
    g.S = S;
    g.ny = (int)ny;
    g.nx = (int)nx;
    return true;
}

// Item blocks per tile (one more holds the halo ring) and blocks in all; false for what the scan refuses.
bool blocks_of(int T, int n_tiles, int& bpt, int64_t& blocks)
{
    if (T < 64 || T % 64 || T > T_MAX || n_tiles < 1) return false;
    bpt = (int)((int64_t)T * T / (2 * COLS * NT));
    blocks = (int64_t)n_tiles * (bpt + 1);
    return blocks <= INT32_MAX;
}

// the partials, then the anchors
size_t workspace_of(int64_t blocks, int n_tiles)
{
    return (size_t)((blocks * NACC * (int64_t)sizeof(u64) + (int64_t)n_tiles * 4 + 7) / 8 * 8);
}

bool mult4(int64_t v) { return v % 4 == 0; }

bool plane_wide(const void* p, int64_t sr, int es) { return reinterpret_cast<uintptr_t>(p) % (4 * es) == 0 && mult4(sr); }

// The one place that decides the access path: the scan launches from it, pc_clip_tol_plan reports it.  Once per call: every frame
// of the table has to allow it.
bool wide_path(int fmt, const pc_ct_frame* frames, int n_frames, int O)
{
    if (O % 8) return false;
    const int es = elem_bytes(fmt);
    for (int f = 0; f < n_frames; ++f) {
        const pc_ct_frame* ref = frames + f;
        if (!plane_wide(ref->y, ref->y_row, es) || !plane_wide(ref->u, ref->u_row, es)) return false;
        if (!interleaved(fmt) && !plane_wide(ref->v, ref->v_row, es)) return false;
    }
    return true;
}

template <class T, bool IL>
void launch_diff(bool wide, dim3 grid, hipStream_t st, const pc_ct_frame* frames, int k, const int32_t* anchor, const Grid& gr, int bpt,
                 int halo, u64* part)
{
    if (wide)
        hipLaunchKernelGGL((diff_kernel<T, IL, true>), grid, dim3(NT), 0, st, frames, k, anchor, gr, gr.T / COLS, bpt, halo, part);
    else
        hipLaunchKernelGGL((diff_kernel<T, IL, false>), grid, dim3(NT), 0, st, frames, k, anchor, gr, gr.T / COLS, bpt, halo, part);
}

}  // namespace

extern "C" size_t pc_clip_tol_workspace_size(int T, int n_tiles)
{
    int bpt;
    int64_t blocks;
    return blocks_of(T, n_tiles, bpt, blocks) ? workspace_of(blocks, n_tiles) : 0;
}

extern "C" int pc_clip_tol_plan(int fmt, const pc_ct_frame* frames_host, int n_frames, int O, int* wide)
{
    if (!wide || !fmt_ok(fmt) || O < 0 || !frames_host || n_frames < 1) return PC_ERR_ARG;
    for (int f = 0; f < n_frames; ++f) {
        const pc_ct_frame* ref = frames_host + f;
        if (!ref->y || !ref->u || (!interleaved(fmt) && !ref->v)) return PC_ERR_ARG;
    }
    *wide = wide_path(fmt, frames_host, n_frames, O) ? 1 : 0;
    return PC_OK;
}

extern "C" int pc_clip_tol_scan(const pc_ct_frame* frames_host, const pc_ct_frame* frames_dev, int n_frames, int fmt, int upsample, int H,
                                int W, int T, int O, const int* max_abs, const int* mse_q10, int max_run, void* workspace,
                                size_t workspace_bytes, int32_t* source, uint64_t* stats, void* stream)
{
    Geo g;
    int bpt;
    int64_t blocks;
    if (!fmt_ok(fmt) || !upsample_ok(upsample) || !geo_of(H, W, T, O, g)) return PC_ERR_ARG;
    const int n = g.ny * g.nx;
    if (!blocks_of(T, n, bpt, blocks)) return PC_ERR_ARG;
    if (!frames_host || !frames_dev || reinterpret_cast<uintptr_t>(frames_dev) % 8 || n_frames < 1) return PC_ERR_ARG;
    for (int f = 0; f < n_frames; ++f)
        if (!frame_ok(fmt, frames_host + f, W)) return PC_ERR_ARG;
    if (!max_abs || !mse_q10 || max_run < 0) return PC_ERR_ARG;
    const int top = fmt == PC_CT_P010 ? 1023 : 255;
    Tol tol;
    for (int p = 0; p < 3; ++p) {
        if (max_abs[p] < 0 || max_abs[p] > top || mse_q10[p] < 0 || mse_q10[p] > PC_CT_NO_MSE) return PC_ERR_ARG;
        tol.max_abs[p] = (unsigned)max_abs[p];
        tol.mse_q10[p] = (unsigned)mse_q10[p];
    }
    tol.max_run = max_run;
    if (!workspace || reinterpret_cast<uintptr_t>(workspace) % 8 || workspace_bytes < workspace_of(blocks, n)) return PC_ERR_ARG;
    if (!source || reinterpret_cast<uintptr_t>(source) % 4 || !stats || reinterpret_cast<uintptr_t>(stats) % 8) return PC_ERR_ARG;
    if ((int64_t)n * NACC > INT32_MAX) return PC_ERR_ARG;
    const bool wide = wide_path(fmt, frames_host, n_frames, O);
    const Grid gr{H, W, T, g.S, O, g.ny, g.nx};
    const int halo = upsample == PC_CT_LINEAR ? 1 : 0;
    u64* part = static_cast<u64*>(workspace);
    int32_t* anchor = reinterpret_cast<int32_t*>(part + blocks * NACC);
    u64* st64 = reinterpret_cast<u64*>(stats);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(init_kernel, dim3((unsigned)cdiv((int64_t)n * NACC, NT)), dim3(NT), 0, st, n, anchor, source, st64);
    HIPCHK(hipGetLastError());
    const dim3 grid((unsigned)blocks);
    for (int k = 1; k < n_frames; ++k) {
        if (fmt == PC_CT_NV12) launch_diff<uint8_t, true>(wide, grid, st, frames_dev, k, anchor, gr, bpt, halo, part);
        else if (fmt == PC_CT_I420) launch_diff<uint8_t, false>(wide, grid, st, frames_dev, k, anchor, gr, bpt, halo, part);
        else launch_diff<uint16_t, true>(wide, grid, st, frames_dev, k, anchor, gr, bpt, halo, part);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(decide_kernel, dim3((unsigned)n), dim3(64), 0, st, part, bpt + 1, k, gr, halo, tol, anchor, source + (int64_t)k * n,
                           st64 + (int64_t)k * n * NACC);
        HIPCHK(hipGetLastError());
    }
    return PC_OK;
}

extern "C" const char* pc_clip_tol_strerror(int code)
{
    switch (code) {
    case PC_OK: return "ok";
    case PC_ERR_ARG:
        return "invalid argument, unknown format or upsampling, geometry outside pc_clip_tol.h, an empty frame table, a tolerance outside "
               "its ranges or workspace too small (pc_clip_tol_workspace_size)";
    case PC_ERR_HIP: return "HIP runtime error";
    default: return "unknown error";
    }
}

extern "C" int pc_clip_tol_last_hip_error(void) { return g_last_hip.load(); }

// pc_clip_rate.hip -- the per-plane weighted squared error of decoded float tiles against the frames of a clip of YUV 4:2:0 frames
// (NV12 / I420 / P010), for a list of (frame slot, tile) jobs, in the frames' own codes, on gfx950 (pc_clip_rate.h).  Definition:
// section 15's measure over section 16's work list; the device code shared with pc_frame_rate.hip (plane loads,
// levels, the emit arithmetic, band numerators, the item, the reduction) is restated here.
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
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "pc_clip_rate.h"

static std::atomic<int> g_last_hip{0};
#define HIPCHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { g_last_hip = (int)_e; return PC_ERR_HIP; } } while (0)

namespace {

constexpr int NT = 256;                  // threads per block (4 waves), one work item each
constexpr int COLS = 8;                  // luma columns per work item
constexpr int T_MAX8 = 2048;             // T^4 * 255^2 < 2^60
constexpr int T_MAX10 = 1024;            // T^4 * 1023^2 < 2^60

typedef unsigned long long u64;

template <class T>
struct Planes {                          // pc_cr_frame with typed pointers; row strides in elements
    const T* y;
    int64_t yr;
    const T* u;
    int64_t ur;
    const T* v;
    int64_t vr;
};

struct Levels {
    int yo, ys, co, cs, maxv;
};

struct EmitCoef {
    float kr, kg, kb, ib, ir;
};

struct F32 {                             // a float tile set, strides in elements
    const float* p;
    int64_t st, sc, sh;
};

struct Grid {                            // the frame and the grid
    int H, W, T, S, O, ny, nx;
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

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// The numerator over den of the weight tile i of n gives local coordinate u along an axis (pc_frame_rate.h, restated).
__device__ __forceinline__ unsigned axis_weight(int i, int n, int u, int S, int O, int den)
{
    if (i > 0 && u < O) return (unsigned)(2 * u + 1);
    if (i < n - 1 && u >= S) return (unsigned)(2 * (O - 1 - (u - S)) + 1);
    return (unsigned)den;
}

// One item: rows r0, r0 + 1 and columns q0 .. q0+7 of the tile at xt, of which `rows` rows and the lanes 0 .. hi-1 lie inside the
// frame (rows is 1 or 2, 1 <= hi <= 8); Y, X: the frame position of (r0, q0), both even.  FULL: rows == 2, hi == 8 and every access
// is wide; else element by element, a row or column beyond the frame standing in as the last one inside it (section 13's edge cells).
// ay[2], ax[8]: the band numerators of the item's rows and columns, whether inside the frame or not.
template <class T, bool IL, bool FULL>
__device__ __forceinline__ void sse_item(const float* xt, int64_t sc, int64_t sh, int r0, int q0, int rows, int hi, const Planes<T>& ref,
                                         int64_t Y, int64_t X, const Levels& lv, const EmitCoef& k, const unsigned ay[2],
                                         const unsigned ax[COLS], u64 su[3])
{
    constexpr int SH = sizeof(T) == 2 ? 6 : 0;
    constexpr int CS = IL ? 2 : 1;                                // elements from one Cb (Cr) sample to the next
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
        for (int q = 0; q < COLS; ++q) {
            const float R = clamp01(v[0][q]), Gc = clamp01(v[1][q]), Bc = clamp01(v[2][q]);
            const float Yf = (k.kr * R + k.kg * Gc) + k.kb * Bc;
            const float Cb = (Bc - Yf) * k.ib, Cr = (R - Yf) * k.ir;
            yq[r][q] = (unsigned)clampi((int)rintf(Yf * (float)lv.ys + (float)lv.yo), 0, lv.maxv);
            ub[r][q] = Cb * (float)lv.cs;
            ur[r][q] = Cr * (float)lv.cs;
        }
    }
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
                    const int e = (int)yq[r][q] - (int)(w[q] >> SH);
                    row += (u64)(ax[q] * (unsigned)(e * e));
                }
            }
            su[0] += (u64)ay[r] * row;
        }
    }
    // chroma: the frame's sample (Y / 2, X / 2 + m) is the mean of the tile's cell (r0 / 2, q0 / 2 + m)
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
    const u64 cy = (u64)((ay[0] + ay[1]) >> 1);
    u64 sb = 0ull, sr = 0ull;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (FULL || 2 * m < hi) {
            const float mb = ((ub[0][2 * m] + ub[0][2 * m + 1]) + (ub[1][2 * m] + ub[1][2 * m + 1])) * 0.25f + (float)lv.co;
            const float mr = ((ur[0][2 * m] + ur[0][2 * m + 1]) + (ur[1][2 * m] + ur[1][2 * m + 1])) * 0.25f + (float)lv.co;
            const int eb = clampi((int)rintf(mb), 0, lv.maxv) - (int)(w[0][m] >> SH);
            const int er = clampi((int)rintf(mr), 0, lv.maxv) - (int)(w[1][m] >> SH);
            const unsigned cx = (ax[2 * m] + ax[2 * m + 1]) >> 1;
            sb += (u64)(cx * (unsigned)(eb * eb));
            sr += (u64)(cx * (unsigned)(er * er));
        }
    }
    su[1] += cy * sb;
    su[2] += cy * sr;
}

// Block b of job m is block m * bpt + b: the items b * NT .. of the job's tile, item -> (row pair k, group g), tile rows 2k and
// 2k + 1, tile columns 8g .. 8g+7.  partials[(m * bpt + b) * 3 + p]; every block writes its three, zeros for a job out of range.
template <class T, bool IL, bool WIDE>
__global__ __launch_bounds__(NT) void sse_jobs_kernel(F32 x, const pc_cr_frame* __restrict__ frames, int n_frames,
                                                      const int32_t* __restrict__ jobs, Grid gr, int G8, int bpt, Levels lv, EmitCoef k,
                                                      u64* __restrict__ partials)
{
    __shared__ u64 red[NT / 64][3];
    const int m = (int)(blockIdx.x / (unsigned)bpt), b = (int)(blockIdx.x - (unsigned)m * (unsigned)bpt);
    const int slot = jobs[2 * (int64_t)m], tg = jobs[2 * (int64_t)m + 1];
    u64 su[3] = {0ull, 0ull, 0ull};
    if (slot >= 0 && slot < n_frames && tg >= 0 && tg < gr.ny * gr.nx) {      // block-uniform: the barrier below is outside
        const pc_cr_frame* f = frames + slot;
        const Planes<T> ref{static_cast<const T*>(f->y), f->y_row, static_cast<const T*>(f->u), f->u_row,
                            static_cast<const T*>(f->v), f->v_row};
        const int i = tg / gr.nx, j = tg - i * gr.nx;
        const int S = gr.S, O = gr.O, den = O > 0 ? 2 * O : 1;
        const int Yt = i * S, Xt = j * S;                         // the tile's first row and column in the frame: < H, < W
        const int hh = min(gr.T, gr.H - Yt), ww = min(gr.T, gr.W - Xt);
        const int rem = b * NT + (int)threadIdx.x;                // < T * T / 16 <= 2^18
        const int kp = rem / G8, r0 = 2 * kp, q0 = COLS * (rem - kp * G8);
        if (r0 < hh && q0 < ww) {
            const int rows = r0 + 1 < hh ? 2 : 1, hi = min(COLS, ww - q0);
            unsigned ay[2], ax[COLS];
#pragma unroll
            for (int r = 0; r < 2; ++r) ay[r] = axis_weight(i, gr.ny, r0 + r, S, O, den);
#pragma unroll
            for (int q = 0; q < COLS; ++q) ax[q] = axis_weight(j, gr.nx, q0 + q, S, O, den);
            const float* xt = x.p + (int64_t)m * x.st;
            if (WIDE && rows == 2 && hi == COLS)
                sse_item<T, IL, true>(xt, x.sc, x.sh, r0, q0, rows, hi, ref, (int64_t)Yt + r0, (int64_t)Xt + q0, lv, k, ay, ax, su);
            else
                sse_item<T, IL, false>(xt, x.sc, x.sh, r0, q0, rows, hi, ref, (int64_t)Yt + r0, (int64_t)Xt + q0, lv, k, ay, ax, su);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int p = 0; p < 3; ++p) su[p] += __shfl_down(su[p], off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int p = 0; p < 3; ++p) red[threadIdx.x >> 6][p] = su[p];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int p = threadIdx.x;
        u64 a = red[0][p];
        for (int wv = 1; wv < NT / 64; ++wv) a += red[wv][p];
        partials[(int64_t)blockIdx.x * 3 + p] = a;
    }
}

// One wave per job: its bpt block partials, lane l taking l, l + 64, ..., then the wave tree.
__global__ __launch_bounds__(64) void final_kernel(const u64* __restrict__ p, int bpt, u64* __restrict__ out)
{
    const int64_t t = blockIdx.x;
    u64 su[3] = {0ull, 0ull, 0ull};
    for (int b = threadIdx.x; b < bpt; b += 64) {
#pragma unroll
        for (int c = 0; c < 3; ++c) su[c] += p[(t * bpt + b) * 3 + c];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) su[c] += __shfl_down(su[c], off, 64);
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[t * 3 + c] = su[c];
    }
}

bool fmt_ok(int fmt) { return fmt == PC_CR_NV12 || fmt == PC_CR_I420 || fmt == PC_CR_P010; }
bool interleaved(int fmt) { return fmt != PC_CR_I420; }
int elem_bytes(int fmt) { return fmt == PC_CR_P010 ? 2 : 1; }

bool levels_of(int fmt, int range, Levels& lv)
{
    const int n = fmt == PC_CR_P010 ? 10 : 8, s = 1 << (n - 8), maxv = (1 << n) - 1;
    if (range == PC_CR_LIMITED) lv = Levels{16 * s, 219 * s, 128 * s, 224 * s, maxv};
    else if (range == PC_CR_FULL) lv = Levels{0, maxv, 128 * s, maxv, maxv};
    else return false;
    return true;
}

// One plane of rows of `len` elements: pointer aligned to its element, the row stride at least the row.
bool plane_ok(const void* p, int64_t sr, int es, int64_t len) { return p && reinterpret_cast<uintptr_t>(p) % es == 0 && sr >= len; }

bool frame_ok(int fmt, const pc_cr_frame* f, int W)
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

// pc_tiles.h's geometry, with T <= t_max
bool geo_of(int H, int W, int T, int O, int t_max, Geo& g)
{
    if (H < 1 || W < 1 || T < 64 || T % 64 || T > t_max || O < 0 || O % 4 || O > T / 2) return false;
    const int S = T - O;
    const int64_t ny = axis_tiles(H, T, S), nx = axis_tiles(W, T, S);
    if (ny * nx > INT32_MAX) return false;
    g.S = S;
    g.ny = (int)ny;
    g.nx = (int)nx;
    return true;
}

// Blocks per job and in all; false for what the call refuses.
bool blocks_of(int T, int n_jobs, int& bpt, int64_t& blocks)
{
    if (T < 64 || T % 64 || T > T_MAX8 || n_jobs < 1) return false;
    bpt = (int)((int64_t)T * T / (2 * COLS * NT));
    blocks = (int64_t)n_jobs * bpt;
    return blocks <= INT32_MAX;
}

bool mult4(int64_t v) { return v % 4 == 0; }

bool plane_wide(const void* p, int64_t sr, int es) { return reinterpret_cast<uintptr_t>(p) % (4 * es) == 0 && mult4(sr); }

// The one place that decides the access path: the call launches from it, pc_clip_rate_plan reports it.  Once per call: every frame
// of the table has to allow it, whichever the jobs name.
bool wide_path(const void* x, int64_t st, int64_t sc, int64_t sh, int O, int fmt, const pc_cr_frame* frames, int n_frames)
{
    if (reinterpret_cast<uintptr_t>(x) % 16 || !mult4(st) || !mult4(sc) || !mult4(sh) || O % 8) return false;
    const int es = elem_bytes(fmt);
    for (int f = 0; f < n_frames; ++f) {
        const pc_cr_frame* ref = frames + f;
        if (!plane_wide(ref->y, ref->y_row, es) || !plane_wide(ref->u, ref->u_row, es)) return false;
        if (!interleaved(fmt) && !plane_wide(ref->v, ref->v_row, es)) return false;
    }
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
    return blocks_of(T, n_jobs, bpt, blocks) ? (size_t)blocks * 3 * sizeof(u64) : 0;
}

extern "C" int pc_clip_rate_plan(const void* x, int64_t sxt, int64_t sxc, int64_t sxh, int O, int fmt, const pc_cr_frame* frames_host,
                                 int n_frames, int* wide)
{
    if (!x || !wide || !fmt_ok(fmt) || O < 0 || !frames_host || n_frames < 1) return PC_ERR_ARG;
    for (int f = 0; f < n_frames; ++f) {
        const pc_cr_frame* ref = frames_host + f;
        if (!ref->y || !ref->u || (!interleaved(fmt) && !ref->v)) return PC_ERR_ARG;
    }
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
    if (!geo_of(H, W, T, O, fmt == PC_CR_P010 ? T_MAX10 : T_MAX8, g) || !blocks_of(T, n_jobs, bpt, blocks)) return PC_ERR_ARG;
    if (!x || reinterpret_cast<uintptr_t>(x) % 4 || sxh < T || sxc < 1 || sxt < 1) return PC_ERR_ARG;
    if (!frames_host || !frames_dev || reinterpret_cast<uintptr_t>(frames_dev) % 8 || n_frames < 1) return PC_ERR_ARG;
    for (int f = 0; f < n_frames; ++f)
        if (!frame_ok(fmt, frames_host + f, W)) return PC_ERR_ARG;
    if (!jobs || reinterpret_cast<uintptr_t>(jobs) % 4) return PC_ERR_ARG;
    if (!workspace || reinterpret_cast<uintptr_t>(workspace) % 8 || !out || reinterpret_cast<uintptr_t>(out) % 8) return PC_ERR_ARG;
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

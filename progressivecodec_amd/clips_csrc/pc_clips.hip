// pc_clips.hip -- clips of YUV 4:2:0 frames (NV12 / I420 / P010) on gfx950 (pc_clips.h): which tiles of a frame changed since the
// previous one, counted exactly over each tile's footprint, and the cut of a LIST of tiles into float32 RGB.  Definition: DESIGN.md
// section 16, on top of sections 14 (the cut) and 11 (geometry); the device code shared with pc_frame_tiles.hip (plane loads,
// levels, to_rgb, the cut itself) and pc_frame_rate.hip (the item space of a tile, the reduction) is restated here.
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
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "pc_clips.h"

static std::atomic<int> g_last_hip{0};
#define HIPCHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { g_last_hip = (int)_e; return PC_ERR_HIP; } } while (0)

namespace {

constexpr int NT = 256;                  // threads per block (4 waves), one work item each
constexpr int COLS = 8;                  // luma columns per work item
constexpr int T_MAX = 2048;

typedef unsigned long long u64;

template <class T>
struct Planes {                          // pc_cl_frame with typed pointers; row strides in elements
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

struct IngestCoef {
    float a, b, c, d;
};

struct Grid {                            // the frame, the grid and the linear range of the call
    int H, W, T, S, O, ny, nx, first_tile;
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

// -- changes -------------------------------------------------------------------------------------------------------------------------

// One item: luma rows Y, Y + 1 and columns X .. X+7 of the frame (both even), of which `rows` rows and the lanes 0 .. hi-1 lie
// inside the tile's part of the frame (rows is 1 or 2, 1 <= hi <= 8), and the chroma samples (Y / 2, X / 2 + m), 2m < hi.
// FULL: rows == 2, hi == 8 and every access is wide; else element by element.
template <class T, bool IL, bool FULL>
__device__ __forceinline__ void diff_item(const Planes<T>& a, const Planes<T>& b, int64_t Y, int64_t X, int rows, int hi, unsigned su[3])
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
            for (int q = 0; q < COLS; ++q) su[0] += (wa[q] >> SH) != (wb[q] >> SH) ? 1u : 0u;
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
        su[1] += (ca[0][m] >> SH) != (cb[0][m] >> SH) ? 1u : 0u;
        su[2] += (ca[1][m] >> SH) != (cb[1][m] >> SH) ? 1u : 0u;
    }
}

// Blocks t * (bpt + 1) .. + bpt - 1 hold the items of tile t: item -> (row pair k, group g), tile rows 2k and 2k + 1, tile columns
// 8g .. 8g+7; block t * (bpt + 1) + bpt holds its halo ring.  partials[blockIdx.x * 3 + p].
template <class T, bool IL, bool WIDE>
__global__ __launch_bounds__(NT) void changes_kernel(Planes<T> a, Planes<T> b, Grid gr, int G8, int bpt, int halo, u64* __restrict__ partials)
{
    constexpr int SH = sizeof(T) == 2 ? 6 : 0;
    constexpr int CS = IL ? 2 : 1;
    __shared__ unsigned red[NT / 64][3];
    const int bpt1 = bpt + 1;
    const int t = (int)(blockIdx.x / (unsigned)bpt1), bl = (int)(blockIdx.x - (unsigned)t * (unsigned)bpt1);
    const int tg = gr.first_tile + t, i = tg / gr.nx, j = tg - i * gr.nx;
    const int Yt = i * gr.S, Xt = j * gr.S;                       // the tile's first row and column in the frame: < H, < W
    const int hh = min(gr.T, gr.H - Yt), ww = min(gr.T, gr.W - Xt);
    unsigned su[3] = {0u, 0u, 0u};
    if (bl < bpt) {
        const int rem = bl * NT + (int)threadIdx.x;               // < T * T / 16 <= 2^18
        const int kp = rem / G8, r0 = 2 * kp, q0 = COLS * (rem - kp * G8);
        if (r0 < hh && q0 < ww) {
            const int rows = r0 + 1 < hh ? 2 : 1, hi = min(COLS, ww - q0);
            if (WIDE && rows == 2 && hi == COLS)
                diff_item<T, IL, true>(a, b, (int64_t)Yt + r0, (int64_t)Xt + q0, rows, hi, su);
            else
                diff_item<T, IL, false>(a, b, (int64_t)Yt + r0, (int64_t)Xt + q0, rows, hi, su);
        }
    } else if (halo) {
        // the chroma rectangle the items covered: rows r0c .. r1c, columns c0c .. c1c; the ring around it where the frame has it
        const int Hc = (gr.H + 1) >> 1, Wc = (gr.W + 1) >> 1;
        const int r0c = Yt >> 1, r1c = r0c + ((hh + 1) >> 1) - 1, c0c = Xt >> 1, c1c = c0c + ((ww + 1) >> 1) - 1;
        const bool top = r0c > 0, bottom = r1c < Hc - 1, left = c0c > 0, right = c1c < Wc - 1;
        const int ca = c0c - (left ? 1 : 0), nw = c1c + (right ? 1 : 0) - ca + 1, nh = r1c - r0c + 1;
        for (int idx = (int)threadIdx.x; idx < 2 * nw + 2 * nh; idx += NT) {
            int row, col;
            bool on;
            if (idx < nw) { row = r0c - 1; col = ca + idx; on = top; }
            else if (idx < 2 * nw) { row = r1c + 1; col = ca + idx - nw; on = bottom; }
            else if (idx < 2 * nw + nh) { row = r0c + idx - 2 * nw; col = c0c - 1; on = left; }
            else { row = r0c + idx - 2 * nw - nh; col = c1c + 1; on = right; }
            if (on) {                                              // 0 <= row < Hc and 0 <= col < Wc
                const int64_t oa = (int64_t)row * a.ur + CS * (int64_t)col, ob = (int64_t)row * b.ur + CS * (int64_t)col;
                const T* va = IL ? a.u + oa + 1 : a.v + (int64_t)row * a.vr + col;
                const T* vb = IL ? b.u + ob + 1 : b.v + (int64_t)row * b.vr + col;
                su[1] += ((unsigned)a.u[oa] >> SH) != ((unsigned)b.u[ob] >> SH) ? 1u : 0u;
                su[2] += ((unsigned)*va >> SH) != ((unsigned)*vb >> SH) ? 1u : 0u;
            }
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
        u64 s = red[0][p];
        for (int wv = 1; wv < NT / 64; ++wv) s += red[wv][p];
        partials[(int64_t)blockIdx.x * 3 + p] = s;
    }
}

// One wave per tile: its nb block partials, lane l taking l, l + 64, ..., then the wave tree.
__global__ __launch_bounds__(64) void final_kernel(const u64* __restrict__ p, int nb, u64* __restrict__ out)
{
    const int64_t t = blockIdx.x;
    u64 su[3] = {0ull, 0ull, 0ull};
    for (int b = threadIdx.x; b < nb; b += 64) {
#pragma unroll
        for (int c = 0; c < 3; ++c) su[c] += p[(t * nb + b) * 3 + c];
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

// -- cut -----------------------------------------------------------------------------------------------------------------------------

// One luma pixel of the ingest: its code and the two 16-fold chroma sums -> R, G, B.
__device__ __forceinline__ void to_rgb(int Y, int cb16, int cr16, const Levels& lv, const IngestCoef& k, float& R, float& G, float& B)
{
    const float y = (float)(Y - lv.yo) / (float)lv.ys;
    const float cb = (float)(cb16 - 16 * lv.co) / (float)(16 * lv.cs);
    const float cr = (float)(cr16 - 16 * lv.co) / (float)(16 * lv.cs);
    R = clamp01(y + cr * k.a);
    G = clamp01((y - cb * k.b) - cr * k.c);
    B = clamp01(y + cb * k.d);
}

// Items are the eight-column groups of the listed tiles' rows: item -> (entry m of the list, row r, group g), tile columns 8g .. 8g+7.
// G8 = T / 8, tile_items = T * G8, items = n * tile_items.  SH: the bits below the code in an element (P010: 6).  The chroma taps are
// clamped at the FRAME's edges Hc - 1, Wc - 1.  WIDE needs S a multiple of 8: X0 is then one, and X0 / 2 a multiple of 4.
template <class T, bool IL, bool WIDE>
__global__ __launch_bounds__(NT) void cut_list_kernel(Planes<T> s, int H, int W, int Hc, int Wc, int TT, int S, int ny, int nx,
                                                      const int32_t* __restrict__ tiles, float* __restrict__ dst, int G8, int tile_items,
                                                      int64_t items, int linear, Levels lv, IngestCoef k)
{
    constexpr int SH = sizeof(T) == 2 ? 6 : 0;
    constexpr int CS = IL ? 2 : 1;                                // elements from one Cb (Cr) sample to the next
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
    if (listed && Y64 < H && X64 < W) {
        const int y = (int)Y64, x0 = (int)X64;
        const int i0 = y >> 1;
        const int i1 = clampi(i0 + ((y & 1) ? 1 : -1), 0, Hc - 1);
        const T* yrow = s.y + (int64_t)y * s.yr;
        const T* u0 = s.u + (int64_t)i0 * s.ur;                   // Cb of chroma row i0, i1; Cr: one element on, or the V plane
        const T* u1 = s.u + (int64_t)i1 * s.ur;
        const T* v0 = IL ? u0 + 1 : s.v + (int64_t)i0 * s.vr;
        const T* v1 = IL ? u1 + 1 : s.v + (int64_t)i1 * s.vr;
        if (WIDE && x0 + COLS - 1 < W) {                          // x0 is a multiple of 8 here
            unsigned Yc[COLS];
            load4(yrow + x0, Yc);
            load4(yrow + x0 + 4, Yc + 4);
            const int jc = x0 >> 1;                                // chroma columns jc .. jc+3 exist; a multiple of 4
            const int jl = max(jc - 1, 0), jr = min(jc + 4, Wc - 1);
            unsigned cw[2][2][6];                                  // [row i0, i1][Cb, Cr][columns jl, jc .. jc+3, jr]
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const T* pu = rr ? u1 : u0;
                const T* pv = rr ? v1 : v0;
                if (rr == 1 && !linear) {
#pragma unroll
                    for (int j = 0; j < 6; ++j) { cw[1][0][j] = cw[0][0][j]; cw[1][1][j] = cw[0][1][j]; }
                    break;
                }
                if (IL) {
                    unsigned e[8];
                    load4(pu + 2 * (int64_t)jc, e);
                    load4(pu + 2 * (int64_t)jc + 4, e + 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { cw[rr][0][1 + j] = e[2 * j]; cw[rr][1][1 + j] = e[2 * j + 1]; }
                } else {
                    load4(pu + jc, &cw[rr][0][1]);
                    load4(pv + jc, &cw[rr][1][1]);
                }
                cw[rr][0][0] = pu[CS * (int64_t)jl]; cw[rr][1][0] = pv[CS * (int64_t)jl];
                cw[rr][0][5] = pu[CS * (int64_t)jr]; cw[rr][1][5] = pv[CS * (int64_t)jr];
            }
#pragma unroll
            for (int i = 0; i < COLS; ++i) {
                const int j0 = 1 + (i >> 1), j1 = (i & 1) ? j0 + 1 : j0 - 1;
                int c16[2];
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const int c00 = (int)(cw[0][p][j0] >> SH), c01 = (int)(cw[0][p][j1] >> SH);
                    const int c10 = (int)(cw[1][p][j0] >> SH), c11 = (int)(cw[1][p][j1] >> SH);
                    c16[p] = linear ? 9 * c00 + 3 * c01 + 3 * c10 + c11 : 16 * c00;
                }
                to_rgb((int)(Yc[i] >> SH), c16[0], c16[1], lv, k, o[0][i], o[1][i], o[2][i]);
            }
        } else {                                                  // element by element; also the items that straddle the right edge
#pragma unroll
            for (int i = 0; i < COLS; ++i) {
                const int x = x0 + i;
                if (x < W) {
                    const int64_t j0 = x >> 1;
                    const int64_t j1 = clampi((int)j0 + ((x & 1) ? 1 : -1), 0, Wc - 1);
                    int c16[2];
#pragma unroll
                    for (int p = 0; p < 2; ++p) {
                        const T* r0 = p ? v0 : u0;
                        const T* r1 = p ? v1 : u1;
                        const int c00 = (int)(r0[CS * j0] >> SH);
                        if (linear) {
                            const int c01 = (int)(r0[CS * j1] >> SH), c10 = (int)(r1[CS * j0] >> SH), c11 = (int)(r1[CS * j1] >> SH);
                            c16[p] = 9 * c00 + 3 * c01 + 3 * c10 + c11;
                        } else {
                            c16[p] = 16 * c00;
                        }
                    }
                    to_rgb((int)(yrow[x] >> SH), c16[0], c16[1], lv, k, o[0][i], o[1][i], o[2][i]);
                }
            }
        }
    }
    const int64_t plane = (int64_t)TT * TT;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* d = dst + ((int64_t)m * 3 + c) * plane + (int64_t)r * TT + COLS * g;
        if (WIDE) {
            *reinterpret_cast<float4*>(d) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
            *reinterpret_cast<float4*>(d + 4) = make_float4(o[c][4], o[c][5], o[c][6], o[c][7]);
        } else {
#pragma unroll
            for (int i = 0; i < COLS; ++i) d[i] = o[c][i];
        }
    }
}

// -- host ----------------------------------------------------------------------------------------------------------------------------

bool fmt_ok(int fmt) { return fmt == PC_CL_NV12 || fmt == PC_CL_I420 || fmt == PC_CL_P010; }
bool interleaved(int fmt) { return fmt != PC_CL_I420; }
int elem_bytes(int fmt) { return fmt == PC_CL_P010 ? 2 : 1; }
bool upsample_ok(int u) { return u == PC_CL_NEAREST || u == PC_CL_LINEAR; }

bool levels_of(int fmt, int range, Levels& lv)
{
    const int n = fmt == PC_CL_P010 ? 10 : 8, s = 1 << (n - 8), maxv = (1 << n) - 1;
    if (range == PC_CL_LIMITED) lv = Levels{16 * s, 219 * s, 128 * s, 224 * s, maxv};
    else if (range == PC_CL_FULL) lv = Levels{0, maxv, 128 * s, maxv, maxv};
    else return false;
    return true;
}

// One plane of rows of `len` elements: pointer aligned to its element, the row stride at least the row.
bool plane_ok(const void* p, int64_t sr, int es, int64_t len) { return p && reinterpret_cast<uintptr_t>(p) % es == 0 && sr >= len; }

bool frame_ok(int fmt, const pc_cl_frame* f, int W)
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

// Item blocks per tile (one more holds the halo ring) and blocks in all; false for what the call refuses.
bool blocks_of(int T, int n_tiles, int& bpt, int64_t& blocks)
{
    if (T < 64 || T % 64 || T > T_MAX || n_tiles < 1) return false;
    bpt = (int)((int64_t)T * T / (2 * COLS * NT));
    blocks = (int64_t)n_tiles * (bpt + 1);
    return blocks <= INT32_MAX;
}

bool mult4(int64_t v) { return v % 4 == 0; }

bool plane_wide(const void* p, int64_t sr, int es) { return reinterpret_cast<uintptr_t>(p) % (4 * es) == 0 && mult4(sr); }

bool frame_wide(int fmt, const pc_cl_frame* f)
{
    const int es = elem_bytes(fmt);
    if (!plane_wide(f->y, f->y_row, es) || !plane_wide(f->u, f->u_row, es)) return false;
    return interleaved(fmt) || plane_wide(f->v, f->v_row, es);
}

// The one place that decides the access path: the calls launch from it, pc_clips_plan reports it.
bool wide_path(int op, int fmt, const pc_cl_frame* frame, const pc_cl_frame* other, const void* f32, int O)
{
    if (O % 8 || !frame_wide(fmt, frame)) return false;
    if (op == PC_CL_CHANGES) return frame_wide(fmt, other);
    return reinterpret_cast<uintptr_t>(f32) % 16 == 0;             // the strides 3*T*T, T*T and T are multiples of 4
}

template <class T>
Planes<T> planes_of(const pc_cl_frame* f)
{
    return Planes<T>{static_cast<const T*>(f->y), f->y_row, static_cast<const T*>(f->u), f->u_row, static_cast<const T*>(f->v), f->v_row};
}

template <class T, bool IL>
void launch_changes(bool wide, dim3 grid, hipStream_t st, const pc_cl_frame* cur, const pc_cl_frame* prev, const Grid& gr, int bpt,
                    int halo, u64* part)
{
    const Planes<T> a = planes_of<T>(cur), b = planes_of<T>(prev);
    if (wide)
        hipLaunchKernelGGL((changes_kernel<T, IL, true>), grid, dim3(NT), 0, st, a, b, gr, gr.T / COLS, bpt, halo, part);
    else
        hipLaunchKernelGGL((changes_kernel<T, IL, false>), grid, dim3(NT), 0, st, a, b, gr, gr.T / COLS, bpt, halo, part);
}

template <class T, bool IL>
void launch_cut(bool wide, dim3 grid, hipStream_t st, const pc_cl_frame* src, int H, int W, int T_, const Geo& g, const int32_t* tiles,
                float* dst, int G8, int tile_items, int64_t items, int linear, const Levels& lv, const IngestCoef& k)
{
    const Planes<T> s = planes_of<T>(src);
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
    return blocks_of(T, n_tiles, bpt, blocks) ? (size_t)blocks * 3 * sizeof(u64) : 0;
}

extern "C" int pc_clips_plan(int op, int fmt, const pc_cl_frame* frame, const pc_cl_frame* other, const void* f32, int O, int* wide)
{
    if ((op != PC_CL_CHANGES && op != PC_CL_CUT) || !fmt_ok(fmt) || !wide || O < 0) return PC_ERR_ARG;
    if (op == PC_CL_CUT) other = nullptr;
    if (!frame || (op == PC_CL_CHANGES && !other) || (op == PC_CL_CUT && !f32)) return PC_ERR_ARG;
    for (const pc_cl_frame* f : {frame, other})
        if (f && (!f->y || !f->u || (!interleaved(fmt) && !f->v))) return PC_ERR_ARG;
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
    if (!geo_of(H, W, T, O, g) || !blocks_of(T, n_tiles, bpt, blocks)) return PC_ERR_ARG;
    if (first_tile < 0 || (int64_t)first_tile + n_tiles > (int64_t)g.ny * g.nx) return PC_ERR_ARG;
    if (!frame_ok(fmt, cur, W) || !frame_ok(fmt, prev, W)) return PC_ERR_ARG;
    if (!workspace || reinterpret_cast<uintptr_t>(workspace) % 8 || !out || reinterpret_cast<uintptr_t>(out) % 8) return PC_ERR_ARG;
    if (workspace_bytes < (size_t)blocks * 3 * sizeof(u64)) return PC_ERR_ARG;
    const bool wide = wide_path(PC_CL_CHANGES, fmt, cur, prev, nullptr, O);
    const Grid gr{H, W, T, g.S, O, g.ny, g.nx, first_tile};
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
    if (!geo_of(H, W, T, O, g) || !upsample_ok(upsample)) return PC_ERR_ARG;
    if (!dst || reinterpret_cast<uintptr_t>(dst) % 4 || !frame_ok(fmt, src, W) || !levels_of(fmt, range, lv)) return PC_ERR_ARG;
    if (!tiles || reinterpret_cast<uintptr_t>(tiles) % 4 || n < 1 || n > INT32_MAX / 3) return PC_ERR_ARG;
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

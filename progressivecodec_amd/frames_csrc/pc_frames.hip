// pc_frames.hip -- YUV 4:2:0 frames (NV12 / I420 / P010) <-> the codec's float32 RGB planes on gfx950 (pc_frames.h).  Definition:
// DESIGN.md section 13.
//
// A work item is eight consecutive luma columns: of ONE padded row for the ingest (its two chroma rows are chosen per luma row, so a
// row pair shares no arithmetic there), of one ROW PAIR of the window for the emit (four chroma samples, each the mean of 2 x 2 luma
// positions).  A thread takes one item, a block NT consecutive items of ONE picture.  Eight columns, not four, so that every plane
// moves at least 32 bits per access (four I420 chroma bytes) and the float planes two 128-bit words.  The access path (WIDE: four
// elements of a plane and four floats per access; else one by one) only changes the load and store instructions, never which thread
// handles which sample or in which order it adds: the bits are the same on both.  No LDS on the data path; the sums go thread, wave
// tree, waves in order (12 words of LDS), then emit_final over the block partials, no atomics.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "pc_frames.h"

static std::atomic<int> g_last_hip{0};
#define HIPCHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { g_last_hip = (int)_e; return PC_ERR_HIP; } } while (0)

namespace {

constexpr int NT = 256;                  // threads per block (4 waves)
constexpr int COLS = 8;                  // luma columns per work item

template <class T>
struct Planes {                          // pc_frame with typed pointers; strides in elements
    T* y;
    int64_t yb, yr;
    T* u;
    int64_t ub, ur;
    T* v;
    int64_t vb, vr;
};

struct Levels {
    int yo, ys, co, cs, maxv;
};

struct IngestCoef {
    float a, b, c, d;
};

struct EmitCoef {
    float kr, kg, kb, ib, ir;
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

__device__ __forceinline__ void store4(uint8_t* p, const unsigned v[4])
{
    *reinterpret_cast<uint32_t*>(p) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
}

__device__ __forceinline__ void store4(uint16_t* p, const unsigned v[4])
{
    *reinterpret_cast<uint2*>(p) = make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

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

// Items are the eight-column groups of the PADDED rows: item -> (yp, g), columns 8g .. 8g+7 of row yp of dst.  G = ceil(Wp / 8),
// items = Hp * G per picture, blocks = ceil(items / NT) per picture.  SH: the bits below the code in an element (P010: 6).
template <class T, bool IL, bool WIDE>
__global__ __launch_bounds__(NT) void ingest_kernel(Planes<const T> s, int H, int W, int Hc, int Wc, float* __restrict__ dst, int Hp,
                                                    int Wp, int top, int left, int G, int items, int blocks, int linear, Levels lv,
                                                    IngestCoef k)
{
    constexpr int SH = sizeof(T) == 2 ? 6 : 0;
    constexpr int CS = IL ? 2 : 1;                                // elements from one Cb (Cr) sample to the next
    const int b = blockIdx.x / blocks, blk = blockIdx.x - b * blocks;
    const int item = blk * NT + threadIdx.x;
    if (item >= items) return;
    const int yp = item / G, g = item - yp * G;
    const int xp0 = COLS * g, n = min(COLS, Wp - xp0);            // n columns of dst exist
    const int y = yp - top, x0 = xp0 - left;                      // picture coordinates of the first column
    float o[3][COLS];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < COLS; ++i) o[c][i] = 0.f;
    if (y >= 0 && y < H && x0 + COLS - 1 >= 0 && x0 < W) {
        const int i0 = y >> 1;
        const int i1 = clampi(i0 + ((y & 1) ? 1 : -1), 0, Hc - 1);
        const T* yrow = s.y + b * s.yb + (int64_t)y * s.yr;
        const T* u0 = s.u + b * s.ub + (int64_t)i0 * s.ur;        // Cb of chroma row i0, i1; Cr: one element on, or the V plane
        const T* u1 = s.u + b * s.ub + (int64_t)i1 * s.ur;
        const T* v0 = IL ? u0 + 1 : s.v + b * s.vb + (int64_t)i0 * s.vr;
        const T* v1 = IL ? u1 + 1 : s.v + b * s.vb + (int64_t)i1 * s.vr;
        if (WIDE && x0 >= 0 && x0 + COLS - 1 < W) {               // x0 is a multiple of 8 here (left is)
            unsigned Y[COLS];
            load4(yrow + x0, Y);
            load4(yrow + x0 + 4, Y + 4);
            const int jc = x0 >> 1;                                // chroma columns jc .. jc+3 exist; a multiple of 4
            const int jl = max(jc - 1, 0), jr = min(jc + 4, Wc - 1);
            unsigned cw[2][2][6];                                  // [row i0, i1][Cb, Cr][columns jl, jc .. jc+3, jr]
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const T* pu = r ? u1 : u0;
                const T* pv = r ? v1 : v0;
                if (r == 1 && !linear) {
#pragma unroll
                    for (int j = 0; j < 6; ++j) { cw[1][0][j] = cw[0][0][j]; cw[1][1][j] = cw[0][1][j]; }
                    break;
                }
                if (IL) {
                    unsigned e[8];
                    load4(pu + 2 * (int64_t)jc, e);
                    load4(pu + 2 * (int64_t)jc + 4, e + 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { cw[r][0][1 + j] = e[2 * j]; cw[r][1][1 + j] = e[2 * j + 1]; }
                } else {
                    load4(pu + jc, &cw[r][0][1]);
                    load4(pv + jc, &cw[r][1][1]);
                }
                cw[r][0][0] = pu[CS * (int64_t)jl]; cw[r][1][0] = pv[CS * (int64_t)jl];
                cw[r][0][5] = pu[CS * (int64_t)jr]; cw[r][1][5] = pv[CS * (int64_t)jr];
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
                to_rgb((int)(Y[i] >> SH), c16[0], c16[1], lv, k, o[0][i], o[1][i], o[2][i]);
            }
        } else {                                                  // element by element; also the items that straddle an edge
#pragma unroll
            for (int i = 0; i < COLS; ++i) {
                const int x = x0 + i;
                if (x >= 0 && x < W) {
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
    const int64_t plane = (int64_t)Hp * Wp;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* d = dst + (b * (int64_t)3 + c) * plane + (int64_t)yp * Wp + xp0;
        if (WIDE) {                                               // Wp is a multiple of 8 here: n == 8
            *reinterpret_cast<float4*>(d) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
            *reinterpret_cast<float4*>(d + 4) = make_float4(o[c][4], o[c][5], o[c][6], o[c][7]);
        } else {
#pragma unroll
            for (int i = 0; i < COLS; ++i)
                if (i < n) d[i] = o[c][i];
        }
    }
}

struct F32 {                             // float planes, strides in elements
    const float* p;
    int64_t sb, sc, sh;
};

// One item of the emit: rows 2i and 2i+1 (`rows` of them exist), luma columns x0 .. x0+n-1, chroma row i, columns x0/2 ...  FULL: n == 8
// and every access is wide; else element by element.  The whole item is compiled twice, not only its loads and stores, so that the
// two kinds of access never meet in one basic block (where the compiler merges them into the narrow kind).
template <class T, bool IL, bool FULL, bool HAS_REF>
__device__ __forceinline__ void emit_item(const F32& x, int top, int left, int H, const Planes<T>& dst, const Planes<const T>& ref, int b,
                                          int i, int x0, int n, const Levels& lv, const EmitCoef& k, unsigned long long su[3])
{
    constexpr int SH = sizeof(T) == 2 ? 6 : 0;
    constexpr int CS = IL ? 2 : 1;
    const int nc = (n + 1) >> 1;
    const int rows = min(2, H - 2 * i);                       // 1 at the odd last row
    unsigned yq[2][COLS], cq[2][4];
    float ub[2][COLS], ur[2][COLS];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int yy = min(2 * i + r, H - 1);                 // the last row stands in for the one below it
        float c[3][COLS];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float* s = x.p + b * x.sb + ch * x.sc + (int64_t)(top + yy) * x.sh + left + x0;
            if (FULL) {
                const float4 f0 = *reinterpret_cast<const float4*>(s), f1 = *reinterpret_cast<const float4*>(s + 4);
                c[ch][0] = f0.x; c[ch][1] = f0.y; c[ch][2] = f0.z; c[ch][3] = f0.w;
                c[ch][4] = f1.x; c[ch][5] = f1.y; c[ch][6] = f1.z; c[ch][7] = f1.w;
            } else {
#pragma unroll
                for (int q = 0; q < COLS; ++q) c[ch][q] = s[min(q, n - 1)];   // the last column stands in for those right of it
            }
        }
#pragma unroll
        for (int q = 0; q < COLS; ++q) {
            const float R = clamp01(c[0][q]), Gc = clamp01(c[1][q]), Bc = clamp01(c[2][q]);
            const float Yf = (k.kr * R + k.kg * Gc) + k.kb * Bc;
            const float Cb = (Bc - Yf) * k.ib, Cr = (R - Yf) * k.ir;
            yq[r][q] = (unsigned)clampi((int)rintf(Yf * (float)lv.ys + (float)lv.yo), 0, lv.maxv);
            ub[r][q] = Cb * (float)lv.cs;
            ur[r][q] = Cr * (float)lv.cs;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float mb = ((ub[0][2 * j] + ub[0][2 * j + 1]) + (ub[1][2 * j] + ub[1][2 * j + 1])) * 0.25f + (float)lv.co;
        const float mr = ((ur[0][2 * j] + ur[0][2 * j + 1]) + (ur[1][2 * j] + ur[1][2 * j + 1])) * 0.25f + (float)lv.co;
        cq[0][j] = (unsigned)clampi((int)rintf(mb), 0, lv.maxv);
        cq[1][j] = (unsigned)clampi((int)rintf(mr), 0, lv.maxv);
    }
    if (dst.y) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r < rows) {
                T* d = dst.y + b * dst.yb + (int64_t)(2 * i + r) * dst.yr + x0;
                if (FULL) {
                    unsigned w[COLS];
#pragma unroll
                    for (int q = 0; q < COLS; ++q) w[q] = yq[r][q] << SH;
                    store4(d, w);
                    store4(d + 4, w + 4);
                } else {
#pragma unroll
                    for (int q = 0; q < COLS; ++q)
                        if (q < n) d[q] = (T)(yq[r][q] << SH);
                }
            }
        }
        T* du = dst.u + b * dst.ub + (int64_t)i * dst.ur + CS * (int64_t)(x0 >> 1);
        T* dv = IL ? du + 1 : dst.v + b * dst.vb + (int64_t)i * dst.vr + (x0 >> 1);
        if (FULL) {
            if (IL) {
                unsigned w[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) { w[2 * j] = cq[0][j] << SH; w[2 * j + 1] = cq[1][j] << SH; }
                store4(du, w);
                store4(du + 4, w + 4);
            } else {
                unsigned w[2][4];
#pragma unroll
                for (int j = 0; j < 4; ++j) { w[0][j] = cq[0][j] << SH; w[1][j] = cq[1][j] << SH; }
                store4(du, w[0]);
                store4(dv, w[1]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nc) { du[CS * j] = (T)(cq[0][j] << SH); dv[CS * j] = (T)(cq[1][j] << SH); }
        }
    }
    if (HAS_REF) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r < rows) {
                const T* s = ref.y + b * ref.yb + (int64_t)(2 * i + r) * ref.yr + x0;
                unsigned w[COLS];
                if (FULL) {
                    load4(s, w);
                    load4(s + 4, w + 4);
                } else {
#pragma unroll
                    for (int q = 0; q < COLS; ++q) w[q] = q < n ? (unsigned)s[q] : 0u;
                }
#pragma unroll
                for (int q = 0; q < COLS; ++q) {
                    if (q < n) {
                        const int e = (int)yq[r][q] - (int)(w[q] >> SH);
                        su[0] += (unsigned long long)(e * e);
                    }
                }
            }
        }
        const T* ru = ref.u + b * ref.ub + (int64_t)i * ref.ur + CS * (int64_t)(x0 >> 1);
        const T* rv = IL ? ru + 1 : ref.v + b * ref.vb + (int64_t)i * ref.vr + (x0 >> 1);
        unsigned w[2][4];
        if (FULL) {
            if (IL) {
                unsigned e[8];
                load4(ru, e);
                load4(ru + 4, e + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) { w[0][j] = e[2 * j]; w[1][j] = e[2 * j + 1]; }
            } else {
                load4(ru, w[0]);
                load4(rv, w[1]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                w[0][j] = j < nc ? (unsigned)ru[CS * j] : 0u;
                w[1][j] = j < nc ? (unsigned)rv[CS * j] : 0u;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < nc) {
                const int eb = (int)cq[0][j] - (int)(w[0][j] >> SH), er = (int)cq[1][j] - (int)(w[1][j] >> SH);
                su[1] += (unsigned long long)(eb * eb);
                su[2] += (unsigned long long)(er * er);
            }
        }
    }
}

// Items are the eight-column groups of the WINDOW's row pairs: item -> (i, g), rows 2i and 2i+1, columns 8g .. 8g+7 of the picture,
// chroma row i, columns 4g .. 4g+3.  G = ceil(W / 8), items = Hc * G per picture.  partials: [gridDim.x][3].
template <class T, bool IL, bool WIDE, bool HAS_REF>
__global__ __launch_bounds__(NT) void emit_kernel(F32 x, int top, int left, int H, int W, Planes<T> dst, Planes<const T> ref, int G,
                                                  int items, int blocks, Levels lv, EmitCoef k,
                                                  unsigned long long* __restrict__ partials)
{
    __shared__ unsigned long long red[NT / 64][3];
    const int b = blockIdx.x / blocks, blk = blockIdx.x - b * blocks;
    const int item = blk * NT + threadIdx.x;
    unsigned long long su[3] = {0ull, 0ull, 0ull};
    if (item < items) {
        const int i = item / G, g = item - i * G;
        const int x0 = COLS * g, n = min(COLS, W - x0);           // n luma columns exist
        if (WIDE && n == COLS) emit_item<T, IL, true, HAS_REF>(x, top, left, H, dst, ref, b, i, x0, n, lv, k, su);
        else emit_item<T, IL, false, HAS_REF>(x, top, left, H, dst, ref, b, i, x0, n, lv, k, su);
    }
    if (HAS_REF) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
#pragma unroll
            for (int p = 0; p < 3; ++p) su[p] += __shfl_down(su[p], off, 64);
        if ((threadIdx.x & 63) == 0)
#pragma unroll
            for (int p = 0; p < 3; ++p) red[threadIdx.x >> 6][p] = su[p];
        __syncthreads();
        if (threadIdx.x < 3) {
            unsigned long long a = red[0][threadIdx.x];
            for (int wv = 1; wv < NT / 64; ++wv) a += red[wv][threadIdx.x];
            partials[(int64_t)blockIdx.x * 3 + threadIdx.x] = a;
        }
    }
}

// One block per picture: its block partials (thread t takes t, t + NT, ...; wave tree; waves in order).
__global__ __launch_bounds__(NT) void emit_final_kernel(const unsigned long long* __restrict__ partials, int blocks,
                                                        unsigned long long* __restrict__ sse)
{
    __shared__ unsigned long long red[NT / 64][3];
    const int b = blockIdx.x;
    const unsigned long long* p = partials + (int64_t)b * blocks * 3;
    unsigned long long su[3] = {0ull, 0ull, 0ull};
    for (int t = threadIdx.x; t < blocks; t += NT)
#pragma unroll
        for (int c = 0; c < 3; ++c) su[c] += p[(int64_t)t * 3 + c];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int c = 0; c < 3; ++c) su[c] += __shfl_down(su[c], off, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int c = 0; c < 3; ++c) red[threadIdx.x >> 6][c] = su[c];
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long a = red[0][threadIdx.x];
        for (int wv = 1; wv < NT / 64; ++wv) a += red[wv][threadIdx.x];
        sse[b * 3 + threadIdx.x] = a;
    }
}

bool fmt_ok(int fmt) { return fmt == PC_FRAMES_NV12 || fmt == PC_FRAMES_I420 || fmt == PC_FRAMES_P010; }
bool interleaved(int fmt) { return fmt != PC_FRAMES_I420; }
int elem_bytes(int fmt) { return fmt == PC_FRAMES_P010 ? 2 : 1; }

bool levels_of(int fmt, int range, Levels& lv)
{
    const int n = fmt == PC_FRAMES_P010 ? 10 : 8, s = 1 << (n - 8), maxv = (1 << n) - 1;
    if (range == PC_FRAMES_LIMITED) lv = Levels{16 * s, 219 * s, 128 * s, 224 * s, maxv};
    else if (range == PC_FRAMES_FULL) lv = Levels{0, maxv, 128 * s, maxv, maxv};
    else return false;
    return true;
}

// One plane of B pictures of `rows` rows of `len` elements: pointer aligned to its element, strides in range; `disjoint`
// (destinations): rows inside pictures, which is sufficient (not necessary) for no element of the plane to be written twice.
bool plane_ok(const void* p, int64_t sb, int64_t sr, int es, int B, int rows, int64_t len, bool disjoint)
{
    if (!p || reinterpret_cast<uintptr_t>(p) % es || sr < len || sb < 1) return false;
    if (disjoint && B > 1 && sb < (int64_t)(rows - 1) * sr + len) return false;
    return true;
}

bool frame_ok(int fmt, const pc_frame* f, int B, int H, int W, bool disjoint)
{
    if (!f || !fmt_ok(fmt)) return false;
    const int es = elem_bytes(fmt), Hc = (int)cdiv(H, 2);
    const int64_t Wc = cdiv(W, 2);
    if (!plane_ok(f->y, f->y_batch, f->y_row, es, B, H, W, disjoint)) return false;
    if (interleaved(fmt)) return plane_ok(f->u, f->u_batch, f->u_row, es, B, Hc, 2 * Wc, disjoint);
    return plane_ok(f->u, f->u_batch, f->u_row, es, B, Hc, Wc, disjoint) && plane_ok(f->v, f->v_batch, f->v_row, es, B, Hc, Wc, disjoint);
}

// Sizes every call shares: B, rows, cols >= 1 and the block count of an item space of rows x ceil(cols / 8) per picture in 32 bits.
struct Grid {
    int G, items, blocks;
};

bool grid_of(int B, int rows, int cols, Grid& g)
{
    if (B < 1 || rows < 1 || cols < 1) return false;
    const int64_t G = cdiv(cols, COLS), items = (int64_t)rows * G;
    if (items > INT32_MAX - NT) return false;
    const int64_t blocks = cdiv(items, NT);
    if ((int64_t)B * blocks > INT32_MAX) return false;
    g.G = (int)G;
    g.items = (int)items;
    g.blocks = (int)blocks;
    return true;
}

bool mult4(int64_t v) { return v % 4 == 0; }

// The alignment of a frame as the wide path needs it: every plane pointer on four elements, every stride a multiple of 4.
bool frame_wide(int fmt, const pc_frame* f)
{
    const uintptr_t a = 4 * (uintptr_t)elem_bytes(fmt);
    if (reinterpret_cast<uintptr_t>(f->y) % a || !mult4(f->y_batch) || !mult4(f->y_row)) return false;
    if (reinterpret_cast<uintptr_t>(f->u) % a || !mult4(f->u_batch) || !mult4(f->u_row)) return false;
    if (!interleaved(fmt) && (reinterpret_cast<uintptr_t>(f->v) % a || !mult4(f->v_batch) || !mult4(f->v_row))) return false;
    return true;
}

// The one place that decides the access path: the calls launch from it, pc_frames_plan reports it.
bool wide_path(int op, int fmt, const pc_frame* frame, const void* f32, int64_t fb, int64_t fc, int64_t fh, int left,
               const pc_frame* ref)
{
    if (reinterpret_cast<uintptr_t>(f32) % 16 || !mult4(fb) || !mult4(fc) || !mult4(fh)) return false;
    if (op == PC_FRAMES_INGEST) return fh % 8 == 0 && left % 8 == 0 && frame_wide(fmt, frame);     // fh = Wp: no partial last item
    return left % 4 == 0 && (!frame || frame_wide(fmt, frame)) && (!ref || frame_wide(fmt, ref));
}

bool window_ok(int B, int H, int W, int Hp, int Wp, int top, int left)
{
    if (B < 1 || H < 1 || W < 1 || top < 0 || left < 0 || Hp < 1 || Wp < 1) return false;
    return (int64_t)top + H <= Hp && (int64_t)left + W <= Wp;
}

template <class T>
Planes<T> planes_of(const pc_frame* f)
{
    if (!f) return Planes<T>{nullptr, 0, 0, nullptr, 0, 0, nullptr, 0, 0};
    return Planes<T>{static_cast<T*>(f->y), f->y_batch, f->y_row, static_cast<T*>(f->u), f->u_batch, f->u_row, static_cast<T*>(f->v),
                     f->v_batch, f->v_row};
}

template <class T, bool IL>
void launch_ingest(bool wide, dim3 grid, hipStream_t st, const pc_frame* src, int H, int W, float* dst, int Hp, int Wp, int top, int left,
                   const Grid& g, int linear, const Levels& lv, const IngestCoef& k)
{
    const Planes<const T> s = planes_of<const T>(src);
    const int Hc = (H + 1) / 2, Wc = (W + 1) / 2;
    if (wide)
        hipLaunchKernelGGL((ingest_kernel<T, IL, true>), grid, dim3(NT), 0, st, s, H, W, Hc, Wc, dst, Hp, Wp, top, left, g.G, g.items,
                           g.blocks, linear, lv, k);
    else
        hipLaunchKernelGGL((ingest_kernel<T, IL, false>), grid, dim3(NT), 0, st, s, H, W, Hc, Wc, dst, Hp, Wp, top, left, g.G, g.items,
                           g.blocks, linear, lv, k);
}

template <class T, bool IL>
void launch_emit(bool wide, bool has_ref, dim3 grid, hipStream_t st, const F32& x, int top, int left, int H, int W, const pc_frame* dst,
                 const pc_frame* ref, const Grid& g, const Levels& lv, const EmitCoef& k, unsigned long long* part)
{
    const Planes<T> d = planes_of<T>(dst);
    const Planes<const T> r = planes_of<const T>(ref);
#define PC_EMIT(WIDE, REF)                                                                                                            \
    hipLaunchKernelGGL((emit_kernel<T, IL, WIDE, REF>), grid, dim3(NT), 0, st, x, top, left, H, W, d, r, g.G, g.items, g.blocks, lv, k, \
                       part)
    if (has_ref) {
        if (wide) PC_EMIT(true, true); else PC_EMIT(false, true);
    } else {
        if (wide) PC_EMIT(true, false); else PC_EMIT(false, false);
    }
#undef PC_EMIT
}

}  // namespace

extern "C" int pc_frames_plan(int op, int fmt, const pc_frame* frame, const void* f32, int64_t fb, int64_t fc, int64_t fh, int left,
                              const pc_frame* ref, int* wide)
{
    if ((op != PC_FRAMES_INGEST && op != PC_FRAMES_EMIT) || !fmt_ok(fmt) || !f32 || !wide || left < 0) return PC_ERR_ARG;
    if (op == PC_FRAMES_INGEST) ref = nullptr;
    if (!frame && (op != PC_FRAMES_EMIT || !ref)) return PC_ERR_ARG;
    for (const pc_frame* f : {frame, ref})
        if (f && (!f->y || !f->u || (!interleaved(fmt) && !f->v))) return PC_ERR_ARG;
    *wide = wide_path(op, fmt, frame, f32, fb, fc, fh, left, ref) ? 1 : 0;
    return PC_OK;
}

extern "C" int pc_frames_ingest(const pc_frame* src, int fmt, int range, int upsample, float a, float b, float c, float d, int B, int H,
                                int W, float* dst, int Hp, int Wp, int top, int left, void* stream)
{
    Grid g;
    Levels lv;
    if (!dst || reinterpret_cast<uintptr_t>(dst) % 4 || !window_ok(B, H, W, Hp, Wp, top, left)) return PC_ERR_ARG;
    if (!frame_ok(fmt, src, B, H, W, false) || !levels_of(fmt, range, lv)) return PC_ERR_ARG;
    if (upsample != PC_FRAMES_NEAREST && upsample != PC_FRAMES_LINEAR) return PC_ERR_ARG;
    if (!grid_of(B, Hp, Wp, g)) return PC_ERR_ARG;
    const int64_t plane = (int64_t)Hp * Wp;
    const bool wide = wide_path(PC_FRAMES_INGEST, fmt, src, dst, 3 * plane, plane, Wp, left, nullptr);
    const IngestCoef k{a, b, c, d};
    const int linear = upsample == PC_FRAMES_LINEAR;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(B * g.blocks));
    if (fmt == PC_FRAMES_NV12) launch_ingest<uint8_t, true>(wide, grid, st, src, H, W, dst, Hp, Wp, top, left, g, linear, lv, k);
    else if (fmt == PC_FRAMES_I420) launch_ingest<uint8_t, false>(wide, grid, st, src, H, W, dst, Hp, Wp, top, left, g, linear, lv, k);
    else launch_ingest<uint16_t, true>(wide, grid, st, src, H, W, dst, Hp, Wp, top, left, g, linear, lv, k);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

extern "C" size_t pc_frames_emit_workspace_size(int B, int H, int W)
{
    Grid g;
    return H >= 1 && grid_of(B, (int)cdiv(H, 2), W, g) ? (size_t)B * g.blocks * 3 * sizeof(unsigned long long) : 0;
}

extern "C" int pc_frames_emit(const float* x, int64_t sxb, int64_t sxc, int64_t sxh, int Hp, int Wp, int top, int left, int B, int H,
                              int W, int fmt, int range, float kr, float kg, float kb, float ib, float ir, const pc_frame* dst,
                              const pc_frame* ref, void* workspace, size_t workspace_bytes, uint64_t* sse, void* stream)
{
    Grid g;
    Levels lv;
    if (!x || reinterpret_cast<uintptr_t>(x) % 4 || !window_ok(B, H, W, Hp, Wp, top, left)) return PC_ERR_ARG;
    if (sxh < Wp || sxc < 1 || sxb < 1 || !fmt_ok(fmt) || !levels_of(fmt, range, lv)) return PC_ERR_ARG;
    if (!dst && !ref) return PC_ERR_ARG;
    if (dst && !frame_ok(fmt, dst, B, H, W, true)) return PC_ERR_ARG;
    if (ref && !frame_ok(fmt, ref, B, H, W, false)) return PC_ERR_ARG;
    if (!grid_of(B, (int)cdiv(H, 2), W, g)) return PC_ERR_ARG;
    if (ref) {
        if (!workspace || reinterpret_cast<uintptr_t>(workspace) % 8 || !sse || reinterpret_cast<uintptr_t>(sse) % 8) return PC_ERR_ARG;
        if (workspace_bytes < (size_t)B * g.blocks * 3 * sizeof(unsigned long long)) return PC_ERR_ARG;
    }
    const bool wide = wide_path(PC_FRAMES_EMIT, fmt, dst, x, sxb, sxc, sxh, left, ref);
    const F32 xv{x, sxb, sxc, sxh};
    const EmitCoef k{kr, kg, kb, ib, ir};
    unsigned long long* part = static_cast<unsigned long long*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(B * g.blocks));
    if (fmt == PC_FRAMES_NV12) launch_emit<uint8_t, true>(wide, ref != nullptr, grid, st, xv, top, left, H, W, dst, ref, g, lv, k, part);
    else if (fmt == PC_FRAMES_I420) launch_emit<uint8_t, false>(wide, ref != nullptr, grid, st, xv, top, left, H, W, dst, ref, g, lv, k, part);
    else launch_emit<uint16_t, true>(wide, ref != nullptr, grid, st, xv, top, left, H, W, dst, ref, g, lv, k, part);
    HIPCHK(hipGetLastError());
    if (ref) {
        hipLaunchKernelGGL(emit_final_kernel, dim3((unsigned)B), dim3(NT), 0, st, part, g.blocks, reinterpret_cast<unsigned long long*>(sse));
        HIPCHK(hipGetLastError());
    }
    return PC_OK;
}

extern "C" const char* pc_frames_strerror(int code)
{
    switch (code) {
    case PC_OK: return "ok";
    case PC_ERR_ARG: return "invalid argument, unknown format, unsupported shape or workspace too small (pc_frames_emit_workspace_size)";
    case PC_ERR_HIP: return "HIP runtime error";
    default: return "unknown error";
    }
}

extern "C" int pc_frames_last_hip_error(void) { return g_last_hip.load(); }

// pc_metrics.hip -- MS-SSIM / SSIM on gfx950 (pc_metrics.h).  Definition: DESIGN.md section 9.
//
// Per call, for each scale s < levels: one msssim_scale launch (a block = one output tile of one (b, c) plane; its two partial sums
// go to a slab [s][plane][tile]), then, except after the last scale, one pool2x2 launch into the workspace.  One msssim_final launch
// reduces the slabs per image.  Every sum runs in a fixed order (no atomics), and no block reads two planes, so a value is bitwise
// reproducible and independent of the image's batch neighbours.
#include <cmath>

#include "pc_image_host.h"

#include "pc_metrics.h"

namespace {

constexpr int TH = 32;         // output rows per tile
constexpr int TW = 64;         // output columns per tile
constexpr int NT = 256;        // threads per block (4 waves)
constexpr int RPT = 8;         // H pass: output rows per work item; W pass: output columns per thread
constexpr int MAX_WIN = 31;
constexpr int MAX_LEVELS = 5;

struct Taps {
    float g[MAX_WIN + 1];
};

struct FinalArgs {
    int levels, C, nonnegative;
    int tiles[MAX_LEVELS];
    int64_t slab_off[MAX_LEVELS];      // in f64 pairs
    double count[MAX_LEVELS];          // output pixels of a plane at scale s
    double w[MAX_LEVELS];
};

inline int64_t align256(int64_t n) { return (n + 255) / 256 * 256; }

// Staged plane tile: (TH + WS - 1) rows of SX floats (16-byte rows for float4 stores); the H pass output: five moments of TH rows of
// SV floats, SV odd so that the W pass (lane = row) reads 32 distinct banks.
template <int WS> struct Tile {
    static constexpr int R = TH + WS - 1;
    static constexpr int CC = TW + WS - 1;
    static constexpr int SX = (CC + 3) / 4 * 4;
    static constexpr int SV = CC | 1;
    static constexpr int NQ = SX / 4;
    static constexpr int LDS_FLOATS = 2 * R * SX + 5 * TH * SV;
};

template <int WS>
__global__ __launch_bounds__(NT) void msssim_scale_kernel(const float* __restrict__ X, int64_t sxb, int64_t sxc, int64_t sxh,
                                                          const float* __restrict__ Y, int64_t syb, int64_t syc, int64_t syh,
                                                          int C, int H, int W, int tiles_x, int tiles, int vec, Taps taps, float C1,
                                                          float C2, double2* __restrict__ slab)
{
    using T = Tile<WS>;
    __shared__ __attribute__((aligned(16))) float lds[T::LDS_FLOATS];
    __shared__ double red[2 * (NT / 64)];
    float* sX = lds;
    float* sY = lds + T::R * T::SX;
    float* sV = lds + 2 * T::R * T::SX;                  // [5][TH][SV]

    const int tid = threadIdx.x;
    const int plane = blockIdx.x / tiles;
    const int tile = blockIdx.x - plane * tiles;
    const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
    const int b = plane / C, c = plane - b * C;
    const float* xp = X + b * sxb + c * sxc;
    const float* yp = Y + b * syb + c * syc;
    const int Ho = H - WS + 1, Wo = W - WS + 1;

    // 1) stage X and Y rows y0 .. y0+R-1, columns x0 .. x0+SX-1 (zeros past the plane: they only feed outputs that are masked)
    for (int q = tid; q < T::R * T::NQ; q += NT) {
        const int r = q / T::NQ, cq = q - r * T::NQ;
        const int gy = y0 + r, gx = x0 + 4 * cq;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), d = a;
        if (gy < H) {
            const float* xr = xp + gy * sxh + gx;
            const float* yr = yp + gy * syh + gx;
            if (vec && gx + 3 < W) {
                a = *reinterpret_cast<const float4*>(xr);
                d = *reinterpret_cast<const float4*>(yr);
            } else {
                if (gx + 0 < W) { a.x = xr[0]; d.x = yr[0]; }
                if (gx + 1 < W) { a.y = xr[1]; d.y = yr[1]; }
                if (gx + 2 < W) { a.z = xr[2]; d.z = yr[2]; }
                if (gx + 3 < W) { a.w = xr[3]; d.w = yr[3]; }
            }
        }
        *reinterpret_cast<float4*>(sX + r * T::SX + 4 * cq) = a;
        *reinterpret_cast<float4*>(sY + r * T::SX + 4 * cq) = d;
    }
    __syncthreads();

    // 2) H pass: a work item = one staged column x RPT consecutive output rows; the products are formed in f32 on the fly and every
    //    tap is an fmaf, taps in order
    for (int it = tid; it < T::CC * (TH / RPT); it += NT) {
        const int col = it % T::CC, r0 = (it / T::CC) * RPT;
        float acc[RPT][5];
#pragma unroll
        for (int o = 0; o < RPT; ++o)
#pragma unroll
            for (int m = 0; m < 5; ++m) acc[o][m] = 0.f;
#pragma unroll
        for (int i = 0; i < RPT + WS - 1; ++i) {
            const float xv = sX[(r0 + i) * T::SX + col], yv = sY[(r0 + i) * T::SX + col];
            const float v[5] = {xv, yv, xv * xv, yv * yv, xv * yv};
#pragma unroll
            for (int o = 0; o < RPT; ++o) {
                const int k = i - o;
                if (k >= 0 && k < WS) {
#pragma unroll
                    for (int m = 0; m < 5; ++m) acc[o][m] = fmaf(taps.g[k], v[m], acc[o][m]);
                }
            }
        }
#pragma unroll
        for (int o = 0; o < RPT; ++o)
#pragma unroll
            for (int m = 0; m < 5; ++m) sV[(m * TH + r0 + o) * T::SV + col] = acc[o][m];
    }
    __syncthreads();

    // 3) W pass: thread = one output row x RPT consecutive output columns; then the two maps, summed in f64
    const int r = tid % TH, c0 = (tid / TH) * RPT;
    float mom[5][RPT];
#pragma unroll
    for (int m = 0; m < 5; ++m) {
        float acc[RPT];
#pragma unroll
        for (int o = 0; o < RPT; ++o) acc[o] = 0.f;
        const float* row = sV + (m * TH + r) * T::SV + c0;
#pragma unroll
        for (int i = 0; i < RPT + WS - 1; ++i) {
            const float v = row[i];
#pragma unroll
            for (int o = 0; o < RPT; ++o) {
                const int k = i - o;
                if (k >= 0 && k < WS) acc[o] = fmaf(taps.g[k], v, acc[o]);
            }
        }
#pragma unroll
        for (int o = 0; o < RPT; ++o) mom[m][o] = acc[o];
    }
    double s_ssim = 0.0, s_cs = 0.0;
    if (y0 + r < Ho) {
#pragma unroll
        for (int o = 0; o < RPT; ++o) {
            if (x0 + c0 + o < Wo) {
                const float mu1 = mom[0][o], mu2 = mom[1][o];
                const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
                const float s1 = mom[2][o] - mu1_sq, s2 = mom[3][o] - mu2_sq, s12 = mom[4][o] - mu12;
                const float cs = (2.f * s12 + C2) / (s1 + s2 + C2);
                const float ss = ((2.f * mu12 + C1) / (mu1_sq + mu2_sq + C1)) * cs;
                s_ssim += (double)ss;
                s_cs += (double)cs;
            }
        }
    }
    // 4) block sum in a fixed order: wave tree, then the four waves in order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s_ssim += __shfl_down(s_ssim, off, 64);
        s_cs += __shfl_down(s_cs, off, 64);
    }
    if ((tid & 63) == 0) {
        red[2 * (tid >> 6)] = s_ssim;
        red[2 * (tid >> 6) + 1] = s_cs;
    }
    __syncthreads();
    if (tid == 0) {
        double a = red[0], d = red[1];
        for (int wv = 1; wv < NT / 64; ++wv) {
            a += red[2 * wv];
            d += red[2 * wv + 1];
        }
        slab[(int64_t)plane * tiles + tile] = make_double2(a, d);
    }
}

// avg_pool2d(kernel 2, stride 2, padding (H % 2, W % 2), count_include_pad): an odd side gets a zero on both ends, the divisor stays 4.
// Output planes are contiguous [B*C][Hp][Wp].
__global__ __launch_bounds__(NT) void pool2x2_kernel(const float* __restrict__ X, int64_t sxb, int64_t sxc, int64_t sxh,
                                                     const float* __restrict__ Y, int64_t syb, int64_t syc, int64_t syh, int C, int H,
                                                     int W, int Hp, int Wp, int64_t total, float* __restrict__ Xp, float* __restrict__ Yp)
{
    const int ph = H & 1, pw = W & 1;
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
        const int ox = (int)(i % Wp);
        const int64_t t = i / Wp;
        const int oy = (int)(t % Hp);
        const int plane = (int)(t / Hp);
        const int b = plane / C, c = plane - b * C;
        const int iy = 2 * oy - ph, ix = 2 * ox - pw;
        const bool r0 = iy >= 0, r1 = iy + 1 < H, q0 = ix >= 0, q1 = ix + 1 < W;
        const float* xr = X + b * sxb + c * sxc + (int64_t)iy * sxh + ix;
        const float* yr = Y + b * syb + c * syc + (int64_t)iy * syh + ix;
        const float x00 = (r0 && q0) ? xr[0] : 0.f, x01 = (r0 && q1) ? xr[1] : 0.f;
        const float x10 = (r1 && q0) ? xr[sxh] : 0.f, x11 = (r1 && q1) ? xr[sxh + 1] : 0.f;
        const float y00 = (r0 && q0) ? yr[0] : 0.f, y01 = (r0 && q1) ? yr[1] : 0.f;
        const float y10 = (r1 && q0) ? yr[syh] : 0.f, y11 = (r1 && q1) ? yr[syh + 1] : 0.f;
        Xp[i] = (((x00 + x01) + x10) + x11) * 0.25f;
        Yp[i] = (((y00 + y01) + y10) + y11) * 0.25f;
    }
}

// One block per image: the slab sums of every (scale, channel) in a fixed order, their means, relu / pow per (scale, channel) in
// parallel lanes, the product per channel and the mean over channels.
__global__ __launch_bounds__(NT) void msssim_final_kernel(const double2* __restrict__ slab, FinalArgs a, int B, float* __restrict__ out,
                                                          double* __restrict__ out_scales)
{
    constexpr int CB = 64;                           // channels per pass
    __shared__ double mean[MAX_LEVELS * 2 * CB];     // [s][k][c]
    __shared__ double term[MAX_LEVELS * CB];         // [s][c]: relu(m)^w, or the (relu'd) SSIM when levels == 1
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double total = 0.0;                              // thread 0 only
    for (int cb = 0; cb < a.C; cb += CB) {
        const int nc = min(CB, a.C - cb);
        for (int job = wave; job < a.levels * nc; job += NT / 64) {
            const int s = job / nc, c = cb + job % nc;
            const double2* p = slab + a.slab_off[s] + (int64_t)(b * a.C + c) * a.tiles[s];
            double x = 0.0, y = 0.0;
            for (int t = lane; t < a.tiles[s]; t += 64) {
                x += p[t].x;
                y += p[t].y;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                x += __shfl_down(x, off, 64);
                y += __shfl_down(y, off, 64);
            }
            if (lane == 0) {
                mean[(s * 2 + 0) * CB + (c - cb)] = x / a.count[s];
                mean[(s * 2 + 1) * CB + (c - cb)] = y / a.count[s];
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < a.levels * nc; i += NT) {
            const int s = i / nc, ci = i % nc;
            if (out_scales)
                for (int k = 0; k < 2; ++k) out_scales[((int64_t)(s * 2 + k) * B + b) * a.C + cb + ci] = mean[(s * 2 + k) * CB + ci];
            double m = mean[(s * 2 + (s == a.levels - 1 ? 0 : 1)) * CB + ci];
            if (a.levels == 1) {
                term[ci] = (a.nonnegative && m < 0.0) ? 0.0 : m;
            } else {
                m = m < 0.0 ? 0.0 : m;
                term[s * CB + ci] = pow(m, a.w[s]);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int ci = 0; ci < nc; ++ci) {
                double v = term[ci];
                for (int s = 1; s < a.levels; ++s) v *= term[s * CB + ci];
                total += v;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[b] = (float)(total / a.C);
}

struct Geometry {
    int levels, P;
    int H[MAX_LEVELS], W[MAX_LEVELS], tiles_x[MAX_LEVELS], tiles[MAX_LEVELS];
    int64_t slab_off[MAX_LEVELS], pooled_off[MAX_LEVELS], bytes;
};

// Shapes, tile counts and workspace layout; false if the arguments are out of range.
bool geometry(int B, int C, int H, int W, int ws, int levels, Geometry& g)
{
    if (B < 1 || C < 1 || H < 1 || W < 1 || ws < 1 || ws > MAX_WIN || (ws & 1) == 0 || levels < 1 || levels > MAX_LEVELS) return false;
    if (levels == 1 ? (H < ws || W < ws) : ((int64_t)(H < W ? H : W) <= (int64_t)(ws - 1) * 16)) return false;
    g.levels = levels;
    if ((int64_t)B * C > INT32_MAX) return false;
    g.P = B * C;
    int64_t slab = 0;
    for (int s = 0; s < levels; ++s) {
        g.H[s] = s ? (g.H[s - 1] + 1) / 2 : H;
        g.W[s] = s ? (g.W[s - 1] + 1) / 2 : W;
        const int64_t tx = cdiv(g.W[s] - ws + 1, TW), ty = cdiv(g.H[s] - ws + 1, TH);
        if ((int64_t)g.P * tx * ty > INT32_MAX / NT) return false;     // grid size in work-items fits 32 bits
        g.tiles_x[s] = (int)tx;
        g.tiles[s] = (int)(tx * ty);
        g.slab_off[s] = slab;
        slab += (int64_t)g.P * g.tiles[s];
    }
    int64_t off = align256(slab * 16);
    for (int s = 1; s < levels; ++s) {
        g.pooled_off[s] = off;
        off += 2 * align256((int64_t)g.P * g.H[s] * g.W[s] * 4);
    }
    g.bytes = off;
    return true;
}

template <int WS>
void launch_scale(const float* X, int64_t sxb, int64_t sxc, int64_t sxh, const float* Y, int64_t syb, int64_t syc, int64_t syh, int C,
                  int H, int W, int tiles_x, int tiles, int P, int vec, const Taps& taps, float C1, float C2, double2* slab,
                  hipStream_t st)
{
    hipLaunchKernelGGL(msssim_scale_kernel<WS>, dim3(P * tiles), dim3(NT), 0, st, X, sxb, sxc, sxh, Y, syb, syc, syh, C, H, W, tiles_x,
                       tiles, vec, taps, C1, C2, slab);
}

using ScaleLaunch = decltype(&launch_scale<1>);
const ScaleLaunch kScale[] = {launch_scale<1>, launch_scale<3>, launch_scale<5>, launch_scale<7>, launch_scale<9>, launch_scale<11>,
                              launch_scale<13>, launch_scale<15>, launch_scale<17>, launch_scale<19>, launch_scale<21>,
                              launch_scale<23>, launch_scale<25>, launch_scale<27>, launch_scale<29>, launch_scale<31>};

// The inputs of every scale as the scale and pool kernels read them, and the staging path of each: scale 0 is the caller's X and Y, scale
// s > 0 the pooled planes in the workspace.  vec = 1 (16-byte staging loads) needs both bases 16-byte aligned and all six strides
// multiples of four floats.  The one place that decides it: pc_msssim launches from this, pc_msssim_plan reports it.
struct ScaleView {
    const float *x, *y;
    int64_t xb, xc, xh, yb, yc, yh;
    int vec;
};

void scale_views(const Geometry& g, int C, const float* X, int64_t sxb, int64_t sxc, int64_t sxh, const float* Y, int64_t syb,
                 int64_t syc, int64_t syh, const void* workspace, ScaleView* v)
{
    const char* ws = static_cast<const char*>(workspace);
    for (int s = 0; s < g.levels; ++s) {
        ScaleView& a = v[s];
        if (s == 0) {
            a = ScaleView{X, Y, sxb, sxc, sxh, syb, syc, syh, 0};
        } else {
            const int64_t hw = (int64_t)g.H[s] * g.W[s];
            a.x = reinterpret_cast<const float*>(ws + g.pooled_off[s]);
            a.y = reinterpret_cast<const float*>(ws + g.pooled_off[s] + align256((int64_t)g.P * hw * 4));
            a.xc = a.yc = hw;
            a.xb = a.yb = (int64_t)C * hw;
            a.xh = a.yh = g.W[s];
        }
        a.vec = (reinterpret_cast<uintptr_t>(a.x) % 16 == 0 && reinterpret_cast<uintptr_t>(a.y) % 16 == 0 && a.xb % 4 == 0 &&
                 a.xc % 4 == 0 && a.xh % 4 == 0 && a.yb % 4 == 0 && a.yc % 4 == 0 && a.yh % 4 == 0);
    }
}

}  // namespace

extern "C" int pc_msssim_plan(const float* X, int64_t sxb, int64_t sxc, int64_t sxh, const float* Y, int64_t syb, int64_t syc,
                              int64_t syh, int B, int C, int H, int W, int win_size, int levels, const void* workspace, int* vec)
{
    Geometry g;
    if (!X || !Y || !workspace || !vec || !geometry(B, C, H, W, win_size, levels, g)) return PC_ERR_ARG;
    if (sxb < 1 || sxc < 1 || sxh < 1 || syb < 1 || syc < 1 || syh < 1) return PC_ERR_ARG;
    ScaleView v[MAX_LEVELS];
    scale_views(g, C, X, sxb, sxc, sxh, Y, syb, syc, syh, workspace, v);
    for (int s = 0; s < levels; ++s) vec[s] = v[s].vec;
    return PC_OK;
}

extern "C" size_t pc_msssim_workspace_size(int B, int C, int H, int W, int win_size, int levels)
{
    Geometry g;
    return geometry(B, C, H, W, win_size, levels, g) ? (size_t)g.bytes : 0;
}

extern "C" int pc_msssim(const float* X, int64_t sxb, int64_t sxc, int64_t sxh, const float* Y, int64_t syb, int64_t syc, int64_t syh,
                         int B, int C, int H, int W, float data_range, int win_size, float win_sigma, float K1, float K2, int levels,
                         const float* weights, int nonnegative, void* workspace, size_t workspace_bytes, float* out,
                         double* out_scales, void* stream)
{
    Geometry g;
    if (!X || !Y || !out || !workspace || !geometry(B, C, H, W, win_size, levels, g)) return PC_ERR_ARG;
    if (sxb < 1 || sxc < 1 || sxh < 1 || syb < 1 || syc < 1 || syh < 1) return PC_ERR_ARG;
    if (!std::isfinite(data_range) || !std::isfinite(K1) || !std::isfinite(K2) || !(win_sigma > 0.f) || !std::isfinite(win_sigma))
        return PC_ERR_ARG;
    FinalArgs fa{};
    fa.levels = levels;
    fa.C = C;
    fa.nonnegative = nonnegative ? 1 : 0;
    if (levels > 1) {
        if (!weights) return PC_ERR_ARG;
        for (int s = 0; s < levels; ++s) {
            if (!std::isfinite(weights[s])) return PC_ERR_ARG;
            fa.w[s] = weights[s];
        }
    }
    if (workspace_bytes < (size_t)g.bytes) return PC_ERR_BUFFER;

    // the window, in float32 as the library builds it: exp(-(i - ws/2)^2 / (2 sigma^2)), divided by its sum.  The sum is the float32
    // rounding of the exact sum (accumulated in f64), which is what torch's vectorised float sum gives for the default window: the
    // E[X^2] - mu^2 form amplifies a tap-sum offset by mu^2 / sigma^2, so the window's last bits matter on smooth images
    Taps taps{};
    const float two_s2 = (float)(2.0 * (double)win_sigma * (double)win_sigma);
    double sum = 0.0;
    for (int i = 0; i < win_size; ++i) {
        const float d = (float)(i - win_size / 2);
        taps.g[i] = std::exp(-(d * d) / two_s2);
        sum += (double)taps.g[i];
    }
    for (int i = 0; i < win_size; ++i) taps.g[i] /= (float)sum;
    const float C1 = (K1 * data_range) * (K1 * data_range), C2 = (K2 * data_range) * (K2 * data_range);

    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    double2* slab = reinterpret_cast<double2*>(ws);
    ScaleView sv[MAX_LEVELS];
    scale_views(g, C, X, sxb, sxc, sxh, Y, syb, syc, syh, workspace, sv);
    for (int s = 0; s < levels; ++s) {
        const int h = g.H[s], w = g.W[s];
        const ScaleView& a = sv[s];
        kScale[win_size / 2](a.x, a.xb, a.xc, a.xh, a.y, a.yb, a.yc, a.yh, C, h, w, g.tiles_x[s], g.tiles[s], g.P, a.vec, taps, C1, C2,
                             slab + g.slab_off[s], st);
        HIPCHK(hipGetLastError());
        fa.tiles[s] = g.tiles[s];
        fa.slab_off[s] = g.slab_off[s];
        fa.count[s] = (double)(h - win_size + 1) * (double)(w - win_size + 1);
        if (s + 1 < levels) {
            const int hp = g.H[s + 1], wp = g.W[s + 1];
            const int64_t n = (int64_t)g.P * hp * wp;
            const int blocks = (int)(cdiv(n, NT) < 8192 ? cdiv(n, NT) : 8192);
            hipLaunchKernelGGL(pool2x2_kernel, dim3(blocks), dim3(NT), 0, st, a.x, a.xb, a.xc, a.xh, a.y, a.yb, a.yc, a.yh, C, h, w, hp,
                               wp, n, const_cast<float*>(sv[s + 1].x), const_cast<float*>(sv[s + 1].y));
            HIPCHK(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(msssim_final_kernel, dim3(B), dim3(NT), 0, st, slab, fa, B, out, out_scales);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

extern "C" const char* pc_metrics_strerror(int code)
{
    switch (code) {
    case PC_OK: return "ok";
    case PC_ERR_ARG: return "invalid argument or unsupported shape";
    case PC_ERR_BUFFER: return "workspace too small (pc_msssim_workspace_size)";
    case PC_ERR_HIP: return "HIP runtime error";
    default: return "unknown error";
    }
}

extern "C" int pc_metrics_last_hip_error(void) { return g_last_hip.load(); }

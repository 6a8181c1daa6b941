// pc_rate.hip -- the per-tile, per-channel weighted squared error of decoded tiles against the original 8-bit image on gfx950
// (pc_rate.h).  Definition: DESIGN.md section 12.
//
// The decomposition is pc_tiles.hip's: a work item is four consecutive columns of one tile row, all three channels (three runs of
// four floats, 12 bytes of the original); a thread takes ITEMS items NT apart, a block ITEMS * NT consecutive items of ONE tile
// (T * T / 4 is a multiple of 1024 for every T that is a multiple of 64, so no block straddles two tiles and none has a tail).  The
// groups are aligned to multiples of 4 in tile columns and, the stride S = T - O being a multiple of 4, in image columns.  The access
// path (WIDE: a 128-bit word of floats, a 32-bit word of bytes; else float by float and byte by byte) only changes the load
// instructions.  Everything that is added is an integer: a thread's sums, the wave tree, the waves of a block, then final_kernel over
// a tile's block partials.  No floats are accumulated, no atomics.
#include "pc_image_host.h"
#include "pc_reduce.h"
#include "pc_tile_grid.h"

#include "pc_rate.h"

namespace {

constexpr int ITEMS = 4;                 // work items per thread
constexpr int BLOCK_ITEMS = NT * ITEMS;
constexpr int T_MAX = 2048;              // T^4 * 65025 < 2^60: the sums fit 63 bits

struct U8 {                              // a u8 view (pc_rate.h), strides in bytes
    const uint8_t* p;
    int layout;
    int64_t sp, sr;
};

// The bytes of pixels x0 .. x0 + n - 1 of row y: v[c][i]; the other lanes read as 0 and are not addressed.
template <bool WIDE>
__device__ __forceinline__ void load_px(const U8& s, int64_t y, int64_t x0, int n, unsigned v[3][4])
{
    if (s.layout == PC_RATE_HWC) {
        const uint8_t* q = s.p + y * s.sr + 3 * x0;
        if (WIDE && n == 4) {
            const uint32_t* w = reinterpret_cast<const uint32_t*>(q);
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
            v[0][0] = w0 & 255u; v[1][0] = (w0 >> 8) & 255u; v[2][0] = (w0 >> 16) & 255u;
            v[0][1] = w0 >> 24;  v[1][1] = w1 & 255u;        v[2][1] = (w1 >> 8) & 255u;
            v[0][2] = (w1 >> 16) & 255u; v[1][2] = w1 >> 24; v[2][2] = w2 & 255u;
            v[0][3] = (w2 >> 8) & 255u;  v[1][3] = (w2 >> 16) & 255u; v[2][3] = w2 >> 24;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][i] = i < n ? q[3 * i + c] : 0u;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint8_t* q = s.p + c * s.sp + y * s.sr + x0;
            if (WIDE && n == 4) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(q);
                v[c][0] = w & 255u; v[c][1] = (w >> 8) & 255u; v[c][2] = (w >> 16) & 255u; v[c][3] = w >> 24;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[c][i] = i < n ? q[i] : 0u;
            }
        }
    }
}

// Block b of tile t is block t * bpt + b: the items b * BLOCK_ITEMS .. of the tile, item -> (row r, group g), tile columns 4g .. 4g+3.
// partials[(t * bpt + b) * 3 + c].
template <bool WIDE>
__global__ __launch_bounds__(NT) void sse_kernel(F32 x, U8 ref, int H, int W, int S, int O, int ny, int nx, int first_tile, int trunc,
                                                 int G4, int bpt, u64* __restrict__ partials)
{
    const int t = (int)(blockIdx.x / (unsigned)bpt), b = (int)(blockIdx.x - (unsigned)t * (unsigned)bpt);
    const int tg = first_tile + t, i = tg / nx, j = tg - i * nx;
    const int den = O > 0 ? 2 * O : 1;
    const int64_t Yt = (int64_t)i * S, Xt = (int64_t)j * S;          // the tile's first row and column in the image
    u64 su[3] = {0ull, 0ull, 0ull};
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int rem = b * BLOCK_ITEMS + k * NT + (int)threadIdx.x; // < T * G4 <= 2^20
        const int r = rem / G4, q0 = 4 * (rem - r * G4);
        const int64_t Y = Yt + r, X0 = Xt + q0;
        if (Y < H && X0 < W) {
            const int n = (int)(W - X0 < 4 ? W - X0 : 4);            // n < 4: the group straddles the image's right edge
            unsigned rv[3][4];
            load_px<WIDE>(ref, Y, X0, n, rv);
            unsigned ax[4];
#pragma unroll
            for (int l = 0; l < 4; ++l) ax[l] = l < n ? axis_weight(j, nx, q0 + l, S, O, den) : 0u;
            const u64 ay = axis_weight(i, ny, r, S, O, den);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                // q0 + 3 < T <= sxh: the four floats lie inside the tile's row whatever the image's edge
                const float* s = x.p + (int64_t)t * x.st + ch * x.sc + (int64_t)r * x.sh + q0;
                float v[4];
                if (WIDE) {
                    const float4 f = *reinterpret_cast<const float4*>(s);
                    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
                } else {
#pragma unroll
                    for (int l = 0; l < 4; ++l) v[l] = s[l];
                }
                unsigned row = 0u;                                   // <= 4 * 2048 * 65025 < 2^30
#pragma unroll
                for (int l = 0; l < 4; ++l) {
                    const float s255 = fminf(fmaxf(v[l], 0.f), 1.f) * 255.0f;
                    const int e = (int)(trunc ? truncf(s255) : rintf(s255)) - (int)rv[ch][l];
                    row += ax[l] * (unsigned)(e * e);                // ax = 0 on the lanes beyond the image
                }
                su[ch] += ay * (u64)row;
            }
        }
    }
    block_reduce<Sum>(su, partials + (int64_t)blockIdx.x * 3);
}

// One wave per tile: its bpt block partials, lane l taking l, l + 64, ..., then the wave tree.
__global__ __launch_bounds__(64) void final_kernel(const u64* __restrict__ p, int bpt, u64* __restrict__ out)
{
    row_final<Sum, 3>(p, bpt, out);
}

bool layout_ok(int layout) { return layout == PC_RATE_HWC || layout == PC_RATE_CHW; }

// Blocks per tile and in all; false for what the call refuses.
bool blocks_of(int T, int n_tiles, int& bpt, int64_t& blocks)
{
    if (T < 64 || T % 64 || T > T_MAX || n_tiles < 1) return false;
    bpt = (int)((int64_t)T * (T / 4) / BLOCK_ITEMS);
    blocks = (int64_t)n_tiles * bpt;
    return blocks <= INT32_MAX;
}

// The one place that decides the access path: the call launches from it, pc_rate_plan reports it.
bool wide_path(const void* x, int64_t st, int64_t sc, int64_t sh, const void* ref, int layout, int64_t rp, int64_t rr)
{
    return f32_wide(x, st, sc, sh) && aligned(ref, 4) && mult4(rr) && (layout == PC_RATE_HWC || mult4(rp));
}

}  // namespace

extern "C" size_t pc_rate_workspace_size(int T, int n_tiles)
{
    int bpt;
    int64_t blocks;
    return blocks_of(T, n_tiles, bpt, blocks) ? (size_t)blocks * 3 * sizeof(u64) : 0;
}

extern "C" int pc_rate_plan(const void* x, int64_t sxt, int64_t sxc, int64_t sxh, const void* ref, int ref_layout, int64_t r_plane,
                            int64_t r_row, int* wide)
{
    if (!x || !ref || !wide || !layout_ok(ref_layout)) return PC_ERR_ARG;
    *wide = wide_path(x, sxt, sxc, sxh, ref, ref_layout, r_plane, r_row) ? 1 : 0;
    return PC_OK;
}

extern "C" int pc_rate_tile_sse_u8(const float* x, int64_t sxt, int64_t sxc, int64_t sxh, int H, int W, int T, int O, int first_tile,
                                   int n_tiles, int rounding, const uint8_t* ref, int ref_layout, int64_t r_plane, int64_t r_row,
                                   void* workspace, size_t workspace_bytes, uint64_t* out, void* stream)
{
    Geo g;
    int bpt;
    int64_t blocks;
    if (!geo_of(H, W, T, O, T_MAX, g) || !blocks_of(T, n_tiles, bpt, blocks)) return PC_ERR_ARG;
    if (first_tile < 0 || (int64_t)first_tile + n_tiles > (int64_t)g.ny * g.nx) return PC_ERR_ARG;
    if (!x || !aligned(x, 4) || sxh < T || sxc < 1 || sxt < 1) return PC_ERR_ARG;
    if (rounding != PC_RATE_NEAREST && rounding != PC_RATE_TRUNC) return PC_ERR_ARG;
    if (!ref || !layout_ok(ref_layout)) return PC_ERR_ARG;
    const bool chw = ref_layout == PC_RATE_CHW;
    if (r_row < (chw ? (int64_t)W : 3 * (int64_t)W) || (chw && r_plane < 1)) return PC_ERR_ARG;
    if (!workspace || !aligned(workspace, 8) || !out || !aligned(out, 8)) return PC_ERR_ARG;
    if (workspace_bytes < (size_t)blocks * 3 * sizeof(u64)) return PC_ERR_ARG;
    const bool wide = wide_path(x, sxt, sxc, sxh, ref, ref_layout, r_plane, r_row);
    const F32 xv{x, sxt, sxc, sxh};
    const U8 rv{ref, ref_layout, r_plane, r_row};
    const int trunc = rounding == PC_RATE_TRUNC;
    u64* part = static_cast<u64*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks), block(NT);
    if (wide)
        hipLaunchKernelGGL(sse_kernel<true>, grid, block, 0, st, xv, rv, H, W, g.S, O, g.ny, g.nx, first_tile, trunc, T / 4, bpt, part);
    else
        hipLaunchKernelGGL(sse_kernel<false>, grid, block, 0, st, xv, rv, H, W, g.S, O, g.ny, g.nx, first_tile, trunc, T / 4, bpt, part);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(final_kernel, dim3((unsigned)n_tiles), dim3(64), 0, st, part, bpt, reinterpret_cast<u64*>(out));
    HIPCHK(hipGetLastError());
    return PC_OK;
}

extern "C" const char* pc_rate_strerror(int code)
{
    switch (code) {
    case PC_OK: return "ok";
    case PC_ERR_ARG: return "invalid argument, geometry outside pc_rate.h, tile range outside the grid or workspace too small";
    case PC_ERR_HIP: return "HIP runtime error";
    default: return "unknown error";
    }
}

extern "C" int pc_rate_last_hip_error(void) { return g_last_hip.load(); }

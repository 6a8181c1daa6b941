// pc_tile_grid.h -- the tile geometry of the tiled image-side libraries (pc_tiles.h states it): tile size T,
// overlap O, stride S = T - O, the ny x nx grid of an H x W picture, a float tile set, and the integer band weights of section 12.
// The largest T differs per library and format and is a parameter.  Include after pc_image_host.h.
#ifndef PC_TILE_GRID_H
#define PC_TILE_GRID_H

#include <climits>

namespace {

// a float tile set, or the float planes of a batch of pictures; st: from one tile (picture) to the next; strides in elements
struct F32 {
    const float* p;
    int64_t st, sc, sh;
};

struct Grid {                            // the picture and its grid, as the kernels take them
    int H, W, T, S, O, ny, nx;
};

int64_t axis_tiles(int L, int T, int S) { return L <= T ? 1 : cdiv((int64_t)L - T, S) + 1; }

struct Geo {
    int S, ny, nx;
};

// The geometry every call shares: T a multiple of 64 and at most t_max (INT_MAX: no limit), O a multiple of 4 in [0, T/2], and the
// grid of an H x W picture within 32 bits.
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

// a rectangle of nty x ntx tiles at (ty0, tx0) inside the grid
bool rect_ok(const Geo& g, int ty0, int tx0, int nty, int ntx)
{
    return ty0 >= 0 && tx0 >= 0 && nty >= 1 && ntx >= 1 && (int64_t)ty0 + nty <= g.ny && (int64_t)tx0 + ntx <= g.nx;
}

// The first and the last tile along an axis of n tiles that cover pixel p.
int last_tile(int p, int S, int n) { return p / S < n - 1 ? p / S : n - 1; }
int first_tile(int p, int S, int O, int n)
{
    const int i = last_tile(p, S, n);
    return i > 0 && p - i * S < O ? i - 1 : i;
}

// The numerator over den of the weight tile i of n gives local coordinate u along an axis (pc_rate.h).
__device__ __forceinline__ unsigned axis_weight(int i, int n, int u, int S, int O, int den)
{
    if (i > 0 && u < O) return (unsigned)(2 * u + 1);
    if (i < n - 1 && u >= S) return (unsigned)(2 * (O - 1 - (u - S)) + 1);
    return (unsigned)den;
}

}  // namespace

#endif  // PC_TILE_GRID_H

/* pc_rate.h -- C ABI of libpc_rate.so: the per-tile distortion behind rate-controlled tiled coding (pc_rate_tile_sse_u8), on gfx950.
 * DESIGN.md section 12.
 *
 * Kept apart from libpc_tiles.so, as that is from libpc_pixels.so and libpcodec.so: nothing here is part of the codec's numeric
 * contract, byte strings or profiles, and no library of the image domain links another.  Plain C, the conventions of
 * pc_tiles.h: device pointers, int64 strides, status codes PC_OK / PC_ERR_* (pcodec.h), `stream` is a hipStream_t passed as void*
 * (NULL = default stream).  No call allocates device memory or synchronises the host.  Every argument is checked before the first
 * HIP call; a call that returns PC_ERR_ARG has launched nothing.  All offsets are 64-bit.
 *
 * Geometry, u8 views and float32 tile sets are those of pc_tiles.h: tile size T (a multiple of 64), overlap O (a multiple of 4,
 * 0 <= O <= T/2), stride S = T - O, 1 tile along an axis of length L <= T and ceil((L - T) / S) + 1 otherwise, tiles numbered
 * row-major over the ny x nx grid.  Here T <= 2048.  A u8 view is a pointer, a layout and two strides in BYTES:
 *   PC_RATE_HWC  [h,w,3] interleaved: byte (y, x, c) at p[y*s_row + 3*x + c]; s_plane is ignored.
 *   PC_RATE_CHW  [3,h,w] planar:      byte (c, y, x) at p[c*s_plane + y*s_row + x].
 * A float32 tile set is a pointer and tile, channel and row strides in ELEMENTS, unit stride along a row.
 */
#ifndef PC_RATE_H
#define PC_RATE_H

#include "pcodec.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PC_RATE_HWC = 0, PC_RATE_CHW = 1 };
enum { PC_RATE_NEAREST = 0, PC_RATE_TRUNC = 1 };

/* Bytes of device workspace pc_rate_tile_sse_u8 needs for n_tiles tiles of size T: 24 bytes (three 64-bit sums) per block of 1024
 * four-column groups, T*T/4096 blocks per tile.  0 for arguments the call would refuse (T < 64, no multiple of 64 or > 2048,
 * n_tiles < 1, more than 2^31 - 1 blocks). */
PC_API size_t pc_rate_workspace_size(int T, int n_tiles);

/* out[t][c] = sum over the pixels (r, q) of tile first_tile + t that lie inside the H x W image of  ay(r) * ax(q) * e^2,  all in
 * unsigned 64-bit integers (exact; the order of the additions is free), where for tile (i, j) = ((first_tile + t) / nx,
 * (first_tile + t) % nx), Y = i*S + r, X = j*S + q:
 *   e      = Q(x[t, c, r, q]) - ref(c, Y, X),  Q(v) = NaN -> 0, clamp to [0, 1], * 255.0f, then rintf (PC_RATE_NEAREST, half to even)
 *            or truncf (PC_RATE_TRUNC): the quantiser of pc_tiles_stitch_u8 applied to the tile ALONE.
 *   ay, ax = the numerators of the stitch's band weights over den = 2*O (den = 1 for O = 0): for tile index i of n along the axis
 *            and local coordinate u,  2u + 1 if i > 0 and u < O;  2 (O - 1 - (u - S)) + 1 if i < n - 1 and u >= S;  den otherwise.
 *            For every image pixel, ay * ax summed over its covering tiles is den^2 exactly.
 * The sum is at most T^4 * 65025 < 2^60 for T <= 2048; a larger T is refused.
 *   x             float32 tile set of n_tiles tiles: element (t, c, r, q) at x[t*sxt + c*sxc + r*sxh + q]; sxh >= T; 4-byte aligned.
 *   first_tile, n_tiles   a LINEAR range of the row-major grid of pc_tiles_grid(H, W, T, O), inside it.
 *   ref           u8 view of the whole H x W original image.
 *   workspace     at least pc_rate_workspace_size(T, n_tiles) bytes, 8-byte aligned; PC_ERR_ARG if smaller.
 *   out           [n_tiles][3] uint64, 8-byte aligned; every element is written (no memset needed).
 * The result for a tile depends on that tile and the image only: not on first_tile, n_tiles, the stream or the access path.  No
 * float is accumulated anywhere and there are no atomics.  Two launches: the per-block sums, then one ordered reduction per tile. */
PC_API int pc_rate_tile_sse_u8(const float* x, int64_t sxt, int64_t sxc, int64_t sxh, int H, int W, int T, int O, int first_tile,
                               int n_tiles, int rounding, const uint8_t* ref, int ref_layout, int64_t r_plane, int64_t r_row,
                               void* workspace, size_t workspace_bytes, uint64_t* out, void* stream);

/* Host only, launches nothing: *wide = 1 where pc_rate_tile_sse_u8 with exactly these pointers and strides moves four pixels per
 * access (a 128-bit word of floats; a 32-bit word of a planar ref, three for an interleaved one), 0 where it moves them float by
 * float and byte by byte.  Both give the same integers.  A work item is four consecutive columns of one tile row, aligned to a
 * multiple of 4 in tile columns and, S being a multiple of 4, in image columns.  The wide path needs: x 16-byte aligned and sxt, sxc,
 * sxh multiples of 4; ref 4-byte aligned, r_row a multiple of 4 and, planar, r_plane a multiple of 4.  The call decides with the same
 * code.  PC_ERR_ARG for NULL pointers or an unknown layout. */
PC_API int pc_rate_plan(const void* x, int64_t sxt, int64_t sxc, int64_t sxh, const void* ref, int ref_layout, int64_t r_plane,
                        int64_t r_row, int* wide);

PC_API const char* pc_rate_strerror(int code);
PC_API int pc_rate_last_hip_error(void);

#ifdef __cplusplus
}
#endif

#endif /* PC_RATE_H */

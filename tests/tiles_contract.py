"""Tiled image coding (progressivecodec_amd/tiles.py, tiles_csrc/pc_tiles.h) restated in numpy from its definition (DESIGN.md section
11), not from the kernels: what tests/test_tiles_host.py checks on its own and tests/test_gpu_tiles.py checks the GPU against.

An image is a uint8 array [H,W,3] ("hwc") or [3,H,W] ("chw"); tiles are float32 [n,3,T,T], row-major over a grid rectangle
(ty0, tx0, nty, ntx).  `unit`, `clamp01`, `quantise` and the layout helpers are those of tests/pixels_contract.py.
"""
import math

import numpy as np

from tests import pixels_contract as K


def check(T, O):
    if T < 64 or T % 64 or O < 0 or O % 4 or 2 * O > T:
        raise ValueError((T, O))


def axis_tiles(L, T, O):
    """1 tile if L <= T, otherwise ceil((L - T) / S) + 1"""
    check(T, O)
    if L < 1:
        raise ValueError(L)
    S = T - O
    return 1 if L <= T else -(-(L - T) // S) + 1


def grid(H, W, T, O):
    return axis_tiles(H, T, O), axis_tiles(W, T, O)


def covering(p, L, T, O):
    """the tiles of an axis of length L whose span [i*S, i*S + T) holds pixel p, ascending"""
    S = T - O
    return [i for i in range(axis_tiles(L, T, O)) if i * S <= p < i * S + T]


def chw_of(img, layout):
    return K.to_chw(np.asarray(img)[None], layout)[0]


def cut(img, layout, T, O, rect=None):
    """float32 [nty*ntx,3,T,T]: tile (i, j) is unit(img) over [i*S, i*S + T) x [j*S, j*S + T), +0.0 beyond the image"""
    x = K.unit(chw_of(img, layout))
    _, H, W = x.shape
    ny, nx = grid(H, W, T, O)
    ty0, tx0, nty, ntx = (0, 0, ny, nx) if rect is None else rect
    S = T - O
    out = np.zeros((nty * ntx, 3, T, T), np.float32)
    for a in range(nty):
        for b in range(ntx):
            y, x0 = (ty0 + a) * S, (tx0 + b) * S
            part = x[:, y:y + T, x0:x0 + T]
            out[a * ntx + b, :, :part.shape[1], :part.shape[2]] = part
    return out


def weight(i, u, n, T, O):
    """float32 weight of tile i of n along an axis at local coordinate u (0 <= u < T)"""
    S = T - O
    if i > 0 and u < O:
        return np.float32(2 * u + 1) / np.float32(2 * O)
    if i < n - 1 and u >= S:
        return np.float32(2 * (O - 1 - (u - S)) + 1) / np.float32(2 * O)
    return np.float32(1.0)


def weights(i, n, T, O):
    """float32 [T]: weight(i, u) for every u"""
    return np.array([weight(i, u, n, T, O) for u in range(T)], np.float32)


def fmaf(a, b, c):
    """the float32 fused multiply-add of non-negative finite float32 arrays, exactly: the product is exact in float64, the sum is
    rounded to odd in float64 (53 >= 2 * 24 + 2 bits), and rounding that to float32 rounds the exact a * b + c once"""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                                    # TwoSum: p + c = s + err exactly
    even = (s.view(np.int64) & 1) == 0
    other = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    s = np.where((err != 0) & even, other, s)
    return s.astype(np.float32)


def product(wy, wx):
    """float32 [h,w]: a pixel's weight for a tile, the one rounded float32 product wy * wx of its two axis weights"""
    return (wy[:, None] * wx[None, :]).astype(np.float32)


def blend(tiles, H, W, T, O, rect=None, window=None):
    """float32 [3,h,w]: m = fmaf(w_t, clamp01(x_t), acc) chained from +0.0 over the covering tiles in ascending tile index"""
    ny, nx = grid(H, W, T, O)
    ty0, tx0, nty, ntx = (0, 0, ny, nx) if rect is None else rect
    y0, x0, h, w = (0, 0, H, W) if window is None else window
    if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > H or x0 + w > W:
        raise ValueError(window)
    S = T - O
    acc = np.zeros((3, H, W), np.float32)
    need = set()
    for i in range(ny):
        ys = slice(i * S, min(i * S + T, H))
        if ys.start >= y0 + h or ys.stop <= y0:
            continue
        wy = weights(i, ny, T, O)[:ys.stop - ys.start]
        for j in range(nx):
            xs = slice(j * S, min(j * S + T, W))
            if xs.start >= x0 + w or xs.stop <= x0:
                continue
            need.add((i, j))
            if not (ty0 <= i < ty0 + nty and tx0 <= j < tx0 + ntx):
                raise ValueError(f"tile {(i, j)} covers the window and is not in the rectangle")
            wx = weights(j, nx, T, O)[:xs.stop - xs.start]
            wt = product(wy, wx)
            c = K.clamp01(tiles[(i - ty0) * ntx + (j - tx0), :, :ys.stop - ys.start, :xs.stop - xs.start])
            acc[:, ys, xs] = fmaf(wt[None], c, acc[:, ys, xs])
    return acc[:, y0:y0 + h, x0:x0 + w]


def stitch(tiles, H, W, T, O, rounding, layout, rect=None, window=None):
    """uint8 window of the image in `layout`"""
    m = blend(tiles, H, W, T, O, rect, window)
    return K.from_chw(K.quantise(m, rounding)[None], layout)[0]


def sums(tiles, H, W, T, O, rounding, ref, ref_layout, rect=None, window=None):
    """(sse_u8 [3] of Python ints, sse_f [3] of floats) over the window, defined as pixels_contract.sums with m in place of c"""
    y0, x0, h, w = (0, 0, H, W) if window is None else window
    m = blend(tiles, H, W, T, O, rect, window)
    q = K.quantise(m, rounding).astype(np.int64)
    r = chw_of(ref, ref_layout)[:, y0:y0 + h, x0:x0 + w]
    e = q - r.astype(np.int64)
    d = (K.unit(r) - m).astype(np.float32).astype(np.float64)
    return ([int((e[ch] * e[ch]).sum()) for ch in range(3)], [math.fsum((d[ch] * d[ch]).ravel().tolist()) for ch in range(3)])


def hostile_tiles(n, T, seed):
    """float32 [n,3,T,T]: random values over [-0.5, 1.5] with NaN, +-inf, -0.0, denormals and exact .5 ties after x 255 sprinkled in"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.5, 1.5, (n, 3, T, T)).astype(np.float32)
    flat = x.reshape(-1)
    special = np.concatenate([np.array([-0.0, 0.0, 1.0, -1.5, 2.5, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 0.5, 1 - 2.0 ** -24],
                                       np.float32), K.exact_ties()])
    k = max(len(special), flat.size // 7)
    idx = rng.choice(flat.size, k, replace=False)
    flat[idx] = special[np.arange(k) % len(special)]
    return x

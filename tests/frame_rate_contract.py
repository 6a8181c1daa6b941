"""Rate-controlled tiled coding of YUV 4:2:0 frames (progressivecodec_amd/frame_rate.py, frame_rate_csrc/pc_frame_rate.h) restated in
numpy from its definition, not from the kernel or the module: what tests/test_frame_rate_host.py checks on its
own and tests/test_gpu_frame_rate.py checks the GPU against.  Not a test file.  It is the composition of three restatements:
tests/frames_contract.py (section 13: `emit_codes`, `codes`) per tile, tests/tiles_contract.py (section 11: `grid`) and
tests/rate_contract.py (section 12: `weight_int`, `den_of`, `allocate`).

A frame is frames_contract's, with its leading batch axis of 1; tiles are float32 [n,3,T,T], a linear range of the row-major grid.
"""
import numpy as np

from tests import frames_contract as FC
from tests import rate_contract as RC
from tests import tiles_contract as TC


def max_tile(fmt):
    """T^4 (2^n - 1)^2 < 2^60"""
    T = 1024 if fmt == "p010" else 2048
    assert T ** 4 * (2 ** FC.bits(fmt) - 1) ** 2 < 2 ** 60
    return T


def chroma_weights(i, n, T, O):
    """Python ints [T/2]: cy(k) = (ay(2k) + ay(2k+1)) / 2, which must divide evenly"""
    a = [RC.weight_int(i, u, n, T, O) for u in range(T)]
    out = []
    for k in range(T // 2):
        s = a[2 * k] + a[2 * k + 1]
        if s % 2:
            raise ValueError(f"cy({k}) of tile {i} of {n} is not an integer: {a[2 * k]} + {a[2 * k + 1]}")
        out.append(s // 2)
    return out


def chroma_weight_closed(i, k, n, T, O):
    """the same as the band weight at the cell's centre, in closed form"""
    S = T - O
    if i > 0 and 2 * k < O:
        return 4 * k + 2
    if i < n - 1 and 2 * k >= S:
        return 2 * (O - 1 - (2 * k - S))
    return RC.den_of(O)


def tile_codes(tile, hh, ww, fmt, matrix, rng):
    """(Y [hh,ww], Cb, Cr [ceil(hh/2), ceil(ww/2)]) int64: section 13's emit on the tile with its in-frame part as the picture"""
    Y, Cb, Cr = FC.emit_codes(tile[None], 0, 0, hh, ww, fmt, matrix, rng)
    return Y[0], Cb[0], Cr[0]


def tile_sse(tiles, H, W, T, O, fmt, matrix, rng, ref, first_tile=0):
    """tiles: float32 [n,3,T,T], the tiles first_tile .. first_tile + n - 1 of the row-major grid; ref: the whole original frame ->
    [n][3] Python ints, [Y, Cb, Cr]: the weighted sums of squared code errors.  int64 products (< 2^42 each), the sums in Python
    integers."""
    if T > max_tile(fmt):
        raise ValueError((T, fmt))
    ny, nx = TC.grid(H, W, T, O)
    S = T - O
    n = tiles.shape[0]
    if first_tile < 0 or first_tile + n > ny * nx:
        raise ValueError((first_tile, n, ny, nx))
    rY, rCb, rCr = (p[0] for p in FC.codes(ref, fmt))
    out = []
    for t in range(n):
        i, j = divmod(first_tile + t, nx)
        hh, ww = min(T, H - i * S), min(T, W - j * S)
        hc, wc = FC.chroma_size(hh, ww)
        Y, Cb, Cr = tile_codes(tiles[t], hh, ww, fmt, matrix, rng)
        ay, ax = RC.weights_int(i, ny, T, O)[:hh], RC.weights_int(j, nx, T, O)[:ww]
        cy, cx = np.array(chroma_weights(i, ny, T, O)[:hc], np.int64), np.array(chroma_weights(j, nx, T, O)[:wc], np.int64)
        eY = Y - rY[i * S:i * S + hh, j * S:j * S + ww]
        ci, cj = i * S // 2, j * S // 2
        eB, eR = Cb - rCb[ci:ci + hc, cj:cj + wc], Cr - rCr[ci:ci + hc, cj:cj + wc]
        assert eY.shape == (hh, ww) and eB.shape == eR.shape == (hc, wc)
        wl, wch = ay[:, None] * ax[None, :], cy[:, None] * cx[None, :]
        out.append([sum(int(v) for v in (w * e * e).ravel()) for w, e in ((wl, eY), (wch, eB), (wch, eR))])
    return out


def coverage(L, T, O, chroma):
    """Python ints, one per luma (chroma) sample of an axis of length L: the sum over the covering tiles of ay (cy)"""
    n = TC.axis_tiles(L, T, O)
    S = T - O
    Lc = -(-L // 2)
    tot = [0] * (Lc if chroma else L)
    for i in range(n):
        ll = min(T, L - i * S)
        if chroma:
            for k, w in enumerate(chroma_weights(i, n, T, O)[:-(-ll // 2)]):
                tot[i * S // 2 + k] += w
        else:
            for u in range(ll):
                tot[i * S + u] += RC.weight_int(i, u, n, T, O)
    return tot

"""Rate-controlled tiled coding of YUV frames of any subsampling and siting (progressivecodec_amd/chroma_rate.py,
chroma_rate_hip/pc_chroma_rate.h) restated in numpy from its definition, not from the kernel or the module: what
tests/test_chroma_rate_host.py checks on its own and tests/test_gpu_chroma_rate.py checks the GPU against.  Not a test file.  It is the
composition of three restatements and restates none: tests/chroma_contract.py (section 21: `emit_codes`, `codes`) per tile,
tests/tiles_contract.py (section 11: `grid`) and tests/rate_contract.py (section 12: `weights_int`, `den_of`, `allocate`).

A frame is chroma_contract's, with its leading batch axis of 1; tiles are float32 [n,3,T,T], a linear range of the row-major grid.
"""
import numpy as np

from tests import chroma_contract as CC
from tests import rate_contract as RC
from tests import tiles_contract as TC


def max_tile(fmt):
    """T^4 (2^n - 1)^2 < 2^60"""
    T = 1024 if CC.bits(fmt) == 10 else 2048
    assert T ** 4 * (2 ** CC.bits(fmt) - 1) ** 2 < 2 ** 60 <= (2 * T) ** 4 * (2 ** CC.bits(fmt) - 1) ** 2
    return T


def chroma_weights(i, n, T, O, s):
    """int64 [T / s]: the weight of chroma index k of tile i of n along an axis with s luma samples per chroma sample:
    (a(2k) + a(2k+1)) / 2 at s == 2, which must divide evenly, a(k) at s == 1"""
    a = RC.weights_int(i, n, T, O)
    if s == 1:
        return a
    pair = a[0::2] + a[1::2]
    if (pair % 2).any():
        raise ValueError(f"the chroma weights of tile {i} of {n} are not integers: T {T}, O {O}")
    return pair // 2


def tile_codes(tile, hh, ww, fmt, matrix, rng, siting):
    """(Y [hh,ww], Cb, Cr [ceil(hh/sy), ceil(ww/sx)]) int64: section 21's emit on the tile with its in-frame part as the picture, so
    that every clamp of the chroma filter is at that part's edges"""
    Y, Cb, Cr = CC.emit_codes(tile[None], 0, 0, hh, ww, fmt, matrix, rng, siting)
    return Y[0], Cb[0], Cr[0]


def tile_parts(tiles, H, W, T, O, fmt, matrix, rng, siting, first_tile=0):
    """per tile: (i, j, the tile's codes, its luma weights [hh,ww], its chroma weights [hc,wc])"""
    if T > max_tile(fmt):
        raise ValueError((T, fmt))
    ny, nx = TC.grid(H, W, T, O)
    S = T - O
    sx, sy = CC.sub(fmt)
    n = tiles.shape[0]
    if first_tile < 0 or first_tile + n > ny * nx:
        raise ValueError((first_tile, n, ny, nx))
    out = []
    for t in range(n):
        i, j = divmod(first_tile + t, nx)
        hh, ww = min(T, H - i * S), min(T, W - j * S)
        hc, wc = CC.chroma_size(hh, ww, fmt)
        codes = tile_codes(tiles[t], hh, ww, fmt, matrix, rng, siting)
        ay, ax = RC.weights_int(i, ny, T, O)[:hh], RC.weights_int(j, nx, T, O)[:ww]
        cy, cx = chroma_weights(i, ny, T, O, sy)[:hc], chroma_weights(j, nx, T, O, sx)[:wc]
        out.append((i, j, codes, ay[:, None] * ax[None, :], cy[:, None] * cx[None, :]))
    return out


def tile_sse(tiles, H, W, T, O, fmt, matrix, rng, siting, ref, first_tile=0):
    """tiles: float32 [n,3,T,T], the tiles first_tile .. first_tile + n - 1 of the row-major grid; ref: the whole original frame ->
    [n][3] Python ints, [Y, Cb, Cr]: the weighted sums of squared code errors.  int64 products (< 2^42 each), the sums in Python
    integers."""
    S = T - O
    sx, sy = CC.sub(fmt)
    rY, rCb, rCr = (p[0] for p in CC.codes(ref, fmt))
    out = []
    for i, j, (Y, Cb, Cr), wl, wch in tile_parts(tiles, H, W, T, O, fmt, matrix, rng, siting, first_tile):
        hh, ww = Y.shape
        hc, wc = Cb.shape
        eY = Y - rY[i * S:i * S + hh, j * S:j * S + ww]
        ci, cj = i * S // sy, j * S // sx
        eB, eR = Cb - rCb[ci:ci + hc, cj:cj + wc], Cr - rCr[ci:ci + hc, cj:cj + wc]
        assert eY.shape == wl.shape == (hh, ww) and eB.shape == eR.shape == wch.shape == (hc, wc)
        out.append([sum(int(v) for v in (w * e * e).ravel()) for w, e in ((wl, eY), (wch, eB), (wch, eR))])
    return out


def coverage(L, T, O, s):
    """Python ints, one per sample of an axis of L luma samples with s luma samples per sample (1: luma, or chroma on an axis that is
    not subsampled): the sum over the covering tiles of the weights"""
    n = TC.axis_tiles(L, T, O)
    S = T - O
    tot = [0] * -(-L // s)
    for i in range(n):
        ll = min(T, L - i * S)
        for k, w in enumerate(chroma_weights(i, n, T, O, s)[:-(-ll // s)]):
            tot[i * S // s + k] += int(w)
    return tot


def sse_exact(H, W, T, O, fmt, siting):
    """where the sums over the tiles are the decoded frame's: no overlap, and no subsampled, co-sited axis with more than one tile"""
    ny, nx = TC.grid(H, W, T, O)
    sx, sy = CC.sub(fmt)
    hco, vco = CC.SITINGS[siting]
    return O == 0 and not (sx == 2 and hco and nx > 1) and not (sy == 2 and vco and ny > 1)

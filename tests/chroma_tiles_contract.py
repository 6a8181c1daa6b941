"""Tiled coding of YUV frames of any subsampling and siting (progressivecodec_amd/chroma_tiles.py, chroma_tiles_hip/pc_chroma_tiles.h)
restated in numpy from its definition, not from the kernels: what tests/test_chroma_tiles_host.py checks on
its own and tests/test_gpu_chroma_tiles.py checks the GPU against.  It is the composition of two restatements and restates neither:
tests/chroma_contract.py (section 21: `rgb`, `emit_codes`, `codes`) per pixel and tests/tiles_contract.py (section 11: `grid`,
`blend`) per tile.

A frame is chroma_contract's, with its leading batch axis of 1; tiles are float32 [n,3,T,T], row-major over a grid rectangle
(ty0, tx0, nty, ntx); a window is (y0, x0, h, w).

The one thing that is this section's own is the halo: the emit is section 21's WITH THE FRAME AS THE PICTURE, restricted to the
window, so the co-sited filter of the window's first chroma column (row) reads frame column x0 - 1 (row y0 - 1).  `stitch_codes`
blends the window extended by that halo -- tiles_contract.blend raises if a tile that covers it is missing from the rectangle, which
is the halo rule -- and hands chroma_contract.emit_codes a picture in which the halo column stands where the frame has it: one
whole chroma sample (sx columns, sy rows) left of / above the window, of which only the luma sample next to the window is ever read
by a sample that is kept.
"""
import numpy as np

from tests import chroma_contract as CC
from tests import tiles_contract as TC


def admissible(H, W, fmt, window):
    """y0 % sy == 0, x0 % sx == 0, h % sy == 0 or the window ends on the frame's last row, w % sx == 0 or on its last column"""
    y0, x0, h, w = window
    sx, sy = CC.sub(fmt)
    return y0 % sy == 0 and x0 % sx == 0 and (h % sy == 0 or y0 + h == H) and (w % sx == 0 or x0 + w == W)


def halo(fmt, siting, window):
    """(rows above, columns left) of the window that its first chroma samples read: 1 where the axis is subsampled and co-sited and
    the window does not start on the frame's edge"""
    y0, x0, _, _ = window
    sx, sy = CC.sub(fmt)
    hco, vco = CC.SITINGS[siting]
    return (1 if sy == 2 and vco and y0 > 0 else 0, 1 if sx == 2 and hco and x0 > 0 else 0)


def halo_window(fmt, siting, window):
    y0, x0, h, w = window
    dy, dx = halo(fmt, siting, window)
    return (y0 - dy, x0 - dx, h + dy, w + dx)


def cut(planes, fmt, matrix, rng, upsample, siting, T, O, rect=None):
    """float32 [nty*ntx,3,T,T]: tile (i, j) is the crop over [i*S, i*S + T) x [j*S, j*S + T) of the WHOLE frame's ingest (so the chroma
    taps clamp at the frame's edges), +0.0 beyond the frame"""
    x = CC.rgb(planes, fmt, matrix, rng, upsample, siting)[0]
    _, H, W = x.shape
    ny, nx = TC.grid(H, W, T, O)
    ty0, tx0, nty, ntx = (0, 0, ny, nx) if rect is None else rect
    S = T - O
    out = np.zeros((nty * ntx, 3, T, T), np.float32)
    for a in range(nty):
        for b in range(ntx):
            y, x0 = (ty0 + a) * S, (tx0 + b) * S
            part = x[:, y:y + T, x0:x0 + T]
            out[a * ntx + b, :, :part.shape[1], :part.shape[2]] = part
    return out


def stitch_codes(tiles, H, W, T, O, fmt, matrix, rng, siting, rect=None, window=None, check=True, frame_edges=True):
    """(Y, Cb, Cr) int64 with a leading axis of 1: section 11's blend m, then section 21's emit on m with the frame as the picture,
    restricted to the window.  check=False: also for a window that is not admissible (what the rule is there to exclude; the window
    is then the picture).  frame_edges=False: the filter clamps at the WINDOW's edges instead (what section 14 could do and this
    section must not; for the tests that show the difference)."""
    y0, x0, h, w = (0, 0, H, W) if window is None else window
    ok = admissible(H, W, fmt, (y0, x0, h, w))
    if check and not ok:
        raise ValueError(f"window {(y0, x0, h, w)} of a {H}x{W} {fmt} frame is not admissible")
    if not ok or not frame_edges:
        m = TC.blend(tiles, H, W, T, O, rect, (y0, x0, h, w))
        return CC.emit_codes(m[None], 0, 0, h, w, fmt, matrix, rng, siting)
    sx, sy = CC.sub(fmt)
    dy, dx = halo(fmt, siting, (y0, x0, h, w))
    m = TC.blend(tiles, H, W, T, O, rect, (y0 - dy, x0 - dx, h + dy, w + dx))
    py, px = sy * dy, sx * dx                                     # one whole chroma sample in front of the window
    pic = np.zeros((3, h + py, w + px), np.float32)
    pic[:, py - dy:, px - dx:] = m
    Y, Cb, Cr = CC.emit_codes(pic[None], 0, 0, h + py, w + px, fmt, matrix, rng, siting)
    return Y[:, py:, px:], Cb[:, dy:, dx:], Cr[:, dy:, dx:]


def stitch(tiles, H, W, T, O, fmt, matrix, rng, siting, rect=None, window=None):
    """the window's frame in `fmt`"""
    return CC.frame(*stitch_codes(tiles, H, W, T, O, fmt, matrix, rng, siting, rect, window), fmt)


def crop_codes(codes, fmt, window):
    """the window of a whole frame's (Y, Cb, Cr): luma [y0:y0+h, x0:x0+w], chroma [y0/sy : y0/sy + ceil(h/sy), x0/sx : ...]"""
    y0, x0, h, w = window
    sx, sy = CC.sub(fmt)
    hc, wc = CC.chroma_size(h, w, fmt)
    Y, Cb, Cr = codes
    cs = (slice(None), slice(y0 // sy, y0 // sy + hc), slice(x0 // sx, x0 // sx + wc))
    return Y[:, y0:y0 + h, x0:x0 + w], Cb[cs], Cr[cs]


def sums(tiles, H, W, T, O, fmt, matrix, rng, siting, ref, rect=None, window=None):
    """[3] Python ints: per plane [Y, Cb, Cr] the sum over the window of (code - refcode)^2; ref is the whole original frame"""
    win = (0, 0, H, W) if window is None else window
    got = stitch_codes(tiles, H, W, T, O, fmt, matrix, rng, siting, rect, win)
    want = crop_codes(CC.codes(ref, fmt), fmt, win)
    return [int(((g - r) ** 2).sum()) for g, r in zip(got, want)]


def covering(H, W, T, O, window):
    """the smallest rectangle (ty0, tx0, nty, ntx) holding every tile that covers a pixel of the window"""
    y0, x0, h, w = window
    ys = sorted({i for p in (y0, y0 + h - 1) for i in TC.covering(p, H, T, O)})
    xs = sorted({j for p in (x0, x0 + w - 1) for j in TC.covering(p, W, T, O)})
    return (ys[0], xs[0], ys[-1] - ys[0] + 1, xs[-1] - xs[0] + 1)

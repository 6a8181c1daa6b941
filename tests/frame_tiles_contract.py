"""Tiled coding of YUV 4:2:0 frames (progressivecodec_amd/frame_tiles.py, frame_tiles_csrc/pc_frame_tiles.h) restated in numpy from its
definition, not from the kernels: what tests/test_frame_tiles_host.py checks on its own and
tests/test_gpu_frame_tiles.py checks the GPU against.  It is the composition of two restatements: tests/frames_contract.py (section 13:
`rgb`, `emit_codes`, `codes`) per pixel and tests/tiles_contract.py (section 11: `grid`, `blend`, `weights`) per tile.

A frame is frames_contract's, with its leading batch axis of 1; tiles are float32 [n,3,T,T], row-major over a grid rectangle
(ty0, tx0, nty, ntx); a window is (y0, x0, h, w).
"""
import numpy as np

from tests import frames_contract as FC
from tests import tiles_contract as TC


def admissible(H, W, window):
    """y0 and x0 even, h even or the window ends on the frame's last row, w even or it ends on the frame's last column"""
    y0, x0, h, w = window
    return y0 % 2 == 0 and x0 % 2 == 0 and (h % 2 == 0 or y0 + h == H) and (w % 2 == 0 or x0 + w == W)


def cut(planes, fmt, matrix, rng, upsample, T, O, rect=None):
    """float32 [nty*ntx,3,T,T]: tile (i, j) is the crop over [i*S, i*S + T) x [j*S, j*S + T) of the WHOLE frame's ingest (so the chroma
    taps clamp at the frame's edges), +0.0 beyond the frame"""
    x = FC.rgb(planes, fmt, matrix, rng, upsample)[0]
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


def stitch_codes(tiles, H, W, T, O, fmt, matrix, rng, rect=None, window=None, check=True):
    """(Y, Cb, Cr) int64 with a leading axis of 1: section 11's blend m over the window, then section 13's emit on m as if it were the
    decoder's planes, the window being the picture (rows min(2i+1, h-1), columns min(2j+1, w-1)).  check=False: also for a window that
    is not admissible (what the rule is there to exclude)."""
    y0, x0, h, w = (0, 0, H, W) if window is None else window
    if check and not admissible(H, W, (y0, x0, h, w)):
        raise ValueError(f"window {(y0, x0, h, w)} of a {H}x{W} frame is not admissible")
    m = TC.blend(tiles, H, W, T, O, rect, (y0, x0, h, w))
    return FC.emit_codes(m[None], 0, 0, h, w, fmt, matrix, rng)


def stitch(tiles, H, W, T, O, fmt, matrix, rng, rect=None, window=None):
    """the window's frame in `fmt`"""
    return FC.frame(*stitch_codes(tiles, H, W, T, O, fmt, matrix, rng, rect, window), fmt)


def crop_codes(codes, window):
    """the window of a whole frame's (Y, Cb, Cr): luma [y0:y0+h, x0:x0+w], chroma [y0/2 : y0/2 + ceil(h/2), x0/2 : x0/2 + ceil(w/2)]"""
    y0, x0, h, w = window
    hc, wc = FC.chroma_size(h, w)
    Y, Cb, Cr = codes
    return (Y[:, y0:y0 + h, x0:x0 + w], Cb[:, y0 // 2:y0 // 2 + hc, x0 // 2:x0 // 2 + wc], Cr[:, y0 // 2:y0 // 2 + hc, x0 // 2:x0 // 2 + wc])


def sums(tiles, H, W, T, O, fmt, matrix, rng, ref, rect=None, window=None):
    """[3] Python ints: per plane [Y, Cb, Cr] the sum over the window of (code - refcode)^2; ref is the whole original frame"""
    win = (0, 0, H, W) if window is None else window
    got = stitch_codes(tiles, H, W, T, O, fmt, matrix, rng, rect, win)
    want = crop_codes(FC.codes(ref, fmt), win)
    return [int(((g - r) ** 2).sum()) for g, r in zip(got, want)]

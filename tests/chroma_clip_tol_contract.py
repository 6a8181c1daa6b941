"""Tolerant clips of YUV frames of any subsampling and siting (progressivecodec_amd/chroma_clip_tol.py,
chroma_clip_tol_gpu/pc_chroma_clip_tol.h) restated in numpy and pure Python from their definition, not from the
kernels: the difference of a tile between two frames over section 25's footprint, closeness, and section 18's scan.  What
tests/test_chroma_clip_tol_host.py checks on its own and tests/test_gpu_chroma_clip_tol.py checks the GPU against.

A frame is chroma_contract's, with its leading batch axis of 1.  Geometry and footprint are chroma_clips_contract's (section 25):
footprint is imported, not derived again.
"""
import numpy as np

from tests import chroma_clips_contract as CK
from tests import chroma_contract as CC
from tests import tiles_contract as TC
from tests.clip_tol_contract import NO_MSE, close, mse_q10, worst  # noqa: F401  (section 18's, word for word)


def regions(t, H, W, T, O, fmt, siting, upsample):
    """tile t -> the footprint's rectangle (y0, y1, x0, x1), half-open, in each of the three planes"""
    ny, nx = TC.grid(H, W, T, O)
    lu, ch = CK.footprint(t // nx, t % nx, H, W, T, O, fmt, siting, upsample)
    return [lu, ch, ch]


def nsamp(t, H, W, T, O, fmt, siting, upsample):
    return [(r[1] - r[0]) * (r[3] - r[2]) for r in regions(t, H, W, T, O, fmt, siting, upsample)]


def difference(a, b, t, T, O, fmt, siting, upsample):
    """a, b: the three code planes [H, W], [Hc, Wc], [Hc, Wc] of two frames as int64 -> [[count, sse, maxabs] per plane] of tile t"""
    H, W = a[0].shape
    out = []
    for p, r in enumerate(regions(t, H, W, T, O, fmt, siting, upsample)):
        d = np.abs(a[p][r[0]:r[1], r[2]:r[3]] - b[p][r[0]:r[1], r[2]:r[3]])
        out.append([int((d != 0).sum()), int((d * d).sum()), int(d.max())])
    return out


def code_planes(frame, fmt):
    """codes are (element >> shift) & (2^bits - 1)"""
    return [np.asarray(c[0]).astype(np.int64) for c in CC.codes(frame, fmt)]


def scan(frames, fmt, siting, T, O, upsample, max_abs=(0, 0, 0), q10=(NO_MSE,) * 3, max_run=0, against_previous=False):
    """-> (source [F][n], stats [F][n][3][3]).  against_previous: the rule the contract REJECTS -- the difference taken against frame
    k - 1 instead of the anchor -- kept here so that a test can show the two apart."""
    cs = [code_planes(f, fmt) for f in frames]
    H, W = cs[0][0].shape
    ny, nx = TC.grid(H, W, T, O)
    n = ny * nx
    ns = [nsamp(t, H, W, T, O, fmt, siting, upsample) for t in range(n)]
    anchor = [0] * n
    source, stats = [[0] * n], [[[[0, 0, 0] for _ in range(3)] for _ in range(n)]]
    for k in range(1, len(cs)):
        srow, strow = [], []
        for t in range(n):
            d = difference(cs[k], cs[k - 1 if against_previous else anchor[t]], t, T, O, fmt, siting, upsample)
            strow.append(d)
            if close(d, ns[t], max_abs, q10) and (max_run == 0 or k - anchor[t] + 1 <= max_run):
                srow.append(anchor[t])
            else:
                srow.append(k)
                anchor[t] = k
        source.append(srow)
        stats.append(strow)
    return source, stats


def workspace_size(T, sy, n_tiles):
    """72 bytes per block, T*T/(2048*sy) + 1 blocks per tile, 4 bytes per tile for the anchors, rounded up to 8"""
    return (72 * n_tiles * (T * T // (2048 * sy) + 1) + 4 * n_tiles + 7) // 8 * 8

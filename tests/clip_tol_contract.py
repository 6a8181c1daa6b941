"""Tolerant clips (progressivecodec_amd/clip_tol.py, clip_tol_csrc/pc_clip_tol.h) restated in numpy and pure Python from their
definition, not from the kernels: the difference of a tile between two frames, closeness, and the scan.  What
tests/test_clip_tol_host.py checks on its own and tests/test_gpu_clip_tol.py checks the GPU against.

A frame is frames_contract's, with its leading batch axis of 1.  Geometry and footprint are clips_contract's (section 16).
"""
from fractions import Fraction

import numpy as np

from tests import clips_contract as CC
from tests import frames_contract as FC
from tests import tiles_contract as TC

NO_MSE = 1 << 30


def mse_q10(max_mse):
    """the unit is 1/1024 code^2, the value taken exactly; None: no MSE condition"""
    if max_mse is None:
        return NO_MSE
    q = Fraction(max_mse) * 1024
    return q.numerator // q.denominator


def regions(t, H, W, T, O, upsample):
    """tile t -> the footprint's rectangle (y0, y1, x0, x1), half-open, in each of the three planes"""
    ny, nx = TC.grid(H, W, T, O)
    lu, ch = CC.footprint(t // nx, t % nx, H, W, T, O, upsample)
    return [lu, ch, ch]


def nsamp(t, H, W, T, O, upsample):
    return [(r[1] - r[0]) * (r[3] - r[2]) for r in regions(t, H, W, T, O, upsample)]


def difference(a, b, t, T, O, upsample):
    """a, b: the three code planes [H, W], [Hc, Wc], [Hc, Wc] of two frames as int64 -> [[count, sse, maxabs] per plane] of tile t"""
    H, W = a[0].shape
    out = []
    for p, r in enumerate(regions(t, H, W, T, O, upsample)):
        d = np.abs(a[p][r[0]:r[1], r[2]:r[3]] - b[p][r[0]:r[1], r[2]:r[3]])
        out.append([int((d != 0).sum()), int((d * d).sum()), int(d.max())])
    return out


def close(diff, ns, max_abs, q10):
    return all(diff[p][2] <= max_abs[p] and 1024 * diff[p][1] <= q10[p] * ns[p] for p in range(3))


def code_planes(frame, fmt):
    return [np.asarray(c[0]).astype(np.int64) for c in FC.codes(frame, fmt)]


def scan(frames, fmt, T, O, upsample, max_abs=(0, 0, 0), q10=(NO_MSE,) * 3, max_run=0, against_previous=False):
    """-> (source [F][n], stats [F][n][3][3]).  against_previous: the rule the contract REJECTS -- the difference taken against frame
    k - 1 instead of the anchor -- kept here so that a test can show the two apart."""
    cs = [code_planes(f, fmt) for f in frames]
    H, W = cs[0][0].shape
    ny, nx = TC.grid(H, W, T, O)
    n = ny * nx
    ns = [nsamp(t, H, W, T, O, upsample) for t in range(n)]
    anchor = [0] * n
    source, stats = [[0] * n], [[[[0, 0, 0] for _ in range(3)] for _ in range(n)]]
    for k in range(1, len(cs)):
        srow, strow = [], []
        for t in range(n):
            d = difference(cs[k], cs[k - 1 if against_previous else anchor[t]], t, T, O, upsample)
            strow.append(d)
            if close(d, ns[t], max_abs, q10) and (max_run == 0 or k - anchor[t] + 1 <= max_run):
                srow.append(anchor[t])
            else:
                srow.append(k)
                anchor[t] = k
        source.append(srow)
        stats.append(strow)
    return source, stats


def worst(source, stats):
    """per plane the largest maxabs over the reused (k, t); 0 where nothing was reused"""
    return [max([stats[k][t][p][2] for k, row in enumerate(source) for t, s in enumerate(row) if s != k], default=0) for p in range(3)]


def workspace_size(T, n_tiles):
    return (72 * n_tiles * (T * T // 4096 + 1) + 4 * n_tiles + 7) // 8 * 8

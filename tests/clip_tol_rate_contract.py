"""Tolerant rate-controlled clips (progressivecodec_amd/clip_tol_rate.py, clip_tol_rate_hip/pc_clip_tol_rate.h) restated from their
definition, not from the module: the distortions of a decoded tile against every frame of its run, the
allocation's dists / weights / M, the per-frame sums of the plan, the container's length and the workspace formula.  What
tests/test_clip_tol_rate_host.py checks on its own and tests/test_gpu_clip_tol_rate.py checks the GPU against.  One (tile, frame) pair
is tests/clip_rate_contract.job_sse's job; the source table is tests/clip_tol_contract.scan's; the allocator is
tests/rate_contract.allocate.
"""
import math
from fractions import Fraction

from tests import clip_rate_contract as RC2

HEADER_BYTES = RC2.HEADER_BYTES
ENTRY_BYTES = RC2.ENTRY_BYTES


def offsets_of(runs):
    """job m's entries are [offsets[m], offsets[m + 1])"""
    off = [0]
    for run in runs:
        off.append(off[-1] + len(run))
    return off


def expanded(tile_ids, runs):
    """the job list clip_rate would need -- one (frame, tile) job per entry -- and, per entry, the decoded tile it belongs to"""
    jobs = [(f, t) for t, run in zip(tile_ids, runs) for f in run]
    owner = [m for m, run in enumerate(runs) for _ in run]
    return jobs, owner


def run_sse(tiles, frames, tile_ids, runs, H, W, T, O, fmt, matrix, rng):
    """[n_entries][3] Python ints: row offsets[m] + j is clip_rate_contract.job_sse of tiles[m] for the job (runs[m][j], tile_ids[m])"""
    jobs, owner = expanded(tile_ids, runs)
    return RC2.job_sse(tiles[owner], frames, jobs, H, W, T, O, fmt, matrix, rng)


def frame_scale(frame_weights, F):
    """(M, fwi): the least common multiple of the denominators of the frame weights taken exactly, and frame_weights[k] * M as ints"""
    fw = [Fraction(1)] * F if frame_weights is None else [Fraction(v) for v in frame_weights]
    M = math.lcm(*[v.denominator for v in fw])
    fwi = [v * M for v in fw]
    assert all(v.denominator == 1 for v in fwi)
    return M, [v.numerator for v in fwi]


def dists(plane_dists, runs, plane_weights=(1, 1, 1), frame_weights=None, F=None):
    """dists[i][l] = sum over j of fwi[runs[i][j]] * (wY d[0] + wCb d[1] + wCr d[2]), d = plane_dists[i][l][j]"""
    F = 1 + max(k for run in runs for k in run) if F is None else F
    _, fwi = frame_scale(frame_weights, F)
    out = []
    for run, item in zip(runs, plane_dists):
        row = []
        for per_frame in item:
            assert len(per_frame) == len(run)
            row.append(sum(fwi[k] * sum(w * v for w, v in zip(plane_weights, d)) for k, d in zip(run, per_frame)))
        out.append(row)
    return out


def weights(items, importance=None):
    """weights[i] = importance[t], exactly; the frames' weights are inside dists"""
    return [Fraction(1) if importance is None else Fraction(importance[t]) for _, t in items]


def frame_sse(source, plane_dists, levels):
    """sse[k][p]: over the tiles t of frame k, plane_dists[i][levels[i]][j][p] of the item i = (source[k][t], t), j the position of k in
    its run"""
    items, runs = RC2.items_of(source)
    out = []
    for k in range(len(source)):
        row = [0, 0, 0]
        for t, s in enumerate(source[k]):
            i = items.index((s, t))
            d = plane_dists[i][levels[i]][runs[i].index(k)]
            for p in range(3):
                row[p] += d[p]
        out.append(row)
    return out


def predicted(plane_dists, levels, plane_weights=(1, 1, 1)):
    """the chosen distortions over every frame of every run, the planes weighted, the frames not"""
    return sum(sum(w * v for w, v in zip(plane_weights, d)) for item, l in zip(plane_dists, levels) for d in item[l])


def container_bytes(rates, levels, F, n_tiles):
    return RC2.container_bytes(rates, levels, F, n_tiles)


def workspace_size(T, n_entries):
    """24 bytes per wave and entry: T * T / 4096 blocks of four waves per job"""
    return 96 * (T * T // 4096) * n_entries

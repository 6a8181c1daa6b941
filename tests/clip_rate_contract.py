"""Rate-controlled clips (progressivecodec_amd/clip_rate.py, clip_rate_csrc/pc_clip_rate.h) restated from their definition (DESIGN.md
section 17), not from the module: the allocation's items and the frames each is shown in, the item weights, the allocator's budget,
the PCS2 layout and the per-frame sums of the plan.  What tests/test_clip_rate_host.py checks on its own and tests/test_gpu_clip_rate.py
checks the GPU against.  The distortion of one job is tests/frame_rate_contract.tile_sse of its tile against its frame; the allocator
is tests/rate_contract.allocate.
"""
from fractions import Fraction

from tests import clips_contract as CC
from tests import frame_rate_contract as QC

MAGIC = b"PCS2"
HEADER_BYTES = 42
ENTRY_BYTES = 16


def items_of(source):
    """(items, runs): an item is a tile where it is coded, (f, t) with source[f][t] == f, in (f, t) order; its run is every frame k
    whose tile t points at frame f, ascending"""
    items, runs = [], []
    for f in range(len(source)):
        for t in range(len(source[f])):
            if source[f][t] == f:
                items.append((f, t))
                runs.append([k for k in range(len(source)) if source[k][t] == f])
    return items, runs


def weights(source, importance=None, frame_weights=None):
    """per item: importance[t] times the sum of frame_weights over its run, exactly; the defaults are 1"""
    items, runs = items_of(source)
    out = []
    for (f, t), run in zip(items, runs):
        w = Fraction(0)
        for k in run:
            w += Fraction(1) if frame_weights is None else Fraction(frame_weights[k])
        out.append(w * (Fraction(1) if importance is None else Fraction(importance[t])))
    return out


def budget(target_bytes, F, n_tiles):
    """what is left for the coded tiles' containers: the header and the table (16 bytes per frame and tile, reused or not) are fixed"""
    return target_bytes - HEADER_BYTES - ENTRY_BYTES * F * n_tiles


def pack_clip(blobs, source, H, W, T, O, fmt, matrix, rng, upsample, contract):
    """PCS2: PCS1's layout (tests/clips_contract.pack_clip) under the magic "PCS2" """
    b = CC.pack_clip(blobs, source, H, W, T, O, fmt, matrix, rng, upsample, contract)
    assert b[:4] == CC.MAGIC
    return MAGIC + b[4:]


def container_bytes(rates, levels, F, n_tiles):
    """42 + the table + the chosen containers of the items"""
    return HEADER_BYTES + ENTRY_BYTES * F * n_tiles + sum(r[l] for r, l in zip(rates, levels))


def frame_sse(source, plane_dists, levels):
    """sse[k][p]: over the tiles of frame k, the chosen plane_dists of the items they point at"""
    items, _ = items_of(source)
    out = []
    for k in range(len(source)):
        row = [0, 0, 0]
        for t, s in enumerate(source[k]):
            i = items.index((s, t))
            for p in range(3):
                row[p] += plane_dists[i][levels[i]][p]
        out.append(row)
    return out


def predicted(source, dists, levels):
    """the chosen dists summed over every frame and tile: an item counts once per frame of its run"""
    items, runs = items_of(source)
    return sum(len(run) * dists[i][levels[i]] for i, run in enumerate(runs))


def job_sse(tiles, frames, jobs, H, W, T, O, fmt, matrix, rng):
    """[n][3] Python ints: row m is frame_rate_contract.tile_sse of tiles[m] as tile jobs[m][1] against frames[jobs[m][0]]"""
    return [QC.tile_sse(tiles[m:m + 1], H, W, T, O, fmt, matrix, rng, frames[f], first_tile=t)[0] for m, (f, t) in enumerate(jobs)]

"""Tolerant rate-controlled clips of YUV frames of any subsampling and siting (progressivecodec_amd/chroma_clip_tol_rate.py,
chroma_clip_tol_rate_gpu/pc_chroma_clip_tol_rate.h) restated from their definition, not from the module: the
distortions of a decoded tile against every frame of its run, the allocation's numbers, the per-frame sums of the plan, the
container's length and the workspace formula.  What tests/test_chroma_clip_tol_rate_host.py checks on its own and
tests/test_gpu_chroma_clip_tol_rate.py checks the GPU against.  Not a test file.  One (tile, frame) pair is
tests/chroma_rate_contract.tile_sse of the tile against the frame: imported, not derived again.  Section 20's numbers -- offsets, the
expanded job list, M and fwi, dists, weights, sse, predicted -- do not depend on the format and are tests/clip_tol_rate_contract's;
the source table is tests/chroma_clip_tol_contract.scan's; the allocator is tests/rate_contract.allocate; the budget and the
container are section 28's (47 bytes of header where section 20 has 42, PCL2 where it has PCS2).
"""
from tests import chroma_clip_rate_contract as JC
from tests import chroma_rate_contract as XC
from tests.clip_tol_rate_contract import dists, expanded, frame_scale, frame_sse, offsets_of, predicted, weights  # noqa: F401

MAGIC = JC.MAGIC
HEADER_BYTES = 47
ENTRY_BYTES = 16
assert (MAGIC, JC.HEADER_BYTES, JC.ENTRY_BYTES) == (b"PCL2", HEADER_BYTES, ENTRY_BYTES)


def run_sse(tiles, frames, tile_ids, runs, H, W, T, O, fmt, matrix, rng, siting):
    """[n_entries][3] Python ints: row offsets[m] + j is chroma_rate_contract.tile_sse of tiles[m] as tile tile_ids[m] against
    frames[runs[m][j]]"""
    return [XC.tile_sse(tiles[m:m + 1], H, W, T, O, fmt, matrix, rng, siting, frames[f], first_tile=t)[0]
            for m, (t, run) in enumerate(zip(tile_ids, runs)) for f in run]


def budget(target_bytes, F, n_tiles):
    """what is left for the coded tiles' containers: target_bytes - 47 - 16 * F * ny * nx"""
    return target_bytes - HEADER_BYTES - ENTRY_BYTES * F * n_tiles


def container_bytes(rates, levels, F, n_tiles):
    """47 + the table + the chosen containers of the items"""
    return HEADER_BYTES + ENTRY_BYTES * F * n_tiles + sum(r[l] for r, l in zip(rates, levels))


def workspace_size(T, sy, n_entries):
    """24 bytes per wave and entry: T * T / (2048 sy) blocks of four waves per job"""
    return 96 * (T * T // (2048 * sy)) * n_entries

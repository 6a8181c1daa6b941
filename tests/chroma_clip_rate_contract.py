"""Rate-controlled clips of YUV frames of any subsampling and siting (progressivecodec_amd/chroma_clip_rate.py,
chroma_clip_rate_kernels/pc_chroma_clip_rate.h) restated from their definition, not from the module: the sums
of a job, the allocator's budget and the PCL2 bytes.  What tests/test_chroma_clip_rate_host.py checks on its own and
tests/test_gpu_chroma_clip_rate.py checks the GPU against.  Not a test file.  The distortion of one job is
tests/chroma_rate_contract.tile_sse of its tile against its frame; the items, the weights and the plan's sums are
tests/clip_rate_contract's (they do not depend on the format); the allocator is tests/rate_contract.allocate.
"""
from tests import chroma_clips_contract as CK
from tests import chroma_rate_contract as XC
from tests.clip_rate_contract import frame_sse, items_of, predicted, weights  # noqa: F401

MAGIC = b"PCL2"
HEADER_BYTES = 47
ENTRY_BYTES = 16


def job_sse(tiles, frames, jobs, H, W, T, O, fmt, matrix, rng, siting):
    """[n][3] Python ints: row m is chroma_rate_contract.tile_sse of tiles[m] as tile jobs[m][1] against frames[jobs[m][0]]"""
    return [XC.tile_sse(tiles[m:m + 1], H, W, T, O, fmt, matrix, rng, siting, frames[f], first_tile=t)[0] for m, (f, t) in enumerate(jobs)]


def measured(i, L, T, O, subsampled):
    """tile i along an axis of length L -> ((luma first, luma end), (chroma first, chroma last)), the second pair inclusive: what a
    job reads of the ORIGINAL frame along the axis -- the tile's luma positions and its chroma cells, no halo under any siting"""
    S = T - O
    e = min(i * S + T, L)
    if not subsampled:
        return (i * S, e), (i * S, e - 1)
    return (i * S, e), (i * S // 2, i * S // 2 + -(-(e - i * S) // 2) - 1)


def budget(target_bytes, F, n_tiles):
    """what is left for the coded tiles' containers: the header and the table (16 bytes per frame and tile, reused or not) are fixed"""
    return target_bytes - HEADER_BYTES - ENTRY_BYTES * F * n_tiles


def container_bytes(rates, levels, F, n_tiles):
    """47 + the table + the chosen containers of the items"""
    return HEADER_BYTES + ENTRY_BYTES * F * n_tiles + sum(r[l] for r, l in zip(rates, levels))


def pack_clip(blobs, source, H, W, T, O, fmt, matrix, rng, upsample, siting, contract):
    """PCL2: PCL1's layout (tests/chroma_clips_contract.pack_clip) under the magic "PCL2" """
    b = CK.pack_clip(blobs, source, H, W, T, O, fmt, matrix, rng, upsample, siting, contract)
    assert b[:4] == CK.MAGIC and len(MAGIC) == 4
    return MAGIC + b[4:]


def frame_container(blobs, H, W, T, O, fmt, matrix, rng, upsample, siting, contract):
    """the PCK1 container of one frame from its tiles' single-level blobs: PCK1's 15 bytes, then PCT1's layout under the magic "PCT2" """
    b = CK.frame_container(blobs, H, W, T, O, fmt, matrix, rng, upsample, siting, contract)
    assert b[15:19] == b"PCT1"
    return b[:15] + b"PCT2" + b[19:]

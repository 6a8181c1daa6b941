"""Clips of YUV 4:2:0 frames (progressivecodec_amd/clips.py, clips_csrc/pc_clips.h) restated in numpy from their definition (DESIGN.md
section 16), not from the kernels: the footprint of a tile, the change counts over it, the source table and the PCS1 layout.  What
tests/test_clips_host.py checks on its own (against tests/frame_tiles_contract.cut) and tests/test_gpu_clips.py checks the GPU against.

A frame is frames_contract's, with its leading batch axis of 1.  Geometry is tiles_contract's: T, O, S = T - O, the ny x nx grid.
"""
import struct

import numpy as np

from tests import frames_contract as FC
from tests import tiles_contract as TC

MAGIC = b"PCS1"
HEADER_BYTES = 42
FMT_ID = {"nv12": 0, "i420": 1, "p010": 2}
MATRIX_ID = {"bt601": 0, "bt709": 1, "bt2020": 2}
RANGE_ID = {"limited": 0, "full": 1}
UPSAMPLE_ID = {"nearest": 0, "linear": 1}


def halo_of(upsample):
    return {"linear": 1, "nearest": 0}[upsample]


def axis_footprint(i, L, T, O, halo):
    """tile i along an axis of length L -> ((luma first, luma end), (chroma first, chroma last)): the second pair is inclusive"""
    S = T - O
    Lc = -(-L // 2)
    e = min(i * S + T, L)
    return (i * S, e), (max(i * S // 2 - halo, 0), min(-(-e // 2) - 1 + halo, Lc - 1))


def footprint(i, j, H, W, T, O, upsample):
    """tile (i, j) -> (luma (y0, y1, x0, x1), chroma (y0, y1, x0, x1)) as half-open ranges of the planes; Cb and Cr share the second"""
    h = halo_of(upsample)
    (ly0, ly1), (cy0, cy1) = axis_footprint(i, H, T, O, h)
    (lx0, lx1), (cx0, cx1) = axis_footprint(j, W, T, O, h)
    return (ly0, ly1, lx0, lx1), (cy0, cy1 + 1, cx0, cx1 + 1)


def tile_changes(cur, prev, fmt, T, O, upsample, first_tile=0, n_tiles=None):
    """[n][3] Python ints: per tile of the linear range and plane [Y, Cb, Cr], the number of samples of the footprint whose codes
    (the element, or word >> 6 for P010) differ between the two frames"""
    a, b = FC.codes(cur, fmt), FC.codes(prev, fmt)
    H, W = a[0].shape[1:]
    ny, nx = TC.grid(H, W, T, O)
    n = ny * nx - first_tile if n_tiles is None else n_tiles
    if first_tile < 0 or n < 1 or first_tile + n > ny * nx:
        raise ValueError((first_tile, n_tiles))
    d = [x[0] != y[0] for x, y in zip(a, b)]
    out = []
    for t in range(first_tile, first_tile + n):
        lu, ch = footprint(t // nx, t % nx, H, W, T, O, upsample)
        out.append([int(d[0][lu[0]:lu[1], lu[2]:lu[3]].sum())] + [int(d[p][ch[0]:ch[1], ch[2]:ch[3]].sum()) for p in (1, 2)])
    return out


def source_table(frames, fmt, T, O, upsample):
    """source[f][t] for a list of frames: 0 in frame 0; source[f - 1][t] where all three counts of tile t between frames f - 1 and f
    are zero; else f"""
    H, W = np.asarray(frames[0][0]).shape[1:]
    ny, nx = TC.grid(H, W, T, O)
    source = [[0] * (ny * nx)]
    for f in range(1, len(frames)):
        counts = tile_changes(frames[f], frames[f - 1], fmt, T, O, upsample)
        source.append([source[f - 1][t] if counts[t] == [0, 0, 0] else f for t in range(ny * nx)])
    return source


def pack_clip(blobs, source, H, W, T, O, fmt, matrix, rng, upsample, contract):
    """PCS1: the 42-byte header, F*ny*nx entries (offset u64, length u64) from the container's start, frame first and row-major
    within a frame, then the blobs of the coded tiles (source[f][t] == f) in (frame, tile) order; a reused tile repeats the entry of
    the frame it was last coded in"""
    ny, nx = TC.grid(H, W, T, O)
    n, F = ny * nx, len(source)
    head = MAGIC + struct.pack("<6B", 1, FMT_ID[fmt], MATRIX_ID[matrix], RANGE_ID[rng], UPSAMPLE_ID[upsample], FC.bits(fmt))
    head += struct.pack("<I", contract) + struct.pack("<7I", H, W, T, O, ny, nx, F)
    assert len(head) == HEADER_BYTES
    off = HEADER_BYTES + 16 * F * n
    where, table, payload = {}, b"", b""
    for f in range(F):
        for t in range(n):
            if source[f][t] == f:
                where[(f, t)] = (off, len(blobs[f][t]))
                payload += blobs[f][t]
                off += len(blobs[f][t])
            table += struct.pack("<QQ", *where[(source[f][t], t)])
    return head + table + payload


def container_bytes(blobs, source):
    """42 + the table + the sum of the coded tiles' blobs"""
    F, n = len(source), len(source[0])
    return HEADER_BYTES + 16 * F * n + sum(len(blobs[f][t]) for f in range(F) for t in range(n) if source[f][t] == f)

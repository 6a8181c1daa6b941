"""Clips of YUV frames of any subsampling and siting (progressivecodec_amd/chroma_clips.py, chroma_clips_kernels/pc_chroma_clips.h)
restated in numpy from their definition, not from the kernels: the footprint of a tile, the change counts over
it, the source table, the PCL1 layout and the PCK1 / PCT1 bytes of one frame of it.  What tests/test_chroma_clips_host.py checks on its
own (against tests/chroma_tiles_contract.cut and tests/chroma_contract.taps) and tests/test_gpu_chroma_clips.py checks the GPU against.

A frame is chroma_contract's, with its leading batch axis of 1.  Geometry is tiles_contract's: T, O, S = T - O, the ny x nx grid.
"""
import struct

import numpy as np

from tests import chroma_contract as CC
from tests import tiles_contract as TC

MAGIC = b"PCL1"
HEADER_BYTES = 47
MATRIX_ID = {"bt601": 0, "bt709": 1, "bt2020": 2}
RANGE_ID = {"limited": 0, "full": 1}
UPSAMPLE_ID = {"nearest": 0, "linear": 1}


def axis_footprint(i, L, T, O, subsampled, linear, cosited):
    """tile i along an axis of length L -> ((luma first, luma end), (chroma first, chroma last)): the second pair is inclusive"""
    S = T - O
    e = min(i * S + T, L)
    if not subsampled:
        return (i * S, e), (i * S, e - 1)
    Lc = -(-L // 2)
    hi = 1 if linear else 0
    lo = 1 if linear and not cosited else 0
    return (i * S, e), (max(i * S // 2 - lo, 0), min(-(-e // 2) - 1 + hi, Lc - 1))


def footprint(i, j, H, W, T, O, fmt, siting, upsample):
    """tile (i, j) -> (luma (y0, y1, x0, x1), chroma (y0, y1, x0, x1)) as half-open ranges of the planes; Cb and Cr share the second"""
    sx, sy = CC.sub(fmt)
    hco, vco = CC.SITINGS[siting]
    linear = {"nearest": False, "linear": True}[upsample]
    (ly0, ly1), (cy0, cy1) = axis_footprint(i, H, T, O, sy == 2, linear, vco)
    (lx0, lx1), (cx0, cx1) = axis_footprint(j, W, T, O, sx == 2, linear, hco)
    return (ly0, ly1, lx0, lx1), (cy0, cy1 + 1, cx0, cx1 + 1)


def footprint_sizes(H, W, T, O, fmt, siting, upsample):
    """[n][3]: the number of samples of every tile's footprint per plane"""
    ny, nx = TC.grid(H, W, T, O)
    out = []
    for t in range(ny * nx):
        lu, ch = footprint(t // nx, t % nx, H, W, T, O, fmt, siting, upsample)
        out.append([(lu[1] - lu[0]) * (lu[3] - lu[2])] + [(ch[1] - ch[0]) * (ch[3] - ch[2])] * 2)
    return out


def tile_changes(cur, prev, fmt, siting, T, O, upsample, first_tile=0, n_tiles=None):
    """[n][3] Python ints: per tile of the linear range and plane [Y, Cb, Cr], the number of samples of the footprint whose codes
    ((element >> shift) & (2^bits - 1)) differ between the two frames"""
    a, b = CC.codes(cur, fmt), CC.codes(prev, fmt)
    H, W = a[0].shape[1:]
    ny, nx = TC.grid(H, W, T, O)
    n = ny * nx - first_tile if n_tiles is None else n_tiles
    if first_tile < 0 or n < 1 or first_tile + n > ny * nx:
        raise ValueError((first_tile, n_tiles))
    d = [x[0] != y[0] for x, y in zip(a, b)]
    out = []
    for t in range(first_tile, first_tile + n):
        lu, ch = footprint(t // nx, t % nx, H, W, T, O, fmt, siting, upsample)
        out.append([int(d[0][lu[0]:lu[1], lu[2]:lu[3]].sum())] + [int(d[p][ch[0]:ch[1], ch[2]:ch[3]].sum()) for p in (1, 2)])
    return out


def source_table(frames, fmt, siting, T, O, upsample):
    """source[f][t] for a list of frames: 0 in frame 0; source[f - 1][t] where all three counts of tile t between frames f - 1 and f
    are zero; else f"""
    H, W = np.asarray(frames[0][0]).shape[1:]
    ny, nx = TC.grid(H, W, T, O)
    source = [[0] * (ny * nx)]
    for f in range(1, len(frames)):
        counts = tile_changes(frames[f], frames[f - 1], fmt, siting, T, O, upsample)
        source.append([source[f - 1][t] if counts[t] == [0, 0, 0] else f for t in range(ny * nx)])
    return source


def format_bytes(fmt, matrix, rng, upsample, siting):
    """PCK1's ten bytes: layout, shift, sx, sy, horizontal siting, vertical siting, matrix, range, upsample, bits"""
    semi, bits, shift, sx, sy = CC.FORMATS[fmt]
    hco, vco = CC.SITINGS[siting]
    return struct.pack("<10B", int(semi), shift, sx, sy, int(hco), int(vco), MATRIX_ID[matrix], RANGE_ID[rng], UPSAMPLE_ID[upsample], bits)


def pack_clip(blobs, source, H, W, T, O, fmt, matrix, rng, upsample, siting, contract):
    """PCL1: the 47-byte header, F*ny*nx entries (offset u64, length u64) from the container's start, frame first and row-major
    within a frame, then the blobs of the coded tiles (source[f][t] == f) in (frame, tile) order; a reused tile repeats the entry of
    the frame it was last coded in"""
    ny, nx = TC.grid(H, W, T, O)
    n, F = ny * nx, len(source)
    head = MAGIC + struct.pack("<B", 1) + format_bytes(fmt, matrix, rng, upsample, siting)
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


def frame_container(blobs, H, W, T, O, fmt, matrix, rng, upsample, siting, contract):
    """the PCK1 container of one frame from its tiles' blobs: "PCK1", version 1, the ten bytes, then the PCT1 container -- "PCT1",
    version u8, contract u32, H, W, T, O, ny, nx as u32, one (offset u64, length u64) entry per tile from ITS start, the blobs"""
    ny, nx = TC.grid(H, W, T, O)
    assert len(blobs) == ny * nx
    inner = b"PCT1" + struct.pack("<BI6I", 1, contract, H, W, T, O, ny, nx)
    off = len(inner) + 16 * len(blobs)
    for b in blobs:
        inner += struct.pack("<QQ", off, len(b))
        off += len(b)
    return b"PCK1" + struct.pack("<B", 1) + format_bytes(fmt, matrix, rng, upsample, siting) + inner + b"".join(blobs)

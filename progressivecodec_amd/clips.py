"""Clips of YUV 4:2:0 frames (libpc_clips.so, clips_csrc/pc_clips.h): a sequence of NV12 / I420 / P010 frames is
coded tile by tile as frame_tiles.py codes one frame, with two differences: the tiles of several frames share a codec call, and a tile
whose samples did not change since the previous frame is neither cut, coded nor stored again -- its table entry points at the bytes
of the frame it was last coded in.  No inter-frame prediction, no drift, no decode dependency: every frame of the clip is what
frame_tiles.encode_frame_tiled / decode_frame_tiled give for that frame alone, byte for byte and bit for bit.

  tile_changes     two frames -> per tile and plane the number of samples of the tile's footprint whose codes differ, exact, on the GPU
  clip_changes     a clip -> the same for every frame against the one before it, F - 1 launches and no host synchronisation
  cut_tiles        frame + a list of tile indices -> float32 tiles [n,3,T,T], one launch (frame_tiles.cut_frame takes rectangles only)
  encode_clip      clip -> (one PCS1 container, ClipPlan): static tiles coded once, the work list chunked across frames
  decode_clip      PCS1 container -> a list of frames (or of one region of each); among consecutive frames a byte range is decoded once
  frame_container  PCS1 container, k -> the PCG1 container of frame k (pure byte work)

Footprint of a tile (the contract, pc_clips.h).  Geometry is tiles.py's: T, O, S = T - O, the ny x nx grid.  halo = 1 for
upsample = "linear", 0 for "nearest".  Along an axis of length L with Lc = ceil(L / 2), tile i reads luma positions [i*S, e),
e = min(i*S + T, L), and chroma positions [max(i*S/2 - halo, 0), min(ceil(e/2) - 1 + halo, Lc - 1)]; the footprint of tile (i, j) is
the product of the two axes' ranges, once in the luma plane and once each in Cb and Cr.  Codes are the element for the 8-bit formats
and word >> 6 for P010.  If every code in the footprint is the same in two frames, the cut of the tile is the same bits, and so are
its PCB1 bytes (they do not depend on the batch a tile is coded in).

A clip is a list of frames (frames.py's tuples) of one size on one device, or one tuple of batched planes ([F,H,W] and so on), taken
frame by frame through their batch stride without a copy.

PCS1 layout (little endian): magic "PCS1", version u8 (= 1), fmt, matrix, range, upsample, bits as one byte each (PCF1's ids),
numeric contract id u32, H, W, T, O, ny, nx, F as u32 each -- 42 bytes; then F*ny*nx table entries (offset u64, length u64) from the
container's start, frame by frame and row-major within a frame; then the PCB1 containers of the CODED tiles in (frame, tile) order,
each exactly what container.pack makes (image_size = (T, T)).  The entry of a reused tile repeats the entry of the frame it was last
coded in: two entries are either equal or disjoint, anything else is refused.  An entry is checked against the buffer when its tile
is asked for, so a clip cut off inside its payload still gives every frame whose tiles it holds completely.

There is no CPU fallback: CPU tensors raise ValueError before any device call.  Everything runs on the current stream of the tensors'
device.  A tolerance (near-static tiles reused under an exact error bound) is clip_tol.py's, which produces this module's container.
Out of scope: any inter-frame prediction, matching a tile against anything but the same tile of an earlier frame, rate control over
a clip (clip_rate.py), compress_with_ac.  4:2:2 / 4:4:4 and left- / top-left-sited chroma: chroma_clips.py, which is this module for
the twelve formats and three sitings of chroma.py and shares this module's decode loop.
"""
import collections
import ctypes as C
import operator
import struct

from . import _imagelib, _tilecodec
from ._lib import PC_OK
from .container import ContainerError
from .frame_tiles import _admissible_window, _one_frame, pack_frame_tiled, stitch_frame
from .frames import FORMATS, RANGES, UPSAMPLES, _MATRIX_ID, Frame, _check_enums, _frame_struct, _frame_view, bits_of, coefficients
from .tiles import grid_of, pack_tiled

LIB_PATH = _imagelib.lib_path("clips")

#: every symbol clips_csrc/pc_clips.h declares
EXPORTS = ["pc_clips_changes_workspace_size", "pc_clips_tile_changes", "pc_clips_cut_list", "pc_clips_plan", "pc_clips_strerror",
           "pc_clips_last_hip_error"]

CHANGES, CUT = 0, 1                       # pc_clips_plan's `op`
MAX_TILE = 2048                           # pc_clips.h

MAGIC = b"PCS1"
VERSION = 1
_HEAD = "<BBBBBBIIIIIIII"                 # version, fmt, matrix, range, upsample, bits, contract id, H, W, T, O, ny, nx, F
HEADER_BYTES = 4 + struct.calcsize(_HEAD)
ENTRY_BYTES = 16

_range = range                            # the functions below take a parameter of that name


def _prototypes():
    vp, ci, cf, fp = C.c_void_p, C.c_int, C.c_float, C.POINTER(Frame)
    return {
        "pc_clips_changes_workspace_size": (C.c_size_t, [ci, ci]),
        "pc_clips_tile_changes": (None, [fp, fp] + [ci] * 8 + [vp, C.c_size_t, vp, vp]),
        "pc_clips_cut_list": (None, [fp, ci, ci, ci, cf, cf, cf, cf] + [ci] * 4 + [vp, ci, vp, vp]),
        "pc_clips_plan": (None, [ci, ci, fp, fp, vp, ci, C.POINTER(ci)]),
        "pc_clips_strerror": (C.c_char_p, [ci]),
    }


def lib():
    return _imagelib.load(LIB_PATH, _prototypes)


class ClipsError(_imagelib.ImageLibError):
    _lib, _prefix = staticmethod(lib), "pc_clips"


#: what encode_clip decided: source[f][t] (the frame tile t of frame f was last coded in: f itself where it was coded for frame f),
#: n_coded and n_reused (they add up to F * ny * nx) and container_bytes (the length of the container)
ClipPlan = collections.namedtuple("ClipPlan", "source n_coded n_reused container_bytes")


def _grid(H, W, tile, overlap):
    g = grid_of(H, W, tile, overlap)
    if g.T > MAX_TILE:
        raise ValueError(f"tile must be at most {MAX_TILE}, got {g.T}")
    return g


def _clip_frames(frames, fmt, what="frames", view=None, one=None):
    """a clip -> ([the planes of frame k as batched views [1,...], ...], H, W): a list of frames of one size on one device, or one
    tuple of batched planes, taken through their batch stride without a copy (frames._frame_view copies a plane only where its
    innermost strides do not fit).  view, one: another module's _frame_view and _one_frame (chroma_clips.py: the twelve formats)"""
    import torch
    if isinstance(frames, (tuple, list)) and frames and torch.is_tensor(frames[0]):
        if frames[0].dim() == 2:
            raise ValueError(f"{what} must be a list of frames or batched planes [F,H,W], got one frame")
        ts, B, H, W, _ = (view or _frame_view)(frames, fmt, what)
        return [[t[k:k + 1] for t in ts] for k in _range(B)], H, W
    if not isinstance(frames, (tuple, list)) or not frames:
        raise ValueError(f"{what} must be a non-empty list of frames or a tuple of batched planes")
    out, size = [], None
    for k, f in enumerate(frames):
        ts, H, W = (one or _one_frame)(f, fmt, f"{what}[{k}]")
        if size is None:
            size = (H, W, ts[0].device)
        elif size != (H, W, ts[0].device):
            raise ValueError(f"{what}[{k}] is {H}x{W} on {ts[0].device}, {what}[0] is {size[0]}x{size[1]} on {size[2]}")
        out.append(ts)
    return out, size[0], size[1]


def _tile_range(g, first_tile, n_tiles):
    first_tile = int(first_tile)
    n = g.ny * g.nx - first_tile if n_tiles is None else int(n_tiles)
    if first_tile < 0 or n < 1 or first_tile + n > g.ny * g.nx:
        raise ValueError(f"tiles {first_tile} .. {first_tile + n - 1} lie outside the {g.ny}x{g.nx} grid")
    return first_tile, n


def _changes_into(L, cur, prev, fmt, upsample, g, first, n, ws, nbytes, out, stream):
    a, b = _frame_struct(cur), _frame_struct(prev)
    rc = L.pc_clips_tile_changes(C.byref(a), C.byref(b), FORMATS[fmt], UPSAMPLES[upsample], g.H, g.W, g.T, g.O, first, n, ws.data_ptr(),
                                 nbytes, out.data_ptr(), stream)
    if rc != PC_OK:
        raise ClipsError(rc, "pc_clips_tile_changes")


def tile_changes(cur, prev, fmt, tile=512, overlap=0, upsample="linear", first_tile=0, n_tiles=None):
    """cur, prev: two frames of one size in `fmt` (frames.py's tuples, any row strides, pitched differently or not) -> int64 cuda
    [n,3]: for the tiles first_tile .. first_tile + n - 1 of the row-major grid (default: all) and the planes [Y, Cb, Cr], the number
    of samples of the tile's footprint whose codes differ between cur and prev (pc_clips.h).  Exact; a tile's counts do not depend on
    the range it is part of.  A tile whose three counts are zero is cut to the same bits from either frame."""
    import torch
    _check_enums(fmt, upsample=upsample)
    ca, H, W = _one_frame(cur, fmt, "cur")
    pa, pH, pW = _one_frame(prev, fmt, "prev")
    if (pH, pW) != (H, W) or pa[0].device != ca[0].device:
        raise ValueError(f"prev must be a {H}x{W} frame on {ca[0].device}, got {pH}x{pW} on {pa[0].device}")
    g = _grid(H, W, tile, overlap)
    first, n = _tile_range(g, first_tile, n_tiles)
    dev = ca[0].device
    L = lib()
    with torch.cuda.device(dev):
        nbytes = L.pc_clips_changes_workspace_size(g.T, n)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        out = torch.empty((n, 3), dtype=torch.int64, device=dev)
        _changes_into(L, ca, pa, fmt, upsample, g, first, n, ws, nbytes, out, torch.cuda.current_stream(dev).cuda_stream)
    return out


def _clip_changes(fs, fmt, g, upsample, first, n):
    """clip_changes on checked arguments: fs[k] the planes of frame k as batched views"""
    import torch
    dev = fs[0][0].device
    L = lib()
    with torch.cuda.device(dev):
        out = torch.empty((len(fs) - 1, n, 3), dtype=torch.int64, device=dev)
        if len(fs) > 1:
            nbytes = L.pc_clips_changes_workspace_size(g.T, n)
            ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
            st = torch.cuda.current_stream(dev).cuda_stream
            for k in _range(1, len(fs)):
                _changes_into(L, fs[k], fs[k - 1], fmt, upsample, g, first, n, ws, nbytes, out[k - 1], st)
    return out


def clip_changes(frames, fmt, tile=512, overlap=0, upsample="linear", first_tile=0, n_tiles=None):
    """a clip of F frames -> int64 cuda [F - 1, n, 3]: entry k is tile_changes(frame k + 1, frame k, ...).  F - 1 launches into one
    tensor through one workspace (the launches are ordered on the stream), no host synchronisation."""
    _check_enums(fmt, upsample=upsample)
    fs, H, W = _clip_frames(frames, fmt)
    g = _grid(H, W, tile, overlap)
    first, n = _tile_range(g, first_tile, n_tiles)
    return _clip_changes(fs, fmt, g, upsample, first, n)


def _tile_indices(tile_indices, g):
    import torch
    idx = tile_indices.tolist() if torch.is_tensor(tile_indices) else list(tile_indices)
    if not idx:
        raise ValueError("tile_indices must name at least one tile")
    for v in idx:
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < g.ny * g.nx:
            raise ValueError(f"tile index {v!r} lies outside the {g.ny}x{g.nx} grid (row-major indices 0 .. {g.ny * g.nx - 1})")
    return idx


def _check_out(out, n, T, dev):
    import torch
    if not torch.is_tensor(out) or out.dtype != torch.float32:
        raise TypeError("out must be a float32 tensor")
    if tuple(out.shape) != (n, 3, T, T) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous [{n},3,{T},{T}] tensor (a slice of a larger batch buffer does), got "
                         f"{tuple(out.shape)} with strides {tuple(out.stride())}")
    if out.device != dev:
        raise ValueError(f"out must be on {dev}, got {out.device}")


def _cut_into(L, ts, fmt, range, upsample, k, g, idx_ptr, n, out, stream):
    src = _frame_struct(ts)
    rc = L.pc_clips_cut_list(C.byref(src), FORMATS[fmt], RANGES[range], UPSAMPLES[upsample], k.a, k.b, k.c, k.d, g.H, g.W, g.T, g.O, idx_ptr,
                             n, out.data_ptr(), stream)
    if rc != PC_OK:
        raise ClipsError(rc, "pc_clips_cut_list")


def cut_tiles(planes, fmt, tile_indices, matrix="bt709", range="limited", upsample="linear", tile=512, overlap=0, out=None):
    """frame + tile_indices (ints, row-major in the whole grid, any order, repeats allowed; validated here, on the host, before they
    are uploaded) -> float32 [n,3,T,T]: entry m is bit for bit frame_tiles.cut_frame(..., rect=(ty, tx, 1, 1)) of tile
    tile_indices[m].  One launch.  out: a contiguous float32 [n,3,T,T] tensor to fill instead (a slice of a larger batch buffer)."""
    import torch
    _check_enums(fmt, matrix, range, upsample)
    ts, H, W = _one_frame(planes, fmt, "planes")
    g = _grid(H, W, tile, overlap)
    idx = _tile_indices(tile_indices, g)
    dev = ts[0].device
    if out is not None:
        _check_out(out, len(idx), g.T, dev)
    k = coefficients(matrix)
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((len(idx), 3, g.T, g.T), dtype=torch.float32, device=dev)
        didx = torch.tensor(idx, dtype=torch.int32).to(dev)
        _cut_into(lib(), ts, fmt, range, upsample, k, g, didx.data_ptr(), len(idx), out, torch.cuda.current_stream(dev).cuda_stream)
    return out


def plan(op, planes, fmt, other=None, f32=None, overlap=0):
    """pc_clips_plan for tensors (host only, nothing is launched or copied): True where tile_changes (op = CHANGES: planes is cur,
    other is prev) or cut_tiles (op = CUT: planes the source frame, f32 the tile tensor) of exactly these tensors with this overlap
    takes the wide-access path.  planes and other are tuples of batched tensors ([1,...]) whose strides already fit a frame."""
    _check_enums(fmt)
    wide = C.c_int(-1)
    fr = _frame_struct(planes)
    ot = _frame_struct(other) if other is not None else None
    rc = lib().pc_clips_plan(op, FORMATS[fmt], C.byref(fr), C.byref(ot) if ot is not None else None,
                             f32.data_ptr() if f32 is not None else None, int(overlap), C.byref(wide))
    if rc != PC_OK:
        raise ClipsError(rc, "pc_clips_plan")
    return bool(wide.value)


# -- PCS1 ----------------------------------------------------------------------------------------------------------------------------

def source_table(changed):
    """changed[f - 1][t]: whether tile t differs between frames f - 1 and f (F - 1 rows) -> source[f][t] for F frames: 0 in frame 0,
    source[f - 1][t] where the tile did not change, else f"""
    n = len(changed[0]) if changed else 0
    source = [[0] * n]
    for f, row in enumerate(changed, 1):
        source.append([f if c else source[f - 1][t] for t, c in enumerate(row)])
    return source


def pack_clip(blobs, source, H, W, tile, overlap, fmt, matrix, range, upsample, contract=None):
    """blobs[f][t]: the PCB1 container of tile t of frame f where source[f][t] == f (anything else there is ignored); source[f][t]: the
    frame the tile was last coded in -- source[0][t] = 0, source[f][t] is f or source[f - 1][t] -> one PCS1 container."""
    from . import container
    _check_enums(fmt, matrix, range, upsample)
    g = grid_of(H, W, tile, overlap)
    F = _check_source(blobs, source, g)
    contract = container.build_contract_id() if contract is None else int(contract)
    head = MAGIC + struct.pack(_HEAD, VERSION, FORMATS[fmt], _MATRIX_ID[matrix], RANGES[range], UPSAMPLES[upsample], bits_of(fmt), contract,
                               g.H, g.W, g.T, g.O, g.ny, g.nx, F)
    return head + _table_and_payload(len(head), blobs, source)


def _check_source(blobs, source, g):
    """what pack_clip asks of blobs and source for the grid g -> the number of frames"""
    n, F = g.ny * g.nx, len(source)
    if F < 1 or F >= 1 << 32 or len(blobs) != F or any(len(r) != n for r in source) or any(len(r) != n for r in blobs):
        raise ContainerError(f"blobs and source must be [F][{n}] for the {g.ny}x{g.nx} grid, F >= 1")
    for f, row in enumerate(source):
        for t, s in enumerate(row):
            if s != f and (f == 0 or s != source[f - 1][t]):
                raise ContainerError(f"source[{f}][{t}] = {s!r}: a tile is coded in its own frame or repeats the frame before it")
    return F


def _table_and_payload(head_bytes, blobs, source):
    """the table and the payload behind a header of head_bytes bytes (PCS1's, or chroma_clips.py's PCL1): the coded tiles' blobs in
    (frame, tile) order, a reused tile repeating the entry of the frame it was last coded in"""
    F, n = len(source), len(source[0])
    off = head_bytes + ENTRY_BYTES * F * n
    entries, table, payload = [], [], []
    for f, row in enumerate(source):
        cur = []
        for t, s in enumerate(row):
            if s == f:
                b = bytes(blobs[f][t])
                cur.append((off, len(b)))
                payload.append(b)
                off += len(b)
            else:
                cur.append(entries[f - 1][t])
        entries.append(cur)
        table += [struct.pack("<QQ", *e) for e in cur]
    return b"".join(table) + b"".join(payload)


def _equal_or_disjoint(pairs, name):
    """two table entries of the container `name` are either equal or disjoint"""
    end = 0
    for off, ln in sorted(set(pairs)):
        if off < end:
            raise ContainerError(f"corrupt {name} table: the entry ({off}, {ln}) overlaps another without being equal to it")
        end = max(end, off + ln)


def _parse(buf, magic):
    """parse_clip for the container whose magic this is: PCS1, or clip_rate's PCS2, which differs in nothing else"""
    name = magic.decode()
    if len(buf) < 4 or bytes(buf[:4]) != magic:
        raise ContainerError(f"not a {name} container")
    if len(buf) < HEADER_BYTES:
        raise ContainerError(f"truncated {name} header")
    ver, f, m, r, u, bits, contract, H, W, T, O, ny, nx, F = struct.unpack_from(_HEAD, buf, 4)
    if ver != VERSION:
        raise ContainerError(f"unsupported {name} version {ver}")
    params = _tilecodec.frame_params(f, m, r, u, bits, name)
    g, pairs, start = _tilecodec.tile_table(buf, HEADER_BYTES, H, W, T, O, ny, nx, F, f"{name} header", "frame", f"{name} table")
    _equal_or_disjoint(pairs, name)
    n = ny * nx
    return dict(params, contract=contract, grid=g, F=F, table=[pairs[k * n:(k + 1) * n] for k in _range(F)], payload_start=start)


def parse_clip(buf):
    """-> dict(fmt, matrix, range, upsample, bits, contract, grid (TileGrid, whole grid), F, table [F][ny*nx] of (offset, length),
    payload_start).  Checks the header, the geometry against pc_tiles_grid, that the whole table is there and that two entries are
    either equal or disjoint; an entry is checked against the buffer when its tile is asked for (clip_tile_bytes), so that a clip cut
    off inside its payload still gives the frames it holds completely.  ContainerError for everything else."""
    return _parse(buf, MAGIC)


def _frame_index(hd, k):
    try:
        k = operator.index(k)
    except TypeError:
        raise ContainerError(f"a frame index is an integer, got {k!r}") from None
    if not 0 <= k < hd["F"]:
        raise ContainerError(f"no frame {k} among {hd['F']}")
    return k


def clip_tile_bytes(buf, hd, k, t, one_level=False):
    """The PCB1 container of tile t of frame k and its parsed header, after checking its table entry against the buffer and its
    header against the grid and the clip's contract; with one_level (PCS2, clip_rate.py) also that it holds exactly one level."""
    tb, th = _tilecodec.entry_bytes(buf, hd, hd["table"][k][t], f"frame {k}, tile {t}", "clip")
    if one_level and len(th["qualities"]) != 1:
        raise ContainerError(f"frame {k}, tile {t} holds {len(th['qualities'])} levels, a PCS2 tile holds exactly one")
    return tb, th


def frame_container(buf, k):
    """The PCG1 container of frame k of a PCS1 container: frame_tiles.pack_frame_tiled(tiles.pack_tiled(the blobs of frame k)), pure
    byte work -- what frame_tiles.encode_frame_tiled gives for that frame alone."""
    hd = parse_clip(buf)
    k = _frame_index(hd, k)
    g = hd["grid"]
    blobs = [clip_tile_bytes(buf, hd, k, t)[0] for t in _range(g.ny * g.nx)]
    return pack_frame_tiled(pack_tiled(blobs, g.H, g.W, g.T, g.O, contract=hd["contract"]), hd["fmt"], hd["matrix"], hd["range"], hd["upsample"])


# -- through the codec ---------------------------------------------------------------------------------------------------------------

def _frame_table(fs, dev):
    """the planes of every frame as batched views -> (the frame records in host memory, the same bytes on the device)"""
    import torch
    host = (Frame * len(fs))(*[_frame_struct(ts) for ts in fs])
    return host, torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev)


def _cut_of(fs, g, work, fmt, matrix, range, upsample):
    """-> cut(a, b) for _tilecodec.encode_items: the tiles work[a:a + b] -- (frame, tile) pairs in (frame, tile) order -- as one batch
    buffer, one cut launch per frame present in the chunk.  The tile list of the whole clip is uploaded once, here."""
    import torch
    k = coefficients(matrix)
    dev = fs[0][0].device
    L = lib()
    with torch.cuda.device(dev):
        didx = torch.tensor([t for _, t in work], dtype=torch.int32).to(dev)

    def cut(a, b):
        with torch.cuda.device(dev):
            x = torch.empty((b, 3, g.T, g.T), dtype=torch.float32, device=dev)
            st = torch.cuda.current_stream(dev).cuda_stream
            for f, m0, m1 in _tilecodec.frame_pieces(work[a:a + b]):
                _cut_into(L, fs[f], fmt, range, upsample, k, g, didx[a + m0:].data_ptr(), m1 - m0, x[m0:m1], st)
        return x
    return cut


def _source(fs, fmt, g, upsample, reuse):
    """the source table of a clip: with reuse, from one clip_changes and one device-to-host copy of its result"""
    n, F = g.ny * g.nx, len(fs)
    if reuse and F > 1:
        counts = _clip_changes(fs, fmt, g, upsample, 0, n).cpu()
        return source_table((counts != 0).any(dim=2).tolist())
    return [[f] * n for f in _range(F)]


def _encode_source(model, fs, g, source, qualities, fmt, matrix, range, upsample, mask_pol, step):
    """encode_clip once the source table is known (clip_tol.encode_clip comes here with its own): fs[k] the planes of frame k as
    batched views, everything checked -> (the PCS1 container, the number of coded tiles).  The work list -- every (f, t) with
    source[f][t] == f, in (f, t) order -- is chunked by `step` across frames (_tilecodec.encode_items over _cut_of's cut)."""
    n, F = g.ny * g.nx, len(fs)
    work = [(f, t) for f in _range(F) for t in _range(n) if source[f][t] == f]
    bufs = _tilecodec.encode_items(model, len(work), step, qualities, mask_pol, g.T, _cut_of(fs, g, work, fmt, matrix, range, upsample))
    blobs = [[None] * n for _ in _range(F)]
    for (f, t), b in zip(work, bufs):
        blobs[f][t] = b
    return pack_clip(blobs, source, g.H, g.W, g.T, g.O, fmt, matrix, range, upsample), len(work)


def encode_clip(model, frames, qualities, fmt, matrix="bt709", range="limited", upsample="linear", tile=512, overlap=0,
                mask_pol="point-based-std", reuse=True, max_tiles_per_call=32):
    """clip -> (PCS1 container (bytes), ClipPlan) holding every level of `qualities` for every tile of every frame.  With reuse, one
    clip_changes and one device-to-host copy of its result say which tiles changed: source[0][t] = 0, source[f][t] = source[f-1][t]
    where all three counts of (f-1, t) are zero, else f.  The work list -- every (f, t) with source[f][t] == f, in (f, t) order --
    is chunked by max_tiles_per_call ACROSS frames, so a codec call is filled even where a frame has few tiles to code: per chunk one
    cut launch per frame present in it into one batch buffer, then model.compress_levels, then container.pack per tile.
    reuse=False codes every tile (no change kernel, no aliasing).  The bytes depend neither on max_tiles_per_call nor on how the
    frames are laid out in memory; frame_container(buf, k) is frame_tiles.encode_frame_tiled of frame k."""
    qualities = [float(q) for q in qualities]
    _check_enums(fmt, matrix, range, upsample)
    step = _tilecodec.tiles_per_call(max_tiles_per_call)
    fs, H, W = _clip_frames(frames, fmt)
    g = _grid(H, W, tile, overlap)
    n, F = g.ny * g.nx, len(fs)
    source = _source(fs, fmt, g, upsample, reuse)
    buf, n_coded = _encode_source(model, fs, g, source, qualities, fmt, matrix, range, upsample, mask_pol, step)
    return buf, ClipPlan(source, n_coded, F * n - n_coded, len(buf))


def _decode(model, buf, hd, one_level, frames, level, region, fmt, step, stitch, window_of=None, covering_of=None):
    """decode_clip on a parsed header: of a PCS1 container (one level of tiles that hold several), or with one_level of a PCS2
    container (clip_rate.decode_clip: the one level every tile holds; tiles may differ in quality).  All byte work comes first, and
    every refusal is a ContainerError raised before the model is touched.  stitch is the caller's stitch_frame.  The two hooks are
    for a caller whose formats have another window rule (chroma_clips.py, which has checked its output format itself):
    window_of(region, H, W, out_fmt) -> the admissible window or ValueError, covering_of(grid, window, out_fmt) -> the rectangle of
    tiles to read; by default the 4:2:0 check and the tiles that cover the window."""
    out_fmt = hd["fmt"] if fmt is None else fmt
    if window_of is None:
        _check_enums(out_fmt)
    g = hd["grid"]
    try:
        window = _admissible_window(region, g.H, g.W) if window_of is None else window_of(region, g.H, g.W, out_fmt)
    except ValueError as e:
        raise ContainerError(str(e)) from None
    try:
        wanted = list(_range(hd["F"])) if frames is None else [_frame_index(hd, k) for k in frames]
    except TypeError:
        raise ContainerError(f"frames must be an iterable of frame indices, got {frames!r}") from None
    g = g.with_rect(g.covering(window) if covering_of is None else covering_of(g, window, out_fmt))
    need = [(g.ty0 + a) * g.nx + g.tx0 + b for a in _range(g.nty) for b in _range(g.ntx)]
    # per requested frame the tiles it takes from the frame handled just before it and, of the rest, the strings by quality (one
    # quality where the tiles hold several levels: it is part of what they must share).  Under one_level, what a frame's tiles
    # must share is carried along with a reused tile, so that a frame is refused exactly where decode_frame_tiled of its own
    # container is; otherwise the fresh tiles are held to each other only
    todo, prev_entries, prev_keys = [], None, None
    for k in wanted:
        entries = [hd["table"][k][t] for t in need]
        keys, groups, strings_of, first, shared = [None] * len(need), {}, {}, None, (None, None)
        for p, t in enumerate(need):
            if prev_entries is not None and entries[p] == prev_entries[p]:
                if not one_level:
                    continue
                keys[p] = prev_keys[p]
            else:
                tb, th = clip_tile_bytes(buf, hd, k, t, one_level)
                shape, q, mask_pol, strings = _tilecodec.level_strings(tb, th, 0 if one_level else level, f"frame {k}, tile {t}: ")
                keys[p] = (shape, mask_pol) if one_level else (shape, q, mask_pol, len(strings[0]))
                strings_of[p], shared = strings, (shape, mask_pol)
                groups.setdefault(q, []).append(p)
            if first is None:
                first = p
            _tilecodec.same_coding(keys[p], keys[first], f"frame {k}, tile {t}", f"tile {need[first]}")
        todo.append((sorted(groups.items()), strings_of, shared))
        prev_entries, prev_keys = entries, keys
    if todo:
        _tilecodec.check_contract(hd["contract"])
    out, prev = [], None
    for groups, strings_of, shared in todo:
        prev = _tilecodec.decode_positions(model, strings_of, groups, *shared, step, len(need), prev)
        out.append(stitch(prev, g, out_fmt, hd["matrix"], hd["range"], window=window))
    return out


def decode_clip(model, buf, frames=None, level=-1, region=None, fmt=None, max_tiles_per_call=32):
    """One level of the frames `frames` (an iterable of indices, default all of them, in the order given) of a PCS1 container -> a list
    of frames (tuples of planes without a batch axis) on the model's device, or of their admissible region = (y0, x0, h, w), in the
    stored format or in `fmt` (as frame_tiles.decode_frame_tiled).  Only the tiles that cover the region are read.  Among consecutive
    requested frames a byte range is decoded once: a tile whose table entry equals that of the frame handled just before reuses that
    frame's decoded float tile; the rest are decoded max_tiles_per_call at a time.  Device memory is bounded by two frames' tile sets
    plus one call.  Every refusal is a ContainerError raised before the model is touched.  Frame k is bit for bit
    frame_tiles.decode_frame_tiled(model, frame_container(buf, k), ...)."""
    step = _tilecodec.tiles_per_call(max_tiles_per_call)
    return _decode(model, buf, parse_clip(buf), False, frames, level, region, fmt, step, stitch_frame)

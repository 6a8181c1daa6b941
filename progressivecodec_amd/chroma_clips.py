"""Clips of YUV frames of any chroma subsampling and siting (libpc_chroma_clips.so, chroma_clips_kernels/pc_chroma_clips.h; DESIGN.md
section 25): what `clips` is for NV12 / I420 / P010 with centre-sited chroma, for the twelve formats and three sitings of `chroma`.
A sequence of frames is coded tile by tile as chroma_tiles.py codes one frame, with two differences: the tiles of several frames share
a codec call, and a tile whose samples did not change since the previous frame is neither cut, coded nor stored again -- its table
entry points at the bytes of the frame it was last coded in.  No inter-frame prediction, no drift, no decode dependency: every frame
of the clip is what chroma_tiles.encode_frame_tiled / decode_frame_tiled give for that frame alone, byte for byte and bit for bit.

  tile_changes     two frames -> per tile and plane the number of samples of the tile's footprint whose codes differ, exact, on the GPU
  clip_changes     a clip -> the same for every frame against the one before it, F - 1 launch pairs and no host synchronisation
  cut_tiles        frame + a list of tile indices -> float32 tiles [n,3,T,T], one launch (chroma_tiles.cut_frame takes rectangles only)
  encode_clip      clip -> (one PCL1 container, ClipPlan): static tiles coded once, the work list chunked across frames
  decode_clip      PCL1 container -> a list of frames (or of one region of each); among consecutive frames a byte range is decoded once
  frame_container  PCL1 container, k -> the PCK1 container of frame k (pure byte work)

Footprint of a tile (the contract, pc_chroma_clips.h).  Geometry is tiles.py's: T, O, S = T - O, the ny x nx grid.  Along an axis of
length L, with e = min(i*S + T, L), tile i reads luma positions [i*S, e) and chroma positions
  [i*S, e - 1]                                             where the axis is not subsampled, whatever the siting and upsampling;
  [max(i*S/2 - lo, 0), min(ceil(e/2) - 1 + hi, Lc - 1)]    where it is, with Lc = ceil(L / 2), hi = 1 for upsample = "linear" (else 0)
                                                           and lo = 1 for "linear" AND centre siting on that axis (else 0):
the co-sited rule gives an even luma index one tap and an odd one the sample after it, so it never reaches below i*S/2 -- under
"left" a tile reads no chroma column left of its first one.  The footprint of tile (i, j) is the product of the two axes' ranges, once
in the luma plane and once each in Cb and Cr.  Codes are (element >> shift) & (2^bits - 1): two frames that differ only in a word's
other bits are equal.  If every code in the footprint is the same in two frames, the cut of the tile is the same bits, and so are its
PCB1 bytes.  The footprint is tight as well: it is exactly the set of samples the cut reads with a non-zero weight.  For "nv12",
"i420" and "p010" at "centre" it is clips.py's.

A clip is a list of frames (chroma.py's tuples) of one size on one device, or one tuple of batched planes ([F,H,W] and so on), taken
frame by frame through their batch stride without a copy.

PCL1 layout (little endian): magic "PCL1", version u8 (= 1), then PCK1's ten bytes -- layout, shift, sx, sy, horizontal siting,
vertical siting, matrix, range, upsample, bits --, the numeric contract id u32, H, W, T, O, ny, nx, F as u32 each -- 47 bytes; then
PCS1's table of F*ny*nx entries (offset u64, length u64) from the container's start, frame by frame and row-major within a frame; then
the PCB1 containers of the CODED tiles in (frame, tile) order.  The entry of a reused tile repeats the entry of the frame it was last
coded in: two entries are either equal or disjoint, anything else is refused.  An entry is checked against the buffer when its tile
is asked for, so a clip cut off inside its payload still gives every frame whose tiles it holds completely.

There is no CPU fallback: CPU tensors raise ValueError before any device call.  Everything runs on the current stream of the tensors'
device.  Rate control over a clip is the layer above this one (chroma_clip_rate.py, DESIGN.md section 28: what clip_rate.py is to
clips.py).  A tolerance for near-static tiles is the other layer above this one (chroma_clip_tol.py, DESIGN.md section 29: what
clip_tol.py is to clips.py).  Out of scope: a tolerance under a byte budget (what clip_tol_rate.py is to clips.py), any inter-frame
prediction.
"""
import ctypes as C
import struct

from . import _imagelib, _tilecodec, clips
from ._lib import PC_OK
from .chroma import FORMATS, SITINGS, _MATRIX_ID, _check_enums, _frame_view, _inv  # noqa: F401
from .chroma_tiles import _admissible_window, _one_frame, covering, pack_frame_tiled, stitch_frame
from .clips import ClipPlan, source_table
from .container import ContainerError
from .frames import RANGES, UPSAMPLES, Frame, _frame_struct, coefficients
from .tiles import grid_of, pack_tiled

LIB_PATH = _imagelib.lib_path("chroma_clips")

#: every symbol chroma_clips_kernels/pc_chroma_clips.h declares
EXPORTS = ["pc_chroma_clips_changes_workspace_size", "pc_chroma_clips_tile_changes", "pc_chroma_clips_cut_list", "pc_chroma_clips_plan",
           "pc_chroma_clips_strerror", "pc_chroma_clips_last_hip_error"]

CHANGES, CUT = 0, 1                       # pc_chroma_clips_plan's `op`
MAX_TILE = 2048                           # pc_chroma_clips.h

MAGIC = b"PCL1"
VERSION = 1
_HEAD = "<BBBBBBBBBBBIIIIIIII"            # version, PCK1's ten bytes, contract id, H, W, T, O, ny, nx, F
HEADER_BYTES = 4 + struct.calcsize(_HEAD)

_range = range                            # the functions below take a parameter of that name


def _prototypes():
    vp, ci, cf, fp = C.c_void_p, C.c_int, C.c_float, C.POINTER(Frame)
    return {
        "pc_chroma_clips_changes_workspace_size": (C.c_size_t, [ci, ci, ci]),
        "pc_chroma_clips_tile_changes": (None, [fp, fp] + [ci] * 14 + [vp, C.c_size_t, vp, vp]),
        "pc_chroma_clips_cut_list": (None, [fp] + [ci] * 9 + [cf] * 4 + [ci] * 4 + [vp, ci, vp, vp]),
        "pc_chroma_clips_plan": (None, [ci, ci, ci, ci, fp, fp, vp, ci, C.POINTER(ci)]),
        "pc_chroma_clips_strerror": (C.c_char_p, [ci]),
    }


def lib():
    return _imagelib.load(LIB_PATH, _prototypes)


class ChromaClipsError(_imagelib.ImageLibError):
    _lib, _prefix = staticmethod(lib), "pc_chroma_clips"


def _grid(H, W, tile, overlap):
    g = grid_of(H, W, tile, overlap)
    if g.T > MAX_TILE:
        raise ValueError(f"tile must be at most {MAX_TILE}, got {g.T}")
    return g


def _clip_frames(frames, fmt):
    return clips._clip_frames(frames, fmt, view=_frame_view, one=_one_frame)


def _changes_into(L, cur, prev, fmt, siting, upsample, g, first, n, ws, nbytes, out, stream):
    a, b = _frame_struct(cur), _frame_struct(prev)
    rc = L.pc_chroma_clips_tile_changes(C.byref(a), C.byref(b), *FORMATS[fmt], *SITINGS[siting], UPSAMPLES[upsample], g.H, g.W, g.T, g.O,
                                        first, n, ws.data_ptr(), nbytes, out.data_ptr(), stream)
    if rc != PC_OK:
        raise ChromaClipsError(rc, "pc_chroma_clips_tile_changes")


def tile_changes(cur, prev, fmt, siting="centre", tile=512, overlap=0, upsample="linear", first_tile=0, n_tiles=None):
    """cur, prev: two frames of one size in `fmt` (chroma.py's tuples, any row strides, pitched differently or not) -> int64 cuda
    [n,3]: for the tiles first_tile .. first_tile + n - 1 of the row-major grid (default: all) and the planes [Y, Cb, Cr], the number
    of samples of the tile's footprint under `siting` and `upsample` whose codes differ between cur and prev (pc_chroma_clips.h).
    Exact; a tile's counts do not depend on the range it is part of.  A tile whose three counts are zero is cut to the same bits from
    either frame."""
    import torch
    _check_enums(fmt, upsample=upsample, siting=siting)
    ca, H, W = _one_frame(cur, fmt, "cur")
    pa, pH, pW = _one_frame(prev, fmt, "prev")
    if (pH, pW) != (H, W) or pa[0].device != ca[0].device:
        raise ValueError(f"prev must be a {H}x{W} frame on {ca[0].device}, got {pH}x{pW} on {pa[0].device}")
    g = _grid(H, W, tile, overlap)
    first, n = clips._tile_range(g, first_tile, n_tiles)
    dev = ca[0].device
    L = lib()
    with torch.cuda.device(dev):
        nbytes = L.pc_chroma_clips_changes_workspace_size(g.T, FORMATS[fmt].sy, n)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        out = torch.empty((n, 3), dtype=torch.int64, device=dev)
        _changes_into(L, ca, pa, fmt, siting, upsample, g, first, n, ws, nbytes, out, torch.cuda.current_stream(dev).cuda_stream)
    return out


def _clip_changes(fs, fmt, siting, g, upsample, first, n):
    """clip_changes on checked arguments: fs[k] the planes of frame k as batched views"""
    import torch
    dev = fs[0][0].device
    L = lib()
    with torch.cuda.device(dev):
        out = torch.empty((len(fs) - 1, n, 3), dtype=torch.int64, device=dev)
        if len(fs) > 1:
            nbytes = L.pc_chroma_clips_changes_workspace_size(g.T, FORMATS[fmt].sy, n)
            ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
            st = torch.cuda.current_stream(dev).cuda_stream
            for k in _range(1, len(fs)):
                _changes_into(L, fs[k], fs[k - 1], fmt, siting, upsample, g, first, n, ws, nbytes, out[k - 1], st)
    return out


def clip_changes(frames, fmt, siting="centre", tile=512, overlap=0, upsample="linear", first_tile=0, n_tiles=None):
    """a clip of F frames -> int64 cuda [F - 1, n, 3]: entry k is tile_changes(frame k + 1, frame k, ...).  F - 1 launch pairs into
    one tensor through one workspace (the launches are ordered on the stream), no host synchronisation."""
    _check_enums(fmt, upsample=upsample, siting=siting)
    fs, H, W = _clip_frames(frames, fmt)
    g = _grid(H, W, tile, overlap)
    first, n = clips._tile_range(g, first_tile, n_tiles)
    return _clip_changes(fs, fmt, siting, g, upsample, first, n)


def _cut_into(L, ts, fmt, range, upsample, siting, k, g, idx_ptr, n, out, stream):
    src = _frame_struct(ts)
    rc = L.pc_chroma_clips_cut_list(C.byref(src), *FORMATS[fmt], *SITINGS[siting], RANGES[range], UPSAMPLES[upsample], k.a, k.b, k.c, k.d,
                                    g.H, g.W, g.T, g.O, idx_ptr, n, out.data_ptr(), stream)
    if rc != PC_OK:
        raise ChromaClipsError(rc, "pc_chroma_clips_cut_list")


def cut_tiles(planes, fmt, tile_indices, matrix="bt709", range="limited", upsample="linear", siting="centre", tile=512, overlap=0, out=None):
    """frame + tile_indices (ints, row-major in the whole grid, any order, repeats allowed; validated here, on the host, before they
    are uploaded) -> float32 [n,3,T,T]: entry m is bit for bit chroma_tiles.cut_frame(..., rect=(ty, tx, 1, 1))[0] of tile
    tile_indices[m].  One launch.  out: a contiguous float32 [n,3,T,T] tensor to fill instead (a slice of a larger batch buffer)."""
    import torch
    _check_enums(fmt, matrix, range, upsample, siting)
    ts, H, W = _one_frame(planes, fmt, "planes")
    g = _grid(H, W, tile, overlap)
    idx = clips._tile_indices(tile_indices, g)
    dev = ts[0].device
    if out is not None:
        clips._check_out(out, len(idx), g.T, dev)
    k = coefficients(matrix)
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((len(idx), 3, g.T, g.T), dtype=torch.float32, device=dev)
        didx = torch.tensor(idx, dtype=torch.int32).to(dev)
        _cut_into(lib(), ts, fmt, range, upsample, siting, k, g, didx.data_ptr(), len(idx), out, torch.cuda.current_stream(dev).cuda_stream)
    return out


def plan(op, planes, fmt, other=None, f32=None, overlap=0):
    """pc_chroma_clips_plan for tensors (host only, nothing is launched or copied): True where tile_changes (op = CHANGES: planes is
    cur, other is prev) or cut_tiles (op = CUT: planes the source frame, f32 the tile tensor) of exactly these tensors with this
    overlap takes the wide-access path.  planes and other are tuples of batched tensors ([1,...]) whose strides already fit a frame."""
    _check_enums(fmt)
    f = FORMATS[fmt]
    wide = C.c_int(-1)
    fr = _frame_struct(planes)
    ot = _frame_struct(other) if other is not None else None
    rc = lib().pc_chroma_clips_plan(op, f.layout, f.bits, f.sx, C.byref(fr), C.byref(ot) if ot is not None else None,
                                    f32.data_ptr() if f32 is not None else None, int(overlap), C.byref(wide))
    if rc != PC_OK:
        raise ChromaClipsError(rc, "pc_chroma_clips_plan")
    return bool(wide.value)


# -- PCL1 ----------------------------------------------------------------------------------------------------------------------------

def pack_clip(blobs, source, H, W, tile, overlap, fmt, matrix, range, upsample, siting, contract=None):
    """blobs[f][t]: the PCB1 container of tile t of frame f where source[f][t] == f (anything else there is ignored); source[f][t]: the
    frame the tile was last coded in -- source[0][t] = 0, source[f][t] is f or source[f - 1][t] -> one PCL1 container."""
    from . import container
    _check_enums(fmt, matrix, range, upsample, siting)
    g = grid_of(H, W, tile, overlap)
    F = clips._check_source(blobs, source, g)
    contract = container.build_contract_id() if contract is None else int(contract)
    head = MAGIC + struct.pack(_HEAD, VERSION, *_tilecodec.sited_head(fmt, matrix, range, upsample, siting), contract, g.H, g.W, g.T, g.O,
                               g.ny, g.nx, F)
    return head + clips._table_and_payload(len(head), blobs, source)


def _parse(buf, magic):
    """parse_clip for the container whose magic this is: PCL1 (a later container that differs in its magic alone comes here, too)"""
    name = magic.decode()
    if len(buf) < 4 or bytes(buf[:4]) != magic:
        raise ContainerError(f"not a {name} container")
    if len(buf) < HEADER_BYTES:
        raise ContainerError(f"truncated {name} header")
    ver, *sited, contract, H, W, T, O, ny, nx, F = struct.unpack_from(_HEAD, buf, 4)
    if ver != VERSION:
        raise ContainerError(f"unsupported {name} version {ver}")
    params = _tilecodec.sited_params(*sited, name)
    g, pairs, start = _tilecodec.tile_table(buf, HEADER_BYTES, H, W, T, O, ny, nx, F, f"{name} header", "frame", f"{name} table")
    clips._equal_or_disjoint(pairs, name)
    n = ny * nx
    return dict(params, contract=contract, grid=g, F=F, table=[pairs[k * n:(k + 1) * n] for k in _range(F)], payload_start=start)


def parse_clip(buf):
    """-> dict(fmt, siting, matrix, range, upsample, bits, contract, grid (TileGrid, whole grid), F, table [F][ny*nx] of (offset,
    length), payload_start).  Checks the header, the geometry against pc_tiles_grid, that the whole table is there and that two
    entries are either equal or disjoint; an entry is checked against the buffer when its tile is asked for (clip_tile_bytes), so
    that a clip cut off inside its payload still gives the frames it holds completely.  ContainerError for everything else."""
    return _parse(buf, MAGIC)


def clip_tile_bytes(buf, hd, k, t):
    """The PCB1 container of tile t of frame k and its parsed header, after checking its table entry against the buffer and its
    header against the grid and the clip's contract."""
    return clips.clip_tile_bytes(buf, hd, k, t)


def frame_container(buf, k):
    """The PCK1 container of frame k of a PCL1 container: chroma_tiles.pack_frame_tiled(tiles.pack_tiled(the blobs of frame k)), pure
    byte work -- what chroma_tiles.encode_frame_tiled gives for that frame alone."""
    hd = parse_clip(buf)
    k = clips._frame_index(hd, k)
    g = hd["grid"]
    blobs = [clip_tile_bytes(buf, hd, k, t)[0] for t in _range(g.ny * g.nx)]
    return pack_frame_tiled(pack_tiled(blobs, g.H, g.W, g.T, g.O, contract=hd["contract"]), hd["fmt"], hd["matrix"], hd["range"],
                            hd["upsample"], hd["siting"])


# -- through the codec ---------------------------------------------------------------------------------------------------------------

def _cut_of(fs, g, work, fmt, matrix, range, upsample, siting):
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
                _cut_into(L, fs[f], fmt, range, upsample, siting, k, g, didx[a + m0:].data_ptr(), m1 - m0, x[m0:m1], st)
        return x
    return cut


def _source(fs, fmt, siting, g, upsample, reuse):
    """the source table of a clip: with reuse, from one clip_changes and one device-to-host copy of its result"""
    n, F = g.ny * g.nx, len(fs)
    if reuse and F > 1:
        counts = _clip_changes(fs, fmt, siting, g, upsample, 0, n).cpu()
        return source_table((counts != 0).any(dim=2).tolist())
    return [[f] * n for f in _range(F)]


def _encode_source(model, fs, g, source, qualities, fmt, matrix, range, upsample, siting, mask_pol, step):
    """encode_clip once the source table is known (chroma_clip_tol.encode_clip comes here with its own): fs[k] the planes of frame k as
    batched views, everything checked -> (the PCL1 container, the number of coded tiles).  The work list -- every (f, t) with
    source[f][t] == f, in (f, t) order -- is chunked by `step` across frames (_tilecodec.encode_items over _cut_of's cut)."""
    n, F = g.ny * g.nx, len(fs)
    work = [(f, t) for f in _range(F) for t in _range(n) if source[f][t] == f]
    bufs = _tilecodec.encode_items(model, len(work), step, qualities, mask_pol, g.T, _cut_of(fs, g, work, fmt, matrix, range, upsample, siting))
    blobs = [[None] * n for _ in _range(F)]
    for (f, t), b in zip(work, bufs):
        blobs[f][t] = b
    return pack_clip(blobs, source, g.H, g.W, g.T, g.O, fmt, matrix, range, upsample, siting), len(work)


def encode_clip(model, frames, qualities, fmt, matrix="bt709", range="limited", upsample="linear", siting="centre", tile=512, overlap=0,
                mask_pol="point-based-std", reuse=True, max_tiles_per_call=32):
    """clip -> (PCL1 container (bytes), ClipPlan) holding every level of `qualities` for every tile of every frame.  With reuse, one
    clip_changes and one device-to-host copy of its result say which tiles changed: source[0][t] = 0, source[f][t] = source[f-1][t]
    where all three counts of (f-1, t) are zero, else f.  The work list -- every (f, t) with source[f][t] == f, in (f, t) order --
    is chunked by max_tiles_per_call ACROSS frames, so a codec call is filled even where a frame has few tiles to code: per chunk one
    cut launch per frame present in it into one batch buffer, then model.compress_levels, then container.pack per tile.
    reuse=False codes every tile (no change kernel, no aliasing).  The bytes depend neither on max_tiles_per_call nor on how the
    frames are laid out in memory; frame_container(buf, k) is chroma_tiles.encode_frame_tiled of frame k."""
    qualities = [float(q) for q in qualities]
    _check_enums(fmt, matrix, range, upsample, siting)
    step = _tilecodec.tiles_per_call(max_tiles_per_call)
    fs, H, W = _clip_frames(frames, fmt)
    g = _grid(H, W, tile, overlap)
    n, F = g.ny * g.nx, len(fs)
    source = _source(fs, fmt, siting, g, upsample, reuse)
    buf, n_coded = _encode_source(model, fs, g, source, qualities, fmt, matrix, range, upsample, siting, mask_pol, step)
    return buf, ClipPlan(source, n_coded, F * n - n_coded, len(buf))


def decode_clip(model, buf, frames=None, level=-1, region=None, fmt=None, siting=None, max_tiles_per_call=32):
    """One level of the frames `frames` (an iterable of indices, default all of them, in the order given) of a PCL1 container -> a list
    of frames (tuples of planes without a batch axis) on the model's device, or of their admissible region = (y0, x0, h, w), in the
    stored format and siting or in `fmt` / `siting` (as chroma_tiles.decode_frame_tiled).  Admissibility and the halo are those of the
    OUTPUT format and siting; the tiles read are covering(halo_window(region)).  Among consecutive requested frames a byte range is
    decoded once: a tile whose table entry equals that of the frame handled just before reuses that frame's decoded float tile; the
    rest are decoded max_tiles_per_call at a time.  Every refusal is a ContainerError raised before the model is touched.  Frame k is
    bit for bit chroma_tiles.decode_frame_tiled(model, frame_container(buf, k), ...).  The loop is clips.py's."""
    step = _tilecodec.tiles_per_call(max_tiles_per_call)
    hd = parse_clip(buf)
    out_siting = hd["siting"] if siting is None else siting
    _check_enums(hd["fmt"] if fmt is None else fmt, siting=out_siting)

    def stitch(x, g, out_fmt, matrix, range, window):
        return stitch_frame(x, g, out_fmt, matrix, range, out_siting, window=window)
    return clips._decode(model, buf, hd, False, frames, level, region, fmt, step, stitch,
                         window_of=lambda region, H, W, out_fmt: _admissible_window(region, H, W, out_fmt),
                         covering_of=lambda g, window, out_fmt: covering(g, window, out_fmt, out_siting))

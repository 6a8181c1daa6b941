"""Rate-controlled clips of YUV frames of any chroma subsampling and siting (libpc_chroma_clip_rate.so,
chroma_clip_rate_kernels/pc_chroma_clip_rate.h): what `clip_rate` is for NV12 / I420 / P010 with centre-sited
chroma, for the twelve formats and three sitings of `chroma`.  One clip in at most N bytes.  The composition of chroma_rate.py
(section 24: one frame in at most N bytes, every tile at the level rate.allocate picks for it) and chroma_clips.py (section 25: static
tiles coded once): a coded tile that is shown in m frames is ONE item of the allocation, stored once, and its distortion counts m
times.  No body is restated here: the loops are _tilecodec's, the items, weights, checks and the allocation clip_rate's, the source
table, the cut and the stitch chroma_clips', the container bytes chroma_clips' and chroma_tiles'.

  tile_distortion_jobs   decoded tiles + a clip + a list of (frame, tile) jobs -> the exact integer weighted squared error per job and
                         plane, one launch pair for jobs scattered over any number of frames (chroma_rate.frame_tile_distortion takes
                         a linear range of tiles of one frame)
  encode_clip_to_size    clip -> (PCL2 container of at most target_bytes bytes, ChromaClipRatePlan)
  decode_clip            PCL2 container -> a list of frames (or of one region of each); PCL1 goes to chroma_clips.decode_clip
  frame_container        PCL2 container, k -> the PCK1 container of frame k holding a PCT2 one (pure byte work)

The reuse identity.  pc_chroma_rate_tile_sse of tile (i, j) reads, of the original frame, per axis the luma positions [i*S, e),
e = min(i*S + T, L), and the chroma samples (i*S/sy + k, j*S/sx + m) with k < ceil(hh/sy), m < ceil(ww/sx) -- the tile's chroma cells
WITHOUT any halo, whatever the siting: the co-sited filter works on the decoded tile, never on the original.  Section 25 calls a tile
unchanged between two frames only where every code of its footprint is equal, and on every axis, for every siting and upsampling,
the footprint [max(i*S/2 - lo, 0), min(ceil(e/2) - 1 + hi, Lc - 1)] (or [i*S, e - 1] on an axis that is not subsampled) contains
[i*S/2, ceil(e/2) - 1] (or [i*S, e - 1]).  The decoded tile is the same bits, too (the same bytes are decoded).  So for an item (f, t)
shown in frames f .. f + m - 1, D(f + j, t) = D(f, t) exactly, the item's total distortion over the clip is m * D(f, t), and its
weight in the allocation is m (times importance and frame weights).

Budget.  The header (47 bytes) and the table (16 bytes per frame and tile, reused or not) do not depend on the levels, so the
allocator gets target_bytes - 47 - 16 * F * ny * nx, and rates[i][l] is the length of item i's single-level PCB1 container alone.

PCL2 is PCL1 (chroma_clips.py: the 47-byte header, PCS1's table and payload rules) with the magic "PCL2" and every coded tile's PCB1
container holding EXACTLY ONE level; tiles may differ in quality.  What PCS2 is to PCS1.

There is no CPU fallback: CPU tensors raise ValueError before any device call.  Everything runs on the current stream of the tensors'
device.  A tolerance for near-static tiles under the same budget is the layer above this one (chroma_clip_tol_rate.py, DESIGN.md
section 30: what clip_tol_rate.py is to clip_rate.py).  Out of scope: measuring all levels of a chunk in one launch, per-frame byte
caps, a target PSNR, inter-frame prediction.
"""
import collections
import ctypes as C

from . import _imagelib, _tilecodec, chroma_clips, chroma_rate, clip_rate, clips
from ._lib import PC_OK
from ._tilecodec import max_tile  # noqa: F401
from .chroma import FORMATS, SITINGS, _check_enums
from .chroma_clips import HEADER_BYTES, _clip_frames, _cut_of, _grid, _source
from .chroma_tiles import _admissible_window, covering, pack_frame_tiled, stitch_frame
from .clip_rate import ClipRatePlan, item_weights, items_of
from .clips import ENTRY_BYTES, _frame_table  # noqa: F401
from .frames import RANGES, Frame, _frame_struct, coefficients
from .tiles import TileGrid, _check_tiles, _fit_tiles, grid_of, pack_tiled

LIB_PATH = _imagelib.lib_path("chroma_clip_rate")

#: every symbol chroma_clip_rate_kernels/pc_chroma_clip_rate.h declares
EXPORTS = ["pc_chroma_clip_rate_workspace_size", "pc_chroma_clip_rate_sse_jobs", "pc_chroma_clip_rate_plan", "pc_chroma_clip_rate_strerror",
           "pc_chroma_clip_rate_last_hip_error"]

MAGIC = b"PCL2"
VERSION = 1

_range = range                            # the functions below take a parameter of that name


def _prototypes():
    i64, vp, ci, cf, fp = C.c_int64, C.c_void_p, C.c_int, C.c_float, C.POINTER(Frame)
    return {
        "pc_chroma_clip_rate_workspace_size": (C.c_size_t, [ci, ci, ci]),
        "pc_chroma_clip_rate_sse_jobs": (None, [vp, i64, i64, i64] + [ci] * 12 + [cf] * 5 + [fp, vp, ci, vp, ci, vp, C.c_size_t, vp, vp]),
        "pc_chroma_clip_rate_plan": (None, [vp, i64, i64, i64, ci, ci, ci, ci, fp, ci, C.POINTER(ci)]),
        "pc_chroma_clip_rate_strerror": (C.c_char_p, [ci]),
    }


def lib():
    return _imagelib.load(LIB_PATH, _prototypes)


class ChromaClipRateError(_imagelib.ImageLibError):
    _lib, _prefix = staticmethod(lib), "pc_chroma_clip_rate"


#: what encode_clip_to_size decided: clip_rate.ClipRatePlan's fields -- source, items, weights, levels, rates, dists, plane_dists
#: (tile_distortion_jobs, in the frame the item was coded for), den, container_bytes, predicted, sse[k][p], n_coded, n_reused -- and
#: sse_exact (chroma_rate.sse_exact of the grid, the format and the siting): where it holds, sse[k][p] is the decoded frame's exact
#: per-plane SSE; sse[k][0] is that at overlap 0 whatever the siting
ChromaClipRatePlan = collections.namedtuple("ChromaClipRatePlan", ClipRatePlan._fields + ("sse_exact",))


# -- the kernel ----------------------------------------------------------------------------------------------------------------------

def _sse_jobs_into(L, x, g, fmt, siting, range, k, host, table, F, jobs_ptr, n, ws, nbytes, out, stream):
    rc = L.pc_chroma_clip_rate_sse_jobs(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), g.H, g.W, g.T, g.O, *FORMATS[fmt], *SITINGS[siting],
                                        RANGES[range], k.kr, k.kg, k.kb, k.ib, k.ir, host, table.data_ptr(), F, jobs_ptr, n, ws.data_ptr(),
                                        nbytes, out.data_ptr(), stream)
    if rc != PC_OK:
        raise ChromaClipRateError(rc, "pc_chroma_clip_rate_sse_jobs")


def tile_distortion_jobs(x_hat_tiles, grid, frames, jobs, fmt, matrix="bt709", range="limited", siting="centre"):
    """x_hat_tiles: float32 cuda [n,3,T,T] (any tile / channel / row strides, unit stride along a row); frames: a clip (a list of
    frames of grid's H x W in `fmt`, or one tuple of batched planes, any row strides) whose chroma is sited as `siting` says; jobs: n
    (frame, tile) pairs of ints, the tile row-major in grid's whole ny x nx grid, in any order, repeats allowed (validated here, on the
    host, before they are uploaded, with clip_rate's texts) -> int64 cuda [n,3]: row m is chroma_rate.frame_tile_distortion(
    x_hat_tiles[m:m+1], grid, frames[f], ..., first_tile=t) for jobs[m] = (f, t), exactly (pc_chroma_clip_rate.h).  One launch pair
    whatever the number of frames the jobs name."""
    import torch
    _check_enums(fmt, matrix, range, siting=siting)
    g = TileGrid(*grid)
    full = grid_of(g.H, g.W, g.T, g.O)
    if (full.ny, full.nx) != (g.ny, g.nx):
        raise ValueError(f"{g}: the grid of a {g.H}x{g.W} frame is {full.ny}x{full.nx}")
    _tilecodec.tile_limit(g.T, fmt)
    fs, H, W = _clip_frames(frames, fmt)
    rows = clip_rate._jobs(jobs, len(fs), full)
    x = x_hat_tiles
    n = len(rows)
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[0] != n:
        raise ValueError(f"x_hat_tiles must be a [{n},3,{g.T},{g.T}] tensor, one tile per job")
    _check_tiles(x, full._replace(nty=1, ntx=n))
    dev = fs[0][0].device
    if (H, W) != (g.H, g.W) or x.device != dev:
        raise ValueError(f"frames must be {g.H}x{g.W} frames on {x.device}, got {H}x{W} on {dev}")
    x = _fit_tiles(x, g.T)
    k = coefficients(matrix)
    L = lib()
    with torch.cuda.device(dev):
        host, table = _frame_table(fs, dev)
        djobs = torch.tensor(rows, dtype=torch.int32).to(dev)
        nbytes = L.pc_chroma_clip_rate_workspace_size(g.T, FORMATS[fmt].sy, n)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        out = torch.empty((n, 3), dtype=torch.int64, device=dev)
        _sse_jobs_into(L, x, full, fmt, siting, range, k, host, table, len(fs), djobs.data_ptr(), n, ws, nbytes, out,
                       torch.cuda.current_stream(dev).cuda_stream)
    del fs
    return out


def plan(x_hat_tiles, frames, fmt, overlap=0):
    """pc_chroma_clip_rate_plan for tensors (host only, nothing is launched or copied): True where tile_distortion_jobs of exactly
    these tensors with this overlap takes the wide-access path -- every frame of the table has to allow it.  frames: a list of tuples of
    batched tensors ([1,...]) whose strides already fit a frame."""
    _check_enums(fmt)
    f = FORMATS[fmt]
    x = x_hat_tiles
    wide = C.c_int(-1)
    host = (Frame * len(frames))(*[_frame_struct(ts) for ts in frames])
    rc = lib().pc_chroma_clip_rate_plan(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), int(overlap), f.layout, f.bits, f.sx, host,
                                        len(frames), C.byref(wide))
    if rc != PC_OK:
        raise ChromaClipRateError(rc, "pc_chroma_clip_rate_plan")
    return bool(wide.value)


# -- PCL2 ----------------------------------------------------------------------------------------------------------------------------

def pack_clip(blobs, source, H, W, tile, overlap, fmt, matrix, range, upsample, siting, contract=None):
    """chroma_clips.pack_clip's arguments -> one PCL2 container: PCL1's bytes under the magic "PCL2".  blobs[f][t], where
    source[f][t] == f, is a PCB1 container holding one level (checked when it is read, not here)."""
    return MAGIC + chroma_clips.pack_clip(blobs, source, H, W, tile, overlap, fmt, matrix, range, upsample, siting, contract)[4:]


def parse_clip(buf):
    """PCL2 only -> what chroma_clips.parse_clip gives for PCL1: dict(fmt, siting, matrix, range, upsample, bits, contract, grid
    (TileGrid, whole grid), F, table [F][ny*nx] of (offset, length), payload_start), after the same checks; an entry is checked
    against the buffer when its tile is asked for (tile_blob), so that a clip cut off inside its payload still gives the frames it
    holds completely."""
    return chroma_clips._parse(buf, MAGIC)


def tile_blob(buf, hd, k, t):
    """clips.clip_tile_bytes for PCL2: the PCB1 container of tile t of frame k and its parsed header, after checking its table entry
    against the buffer, its header against the grid and the clip's contract, and that it holds exactly one level."""
    return clips.clip_tile_bytes(buf, hd, k, t, one_level=True)


def frame_container(buf, k):
    """The PCK1 container of frame k of a PCL2 container: chroma_tiles.pack_frame_tiled(tiles.pack_tiled(the blobs of frame k,
    per_tile_levels=True)), a PCT2 container inside -- pure byte work; chroma_tiles.decode_frame_tiled reads it as it is."""
    hd = parse_clip(buf)
    k = clips._frame_index(hd, k)
    g = hd["grid"]
    blobs = [tile_blob(buf, hd, k, t)[0] for t in _range(g.ny * g.nx)]
    inner = pack_tiled(blobs, g.H, g.W, g.T, g.O, contract=hd["contract"], per_tile_levels=True)
    return pack_frame_tiled(inner, hd["fmt"], hd["matrix"], hd["range"], hd["upsample"], hd["siting"])


# -- through the codec ---------------------------------------------------------------------------------------------------------------

def encode_clip_to_size(model, frames, qualities, target_bytes, fmt, matrix="bt709", range="limited", upsample="linear", siting="centre",
                        tile=512, overlap=0, mask_pol="point-based-std", plane_weights=(1, 1, 1), importance=None, frame_weights=None,
                        reuse=True, max_tiles_per_call=32):
    """clip -> (PCL2 container of at most target_bytes bytes, ChromaClipRatePlan).  The source table is chroma_clips.encode_clip's
    (one clip_changes over the footprint of the format, siting and upsampling and one device-to-host copy; reuse=False makes every
    tile of every frame an item of its own).  The items -- the tiles that are coded -- are chunked by max_tiles_per_call ACROSS
    frames; per chunk one cut launch per frame present in it into one batch buffer, model.compress_levels,
    model.decompress_levels, one pc_chroma_clip_rate_sse_jobs call per level for the whole chunk (the frame table and the job list
    of the whole clip are uploaded once) and container.pack of a single level per item and level.  Every item then gets the level
    rate.allocate picks from the bytes each level costs and the distortion it leaves (the planes weighted by plane_weights = (wY,
    wCb, wCr), non-negative ints), weighted by importance[t] (one positive number per tile, [ny][nx] or flat) times the sum of
    frame_weights[k] (one positive number per frame) over the frames that show it (the reuse identity of the module's docstring),
    under the budget target_bytes - 47 - 16 * F * ny * nx.  ValueError, its message holding the minimum, if the cheapest level of
    every item does not fit.  Neither the bytes nor the plan depend on max_tiles_per_call or on how the frames lie in memory;
    frame_container(buf, k) is a PCK1 container chroma_tiles.decode_frame_tiled reads."""
    import torch
    qualities, step, pw, target_bytes, fs, g, importance, frame_weights = clip_rate._to_size_arguments(
        frames, qualities, target_bytes, fmt, matrix, range, upsample, tile, overlap, plane_weights, importance, frame_weights, max_tiles_per_call,
        check_enums=lambda f, m, r, u: _check_enums(f, m, r, u, siting), clip_frames=_clip_frames, grid=_grid)
    n, F, nl = g.ny * g.nx, len(fs), len(qualities)
    source = _source(fs, fmt, siting, g, upsample, reuse)
    items, runs = items_of(source)
    weights = item_weights(items, runs, n, F, importance, frame_weights)
    k = coefficients(matrix)
    dev = fs[0][0].device
    L = lib()
    with torch.cuda.device(dev):
        host, table = _frame_table(fs, dev)
        djobs = torch.tensor(items, dtype=torch.int32).to(dev)                 # [(f, t)] of the whole clip, uploaded once
        nbytes = L.pc_chroma_clip_rate_workspace_size(g.T, FORMATS[fmt].sy, min(step, len(items)))
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)

    def measure(a, b, decoded):
        with torch.cuda.device(dev):
            d = torch.empty((nl, b, 3), dtype=torch.int64, device=dev)
            st = torch.cuda.current_stream(dev).cuda_stream
            for l, o in enumerate(decoded):                                    # one call per level, ordered on the stream: one workspace
                xh = _fit_tiles(o["x_hat"], g.T)
                _sse_jobs_into(L, xh, g, fmt, siting, range, k, host, table, F, djobs[a:].data_ptr(), b, ws, nbytes, d[l], st)
            d = d.tolist()                                                     # [levels][b][3]; synchronises: xh may go
        return [[[int(v) for v in d[l][m]] for l in _range(nl)] for m in _range(b)]
    bufs, plane_dists = _tilecodec.encode_items(model, len(items), step, qualities, mask_pol, g.T,
                                                _cut_of(fs, g, items, fmt, matrix, range, upsample, siting), measure)
    del fs
    dists = [[pw[0] * v[0] + pw[1] * v[1] + pw[2] * v[2] for v in row] for row in plane_dists]
    buf, levels, rates = clip_rate._allocate_and_pack(
        bufs, dists, weights, items, source, target_bytes, g, fmt, matrix, range, upsample, header_bytes=HEADER_BYTES,
        pack=lambda *a: pack_clip(*a, siting))
    index = {it: i for i, it in enumerate(items)}
    chosen = [plane_dists[i][levels[i]] for i in _range(len(items))]
    sse = [[sum(chosen[index[(source[f][t], t)]][p] for t in _range(n)) for p in _range(3)] for f in _range(F)]
    predicted = sum(len(runs[i]) * dists[i][levels[i]] for i in _range(len(items)))
    return buf, ChromaClipRatePlan(source, items, weights, levels, rates, dists, plane_dists, 2 * g.O if g.O else 1, len(buf), predicted, sse,
                                   len(items), F * n - len(items), chroma_rate.sse_exact(g, fmt, siting))


def decode_clip(model, buf, frames=None, level=-1, region=None, fmt=None, siting=None, max_tiles_per_call=32):
    """The frames `frames` (an iterable of indices, default all of them, in the order given) of a PCL2 container -> a list of frames
    (tuples of planes without a batch axis) on the model's device, or of their admissible region = (y0, x0, h, w), in the stored
    format and siting or in `fmt` / `siting` (as chroma_tiles.decode_frame_tiled).  Admissibility and the halo are those of the OUTPUT
    format and siting; the tiles read are covering(halo_window(region)).  A PCL2 tile holds one level: level must be -1 or 0.  All
    byte work comes first, and every refusal is a ContainerError raised before the model is touched.  Among consecutive requested
    frames a byte range is decoded once: a tile whose table entry equals that of the frame handled just before reuses that frame's
    decoded float tile; the rest are grouped by quality (ascending, tile order within a group: the rule of a PCT2 container's tiles)
    and decoded max_tiles_per_call at a time.  Frame k is bit for bit chroma_tiles.decode_frame_tiled(model, frame_container(buf, k),
    ...).  The loop is clips.py's; a PCL1 container is passed to chroma_clips.decode_clip unchanged."""
    if len(buf) >= 4 and bytes(buf[:4]) == chroma_clips.MAGIC:
        return chroma_clips.decode_clip(model, buf, frames=frames, level=level, region=region, fmt=fmt, siting=siting,
                                        max_tiles_per_call=max_tiles_per_call)
    step = _tilecodec.tiles_per_call(max_tiles_per_call)
    hd = parse_clip(buf)
    _tilecodec.one_level(level, "PCL2")
    out_siting = hd["siting"] if siting is None else siting
    _check_enums(hd["fmt"] if fmt is None else fmt, siting=out_siting)

    def stitch(x, g, out_fmt, matrix, range, window):
        return stitch_frame(x, g, out_fmt, matrix, range, out_siting, window=window)
    return clips._decode(model, buf, hd, True, frames, level, region, fmt, step, stitch,
                         window_of=lambda region, H, W, out_fmt: _admissible_window(region, H, W, out_fmt),
                         covering_of=lambda g, window, out_fmt: covering(g, window, out_fmt, out_siting))

"""Rate-controlled clips of YUV 4:2:0 frames (libpc_clip_rate.so, clip_rate_csrc/pc_clip_rate.h): one clip of
NV12 / I420 / P010 frames in at most N bytes.  The composition of frame_rate.py (section 15: one frame in at most N bytes, every tile
at the level rate.allocate picks for it) and clips.py (section 16: static tiles coded once): a coded tile that is shown in m frames
is ONE item of the allocation, stored once, and its distortion counts m times.

  tile_distortion_jobs   decoded tiles + a clip + a list of (frame, tile) jobs -> the exact integer weighted squared error per job and
                         plane, one launch pair for jobs scattered over any number of frames (frame_rate.frame_tile_distortion takes
                         a linear range of tiles of one frame)
  items_of               source table -> (the coded tiles (f, t), the frames each is shown in)
  encode_clip_to_size    clip -> (PCS2 container of at most target_bytes bytes, ClipRatePlan)
  decode_clip            PCS2 container -> a list of frames (or of one region of each); PCS1 goes to clips.decode_clip
  frame_container        PCS2 container, k -> the PCG1 container of frame k holding a PCT2 one (pure byte work)

The reuse identity.  frame_tile_distortion of tile t reads, of the original frame, the tile's luma rectangle and its chroma rectangle
WITHOUT the halo; section 16 calls a tile unchanged between two frames only where every code of a superset of both (the footprint,
with the halo under linear upsampling) is equal.  The decoded tile is the same bits, too (the same bytes are decoded).  So for an
item (f, t) shown in frames f .. f + m - 1, D(f + j, t) = D(f, t) exactly, and the item's total distortion over the clip is m * D(f, t)
-- which is what rate.allocate's `importance` multiplies by.

Budget.  The header (42 bytes) and the table (16 bytes per frame and tile, reused or not) do not depend on the levels, so the
allocator gets target_bytes - 42 - 16 * F * ny * nx, and rates[i][l] is the length of item i's single-level PCB1 container alone.

PCS2 is PCS1 (clips.py: header, table, payload rules) with the magic "PCS2" and every coded tile's PCB1 container holding EXACTLY ONE
level; tiles may differ in quality.  What PCT2 is to PCT1.

There is no CPU fallback: CPU tensors raise ValueError before any device call.  Everything runs on the current stream of the tensors'
device.  Out of scope: per-frame byte caps and constant bitrate, a target PSNR (the dual problem), a tolerance inside
encode_clip_to_size (the reuse identity above does not hold under it: clip_tol_rate.py is that encoder), inter-frame
prediction, batching the decode across frames.  The same layer for the twelve formats and three sitings of `chroma` is
chroma_clip_rate.py (section 28); it comes through _to_size_arguments and _allocate_and_pack below with its own checks and packer.
"""
import collections
import ctypes as C
from fractions import Fraction

from . import clips
from . import _imagelib, _tilecodec
from ._lib import PC_OK
from ._tilecodec import max_tile  # noqa: F401
from .clips import ENTRY_BYTES, HEADER_BYTES, _clip_frames, _cut_of, _frame_index, _frame_table, _source, clip_tile_bytes, source_table  # noqa: F401
from .frame_tiles import pack_frame_tiled, stitch_frame
from .frames import FORMATS, RANGES, UPSAMPLES, Frame, _check_enums, _frame_struct, bits_of, coefficients  # noqa: F401
from .rate import allocate
from .tiles import TileGrid, _check_tiles, _fit_tiles, grid_of, pack_tiled

LIB_PATH = _imagelib.lib_path("clip_rate")

#: every symbol clip_rate_csrc/pc_clip_rate.h declares
EXPORTS = ["pc_clip_rate_workspace_size", "pc_clip_rate_sse_jobs", "pc_clip_rate_plan", "pc_clip_rate_strerror",
           "pc_clip_rate_last_hip_error"]

MAGIC = b"PCS2"
VERSION = 1

_range = range                            # the functions below take a parameter of that name


def _prototypes():
    i64, vp, ci, cf, fp = C.c_int64, C.c_void_p, C.c_int, C.c_float, C.POINTER(Frame)
    return {
        "pc_clip_rate_workspace_size": (C.c_size_t, [ci, ci]),
        "pc_clip_rate_sse_jobs": (None, [vp, i64, i64, i64] + [ci] * 6 + [cf] * 5 + [fp, vp, ci, vp, ci, vp, C.c_size_t, vp, vp]),
        "pc_clip_rate_plan": (None, [vp, i64, i64, i64, ci, ci, fp, ci, C.POINTER(ci)]),
        "pc_clip_rate_strerror": (C.c_char_p, [ci]),
    }


def lib():
    return _imagelib.load(LIB_PATH, _prototypes)


class ClipRateError(_imagelib.ImageLibError):
    _lib, _prefix = staticmethod(lib), "pc_clip_rate"


#: what encode_clip_to_size decided: source[f][t] (clips.ClipPlan's); items[i] = (f, t), the coded tiles in (f, t) order; weights[i]
#: (Fractions: importance[t] times the sum of frame_weights over the frames that show item i -- by default the number of those
#: frames); levels[i] (index into the quality list); rates[i][l] (the bytes of item i's PCB1 container at level l); dists[i][l]
#: (plane_dists weighted by plane_weights); plane_dists[i][l] = [D_Y, D_Cb, D_Cr] (tile_distortion_jobs, in the frame the item was
#: coded for); den (the band weights' denominator per axis); container_bytes; sse[k][p] (per frame k and plane p the sum over its
#: tiles of the chosen plane_dists of the items they point at: at overlap 0 the decoded frame's exact SSE); predicted (the same sum
#: of the chosen dists over all frames and tiles); n_coded and n_reused (they add up to F * ny * nx)
ClipRatePlan = collections.namedtuple("ClipRatePlan", "source items weights levels rates dists plane_dists den container_bytes predicted sse "
                                      "n_coded n_reused")


# -- the kernel ----------------------------------------------------------------------------------------------------------------------

def _sse_jobs_into(L, x, g, fmt, range, k, host, table, F, jobs_ptr, n, ws, nbytes, out, stream):
    rc = L.pc_clip_rate_sse_jobs(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), g.H, g.W, g.T, g.O, FORMATS[fmt], RANGES[range],
                                 k.kr, k.kg, k.kb, k.ib, k.ir, host, table.data_ptr(), F, jobs_ptr, n, ws.data_ptr(), nbytes, out.data_ptr(),
                                 stream)
    if rc != PC_OK:
        raise ClipRateError(rc, "pc_clip_rate_sse_jobs")


def _jobs(jobs, F, g):
    import torch
    rows = jobs.tolist() if torch.is_tensor(jobs) else [list(j) if isinstance(j, (tuple, list)) else j for j in jobs]
    if not rows:
        raise ValueError("jobs must name at least one (frame, tile) pair")
    for j in rows:
        if not isinstance(j, list) or len(j) != 2 or any(isinstance(v, bool) or not isinstance(v, int) for v in j):
            raise ValueError(f"a job is a (frame, tile) pair of ints, got {j!r}")
        if not 0 <= j[0] < F or not 0 <= j[1] < g.ny * g.nx:
            raise ValueError(f"job {tuple(j)!r} lies outside the {F} frames or the {g.ny}x{g.nx} grid (row-major tile indices 0 .. {g.ny * g.nx - 1})")
    return rows


def tile_distortion_jobs(x_hat_tiles, grid, frames, jobs, fmt, matrix="bt709", range="limited"):
    """x_hat_tiles: float32 cuda [n,3,T,T] (any tile / channel / row strides, unit stride along a row); frames: a clip (a list of
    frames of grid's H x W, or one tuple of batched planes, any row strides); jobs: n (frame, tile) pairs of ints, the tile row-major
    in grid's whole ny x nx grid, in any order, repeats allowed (validated here, on the host, before they are uploaded) -> int64 cuda
    [n,3]: row m is frame_rate.frame_tile_distortion(x_hat_tiles[m:m+1], grid, frames[f], ..., first_tile=t) for jobs[m] = (f, t),
    exactly (pc_clip_rate.h).  One launch pair whatever the number of frames the jobs name."""
    import torch
    _check_enums(fmt, matrix, range)
    g = TileGrid(*grid)
    full = grid_of(g.H, g.W, g.T, g.O)
    if (full.ny, full.nx) != (g.ny, g.nx):
        raise ValueError(f"{g}: the grid of a {g.H}x{g.W} frame is {full.ny}x{full.nx}")
    _tilecodec.tile_limit(g.T, fmt)
    fs, H, W = _clip_frames(frames, fmt)
    rows = _jobs(jobs, len(fs), full)
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
        nbytes = L.pc_clip_rate_workspace_size(g.T, n)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        out = torch.empty((n, 3), dtype=torch.int64, device=dev)
        _sse_jobs_into(L, x, full, fmt, range, k, host, table, len(fs), djobs.data_ptr(), n, ws, nbytes, out,
                       torch.cuda.current_stream(dev).cuda_stream)
    del fs
    return out


def plan(x_hat_tiles, frames, fmt, overlap=0):
    """pc_clip_rate_plan for tensors (host only, nothing is launched or copied): True where tile_distortion_jobs of exactly these
    tensors with this overlap takes the wide-access path.  frames: a list of tuples of batched tensors ([1,...]) whose strides already
    fit a frame."""
    _check_enums(fmt)
    x = x_hat_tiles
    wide = C.c_int(-1)
    host = (Frame * len(frames))(*[_frame_struct(ts) for ts in frames])
    rc = lib().pc_clip_rate_plan(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), int(overlap), FORMATS[fmt], host, len(frames), C.byref(wide))
    if rc != PC_OK:
        raise ClipRateError(rc, "pc_clip_rate_plan")
    return bool(wide.value)


# -- PCS2 ----------------------------------------------------------------------------------------------------------------------------

def pack_clip(blobs, source, H, W, tile, overlap, fmt, matrix, range, upsample, contract=None):
    """clips.pack_clip's arguments -> one PCS2 container: PCS1's bytes under the magic "PCS2".  blobs[f][t], where source[f][t] == f,
    is a PCB1 container holding one level (checked when it is read, not here)."""
    return MAGIC + clips.pack_clip(blobs, source, H, W, tile, overlap, fmt, matrix, range, upsample, contract)[4:]


def parse_clip(buf):
    """PCS2 only -> what clips.parse_clip gives for PCS1: dict(fmt, matrix, range, upsample, bits, contract, grid (TileGrid, whole
    grid), F, table [F][ny*nx] of (offset, length), payload_start).  The same checks: the header, the geometry against pc_tiles_grid,
    that the whole table is there and that two entries are either equal or disjoint; an entry is checked against the buffer when
    its tile is asked for (tile_blob), so that a clip cut off inside its payload still gives the frames it holds completely."""
    return clips._parse(buf, MAGIC)


def tile_blob(buf, hd, k, t):
    """clips.clip_tile_bytes for PCS2: the PCB1 container of tile t of frame k and its parsed header, after checking its table entry
    against the buffer, its header against the grid and the clip's contract, and that it holds exactly one level."""
    return clip_tile_bytes(buf, hd, k, t, one_level=True)


def frame_container(buf, k):
    """The PCG1 container of frame k of a PCS2 container: frame_tiles.pack_frame_tiled(tiles.pack_tiled(the blobs of frame k,
    per_tile_levels=True)), a PCT2 container inside -- pure byte work; frame_tiles.decode_frame_tiled reads it as it is."""
    hd = parse_clip(buf)
    k = _frame_index(hd, k)
    g = hd["grid"]
    blobs = [tile_blob(buf, hd, k, t)[0] for t in _range(g.ny * g.nx)]
    inner = pack_tiled(blobs, g.H, g.W, g.T, g.O, contract=hd["contract"], per_tile_levels=True)
    return pack_frame_tiled(inner, hd["fmt"], hd["matrix"], hd["range"], hd["upsample"])


# -- the allocation's items ------------------------------------------------------------------------------------------------------------

def items_of(source):
    """source[f][t] (clips.source_table) -> (items, runs): items, every (f, t) with source[f][t] == f in (f, t) order -- the tiles
    that are coded --, and runs[i], the frames that show item i, ascending (f first)."""
    items = [(f, t) for f, row in enumerate(source) for t, s in enumerate(row) if s == f]
    index = {it: i for i, it in enumerate(items)}
    runs = [[] for _ in items]
    for k, row in enumerate(source):
        for t, s in enumerate(row):
            if (s, t) not in index:
                raise ValueError(f"source[{k}][{t}] = {s!r} names a frame tile {t} was not coded in")
            runs[index[(s, t)]].append(k)
    return items, runs


def item_weights(items, runs, n_tiles, n_frames, importance=None, frame_weights=None):
    """importance[t] * sum of frame_weights[k] over runs[i], as exact Fractions; the defaults are 1, so the default is len(runs[i])"""
    imp = [Fraction(1)] * n_tiles if importance is None else [Fraction(v) for v in importance]
    fw = [Fraction(1)] * n_frames if frame_weights is None else [Fraction(v) for v in frame_weights]
    if len(imp) != n_tiles or any(v <= 0 for v in imp):
        raise ValueError(f"importance needs one positive number per tile, {n_tiles} in all")
    if len(fw) != n_frames or any(v <= 0 for v in fw):
        raise ValueError(f"frame_weights needs one positive number per frame, {n_frames} in all")
    return [imp[t] * sum(fw[k] for k in run) for (_, t), run in zip(items, runs)]


# -- through the codec ---------------------------------------------------------------------------------------------------------------

def _to_size_arguments(frames, qualities, target_bytes, fmt, matrix, range, upsample, tile, overlap, plane_weights, importance, frame_weights,
                       max_tiles_per_call, check_enums=None, clip_frames=None, grid=None):
    """the argument checks of encode_clip_to_size (clip_tol_rate.encode_clip_to_size comes here, too), in its order and with its
    messages -> (qualities, step, plane weights, target_bytes, fs (the planes of frame k as batched views), the grid, importance
    flat or None, frame_weights as a list or None).  The three keywords are for a caller with other formats (chroma_clip_rate.py):
    check_enums(fmt, matrix, range, upsample), clip_frames(frames, fmt) and grid(H, W, tile, overlap); by default the 4:2:0 checks,
    clips._clip_frames and clips._grid."""
    qualities = _tilecodec.levels_of(qualities)
    (check_enums or _check_enums)(fmt, matrix, range, upsample)
    step = _tilecodec.tiles_per_call(max_tiles_per_call)
    pw = _tilecodec.plane_weights_of(plane_weights)
    target_bytes = int(target_bytes)
    fs, H, W = (clip_frames or _clip_frames)(frames, fmt)
    g = (grid or clips._grid)(H, W, tile, overlap)
    _tilecodec.tile_limit(g.T, fmt)
    return qualities, step, pw, target_bytes, fs, g, _tilecodec.importance_of(importance, g), _tilecodec.frame_weights_of(frame_weights, len(fs))


def _allocate_and_pack(bufs, dists, weights, items, source, target_bytes, g, fmt, matrix, range, upsample, header_bytes=None, pack=None):
    """What follows the work loop of encode_clip_to_size (and of clip_tol_rate's): bufs[i][l] the single-level containers of item
    i, dists[i][l] what each level leaves -> (the PCS2 container of at most target_bytes bytes, levels[i], rates[i][l]).
    ValueError, its message holding the minimum, if the cheapest level of every item does not fit.  The two keywords are for a
    caller with another container (chroma_clip_rate.py's PCL2): the bytes of its header and its packer, called with pack_clip's
    arguments; by default PCS2's 42 bytes and pack_clip."""
    n, F = g.ny * g.nx, len(source)
    rates = [[len(p) for p in row] for row in bufs]
    fixed = (HEADER_BYTES if header_bytes is None else header_bytes) + ENTRY_BYTES * F * n
    minimum = sum(min(r) for r in rates)
    if fixed + minimum > target_bytes:
        raise ValueError(f"target_bytes = {target_bytes} is below the minimum of {fixed + minimum} bytes: {fixed} bytes of header and table "
                         f"and {minimum} bytes for every coded tile at its cheapest level")
    levels = allocate(rates, dists, target_bytes - fixed, weights)
    blobs = [[None] * n for _ in _range(F)]
    for (f, t), row, l in zip(items, bufs, levels):
        blobs[f][t] = row[l]
    return (pack or pack_clip)(blobs, source, g.H, g.W, g.T, g.O, fmt, matrix, range, upsample), levels, rates


def encode_clip_to_size(model, frames, qualities, target_bytes, fmt, matrix="bt709", range="limited", upsample="linear", tile=512,
                        overlap=0, mask_pol="point-based-std", plane_weights=(1, 1, 1), importance=None, frame_weights=None, reuse=True,
                        max_tiles_per_call=32):
    """clip -> (PCS2 container of at most target_bytes bytes, ClipRatePlan).  The source table is clips.encode_clip's (one
    clip_changes and one device-to-host copy; reuse=False makes every tile of every frame an item of its own).  The items -- the
    tiles that are coded -- are chunked by max_tiles_per_call ACROSS frames; per chunk one cut launch per frame present in it into
    one batch buffer, model.compress_levels, model.decompress_levels, one pc_clip_rate_sse_jobs call per level for the whole chunk
    (the frame table and the job list of the whole clip are uploaded once) and container.pack of a single level per item and level.
    Every item then gets the level rate.allocate picks from the bytes each level costs and the distortion it leaves (the planes
    weighted by plane_weights = (wY, wCb, wCr), non-negative ints), weighted by importance[t] (one positive number per tile, [ny][nx]
    or flat) times the sum of frame_weights[k] (one positive number per frame) over the frames that show it, under the budget
    target_bytes - 42 - 16 * F * ny * nx.  ValueError, its message holding the minimum, if the cheapest level of every item does not
    fit.  Neither the bytes nor the plan depend on max_tiles_per_call or on how the frames lie in memory; frame_container(buf, k)
    is a PCG1 container frame_tiles.decode_frame_tiled reads."""
    import torch
    qualities, step, pw, target_bytes, fs, g, importance, frame_weights = _to_size_arguments(
        frames, qualities, target_bytes, fmt, matrix, range, upsample, tile, overlap, plane_weights, importance, frame_weights, max_tiles_per_call)
    n, F, nl = g.ny * g.nx, len(fs), len(qualities)
    source = _source(fs, fmt, g, upsample, reuse)
    items, runs = items_of(source)
    weights = item_weights(items, runs, n, F, importance, frame_weights)
    k = coefficients(matrix)
    dev = fs[0][0].device
    L = lib()
    with torch.cuda.device(dev):
        host, table = _frame_table(fs, dev)
        djobs = torch.tensor(items, dtype=torch.int32).to(dev)                 # [(f, t)] of the whole clip, uploaded once
        nbytes = L.pc_clip_rate_workspace_size(g.T, min(step, len(items)))
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)

    def measure(a, b, decoded):
        with torch.cuda.device(dev):
            d = torch.empty((nl, b, 3), dtype=torch.int64, device=dev)
            st = torch.cuda.current_stream(dev).cuda_stream
            for l, o in enumerate(decoded):                                    # one call per level, ordered on the stream: one workspace
                xh = _fit_tiles(o["x_hat"], g.T)
                _sse_jobs_into(L, xh, g, fmt, range, k, host, table, F, djobs[a:].data_ptr(), b, ws, nbytes, d[l], st)
            d = d.tolist()                                                     # [levels][b][3]; synchronises: xh may go
        return [[[int(v) for v in d[l][m]] for l in _range(nl)] for m in _range(b)]
    bufs, plane_dists = _tilecodec.encode_items(model, len(items), step, qualities, mask_pol, g.T,
                                                _cut_of(fs, g, items, fmt, matrix, range, upsample), measure)
    del fs
    dists = [[pw[0] * v[0] + pw[1] * v[1] + pw[2] * v[2] for v in row] for row in plane_dists]
    buf, levels, rates = _allocate_and_pack(bufs, dists, weights, items, source, target_bytes, g, fmt, matrix, range, upsample)
    index = {it: i for i, it in enumerate(items)}
    chosen = [plane_dists[i][levels[i]] for i in _range(len(items))]
    sse = [[sum(chosen[index[(source[f][t], t)]][p] for t in _range(n)) for p in _range(3)] for f in _range(F)]
    predicted = sum(len(runs[i]) * dists[i][levels[i]] for i in _range(len(items)))
    return buf, ClipRatePlan(source, items, weights, levels, rates, dists, plane_dists, 2 * g.O if g.O else 1, len(buf), predicted, sse,
                             len(items), F * n - len(items))


def decode_clip(model, buf, frames=None, level=-1, region=None, fmt=None, max_tiles_per_call=32):
    """The frames `frames` (an iterable of indices, default all of them, in the order given) of a PCS2 container -> a list of frames
    (tuples of planes without a batch axis) on the model's device, or of their admissible region = (y0, x0, h, w), in the stored
    format or in `fmt` (as frame_tiles.decode_frame_tiled).  A PCS2 tile holds one level: level must be -1 or 0.  All byte work comes
    first, and every refusal is a ContainerError raised before the model is touched.  Among consecutive requested frames a byte range
    is decoded once: a tile whose table entry equals that of the frame handled just before reuses that frame's decoded float tile;
    the rest are grouped by quality (ascending, tile order within a group: the rule of a PCT2 container's tiles) and decoded
    max_tiles_per_call at a time.  Frame k is bit for bit frame_tiles.decode_frame_tiled(model, frame_container(buf, k), ...).  A PCS1
    container is passed to clips.decode_clip unchanged."""
    if len(buf) >= 4 and bytes(buf[:4]) == clips.MAGIC:
        return clips.decode_clip(model, buf, frames=frames, level=level, region=region, fmt=fmt, max_tiles_per_call=max_tiles_per_call)
    step = _tilecodec.tiles_per_call(max_tiles_per_call)
    hd = parse_clip(buf)
    _tilecodec.one_level(level, "PCS2")
    return clips._decode(model, buf, hd, True, frames, level, region, fmt, step, stitch_frame)

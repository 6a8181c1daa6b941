"""Tolerant rate-controlled clips of YUV frames of any chroma subsampling and siting (libpc_chroma_clip_tol_rate.so,
chroma_clip_tol_rate_gpu/pc_chroma_clip_tol_rate.h): what `clip_tol_rate` is for NV12 / I420 / P010 with
centre-sited chroma, for the twelve formats and three sitings of `chroma`.  One clip in at most N bytes, where a tile is coded once
while its footprint stays CLOSE to the frame it was last coded in.  The composition of chroma_clip_rate.py (section 28: a byte budget,
every coded tile at the level rate.allocate picks for it) and chroma_clip_tol.py (section 29: the tolerant scan): the source table is
chroma_clip_tol.scan_clip's, the container is PCL2.  No body is restated here: the loops are _tilecodec's, the argument checks, the
items and the allocation clip_rate's, the run checks, the offsets and the allocation's numbers clip_tol_rate's, the scan
chroma_clip_tol's, the cut chroma_clips', the container bytes chroma_clip_rate's.

  tile_distortion_runs   decoded tiles + a clip + per tile the frames it is shown in -> the exact integer weighted squared error per
                         (tile, frame) and plane: one launch pair, every tile read and emitted once
  plan                   host only: whether tile_distortion_runs of these tensors takes the wide-access path
  encode_clip_to_size    clip + tolerance -> (PCL2 container of at most target_bytes bytes, ChromaClipTolRatePlan)
  decode_clip, frame_container, parse_clip, tile_blob   chroma_clip_rate's: nothing new is needed to decode

Why a kernel of its own.  chroma_clip_rate's reuse identity D(k, t) = D(f, t) holds because a reused tile's footprint is EQUAL in
every frame of its run; under a tolerance it is only close, so an item's distortion has to be measured against every frame that shows
it.  chroma_clip_rate.tile_distortion_jobs can express that only with one copy of the decoded tile per frame, each read and emitted
again -- colour matrix, rounding, clamps, the chroma filters with their co-sited halo; here the tile's codes are held in registers
and compared against each frame of the run.

The contract.  source is chroma_clip_tol.scan_clip's table for the given Tolerance; items and runs are clip_rate.items_of(source).
plane_dists[i][l][j][p] is chroma_rate.frame_tile_distortion of item i = (f, t) decoded at level l against frame runs[i][j], plane p.
M (frame_scale) is the least common multiple of the denominators of Fraction(frame_weights[k]), fwi[k] = frame_weights[k] * M an int;
dists[i][l] = sum over j of fwi[runs[i][j]] * (wY, wCb, wCr) . plane_dists[i][l][j], Python ints; weights[i] = importance[t]
(a uniform scale of the distortions changes nothing, so M is not divided out); rates[i][l] the length of the item's single-level
PCB1 container; levels = rate.allocate(rates, dists, target_bytes - 47 - 16 * F * ny * nx, weights).  sse[k][p] is the sum over the
tiles t of frame k of plane_dists[i][levels[i]][j][p], i the item (source[k][t], t) and j the position of k in its run: sse[k][0] is
at overlap 0 the exact luma SSE of the decoded frame k against the frame k that was shown, for every format and siting, a reused
tile's error against a frame it was not cut from included; the chroma planes are exact where sse_exact holds (chroma_rate.sse_exact),
elsewhere the sum of the per-tile measures against frame k.  predicted is that sum over all frames weighted by plane_weights,
unweighted by frames, as chroma_clip_rate's.  With Tolerance() the bytes, levels, rates, sse and predicted are
chroma_clip_rate.encode_clip_to_size's; with Tolerance(max_run=1) those of reuse=False.  For "nv12", "i420" and "p010" at "centre"
the levels, rates, plane_dists and tile blobs are clip_tol_rate's.

There is no CPU fallback: CPU tensors raise ValueError before any device call.  Everything runs on the current stream of the tensors'
device.  Out of scope: per-frame byte caps and constant bitrate, a target PSNR, inter-frame prediction, letting the allocation choose
where a run ends.
"""
import collections
import ctypes as C

from . import _imagelib, _tilecodec, chroma_rate, clip_rate
from ._lib import PC_OK
from ._tilecodec import max_tile  # noqa: F401
from .chroma import FORMATS, SITINGS, _check_enums
from .chroma_clip_rate import decode_clip, frame_container, pack_clip, parse_clip, tile_blob  # noqa: F401
from .chroma_clip_tol import _scan, _tolerance
from .chroma_clips import HEADER_BYTES, _clip_frames, _cut_of, _grid
from .clip_rate import items_of
from .clip_tol import Tolerance
from .clip_tol_rate import ClipTolRatePlan, _offsets, _runs, frame_scale, item_importance
from .clips import ENTRY_BYTES, _frame_table  # noqa: F401
from .frames import RANGES, Frame, _frame_struct, coefficients
from .tiles import TileGrid, _check_tiles, _fit_tiles, grid_of

LIB_PATH = _imagelib.lib_path("chroma_clip_tol_rate")

#: every symbol chroma_clip_tol_rate_gpu/pc_chroma_clip_tol_rate.h declares
EXPORTS = ["pc_chroma_clip_tol_rate_workspace_size", "pc_chroma_clip_tol_rate_sse_runs", "pc_chroma_clip_tol_rate_plan",
           "pc_chroma_clip_tol_rate_strerror", "pc_chroma_clip_tol_rate_last_hip_error"]

_range = range                            # the functions below take a parameter of that name


def _prototypes():
    i64, vp, ci, cf, fp, ip = C.c_int64, C.c_void_p, C.c_int, C.c_float, C.POINTER(Frame), C.POINTER(C.c_int32)
    return {
        "pc_chroma_clip_tol_rate_workspace_size": (C.c_size_t, [ci, ci, ci]),
        "pc_chroma_clip_tol_rate_sse_runs": (None, [vp, i64, i64, i64] + [ci] * 12 + [cf] * 5
                                             + [fp, vp, ci, vp, ip, vp, vp, ci, ci, vp, C.c_size_t, vp, vp]),
        "pc_chroma_clip_tol_rate_plan": (None, [vp, i64, i64, i64, ci, ci, ci, ci, fp, ci, C.POINTER(ci)]),
        "pc_chroma_clip_tol_rate_strerror": (C.c_char_p, [ci]),
    }


def lib():
    return _imagelib.load(LIB_PATH, _prototypes)


class ChromaClipTolRateError(_imagelib.ImageLibError):
    _lib, _prefix = staticmethod(lib), "pc_chroma_clip_tol_rate"


#: what encode_clip_to_size decided: clip_tol_rate.ClipTolRatePlan's fields -- source, items, runs, weights, frame_scale, levels,
#: rates, dists, plane_dists (against every frame of the run), den, container_bytes, predicted, sse[k][p], n_coded, n_reused, stats,
#: worst -- and sse_exact (chroma_rate.sse_exact of the grid, the format and the siting): where it holds, sse[k][p] is the decoded
#: frame's exact per-plane SSE against frame k; sse[k][0] is that at overlap 0 whatever the siting
ChromaClipTolRatePlan = collections.namedtuple("ChromaClipTolRatePlan", ClipTolRatePlan._fields + ("sse_exact",))


# -- the kernel ----------------------------------------------------------------------------------------------------------------------

def _sse_runs_into(L, x, g, fmt, siting, range, k, host, table, F, tiles_ptr, offsets_host, offsets_ptr, slots_ptr, n, ne, ws, nbytes, out,
                   stream):
    rc = L.pc_chroma_clip_tol_rate_sse_runs(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), g.H, g.W, g.T, g.O, *FORMATS[fmt],
                                            *SITINGS[siting], RANGES[range], k.kr, k.kg, k.kb, k.ib, k.ir, host, table.data_ptr(), F,
                                            tiles_ptr, offsets_host, offsets_ptr, slots_ptr, n, ne, ws.data_ptr(), nbytes, out.data_ptr(),
                                            stream)
    if rc != PC_OK:
        raise ChromaClipTolRateError(rc, "pc_chroma_clip_tol_rate_sse_runs")


def tile_distortion_runs(x_hat_tiles, grid, frames, tiles, runs, fmt, matrix="bt709", range="limited", siting="centre"):
    """x_hat_tiles: float32 cuda [n,3,T,T] (any tile / channel / row strides, unit stride along a row); frames: a clip (a list of
    frames of grid's H x W in `fmt`, or one tuple of batched planes, any row strides) whose chroma is sited as `siting` says;
    tiles[m]: an int, the tile of x_hat_tiles[m], row-major in grid's whole ny x nx grid, repeats allowed; runs[m]: a non-empty list
    of frame indices, in any order, repeats allowed (both validated here, on the host, before they are uploaded, with
    clip_tol_rate's texts) -> (out, offsets): out int64 cuda [n_entries,3], offsets a Python list of n + 1 ints; row offsets[m] + j is
    chroma_clip_rate.tile_distortion_jobs' row for x_hat_tiles[m] and the job (runs[m][j], tiles[m]), exactly
    (pc_chroma_clip_tol_rate.h).  One upload of tiles, offsets and slots and one launch pair; every tile is read and emitted once,
    however long its run."""
    import torch
    _check_enums(fmt, matrix, range, siting=siting)
    g = TileGrid(*grid)
    full = grid_of(g.H, g.W, g.T, g.O)
    if (full.ny, full.nx) != (g.ny, g.nx):
        raise ValueError(f"{g}: the grid of a {g.H}x{g.W} frame is {full.ny}x{full.nx}")
    _tilecodec.tile_limit(g.T, fmt)
    fs, H, W = _clip_frames(frames, fmt)
    ts, rs = _runs(tiles, runs, len(fs), full)
    x = x_hat_tiles
    n = len(ts)
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[0] != n:
        raise ValueError(f"x_hat_tiles must be a [{n},3,{g.T},{g.T}] tensor, one tile per entry of tiles")
    _check_tiles(x, full._replace(nty=1, ntx=n))
    dev = fs[0][0].device
    if (H, W) != (g.H, g.W) or x.device != dev:
        raise ValueError(f"frames must be {g.H}x{g.W} frames on {x.device}, got {H}x{W} on {dev}")
    x = _fit_tiles(x, g.T)
    k = coefficients(matrix)
    off = _offsets(rs)
    ne = off[-1]
    L = lib()
    with torch.cuda.device(dev):
        host, table = _frame_table(fs, dev)
        words = torch.tensor(ts + off + [v for run in rs for v in run], dtype=torch.int32).to(dev)      # one upload: tiles, offsets, slots
        nbytes = L.pc_chroma_clip_tol_rate_workspace_size(g.T, FORMATS[fmt].sy, ne)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        out = torch.empty((ne, 3), dtype=torch.int64, device=dev)
        _sse_runs_into(L, x, full, fmt, siting, range, k, host, table, len(fs), words.data_ptr(), (C.c_int32 * (n + 1))(*off),
                       words[n:].data_ptr(), words[2 * n + 1:].data_ptr(), n, ne, ws, nbytes, out, torch.cuda.current_stream(dev).cuda_stream)
    del fs
    return out, off


def plan(x_hat_tiles, frames, fmt, overlap=0):
    """pc_chroma_clip_tol_rate_plan for tensors (host only, nothing is launched or copied): True where tile_distortion_runs of
    exactly these tensors with this overlap takes the wide-access path -- every frame of the table has to allow it.  frames: a list of
    tuples of batched tensors ([1,...]) whose strides already fit a frame."""
    _check_enums(fmt)
    f = FORMATS[fmt]
    x = x_hat_tiles
    wide = C.c_int(-1)
    host = (Frame * len(frames))(*[_frame_struct(ts) for ts in frames])
    rc = lib().pc_chroma_clip_tol_rate_plan(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), int(overlap), f.layout, f.bits, f.sx, host,
                                            len(frames), C.byref(wide))
    if rc != PC_OK:
        raise ChromaClipTolRateError(rc, "pc_chroma_clip_tol_rate_plan")
    return bool(wide.value)


# -- through the codec ---------------------------------------------------------------------------------------------------------------

def encode_clip_to_size(model, frames, qualities, target_bytes, fmt, matrix="bt709", range="limited", upsample="linear", siting="centre",
                        tile=512, overlap=0, mask_pol="point-based-std", tolerance=Tolerance(), plane_weights=(1, 1, 1), importance=None,
                        frame_weights=None, max_tiles_per_call=32):
    """clip -> (PCL2 container of at most target_bytes bytes, ChromaClipTolRatePlan).  The argument checks are
    chroma_clip_rate.encode_clip_to_size's; the source table is chroma_clip_tol.scan_clip's under `tolerance` over the footprint of
    the format, siting and upsampling (one scan, one device-to-host copy of source and stats).  Then chroma_clip_rate's work loop over
    the coded tiles, chunked by max_tiles_per_call ACROSS frames -- the cut launches, model.compress_levels,
    model.decompress_levels, container.pack of a single level per item and level -- with one pc_chroma_clip_tol_rate_sse_runs call
    per level for the chunk's jobs: every decoded tile against every frame of its run (the frame table, the tile list, the offsets
    and the slots of the whole clip are uploaded once; one workspace, sized for the chunk with the most entries).  Every item then
    gets the level rate.allocate picks from the bytes each level costs and the distortion it leaves over its run (the planes weighted
    by plane_weights = (wY, wCb, wCr), non-negative ints; frame k by frame_weights[k], one positive number per frame), weighted by
    importance[t] (one positive number per tile, [ny][nx] or flat), under the budget target_bytes - 47 - 16 * F * ny * nx.
    ValueError, its message holding the minimum, if the cheapest level of every item does not fit.  Neither the bytes nor the plan
    depend on max_tiles_per_call or on how the frames lie in memory; frame_container(buf, k) is a PCK1 container
    chroma_tiles.decode_frame_tiled reads; decode_clip is chroma_clip_rate's."""
    import torch
    qualities, step, pw, target_bytes, fs, g, importance, frame_weights = clip_rate._to_size_arguments(
        frames, qualities, target_bytes, fmt, matrix, range, upsample, tile, overlap, plane_weights, importance, frame_weights, max_tiles_per_call,
        check_enums=lambda f, m, r, u: _check_enums(f, m, r, u, siting), clip_frames=_clip_frames, grid=_grid)
    tol = _tolerance(tolerance, fmt)
    n, F, nl = g.ny * g.nx, len(fs), len(qualities)
    M, fwi = frame_scale(frame_weights, F)
    per_tile = item_importance([(0, t) for t in _range(n)], n, importance)     # checked before the scan
    src, st = _scan(fs, fmt, siting, g, upsample, tol)
    both = torch.cat([src.to(torch.int64).reshape(F, n, 1), st.reshape(F, n, 9)], dim=2).cpu()         # the one copy
    source, stats = both[:, :, 0].tolist(), both[:, :, 1:].reshape(F, n, 3, 3).tolist()
    worst = [max([stats[k][t][p][2] for k in _range(F) for t in _range(n) if source[k][t] != k], default=0) for p in _range(3)]
    items, runs = items_of(source)
    weights = [per_tile[t] for _, t in items]
    off = _offsets(runs)
    chunks = [(a, min(a + step, len(items))) for a in _range(0, len(items), step)]
    k = coefficients(matrix)
    dev = fs[0][0].device
    L = lib()
    with torch.cuda.device(dev):
        host, table = _frame_table(fs, dev)
        # the tables of the whole clip in one upload: the tiles; per chunk its offsets from 0; the slots
        rebased = [[off[m] - off[a] for m in _range(a, b + 1)] for a, b in chunks]
        words = torch.tensor([t for _, t in items] + [v for row in rebased for v in row] + [v for run in runs for v in run],
                             dtype=torch.int32).to(dev)
        at_offsets = [len(items)]
        for row in rebased:
            at_offsets.append(at_offsets[-1] + len(row))
        at_slots = at_offsets[-1]
        most = max(off[b] - off[a] for a, b in chunks)
        nbytes = L.pc_chroma_clip_tol_rate_workspace_size(g.T, FORMATS[fmt].sy, most)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)

    def measure(a, b, decoded):
        c = a // step
        ne = off[a + b] - off[a]
        host_off = (C.c_int32 * (b + 1))(*rebased[c])
        with torch.cuda.device(dev):
            d = torch.empty((nl, ne, 3), dtype=torch.int64, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            for l, o in enumerate(decoded):                                    # one call per level, ordered on the stream: one workspace
                xh = _fit_tiles(o["x_hat"], g.T)
                _sse_runs_into(L, xh, g, fmt, siting, range, k, host, table, F, words[a:].data_ptr(), host_off,
                               words[at_offsets[c]:].data_ptr(), words[at_slots + off[a]:].data_ptr(), b, ne, ws, nbytes, d[l], stream)
            d = d.tolist()                                                     # [levels][entries][3]; synchronises: xh may go
        return [[[[int(v) for v in d[l][e]] for e in _range(off[a + m] - off[a], off[a + m + 1] - off[a])] for l in _range(nl)]
                for m in _range(b)]
    bufs, plane_dists = _tilecodec.encode_items(model, len(items), step, qualities, mask_pol, g.T,
                                                _cut_of(fs, g, items, fmt, matrix, range, upsample, siting), measure)
    del fs
    dists = [[sum(fwi[f] * (pw[0] * v[0] + pw[1] * v[1] + pw[2] * v[2]) for f, v in zip(run, per_frame)) for per_frame in row]
             for run, row in zip(runs, plane_dists)]
    buf, levels, rates = clip_rate._allocate_and_pack(
        bufs, dists, weights, items, source, target_bytes, g, fmt, matrix, range, upsample, header_bytes=HEADER_BYTES,
        pack=lambda *a: pack_clip(*a, siting))
    chosen = [plane_dists[i][levels[i]] for i in _range(len(items))]                                   # [i][j][p]
    sse = [[0, 0, 0] for _ in _range(F)]
    predicted = 0
    for run, per_frame in zip(runs, chosen):
        for f, v in zip(run, per_frame):
            for p in _range(3):
                sse[f][p] += v[p]
            predicted += pw[0] * v[0] + pw[1] * v[1] + pw[2] * v[2]
    return buf, ChromaClipTolRatePlan(source, items, runs, weights, M, levels, rates, dists, plane_dists, 2 * g.O if g.O else 1, len(buf),
                                      predicted, sse, len(items), F * n - len(items), stats, worst, chroma_rate.sse_exact(g, fmt, siting))

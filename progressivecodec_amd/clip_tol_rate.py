"""Tolerant rate-controlled clips of YUV 4:2:0 frames (libpc_clip_tol_rate.so, clip_tol_rate_hip/pc_clip_tol_rate.h; DESIGN.md section
20): one clip of NV12 / I420 / P010 frames in at most N bytes, where a tile is coded once while its footprint stays CLOSE to the frame
it was last coded in.  The composition of clip_rate.py (section 17: a byte budget, every coded tile at the level rate.allocate picks
for it) and clip_tol.py (section 18: the tolerant scan): the source table is clip_tol.scan_clip's, the container is PCS2.

  tile_distortion_runs   decoded tiles + a clip + per tile the frames it is shown in -> the exact integer weighted squared error per
                         (tile, frame) and plane: one launch pair, every tile read and emitted once
  encode_clip_to_size    clip + tolerance -> (PCS2 container of at most target_bytes bytes, ClipTolRatePlan)
  decode_clip, frame_container, parse_clip   clip_rate's: nothing new is needed to decode

Why a kernel of its own.  clip_rate's reuse identity D(k, t) = D(f, t) holds because a reused tile's footprint is EQUAL in every frame
of its run; under a tolerance it is only close, so an item's distortion has to be measured against every frame that shows it.
clip_rate.tile_distortion_jobs can express that only with one copy of the decoded tile per frame, each read and emitted again; here
the tile's codes are held in registers and compared against each frame of the run.

The contract.  source is clip_tol.scan_clip's table for the given Tolerance; items and runs are clip_rate.items_of(source).
plane_dists[i][l][j][p] is frame_rate.frame_tile_distortion of item i = (f, t) decoded at level l against frame runs[i][j], plane p.
M (frame_scale) is the least common multiple of the denominators of Fraction(frame_weights[k]), fwi[k] = frame_weights[k] * M an int;
dists[i][l] = sum over j of fwi[runs[i][j]] * (wY, wCb, wCr) . plane_dists[i][l][j], Python ints; weights[i] = importance[t]
(a uniform scale of the distortions changes nothing, so M is not divided out); rates[i][l] the length of the item's single-level
PCB1 container; levels = rate.allocate(rates, dists, target_bytes - 42 - 16 * F * ny * nx, weights).  sse[k][p] is the sum over the
tiles t of frame k of plane_dists[i][levels[i]][j][p], i the item (source[k][t], t) and j the position of k in its run: at overlap 0
the exact SSE of the decoded frame k against the frame k that was shown, a reused tile's error against a frame it was not cut from
included.  predicted is that sum over all frames weighted by plane_weights, unweighted by frames, as clip_rate's.  With Tolerance()
the bytes, levels, rates, sse and predicted are clip_rate.encode_clip_to_size's; with Tolerance(max_run=1) those of reuse=False.

There is no CPU fallback: CPU tensors raise ValueError before any device call.  Everything runs on the current stream of the tensors'
device.  Out of scope: per-frame byte caps and constant bitrate, a target PSNR, inter-frame prediction, letting the allocation choose
where a run ends.
"""
import collections
import ctypes as C
from fractions import Fraction
from math import gcd

from . import _imagelib, _tilecodec
from ._lib import PC_OK
from .clip_rate import _allocate_and_pack, _to_size_arguments, decode_clip, frame_container, items_of, pack_clip, parse_clip  # noqa: F401
from .clip_tol import Tolerance, _scan, _tolerance
from .clips import ENTRY_BYTES, HEADER_BYTES, _clip_frames, _cut_of, _frame_table  # noqa: F401
from .frame_rate import max_tile  # noqa: F401
from .frames import FORMATS, RANGES, Frame, _check_enums, _frame_struct, coefficients
from .rate import allocate  # noqa: F401
from .tiles import TileGrid, _check_tiles, _fit_tiles, grid_of

LIB_PATH = _imagelib.lib_path("clip_tol_rate")

#: every symbol clip_tol_rate_hip/pc_clip_tol_rate.h declares
EXPORTS = ["pc_clip_tol_rate_workspace_size", "pc_clip_tol_rate_sse_runs", "pc_clip_tol_rate_plan", "pc_clip_tol_rate_strerror",
           "pc_clip_tol_rate_last_hip_error"]

_range = range                            # the functions below take a parameter of that name


def _prototypes():
    i64, vp, ci, cf, fp, ip = C.c_int64, C.c_void_p, C.c_int, C.c_float, C.POINTER(Frame), C.POINTER(C.c_int32)
    return {
        "pc_clip_tol_rate_workspace_size": (C.c_size_t, [ci, ci]),
        "pc_clip_tol_rate_sse_runs": (None, [vp, i64, i64, i64] + [ci] * 6 + [cf] * 5 + [fp, vp, ci, vp, ip, vp, vp, ci, ci, vp, C.c_size_t, vp, vp]),
        "pc_clip_tol_rate_plan": (None, [vp, i64, i64, i64, ci, ci, fp, ci, C.POINTER(ci)]),
        "pc_clip_tol_rate_strerror": (C.c_char_p, [ci]),
    }


def lib():
    return _imagelib.load(LIB_PATH, _prototypes)


class ClipTolRateError(_imagelib.ImageLibError):
    _lib, _prefix = staticmethod(lib), "pc_clip_tol_rate"


#: what encode_clip_to_size decided: source[k][t] (clip_tol.scan_clip's); items[i] = (f, t), the coded tiles in (f, t) order; runs[i],
#: the frames that show item i; weights[i] = importance[t] (Fractions); frame_scale = M, the least common multiple of the
#: denominators of the frame weights; levels[i]; rates[i][l]; dists[i][l] (the run's plane_dists weighted by plane_weights and by
#: M * frame_weights, exact ints); plane_dists[i][l][j] = [D_Y, D_Cb, D_Cr] against frame runs[i][j]; den (the band weights'
#: denominator per axis); container_bytes; predicted; sse[k][p] (at overlap 0 the decoded frame's exact SSE against frame k);
#: n_coded and n_reused (they add up to F * ny * nx); stats and worst as in clip_tol.ClipTolPlan
ClipTolRatePlan = collections.namedtuple("ClipTolRatePlan", "source items runs weights frame_scale levels rates dists plane_dists den "
                                         "container_bytes predicted sse n_coded n_reused stats worst")


# -- the kernel ----------------------------------------------------------------------------------------------------------------------

def _sse_runs_into(L, x, g, fmt, range, k, host, table, F, tiles_ptr, offsets_host, offsets_ptr, slots_ptr, n, ne, ws, nbytes, out, stream):
    rc = L.pc_clip_tol_rate_sse_runs(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), g.H, g.W, g.T, g.O, FORMATS[fmt], RANGES[range],
                                     k.kr, k.kg, k.kb, k.ib, k.ir, host, table.data_ptr(), F, tiles_ptr, offsets_host, offsets_ptr, slots_ptr,
                                     n, ne, ws.data_ptr(), nbytes, out.data_ptr(), stream)
    if rc != PC_OK:
        raise ClipTolRateError(rc, "pc_clip_tol_rate_sse_runs")


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _runs(tiles, runs, F, g):
    """-> (tiles, runs) as lists of ints and of lists of ints, checked against the F frames and the grid"""
    import torch
    ts = tiles.tolist() if torch.is_tensor(tiles) else list(tiles)
    rs = [list(r) if isinstance(r, (tuple, list)) else r for r in runs]
    if not ts:
        raise ValueError("tiles must name at least one tile")
    if len(rs) != len(ts):
        raise ValueError(f"runs needs one list of frames per tile, {len(ts)} in all, got {len(rs)}")
    for t, run in zip(ts, rs):
        if not _is_int(t):
            raise ValueError(f"a tile is an int, got {t!r}")
        if not isinstance(run, list) or not run or any(not _is_int(v) for v in run):
            raise ValueError(f"a run is a non-empty list of frame indices (ints), got {run!r}")
        if not 0 <= t < g.ny * g.nx or any(not 0 <= v < F for v in run):
            raise ValueError(f"tile {t!r} with run {run!r} lies outside the {F} frames or the {g.ny}x{g.nx} grid (row-major tile indices 0 .. "
                             f"{g.ny * g.nx - 1})")
    return ts, rs


def _offsets(runs):
    off = [0]
    for run in runs:
        off.append(off[-1] + len(run))
    return off


def tile_distortion_runs(x_hat_tiles, grid, frames, tiles, runs, fmt, matrix="bt709", range="limited"):
    """x_hat_tiles: float32 cuda [n,3,T,T] (any tile / channel / row strides, unit stride along a row); frames: a clip (a list of
    frames of grid's H x W, or one tuple of batched planes, any row strides); tiles[m]: an int, the tile of x_hat_tiles[m], row-major
    in grid's whole ny x nx grid, repeats allowed; runs[m]: a non-empty list of frame indices, in any order, repeats allowed (both
    validated here, on the host, before they are uploaded) -> (out, offsets): out int64 cuda [n_entries,3], offsets a Python list of
    n + 1 ints; row offsets[m] + j is clip_rate.tile_distortion_jobs' row for x_hat_tiles[m] and the job (runs[m][j], tiles[m]),
    exactly (pc_clip_tol_rate.h).  One launch pair; every tile is read and emitted once, however long its run."""
    import torch
    _check_enums(fmt, matrix, range)
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
        nbytes = L.pc_clip_tol_rate_workspace_size(g.T, ne)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        out = torch.empty((ne, 3), dtype=torch.int64, device=dev)
        _sse_runs_into(L, x, full, fmt, range, k, host, table, len(fs), words.data_ptr(), (C.c_int32 * (n + 1))(*off), words[n:].data_ptr(),
                       words[2 * n + 1:].data_ptr(), n, ne, ws, nbytes, out, torch.cuda.current_stream(dev).cuda_stream)
    del fs
    return out, off


def plan(x_hat_tiles, frames, fmt, overlap=0):
    """pc_clip_tol_rate_plan for tensors (host only, nothing is launched or copied): True where tile_distortion_runs of exactly these
    tensors with this overlap takes the wide-access path.  frames: a list of tuples of batched tensors ([1,...]) whose strides already
    fit a frame."""
    _check_enums(fmt)
    x = x_hat_tiles
    wide = C.c_int(-1)
    host = (Frame * len(frames))(*[_frame_struct(ts) for ts in frames])
    rc = lib().pc_clip_tol_rate_plan(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), int(overlap), FORMATS[fmt], host, len(frames),
                                     C.byref(wide))
    if rc != PC_OK:
        raise ClipTolRateError(rc, "pc_clip_tol_rate_plan")
    return bool(wide.value)


# -- the allocation's numbers ----------------------------------------------------------------------------------------------------------

def frame_scale(frame_weights, n_frames):
    """frame_weights (one positive number per frame, or None: all 1) -> (M, fwi): M the least common multiple of the denominators of
    Fraction(frame_weights[k]), fwi[k] = frame_weights[k] * M as ints"""
    fw = [Fraction(1)] * n_frames if frame_weights is None else [Fraction(v) for v in frame_weights]
    if len(fw) != n_frames or any(v <= 0 for v in fw):
        raise ValueError(f"frame_weights needs one positive number per frame, {n_frames} in all")
    M = 1
    for v in fw:
        M = M * v.denominator // gcd(M, v.denominator)
    return M, [int(v * M) for v in fw]


def item_importance(items, n_tiles, importance=None):
    """importance[t] of every item (f, t) as exact Fractions; the default is 1"""
    imp = [Fraction(1)] * n_tiles if importance is None else [Fraction(v) for v in importance]
    if len(imp) != n_tiles or any(v <= 0 for v in imp):
        raise ValueError(f"importance needs one positive number per tile, {n_tiles} in all")
    return [imp[t] for _, t in items]


# -- through the codec ---------------------------------------------------------------------------------------------------------------

def encode_clip_to_size(model, frames, qualities, target_bytes, fmt, matrix="bt709", range="limited", upsample="linear", tile=512,
                        overlap=0, mask_pol="point-based-std", tolerance=Tolerance(), plane_weights=(1, 1, 1), importance=None,
                        frame_weights=None, max_tiles_per_call=32):
    """clip -> (PCS2 container of at most target_bytes bytes, ClipTolRatePlan).  The argument checks are
    clip_rate.encode_clip_to_size's; the source table is clip_tol.scan_clip's under `tolerance` (one scan, one device-to-host copy of
    source and stats).  Then clip_rate's work loop over the coded tiles, chunked by max_tiles_per_call ACROSS frames -- the cut
    launches, model.compress_levels, model.decompress_levels, container.pack of a single level per item and level -- with one
    pc_clip_tol_rate_sse_runs call per level for the chunk's jobs: every decoded tile against every frame of its run (the frame
    table, the tile list, the offsets and the slots of the whole clip are uploaded once; one workspace, sized for the chunk with the
    most entries).  Every item then gets the level rate.allocate picks from the bytes each level costs and the distortion it leaves
    over its run (the planes weighted by plane_weights = (wY, wCb, wCr), non-negative ints; frame k by frame_weights[k], one positive
    number per frame), weighted by importance[t] (one positive number per tile, [ny][nx] or flat), under the budget
    target_bytes - 42 - 16 * F * ny * nx.  ValueError, its message holding the minimum, if the cheapest level of every item does not
    fit.  Neither the bytes nor the plan depend on max_tiles_per_call or on how the frames lie in memory; frame_container(buf, k) is a
    PCG1 container frame_tiles.decode_frame_tiled reads; decode_clip is clip_rate's."""
    import torch
    qualities, step, pw, target_bytes, fs, g, importance, frame_weights = _to_size_arguments(
        frames, qualities, target_bytes, fmt, matrix, range, upsample, tile, overlap, plane_weights, importance, frame_weights, max_tiles_per_call)
    tol = _tolerance(tolerance, fmt)
    n, F, nl = g.ny * g.nx, len(fs), len(qualities)
    M, fwi = frame_scale(frame_weights, F)
    per_tile = item_importance([(0, t) for t in _range(n)], n, importance)     # checked before the scan
    src, st = _scan(fs, fmt, g, upsample, tol)
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
        nbytes = L.pc_clip_tol_rate_workspace_size(g.T, most)
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
                _sse_runs_into(L, xh, g, fmt, range, k, host, table, F, words[a:].data_ptr(), host_off, words[at_offsets[c]:].data_ptr(),
                               words[at_slots + off[a]:].data_ptr(), b, ne, ws, nbytes, d[l], stream)
            d = d.tolist()                                                     # [levels][entries][3]; synchronises: xh may go
        return [[[[int(v) for v in d[l][e]] for e in _range(off[a + m] - off[a], off[a + m + 1] - off[a])] for l in _range(nl)]
                for m in _range(b)]
    bufs, plane_dists = _tilecodec.encode_items(model, len(items), step, qualities, mask_pol, g.T,
                                                _cut_of(fs, g, items, fmt, matrix, range, upsample), measure)
    del fs
    dists = [[sum(fwi[f] * (pw[0] * v[0] + pw[1] * v[1] + pw[2] * v[2]) for f, v in zip(run, per_frame)) for per_frame in row]
             for run, row in zip(runs, plane_dists)]
    buf, levels, rates = _allocate_and_pack(bufs, dists, weights, items, source, target_bytes, g, fmt, matrix, range, upsample)
    chosen = [plane_dists[i][levels[i]] for i in _range(len(items))]                                   # [i][j][p]
    sse = [[0, 0, 0] for _ in _range(F)]
    predicted = 0
    for run, per_frame in zip(runs, chosen):
        for f, v in zip(run, per_frame):
            for p in _range(3):
                sse[f][p] += v[p]
            predicted += pw[0] * v[0] + pw[1] * v[1] + pw[2] * v[2]
    return buf, ClipTolRatePlan(source, items, runs, weights, M, levels, rates, dists, plane_dists, 2 * g.O if g.O else 1, len(buf), predicted,
                                sse, len(items), F * n - len(items), stats, worst)

"""Tolerant clips of YUV 4:2:0 frames (libpc_clip_tol.so, clip_tol_csrc/pc_clip_tol.h): clips.py codes a tile
once while its footprint holds the SAME codes frame after frame, which is true of screen content and of nothing a camera or a video
decoder hands over -- one code of noise anywhere in the footprint recodes the tile.  Here a tile is coded once while its footprint
stays CLOSE to the frame it was last coded in (its anchor): within max_abs codes sample by sample, within max_mse on the footprint's
mean, and for at most max_run frames.  The comparison is against the anchor, never against the previous frame, so the error of a
reused tile against its source is bounded by the tolerance however long the run: a fade of one code per frame is recoded every
max_abs + 1 frames.  The decision for frame k depends on the decision for frame k - 1; it is taken on the device, so the scan of a
whole clip is one call without a host synchronisation.

  Tolerance      max_abs, max_mse, max_run -> the seven integers of the contract
  scan_clip      clip + tolerance -> (source int32 [F, n], stats int64 [F, n, 3, 3]) on the device: one table upload, one C call
  encode_clip    clip + tolerance -> (PCS1 container, ClipTolPlan): one scan, one device-to-host copy, then clips.encode_clip's
                 work loop over the scan's source table

The product is an ordinary PCS1 container: clips.decode_clip, clips.frame_container and frame_tiles.decode_frame_tiled read it
unchanged, and nothing new is needed to decode.

The contract (pc_clip_tol.h).  Geometry and footprint are clips.py's.  The difference of tile t between two frames is, per plane
(Y, Cb, Cr) over the tile's footprint, every sample once: count (the samples whose codes differ), sse (the sum of squared code
differences) and maxabs (the largest absolute one).  A tile is close iff for every plane maxabs <= max_abs and
1024 * sse <= mse_q10 * nsamp (nsamp: the samples of the footprint in that plane; integers, no division).  anchor[t] = 0 and
source[0][t] = 0; for k = 1 .. F - 1 in order, stats[k][t] is the difference of frame k and frame anchor[t]; the tile is reused iff
it is close and (max_run == 0 or k - anchor[t] + 1 <= max_run), and then source[k][t] = anchor[t]; otherwise source[k][t] = k and
anchor[t] = k.  stats[0] is all zeros.  With the all-zero tolerance and no max_run, source is clips.encode_clip's; with max_run = 1
every tile is coded (reuse=False).

There is no CPU fallback: CPU tensors raise ValueError before any device call.  Everything runs on the current stream of the tensors'
device.  Out of scope: a tolerance inside clip_rate.encode_clip_to_size (its reuse identity D(k, t) = D(f, t) does not hold for a
tile that is only close; clip_tol_rate.encode_clip_to_size measures every frame of a run and is that encoder),
inter-frame prediction, matching a tile against other tiles.  4:2:2 / 4:4:4 and left- / top-left-sited frames: chroma_clip_tol.py
(DESIGN.md section 29), this module for the twelve formats and three sitings of `chroma`.
"""
import collections
import ctypes as C
from fractions import Fraction

from . import clips
from . import _imagelib, _tilecodec
from ._lib import PC_OK
from .clips import _clip_frames, _encode_source, _frame_table
from .frames import FORMATS, UPSAMPLES, Frame, _check_enums, _frame_struct, bits_of

LIB_PATH = _imagelib.lib_path("clip_tol")

#: every symbol clip_tol_csrc/pc_clip_tol.h declares
EXPORTS = ["pc_clip_tol_workspace_size", "pc_clip_tol_scan", "pc_clip_tol_plan", "pc_clip_tol_strerror", "pc_clip_tol_last_hip_error"]

NO_MSE = 1 << 30                          # pc_clip_tol.h: the mse_q10 that never binds
MAX_BITS = 10                             # P010

_range = range                            # the functions below take a parameter of that name


def _prototypes():
    vp, ci, fp, ip = C.c_void_p, C.c_int, C.POINTER(Frame), C.POINTER(C.c_int)
    return {
        "pc_clip_tol_workspace_size": (C.c_size_t, [ci, ci]),
        "pc_clip_tol_scan": (None, [fp, vp] + [ci] * 7 + [ip, ip, ci, vp, C.c_size_t, vp, vp, vp]),
        "pc_clip_tol_plan": (None, [ci, fp, ci, ci, ip]),
        "pc_clip_tol_strerror": (C.c_char_p, [ci]),
    }


def lib():
    return _imagelib.load(LIB_PATH, _prototypes)


class ClipTolError(_imagelib.ImageLibError):
    _lib, _prefix = staticmethod(lib), "pc_clip_tol"


def _three(v, what):
    vals = list(v) if isinstance(v, (tuple, list)) else [v] * 3
    if len(vals) != 3:
        raise ValueError(f"{what} is one number or three (Y, Cb, Cr), got {v!r}")
    return vals


class Tolerance(collections.namedtuple("Tolerance", "max_abs mse_q10 max_run")):
    """Tolerance(max_abs=0, max_mse=None, max_run=None) -> (max_abs (three ints), mse_q10 (three ints), max_run (int)): the seven
    integers of the contract.  Scalars stand for all three planes (Y, Cb, Cr).  max_abs: ints in [0, 1023] (the scan refuses a value
    above the format's top code).  max_mse: in code^2, taken exactly -- mse_q10 = floor(Fraction(max_mse) * 1024), which must lie in
    [0, 2^30]; None is 2^30, "no condition" (1023^2 * 1024 < 2^30).  max_run: the largest number of frames one coded tile may be
    shown in, at least 1; None (stored as 0) is unlimited.  ValueError for everything else."""
    __slots__ = ()

    def __new__(cls, max_abs=0, max_mse=None, max_run=None):
        ma = _three(max_abs, "max_abs")
        for v in ma:
            if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 1 << MAX_BITS:
                raise ValueError(f"max_abs must be ints in [0, {(1 << MAX_BITS) - 1}], got {max_abs!r}")
        q10 = []
        for v in _three(max_mse, "max_mse"):
            if v is None:
                q10.append(NO_MSE)
                continue
            try:
                if isinstance(v, bool):
                    raise TypeError
                q = Fraction(v) * 1024
            except (TypeError, ValueError, OverflowError):
                raise ValueError(f"max_mse must be None or numbers whose 1024-fold lies in [0, 2^30], got {max_mse!r}") from None
            q = q.numerator // q.denominator
            if not 0 <= q <= NO_MSE:
                raise ValueError(f"max_mse must be None or numbers whose 1024-fold lies in [0, 2^30], got {max_mse!r}")
            q10.append(q)
        if max_run is None:
            run = 0
        elif isinstance(max_run, bool) or not isinstance(max_run, int) or not 1 <= max_run < 1 << 31:
            raise ValueError(f"max_run must be None (unlimited) or an int of at least 1, got {max_run!r}")
        else:
            run = max_run
        return super().__new__(cls, tuple(ma), tuple(q10), run)


def _tolerance(tolerance, fmt):
    tol = tolerance if isinstance(tolerance, Tolerance) else None
    if tol is None:
        raise ValueError(f"tolerance must be a clip_tol.Tolerance, got {tolerance!r}")
    top = (1 << bits_of(fmt)) - 1
    if max(tol.max_abs) > top:
        raise ValueError(f"max_abs must be at most {top} for {fmt!r}, got {tol.max_abs!r}")
    return tol


#: what encode_clip decided: source, n_coded, n_reused, container_bytes (clips.ClipPlan's); stats[k][t][p] = [count, sse, maxabs] of
#: tile t of frame k against the frame it was anchored in when frame k was scanned (the evidence, for reused and recoded tiles alike;
#: all zeros in frame 0); worst[p], the largest maxabs of plane p over the REUSED (k, t) -- the bound that actually held (0 where
#: nothing was reused)
ClipTolPlan = collections.namedtuple("ClipTolPlan", "source n_coded n_reused container_bytes stats worst")


def _scan(fs, fmt, g, upsample, tol):
    """scan_clip on checked arguments: fs[k] the planes of frame k as batched views"""
    import torch
    dev = fs[0][0].device
    n, F = g.ny * g.nx, len(fs)
    L = lib()
    with torch.cuda.device(dev):
        host, table = _frame_table(fs, dev)
        nbytes = L.pc_clip_tol_workspace_size(g.T, n)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        source = torch.empty((F, n), dtype=torch.int32, device=dev)
        stats = torch.empty((F, n, 3, 3), dtype=torch.int64, device=dev)
        rc = L.pc_clip_tol_scan(host, table.data_ptr(), F, FORMATS[fmt], UPSAMPLES[upsample], g.H, g.W, g.T, g.O, (C.c_int * 3)(*tol.max_abs),
                                (C.c_int * 3)(*tol.mse_q10), tol.max_run, ws.data_ptr(), nbytes, source.data_ptr(), stats.data_ptr(),
                                torch.cuda.current_stream(dev).cuda_stream)
        if rc != PC_OK:
            raise ClipTolError(rc, "pc_clip_tol_scan")
    return source, stats


def scan_clip(frames, fmt, tolerance, tile=512, overlap=0, upsample="linear"):
    """a clip of F frames (a list of frames or batched planes, as clips._clip_frames takes them) and a Tolerance ->
    (source int32 cuda [F, n], stats int64 cuda [F, n, 3, 3]) over the n = ny * nx tiles: the scan of the contract.  One upload of the
    frame table and one C call (1 + 2 (F - 1) launches on the current stream); no host synchronisation.  The stats are PER TILE: with
    overlap > 0, or under linear upsampling (the halo), footprints overlap, so the stats of a frame's tiles are not a partition of the
    frame and do not add up to the frame's."""
    _check_enums(fmt, upsample=upsample)
    tol = _tolerance(tolerance, fmt)
    fs, H, W = _clip_frames(frames, fmt)
    g = clips._grid(H, W, tile, overlap)
    return _scan(fs, fmt, g, upsample, tol)


def plan(frames, fmt, overlap=0):
    """pc_clip_tol_plan for tensors (host only, nothing is launched or copied): True where scan_clip of exactly these tensors with
    this overlap takes the wide-access path.  frames: a list of tuples of batched tensors ([1,...]) whose strides already fit a frame."""
    _check_enums(fmt)
    wide = C.c_int(-1)
    host = (Frame * len(frames))(*[_frame_struct(ts) for ts in frames])
    rc = lib().pc_clip_tol_plan(FORMATS[fmt], host, len(frames), int(overlap), C.byref(wide))
    if rc != PC_OK:
        raise ClipTolError(rc, "pc_clip_tol_plan")
    return bool(wide.value)


def encode_clip(model, frames, qualities, fmt, matrix="bt709", range="limited", upsample="linear", tile=512, overlap=0,
                mask_pol="point-based-std", tolerance=Tolerance(), max_tiles_per_call=32):
    """clip -> (PCS1 container (bytes), ClipTolPlan) holding every level of `qualities` for every tile of every frame: clips.encode_clip
    with the source table of scan_clip under `tolerance` (one scan, one device-to-host copy of source and stats) and then exactly
    its work loop -- the coded tiles chunked by max_tiles_per_call across frames, one cut launch per frame present in a chunk,
    model.compress_levels, container.pack.  A coded tile is coded from its OWN frame, losslessly as far as this layer goes; a reused
    (k, t) shows the bytes of frame source[k][t], whose footprint lies within the tolerance of frame k's.  plan.stats is the evidence
    per (k, t) and plan.worst[p] the largest maxabs of plane p over the reused ones.  The stats are PER TILE: with overlap > 0, or a
    halo, footprints overlap, so they are not a partition of the frame.  With Tolerance() the bytes are clips.encode_clip's.  The bytes
    depend neither on max_tiles_per_call nor on how the frames are laid out in memory; clips.decode_clip reads the container."""
    qualities = [float(q) for q in qualities]
    _check_enums(fmt, matrix, range, upsample)
    tol = _tolerance(tolerance, fmt)
    step = _tilecodec.tiles_per_call(max_tiles_per_call)
    fs, H, W = _clip_frames(frames, fmt)
    g = clips._grid(H, W, tile, overlap)
    n, F = g.ny * g.nx, len(fs)
    src, st = _scan(fs, fmt, g, upsample, tol)
    import torch
    both = torch.cat([src.to(torch.int64).reshape(F, n, 1), st.reshape(F, n, 9)], dim=2).cpu()         # the one copy
    source, stats = both[:, :, 0].tolist(), both[:, :, 1:].reshape(F, n, 3, 3).tolist()
    worst = [max([stats[k][t][p][2] for k in _range(F) for t in _range(n) if source[k][t] != k], default=0) for p in _range(3)]
    buf, n_coded = _encode_source(model, fs, g, source, qualities, fmt, matrix, range, upsample, mask_pol, step)
    return buf, ClipTolPlan(source, n_coded, F * n - n_coded, len(buf), stats, worst)

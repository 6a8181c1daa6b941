"""Tolerant clips of YUV frames of any chroma subsampling and siting (libpc_chroma_clip_tol.so, chroma_clip_tol_gpu/pc_chroma_clip_tol.h;
DESIGN.md section 29): what `clip_tol` is for NV12 / I420 / P010 with centre-sited chroma, for the twelve formats and three sitings of
`chroma`.  chroma_clips.py codes a tile once while its footprint holds the SAME codes frame after frame; one code of camera or decoder
noise anywhere in the footprint recodes the tile.  Here a tile is coded once while its footprint stays CLOSE to the frame it was last
coded in (its anchor): within max_abs codes sample by sample, within max_mse on the footprint's mean, and for at most max_run frames.
The comparison is against the anchor, never against the previous frame, so the error of a reused tile against its source is bounded
by the tolerance however long the run.  The decision is taken on the device: the scan of a whole clip is one call without a host
synchronisation.  No body is restated here: Tolerance and ClipTolPlan are clip_tol's, the frames, the grid and the work loop
chroma_clips', the frame table clips'.

  Tolerance      clip_tol.Tolerance: max_abs, max_mse, max_run -> the seven integers of the contract
  scan_clip      clip + tolerance -> (source int32 [F, n], stats int64 [F, n, 3, 3]) on the device: one table upload, one C call
  plan           host only: whether scan_clip of these tensors takes the wide-access path
  encode_clip    clip + tolerance -> (PCL1 container, ClipTolPlan): one scan, one device-to-host copy, then chroma_clips.encode_clip's
                 work loop over the scan's source table

The product is an ordinary PCL1 container: chroma_clips.decode_clip, chroma_clips.frame_container and
chroma_tiles.decode_frame_tiled read it unchanged, and nothing new is needed to decode.

The contract (pc_chroma_clip_tol.h).  Geometry and footprint are chroma_clips.py's: the footprint depends on the format, the siting
and the upsampling.  Codes are (element >> shift) & (2^bits - 1).  The difference of tile t between two frames is, per plane (Y, Cb,
Cr) over the tile's footprint, every sample once: count (the samples whose codes differ), sse (the sum of squared code differences)
and maxabs (the largest absolute one).  A tile is close iff for every plane maxabs <= max_abs and 1024 * sse <= mse_q10 * nsamp
(nsamp: the samples of the footprint in that plane under this format, siting and upsampling; integers, no division).  anchor[t] = 0
and source[0][t] = 0; for k = 1 .. F - 1 in order, stats[k][t] is the difference of frame k and frame anchor[t]; the tile is reused
iff it is close and (max_run == 0 or k - anchor[t] + 1 <= max_run), and then source[k][t] = anchor[t]; otherwise source[k][t] = k and
anchor[t] = k.  stats[0] is all zeros.  With the all-zero tolerance and no max_run, source is chroma_clips.encode_clip's; with
max_run = 1 every tile is coded (reuse=False).  For "nv12", "i420" and "p010" at "centre" everything is clip_tol's, bit for bit.

There is no CPU fallback: CPU tensors raise ValueError before any device call.  Everything runs on the current stream of the tensors'
device.  The same tolerance under a byte budget is the layer above this one (chroma_clip_tol_rate.py, DESIGN.md section 30: what
clip_tol_rate.py is to clip_rate.py).  Out of scope: inter-frame prediction, matching a tile against other tiles.
"""
import ctypes as C

from . import _imagelib, _tilecodec
from ._lib import PC_OK
from .chroma import FORMATS, SITINGS, _check_enums
from .chroma_clips import _clip_frames, _encode_source, _grid
from .clip_tol import NO_MSE, ClipTolPlan, Tolerance  # noqa: F401
from .clips import _frame_table
from .frames import UPSAMPLES, Frame, _frame_struct

LIB_PATH = _imagelib.lib_path("chroma_clip_tol")

#: every symbol chroma_clip_tol_gpu/pc_chroma_clip_tol.h declares
EXPORTS = ["pc_chroma_clip_tol_workspace_size", "pc_chroma_clip_tol_scan", "pc_chroma_clip_tol_plan", "pc_chroma_clip_tol_strerror",
           "pc_chroma_clip_tol_last_hip_error"]

_range = range                            # the functions below take a parameter of that name


def _prototypes():
    vp, ci, fp, ip = C.c_void_p, C.c_int, C.POINTER(Frame), C.POINTER(C.c_int)
    return {
        "pc_chroma_clip_tol_workspace_size": (C.c_size_t, [ci, ci, ci]),
        "pc_chroma_clip_tol_scan": (None, [fp, vp] + [ci] * 13 + [ip, ip, ci, vp, C.c_size_t, vp, vp, vp]),
        "pc_chroma_clip_tol_plan": (None, [ci, ci, ci, fp, ci, ci, ip]),
        "pc_chroma_clip_tol_strerror": (C.c_char_p, [ci]),
    }


def lib():
    return _imagelib.load(LIB_PATH, _prototypes)


class ChromaClipTolError(_imagelib.ImageLibError):
    _lib, _prefix = staticmethod(lib), "pc_chroma_clip_tol"


def _tolerance(tolerance, fmt):
    tol = tolerance if isinstance(tolerance, Tolerance) else None
    if tol is None:
        raise ValueError(f"tolerance must be a clip_tol.Tolerance, got {tolerance!r}")
    top = (1 << FORMATS[fmt].bits) - 1
    if max(tol.max_abs) > top:
        raise ValueError(f"max_abs must be at most {top} for {fmt!r}, got {tol.max_abs!r}")
    return tol


def _scan(fs, fmt, siting, g, upsample, tol):
    """scan_clip on checked arguments: fs[k] the planes of frame k as batched views"""
    import torch
    dev = fs[0][0].device
    n, F = g.ny * g.nx, len(fs)
    L = lib()
    with torch.cuda.device(dev):
        host, table = _frame_table(fs, dev)
        nbytes = L.pc_chroma_clip_tol_workspace_size(g.T, FORMATS[fmt].sy, n)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        source = torch.empty((F, n), dtype=torch.int32, device=dev)
        stats = torch.empty((F, n, 3, 3), dtype=torch.int64, device=dev)
        rc = L.pc_chroma_clip_tol_scan(host, table.data_ptr(), F, *FORMATS[fmt], *SITINGS[siting], UPSAMPLES[upsample], g.H, g.W, g.T, g.O,
                                       (C.c_int * 3)(*tol.max_abs), (C.c_int * 3)(*tol.mse_q10), tol.max_run, ws.data_ptr(), nbytes,
                                       source.data_ptr(), stats.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        if rc != PC_OK:
            raise ChromaClipTolError(rc, "pc_chroma_clip_tol_scan")
    return source, stats


def scan_clip(frames, fmt, tolerance, siting="centre", tile=512, overlap=0, upsample="linear"):
    """a clip of F frames (a list of frames or batched planes, as chroma_clips takes them) and a Tolerance -> (source int32 cuda
    [F, n], stats int64 cuda [F, n, 3, 3]) over the n = ny * nx tiles: the scan of the contract over the footprint of `fmt`, `siting`
    and `upsample`.  One upload of the frame table and one C call (1 + 2 (F - 1) launches on the current stream); no host
    synchronisation.  The stats are PER TILE: with overlap > 0, or a halo, footprints overlap, so the stats of a frame's tiles are not
    a partition of the frame and do not add up to the frame's."""
    _check_enums(fmt, upsample=upsample, siting=siting)
    tol = _tolerance(tolerance, fmt)
    fs, H, W = _clip_frames(frames, fmt)
    g = _grid(H, W, tile, overlap)
    return _scan(fs, fmt, siting, g, upsample, tol)


def plan(frames, fmt, overlap=0):
    """pc_chroma_clip_tol_plan for tensors (host only, nothing is launched or copied): True where scan_clip of exactly these tensors
    with this overlap takes the wide-access path -- every frame of the table has to allow it.  frames: a list of tuples of batched
    tensors ([1,...]) whose strides already fit a frame."""
    _check_enums(fmt)
    f = FORMATS[fmt]
    wide = C.c_int(-1)
    host = (Frame * len(frames))(*[_frame_struct(ts) for ts in frames])
    rc = lib().pc_chroma_clip_tol_plan(f.layout, f.bits, f.sx, host, len(frames), int(overlap), C.byref(wide))
    if rc != PC_OK:
        raise ChromaClipTolError(rc, "pc_chroma_clip_tol_plan")
    return bool(wide.value)


def encode_clip(model, frames, qualities, fmt, matrix="bt709", range="limited", upsample="linear", siting="centre", tile=512, overlap=0,
                mask_pol="point-based-std", tolerance=Tolerance(), max_tiles_per_call=32):
    """clip -> (PCL1 container (bytes), ClipTolPlan) holding every level of `qualities` for every tile of every frame:
    chroma_clips.encode_clip with the source table of scan_clip under `tolerance` (one scan, one device-to-host copy of source and
    stats) and then exactly its work loop -- the coded tiles chunked by max_tiles_per_call across frames, one cut launch per frame
    present in a chunk, model.compress_levels, container.pack.  A coded tile is coded from its OWN frame; a reused (k, t) shows the
    bytes of frame source[k][t], whose footprint lies within the tolerance of frame k's.  plan.stats is the evidence per (k, t) and
    plan.worst[p] the largest maxabs of plane p over the reused ones.  With Tolerance() the bytes are chroma_clips.encode_clip's.  The
    bytes depend neither on max_tiles_per_call nor on how the frames are laid out in memory; chroma_clips.decode_clip reads the
    container."""
    qualities = [float(q) for q in qualities]
    _check_enums(fmt, matrix, range, upsample, siting)
    tol = _tolerance(tolerance, fmt)
    step = _tilecodec.tiles_per_call(max_tiles_per_call)
    fs, H, W = _clip_frames(frames, fmt)
    g = _grid(H, W, tile, overlap)
    n, F = g.ny * g.nx, len(fs)
    src, st = _scan(fs, fmt, siting, g, upsample, tol)
    import torch
    both = torch.cat([src.to(torch.int64).reshape(F, n, 1), st.reshape(F, n, 9)], dim=2).cpu()         # the one copy
    source, stats = both[:, :, 0].tolist(), both[:, :, 1:].reshape(F, n, 3, 3).tolist()
    worst = [max([stats[k][t][p][2] for k in _range(F) for t in _range(n) if source[k][t] != k], default=0) for p in _range(3)]
    buf, n_coded = _encode_source(model, fs, g, source, qualities, fmt, matrix, range, upsample, siting, mask_pol, step)
    return buf, ClipTolPlan(source, n_coded, F * n - n_coded, len(buf), stats, worst)

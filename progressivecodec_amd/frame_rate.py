"""Rate-controlled tiled coding of YUV 4:2:0 frames (libpc_frame_rate.so, frame_rate_csrc/pc_frame_rate.h): one
NV12 / I420 / P010 frame in at most N bytes, every tile at the level of the quality list that rate.allocate picks for it, judged in
the frame's own codes.  The composition of rate.py (section 12: the allocator, PCT2) and frame_tiles.py (section 14: the cut, PCG1).

  frame_tile_distortion        decoded tiles + the original frame -> the exact integer weighted squared error per tile and plane
                               (Y, Cb, Cr codes at the format's bit depth, 4:2:0 chroma), one pass over the tiles on the GPU
  encode_frame_tiled_to_size   frame -> (PCG1 container of at most target_bytes bytes holding a PCT2 container, FrameRatePlan);
                               frame_tiles.decode_frame_tiled reads it

Distortion.  A tile is judged by its OWN rendering: section 13's emit on the tile with its in-frame part as the picture, compared
with the original's codes (P010: word >> 6).  A luma sample counts with the integer numerators ay * ax of the stitch's band weights
over den = 2 * overlap (den = 1 without overlap), a chroma sample with cy * cx, cy(k) = (ay(2k) + ay(2k+1)) / 2: per sample of the
frame they sum to den^2 exactly, so sum_t D_t / den^2 is the squared code error of the decoded frame where tiles do not overlap -- at
overlap 0 exactly what frame_tiles.stitch_frame(..., ref=...) reports, per plane -- and bounds the blended error from above, up to
the quantiser, where they do.

There is no CPU fallback: CPU tensors raise ValueError before any device call.  Everything runs on the current stream of the tensor's
device.  Sequences of frames are clips.py's (without rate control) and clip_rate.py's (a clip in at most N bytes).  Out of scope: a
target PSNR (the dual problem), perceptual metrics, compress_with_ac.  4:2:2 / 4:4:4 and left- / top-left-sited chroma are chroma_rate.py's
(section 24), which computes these sums bit for bit for the three formats here.
"""
import collections
import ctypes as C

from . import _imagelib, _tilecodec
from ._lib import PC_OK
from ._tilecodec import max_tile  # noqa: F401
from .frame_tiles import HEADER_BYTES as FRAME_HEADER_BYTES
from .frame_tiles import FrameTilesError, _one_frame, pack_frame_tiled
from .frames import FORMATS, RANGES, UPSAMPLES, Frame, _check_enums, _frame_struct, coefficients
from .rate import TABLE_ENTRY_BYTES, allocate
from .tiles import HEADER_BYTES, TileGrid, _check_tiles, _fit_tiles, grid_of, pack_tiled

LIB_PATH = _imagelib.lib_path("frame_rate")

#: every symbol frame_rate_csrc/pc_frame_rate.h declares
EXPORTS = ["pc_frame_rate_workspace_size", "pc_frame_rate_tile_sse", "pc_frame_rate_plan", "pc_frame_rate_strerror",
           "pc_frame_rate_last_hip_error"]

_range = range                            # the functions below take a parameter of that name


def _prototypes():
    i64, vp, ci, cf, fp = C.c_int64, C.c_void_p, C.c_int, C.c_float, C.POINTER(Frame)
    return {
        "pc_frame_rate_workspace_size": (C.c_size_t, [ci, ci]),
        "pc_frame_rate_tile_sse": (None, [vp, i64, i64, i64] + [ci] * 8 + [cf] * 5 + [fp, vp, C.c_size_t, vp, vp]),
        "pc_frame_rate_plan": (None, [vp, i64, i64, i64, ci, ci, fp, C.POINTER(ci)]),
        "pc_frame_rate_strerror": (C.c_char_p, [ci]),
    }


def lib():
    return _imagelib.load(LIB_PATH, _prototypes)


class FrameRateError(_imagelib.ImageLibError):
    _lib, _prefix = staticmethod(lib), "pc_frame_rate"


#: what encode_frame_tiled_to_size decided: levels[t] (index into the quality list), rates[t][l] (bytes tile t costs at level l, its
#: table entry included), dists[t][l] (plane_dists weighted by plane_weights), plane_dists[t][l] = [D_Y, D_Cb, D_Cr]
#: (frame_tile_distortion), den (the weights' denominator per axis), container_bytes (the length of the container), predicted (the
#: sum of the chosen dists) and sse[p] (the sum of the chosen plane_dists per plane: at overlap 0 the decoded frame's exact SSE)
FrameRatePlan = collections.namedtuple("FrameRatePlan", "levels rates dists plane_dists den container_bytes predicted sse")


def frame_tile_distortion(x_hat_tiles, grid, ref, fmt, matrix="bt709", range="limited", first_tile=0):
    """x_hat_tiles: float32 cuda [n,3,T,T], the decoded tiles first_tile .. first_tile + n - 1 of grid's row-major ny x nx grid (a
    linear range, not a rectangle; grid's own rectangle is ignored; any tile / channel / row strides, unit stride along a row), ref: the
    whole original H x W frame in `fmt` (frames.py's tuple of planes, any row strides) -> int64 cuda [n,3]: per tile and plane
    [Y, Cb, Cr] the sum over the tile's samples inside the frame of weight * (code - refcode)^2, exact (pc_frame_rate.h).  A tile's
    sums do not depend on which range it is part of."""
    import torch
    _check_enums(fmt, matrix, range)
    g = TileGrid(*grid)
    full = grid_of(g.H, g.W, g.T, g.O)
    if (full.ny, full.nx) != (g.ny, g.nx):
        raise ValueError(f"{g}: the grid of a {g.H}x{g.W} frame is {full.ny}x{full.nx}")
    _tilecodec.tile_limit(g.T, fmt)
    x = x_hat_tiles
    n = int(x.shape[0]) if torch.is_tensor(x) and x.dim() == 4 else 0
    first_tile = int(first_tile)
    if n < 1 or first_tile < 0 or first_tile + n > full.ny * full.nx:
        raise ValueError(f"tiles {first_tile} .. {first_tile + n - 1} lie outside the {full.ny}x{full.nx} grid"
                         if n else "x_hat_tiles must be a [n,3,T,T] tensor with n >= 1")
    _check_tiles(x, full._replace(nty=1, ntx=n))
    rts, rH, rW = _one_frame(ref, fmt, "ref")
    if (rH, rW) != (g.H, g.W) or rts[0].device != x.device:
        raise ValueError(f"ref must be the {g.H}x{g.W} frame on {x.device}, got {rH}x{rW} on {rts[0].device}")
    if x.device.type != "cuda":
        raise ValueError(f"x_hat_tiles must be on a GPU (there is no CPU fallback), got {x.device}")
    x = _fit_tiles(x, g.T)
    k = coefficients(matrix)
    L = lib()
    rst = _frame_struct(rts)
    with torch.cuda.device(x.device):
        nbytes = L.pc_frame_rate_workspace_size(g.T, n)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=x.device)
        out = torch.empty((n, 3), dtype=torch.int64, device=x.device)
        rc = L.pc_frame_rate_tile_sse(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), g.H, g.W, g.T, g.O, first_tile, n,
                                      FORMATS[fmt], RANGES[range], k.kr, k.kg, k.kb, k.ib, k.ir, C.byref(rst), ws.data_ptr(), nbytes,
                                      out.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream)
    del rts
    if rc != PC_OK:
        raise FrameRateError(rc, "pc_frame_rate_tile_sse")
    return out


def plan(x_hat_tiles, ref, fmt, overlap=0):
    """pc_frame_rate_plan for tensors (host only, nothing is launched or copied): True where frame_tile_distortion of exactly these
    tensors with this overlap takes the wide-access path.  ref is a tuple of batched tensors ([1,...]) whose strides already fit a
    frame."""
    _check_enums(fmt)
    x = x_hat_tiles
    wide = C.c_int(-1)
    rf = _frame_struct(ref)
    rc = lib().pc_frame_rate_plan(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), int(overlap), FORMATS[fmt], C.byref(rf), C.byref(wide))
    if rc != PC_OK:
        raise FrameRateError(rc, "pc_frame_rate_plan")
    return bool(wide.value)


def encode_frame_tiled_to_size(model, planes, qualities, target_bytes, fmt, matrix="bt709", range="limited", upsample="linear", tile=512,
                               overlap=0, mask_pol="point-based-std", plane_weights=(1, 1, 1), importance=None, max_tiles_per_call=32):
    """frame -> (PCG1 container of at most target_bytes bytes, FrameRatePlan): every tile at the level of `qualities` that
    rate.allocate picks from the bytes each level costs (the tile's single-level PCB1 container plus its table entry) and the
    distortion it leaves (frame_tile_distortion of the tile decoded at that level, the planes weighted by plane_weights = (wY, wCb,
    wCr), non-negative ints; the default is the total squared code error over all samples), optionally weighted by importance
    ([ny][nx] or a flat list, one positive number per tile).  ValueError if even the cheapest level of every tile does not fit.  The
    tiles are cut, coded at every level (compress_levels), decoded again (decompress_levels) and measured max_tiles_per_call at a
    time, so a call holds at most max_tiles_per_call * (1 + len(qualities)) tile tensors on the device; neither the bytes nor the
    plan depend on it.  The container holds a PCT2 container (one level per tile); frame_tiles.decode_frame_tiled reads it."""
    import torch
    from . import frame_tiles
    qualities = _tilecodec.levels_of(qualities)
    _check_enums(fmt, matrix, range, upsample)
    step = _tilecodec.tiles_per_call(max_tiles_per_call)
    pw = _tilecodec.plane_weights_of(plane_weights)
    target_bytes = int(target_bytes)
    ts, H, W = _one_frame(planes, fmt, "planes")
    g = grid_of(H, W, tile, overlap)
    _tilecodec.tile_limit(g.T, fmt)
    n = g.ny * g.nx
    importance = _tilecodec.importance_of(importance, g)
    k = coefficients(matrix)
    dev = ts[0].device
    src = _frame_struct(ts)
    CL = frame_tiles.lib()

    def cut(a, b):
        with torch.cuda.device(dev):
            x = torch.empty((b, 3, g.T, g.T), dtype=torch.float32, device=dev)
            m0 = 0
            for i, j, m in _tilecodec.row_pieces(a, b, g.nx):
                rc = CL.pc_frame_tiles_cut(C.byref(src), FORMATS[fmt], RANGES[range], UPSAMPLES[upsample], k.a, k.b, k.c, k.d, H, W, g.T,
                                           g.O, i, j, 1, m, x[m0:].data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
                if rc != PC_OK:
                    raise FrameTilesError(rc, "pc_frame_tiles_cut")
                m0 += m
        return x

    def measure(a, b, decoded):
        d = torch.stack([frame_tile_distortion(o["x_hat"], g, ts, fmt, matrix, range, a) for o in decoded], 1).tolist()     # [b][levels][3]
        return [[[int(v) for v in row] for row in per_level] for per_level in d]
    bufs, plane_dists = _tilecodec.encode_items(model, n, step, qualities, mask_pol, g.T, cut, measure)
    del ts
    rates = [[TABLE_ENTRY_BYTES + len(p) for p in row] for row in bufs]
    dists = [[pw[0] * v[0] + pw[1] * v[1] + pw[2] * v[2] for v in row] for row in plane_dists]
    levels = allocate(rates, dists, target_bytes - FRAME_HEADER_BYTES - HEADER_BYTES, importance)
    inner = pack_tiled([bufs[t][levels[t]] for t in _range(n)], g.H, g.W, g.T, g.O, per_tile_levels=True)
    buf = pack_frame_tiled(inner, fmt, matrix, range, upsample)
    sse = [sum(plane_dists[t][levels[t]][p] for t in _range(n)) for p in _range(3)]
    return buf, FrameRatePlan(levels, rates, dists, plane_dists, 2 * g.O if g.O else 1, len(buf),
                              sum(dists[t][levels[t]] for t in _range(n)), sse)

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

from . import _imagelib, _yuvlayers
from . import frame_tiles  # noqa: F401  (the layer below: its cut and its container)
from ._tilecodec import max_tile  # noqa: F401
from .frames import FAMILY, Frame
# the names the layers above and the tests reach through this module
from .frame_tiles import HEADER_BYTES as FRAME_HEADER_BYTES  # noqa: F401
from .frame_tiles import FrameTilesError, _one_frame, pack_frame_tiled  # noqa: F401
from .frames import FORMATS, RANGES, UPSAMPLES, _check_enums, _frame_struct, coefficients  # noqa: F401
from .rate import TABLE_ENTRY_BYTES, allocate  # noqa: F401
from .tiles import HEADER_BYTES, TileGrid, _check_tiles, _fit_tiles, grid_of, pack_tiled  # noqa: F401

LIB_PATH = _imagelib.lib_path("frame_rate")

#: every symbol frame_rate_csrc/pc_frame_rate.h declares
EXPORTS = ["pc_frame_rate_workspace_size", "pc_frame_rate_tile_sse", "pc_frame_rate_plan", "pc_frame_rate_strerror",
           "pc_frame_rate_last_hip_error"]


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
    return _yuvlayers.frame_tile_distortion(FAMILY, x_hat_tiles, grid, ref, fmt, matrix, range, None, first_tile)


def plan(x_hat_tiles, ref, fmt, overlap=0):
    """pc_frame_rate_plan for tensors (host only, nothing is launched or copied): True where frame_tile_distortion of exactly these
    tensors with this overlap takes the wide-access path.  ref is a tuple of batched tensors ([1,...]) whose strides already fit a
    frame."""
    return _yuvlayers.rate_plan(FAMILY, x_hat_tiles, ref, fmt, overlap)


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
    buf, fields, _ = _yuvlayers.encode_frame_tiled_to_size(FAMILY, model, planes, qualities, target_bytes, fmt, matrix, range, upsample, None, tile,
                                                           overlap, mask_pol, plane_weights, importance, max_tiles_per_call)
    return buf, FrameRatePlan(*fields)

"""Rate-controlled tiled coding of YUV frames of any chroma subsampling and siting (libpc_chroma_rate.so,
chroma_rate_hip/pc_chroma_rate.h): what `frame_rate` is for NV12 / I420 / P010 with centre-sited chroma, for the
twelve formats and three sitings of `chroma`.  One frame in at most N bytes, every tile at the level of the quality list that
rate.allocate picks for it, judged in the frame's own codes.  The composition of rate.py (section 12: the allocator, PCT2) and
chroma_tiles.py (section 23: the cut, PCK1); for "nv12", "i420" and "p010" at "centre" every sum is frame_rate's, bit for bit.

  frame_tile_distortion        decoded tiles + the original frame -> the exact integer weighted squared error per tile and plane
                               (Y, Cb, Cr codes at the format's bit depth and subsampling), one pass over the tiles on the GPU
  encode_frame_tiled_to_size   frame -> (PCK1 container of at most target_bytes bytes holding a PCT2 container, ChromaRatePlan);
                               chroma_tiles.decode_frame_tiled reads it, regions and another output format or siting included

Distortion.  A tile is judged by its OWN rendering: section 21's emit under (fmt, siting, matrix, range) on the tile with its in-frame
part as the picture -- every clamp of the chroma filter at the tile's in-frame part, a tile never reads another tile -- compared with
the original's codes.  A luma sample counts with the integer numerators ay * ax of the stitch's band weights over den = 2 * overlap
(den = 1 without overlap), a chroma sample with cy * cx, cy(k) = (ay(2k) + ay(2k+1)) / 2 where the axis is subsampled and ay(k) where
it is not: the weights depend on the subsampling, never on the siting, and per sample of the frame they sum to den^2 exactly.

At overlap 0 the sum over the tiles is what chroma_tiles.stitch_frame(..., ref=...) reports, exactly, for luma always and for chroma
on every axis that is not both subsampled and co-sited.  On a co-sited subsampled axis the first chroma column (row) of a tile that
is not the first along the axis reads its own first pixel where the stitch reads the neighbouring tile's last, so the chroma sums may
differ in those samples and nowhere else; ChromaRatePlan.sse_exact says which case holds.  Reading the neighbour would make a tile's
distortion depend on the neighbour's level, and the allocator needs it not to.

There is no CPU fallback: CPU tensors raise ValueError before any device call.  Everything runs on the current stream of the tensor's
device.  A clip of these frames in at most N bytes is chroma_clip_rate.py (section 28, over chroma_clips.py's section 25: the same
measure for a list of (frame, tile) jobs).  Out of scope: a tolerance on clips of these formats (as sections 18 and 20), a target
PSNR, measuring in an output format other than the stored one, batches of frames.
"""
import collections
import ctypes as C

from . import _imagelib, _yuvlayers
from . import chroma_tiles  # noqa: F401  (the layer below: its cut and its container)
from ._tilecodec import max_tile  # noqa: F401
from .chroma import FAMILY, FORMATS, SITINGS
from .frames import Frame
from .tiles import TileGrid
# the names the layers above and the tests reach through this module
from .chroma import _check_enums  # noqa: F401
from .chroma_tiles import HEADER_BYTES as FRAME_HEADER_BYTES  # noqa: F401
from .chroma_tiles import ChromaTilesError, _one_frame, pack_frame_tiled  # noqa: F401
from .frames import RANGES, UPSAMPLES, _frame_struct, coefficients  # noqa: F401
from .rate import TABLE_ENTRY_BYTES, allocate  # noqa: F401
from .tiles import HEADER_BYTES, _check_tiles, _fit_tiles, grid_of, pack_tiled  # noqa: F401

LIB_PATH = _imagelib.lib_path("chroma_rate")

#: every symbol chroma_rate_hip/pc_chroma_rate.h declares
EXPORTS = ["pc_chroma_rate_workspace_size", "pc_chroma_rate_tile_sse", "pc_chroma_rate_plan", "pc_chroma_rate_strerror",
           "pc_chroma_rate_last_hip_error"]


def _prototypes():
    i64, vp, ci, cf, fp = C.c_int64, C.c_void_p, C.c_int, C.c_float, C.POINTER(Frame)
    return {
        "pc_chroma_rate_workspace_size": (C.c_size_t, [ci, ci, ci]),
        "pc_chroma_rate_tile_sse": (None, [vp, i64, i64, i64] + [ci] * 14 + [cf] * 5 + [fp, vp, C.c_size_t, vp, vp]),
        "pc_chroma_rate_plan": (None, [vp, i64, i64, i64, ci, ci, ci, ci, fp, C.POINTER(ci)]),
        "pc_chroma_rate_strerror": (C.c_char_p, [ci]),
    }


def lib():
    return _imagelib.load(LIB_PATH, _prototypes)


class ChromaRateError(_imagelib.ImageLibError):
    _lib, _prefix = staticmethod(lib), "pc_chroma_rate"


#: what encode_frame_tiled_to_size decided: frame_rate.FrameRatePlan's fields -- levels[t] (index into the quality list), rates[t][l]
#: (bytes tile t costs at level l, its table entry included), dists[t][l] (plane_dists weighted by plane_weights), plane_dists[t][l]
#: = [D_Y, D_Cb, D_Cr] (frame_tile_distortion), den (the weights' denominator per axis), container_bytes (the length of the
#: container), predicted (the sum of the chosen dists), sse[p] (the sum of the chosen plane_dists per plane) -- and sse_exact: True
#: where overlap is 0 and no subsampled, co-sited axis has more than one tile; sse[p] is then the decoded frame's exact per-plane SSE
#: (sse[0] is that at overlap 0 whatever the siting)
ChromaRatePlan = collections.namedtuple("ChromaRatePlan", "levels rates dists plane_dists den container_bytes predicted sse sse_exact")


def sse_exact(grid, fmt, siting):
    """whether the sums of frame_tile_distortion over grid's tiles are the decoded frame's exact per-plane SSE (the module's docstring)"""
    g = TileGrid(*grid)
    f, (hs, vs) = FORMATS[fmt], SITINGS[siting]
    return g.O == 0 and not (f.sx == 2 and hs and g.nx > 1) and not (f.sy == 2 and vs and g.ny > 1)


def frame_tile_distortion(x_hat_tiles, grid, ref, fmt, matrix="bt709", range="limited", siting="centre", first_tile=0):
    """x_hat_tiles: float32 cuda [n,3,T,T], the decoded tiles first_tile .. first_tile + n - 1 of grid's row-major ny x nx grid (a
    linear range, not a rectangle; grid's own rectangle is ignored; any tile / channel / row strides, unit stride along a row), ref: the
    whole original H x W frame in `fmt` (chroma.py's tuple of planes, any row strides) whose chroma is sited as `siting` says -> int64
    cuda [n,3]: per tile and plane [Y, Cb, Cr] the sum over the tile's samples inside the frame of weight * (code - refcode)^2, exact
    (pc_chroma_rate.h).  A tile's sums do not depend on which range it is part of."""
    return _yuvlayers.frame_tile_distortion(FAMILY, x_hat_tiles, grid, ref, fmt, matrix, range, siting, first_tile)


def plan(x_hat_tiles, ref, fmt, overlap=0):
    """pc_chroma_rate_plan for tensors (host only, nothing is launched or copied): True where frame_tile_distortion of exactly these
    tensors with this overlap takes the wide-access path.  ref is a tuple of batched tensors ([1,...]) whose strides already fit a
    frame."""
    return _yuvlayers.rate_plan(FAMILY, x_hat_tiles, ref, fmt, overlap)


def encode_frame_tiled_to_size(model, planes, qualities, target_bytes, fmt, matrix="bt709", range="limited", upsample="linear",
                               siting="centre", tile=512, overlap=0, mask_pol="point-based-std", plane_weights=(1, 1, 1), importance=None,
                               max_tiles_per_call=32):
    """frame -> (PCK1 container of at most target_bytes bytes, ChromaRatePlan): every tile at the level of `qualities` that
    rate.allocate picks from the bytes each level costs (the tile's single-level PCB1 container plus its table entry) and the
    distortion it leaves (frame_tile_distortion of the tile decoded at that level, the planes weighted by plane_weights = (wY, wCb,
    wCr), non-negative ints; the default is the total squared code error over all samples), optionally weighted by importance
    ([ny][nx] or a flat list, one positive number per tile).  ValueError if even the cheapest level of every tile does not fit.  The
    tiles are cut, coded at every level (compress_levels), decoded again (decompress_levels) and measured max_tiles_per_call at a
    time, so a call holds at most max_tiles_per_call * (1 + len(qualities)) tile tensors on the device; neither the bytes nor the
    plan depend on it.  The container holds a PCT2 container (one level per tile); chroma_tiles.decode_frame_tiled reads it."""
    buf, fields, g = _yuvlayers.encode_frame_tiled_to_size(FAMILY, model, planes, qualities, target_bytes, fmt, matrix, range, upsample, siting, tile,
                                                           overlap, mask_pol, plane_weights, importance, max_tiles_per_call)
    return buf, ChromaRatePlan(*fields, sse_exact(g, fmt, siting))

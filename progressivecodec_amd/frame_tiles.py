"""Tiled coding of YUV 4:2:0 frames (libpc_frame_tiles.so, frame_tiles_csrc/pc_frame_tiles.h): one NV12 / I420 /
P010 frame is cut straight into independent float32 RGB tiles, the tiles are coded as batches, and any admissible window of the frame
is decoded from the tiles that cover it and stitched straight back into planes.  No frame-sized float intermediate, no 8-bit RGB in
the middle.  The arithmetic is section 13's (frames.py) per pixel and section 11's (tiles.py) per tile.

  cut_frame            frame -> float32 tiles [n,3,T,T] (each the crop of the whole frame's ingest, +0.0 beyond the frame), one kernel
  stitch_frame         decoded tiles -> a window of the frame in the chosen format (overlap bands blended, then section 13's emit) and,
                       given the original frame, the per-plane distortion sums, one kernel (plus a small reduction)
  encode_frame_tiled   frame -> one PCG1 container: a fixed header and one unmodified PCT1 container (tiles.py)
  decode_frame_tiled   PCG1 container -> the frame, or the region (y0, x0, h, w) of it from the tiles that cover it alone

A frame is frames.py's: a tuple of cuda tensors without a batch axis ([1,H,W] and so on are taken too), (Y, UV) for "nv12" and "p010",
(Y, U, V) for "i420"; any row strides.  One frame per call.

Admissible windows.  A window (y0, x0, h, w) of the frame has chroma samples of its own only where its 2 x 2 cells are the frame's:
y0 and x0 even, h even or y0 + h == H, w even or x0 + w == W.  Its output is then the crop of the whole frame's (luma [y0:y0+h],
chroma [y0/2 : y0/2 + ceil(h/2)]); anything else is refused.

PCG1 layout: magic "PCG1", version u8 (= 1), fmt, matrix, range, upsample, bits as one byte each (PCF1's ids) -- 10 bytes -- then
one PCT1 or PCT2 container whose H, W are the frame's, unmodified (its table offsets stay relative to its own start), so that
tiles.decode_tiled of it gives the uint8 RGB rendering.

There is no CPU fallback: CPU tensors raise ValueError before any device call.  Everything runs on the current stream of the tensor's
device.  Rate control from YUV (a frame in at most N bytes, per-tile levels) is frame_rate.py's; sequences of frames (tiles of several
frames in one codec call, static tiles coded once) are clips.py's; 4:2:2 / 4:4:4 and left- or top-left-sited chroma are
chroma_tiles.py's.  Out of scope: compress_with_ac.
"""
import ctypes as C
import struct

from . import _imagelib, _yuvlayers
from .frames import FAMILY, Frame
# the names the layers above and the tests reach through this module
from .frames import FORMATS, RANGES, UPSAMPLES, _MATRIX_ID, Distortion, _check_enums, _frame_struct, _frame_view, bits_of, coefficients, empty_frame  # noqa: F401
from .tiles import TileGrid, _check_tiles, _fit_tiles, _window, grid_of  # noqa: F401

LIB_PATH = _imagelib.lib_path("frame_tiles")

#: every symbol frame_tiles_csrc/pc_frame_tiles.h declares
EXPORTS = ["pc_frame_tiles_cut", "pc_frame_tiles_stitch_workspace_size", "pc_frame_tiles_stitch", "pc_frame_tiles_plan",
           "pc_frame_tiles_strerror", "pc_frame_tiles_last_hip_error"]

CUT, STITCH = 0, 1                        # pc_frame_tiles_plan's `op`
MAGIC = b"PCG1"
VERSION = 1
_HEAD = "<BBBBBB"                         # version, fmt, matrix, range, upsample, bits
HEADER_BYTES = 4 + struct.calcsize(_HEAD)


def _prototypes():
    i64, vp, ci, cf, fp = C.c_int64, C.c_void_p, C.c_int, C.c_float, C.POINTER(Frame)
    return {
        "pc_frame_tiles_cut": (None, [fp, ci, ci, ci, cf, cf, cf, cf] + [ci] * 8 + [vp, vp]),
        "pc_frame_tiles_stitch_workspace_size": (C.c_size_t, [ci, ci, ci]),
        "pc_frame_tiles_stitch": (None, [vp, i64, i64, i64] + [ci] * 14 + [cf] * 5 + [fp, fp, vp, C.c_size_t, vp, vp]),
        "pc_frame_tiles_plan": (None, [ci, ci, fp, vp, i64, i64, i64, ci, ci, fp, C.POINTER(ci)]),
        "pc_frame_tiles_strerror": (C.c_char_p, [ci]),
    }


def lib():
    return _imagelib.load(LIB_PATH, _prototypes)


class FrameTilesError(_imagelib.ImageLibError):
    _lib, _prefix = staticmethod(lib), "pc_frame_tiles"


def admissible(window, H, W):
    """whether (y0, x0, h, w), a window inside an H x W frame, has the frame's own chroma samples (the module's docstring)"""
    return _yuvlayers.admissible(FAMILY, window, H, W, "nv12")       # the three formats have the same 2 x 2 cells


def _admissible_window(window, H, W):
    return _yuvlayers.admissible_window(FAMILY, window, H, W, "nv12")


def _one_frame(planes, fmt, what):
    """frames._frame_view for ONE frame: (tensors kept alive, H, W)"""
    return _yuvlayers.one_frame(FAMILY, planes, fmt, what)


def cut_frame(planes, fmt, matrix="bt709", range="limited", upsample="linear", tile=512, overlap=0, rect=None):
    """frame -> (tiles, grid): float32 [n,3,T,T], the tiles of `rect` = (ty0, tx0, nty, ntx) (default: the whole grid) row-major, each
    the crop over [i*S, i*S + T) per axis of what frames.to_model_input computes for the whole frame (the chroma taps clamp at the
    frame's edges, never at a tile's) and +0.0 beyond the frame, and the TileGrid that says so."""
    return _yuvlayers.cut_frame(FAMILY, planes, fmt, matrix, range, upsample, None, tile, overlap, rect)


def _offset_frame(ts, fmt, y0, x0):
    """the Frame of the window whose first luma sample is (y0, x0) (both even) of the frame held by the batched tensors ts"""
    return _yuvlayers.offset_frame(FAMILY, ts, fmt, y0, x0)


def _full_grid(grid):
    return _yuvlayers.full_grid(grid)


def stitch_frame(x_hat_tiles, grid, fmt, matrix="bt709", range="limited", window=None, ref=None, image=True):
    """x_hat_tiles: float32 cuda [n,3,T,T], the decoded tiles of grid's rectangle (any tile / channel / row strides, unit stride along a
    row) -> the admissible window (y0, x0, h, w) of the frame (default: all of it) in `fmt`, a tuple of contiguous planes without a
    batch axis: every covering tile clamped to [0, 1] and blended with the band weights (tiles.stitch's m), then frames' emit on m.
    The rectangle must hold every tile that covers a window pixel.  With ref (the whole original H x W frame in `fmt`) returns
    (frame, Distortion) with the sums over the window; with image=False (needs ref) the Distortion alone."""
    return _yuvlayers.stitch_frame(FAMILY, x_hat_tiles, grid, fmt, matrix, range, None, window, ref, image)


def plan(op, planes, fmt, f32, overlap=0, x0=0, ref=None):
    """pc_frame_tiles_plan for tensors (host only, nothing is launched or copied): True where the cut (op = CUT: planes the source
    frame, f32 the tile tensor, overlap the grid's) or the stitch (op = STITCH: planes the destination window or None, f32 the decoded
    tiles, x0 the window's first column, ref the original's window) of exactly these tensors takes the wide-access path.  planes and
    ref are tuples of batched tensors ([1,...]) whose strides already fit a frame."""
    return _yuvlayers.tiled_plan(FAMILY, op, planes, fmt, f32, overlap, x0, ref)


# -- PCG1: a frame's parameters in front of one PCT1 / PCT2 container -----------------------------------------------------------------

def pack_frame_tiled(inner, fmt, matrix, range, upsample):
    """PCG1: the magic, the version byte, fmt, matrix, range, upsample and bits as one byte each, then the PCT1 / PCT2 container
    unmodified (its H, W are the frame's)."""
    return _yuvlayers.pack_frame_tiled(FAMILY, inner, fmt, matrix, range, upsample, None)


def parse_frame_tiled(buf):
    """-> dict(fmt, matrix, range, upsample, bits, H, W, inner (the PCT1 / PCT2 container), tiled (tiles.parse_tiled of it)).
    ContainerError on a bad magic, version, enum, bit depth, length or inner header; nothing else is touched."""
    return _yuvlayers.parse_frame_tiled(FAMILY, buf)


def encode_frame_tiled(model, planes, qualities, fmt, matrix="bt709", range="limited", upsample="linear", tile=512, overlap=0,
                       mask_pol="point-based-std", max_tiles_per_call=32):
    """frame -> one PCG1 container (bytes) holding every level of `qualities` for every tile.  The tiles are coded max_tiles_per_call
    at a time as one batch each (model.compress_levels), which bounds the device memory a call needs whatever the frame's size; the
    bytes do not depend on it.  The PCT1 container inside is what tiles.pack_tiled makes of the tiles' PCB1 containers."""
    return _yuvlayers.encode_frame_tiled(FAMILY, model, planes, qualities, fmt, matrix, range, upsample, None, tile, overlap, mask_pol,
                                         max_tiles_per_call)


def decode_frame_tiled(model, buf, level=-1, region=None, fmt=None, max_tiles_per_call=32):
    """One level of a PCG1 container -> the frame (a tuple of planes without a batch axis) on the model's device, or its admissible
    region = (y0, x0, h, w), in the stored format or in `fmt` when given (the stored matrix and range either way; another bit depth
    is computed from the decoder's float output, not converted from codes).  Only the tiles that cover the region are read and
    decoded (max_tiles_per_call at a time, one batch each); every refusal is a ContainerError raised before the model is touched."""
    return _yuvlayers.decode_frame_tiled(FAMILY, model, buf, level, region, fmt, None, max_tiles_per_call)

"""Tiled coding of YUV frames of any chroma subsampling and siting (libpc_chroma_tiles.so, chroma_tiles_hip/pc_chroma_tiles.h; DESIGN.md
section 23): what `frame_tiles` is for NV12 / I420 / P010 with centre-sited chroma, for the twelve formats and three sitings of
`chroma`.  One frame is cut straight into independent float32 RGB tiles, the tiles are coded as batches, and any admissible window of
the frame is decoded from the tiles that cover it and stitched straight back into planes.  No frame-sized float intermediate.  The
arithmetic is section 21's (chroma.py) per pixel and section 11's (tiles.py) per tile; for "nv12", "i420" and "p010" at "centre" every
call computes what frame_tiles' computes, bit for bit.

  cut_frame            frame -> float32 tiles [n,3,T,T] (each the crop of the whole frame's ingest, +0.0 beyond the frame), one kernel
  stitch_frame         decoded tiles -> a window of the frame in the chosen format and siting (overlap bands blended, then section 21's
                       emit with the frame as the picture) and, given the original frame, the per-plane distortion sums, one kernel
                       (plus a small reduction)
  encode_frame_tiled   frame -> one PCK1 container: a fixed header and one unmodified PCT1 container (tiles.py)
  decode_frame_tiled   PCK1 container -> the frame, or the region (y0, x0, h, w) of it from the tiles that cover it alone, in the stored
                       format and siting or another

A frame is chroma.py's: a tuple of cuda tensors without a batch axis ([1,H,W] and so on are taken too), (Y, UV) for the semi-planar
formats, (Y, U, V) for the planar ones; any row strides.  One frame per call.

Admissible windows.  A window (y0, x0, h, w) of the frame has chroma samples of its own only where its sy x sx cells are the frame's:
y0 % sy == 0 and x0 % sx == 0, h % sy == 0 or y0 + h == H, w % sx == 0 or x0 + w == W (at 4:4:4 every window, at 4:2:2 every y0 and
h).  Its output is then the crop of the whole frame's (luma [y0:y0+h], chroma [y0/sy : y0/sy + ceil(h/sy)], columns likewise): the
chroma filter clamps at the frame's edges, never at the window's.  Anything else is refused.

The halo.  Under a co-sited horizontal axis (sx == 2 with "left" or "topleft") the first chroma sample of a window with x0 > 0 reads
frame column x0 - 1, and under "topleft" at sy == 2 a window with y0 > 0 reads frame row y0 - 1.  Those pixels are blended from the
tiles like any other, so a stitch needs every tile that covers a pixel of the window EXTENDED BY ITS HALO: with overlap 0 and x0 on a
tile origin that is one more tile column than frame_tiles would need (`halo_window`, `covering`).

PCK1 layout: magic "PCK1", version u8 (= 1), then layout, shift, sx, sy, horizontal siting, vertical siting, matrix, range, upsample
and bits as one byte each (PCH1's ids) -- 15 bytes -- then one PCT1 or PCT2 container whose H, W are the frame's, unmodified (its
table offsets stay relative to its own start), so that tiles.decode_tiled of it gives the uint8 RGB rendering.

There is no CPU fallback: CPU tensors raise ValueError before any device call.  Everything runs on the current stream of the tensor's
device.  Rate control on these formats is chroma_rate.py's (section 24), clips of them chroma_clips.py's (section 25).
"""
import ctypes as C
import struct

from . import _imagelib, _yuvlayers
from .chroma import FAMILY
from .frames import Frame
# the names the layers above and the tests reach through this module
from .chroma import FORMATS, SITINGS, Distortion, _MATRIX_ID, _check_enums, _frame_view, _inv, empty_frame  # noqa: F401
from .frames import RANGES, UPSAMPLES, _frame_struct, coefficients  # noqa: F401
from .tiles import TileGrid, _check_tiles, _fit_tiles, _window, grid_of  # noqa: F401

LIB_PATH = _imagelib.lib_path("chroma_tiles")

#: every symbol chroma_tiles_hip/pc_chroma_tiles.h declares
EXPORTS = ["pc_chroma_tiles_cut", "pc_chroma_tiles_stitch_workspace_size", "pc_chroma_tiles_stitch", "pc_chroma_tiles_plan",
           "pc_chroma_tiles_strerror", "pc_chroma_tiles_last_hip_error"]

CUT, STITCH = 0, 1                        # pc_chroma_tiles_plan's `op`
MAGIC = b"PCK1"
VERSION = 1
_HEAD = "<BBBBBBBBBBB"                    # version, layout, shift, sx, sy, horizontal siting, vertical siting, matrix, range, upsample, bits
HEADER_BYTES = 4 + struct.calcsize(_HEAD)


def _prototypes():
    i64, vp, ci, cf, fp = C.c_int64, C.c_void_p, C.c_int, C.c_float, C.POINTER(Frame)
    return {
        "pc_chroma_tiles_cut": (None, [fp] + [ci] * 9 + [cf] * 4 + [ci] * 8 + [vp, vp]),
        "pc_chroma_tiles_stitch_workspace_size": (C.c_size_t, [ci, ci, ci, ci]),
        "pc_chroma_tiles_stitch": (None, [vp, i64, i64, i64] + [ci] * 20 + [cf] * 5 + [fp, fp, vp, C.c_size_t, vp, vp]),
        "pc_chroma_tiles_plan": (None, [ci, ci, ci, ci, fp, vp, i64, i64, i64, ci, ci, fp, C.POINTER(ci)]),
        "pc_chroma_tiles_strerror": (C.c_char_p, [ci]),
    }


def lib():
    return _imagelib.load(LIB_PATH, _prototypes)


class ChromaTilesError(_imagelib.ImageLibError):
    _lib, _prefix = staticmethod(lib), "pc_chroma_tiles"


def admissible(window, H, W, fmt):
    """whether (y0, x0, h, w), a window inside an H x W frame of `fmt`, has the frame's own chroma samples (the module's docstring)"""
    return _yuvlayers.admissible(FAMILY, window, H, W, fmt)


def halo_window(window, fmt, siting):
    """The window extended by the pixels its first chroma samples read outside it: one column left where the horizontal axis is
    subsampled and co-sited and x0 > 0, one row above where the vertical one is and y0 > 0.  A stitch needs the tiles covering this."""
    return FAMILY.halo(window, fmt, siting)


def covering(grid, window, fmt, siting):
    """The smallest rectangle (ty0, tx0, nty, ntx) of grid a stitch of `window` in `fmt` / `siting` can be given: every tile covering
    a pixel of the halo-extended window.  With overlap 0 and x0 on a tile origin under "left" or "topleft" that is one more tile
    column than TileGrid.covering(window) gives."""
    return _yuvlayers.covering(FAMILY, grid, window, fmt, siting)


def _admissible_window(window, H, W, fmt):
    return _yuvlayers.admissible_window(FAMILY, window, H, W, fmt)


def _one_frame(planes, fmt, what):
    """chroma._frame_view for ONE frame: (tensors kept alive, H, W)"""
    return _yuvlayers.one_frame(FAMILY, planes, fmt, what)


def cut_frame(planes, fmt, matrix="bt709", range="limited", upsample="linear", siting="centre", tile=512, overlap=0, rect=None):
    """frame -> (tiles, grid): float32 [n,3,T,T], the tiles of `rect` = (ty0, tx0, nty, ntx) (default: the whole grid) row-major, each
    the crop over [i*S, i*S + T) per axis of what chroma.to_model_input computes for the whole frame under `siting` (the chroma taps
    clamp at the frame's edges, never at a tile's) and +0.0 beyond the frame, and the TileGrid that says so."""
    return _yuvlayers.cut_frame(FAMILY, planes, fmt, matrix, range, upsample, siting, tile, overlap, rect)


def _offset_frame(ts, fmt, y0, x0):
    """the Frame of the window whose first luma sample is (y0, x0) (multiples of sy, sx) of the frame held by the batched tensors ts"""
    return _yuvlayers.offset_frame(FAMILY, ts, fmt, y0, x0)


def _full_grid(grid):
    return _yuvlayers.full_grid(grid)


def stitch_frame(x_hat_tiles, grid, fmt, matrix="bt709", range="limited", siting="centre", window=None, ref=None, image=True):
    """x_hat_tiles: float32 cuda [n,3,T,T], the decoded tiles of grid's rectangle (any tile / channel / row strides, unit stride along a
    row) -> the admissible window (y0, x0, h, w) of the frame (default: all of it) in `fmt` with its chroma sited as `siting` says, a
    tuple of contiguous planes without a batch axis: every covering tile clamped to [0, 1] and blended with the band weights
    (tiles.stitch's m), then chroma's emit on m with the frame as the picture, so that the result is the crop of the whole frame's.
    The rectangle must hold every tile that covers a pixel of the window extended by its halo (`covering`): under "left" / "topleft"
    at sx == 2 a window with x0 > 0 reads frame column x0 - 1, under "topleft" at sy == 2 one with y0 > 0 reads frame row y0 - 1 --
    with overlap 0 and x0 on a tile origin that is one more tile column than frame_tiles.stitch_frame needs.  With ref (the whole
    original H x W frame in `fmt`) returns (frame, Distortion) with the sums over the window; with image=False (needs ref) the
    Distortion alone."""
    return _yuvlayers.stitch_frame(FAMILY, x_hat_tiles, grid, fmt, matrix, range, siting, window, ref, image)


def plan(op, planes, fmt, f32, overlap=0, x0=0, ref=None):
    """pc_chroma_tiles_plan for tensors (host only, nothing is launched or copied): True where the cut (op = CUT: planes the source
    frame, f32 the tile tensor, overlap the grid's) or the stitch (op = STITCH: planes the destination window or None, f32 the decoded
    tiles, x0 the window's first column, ref the original's window) of exactly these tensors takes the wide-access path.  planes and
    ref are tuples of batched tensors ([1,...]) whose strides already fit a frame."""
    return _yuvlayers.tiled_plan(FAMILY, op, planes, fmt, f32, overlap, x0, ref)


# -- PCK1: a frame's format, siting and parameters in front of one PCT1 / PCT2 container ----------------------------------------------

def pack_frame_tiled(inner, fmt, matrix, range, upsample, siting):
    """PCK1: the magic, the version byte, then layout, shift, sx, sy, horizontal siting, vertical siting, matrix, range, upsample and
    bits as one byte each, then the PCT1 / PCT2 container unmodified (its H, W are the frame's)."""
    return _yuvlayers.pack_frame_tiled(FAMILY, inner, fmt, matrix, range, upsample, siting)


def parse_frame_tiled(buf):
    """-> dict(fmt, siting, matrix, range, upsample, bits, H, W, inner (the PCT1 / PCT2 container), tiled (tiles.parse_tiled of it)).
    ContainerError on a bad magic, version, enum, format, siting, bit depth, length or inner header; nothing else is touched."""
    return _yuvlayers.parse_frame_tiled(FAMILY, buf)


def encode_frame_tiled(model, planes, qualities, fmt, matrix="bt709", range="limited", upsample="linear", siting="centre", tile=512,
                       overlap=0, mask_pol="point-based-std", max_tiles_per_call=32):
    """frame -> one PCK1 container (bytes) holding every level of `qualities` for every tile.  The tiles are coded max_tiles_per_call
    at a time as one batch each (model.compress_levels), which bounds the device memory a call needs whatever the frame's size; the
    bytes do not depend on it.  The PCT1 container inside is what tiles.pack_tiled makes of the tiles' PCB1 containers."""
    return _yuvlayers.encode_frame_tiled(FAMILY, model, planes, qualities, fmt, matrix, range, upsample, siting, tile, overlap, mask_pol,
                                         max_tiles_per_call)


def decode_frame_tiled(model, buf, level=-1, region=None, fmt=None, siting=None, max_tiles_per_call=32):
    """One level of a PCK1 container -> the frame (a tuple of planes without a batch axis) on the model's device, or its admissible
    region = (y0, x0, h, w), in the stored format and siting or in `fmt` / `siting` when given (the stored matrix and range either
    way; another subsampling, depth or siting is computed from the decoder's float output, not converted from codes: a 4:2:2 master
    decodes a region straight to left-sited NV12).  Admissibility and the halo are those of the OUTPUT format and siting.  Only the
    tiles that cover the halo-extended region are read and decoded (max_tiles_per_call at a time, one batch each); every refusal is a
    ContainerError raised before the model is touched."""
    return _yuvlayers.decode_frame_tiled(FAMILY, model, buf, level, region, fmt, siting, max_tiles_per_call)

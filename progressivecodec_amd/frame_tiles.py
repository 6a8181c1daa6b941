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

from . import _imagelib, _tilecodec
from ._lib import PC_OK
from .frames import (FORMATS, RANGES, UPSAMPLES, _MATRIX_ID, Distortion, Frame, _check_enums, _frame_struct, _frame_view, bits_of, coefficients,
                     empty_frame)
from .tiles import TileGrid, _check_tiles, _fit_tiles, _window, grid_of

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
    y0, x0, h, w = window
    return y0 % 2 == 0 and x0 % 2 == 0 and (h % 2 == 0 or y0 + h == H) and (w % 2 == 0 or x0 + w == W)


def _admissible_window(window, H, W):
    y0, x0, h, w = _window((0, 0, H, W) if window is None else window, H, W)
    if not admissible((y0, x0, h, w), H, W):
        raise ValueError(f"window {(y0, x0, h, w)} of the {H}x{W} frame is not admissible: y0 and x0 must be even, h even or y0 + h == H, "
                         "w even or x0 + w == W")
    return y0, x0, h, w


def _one_frame(planes, fmt, what):
    """frames._frame_view for ONE frame: (tensors kept alive, H, W)"""
    import torch
    if isinstance(planes, (tuple, list)) and planes and torch.is_tensor(planes[0]) and planes[0].dim() == 3 and planes[0].shape[0] != 1:
        raise ValueError(f"{what} must be one frame, got a batch of {planes[0].shape[0]}")
    ts, _, H, W, _ = _frame_view(planes, fmt, what)
    return ts, H, W


def cut_frame(planes, fmt, matrix="bt709", range="limited", upsample="linear", tile=512, overlap=0, rect=None):
    """frame -> (tiles, grid): float32 [n,3,T,T], the tiles of `rect` = (ty0, tx0, nty, ntx) (default: the whole grid) row-major, each
    the crop over [i*S, i*S + T) per axis of what frames.to_model_input computes for the whole frame (the chroma taps clamp at the
    frame's edges, never at a tile's) and +0.0 beyond the frame, and the TileGrid that says so."""
    import torch
    _check_enums(fmt, matrix, range, upsample)
    ts, H, W = _one_frame(planes, fmt, "planes")
    g = grid_of(H, W, tile, overlap)
    if rect is not None:
        g = g.with_rect(rect)
    k = coefficients(matrix)
    dev = ts[0].device
    src = _frame_struct(ts)
    with torch.cuda.device(dev):
        out = torch.empty((g.n, 3, g.T, g.T), dtype=torch.float32, device=dev)
        rc = lib().pc_frame_tiles_cut(C.byref(src), FORMATS[fmt], RANGES[range], UPSAMPLES[upsample], k.a, k.b, k.c, k.d, H, W, g.T, g.O,
                                      *g.rect, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    if rc != PC_OK:
        raise FrameTilesError(rc, "pc_frame_tiles_cut")
    return out, g


def _offset_frame(ts, fmt, y0, x0):
    """the Frame of the window whose first luma sample is (y0, x0) (both even) of the frame held by the batched tensors ts"""
    f = _frame_struct(ts)
    es = ts[0].element_size()
    f.y = ts[0].data_ptr() + es * (y0 * ts[0].stride(1) + x0)
    if fmt == "i420":
        f.u = ts[1].data_ptr() + es * ((y0 // 2) * ts[1].stride(1) + x0 // 2)
        f.v = ts[2].data_ptr() + es * ((y0 // 2) * ts[2].stride(1) + x0 // 2)
    else:
        f.u = ts[1].data_ptr() + es * ((y0 // 2) * ts[1].stride(1) + x0)
    return f


def _full_grid(grid):
    g = TileGrid(*grid)
    full = grid_of(g.H, g.W, g.T, g.O)
    if (full.ny, full.nx) != (g.ny, g.nx):
        raise ValueError(f"{g}: the grid of a {g.H}x{g.W} frame is {full.ny}x{full.nx}")
    return full.with_rect(g.rect)


def stitch_frame(x_hat_tiles, grid, fmt, matrix="bt709", range="limited", window=None, ref=None, image=True):
    """x_hat_tiles: float32 cuda [n,3,T,T], the decoded tiles of grid's rectangle (any tile / channel / row strides, unit stride along a
    row) -> the admissible window (y0, x0, h, w) of the frame (default: all of it) in `fmt`, a tuple of contiguous planes without a
    batch axis: every covering tile clamped to [0, 1] and blended with the band weights (tiles.stitch's m), then frames' emit on m.
    The rectangle must hold every tile that covers a window pixel.  With ref (the whole original H x W frame in `fmt`) returns
    (frame, Distortion) with the sums over the window; with image=False (needs ref) the Distortion alone."""
    import torch
    if not image and ref is None:
        raise ValueError("image=False leaves nothing to compute without ref")
    _check_enums(fmt, matrix, range)
    g = _full_grid(grid)
    _check_tiles(x_hat_tiles, g)
    y0, x0, h, w = _admissible_window(window, g.H, g.W)
    need = g.covering((y0, x0, h, w))
    if need[0] < g.ty0 or need[1] < g.tx0 or need[0] + need[2] > g.ty0 + g.nty or need[1] + need[3] > g.tx0 + g.ntx:
        raise ValueError(f"window {(y0, x0, h, w)} needs the tiles {need}, x_hat_tiles holds {g.rect}")
    x = x_hat_tiles
    rts = None
    if ref is not None:
        rts, rH, rW = _one_frame(ref, fmt, "ref")
        if (rH, rW) != (g.H, g.W) or rts[0].device != x.device:
            raise ValueError(f"ref must be the {g.H}x{g.W} frame on {x.device}, got {rH}x{rW} on {rts[0].device}")
    if x.device.type != "cuda":
        raise ValueError(f"x_hat_tiles must be on a GPU (there is no CPU fallback), got {x.device}")
    x = _fit_tiles(x, g.T)
    k = coefficients(matrix)
    L = lib()
    with torch.cuda.device(x.device):
        out = empty_frame(fmt, 1, h, w, x.device) if image else None
        dst = _frame_struct(out) if image else None
        rst = _offset_frame(rts, fmt, y0, x0) if rts is not None else None
        ws = sse = None
        nbytes = 0
        if rts is not None:
            nbytes = L.pc_frame_tiles_stitch_workspace_size(x0, h, w)
            ws = torch.empty(nbytes // 8, dtype=torch.int64, device=x.device)
            sse = torch.empty((1, 3), dtype=torch.int64, device=x.device)
        rc = L.pc_frame_tiles_stitch(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), g.H, g.W, g.T, g.O, *g.rect, y0, x0, h, w,
                                     FORMATS[fmt], RANGES[range], k.kr, k.kg, k.kb, k.ib, k.ir, C.byref(dst) if dst is not None else None,
                                     C.byref(rst) if rst is not None else None, ws.data_ptr() if ws is not None else None, nbytes,
                                     sse.data_ptr() if sse is not None else None, torch.cuda.current_stream(x.device).cuda_stream)
    del rts
    if rc != PC_OK:
        raise FrameTilesError(rc, "pc_frame_tiles_stitch")
    dist = Distortion(sse, h, w, bits_of(fmt)) if sse is not None else None
    if not image:
        return dist
    out = tuple(t[0] for t in out)
    return (out, dist) if dist is not None else out


def plan(op, planes, fmt, f32, overlap=0, x0=0, ref=None):
    """pc_frame_tiles_plan for tensors (host only, nothing is launched or copied): True where the cut (op = CUT: planes the source
    frame, f32 the tile tensor, overlap the grid's) or the stitch (op = STITCH: planes the destination window or None, f32 the decoded
    tiles, x0 the window's first column, ref the original's window) of exactly these tensors takes the wide-access path.  planes and
    ref are tuples of batched tensors ([1,...]) whose strides already fit a frame."""
    _check_enums(fmt)
    wide = C.c_int(-1)
    fr = _frame_struct(planes) if planes is not None else None
    rf = _frame_struct(ref) if ref is not None else None
    rc = lib().pc_frame_tiles_plan(op, FORMATS[fmt], C.byref(fr) if fr is not None else None, f32.data_ptr(), f32.stride(0), f32.stride(1),
                                   f32.stride(2), int(overlap), int(x0), C.byref(rf) if rf is not None else None, C.byref(wide))
    if rc != PC_OK:
        raise FrameTilesError(rc, "pc_frame_tiles_plan")
    return bool(wide.value)


# -- PCG1: a frame's parameters in front of one PCT1 / PCT2 container -----------------------------------------------------------------

def pack_frame_tiled(inner, fmt, matrix, range, upsample):
    """PCG1: the magic, the version byte, fmt, matrix, range, upsample and bits as one byte each, then the PCT1 / PCT2 container
    unmodified (its H, W are the frame's)."""
    from . import container, tiles
    _check_enums(fmt, matrix, range, upsample)
    try:
        tiles.parse_tiled(inner)
    except container.ContainerError as e:
        raise container.ContainerError(f"PCG1: the inner container does not parse: {e}") from None
    return MAGIC + struct.pack(_HEAD, VERSION, FORMATS[fmt], _MATRIX_ID[matrix], RANGES[range], UPSAMPLES[upsample], bits_of(fmt)) + bytes(inner)


def parse_frame_tiled(buf):
    """-> dict(fmt, matrix, range, upsample, bits, H, W, inner (the PCT1 / PCT2 container), tiled (tiles.parse_tiled of it)).
    ContainerError on a bad magic, version, enum, bit depth, length or inner header; nothing else is touched."""
    from . import container, tiles
    if len(buf) < 4 or bytes(buf[:4]) != MAGIC:
        raise container.ContainerError("not a PCG1 container")
    if len(buf) < HEADER_BYTES:
        raise container.ContainerError("truncated PCG1 header")
    ver, f, m, r, u, bits = struct.unpack_from(_HEAD, buf, 4)
    if ver != VERSION:
        raise container.ContainerError(f"unsupported PCG1 version {ver}")
    params = _tilecodec.frame_params(f, m, r, u, bits, "PCG1")
    inner = bytes(buf[HEADER_BYTES:])
    try:
        hd = tiles.parse_tiled(inner)
    except container.ContainerError as e:
        raise container.ContainerError(f"PCG1: the inner container does not parse: {e}") from None
    g = hd["grid"]
    return dict(params, H=g.H, W=g.W, inner=inner, tiled=hd)


def encode_frame_tiled(model, planes, qualities, fmt, matrix="bt709", range="limited", upsample="linear", tile=512, overlap=0,
                       mask_pol="point-based-std", max_tiles_per_call=32):
    """frame -> one PCG1 container (bytes) holding every level of `qualities` for every tile.  The tiles are coded max_tiles_per_call
    at a time as one batch each (model.compress_levels), which bounds the device memory a call needs whatever the frame's size; the
    bytes do not depend on it.  The PCT1 container inside is what tiles.pack_tiled makes of the tiles' PCB1 containers."""
    from . import tiles
    qualities = [float(q) for q in qualities]
    step = _tilecodec.tiles_per_call(max_tiles_per_call)
    x, g = cut_frame(planes, fmt, matrix, range, upsample, tile, overlap)        # the whole frame in one launch
    bufs = _tilecodec.encode_items(model, g.n, step, qualities, mask_pol, g.T, lambda a, b: x[a:a + b])
    return pack_frame_tiled(tiles.pack_tiled(bufs, g.H, g.W, g.T, g.O), fmt, matrix, range, upsample)


def decode_frame_tiled(model, buf, level=-1, region=None, fmt=None, max_tiles_per_call=32):
    """One level of a PCG1 container -> the frame (a tuple of planes without a batch axis) on the model's device, or its admissible
    region = (y0, x0, h, w), in the stored format or in `fmt` when given (the stored matrix and range either way; another bit depth
    is computed from the decoder's float output, not converted from codes).  Only the tiles that cover the region are read and
    decoded (max_tiles_per_call at a time, one batch each); every refusal is a ContainerError raised before the model is touched."""
    from . import container, tiles
    step = _tilecodec.tiles_per_call(max_tiles_per_call)
    hd = parse_frame_tiled(buf)
    out_fmt = hd["fmt"] if fmt is None else fmt
    _check_enums(out_fmt)
    try:
        window = _admissible_window(region, hd["H"], hd["W"])
    except ValueError as e:
        raise container.ContainerError(str(e)) from None
    x_hat, g, window = tiles._decode_region_tiles(model, hd["inner"], level, window, step)
    return stitch_frame(x_hat, g, out_fmt, hd["matrix"], hd["range"], window=window)

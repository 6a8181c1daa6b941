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

from . import _imagelib, _tilecodec
from ._lib import PC_OK
from .chroma import FORMATS, SITINGS, Distortion, _MATRIX_ID, _check_enums, _frame_view, _inv, empty_frame
from .frames import RANGES, UPSAMPLES, Frame, _frame_struct, coefficients
from .tiles import TileGrid, _check_tiles, _fit_tiles, _window, grid_of

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
    y0, x0, h, w = window
    f = FORMATS[fmt]
    return y0 % f.sy == 0 and x0 % f.sx == 0 and (h % f.sy == 0 or y0 + h == H) and (w % f.sx == 0 or x0 + w == W)


def halo_window(window, fmt, siting):
    """The window extended by the pixels its first chroma samples read outside it: one column left where the horizontal axis is
    subsampled and co-sited and x0 > 0, one row above where the vertical one is and y0 > 0.  A stitch needs the tiles covering this."""
    y0, x0, h, w = window
    f, (hs, vs) = FORMATS[fmt], SITINGS[siting]
    dx = 1 if f.sx == 2 and hs and x0 > 0 else 0
    dy = 1 if f.sy == 2 and vs and y0 > 0 else 0
    return (y0 - dy, x0 - dx, h + dy, w + dx)


def covering(grid, window, fmt, siting):
    """The smallest rectangle (ty0, tx0, nty, ntx) of grid a stitch of `window` in `fmt` / `siting` can be given: every tile covering
    a pixel of the halo-extended window.  With overlap 0 and x0 on a tile origin under "left" or "topleft" that is one more tile
    column than TileGrid.covering(window) gives."""
    return TileGrid(*grid).covering(halo_window(window, fmt, siting))


def _admissible_window(window, H, W, fmt):
    y0, x0, h, w = _window((0, 0, H, W) if window is None else window, H, W)
    if not admissible((y0, x0, h, w), H, W, fmt):
        f = FORMATS[fmt]
        raise ValueError(f"window {(y0, x0, h, w)} of the {H}x{W} {fmt!r} frame is not admissible: y0 must be a multiple of {f.sy} and x0 "
                         f"of {f.sx}, h a multiple of {f.sy} or y0 + h == H, w a multiple of {f.sx} or x0 + w == W")
    return y0, x0, h, w


def _one_frame(planes, fmt, what):
    """chroma._frame_view for ONE frame: (tensors kept alive, H, W)"""
    import torch
    if isinstance(planes, (tuple, list)) and planes and torch.is_tensor(planes[0]) and planes[0].dim() == 3 and planes[0].shape[0] != 1:
        raise ValueError(f"{what} must be one frame, got a batch of {planes[0].shape[0]}")
    ts, _, H, W, _ = _frame_view(planes, fmt, what)
    return ts, H, W


def cut_frame(planes, fmt, matrix="bt709", range="limited", upsample="linear", siting="centre", tile=512, overlap=0, rect=None):
    """frame -> (tiles, grid): float32 [n,3,T,T], the tiles of `rect` = (ty0, tx0, nty, ntx) (default: the whole grid) row-major, each
    the crop over [i*S, i*S + T) per axis of what chroma.to_model_input computes for the whole frame under `siting` (the chroma taps
    clamp at the frame's edges, never at a tile's) and +0.0 beyond the frame, and the TileGrid that says so."""
    import torch
    _check_enums(fmt, matrix, range, upsample, siting)
    ts, H, W = _one_frame(planes, fmt, "planes")
    g = grid_of(H, W, tile, overlap)
    if rect is not None:
        g = g.with_rect(rect)
    k = coefficients(matrix)
    f, (hs, vs) = FORMATS[fmt], SITINGS[siting]
    dev = ts[0].device
    src = _frame_struct(ts)
    with torch.cuda.device(dev):
        out = torch.empty((g.n, 3, g.T, g.T), dtype=torch.float32, device=dev)
        rc = lib().pc_chroma_tiles_cut(C.byref(src), *f, hs, vs, RANGES[range], UPSAMPLES[upsample], k.a, k.b, k.c, k.d, H, W, g.T, g.O,
                                       *g.rect, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    if rc != PC_OK:
        raise ChromaTilesError(rc, "pc_chroma_tiles_cut")
    return out, g


def _offset_frame(ts, fmt, y0, x0):
    """the Frame of the window whose first luma sample is (y0, x0) (multiples of sy, sx) of the frame held by the batched tensors ts"""
    f_ = FORMATS[fmt]
    f = _frame_struct(ts)
    es = ts[0].element_size()
    cy, cx = y0 // f_.sy, x0 // f_.sx
    f.y = ts[0].data_ptr() + es * (y0 * ts[0].stride(1) + x0)
    if len(ts) == 3:
        f.u = ts[1].data_ptr() + es * (cy * ts[1].stride(1) + cx)
        f.v = ts[2].data_ptr() + es * (cy * ts[2].stride(1) + cx)
    else:
        f.u = ts[1].data_ptr() + es * (cy * ts[1].stride(1) + 2 * cx)
    return f


def _full_grid(grid):
    g = TileGrid(*grid)
    full = grid_of(g.H, g.W, g.T, g.O)
    if (full.ny, full.nx) != (g.ny, g.nx):
        raise ValueError(f"{g}: the grid of a {g.H}x{g.W} frame is {full.ny}x{full.nx}")
    return full.with_rect(g.rect)


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
    import torch
    if not image and ref is None:
        raise ValueError("image=False leaves nothing to compute without ref")
    _check_enums(fmt, matrix, range, siting=siting)
    g = _full_grid(grid)
    _check_tiles(x_hat_tiles, g)
    y0, x0, h, w = _admissible_window(window, g.H, g.W, fmt)
    need = covering(g, (y0, x0, h, w), fmt, siting)
    if need[0] < g.ty0 or need[1] < g.tx0 or need[0] + need[2] > g.ty0 + g.nty or need[1] + need[3] > g.tx0 + g.ntx:
        raise ValueError(f"window {(y0, x0, h, w)} with its halo {halo_window((y0, x0, h, w), fmt, siting)} needs the tiles {need}, "
                         f"x_hat_tiles holds {g.rect}")
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
    f, (hs, vs) = FORMATS[fmt], SITINGS[siting]
    L = lib()
    with torch.cuda.device(x.device):
        out = empty_frame(fmt, 1, h, w, x.device) if image else None
        dst = _frame_struct(out) if image else None
        rst = _offset_frame(rts, fmt, y0, x0) if rts is not None else None
        ws = sse = None
        nbytes = 0
        if rts is not None:
            nbytes = L.pc_chroma_tiles_stitch_workspace_size(x0, h, w, f.sy)
            ws = torch.empty(nbytes // 8, dtype=torch.int64, device=x.device)
            sse = torch.empty((1, 3), dtype=torch.int64, device=x.device)
        rc = L.pc_chroma_tiles_stitch(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), g.H, g.W, g.T, g.O, *g.rect, y0, x0, h, w,
                                      *f, hs, vs, RANGES[range], k.kr, k.kg, k.kb, k.ib, k.ir, C.byref(dst) if dst is not None else None,
                                      C.byref(rst) if rst is not None else None, ws.data_ptr() if ws is not None else None, nbytes,
                                      sse.data_ptr() if sse is not None else None, torch.cuda.current_stream(x.device).cuda_stream)
    del rts
    if rc != PC_OK:
        raise ChromaTilesError(rc, "pc_chroma_tiles_stitch")
    dist = Distortion(sse, h, w, fmt) if sse is not None else None
    if not image:
        return dist
    out = tuple(t[0] for t in out)
    return (out, dist) if dist is not None else out


def plan(op, planes, fmt, f32, overlap=0, x0=0, ref=None):
    """pc_chroma_tiles_plan for tensors (host only, nothing is launched or copied): True where the cut (op = CUT: planes the source
    frame, f32 the tile tensor, overlap the grid's) or the stitch (op = STITCH: planes the destination window or None, f32 the decoded
    tiles, x0 the window's first column, ref the original's window) of exactly these tensors takes the wide-access path.  planes and
    ref are tuples of batched tensors ([1,...]) whose strides already fit a frame."""
    _check_enums(fmt)
    f = FORMATS[fmt]
    wide = C.c_int(-1)
    fr = _frame_struct(planes) if planes is not None else None
    rf = _frame_struct(ref) if ref is not None else None
    rc = lib().pc_chroma_tiles_plan(op, f.layout, f.bits, f.sx, C.byref(fr) if fr is not None else None, f32.data_ptr(), f32.stride(0),
                                    f32.stride(1), f32.stride(2), int(overlap), int(x0), C.byref(rf) if rf is not None else None,
                                    C.byref(wide))
    if rc != PC_OK:
        raise ChromaTilesError(rc, "pc_chroma_tiles_plan")
    return bool(wide.value)


# -- PCK1: a frame's format, siting and parameters in front of one PCT1 / PCT2 container ----------------------------------------------

def pack_frame_tiled(inner, fmt, matrix, range, upsample, siting):
    """PCK1: the magic, the version byte, then layout, shift, sx, sy, horizontal siting, vertical siting, matrix, range, upsample and
    bits as one byte each, then the PCT1 / PCT2 container unmodified (its H, W are the frame's)."""
    from . import container, tiles
    _check_enums(fmt, matrix, range, upsample, siting)
    try:
        tiles.parse_tiled(inner)
    except container.ContainerError as e:
        raise container.ContainerError(f"PCK1: the inner container does not parse: {e}") from None
    f, (hs, vs) = FORMATS[fmt], SITINGS[siting]
    return MAGIC + struct.pack(_HEAD, VERSION, f.layout, f.shift, f.sx, f.sy, hs, vs, _MATRIX_ID[matrix], RANGES[range], UPSAMPLES[upsample],
                               f.bits) + bytes(inner)


def parse_frame_tiled(buf):
    """-> dict(fmt, siting, matrix, range, upsample, bits, H, W, inner (the PCT1 / PCT2 container), tiled (tiles.parse_tiled of it)).
    ContainerError on a bad magic, version, enum, format, siting, bit depth, length or inner header; nothing else is touched."""
    from . import container, tiles
    if len(buf) < 4 or bytes(buf[:4]) != MAGIC:
        raise container.ContainerError("not a PCK1 container")
    if len(buf) < HEADER_BYTES:
        raise container.ContainerError("truncated PCK1 header")
    ver, lay, sh, sx, sy, hs, vs, m, r, u, bits = struct.unpack_from(_HEAD, buf, 4)
    if ver != VERSION:
        raise container.ContainerError(f"unsupported PCK1 version {ver}")
    fi, si, mi, ri, ui = _inv(FORMATS), _inv(SITINGS), _inv(_MATRIX_ID), _inv(RANGES), _inv(UPSAMPLES)
    if bits not in (8, 10):
        raise container.ContainerError(f"corrupt PCK1 header: {bits} bits")
    if (lay, bits, sh, sx, sy) not in fi or (hs, vs) not in si or m not in mi or r not in ri or u not in ui:
        raise container.ContainerError(f"corrupt PCK1 header: layout {lay}, shift {sh} at {bits} bits, subsampling {sx}x{sy}, "
                                       f"siting {hs}, {vs}, matrix {m}, range {r}, upsample {u}")
    inner = bytes(buf[HEADER_BYTES:])
    try:
        hd = tiles.parse_tiled(inner)
    except container.ContainerError as e:
        raise container.ContainerError(f"PCK1: the inner container does not parse: {e}") from None
    g = hd["grid"]
    return {"fmt": fi[(lay, bits, sh, sx, sy)], "siting": si[(hs, vs)], "matrix": mi[m], "range": ri[r], "upsample": ui[u], "bits": bits,
            "H": g.H, "W": g.W, "inner": inner, "tiled": hd}


def encode_frame_tiled(model, planes, qualities, fmt, matrix="bt709", range="limited", upsample="linear", siting="centre", tile=512,
                       overlap=0, mask_pol="point-based-std", max_tiles_per_call=32):
    """frame -> one PCK1 container (bytes) holding every level of `qualities` for every tile.  The tiles are coded max_tiles_per_call
    at a time as one batch each (model.compress_levels), which bounds the device memory a call needs whatever the frame's size; the
    bytes do not depend on it.  The PCT1 container inside is what tiles.pack_tiled makes of the tiles' PCB1 containers."""
    from . import tiles
    qualities = [float(q) for q in qualities]
    step = _tilecodec.tiles_per_call(max_tiles_per_call)
    x, g = cut_frame(planes, fmt, matrix, range, upsample, siting, tile, overlap)          # the whole frame in one launch
    bufs = _tilecodec.encode_items(model, g.n, step, qualities, mask_pol, g.T, lambda a, b: x[a:a + b])
    return pack_frame_tiled(tiles.pack_tiled(bufs, g.H, g.W, g.T, g.O), fmt, matrix, range, upsample, siting)


def decode_frame_tiled(model, buf, level=-1, region=None, fmt=None, siting=None, max_tiles_per_call=32):
    """One level of a PCK1 container -> the frame (a tuple of planes without a batch axis) on the model's device, or its admissible
    region = (y0, x0, h, w), in the stored format and siting or in `fmt` / `siting` when given (the stored matrix and range either
    way; another subsampling, depth or siting is computed from the decoder's float output, not converted from codes: a 4:2:2 master
    decodes a region straight to left-sited NV12).  Admissibility and the halo are those of the OUTPUT format and siting.  Only the
    tiles that cover the halo-extended region are read and decoded (max_tiles_per_call at a time, one batch each); every refusal is a
    ContainerError raised before the model is touched."""
    from . import container, tiles
    step = _tilecodec.tiles_per_call(max_tiles_per_call)
    hd = parse_frame_tiled(buf)
    out_fmt = hd["fmt"] if fmt is None else fmt
    out_siting = hd["siting"] if siting is None else siting
    _check_enums(out_fmt, siting=out_siting)
    try:
        window = _admissible_window(region, hd["H"], hd["W"], out_fmt)
    except ValueError as e:
        raise container.ContainerError(str(e)) from None
    x_hat, g, _ = tiles._decode_region_tiles(model, hd["inner"], level, halo_window(window, out_fmt, out_siting), step)
    return stitch_frame(x_hat, g, out_fmt, hd["matrix"], hd["range"], out_siting, window=window)

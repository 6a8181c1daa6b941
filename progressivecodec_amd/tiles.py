"""Tiled image coding (libpc_tiles.so, tiles_csrc/pc_tiles.h): one 8-bit image is cut into independent, equally
sized tiles, the tiles are coded as a batch, and any rectangle of the image is decoded from the tiles that cover it.

  cut             uint8 image -> float32 tiles [n,3,T,T] (zero-extended at the bottom / right), one kernel
  stitch          decoded tiles -> a window of the uint8 image (overlap bands blended) and, given the original, the distortion
                  sums behind PSNR, one kernel
  encode_tiled    uint8 image -> one PCT1 container: one PCB1 container (container.py) per tile behind an offset table
  decode_tiled    PCT1 / PCT2 container -> uint8 image, or the region (y0, x0, h, w) of it from the tiles that cover it alone

Geometry.  Tile size T (a multiple of 64), overlap O (a multiple of 4, 0 <= O <= T/2), stride S = T - O.  An axis of length L has
1 tile if L <= T, otherwise ceil((L - T) / S) + 1; tile i covers [i*S, i*S + T), the image sits at the top-left of the grid, tiles
are numbered row-major.  In the band of O pixels two neighbours share, the later tile weighs local coordinate u with
(2u + 1) / (2 O) and the earlier one with the mirror image; a pixel's weight for a tile is wy * wx.

PCT1 layout (little endian):

    magic  "PCT1"                      4 B
    version                            u8   (= 1)
    numeric contract id                u32  (pc_contract_id() of the encoder, as in every tile's PCB1 header)
    H, W  (image size)                 u32 u32
    T, O  (tile size, overlap)         u32 u32
    ny, nx (tiles along H and W)       u32 u32
    for every tile, row-major:         offset u64, length u64   (offset from the start of the container)
    payload: the tiles' PCB1 containers in tile order, each with image_size = (T, T)

The header is 33 bytes, the table 16 bytes per tile.  Random access: a reader wanting a region needs the header, the table and the
byte ranges of the covering tiles only; inside each, PCB1's own property holds (the base segment and the wanted level's segment).
A container cut off after tile k still decodes every region inside tiles 0 .. k.  ny and nx are redundant with H, W, T and O: a
container whose grid is not the one pc_tiles_grid gives is refused.

PCT2 (written by rate.encode_tiled_to_size): magic "PCT2", version 1, the header and the table exactly as
above; every tile's PCB1 holds exactly ONE level, and tiles may differ in quality (they agree in mask policy and contract).

Layouts: "hwc" is [H,W,3], "chw" is [3,H,W].  There is no CPU fallback: CPU tensors raise ValueError before any device call.
Everything runs on the current stream of the tensor's device.  Out of scope: a level-major container (quality-progressive
truncation across the whole image), tiling inside compress_with_ac and REM models.  Per-tile qualities under a byte budget are
rate.py's (PCT2).
"""
import collections
import ctypes as C
import struct

from . import _imagelib, _tilecodec
from ._lib import PC_OK
from .container import ContainerError
from .pixels import LAYOUTS, ROUNDINGS, Distortion, _hw, _u8_view

LIB_PATH = _imagelib.lib_path("tiles")

#: every symbol tiles_csrc/pc_tiles.h declares
EXPORTS = ["pc_tiles_grid", "pc_tiles_cut_u8", "pc_tiles_stitch_workspace_size", "pc_tiles_stitch_u8", "pc_tiles_plan",
           "pc_tiles_strerror", "pc_tiles_last_hip_error"]

CUT, STITCH = 0, 1                        # pc_tiles_plan's `op`
MAGIC = b"PCT1"
MAGIC2 = b"PCT2"                          # one level per tile, tiles may differ in quality
VERSION = 1
_HEAD = "<BIIIIIII"                       # version, contract id, H, W, T, O, ny, nx
HEADER_BYTES = 4 + struct.calcsize(_HEAD)


def _prototypes():
    i64, vp, ci = C.c_int64, C.c_void_p, C.c_int
    u8v = [vp, ci, i64, i64]                                        # a u8 view: pointer, layout, plane / row stride in bytes
    return {
        "pc_tiles_grid": (None, [ci, ci, ci, ci, C.POINTER(ci), C.POINTER(ci)]),
        "pc_tiles_cut_u8": (None, u8v + [ci] * 8 + [vp, vp]),
        "pc_tiles_stitch_workspace_size": (C.c_size_t, [ci, ci, ci]),
        "pc_tiles_stitch_u8": (None, [vp, i64, i64, i64] + [ci] * 13 + u8v + u8v + [vp, C.c_size_t, vp, vp, vp]),
        "pc_tiles_plan": (None, [ci] + u8v + [vp, i64, i64, i64, ci] + u8v + [C.POINTER(ci)]),
        "pc_tiles_strerror": (C.c_char_p, [ci]),
    }


def lib():
    return _imagelib.load(LIB_PATH, _prototypes)


class TilesError(_imagelib.ImageLibError):
    _lib, _prefix = staticmethod(lib), "pc_tiles"


class TileGrid(collections.namedtuple("TileGrid", "H W T O ny nx ty0 tx0 nty ntx")):
    """The ny x nx grid of T x T tiles with overlap O over an H x W image, and the rectangle (ty0, tx0, nty, ntx) of it a tile
    tensor holds: tile (ty0 + a, tx0 + b) is entry a * ntx + b."""
    __slots__ = ()

    @property
    def S(self):
        return self.T - self.O

    @property
    def rect(self):
        return (self.ty0, self.tx0, self.nty, self.ntx)

    @property
    def n(self):
        return self.nty * self.ntx

    def with_rect(self, rect):
        ty0, tx0, nty, ntx = (int(v) for v in rect)
        if ty0 < 0 or tx0 < 0 or nty < 1 or ntx < 1 or ty0 + nty > self.ny or tx0 + ntx > self.nx:
            raise ValueError(f"rect {tuple(rect)} lies outside the {self.ny}x{self.nx} grid")
        return self._replace(ty0=ty0, tx0=tx0, nty=nty, ntx=ntx)

    def covering(self, window):
        """The smallest rectangle (ty0, tx0, nty, ntx) that holds every tile covering a pixel of window = (y0, x0, h, w)."""
        y0, x0, h, w = _window(window, self.H, self.W)
        ya, yb = _axis_cover(y0, y0 + h - 1, self.S, self.O, self.ny)
        xa, xb = _axis_cover(x0, x0 + w - 1, self.S, self.O, self.nx)
        return (ya, xa, yb - ya + 1, xb - xa + 1)


def _axis_tiles(L, T, S):
    return 1 if L <= T else -(-(L - T) // S) + 1


def _axis_cover(p0, p1, S, O, n):
    """first tile covering p0, last tile covering p1"""
    last = lambda p: min(p // S, n - 1)
    i = last(p0)
    return (i - 1 if i > 0 and p0 - i * S < O else i), last(p1)


def _window(window, H, W):
    try:
        y0, x0, h, w = (int(v) for v in window)
    except (TypeError, ValueError):
        raise ValueError(f"a window / region is (y0, x0, h, w), got {window!r}") from None
    if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > H or x0 + w > W:
        raise ValueError(f"region {(y0, x0, h, w)} lies outside the {H}x{W} image")
    return y0, x0, h, w


def grid_of(H, W, tile=512, overlap=0):
    """TileGrid of an H x W image with its whole grid as the rectangle (pure Python; tests hold it to pc_tiles_grid)."""
    H, W, T, O = int(H), int(W), int(tile), int(overlap)
    if T < 64 or T % 64:
        raise ValueError(f"tile must be a positive multiple of 64, got {tile}")
    if O < 0 or O % 4 or O > T // 2:
        raise ValueError(f"overlap must be a multiple of 4 with 0 <= overlap <= tile / 2, got {overlap}")
    if H < 1 or W < 1:
        raise ValueError(f"image size {H}x{W}")
    ny, nx = _axis_tiles(H, T, T - O), _axis_tiles(W, T, T - O)
    if ny * nx >= 1 << 31:
        raise ValueError(f"{ny}x{nx} tiles: too many")
    return TileGrid(H, W, T, O, ny, nx, 0, 0, ny, nx)


def _view3(t, layout, what):
    """pixels._u8_view for ONE image: (4-D tensor kept alive, (pointer, layout, plane stride, row stride), (H, W))"""
    import torch
    if torch.is_tensor(t) and t.dim() != 3:
        raise ValueError(f"{what} must be one image, [H,W,3] ('hwc') or [3,H,W] ('chw'), got {tuple(t.shape)}")
    t4, (p, lay, _, sp, sr) = _u8_view(t, layout, what)
    return t4, (p, lay, sp, sr), _hw(t4, layout)


def cut(img, tile=512, overlap=0, layout="hwc", rect=None):
    """uint8 cuda image [H,W,3] ("hwc") or [3,H,W] ("chw"), any strides -> (tiles, grid): float32 [n,3,T,T], the tiles of `rect` =
    (ty0, tx0, nty, ntx) (default: the whole grid) row-major, each img.float().div(255) over [i*S, i*S + T) per axis and +0.0 beyond
    the image, and the TileGrid that says so."""
    import torch
    t4, view, (H, W) = _view3(img, layout, "img")
    g = grid_of(H, W, tile, overlap)
    if rect is not None:
        g = g.with_rect(rect)
    with torch.cuda.device(t4.device):
        out = torch.empty((g.n, 3, g.T, g.T), dtype=torch.float32, device=t4.device)
        rc = lib().pc_tiles_cut_u8(*view, H, W, g.T, g.O, *g.rect, out.data_ptr(), torch.cuda.current_stream(t4.device).cuda_stream)
    if rc != PC_OK:
        raise TilesError(rc, "pc_tiles_cut_u8")
    return out, g


def _check_tiles(x, g):
    import torch
    if not torch.is_tensor(x):
        raise TypeError("x_hat_tiles must be a tensor")
    if x.dtype != torch.float32:
        raise TypeError(f"x_hat_tiles must be float32, got {x.dtype}")
    if x.dim() != 4 or tuple(x.shape) != (g.n, 3, g.T, g.T):
        raise ValueError(f"x_hat_tiles must be [{g.n},3,{g.T},{g.T}] for {g}, got {tuple(x.shape)}")


def _fit_tiles(x, T):
    """a tile tensor the kernels can take as it is, or its contiguous copy"""
    return x if x.stride(3) == 1 and x.stride(2) >= T and min(x.stride()[:2]) >= 1 else x.contiguous()


def _linear_tiles(grid, x_hat_tiles, first_tile, what, limit, *of):
    """What the three tile distortions check first: grid is the grid of its `what` ("image", "frame"), limit(T, *of) passes,
    x_hat_tiles is float32 [n,3,T,T] and the tiles first_tile .. first_tile + n - 1 lie in the grid -> (the whole grid, n, the tile
    tensor as the kernels can take it)."""
    import torch
    g = TileGrid(*grid)
    full = grid_of(g.H, g.W, g.T, g.O)
    if (full.ny, full.nx) != (g.ny, g.nx):
        raise ValueError(f"{g}: the grid of a {g.H}x{g.W} {what} is {full.ny}x{full.nx}")
    limit(g.T, *of)
    x = x_hat_tiles
    n = int(x.shape[0]) if torch.is_tensor(x) and x.dim() == 4 else 0
    first_tile = int(first_tile)
    if n < 1 or first_tile < 0 or first_tile + n > full.ny * full.nx:
        raise ValueError(f"tiles {first_tile} .. {first_tile + n - 1} lie outside the {full.ny}x{full.nx} grid"
                         if n else "x_hat_tiles must be a [n,3,T,T] tensor with n >= 1")
    _check_tiles(x, full._replace(nty=1, ntx=n))
    return full, n, _fit_tiles(x, g.T)


def stitch(x_hat_tiles, grid, window=None, layout="hwc", rounding="nearest", ref=None, ref_layout=None, image=True):
    """x_hat_tiles: float32 cuda [n,3,T,T], the decoded tiles of grid's rectangle (any tile / channel / row strides, unit stride along a
    row) -> uint8 [h,w,3] ("hwc") or [3,h,w] ("chw"): the window (y0, x0, h, w) of the image (default: all of it), every covering tile
    clamped to [0, 1] and blended with the band weights, times 255, rounded half to even ("nearest") or towards zero ("trunc").  The
    rectangle must hold every tile that covers a window pixel.  With ref (the original uint8 H x W image in ref_layout, default
    `layout`) returns (image, Distortion) with the sums over the window; with image=False (needs ref) the Distortion alone."""
    import torch
    if not image and ref is None:
        raise ValueError("image=False leaves nothing to compute without ref")
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be 'hwc' or 'chw', got {layout!r}")
    if rounding not in ROUNDINGS:
        raise ValueError(f"rounding must be 'nearest' or 'trunc', got {rounding!r}")
    g = TileGrid(*grid)
    full = grid_of(g.H, g.W, g.T, g.O)
    if (full.ny, full.nx) != (g.ny, g.nx):
        raise ValueError(f"{g}: the grid of a {g.H}x{g.W} image is {full.ny}x{full.nx}")
    g = full.with_rect(g.rect)
    _check_tiles(x_hat_tiles, g)
    y0, x0, h, w = _window((0, 0, g.H, g.W) if window is None else window, g.H, g.W)
    need = g.covering((y0, x0, h, w))
    if need[0] < g.ty0 or need[1] < g.tx0 or need[0] + need[2] > g.ty0 + g.nty or need[1] + need[3] > g.tx0 + g.ntx:
        raise ValueError(f"window {(y0, x0, h, w)} needs the tiles {need}, x_hat_tiles holds {g.rect}")
    x = x_hat_tiles
    rview, r4 = (None, 0, 0, 0), None
    if ref is not None:
        ref_layout = layout if ref_layout is None else ref_layout
        r4, rfull, rhw = _view3(ref, ref_layout, "ref")
        if rhw != (g.H, g.W) or r4.device != x.device:
            raise ValueError(f"ref must be the {g.H}x{g.W} image on {x.device}, got {tuple(ref.shape)} on {ref.device}")
        px = 3 if ref_layout == "hwc" else 1
        rview = (rfull[0] + y0 * rfull[3] + px * x0, rfull[1], rfull[2], rfull[3])
    if x.device.type != "cuda":
        raise ValueError(f"x_hat_tiles must be on a GPU (there is no CPU fallback), got {x.device}")
    x = _fit_tiles(x, g.T)
    L = lib()
    with torch.cuda.device(x.device):
        out, oview = None, (None, 0, 0, 0)
        if image:
            out = torch.empty((h, w, 3) if layout == "hwc" else (3, h, w), dtype=torch.uint8, device=x.device)
            oview = (out.data_ptr(), LAYOUTS[layout], 0 if layout == "hwc" else out.stride(0), out.stride(0 if layout == "hwc" else 1))
        ws = sums = None
        nbytes = 0
        if ref is not None:
            nbytes = L.pc_tiles_stitch_workspace_size(x0, h, w)
            ws = torch.empty(nbytes // 8, dtype=torch.int64, device=x.device)
            sums = torch.empty((2, 1, 3), dtype=torch.int64, device=x.device)
        rc = L.pc_tiles_stitch_u8(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), g.H, g.W, g.T, g.O, *g.rect, y0, x0, h, w,
                                  ROUNDINGS[rounding], *oview, *rview, ws.data_ptr() if ws is not None else None, nbytes,
                                  sums[0].data_ptr() if sums is not None else None, sums[1].data_ptr() if sums is not None else None,
                                  torch.cuda.current_stream(x.device).cuda_stream)
    del r4
    if rc != PC_OK:
        raise TilesError(rc, "pc_tiles_stitch_u8")
    if not image:
        return Distortion(sums, h, w)
    return (out, Distortion(sums, h, w)) if ref is not None else out


def plan(op, u8, layout, f32, x0=0, ref=None, ref_layout=None):
    """pc_tiles_plan for tensors (host only, nothing is launched or copied): True where the cut (op = CUT: u8 the source image, f32 the
    tile tensor) or the stitch (op = STITCH: u8 the destination window, f32 the decoded tiles, x0 the window's first column, ref the
    original's window) of exactly these tensors takes the wide-access path.  u8 and ref are 3-D uint8 tensors whose strides already
    fit a view (unit stride along the channel / column axis); u8 may be None for a stitch with ref (sums only)."""
    def view(t, lay):
        if t is None:
            return (None, 0, 0, 0)
        return (t.data_ptr(), 0, 0, t.stride(0)) if lay == "hwc" else (t.data_ptr(), 1, t.stride(0), t.stride(1))
    rl = layout if ref_layout is None else ref_layout
    wide = C.c_int(-1)
    rc = lib().pc_tiles_plan(op, *view(u8, layout), f32.data_ptr(), f32.stride(0), f32.stride(1), f32.stride(2), int(x0), *view(ref, rl),
                             C.byref(wide))
    if rc != PC_OK:
        raise TilesError(rc, "pc_tiles_plan")
    return bool(wide.value)


# -- PCT1 ----------------------------------------------------------------------------------------------------------------------------

def pack_tiled(tile_bufs, H, W, tile, overlap, contract=None, per_tile_levels=False):
    """The PCB1 containers of every tile of the grid, in tile order -> one PCT1 container; per_tile_levels: a PCT2 container, whose
    tiles hold one level each (checked by decode_tiled, not here)."""
    from . import container
    g = grid_of(H, W, tile, overlap)
    if len(tile_bufs) != g.ny * g.nx:
        raise ContainerError(f"{g.ny * g.nx} tile containers expected, got {len(tile_bufs)}")
    contract = container.build_contract_id() if contract is None else int(contract)
    head = (MAGIC2 if per_tile_levels else MAGIC) + struct.pack(_HEAD, VERSION, contract, g.H, g.W, g.T, g.O, g.ny, g.nx)
    off = len(head) + 16 * len(tile_bufs)
    table = []
    for b in tile_bufs:
        table.append(struct.pack("<QQ", off, len(b)))
        off += len(b)
    return head + b"".join(table) + b"".join(bytes(b) for b in tile_bufs)


def parse_tiled(buf):
    """-> dict(magic (b"PCT1" or b"PCT2"), contract, grid (TileGrid, whole grid), table [(offset, length) per tile], payload_start).
    Checks the header, the geometry against pc_tiles_grid and that the whole table is there; a table entry is checked against the
    buffer when its tile is asked for (tile_bytes), so that a container cut off inside its payload still gives the tiles it holds
    completely."""
    magic = bytes(buf[:4])
    if len(buf) < 4 or magic not in (MAGIC, MAGIC2):
        raise ContainerError("not a PCT1 or PCT2 container")
    if len(buf) < HEADER_BYTES:
        raise ContainerError("truncated header")
    ver, contract, H, W, T, O, ny, nx = struct.unpack_from(_HEAD, buf, 4)
    if ver != VERSION:
        raise ContainerError(f"unsupported version {ver}")
    g, table, start = _tilecodec.tile_table(buf, HEADER_BYTES, H, W, T, O, ny, nx)
    return {"magic": magic, "contract": contract, "grid": g, "table": table, "payload_start": start}


def tile_bytes(buf, hd, t):
    """The PCB1 container of tile t, after checking its table entry against the buffer and its header against the grid."""
    return _tilecodec.entry_bytes(buf, hd, hd["table"][t], f"tile {t}")


def encode_tiled(model, img, qualities, tile=512, overlap=0, mask_pol="point-based-std", layout="hwc", max_tiles_per_call=32):
    """uint8 cuda image [H,W,3] / [3,H,W] -> one PCT1 container (bytes) holding every level of `qualities` for every tile.  The tiles
    are coded max_tiles_per_call at a time as one batch each (model.compress_levels), which bounds the device memory a call needs
    whatever the image's size; the bytes do not depend on it.  model: a loaded ChannelProgresssiveWACNN (any topology / post-filter)."""
    qualities = [float(q) for q in qualities]
    step = _tilecodec.tiles_per_call(max_tiles_per_call)
    tiles, g = cut(img, tile, overlap, layout)                                   # the whole image in one launch
    bufs = _tilecodec.encode_items(model, g.n, step, qualities, mask_pol, g.T, lambda a, b: tiles[a:a + b])
    return pack_tiled(bufs, g.H, g.W, g.T, g.O)


def decode_tiled(model, buf, level=-1, region=None, layout="hwc", rounding="nearest", max_tiles_per_call=32):
    """One level (index into the quality list, negative from the end) of a PCT1 container, or the one level every tile of a PCT2
    container holds (level -1 or 0; tiles may differ in quality and are decoded grouped by it) -> uint8 [h,w,3] ("hwc") or [3,h,w] ("chw")
    on the model's device: region = (y0, x0, h, w) of the image, default all of it.  Only the tiles that cover the region are read,
    decoded (max_tiles_per_call at a time, one batch each) and stitched; of each, only the header, the base segment and that level's
    segment.  ContainerError, before the model is touched, for a corrupt or truncated container and for tiles that disagree with the
    grid or with each other; a region whose tiles are complete decodes whatever follows them."""
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be 'hwc' or 'chw', got {layout!r}")
    if rounding not in ROUNDINGS:
        raise ValueError(f"rounding must be 'nearest' or 'trunc', got {rounding!r}")
    step = _tilecodec.tiles_per_call(max_tiles_per_call)
    x_hat, g, window = _decode_region_tiles(model, buf, level, region, step)
    return stitch(x_hat, g, window, layout=layout, rounding=rounding)


def _decode_region_tiles(model, buf, level, region, step):
    """What decode_tiled (and frame_tiles.decode_frame_tiled, on the PCT1 / PCT2 container inside a PCG1 one) does up to the stitch:
    one level of the tiles that cover region = (y0, x0, h, w) (None: the whole image) -> (x_hat float32 [n,3,T,T], the TileGrid whose
    rectangle they are, the window as four ints), decoded step tiles at a time by _tilecodec.decode_positions: the tiles of a PCT1
    container as one group in tile order, those of a PCT2 container (one level each) grouped by quality, ascending, tile order
    within a group.  Every refusal -- a tile with another number of levels, tiles that differ in what a codec call shares -- is a
    ContainerError (a region outside the image a ValueError) raised before the model is touched."""
    hd = parse_tiled(buf)
    pct2 = hd["magic"] == MAGIC2
    if pct2:
        _tilecodec.one_level(level, "PCT2")
    g = hd["grid"]
    window = _window((0, 0, g.H, g.W) if region is None else region, g.H, g.W)
    g = g.with_rect(g.covering(window))
    blobs = [tile_bytes(buf, hd, (g.ty0 + a) * g.nx + g.tx0 + b) for a in range(g.nty) for b in range(g.ntx)]
    _tilecodec.check_contract(hd["contract"])
    per_tile, groups, common = [], {}, None
    for k, (tb, th) in enumerate(blobs):
        if pct2 and len(th["qualities"]) != 1:
            raise ContainerError(f"tile {k} of the region holds {len(th['qualities'])} levels, a PCT2 tile holds exactly one")
        shape, q, mask_pol, strings = _tilecodec.level_strings(tb, th, 0 if pct2 else level)
        key = (shape, mask_pol) if pct2 else (shape, q, mask_pol, len(strings[0]))
        common = key if common is None else common
        _tilecodec.same_coding(key, common, f"tile {k} of the region", "its first tile")
        per_tile.append(strings)
        groups.setdefault(q, []).append(k)
    return _tilecodec.decode_positions(model, per_tile, sorted(groups.items()), shape, mask_pol, step, g.n), g, window

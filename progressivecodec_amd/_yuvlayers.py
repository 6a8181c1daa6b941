"""What the two stacks of YUV layers share on the host: frames / frame_tiles / frame_rate (4:2:0, centre-sited;
sections 13 to 15) and chroma / chroma_tiles / chroma_rate (twelve formats, three sitings; sections 21, 23, 24) are one body each,
written here against a Family -- the few things in which the stacks differ.  No library of its own, in the spirit of _tilecodec.py:
every C call goes through the owning module's lib(), looked up on each call, under that module's symbol prefix and error class.
What both stacks always used as it is -- RANGES, UPSAMPLES, MATRICES, coefficients, the Frame struct, the x_hat check, the PSNR --
lives here too, and frames.py and chroma.py hand those names on: this module imports neither of them.

  Format, Family      a format as (layout, bits, shift, sx, sy); what a stack says about itself (below)
  frame layer         frame_view, empty_frame, Distortion, to_model_input, from_model_output, plan, pack_frame, parse_frame,
                      encode_frame, decode_frame
  tiled layer         one_frame, full_grid, offset_frame, admissible, admissible_window, halo_window, covering, cut_frame,
                      stitch_frame, tiled_plan, pack_frame_tiled, parse_frame_tiled, encode_frame_tiled, decode_frame_tiled
  rate layer          frame_tile_distortion, rate_plan, encode_frame_tiled_to_size

The six modules keep their docstrings, signatures, libraries, error classes and container constants and delegate.  A stack without
sitings (4:2:0) passes siting=None: its C calls take no siting and its public functions no such parameter.
"""
import collections
import ctypes as C
import importlib
import math
import struct

from . import _tilecodec
from ._lib import PC_OK
from .pixels import Geometry, padding
from .tiles import TileGrid, _check_tiles, _fit_tiles, _linear_tiles, _window, grid_of

Format = collections.namedtuple("Format", "layout bits shift sx sy")
PLANAR, SEMIPLANAR = 0, 1                                 # PC_CH_PLANAR, PC_CH_SEMIPLANAR

#: owners        ((module, its error class), ...) of the frame, tiled and rate layer, by name: lib(), the error and the symbol prefix
#: formats       name -> Format
#: check         the stack's _check_enums: (fmt, matrix, range, upsample[, siting]), None for what is not to be checked
#: c_format      {(fmt, siting): the format integers of ingest / emit / cut / stitch / tile_sse}
#: c_plan        {(fmt, layer): the format integers of the layer's *_plan}
#: c_sy          {fmt: the extra sy of the *_workspace_size calls, as a tuple (empty where the call takes none)}
#: halo          (window, fmt, siting) -> the window extended by what its first chroma samples read, or None: no halo
#: head_of       (fmt, matrix, range, upsample, siting) -> the parameter bytes of the stack's container heads
#: params_of     (the head's fields after the version, container name) -> (dict of names or the refusal, the fields left over)
#: plane_of      what a plane's shape refusal says after "Y plane" ("{fmt!r}" is filled in)
#: inadmissible  the refusal of a window (win, H, W, fmt, sx, sy are filled in)
#: distortion    (sse, H, W, fmt) -> the stack's Distortion
Family = collections.namedtuple("Family", "owners formats check c_format c_plan c_sy halo head_of params_of plane_of inadmissible distortion")
FRAME, TILED, RATE = 0, 1, 2                              # the layers, as indices into Family.owners

_range = range                                            # the functions below take a parameter of that name
_layers = {}


# -- what both stacks use as it is (frames.py and chroma.py hand these names on) -------------------------------------------------------------

RANGES = {"limited": 0, "full": 1}                        # PC_FRAMES_LIMITED, PC_FRAMES_FULL
UPSAMPLES = {"nearest": 0, "linear": 1}                   # PC_FRAMES_NEAREST, PC_FRAMES_LINEAR
MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}     # (Kr, Kb); Kg = 1 - Kr - Kb


class Frame(C.Structure):
    """pc_frame: three planes, each a pointer with batch and row strides in elements"""
    _fields_ = [("y", C.c_void_p), ("y_batch", C.c_int64), ("y_row", C.c_int64),
                ("u", C.c_void_p), ("u_batch", C.c_int64), ("u_row", C.c_int64),
                ("v", C.c_void_p), ("v_batch", C.c_int64), ("v_row", C.c_int64)]


def _f32(v):
    """a Python double rounded once to float32 (and held as the double of that value)"""
    return struct.unpack("<f", struct.pack("<f", v))[0]


Coefficients = collections.namedtuple("Coefficients", "a b c d kr kg kb ib ir")
_coefficients = {}


def coefficients(matrix):
    """The nine float32 coefficients of a matrix, each computed in float64 from Kr and Kb and rounded once: the reconstruction factors
    a = 2(1-Kr), b = 2Kb(1-Kb)/Kg, c = 2Kr(1-Kr)/Kg, d = 2(1-Kb); the luma weights Kr, Kg, Kb; the chroma factors ib = 1/(2(1-Kb)),
    ir = 1/(2(1-Kr)).  What the kernels and the restatement both take."""
    k = _coefficients.get(matrix)
    if k is None:                                                       # computed once per matrix: a call is a table look-up
        if matrix not in MATRICES:
            raise ValueError(f"matrix must be one of {sorted(MATRICES)}, got {matrix!r}")
        kr, kb = MATRICES[matrix]
        kg = 1.0 - kr - kb
        k = _coefficients[matrix] = Coefficients(*map(_f32, (2 * (1 - kr), 2 * kb * (1 - kb) / kg, 2 * kr * (1 - kr) / kg, 2 * (1 - kb), kr, kg,
                                                             kb, 1 / (2 * (1 - kb)), 1 / (2 * (1 - kr)))))
    return k


def _frame_struct(ts):
    f = Frame()
    f.y, f.y_batch, f.y_row = ts[0].data_ptr(), ts[0].stride(0), ts[0].stride(1)
    f.u, f.u_batch, f.u_row = ts[1].data_ptr(), ts[1].stride(0), ts[1].stride(1)
    if len(ts) == 3:
        f.v, f.v_batch, f.v_row = ts[2].data_ptr(), ts[2].stride(0), ts[2].stride(1)
    return f


def psnr_from_sse(sse, n, peak):
    """10 log10(peak^2 n / sse) in Python doubles; inf at sse == 0"""
    return 10.0 * math.log10(float(peak) ** 2 * n / sse) if sse > 0 else float("inf")


def _x4_of(x_hat, geom):
    import torch
    if not torch.is_tensor(x_hat):
        raise TypeError("x_hat must be a tensor")
    if x_hat.dtype != torch.float32:
        raise TypeError(f"x_hat must be float32, got {x_hat.dtype}")
    if x_hat.dim() not in (3, 4):
        raise ValueError(f"x_hat must be [B,3,Hp,Wp] or [3,Hp,Wp], got {tuple(x_hat.shape)}")
    x4 = x_hat if x_hat.dim() == 4 else x_hat.unsqueeze(0)
    if x4.shape[1] != 3 or tuple(x4.shape[2:]) != (geom.Hp, geom.Wp) or x4.shape[0] < 1:
        raise ValueError(f"x_hat must be [B,3,{geom.Hp},{geom.Wp}] for {geom}, got {tuple(x_hat.shape)}")
    if geom.H < 1 or geom.W < 1 or geom.top < 0 or geom.left < 0 or geom.top + geom.H > geom.Hp or geom.left + geom.W > geom.Wp:
        raise ValueError(f"{geom}: the window lies outside the planes")
    return x4


_VERBS = ("ingest", "emit_workspace_size", "emit", "plan", "cut", "stitch_workspace_size", "stitch", "workspace_size", "tile_sse")


def _layer(fam, layer):
    """(the module that owns the layer, its error class, {verb: the C symbol of that verb under the module's prefix}), resolved once
    per module.  `lib`, `cut_frame` and every other function are looked up on the module at each call, so a replaced one is used."""
    name, err = fam.owners[layer]
    got = _layers.get(name)
    if got is None:
        mod = importlib.import_module(f"{__package__}.{name}")
        E = getattr(mod, err)
        got = _layers[name] = (mod, E, {v: f"{E._prefix}_{v}" for v in _VERBS})
    return got


def _sited(siting):
    """the siting as trailing positional arguments of a function that takes one only where the stack has sitings"""
    return () if siting is None else (siting,)


def _ref(p):
    return C.byref(p) if p is not None else None


# -- the frame layer -------------------------------------------------------------------------------------------------------------------

def frame_view(fam, planes, fmt, what):
    """Checks a frame (no device call) and returns (planes as batched tensors whose strides fit a pc_frame -- copied only where the
    innermost strides do not --, B, H, W, batched).  The tensors must stay alive while the Frame built from them is in use."""
    import torch
    f = fam.formats[fmt]
    dtype = torch.uint16 if f.bits == 10 else torch.uint8
    n = 3 if f.layout == PLANAR else 2
    if not isinstance(planes, (tuple, list)) or len(planes) != n:
        raise ValueError(f"{what} must be a tuple of {n} planes for {fmt!r}: " + ("(Y, U, V)" if n == 3 else "(Y, UV)"))
    for t in planes:
        if not torch.is_tensor(t):
            raise TypeError(f"{what}: every plane must be a tensor")
        if t.dtype != dtype:
            raise TypeError(f"{what}: the planes of {fmt!r} must be {dtype}, got {t.dtype}")
    y = planes[0]
    if y.dim() not in (2, 3):
        raise ValueError(f"{what}: Y must be [H,W] or [B,H,W], got {tuple(y.shape)}")
    batched = y.dim() == 3
    y = y if batched else y.unsqueeze(0)
    B, H, W = y.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"{what} is empty: Y is {tuple(planes[0].shape)}")
    Hc, Wc = -(-H // f.sy), -(-W // f.sx)
    want = (Hc, Wc) if n == 3 else (Hc, Wc, 2)
    out = [y]
    for name, t in zip("UV" if n == 3 else ("UV",), planes[1:]):
        if t.dim() != len(want) + batched or tuple(t.shape[-len(want):]) != want or (batched and t.shape[0] != B):
            raise ValueError(f"{what}: {name} must be {list((B,) + want) if batched else list(want)} for a {H}x{W} Y plane"
                             f"{fam.plane_of.format(fmt=fmt)}, got {tuple(t.shape)}")
        out.append(t if batched else t.unsqueeze(0))
    for t in out:
        if t.device.type != "cuda":
            raise ValueError(f"{what} must be on a GPU (there is no CPU fallback), got {t.device}")
        if t.device != y.device:
            raise ValueError(f"{what}: the planes lie on different devices")
    fixed = []
    for t in out:
        pair = t.dim() == 4
        ok = t.stride(-1) == 1 and (not pair or t.stride(2) == 2) and t.stride(1) >= t.shape[2] * (2 if pair else 1) and t.stride(0) >= 1
        fixed.append(t if ok else t.contiguous())
    return fixed, B, H, W, batched


def empty_frame(fam, fmt, B, H, W, device):
    """uninitialised contiguous planes of a batch of B frames"""
    import torch
    f = fam.formats[fmt]
    dtype = torch.uint16 if f.bits == 10 else torch.uint8
    Hc, Wc = -(-H // f.sy), -(-W // f.sx)
    y = torch.empty((B, H, W), dtype=dtype, device=device)
    if f.layout == PLANAR:
        return (y, torch.empty((B, Hc, Wc), dtype=dtype, device=device), torch.empty((B, Hc, Wc), dtype=dtype, device=device))
    return (y, torch.empty((B, Hc, Wc, 2), dtype=dtype, device=device))


class Distortion:
    """The sums of one from_model_output(..., ref=...) call.  sse (int64 [B,3], a device tensor): per frame and plane, in the order
    [Y, Cb, Cr], the exact sum of (code - refcode)^2.  psnr_y / psnr_cb / psnr_cr read it back once and compute in Python doubles with
    peak 2^n - 1 over H W (Y) or Hc Wc (chroma) samples."""
    _sub = (2, 2)                                         # (sx, sy)

    def __init__(self, sse, H, W, bits):
        self.sse = sse
        self.H, self.W, self.bits = H, W, bits
        self._host = None

    def _read(self):
        if self._host is None:
            self._host = self.sse.cpu().tolist()
        return self._host

    def _psnr(self, p):
        sx, sy = self._sub
        n = self.H * self.W if p == 0 else -(-self.H // sy) * -(-self.W // sx)
        return [psnr_from_sse(r[p], n, (1 << self.bits) - 1) for r in self._read()]

    def psnr_y(self):
        return self._psnr(0)

    def psnr_cb(self):
        return self._psnr(1)

    def psnr_cr(self):
        return self._psnr(2)


def to_model_input(fam, planes, fmt, matrix, range, upsample, siting, multiple):
    import torch
    M, E, S = _layer(fam, FRAME)
    fam.check(fmt, matrix, range, upsample, *_sited(siting))
    ts, B, H, W, _ = frame_view(fam, planes, fmt, "planes")
    geom = padding(H, W, multiple)
    k = coefficients(matrix)
    dev = ts[0].device
    src = _frame_struct(ts)
    with torch.cuda.device(dev):
        x = torch.empty((B, 3, geom.Hp, geom.Wp), dtype=torch.float32, device=dev)
        rc = getattr(M.lib(), S["ingest"])(C.byref(src), *fam.c_format[fmt, siting], RANGES[range], UPSAMPLES[upsample], k.a, k.b, k.c, k.d,
                                  B, H, W, x.data_ptr(), geom.Hp, geom.Wp, geom.top, geom.left, torch.cuda.current_stream(dev).cuda_stream)
    if rc != PC_OK:
        raise E(rc, S["ingest"])
    return x, geom


def from_model_output(fam, x_hat, geom, fmt, matrix, range, siting, ref, image):
    import torch
    if not image and ref is None:
        raise ValueError("image=False leaves nothing to compute without ref")
    M, E, S = _layer(fam, FRAME)
    fam.check(fmt, matrix, range, None, *_sited(siting))
    geom = Geometry(*geom)
    x4 = _x4_of(x_hat, geom)
    B, H, W = x4.shape[0], geom.H, geom.W
    rts = None
    if ref is not None:
        rts, rB, rH, rW, _ = frame_view(fam, ref, fmt, "ref")
        if (rB, rH, rW) != (B, H, W) or rts[0].device != x4.device:
            raise ValueError(f"ref must hold {B} frame(s) of {H}x{W} on {x4.device}, got {rB} of {rH}x{rW} on {rts[0].device}")
    if x_hat.device.type != "cuda":
        raise ValueError(f"x_hat must be on a GPU (there is no CPU fallback), got {x_hat.device}")
    if x4.stride(3) != 1 or x4.stride(2) < geom.Wp or min(x4.stride()[:2]) < 1:
        x4 = x4.contiguous()
    k = coefficients(matrix)
    L = M.lib()
    with torch.cuda.device(x4.device):
        out = empty_frame(fam, fmt, B, H, W, x4.device) if image else None
        dst = _frame_struct(out) if image else None
        rst = _frame_struct(rts) if rts is not None else None
        ws = sse = None
        nbytes = 0
        if rts is not None:
            nbytes = getattr(L, S["emit_workspace_size"])(B, H, W, *fam.c_sy[fmt])
            ws = torch.empty(nbytes // 8, dtype=torch.int64, device=x4.device)
            sse = torch.empty((B, 3), dtype=torch.int64, device=x4.device)
        rc = getattr(L, S["emit"])(x4.data_ptr(), x4.stride(0), x4.stride(1), x4.stride(2), geom.Hp, geom.Wp, geom.top, geom.left, B, H, W,
                                   *fam.c_format[fmt, siting], RANGES[range], k.kr, k.kg, k.kb, k.ib, k.ir, _ref(dst), _ref(rst),
                                   ws.data_ptr() if ws is not None else None, nbytes, sse.data_ptr() if sse is not None else None,
                                   torch.cuda.current_stream(x4.device).cuda_stream)
    if rc != PC_OK:
        raise E(rc, S["emit"])
    dist = fam.distortion(sse, H, W, fmt) if rts is not None else None
    if not image:
        return dist
    if x_hat.dim() == 3:
        out = tuple(t[0] for t in out)
    return (out, dist) if dist is not None else out


def plan(fam, op, planes, fmt, f32, geom, ref):
    M, E, S = _layer(fam, FRAME)
    fam.check(fmt)
    geom = Geometry(*geom)
    wide = C.c_int(-1)
    fr = _frame_struct(planes) if planes is not None else None
    rf = _frame_struct(ref) if ref is not None else None
    rc = getattr(M.lib(), S["plan"])(op, *fam.c_plan[fmt, FRAME], _ref(fr), f32.data_ptr(), f32.stride(0), f32.stride(1),
                                               f32.stride(2), geom.left, _ref(rf), C.byref(wide))
    if rc != PC_OK:
        raise E(rc, S["plan"])
    return bool(wide.value)


def _head_fields(M, buf):
    """the fields of M's container head after the version byte, and the container's name"""
    from .container import ContainerError
    name = M.MAGIC.decode()
    if len(buf) < 4 or bytes(buf[:4]) != M.MAGIC:
        raise ContainerError(f"not a {name} container")
    if len(buf) < M.HEADER_BYTES:
        raise ContainerError(f"truncated {name} header")
    ver, *fields = struct.unpack_from(M._HEAD, buf, 4)
    if ver != M.VERSION:
        raise ContainerError(f"unsupported {name} version {ver}")
    return fields, name


def pack_frame(fam, blob, fmt, matrix, range, upsample, siting, H, W):
    from . import container
    M = _layer(fam, FRAME)[0]
    fam.check(fmt, matrix, range, upsample, *_sited(siting))
    H, W = int(H), int(W)
    if not (1 <= H < 1 << 32 and 1 <= W < 1 << 32):
        raise container.ContainerError(f"frame size {H}x{W}")
    hd = container.parse_header(blob)
    if tuple(hd["image_size"]) != (H, W):
        raise container.ContainerError(f"the PCB1 blob holds a {hd['image_size'][0]}x{hd['image_size'][1]} image, the frame is {H}x{W}")
    return M.MAGIC + struct.pack(M._HEAD, M.VERSION, *fam.head_of(fmt, matrix, range, upsample, siting), H, W) + bytes(blob)


def parse_frame(fam, buf):
    from . import container
    M = _layer(fam, FRAME)[0]
    fields, name = _head_fields(M, buf)
    params, (H, W) = fam.params_of(fields, name)
    if H < 1 or W < 1:
        raise container.ContainerError(f"corrupt {name} header: frame size {H}x{W}")
    blob = bytes(buf[M.HEADER_BYTES:])
    try:
        hd = container.parse_header(blob)
    except container.ContainerError as e:
        raise container.ContainerError(f"{name}: the PCB1 blob does not parse: {e}") from None
    if tuple(hd["image_size"]) != (H, W):
        raise container.ContainerError(f"{name} header says {H}x{W}, its PCB1 blob {hd['image_size'][0]}x{hd['image_size'][1]}")
    return dict(params, H=H, W=W, blob=blob, pcb1=hd)


def encode_frame(fam, model, planes, qualities, fmt, matrix, range, upsample, siting, mask_pol):
    from . import container
    M = _layer(fam, FRAME)[0]
    qualities = [float(q) for q in qualities]
    x, geom = M.to_model_input(planes, fmt, matrix, range, upsample, *_sited(siting))
    datas = model.compress_levels(x, qualities, mask_pol=mask_pol)
    strings = [d["strings"] for d in datas]
    bufs = [M.pack_frame(container.pack(strings, datas[0]["shape"], qualities, image_size=(geom.H, geom.W), mask_pol=mask_pol, image_index=b),
                         fmt, matrix, range, upsample, *_sited(siting), geom.H, geom.W) for b in _range(x.shape[0])]
    return bufs[0] if planes[0].dim() == 2 else bufs


def decode_frame(fam, model, buf, level, fmt, siting):
    from . import container
    M = _layer(fam, FRAME)[0]
    hd = M.parse_frame(buf)
    out_fmt = hd["fmt"] if fmt is None else fmt
    out_siting = hd.get("siting") if siting is None else siting
    fam.check(out_fmt, None, None, None, *_sited(out_siting))
    pcb = hd["pcb1"]
    n = len(pcb["qualities"])
    lv = int(level) + n if int(level) < 0 else int(level)
    if not 0 <= lv < n:
        raise container.ContainerError(f"no level {level} among {n}")
    geom = padding(hd["H"], hd["W"])
    if tuple(pcb["shape"]) != (geom.Hp // 64, geom.Wp // 64):
        raise container.ContainerError(f"header shape {tuple(pcb['shape'])} is not that of a {geom.H}x{geom.W} frame padded to {geom.Hp}x{geom.Wp}")
    strings, shape, qs, _, mask_pol = container.unpack(hd["blob"], levels=[lv])
    x_hat = model.decompress(strings[0], shape, qs[0], mask_pol)["x_hat"]
    return tuple(t[0] for t in M.from_model_output(x_hat, geom, out_fmt, hd["matrix"], hd["range"], *_sited(out_siting)))


# -- the tiled layer -------------------------------------------------------------------------------------------------------------------

def admissible(fam, window, H, W, fmt):
    """whether (y0, x0, h, w), a window inside an H x W frame of `fmt`, has the frame's own chroma samples: its sy x sx cells"""
    y0, x0, h, w = window
    f = fam.formats[fmt]
    return y0 % f.sy == 0 and x0 % f.sx == 0 and (h % f.sy == 0 or y0 + h == H) and (w % f.sx == 0 or x0 + w == W)


def admissible_window(fam, window, H, W, fmt):
    win = _window((0, 0, H, W) if window is None else window, H, W)
    if not admissible(fam, win, H, W, fmt):
        f = fam.formats[fmt]
        raise ValueError(fam.inadmissible.format(win=win, H=H, W=W, fmt=fmt, sx=f.sx, sy=f.sy))
    return win


def halo_window(fam, window, fmt, siting):
    return window if fam.halo is None else fam.halo(window, fmt, siting)


def covering(fam, grid, window, fmt, siting):
    """the smallest rectangle (ty0, tx0, nty, ntx) of grid a stitch of `window` can be given: every tile that covers a pixel of the
    window extended by its halo; TileGrid.covering where the stack has no halo"""
    return TileGrid(*grid).covering(halo_window(fam, window, fmt, siting))


def one_frame(fam, planes, fmt, what):
    """frame_view for ONE frame: (tensors kept alive, H, W)"""
    import torch
    if isinstance(planes, (tuple, list)) and planes and torch.is_tensor(planes[0]) and planes[0].dim() == 3 and planes[0].shape[0] != 1:
        raise ValueError(f"{what} must be one frame, got a batch of {planes[0].shape[0]}")
    ts, _, H, W, _ = frame_view(fam, planes, fmt, what)
    return ts, H, W


def _cut(fam, L, E, S, src, fmt, siting, range, upsample, k, g, rect, ptr, stream):
    """one <prefix>_cut launch: the tiles of rect = (ty0, tx0, nty, ntx) of the frame src, written row-major at ptr"""
    rc = getattr(L, S["cut"])(C.byref(src), *fam.c_format[fmt, siting], RANGES[range], UPSAMPLES[upsample], k.a, k.b, k.c,
                                        k.d, g.H, g.W, g.T, g.O, *rect, ptr, stream)
    if rc != PC_OK:
        raise E(rc, S["cut"])


def cut_frame(fam, planes, fmt, matrix, range, upsample, siting, tile, overlap, rect):
    import torch
    M, E, S = _layer(fam, TILED)
    fam.check(fmt, matrix, range, upsample, *_sited(siting))
    ts, H, W = one_frame(fam, planes, fmt, "planes")
    g = grid_of(H, W, tile, overlap)
    if rect is not None:
        g = g.with_rect(rect)
    k = coefficients(matrix)
    dev = ts[0].device
    src = _frame_struct(ts)
    with torch.cuda.device(dev):
        out = torch.empty((g.n, 3, g.T, g.T), dtype=torch.float32, device=dev)
        _cut(fam, M.lib(), E, S, src, fmt, siting, range, upsample, k, g, g.rect, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return out, g


def offset_frame(fam, ts, fmt, y0, x0):
    """the Frame of the window whose first luma sample is (y0, x0) (multiples of sy, sx) of the frame held by the batched tensors ts"""
    f_ = fam.formats[fmt]
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


def full_grid(grid):
    g = TileGrid(*grid)
    full = grid_of(g.H, g.W, g.T, g.O)
    if (full.ny, full.nx) != (g.ny, g.nx):
        raise ValueError(f"{g}: the grid of a {g.H}x{g.W} frame is {full.ny}x{full.nx}")
    return full.with_rect(g.rect)


def stitch_frame(fam, x_hat_tiles, grid, fmt, matrix, range, siting, window, ref, image):
    import torch
    if not image and ref is None:
        raise ValueError("image=False leaves nothing to compute without ref")
    M, E, S = _layer(fam, TILED)
    fam.check(fmt, matrix, range, None, *_sited(siting))
    g = full_grid(grid)
    _check_tiles(x_hat_tiles, g)
    win = y0, x0, h, w = admissible_window(fam, window, g.H, g.W, fmt)
    need = covering(fam, g, win, fmt, siting)
    if need[0] < g.ty0 or need[1] < g.tx0 or need[0] + need[2] > g.ty0 + g.nty or need[1] + need[3] > g.tx0 + g.ntx:
        halo = "" if fam.halo is None else f" with its halo {fam.halo(win, fmt, siting)}"
        raise ValueError(f"window {win}{halo} needs the tiles {need}, x_hat_tiles holds {g.rect}")
    x = x_hat_tiles
    rts = None
    if ref is not None:
        rts, rH, rW = one_frame(fam, ref, fmt, "ref")
        if (rH, rW) != (g.H, g.W) or rts[0].device != x.device:
            raise ValueError(f"ref must be the {g.H}x{g.W} frame on {x.device}, got {rH}x{rW} on {rts[0].device}")
    if x.device.type != "cuda":
        raise ValueError(f"x_hat_tiles must be on a GPU (there is no CPU fallback), got {x.device}")
    x = _fit_tiles(x, g.T)
    k = coefficients(matrix)
    L = M.lib()
    with torch.cuda.device(x.device):
        out = empty_frame(fam, fmt, 1, h, w, x.device) if image else None
        dst = _frame_struct(out) if image else None
        rst = offset_frame(fam, rts, fmt, y0, x0) if rts is not None else None
        ws = sse = None
        nbytes = 0
        if rts is not None:
            nbytes = getattr(L, S["stitch_workspace_size"])(x0, h, w, *fam.c_sy[fmt])
            ws = torch.empty(nbytes // 8, dtype=torch.int64, device=x.device)
            sse = torch.empty((1, 3), dtype=torch.int64, device=x.device)
        rc = getattr(L, S["stitch"])(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), g.H, g.W, g.T, g.O, *g.rect, y0, x0, h, w,
                                     *fam.c_format[fmt, siting], RANGES[range], k.kr, k.kg, k.kb, k.ib, k.ir, _ref(dst), _ref(rst),
                                     ws.data_ptr() if ws is not None else None, nbytes, sse.data_ptr() if sse is not None else None,
                                     torch.cuda.current_stream(x.device).cuda_stream)
    del rts
    if rc != PC_OK:
        raise E(rc, S["stitch"])
    dist = fam.distortion(sse, h, w, fmt) if sse is not None else None
    if not image:
        return dist
    out = tuple(t[0] for t in out)
    return (out, dist) if dist is not None else out


def tiled_plan(fam, op, planes, fmt, f32, overlap, x0, ref):
    M, E, S = _layer(fam, TILED)
    fam.check(fmt)
    wide = C.c_int(-1)
    fr = _frame_struct(planes) if planes is not None else None
    rf = _frame_struct(ref) if ref is not None else None
    rc = getattr(M.lib(), S["plan"])(op, *fam.c_plan[fmt, TILED], _ref(fr), f32.data_ptr(), f32.stride(0), f32.stride(1),
                                               f32.stride(2), int(overlap), int(x0), _ref(rf), C.byref(wide))
    if rc != PC_OK:
        raise E(rc, S["plan"])
    return bool(wide.value)


def _parse_inner(name, inner):
    from . import container, tiles
    try:
        return tiles.parse_tiled(inner)
    except container.ContainerError as e:
        raise container.ContainerError(f"{name}: the inner container does not parse: {e}") from None


def pack_frame_tiled(fam, inner, fmt, matrix, range, upsample, siting):
    M = _layer(fam, TILED)[0]
    fam.check(fmt, matrix, range, upsample, *_sited(siting))
    _parse_inner(M.MAGIC.decode(), inner)
    return M.MAGIC + struct.pack(M._HEAD, M.VERSION, *fam.head_of(fmt, matrix, range, upsample, siting)) + bytes(inner)


def parse_frame_tiled(fam, buf):
    M = _layer(fam, TILED)[0]
    fields, name = _head_fields(M, buf)
    params, _ = fam.params_of(fields, name)
    inner = bytes(buf[M.HEADER_BYTES:])
    hd = _parse_inner(name, inner)
    g = hd["grid"]
    return dict(params, H=g.H, W=g.W, inner=inner, tiled=hd)


def encode_frame_tiled(fam, model, planes, qualities, fmt, matrix, range, upsample, siting, tile, overlap, mask_pol, max_tiles_per_call):
    from . import tiles
    M = _layer(fam, TILED)[0]
    qualities = [float(q) for q in qualities]
    step = _tilecodec.tiles_per_call(max_tiles_per_call)
    x, g = M.cut_frame(planes, fmt, matrix, range, upsample, *_sited(siting), tile, overlap)       # the whole frame in one launch
    bufs = _tilecodec.encode_items(model, g.n, step, qualities, mask_pol, g.T, lambda a, b: x[a:a + b])
    return M.pack_frame_tiled(tiles.pack_tiled(bufs, g.H, g.W, g.T, g.O), fmt, matrix, range, upsample, *_sited(siting))


def decode_frame_tiled(fam, model, buf, level, region, fmt, siting, max_tiles_per_call):
    from . import container, tiles
    M = _layer(fam, TILED)[0]
    step = _tilecodec.tiles_per_call(max_tiles_per_call)
    hd = M.parse_frame_tiled(buf)
    out_fmt = hd["fmt"] if fmt is None else fmt
    out_siting = hd.get("siting") if siting is None else siting
    fam.check(out_fmt, None, None, None, *_sited(out_siting))
    try:
        window = admissible_window(fam, region, hd["H"], hd["W"], out_fmt)
    except ValueError as e:
        raise container.ContainerError(str(e)) from None
    x_hat, g, _ = tiles._decode_region_tiles(model, hd["inner"], level, halo_window(fam, window, out_fmt, out_siting), step)
    return M.stitch_frame(x_hat, g, out_fmt, hd["matrix"], hd["range"], *_sited(out_siting), window=window)


# -- the rate layer --------------------------------------------------------------------------------------------------------------------

def frame_tile_distortion(fam, x_hat_tiles, grid, ref, fmt, matrix, range, siting, first_tile):
    import torch
    M, E, S = _layer(fam, RATE)
    fam.check(fmt, matrix, range, None, *_sited(siting))
    g, n, x = _linear_tiles(grid, x_hat_tiles, first_tile, "frame", _tilecodec.tile_limit, fmt)
    rts, rH, rW = one_frame(fam, ref, fmt, "ref")
    if (rH, rW) != (g.H, g.W) or rts[0].device != x.device:
        raise ValueError(f"ref must be the {g.H}x{g.W} frame on {x.device}, got {rH}x{rW} on {rts[0].device}")
    if x.device.type != "cuda":
        raise ValueError(f"x_hat_tiles must be on a GPU (there is no CPU fallback), got {x.device}")
    k = coefficients(matrix)
    L = M.lib()
    rst = _frame_struct(rts)
    with torch.cuda.device(x.device):
        nbytes = getattr(L, S["workspace_size"])(g.T, *fam.c_sy[fmt], n)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=x.device)
        out = torch.empty((n, 3), dtype=torch.int64, device=x.device)
        rc = getattr(L, S["tile_sse"])(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), g.H, g.W, g.T, g.O, int(first_tile), n,
                                                 *fam.c_format[fmt, siting], RANGES[range], k.kr, k.kg, k.kb, k.ib, k.ir, C.byref(rst),
                                                 ws.data_ptr(), nbytes, out.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream)
    del rts
    if rc != PC_OK:
        raise E(rc, S["tile_sse"])
    return out


def rate_plan(fam, x_hat_tiles, ref, fmt, overlap):
    M, E, S = _layer(fam, RATE)
    fam.check(fmt)
    x = x_hat_tiles
    wide = C.c_int(-1)
    rf = _frame_struct(ref)
    rc = getattr(M.lib(), S["plan"])(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), int(overlap), *fam.c_plan[fmt, RATE],
                                               C.byref(rf), C.byref(wide))
    if rc != PC_OK:
        raise E(rc, S["plan"])
    return bool(wide.value)


def encode_frame_tiled_to_size(fam, model, planes, qualities, target_bytes, fmt, matrix, range, upsample, siting, tile, overlap, mask_pol,
                               plane_weights, importance, max_tiles_per_call):
    """-> (the container, the fields of FrameRatePlan in order, the frame's whole grid)"""
    import torch
    from . import rate, tiles
    M = _layer(fam, RATE)[0]
    TM, TE, TS = _layer(fam, TILED)
    qualities = _tilecodec.levels_of(qualities)
    fam.check(fmt, matrix, range, upsample, *_sited(siting))
    step = _tilecodec.tiles_per_call(max_tiles_per_call)
    pw = _tilecodec.plane_weights_of(plane_weights)
    target_bytes = int(target_bytes)
    ts, H, W = one_frame(fam, planes, fmt, "planes")
    g = grid_of(H, W, tile, overlap)
    _tilecodec.tile_limit(g.T, fmt)
    n = g.ny * g.nx
    importance = _tilecodec.importance_of(importance, g)
    k = coefficients(matrix)
    dev = ts[0].device
    src = _frame_struct(ts)
    CL = TM.lib()

    def cut(a, b):
        with torch.cuda.device(dev):
            x = torch.empty((b, 3, g.T, g.T), dtype=torch.float32, device=dev)
            m0 = 0
            for i, j, m in _tilecodec.row_pieces(a, b, g.nx):
                _cut(fam, CL, TE, TS, src, fmt, siting, range, upsample, k, g, (i, j, 1, m), x[m0:].data_ptr(),
                     torch.cuda.current_stream(dev).cuda_stream)
                m0 += m
        return x

    def measure(a, b, decoded):
        d = torch.stack([M.frame_tile_distortion(o["x_hat"], g, ts, fmt, matrix, range, *_sited(siting), a) for o in decoded], 1).tolist()
        return [[[int(v) for v in row] for row in per_level] for per_level in d]                                # [b][levels][3]
    bufs, plane_dists = _tilecodec.encode_items(model, n, step, qualities, mask_pol, g.T, cut, measure)
    del ts
    rates = [[rate.TABLE_ENTRY_BYTES + len(p) for p in row] for row in bufs]
    dists = [[pw[0] * v[0] + pw[1] * v[1] + pw[2] * v[2] for v in row] for row in plane_dists]
    levels = rate.allocate(rates, dists, target_bytes - TM.HEADER_BYTES - tiles.HEADER_BYTES, importance)
    inner = tiles.pack_tiled([bufs[t][levels[t]] for t in _range(n)], g.H, g.W, g.T, g.O, per_tile_levels=True)
    buf = TM.pack_frame_tiled(inner, fmt, matrix, range, upsample, *_sited(siting))
    sse = [sum(plane_dists[t][levels[t]][p] for t in _range(n)) for p in _range(3)]
    return buf, (levels, rates, dists, plane_dists, 2 * g.O if g.O else 1, len(buf), sum(dists[t][levels[t]] for t in _range(n)), sse), g

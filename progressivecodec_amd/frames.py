"""YUV 4:2:0 frames in, YUV 4:2:0 frames out (libpc_frames.so, frames_csrc/pc_frames.h): what stands between
the surfaces a video or JPEG decoder leaves in device memory (NV12, I420, P010) and the codec's float32 RGB [B,3,H,W] planes with H, W
multiples of 64, and back.

  to_model_input      frame -> centre-padded float RGB planes (chroma upsampled on the integer codes, range expansion, the 3x3
                      matrix, clamp, pad), one kernel
  from_model_output   decoder output -> frame of the chosen format (clamp, matrix, 2x2 chroma mean, rounding) and, given the original
                      frame, the per-plane distortion sums behind PSNR-Y / Cb / Cr, one kernel (plus a small reduction)
  encode_frame        frame -> one PCF1 container per picture: a fixed header and one unmodified PCB1 blob (container.py)
  decode_frame        PCF1 container -> frame of the original size, in the stored format or another

A frame is a tuple of cuda tensors: (Y, UV) for "nv12" (uint8) and "p010" (uint16, the 10-bit code in the upper bits), (Y, U, V) for
"i420" (uint8).  Y is [H,W] or [B,H,W]; UV is [Hc,Wc,2] or [B,Hc,Wc,2]; U and V are [Hc,Wc] or [B,Hc,Wc]; Hc = ceil(H/2),
Wc = ceil(W/2).  Any row and batch strides are taken as they are (pitched surfaces, views into larger allocations); only a plane whose
innermost stride is not 1 (2 for the pair) is copied.  There is no CPU fallback: CPU tensors raise ValueError before any device call.
Everything runs on the current stream of the tensor's device.
"""
import collections
import ctypes as C
import math
import struct

from . import _imagelib, _tilecodec
from ._lib import PC_OK
from .pixels import Geometry, padding

LIB_PATH = _imagelib.lib_path("frames")

#: every symbol frames_csrc/pc_frames.h declares
EXPORTS = ["pc_frames_ingest", "pc_frames_emit_workspace_size", "pc_frames_emit", "pc_frames_plan", "pc_frames_strerror",
           "pc_frames_last_hip_error"]

FORMATS = {"nv12": 0, "i420": 1, "p010": 2}               # PC_FRAMES_NV12, PC_FRAMES_I420, PC_FRAMES_P010
RANGES = {"limited": 0, "full": 1}                        # PC_FRAMES_LIMITED, PC_FRAMES_FULL
UPSAMPLES = {"nearest": 0, "linear": 1}                   # PC_FRAMES_NEAREST, PC_FRAMES_LINEAR
MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}     # (Kr, Kb); Kg = 1 - Kr - Kb
INGEST, EMIT = 0, 1                                       # pc_frames_plan's `op`

_range = range                                            # the functions below take a parameter of that name


class Frame(C.Structure):
    """pc_frame: three planes, each a pointer with batch and row strides in elements"""
    _fields_ = [("y", C.c_void_p), ("y_batch", C.c_int64), ("y_row", C.c_int64),
                ("u", C.c_void_p), ("u_batch", C.c_int64), ("u_row", C.c_int64),
                ("v", C.c_void_p), ("v_batch", C.c_int64), ("v_row", C.c_int64)]


def _prototypes():
    i64, vp, ci, cf, fp = C.c_int64, C.c_void_p, C.c_int, C.c_float, C.POINTER(Frame)
    return {
        "pc_frames_ingest": (None, [fp, ci, ci, ci, cf, cf, cf, cf, ci, ci, ci, vp, ci, ci, ci, ci, vp]),
        "pc_frames_emit_workspace_size": (C.c_size_t, [ci, ci, ci]),
        "pc_frames_emit": (None, [vp, i64, i64, i64, ci, ci, ci, ci, ci, ci, ci, ci, ci, cf, cf, cf, cf, cf, fp, fp, vp, C.c_size_t,
                                  vp, vp]),
        "pc_frames_plan": (None, [ci, ci, fp, vp, i64, i64, i64, ci, fp, C.POINTER(ci)]),
        "pc_frames_strerror": (C.c_char_p, [ci]),
    }


def lib():
    return _imagelib.load(LIB_PATH, _prototypes)


class FramesError(_imagelib.ImageLibError):
    _lib, _prefix = staticmethod(lib), "pc_frames"


def bits_of(fmt):
    return 10 if fmt == "p010" else 8


def levels(fmt, range):
    """(yo, ys, co, cs, max code) of the format's bit depth and the range"""
    n = bits_of(fmt)
    s, top = 1 << (n - 8), (1 << n) - 1
    if range == "limited":
        return 16 * s, 219 * s, 128 * s, 224 * s, top
    if range == "full":
        return 0, top, 128 * s, top, top
    raise ValueError(f"range must be 'limited' or 'full', got {range!r}")


def _f32(v):
    """a Python double rounded once to float32 (and held as the double of that value)"""
    return struct.unpack("<f", struct.pack("<f", v))[0]


Coefficients = collections.namedtuple("Coefficients", "a b c d kr kg kb ib ir")


def coefficients(matrix):
    """The nine float32 coefficients of a matrix, each computed in float64 from Kr and Kb and rounded once: the reconstruction factors
    a = 2(1-Kr), b = 2Kb(1-Kb)/Kg, c = 2Kr(1-Kr)/Kg, d = 2(1-Kb); the luma weights Kr, Kg, Kb; the chroma factors ib = 1/(2(1-Kb)),
    ir = 1/(2(1-Kr)).  What the kernels and the restatement both take."""
    if matrix not in MATRICES:
        raise ValueError(f"matrix must be one of {sorted(MATRICES)}, got {matrix!r}")
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    return Coefficients(*map(_f32, (2 * (1 - kr), 2 * kb * (1 - kb) / kg, 2 * kr * (1 - kr) / kg, 2 * (1 - kb), kr, kg, kb,
                                    1 / (2 * (1 - kb)), 1 / (2 * (1 - kr)))))


def chroma_size(h, w):
    return (int(h) + 1) // 2, (int(w) + 1) // 2


def _check_enums(fmt, matrix=None, range=None, upsample=None):
    if fmt not in FORMATS:
        raise ValueError(f"fmt must be one of {sorted(FORMATS)}, got {fmt!r}")
    if matrix is not None and matrix not in MATRICES:
        raise ValueError(f"matrix must be one of {sorted(MATRICES)}, got {matrix!r}")
    if range is not None and range not in RANGES:
        raise ValueError(f"range must be 'limited' or 'full', got {range!r}")
    if upsample is not None and upsample not in UPSAMPLES:
        raise ValueError(f"upsample must be 'nearest' or 'linear', got {upsample!r}")


def _frame_view(planes, fmt, what):
    """Checks a frame (no device call) and returns (planes as batched tensors whose strides fit a pc_frame -- copied only where the
    innermost strides do not --, B, H, W, batched).  The tensors must stay alive while the Frame built from them is in use."""
    import torch
    dtype = torch.uint16 if fmt == "p010" else torch.uint8
    n = 3 if fmt == "i420" else 2
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
    Hc, Wc = chroma_size(H, W)
    want = (Hc, Wc) if n == 3 else (Hc, Wc, 2)
    out = [y]
    for name, t in zip("UV" if n == 3 else ("UV",), planes[1:]):
        if t.dim() != len(want) + batched or tuple(t.shape[-len(want):]) != want or (batched and t.shape[0] != B):
            raise ValueError(f"{what}: {name} must be {list((B,) + want) if batched else list(want)} for a {H}x{W} Y plane, got {tuple(t.shape)}")
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


def _frame_struct(ts):
    f = Frame()
    f.y, f.y_batch, f.y_row = ts[0].data_ptr(), ts[0].stride(0), ts[0].stride(1)
    f.u, f.u_batch, f.u_row = ts[1].data_ptr(), ts[1].stride(0), ts[1].stride(1)
    if len(ts) == 3:
        f.v, f.v_batch, f.v_row = ts[2].data_ptr(), ts[2].stride(0), ts[2].stride(1)
    return f


def empty_frame(fmt, B, H, W, device):
    """uninitialised contiguous planes of a batch of B frames"""
    import torch
    dtype = torch.uint16 if fmt == "p010" else torch.uint8
    Hc, Wc = chroma_size(H, W)
    y = torch.empty((B, H, W), dtype=dtype, device=device)
    if fmt == "i420":
        return (y, torch.empty((B, Hc, Wc), dtype=dtype, device=device), torch.empty((B, Hc, Wc), dtype=dtype, device=device))
    return (y, torch.empty((B, Hc, Wc, 2), dtype=dtype, device=device))


def to_model_input(planes, fmt, matrix="bt709", range="limited", upsample="linear", multiple=64):
    """frame -> (x_padded, geom): float32 RGB [B,3,Hp,Wp] as DESIGN.md section 13 defines it bit for bit (every padded element +0.0,
    written by the same launch), and geom = pixels.padding(H, W, multiple)."""
    import torch
    _check_enums(fmt, matrix, range, upsample)
    ts, B, H, W, _ = _frame_view(planes, fmt, "planes")
    geom = padding(H, W, multiple)
    k = coefficients(matrix)
    dev = ts[0].device
    src = _frame_struct(ts)
    with torch.cuda.device(dev):
        x = torch.empty((B, 3, geom.Hp, geom.Wp), dtype=torch.float32, device=dev)
        rc = lib().pc_frames_ingest(C.byref(src), FORMATS[fmt], RANGES[range], UPSAMPLES[upsample], k.a, k.b, k.c, k.d, B, H, W,
                                    x.data_ptr(), geom.Hp, geom.Wp, geom.top, geom.left, torch.cuda.current_stream(dev).cuda_stream)
    if rc != PC_OK:
        raise FramesError(rc, "pc_frames_ingest")
    return x, geom


def psnr_from_sse(sse, n, peak):
    """10 log10(peak^2 n / sse) in Python doubles; inf at sse == 0"""
    return 10.0 * math.log10(float(peak) ** 2 * n / sse) if sse > 0 else float("inf")


class Distortion:
    """The sums of one from_model_output(..., ref=...) call.  sse (int64 [B,3], a device tensor): per frame and plane, in the order
    [Y, Cb, Cr], the exact sum of (code - refcode)^2.  psnr_y / psnr_cb / psnr_cr read it back once and compute in Python doubles with
    peak 2^n - 1 over H W (Y) or Hc Wc (chroma) samples."""

    def __init__(self, sse, H, W, bits):
        self.sse = sse
        self.H, self.W, self.bits = H, W, bits
        self._host = None

    def _read(self):
        if self._host is None:
            self._host = self.sse.cpu().tolist()
        return self._host

    def _psnr(self, p):
        Hc, Wc = chroma_size(self.H, self.W)
        n = self.H * self.W if p == 0 else Hc * Wc
        return [psnr_from_sse(r[p], n, (1 << self.bits) - 1) for r in self._read()]

    def psnr_y(self):
        return self._psnr(0)

    def psnr_cb(self):
        return self._psnr(1)

    def psnr_cr(self):
        return self._psnr(2)


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


def from_model_output(x_hat, geom, fmt, matrix="bt709", range="limited", ref=None, image=True):
    """x_hat: float32 cuda [B,3,Hp,Wp] (or [3,Hp,Wp]; any batch / channel / row strides, unit stride along W) -> the frame of the
    window geom in `fmt` (a tuple of contiguous planes; without the batch axis for a 3-D x_hat), as DESIGN.md section 13 defines it.
    With ref (the original frame in `fmt`) returns (frame, Distortion); with image=False (needs ref) no frame is allocated or written
    and the Distortion alone is returned."""
    import torch
    if not image and ref is None:
        raise ValueError("image=False leaves nothing to compute without ref")
    _check_enums(fmt, matrix, range)
    geom = Geometry(*geom)
    x4 = _x4_of(x_hat, geom)
    B, H, W = x4.shape[0], geom.H, geom.W
    rts = None
    if ref is not None:
        rts, rB, rH, rW, _ = _frame_view(ref, fmt, "ref")
        if (rB, rH, rW) != (B, H, W) or rts[0].device != x4.device:
            raise ValueError(f"ref must hold {B} frame(s) of {H}x{W} on {x4.device}, got {rB} of {rH}x{rW} on {rts[0].device}")
    if x_hat.device.type != "cuda":
        raise ValueError(f"x_hat must be on a GPU (there is no CPU fallback), got {x_hat.device}")
    if x4.stride(3) != 1 or x4.stride(2) < geom.Wp or min(x4.stride()[:2]) < 1:
        x4 = x4.contiguous()
    k = coefficients(matrix)
    L = lib()
    with torch.cuda.device(x4.device):
        out = empty_frame(fmt, B, H, W, x4.device) if image else None
        dst = _frame_struct(out) if image else None
        rst = _frame_struct(rts) if rts is not None else None
        ws = sse = None
        nbytes = 0
        if rts is not None:
            nbytes = L.pc_frames_emit_workspace_size(B, H, W)
            ws = torch.empty(nbytes // 8, dtype=torch.int64, device=x4.device)
            sse = torch.empty((B, 3), dtype=torch.int64, device=x4.device)
        rc = L.pc_frames_emit(x4.data_ptr(), x4.stride(0), x4.stride(1), x4.stride(2), geom.Hp, geom.Wp, geom.top, geom.left, B, H, W,
                              FORMATS[fmt], RANGES[range], k.kr, k.kg, k.kb, k.ib, k.ir, C.byref(dst) if dst is not None else None,
                              C.byref(rst) if rst is not None else None, ws.data_ptr() if ws is not None else None, nbytes,
                              sse.data_ptr() if sse is not None else None, torch.cuda.current_stream(x4.device).cuda_stream)
    if rc != PC_OK:
        raise FramesError(rc, "pc_frames_emit")
    dist = Distortion(sse, H, W, bits_of(fmt)) if rts is not None else None
    if not image:
        return dist
    if x_hat.dim() == 3:
        out = tuple(t[0] for t in out)
    return (out, dist) if dist is not None else out


def plan(op, planes, fmt, f32, geom, ref=None):
    """pc_frames_plan for tensors (host only, nothing is launched or copied): True where the ingest (op = INGEST: planes the source,
    f32 the padded destination) or the emit (op = EMIT: planes the destination or None, f32 x_hat) of exactly these tensors takes the
    wide-access path.  planes and ref are tuples of batched tensors whose strides already fit a pc_frame."""
    _check_enums(fmt)
    geom = Geometry(*geom)
    wide = C.c_int(-1)
    fr = _frame_struct(planes) if planes is not None else None
    rf = _frame_struct(ref) if ref is not None else None
    rc = lib().pc_frames_plan(op, FORMATS[fmt], C.byref(fr) if fr is not None else None, f32.data_ptr(), f32.stride(0), f32.stride(1),
                              f32.stride(2), geom.left, C.byref(rf) if rf is not None else None, C.byref(wide))
    if rc != PC_OK:
        raise FramesError(rc, "pc_frames_plan")
    return bool(wide.value)


# -- PCF1: a frame's parameters in front of one PCB1 blob ---------------------------------------------------------------------------

MAGIC = b"PCF1"
VERSION = 1
_HEAD = "<BBBBBBII"          # version, fmt, matrix, range, upsample, bits, H, W
HEADER_BYTES = 4 + struct.calcsize(_HEAD)
_MATRIX_ID = {"bt601": 0, "bt709": 1, "bt2020": 2}


def _inv(d):
    return {v: k for k, v in d.items()}


def pack_frame(blob, fmt, matrix, range, upsample, H, W):
    """PCF1: the magic, the version byte, fmt, matrix, range, upsample and bits as one byte each, H and W as little-endian uint32, then
    the PCB1 blob unmodified."""
    from . import container
    _check_enums(fmt, matrix, range, upsample)
    H, W = int(H), int(W)
    if not (1 <= H < 1 << 32 and 1 <= W < 1 << 32):
        raise container.ContainerError(f"frame size {H}x{W}")
    hd = container.parse_header(blob)
    if tuple(hd["image_size"]) != (H, W):
        raise container.ContainerError(f"the PCB1 blob holds a {hd['image_size'][0]}x{hd['image_size'][1]} image, the frame is {H}x{W}")
    return MAGIC + struct.pack(_HEAD, VERSION, FORMATS[fmt], _MATRIX_ID[matrix], RANGES[range], UPSAMPLES[upsample], bits_of(fmt), H, W) + bytes(blob)


def parse_frame(buf):
    """-> dict(fmt, matrix, range, upsample, bits, H, W, blob (the PCB1 container), pcb1 (its parsed header)).  ContainerError on a bad
    magic, version, enum, bit depth, size or length; nothing else is touched."""
    from . import container
    if len(buf) < 4 or bytes(buf[:4]) != MAGIC:
        raise container.ContainerError("not a PCF1 container")
    if len(buf) < HEADER_BYTES:
        raise container.ContainerError("truncated PCF1 header")
    ver, f, m, r, u, bits, H, W = struct.unpack_from(_HEAD, buf, 4)
    if ver != VERSION:
        raise container.ContainerError(f"unsupported PCF1 version {ver}")
    params = _tilecodec.frame_params(f, m, r, u, bits, "PCF1")
    if H < 1 or W < 1:
        raise container.ContainerError(f"corrupt PCF1 header: frame size {H}x{W}")
    blob = bytes(buf[HEADER_BYTES:])
    try:
        hd = container.parse_header(blob)
    except container.ContainerError as e:
        raise container.ContainerError(f"PCF1: the PCB1 blob does not parse: {e}") from None
    if tuple(hd["image_size"]) != (H, W):
        raise container.ContainerError(f"PCF1 header says {H}x{W}, its PCB1 blob {hd['image_size'][0]}x{hd['image_size'][1]}")
    return dict(params, H=H, W=W, blob=blob, pcb1=hd)


def encode_frame(model, planes, qualities, fmt, matrix="bt709", range="limited", upsample="linear", mask_pol="point-based-std"):
    """frame(s) -> PCF1 container(s) holding every level of `qualities`: `bytes` for one frame (Y is [H,W]), a list with one `bytes`
    per frame for a batch.  The PCB1 blob inside is what pixels.encode_image would pack for the same planes and levels, so
    pixels.decode_image of it gives the RGB rendering."""
    from . import container
    qualities = [float(q) for q in qualities]
    x, geom = to_model_input(planes, fmt, matrix, range, upsample)
    datas = model.compress_levels(x, qualities, mask_pol=mask_pol)
    strings = [d["strings"] for d in datas]
    bufs = [pack_frame(container.pack(strings, datas[0]["shape"], qualities, image_size=(geom.H, geom.W), mask_pol=mask_pol, image_index=b),
                       fmt, matrix, range, upsample, geom.H, geom.W) for b in _range(x.shape[0])]
    return bufs[0] if planes[0].dim() == 2 else bufs


def decode_frame(model, buf, level=-1, fmt=None):
    """One level (index into the container's quality list, negative from the end) of a PCF1 container -> the frame (a tuple of planes
    without a batch axis) on the model's device, in the stored format or in `fmt` when given (the stored matrix and range either way;
    another bit depth is computed from the decoder's float output, not converted from codes).  Only the header, the base segment and
    that level's segment are read; every refusal comes before the model is touched."""
    from . import container
    hd = parse_frame(buf)
    out_fmt = hd["fmt"] if fmt is None else fmt
    _check_enums(out_fmt)
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
    return tuple(t[0] for t in from_model_output(x_hat, geom, out_fmt, hd["matrix"], hd["range"]))


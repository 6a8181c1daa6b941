"""YUV frames of any chroma subsampling and siting in and out (libpc_chroma.so, chroma_hip/pc_chroma.h): what
`frames` is for NV12 / I420 / P010 with centre-sited chroma, for 4:2:0, 4:2:2 and 4:4:4, planar and semi-planar, 8-bit and 10-bit
surfaces whose chroma is sited at the centre of its luma samples, on the left luma column or on the top-left luma sample.

  to_model_input      frame -> centre-padded float RGB planes (chroma upsampled on the integer codes for the frame's siting, range
                      expansion, the 3x3 matrix, clamp, pad), one kernel
  from_model_output   decoder output -> frame of the chosen format and siting (clamp, matrix, chroma filter, rounding) and, given the
                      original frame, the per-plane distortion sums behind PSNR-Y / Cb / Cr, one kernel (plus a small reduction)
  encode_frame        frame -> one PCH1 container per picture: a fixed header and one unmodified PCB1 blob (container.py)
  decode_frame        PCH1 container -> frame of the original size, in the stored format and siting or another

FORMATS names twelve formats as (layout, bits, shift, sx, sy):

                                                       4:2:0     4:2:2     4:4:4
  planar, 8-bit (Y, U, V)                              "i420"    "i422"    "i444"
  semi-planar, 8-bit (Y, interleaved CbCr)             "nv12"    "nv16"    "nv24"
  semi-planar, 16-bit words, 10-bit code << 6          "p010"    "p210"    "p410"
  planar, 16-bit words, 10-bit code in the low bits    "i010"    "i210"    "i410"     (yuv420p10le, yuv422p10le, yuv444p10le)

siting is "centre" (JPEG / JFIF, MPEG-1, and what `frames` assumes), "left" (chroma on the even luma columns, midway between two
rows: the default of MPEG-2, H.264 and HEVC streams, `chroma_sample_loc_type` 0) or "topleft" (chroma on the even luma sample of the
even row: BT.2020 / BT.2100 UHD and HDR material, `chroma_sample_loc_type` 2).  An axis that is not subsampled ignores its part:
4:2:2 treats "left" and "topleft" alike, 4:4:4 all three.

A frame is a tuple of cuda tensors: (Y, UV) for the semi-planar formats, (Y, U, V) for the planar ones; uint8, or uint16 for the
10-bit formats.  Y is [H,W] or [B,H,W]; UV is [Hc,Wc,2] or [B,Hc,Wc,2]; U and V are [Hc,Wc] or [B,Hc,Wc]; Hc = ceil(H/sy),
Wc = ceil(W/sx).  Any row and batch strides are taken as they are; only a plane whose innermost stride is not 1 (2 for the pair) is
copied.  There is no CPU fallback: CPU tensors raise ValueError before any device call.  Everything runs on the current stream of the
tensor's device.
"""
import collections
import ctypes as C
import struct

from . import _imagelib
from ._lib import PC_OK
from .frames import MATRICES, RANGES, UPSAMPLES, Frame, coefficients, psnr_from_sse, _x4_of, _frame_struct
from .pixels import Geometry, padding

LIB_PATH = _imagelib.lib_path("chroma")

#: every symbol chroma_hip/pc_chroma.h declares
EXPORTS = ["pc_chroma_ingest", "pc_chroma_emit_workspace_size", "pc_chroma_emit", "pc_chroma_plan", "pc_chroma_strerror",
           "pc_chroma_last_hip_error"]

Format = collections.namedtuple("Format", "layout bits shift sx sy")
PLANAR, SEMIPLANAR = 0, 1                                 # PC_CH_PLANAR, PC_CH_SEMIPLANAR
FORMATS = {
    "i420": Format(PLANAR, 8, 0, 2, 2), "i422": Format(PLANAR, 8, 0, 2, 1), "i444": Format(PLANAR, 8, 0, 1, 1),
    "nv12": Format(SEMIPLANAR, 8, 0, 2, 2), "nv16": Format(SEMIPLANAR, 8, 0, 2, 1), "nv24": Format(SEMIPLANAR, 8, 0, 1, 1),
    "p010": Format(SEMIPLANAR, 10, 6, 2, 2), "p210": Format(SEMIPLANAR, 10, 6, 2, 1), "p410": Format(SEMIPLANAR, 10, 6, 1, 1),
    "i010": Format(PLANAR, 10, 0, 2, 2), "i210": Format(PLANAR, 10, 0, 2, 1), "i410": Format(PLANAR, 10, 0, 1, 1),
}
CENTRE, COSITED = 0, 1                                    # PC_CH_CENTRE, PC_CH_COSITED
SITINGS = {"centre": (CENTRE, CENTRE), "left": (COSITED, CENTRE), "topleft": (COSITED, COSITED)}      # (horizontal, vertical)
INGEST, EMIT = 0, 1                                       # pc_chroma_plan's `op`

_range = range                                            # the functions below take a parameter of that name


def _prototypes():
    i64, vp, ci, cf, fp = C.c_int64, C.c_void_p, C.c_int, C.c_float, C.POINTER(Frame)
    return {
        "pc_chroma_ingest": (None, [fp] + [ci] * 9 + [cf] * 4 + [ci] * 3 + [vp] + [ci] * 4 + [vp]),
        "pc_chroma_emit_workspace_size": (C.c_size_t, [ci, ci, ci, ci]),
        "pc_chroma_emit": (None, [vp, i64, i64, i64] + [ci] * 15 + [cf] * 5 + [fp, fp, vp, C.c_size_t, vp, vp]),
        "pc_chroma_plan": (None, [ci, ci, ci, fp, vp, i64, i64, i64, ci, fp, C.POINTER(ci)]),
        "pc_chroma_strerror": (C.c_char_p, [ci]),
    }


def lib():
    return _imagelib.load(LIB_PATH, _prototypes)


class ChromaError(_imagelib.ImageLibError):
    _lib, _prefix = staticmethod(lib), "pc_chroma"


def bits_of(fmt):
    return FORMATS[fmt].bits


def chroma_size(h, w, fmt):
    f = FORMATS[fmt]
    return -(-int(h) // f.sy), -(-int(w) // f.sx)


def _check_enums(fmt, matrix=None, range=None, upsample=None, siting=None):
    if fmt not in FORMATS:
        raise ValueError(f"fmt must be one of {sorted(FORMATS)}, got {fmt!r}")
    if matrix is not None and matrix not in MATRICES:
        raise ValueError(f"matrix must be one of {sorted(MATRICES)}, got {matrix!r}")
    if range is not None and range not in RANGES:
        raise ValueError(f"range must be 'limited' or 'full', got {range!r}")
    if upsample is not None and upsample not in UPSAMPLES:
        raise ValueError(f"upsample must be 'nearest' or 'linear', got {upsample!r}")
    if siting is not None and siting not in SITINGS:
        raise ValueError(f"siting must be 'centre', 'left' or 'topleft', got {siting!r}")


def _dtype(fmt):
    import torch
    return torch.uint16 if FORMATS[fmt].bits == 10 else torch.uint8


def _frame_view(planes, fmt, what):
    """Checks a frame (no device call) and returns (planes as batched tensors whose strides fit a pc_ch_frame -- copied only where
    the innermost strides do not --, B, H, W, batched).  The tensors must stay alive while the Frame built from them is in use."""
    import torch
    dtype = _dtype(fmt)
    n = 3 if FORMATS[fmt].layout == PLANAR else 2
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
    Hc, Wc = chroma_size(H, W, fmt)
    want = (Hc, Wc) if n == 3 else (Hc, Wc, 2)
    out = [y]
    for name, t in zip("UV" if n == 3 else ("UV",), planes[1:]):
        if t.dim() != len(want) + batched or tuple(t.shape[-len(want):]) != want or (batched and t.shape[0] != B):
            raise ValueError(f"{what}: {name} must be {list((B,) + want) if batched else list(want)} for a {H}x{W} Y plane of {fmt!r}, "
                             f"got {tuple(t.shape)}")
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


def empty_frame(fmt, B, H, W, device):
    """uninitialised contiguous planes of a batch of B frames"""
    import torch
    _check_enums(fmt)
    dtype = _dtype(fmt)
    Hc, Wc = chroma_size(H, W, fmt)
    y = torch.empty((B, H, W), dtype=dtype, device=device)
    if FORMATS[fmt].layout == PLANAR:
        return (y, torch.empty((B, Hc, Wc), dtype=dtype, device=device), torch.empty((B, Hc, Wc), dtype=dtype, device=device))
    return (y, torch.empty((B, Hc, Wc, 2), dtype=dtype, device=device))


def to_model_input(planes, fmt, matrix="bt709", range="limited", upsample="linear", siting="centre", multiple=64):
    """frame -> (x_padded, geom): float32 RGB [B,3,Hp,Wp] as DESIGN.md section 21 defines it bit for bit (every padded element +0.0,
    written by the same launch), and geom = pixels.padding(H, W, multiple).  siting says where the frame's chroma samples lie:
    "centre" (JPEG, and what frames.to_model_input assumes), "left" (MPEG-2 / H.264 / HEVC streams by default) or "topleft"
    (BT.2020 / UHD material)."""
    import torch
    _check_enums(fmt, matrix, range, upsample, siting)
    ts, B, H, W, _ = _frame_view(planes, fmt, "planes")
    geom = padding(H, W, multiple)
    k = coefficients(matrix)
    f, (hs, vs) = FORMATS[fmt], SITINGS[siting]
    dev = ts[0].device
    src = _frame_struct(ts)
    with torch.cuda.device(dev):
        x = torch.empty((B, 3, geom.Hp, geom.Wp), dtype=torch.float32, device=dev)
        rc = lib().pc_chroma_ingest(C.byref(src), *f, hs, vs, RANGES[range], UPSAMPLES[upsample], k.a, k.b, k.c, k.d, B, H, W,
                                    x.data_ptr(), geom.Hp, geom.Wp, geom.top, geom.left, torch.cuda.current_stream(dev).cuda_stream)
    if rc != PC_OK:
        raise ChromaError(rc, "pc_chroma_ingest")
    return x, geom


class Distortion:
    """The sums of one from_model_output(..., ref=...) call.  sse (int64 [B,3], a device tensor): per frame and plane, in the order
    [Y, Cb, Cr], the exact sum of (code - refcode)^2.  psnr_y / psnr_cb / psnr_cr read it back once and compute in Python doubles with
    peak 2^n - 1 over H W (Y) or Hc Wc (chroma) samples."""

    def __init__(self, sse, H, W, fmt):
        self.sse = sse
        self.H, self.W, self.fmt, self.bits = H, W, fmt, bits_of(fmt)
        self._host = None

    def _read(self):
        if self._host is None:
            self._host = self.sse.cpu().tolist()
        return self._host

    def _psnr(self, p):
        Hc, Wc = chroma_size(self.H, self.W, self.fmt)
        n = self.H * self.W if p == 0 else Hc * Wc
        return [psnr_from_sse(r[p], n, (1 << self.bits) - 1) for r in self._read()]

    def psnr_y(self):
        return self._psnr(0)

    def psnr_cb(self):
        return self._psnr(1)

    def psnr_cr(self):
        return self._psnr(2)


def from_model_output(x_hat, geom, fmt, matrix="bt709", range="limited", siting="centre", ref=None, image=True):
    """x_hat: float32 cuda [B,3,Hp,Wp] (or [3,Hp,Wp]; any batch / channel / row strides, unit stride along W) -> the frame of the
    window geom in `fmt` with its chroma sited as `siting` says (a tuple of contiguous planes; without the batch axis for a 3-D
    x_hat), as DESIGN.md section 21 defines it.  With ref (the original frame in `fmt`) returns (frame, Distortion); with
    image=False (needs ref) no frame is allocated or written and the Distortion alone is returned."""
    import torch
    if not image and ref is None:
        raise ValueError("image=False leaves nothing to compute without ref")
    _check_enums(fmt, matrix, range, siting=siting)
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
    f, (hs, vs) = FORMATS[fmt], SITINGS[siting]
    L = lib()
    with torch.cuda.device(x4.device):
        out = empty_frame(fmt, B, H, W, x4.device) if image else None
        dst = _frame_struct(out) if image else None
        rst = _frame_struct(rts) if rts is not None else None
        ws = sse = None
        nbytes = 0
        if rts is not None:
            nbytes = L.pc_chroma_emit_workspace_size(B, H, W, f.sy)
            ws = torch.empty(nbytes // 8, dtype=torch.int64, device=x4.device)
            sse = torch.empty((B, 3), dtype=torch.int64, device=x4.device)
        rc = L.pc_chroma_emit(x4.data_ptr(), x4.stride(0), x4.stride(1), x4.stride(2), geom.Hp, geom.Wp, geom.top, geom.left, B, H, W,
                              *f, hs, vs, RANGES[range], k.kr, k.kg, k.kb, k.ib, k.ir, C.byref(dst) if dst is not None else None,
                              C.byref(rst) if rst is not None else None, ws.data_ptr() if ws is not None else None, nbytes,
                              sse.data_ptr() if sse is not None else None, torch.cuda.current_stream(x4.device).cuda_stream)
    if rc != PC_OK:
        raise ChromaError(rc, "pc_chroma_emit")
    dist = Distortion(sse, H, W, fmt) if rts is not None else None
    if not image:
        return dist
    if x_hat.dim() == 3:
        out = tuple(t[0] for t in out)
    return (out, dist) if dist is not None else out


def plan(op, planes, fmt, f32, geom, ref=None):
    """pc_chroma_plan for tensors (host only, nothing is launched or copied): True where the ingest (op = INGEST: planes the source,
    f32 the padded destination) or the emit (op = EMIT: planes the destination or None, f32 x_hat) of exactly these tensors takes the
    wide-access path.  planes and ref are tuples of batched tensors whose strides already fit a pc_ch_frame."""
    _check_enums(fmt)
    geom = Geometry(*geom)
    wide = C.c_int(-1)
    fr = _frame_struct(planes) if planes is not None else None
    rf = _frame_struct(ref) if ref is not None else None
    rc = lib().pc_chroma_plan(op, FORMATS[fmt].layout, FORMATS[fmt].bits, C.byref(fr) if fr is not None else None, f32.data_ptr(),
                              f32.stride(0), f32.stride(1), f32.stride(2), geom.left, C.byref(rf) if rf is not None else None,
                              C.byref(wide))
    if rc != PC_OK:
        raise ChromaError(rc, "pc_chroma_plan")
    return bool(wide.value)


# -- PCH1: a frame's format, siting and parameters in front of one PCB1 blob -----------------------------------------------------------

MAGIC = b"PCH1"
VERSION = 1
_HEAD = "<BBBBBBBBBBBII"     # version, layout, shift, sx, sy, horizontal siting, vertical siting, matrix, range, upsample, bits, H, W
HEADER_BYTES = 4 + struct.calcsize(_HEAD)
_MATRIX_ID = {"bt601": 0, "bt709": 1, "bt2020": 2}


def _inv(d):
    return {v: k for k, v in d.items()}


def pack_frame(blob, fmt, matrix, range, upsample, siting, H, W):
    """PCH1: the magic, the version byte, then layout, shift, sx, sy, horizontal siting, vertical siting, matrix, range, upsample and
    bits as one byte each, H and W as little-endian uint32, then the PCB1 blob unmodified."""
    from . import container
    _check_enums(fmt, matrix, range, upsample, siting)
    H, W = int(H), int(W)
    if not (1 <= H < 1 << 32 and 1 <= W < 1 << 32):
        raise container.ContainerError(f"frame size {H}x{W}")
    hd = container.parse_header(blob)
    if tuple(hd["image_size"]) != (H, W):
        raise container.ContainerError(f"the PCB1 blob holds a {hd['image_size'][0]}x{hd['image_size'][1]} image, the frame is {H}x{W}")
    f, (hs, vs) = FORMATS[fmt], SITINGS[siting]
    return MAGIC + struct.pack(_HEAD, VERSION, f.layout, f.shift, f.sx, f.sy, hs, vs, _MATRIX_ID[matrix], RANGES[range],
                               UPSAMPLES[upsample], f.bits, H, W) + bytes(blob)


def parse_frame(buf):
    """-> dict(fmt, siting, matrix, range, upsample, bits, H, W, blob (the PCB1 container), pcb1 (its parsed header)).  ContainerError
    on a bad magic, version, enum, bit depth, size, length or inner header; nothing else is touched."""
    from . import container
    if len(buf) < 4 or bytes(buf[:4]) != MAGIC:
        raise container.ContainerError("not a PCH1 container")
    if len(buf) < HEADER_BYTES:
        raise container.ContainerError("truncated PCH1 header")
    ver, lay, sh, sx, sy, hs, vs, m, r, u, bits, H, W = struct.unpack_from(_HEAD, buf, 4)
    if ver != VERSION:
        raise container.ContainerError(f"unsupported PCH1 version {ver}")
    fi, si, mi, ri, ui = _inv(FORMATS), _inv(SITINGS), _inv(_MATRIX_ID), _inv(RANGES), _inv(UPSAMPLES)
    if bits not in (8, 10):
        raise container.ContainerError(f"corrupt PCH1 header: {bits} bits")
    if (lay, bits, sh, sx, sy) not in fi or (hs, vs) not in si or m not in mi or r not in ri or u not in ui:
        raise container.ContainerError(f"corrupt PCH1 header: layout {lay}, shift {sh} at {bits} bits, subsampling {sx}x{sy}, "
                                       f"siting {hs}, {vs}, matrix {m}, range {r}, upsample {u}")
    if H < 1 or W < 1:
        raise container.ContainerError(f"corrupt PCH1 header: frame size {H}x{W}")
    blob = bytes(buf[HEADER_BYTES:])
    try:
        hd = container.parse_header(blob)
    except container.ContainerError as e:
        raise container.ContainerError(f"PCH1: the PCB1 blob does not parse: {e}") from None
    if tuple(hd["image_size"]) != (H, W):
        raise container.ContainerError(f"PCH1 header says {H}x{W}, its PCB1 blob {hd['image_size'][0]}x{hd['image_size'][1]}")
    return {"fmt": fi[(lay, bits, sh, sx, sy)], "siting": si[(hs, vs)], "matrix": mi[m], "range": ri[r], "upsample": ui[u], "bits": bits,
            "H": H, "W": W, "blob": blob, "pcb1": hd}


def encode_frame(model, planes, qualities, fmt, matrix="bt709", range="limited", upsample="linear", siting="centre",
                 mask_pol="point-based-std"):
    """frame(s) -> PCH1 container(s) holding every level of `qualities`: `bytes` for one frame (Y is [H,W]), a list with one `bytes`
    per frame for a batch.  The PCB1 blob inside is what pixels.encode_image would pack for the same planes and levels, so
    pixels.decode_image of it gives the RGB rendering."""
    from . import container
    qualities = [float(q) for q in qualities]
    x, geom = to_model_input(planes, fmt, matrix, range, upsample, siting)
    datas = model.compress_levels(x, qualities, mask_pol=mask_pol)
    strings = [d["strings"] for d in datas]
    bufs = [pack_frame(container.pack(strings, datas[0]["shape"], qualities, image_size=(geom.H, geom.W), mask_pol=mask_pol, image_index=b),
                       fmt, matrix, range, upsample, siting, geom.H, geom.W) for b in _range(x.shape[0])]
    return bufs[0] if planes[0].dim() == 2 else bufs


def decode_frame(model, buf, level=-1, fmt=None, siting=None):
    """One level (index into the container's quality list, negative from the end) of a PCH1 container -> the frame (a tuple of planes
    without a batch axis) on the model's device, in the stored format and siting or in `fmt` / `siting` when given (the stored matrix
    and range either way; another subsampling, depth or siting is computed from the decoder's float output, not converted from
    codes: a 4:2:2 master decodes straight to left-sited NV12 for a display path).  Only the header, the base segment and that
    level's segment are read; every refusal comes before the model is touched."""
    from . import container
    hd = parse_frame(buf)
    out_fmt = hd["fmt"] if fmt is None else fmt
    out_siting = hd["siting"] if siting is None else siting
    _check_enums(out_fmt, siting=out_siting)
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
    return tuple(t[0] for t in from_model_output(x_hat, geom, out_fmt, hd["matrix"], hd["range"], out_siting))

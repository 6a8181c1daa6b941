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
import ctypes as C
import struct

from . import _imagelib, _tilecodec, _yuvlayers
from .frames import MATRICES, RANGES, UPSAMPLES, Frame, _frame_struct, _x4_of, coefficients, psnr_from_sse  # noqa: F401
from .pixels import Geometry, padding  # noqa: F401

LIB_PATH = _imagelib.lib_path("chroma")

#: every symbol chroma_hip/pc_chroma.h declares
EXPORTS = ["pc_chroma_ingest", "pc_chroma_emit_workspace_size", "pc_chroma_emit", "pc_chroma_plan", "pc_chroma_strerror",
           "pc_chroma_last_hip_error"]

Format, PLANAR, SEMIPLANAR = _yuvlayers.Format, _yuvlayers.PLANAR, _yuvlayers.SEMIPLANAR       # PC_CH_PLANAR, PC_CH_SEMIPLANAR
FORMATS = {
    "i420": Format(PLANAR, 8, 0, 2, 2), "i422": Format(PLANAR, 8, 0, 2, 1), "i444": Format(PLANAR, 8, 0, 1, 1),
    "nv12": Format(SEMIPLANAR, 8, 0, 2, 2), "nv16": Format(SEMIPLANAR, 8, 0, 2, 1), "nv24": Format(SEMIPLANAR, 8, 0, 1, 1),
    "p010": Format(SEMIPLANAR, 10, 6, 2, 2), "p210": Format(SEMIPLANAR, 10, 6, 2, 1), "p410": Format(SEMIPLANAR, 10, 6, 1, 1),
    "i010": Format(PLANAR, 10, 0, 2, 2), "i210": Format(PLANAR, 10, 0, 2, 1), "i410": Format(PLANAR, 10, 0, 1, 1),
}
CENTRE, COSITED = 0, 1                                    # PC_CH_CENTRE, PC_CH_COSITED
SITINGS = {"centre": (CENTRE, CENTRE), "left": (COSITED, CENTRE), "topleft": (COSITED, COSITED)}      # (horizontal, vertical)
INGEST, EMIT = 0, 1                                       # pc_chroma_plan's `op`


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


def _frame_view(planes, fmt, what):
    """Checks a frame (no device call) and returns (planes as batched tensors whose strides fit a pc_ch_frame -- copied only where
    the innermost strides do not --, B, H, W, batched).  The tensors must stay alive while the Frame built from them is in use."""
    return _yuvlayers.frame_view(FAMILY, planes, fmt, what)


def empty_frame(fmt, B, H, W, device):
    """uninitialised contiguous planes of a batch of B frames"""
    _check_enums(fmt)
    return _yuvlayers.empty_frame(FAMILY, fmt, B, H, W, device)


def to_model_input(planes, fmt, matrix="bt709", range="limited", upsample="linear", siting="centre", multiple=64):
    """frame -> (x_padded, geom): float32 RGB [B,3,Hp,Wp] as DESIGN.md section 21 defines it bit for bit (every padded element +0.0,
    written by the same launch), and geom = pixels.padding(H, W, multiple).  siting says where the frame's chroma samples lie:
    "centre" (JPEG, and what frames.to_model_input assumes), "left" (MPEG-2 / H.264 / HEVC streams by default) or "topleft"
    (BT.2020 / UHD material)."""
    return _yuvlayers.to_model_input(FAMILY, planes, fmt, matrix, range, upsample, siting, multiple)


class Distortion(_yuvlayers.Distortion):
    __doc__ = _yuvlayers.Distortion.__doc__

    def __init__(self, sse, H, W, fmt):
        super().__init__(sse, H, W, bits_of(fmt))
        self.fmt, self._sub = fmt, (FORMATS[fmt].sx, FORMATS[fmt].sy)


def from_model_output(x_hat, geom, fmt, matrix="bt709", range="limited", siting="centre", ref=None, image=True):
    """x_hat: float32 cuda [B,3,Hp,Wp] (or [3,Hp,Wp]; any batch / channel / row strides, unit stride along W) -> the frame of the
    window geom in `fmt` with its chroma sited as `siting` says (a tuple of contiguous planes; without the batch axis for a 3-D
    x_hat), as DESIGN.md section 21 defines it.  With ref (the original frame in `fmt`) returns (frame, Distortion); with
    image=False (needs ref) no frame is allocated or written and the Distortion alone is returned."""
    return _yuvlayers.from_model_output(FAMILY, x_hat, geom, fmt, matrix, range, siting, ref, image)


def plan(op, planes, fmt, f32, geom, ref=None):
    """pc_chroma_plan for tensors (host only, nothing is launched or copied): True where the ingest (op = INGEST: planes the source,
    f32 the padded destination) or the emit (op = EMIT: planes the destination or None, f32 x_hat) of exactly these tensors takes the
    wide-access path.  planes and ref are tuples of batched tensors whose strides already fit a pc_ch_frame."""
    return _yuvlayers.plan(FAMILY, op, planes, fmt, f32, geom, ref)


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
    return _yuvlayers.pack_frame(FAMILY, blob, fmt, matrix, range, upsample, siting, H, W)


def parse_frame(buf):
    """-> dict(fmt, siting, matrix, range, upsample, bits, H, W, blob (the PCB1 container), pcb1 (its parsed header)).  ContainerError
    on a bad magic, version, enum, bit depth, size, length or inner header; nothing else is touched."""
    return _yuvlayers.parse_frame(FAMILY, buf)


def encode_frame(model, planes, qualities, fmt, matrix="bt709", range="limited", upsample="linear", siting="centre",
                 mask_pol="point-based-std"):
    """frame(s) -> PCH1 container(s) holding every level of `qualities`: `bytes` for one frame (Y is [H,W]), a list with one `bytes`
    per frame for a batch.  The PCB1 blob inside is what pixels.encode_image would pack for the same planes and levels, so
    pixels.decode_image of it gives the RGB rendering."""
    return _yuvlayers.encode_frame(FAMILY, model, planes, qualities, fmt, matrix, range, upsample, siting, mask_pol)


def decode_frame(model, buf, level=-1, fmt=None, siting=None):
    """One level (index into the container's quality list, negative from the end) of a PCH1 container -> the frame (a tuple of planes
    without a batch axis) on the model's device, in the stored format and siting or in `fmt` / `siting` when given (the stored matrix
    and range either way; another subsampling, depth or siting is computed from the decoder's float output, not converted from
    codes: a 4:2:2 master decodes straight to left-sited NV12 for a display path).  Only the header, the base segment and that
    level's segment are read; every refusal comes before the model is touched."""
    return _yuvlayers.decode_frame(FAMILY, model, buf, level, fmt, siting)


# -- what _yuvlayers needs to know about the stack of twelve formats and three sitings (chroma, chroma_tiles, chroma_rate) ---------------

def _halo(window, fmt, siting):
    """chroma_tiles.halo_window"""
    y0, x0, h, w = window
    f, (hs, vs) = FORMATS[fmt], SITINGS[siting]
    dx = 1 if f.sx == 2 and hs and x0 > 0 else 0
    dy = 1 if f.sy == 2 and vs and y0 > 0 else 0
    return (y0 - dy, x0 - dx, h + dy, w + dx)


FAMILY = _yuvlayers.Family(
    owners=(("chroma", "ChromaError"), ("chroma_tiles", "ChromaTilesError"), ("chroma_rate", "ChromaRateError")),
    formats=FORMATS,
    check=_check_enums,
    c_format={(f, s): (*v, *hv) for f, v in FORMATS.items() for s, hv in SITINGS.items()},
    c_plan={(f, layer): (v.layout, v.bits, v.sx)[:3 if layer else 2] for f, v in FORMATS.items() for layer in (0, 1, 2)},
    c_sy={f: (v.sy,) for f, v in FORMATS.items()},
    halo=_halo,
    head_of=_tilecodec.sited_head,
    params_of=lambda fields, name: (_tilecodec.sited_params(*fields[:10], name), fields[10:]),
    plane_of=" of {fmt!r}",
    inadmissible="window {win} of the {H}x{W} {fmt!r} frame is not admissible: y0 must be a multiple of {sy} and x0 of {sx}, h a multiple "
                 "of {sy} or y0 + h == H, w a multiple of {sx} or x0 + w == W",
    distortion=Distortion)

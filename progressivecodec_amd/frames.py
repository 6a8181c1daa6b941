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
import ctypes as C
import struct

from . import _imagelib, _tilecodec, _yuvlayers
# what both stacks use as it is lives beside their shared bodies; its names stay reachable here
from ._yuvlayers import (MATRICES, RANGES, UPSAMPLES, Coefficients, Frame, _f32, _frame_struct, _x4_of, coefficients,  # noqa: F401
                         psnr_from_sse)
from .pixels import Geometry, padding  # noqa: F401

LIB_PATH = _imagelib.lib_path("frames")

#: every symbol frames_csrc/pc_frames.h declares
EXPORTS = ["pc_frames_ingest", "pc_frames_emit_workspace_size", "pc_frames_emit", "pc_frames_plan", "pc_frames_strerror",
           "pc_frames_last_hip_error"]

FORMATS = {"nv12": 0, "i420": 1, "p010": 2}               # PC_FRAMES_NV12, PC_FRAMES_I420, PC_FRAMES_P010
INGEST, EMIT = 0, 1                                       # pc_frames_plan's `op`


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
    return _yuvlayers.frame_view(FAMILY, planes, fmt, what)


def empty_frame(fmt, B, H, W, device):
    """uninitialised contiguous planes of a batch of B frames"""
    _check_enums(fmt)
    return _yuvlayers.empty_frame(FAMILY, fmt, B, H, W, device)


def to_model_input(planes, fmt, matrix="bt709", range="limited", upsample="linear", multiple=64):
    """frame -> (x_padded, geom): float32 RGB [B,3,Hp,Wp] as DESIGN.md section 13 defines it bit for bit (every padded element +0.0,
    written by the same launch), and geom = pixels.padding(H, W, multiple)."""
    return _yuvlayers.to_model_input(FAMILY, planes, fmt, matrix, range, upsample, None, multiple)


Distortion = _yuvlayers.Distortion


def from_model_output(x_hat, geom, fmt, matrix="bt709", range="limited", ref=None, image=True):
    """x_hat: float32 cuda [B,3,Hp,Wp] (or [3,Hp,Wp]; any batch / channel / row strides, unit stride along W) -> the frame of the
    window geom in `fmt` (a tuple of contiguous planes; without the batch axis for a 3-D x_hat), as DESIGN.md section 13 defines it.
    With ref (the original frame in `fmt`) returns (frame, Distortion); with image=False (needs ref) no frame is allocated or written
    and the Distortion alone is returned."""
    return _yuvlayers.from_model_output(FAMILY, x_hat, geom, fmt, matrix, range, None, ref, image)


def plan(op, planes, fmt, f32, geom, ref=None):
    """pc_frames_plan for tensors (host only, nothing is launched or copied): True where the ingest (op = INGEST: planes the source,
    f32 the padded destination) or the emit (op = EMIT: planes the destination or None, f32 x_hat) of exactly these tensors takes the
    wide-access path.  planes and ref are tuples of batched tensors whose strides already fit a pc_frame."""
    return _yuvlayers.plan(FAMILY, op, planes, fmt, f32, geom, ref)


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
    return _yuvlayers.pack_frame(FAMILY, blob, fmt, matrix, range, upsample, None, H, W)


def parse_frame(buf):
    """-> dict(fmt, matrix, range, upsample, bits, H, W, blob (the PCB1 container), pcb1 (its parsed header)).  ContainerError on a bad
    magic, version, enum, bit depth, size or length; nothing else is touched."""
    return _yuvlayers.parse_frame(FAMILY, buf)


def encode_frame(model, planes, qualities, fmt, matrix="bt709", range="limited", upsample="linear", mask_pol="point-based-std"):
    """frame(s) -> PCF1 container(s) holding every level of `qualities`: `bytes` for one frame (Y is [H,W]), a list with one `bytes`
    per frame for a batch.  The PCB1 blob inside is what pixels.encode_image would pack for the same planes and levels, so
    pixels.decode_image of it gives the RGB rendering."""
    return _yuvlayers.encode_frame(FAMILY, model, planes, qualities, fmt, matrix, range, upsample, None, mask_pol)


def decode_frame(model, buf, level=-1, fmt=None):
    """One level (index into the container's quality list, negative from the end) of a PCF1 container -> the frame (a tuple of planes
    without a batch axis) on the model's device, in the stored format or in `fmt` when given (the stored matrix and range either way;
    another bit depth is computed from the decoder's float output, not converted from codes).  Only the header, the base segment and
    that level's segment are read; every refusal comes before the model is touched."""
    return _yuvlayers.decode_frame(FAMILY, model, buf, level, fmt, None)


# -- what _yuvlayers needs to know about the 4:2:0 stack (frames, frame_tiles, frame_rate) ------------------------------------------------

_F = _yuvlayers.Format
_TABLE = {"nv12": _F(_yuvlayers.SEMIPLANAR, 8, 0, 2, 2), "i420": _F(_yuvlayers.PLANAR, 8, 0, 2, 2), "p010": _F(_yuvlayers.SEMIPLANAR, 10, 6, 2, 2)}

FAMILY = _yuvlayers.Family(
    owners=(("frames", "FramesError"), ("frame_tiles", "FrameTilesError"), ("frame_rate", "FrameRateError")),
    formats=_TABLE,
    check=_check_enums,
    c_format={(f, None): (v,) for f, v in FORMATS.items()},
    c_plan={(f, layer): (v,) for f, v in FORMATS.items() for layer in (0, 1, 2)},
    c_sy=dict.fromkeys(FORMATS, ()),
    halo=None,
    head_of=lambda fmt, matrix, range, upsample, siting: (FORMATS[fmt], _MATRIX_ID[matrix], RANGES[range], UPSAMPLES[upsample], bits_of(fmt)),
    params_of=lambda fields, name: (_tilecodec.frame_params(*fields[:5], name), fields[5:]),
    plane_of="",
    inadmissible="window {win} of the {H}x{W} frame is not admissible: y0 and x0 must be even, h even or y0 + h == H, w even or x0 + w == W",
    distortion=lambda sse, H, W, fmt: Distortion(sse, H, W, bits_of(fmt)))

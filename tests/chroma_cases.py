"""The raw-call cases of tests/test_gpu_chroma.py's matrices as data, and the ledger of kernel instantiations they reach.  Not a test
file and not a conftest: numpy and the restatements (tests/*_contract.py) only.  tests/test_chroma_host.py holds the table to the
loops it replaced and to the 24 + 64 instantiations chroma_hip/pc_chroma.hip states; tests/test_gpu_chroma.py runs every case and
asserts that pc_chroma_plan reports the path the table predicts, so that the ledger is true of the library.

Two rules of the library are restated here, from pc_chroma.h's text:
  the access path   wide exactly where the float pointer is 16-byte aligned and its strides are multiples of 4, left is a multiple of
                    8 (ingest, with Wp a multiple of 8) or of 4 (emit), and every plane of every frame starts on four elements with
                    strides that are multiples of 4;
  the tuple         (element width, interleaved, SX, SY, WIDE) names the ingest kernel, (element width, interleaved, SX, SY, VCO, WIDE,
                    HAS_REF) the emit kernel; VCO: SY = 2 and siting "topleft".
"""
import collections
import itertools

import numpy as np

from tests import chroma_contract as CC
from tests import pixels_contract as K

SIZES = [(1, 1), (2, 3), (3, 2), (37, 53), (64, 64), (67, 130)]
OTHER_FORMATS = ["nv16", "p210", "i444"]
OTHER_SETTINGS = [("bt601", "full"), ("bt2020", "limited"), ("bt2020", "full"), ("bt709", "full"), ("bt601", "limited")]
OTHER_SIZES = [(37, 53), (3, 2)]
#: the narrow decode into pitched planes, image only
DECODE_SIZES = [(37, 53), (3, 2)]
DECODE_SITINGS = ["centre", "topleft"]
#: whole pictures: (format, siting) at 1026 x 1030
WHOLE = dict(H=1026, W=1030, B=2)
WHOLE_FORMATS = [("i420", "left"), ("nv12", "topleft"), ("p010", "topleft"), ("nv16", "left"), ("i210", "topleft")]
#: the 10-bit words Python does not name: (the named format of the same layout, the other shift)
UNNAMED = [(fmt, 6 - CC.FORMATS[fmt][2]) for fmt in ("p010", "p210", "p410", "i010", "i210", "i410")]

#: one raw-call case at batch 2.  n: the seed and, in the loops this table replaced, the position; offset, mode: the frame's Views
#: (tests/test_gpu_frames.View); variant: the float planes (float_planes); dst_offset: floats the ingest's destination lies past an
#: aligned address; ups: the upsamplers the ingest runs under (none: no ingest); emits: (with image, with reference) per emit call
Case = collections.namedtuple("Case", "fmt matrix rng siting H W n left offset mode variant dst_offset ups emits")


def up4(v):
    return -(-v // 4) * 4


def view_strides(rows, rowlen, mode):
    """(batch stride, row stride) in elements of a plane of `rows` rows of `rowlen` elements: tests/test_gpu_frames.View's"""
    sr = {"tight": rowlen, "pad4": up4(rowlen), "loose": rowlen + 3 + (1 if (rowlen + 3) % 4 == 0 else 0)}[mode]
    return {"tight": rows * sr, "pad4": up4(rows * sr) + 4, "loose": rows * sr + 1}[mode], sr


def plane_rows(fmt, H, W):
    """[(rows, elements per row)] of the planes of a frame"""
    Hc, Wc = CC.chroma_size(H, W, fmt)
    return [(H, W), (Hc, 2 * Wc)] if CC.FORMATS[fmt][0] else [(H, W), (Hc, Wc), (Hc, Wc)]


def frame_wide(fmt, H, W, offset, mode):
    return offset % 4 == 0 and all(s % 4 == 0 for rows, n in plane_rows(fmt, H, W) for s in view_strides(rows, n, mode))


def float_strides(Hp, Wp, variant):
    """(offset in floats past an aligned address, (batch, channel, row) strides): tests/test_gpu_frames.float_planes'"""
    if variant == "contiguous":
        return 0, (3 * Hp * Wp, Hp * Wp, Wp)
    sh, off = (Wp + 4, 0) if variant == "loose4" else (Wp + 1, 1)
    sc = Hp * sh + (8 if variant == "loose4" else 3)
    return off, (3 * sc + (4 if variant == "loose4" else 2), sc, sh)


def f32_wide(offset, strides):
    return offset % 4 == 0 and all(s % 4 == 0 for s in strides)


def ingest_wide(c):
    Hp, Wp = K.geometry(c.H, c.W)[:2]
    return f32_wide(c.dst_offset, (3 * Hp * Wp, Hp * Wp, Wp)) and Wp % 8 == 0 and c.left % 8 == 0 and frame_wide(c.fmt, c.H, c.W, c.offset, c.mode)


def emit_wide(c, dst=None, ref=None):
    """dst, ref: (offset, mode) of those frames where they differ from the case's"""
    Hp, Wp = K.geometry(c.H, c.W)[:2]
    frames = [f if f is not None else (c.offset, c.mode) for f in (dst, ref)]
    return f32_wide(*float_strides(Hp, Wp, c.variant)) and c.left % 4 == 0 and all(frame_wide(c.fmt, c.H, c.W, *f) for f in frames)


def ingest_tuple(fmt, wide):
    semi, n, _, sx, sy = CC.FORMATS[fmt]
    return (2 if n == 10 else 1, semi, sx, sy, bool(wide))


def emit_tuple(fmt, siting, wide, has_ref):
    semi, n, _, sx, sy = CC.FORMATS[fmt]
    return (2 if n == 10 else 1, semi, sx, sy, sy == 2 and CC.SITINGS[siting][1], bool(wide), bool(has_ref))


SUBSAMPLINGS = [(2, 2), (2, 1), (1, 1)]
ALL_INGEST = {(es, il, sx, sy, w) for es in (1, 2) for il in (False, True) for sx, sy in SUBSAMPLINGS for w in (False, True)}
ALL_EMIT = {(es, il, sx, sy, vco, w, r) for es in (1, 2) for il in (False, True) for sx, sy in SUBSAMPLINGS
            for vco in ((False, True) if sy == 2 else (False,)) for w in (False, True) for r in (False, True)}


def layout_of(n, H, W):
    """(left, offset, mode, variant, dst_offset) of position n: even positions loose, offset planes under the geometry's own left
    and floats one past an allocation start (narrow), odd ones aligned planes with left rounded down to a multiple of 8 (wide)"""
    left = K.geometry(H, W)[3]
    if n % 2 == 0:
        return left, 1 + n % 3, "loose", "odd", 1
    return left // 8 * 8, 0, "pad4", ("contiguous", "loose4")[n % 4 // 2], 0


def matrix_cases(fmt, matrix, rng, sizes):
    """every siting x size: the ingest under both upsamplers and the emit with image and sums; at 37 x 53 also the sums alone and the
    image alone"""
    out = []
    for n, (siting, (H, W)) in enumerate(itertools.product(CC.SITINGS, sizes)):
        emits = ((True, True), (False, True), (True, False)) if (H, W) == (37, 53) else ((True, True),)
        out.append(Case(fmt, matrix, rng, siting, H, W, n, *layout_of(n, H, W), tuple(CC.UPSAMPLES), emits))
    return out


def decode_cases(fmt, matrix, rng):
    """what a decoder does: the image alone into pitched, unaligned planes (narrow), under centre and top-left siting"""
    out = []
    for k, (siting, (H, W)) in enumerate(itertools.product(DECODE_SITINGS, DECODE_SIZES)):
        n = 100 + 2 * k
        out.append(Case(fmt, matrix, rng, siting, H, W, n, *layout_of(n, H, W), (), ((True, False),)))
    return out


def every_format_cases(fmt):
    return matrix_cases(fmt, "bt709", "limited", SIZES) + decode_cases(fmt, "bt709", "limited")


def other_matrix_cases(fmt):
    return [c for matrix, rng in OTHER_SETTINGS for c in matrix_cases(fmt, matrix, rng, OTHER_SIZES)]


def table():
    """every case of the two matrix tests"""
    return [c for fmt in sorted(CC.FORMATS) for c in every_format_cases(fmt)] + [c for fmt in OTHER_FORMATS for c in other_matrix_cases(fmt)]


def reached(cases):
    """(ingest tuples, emit tuples) the cases launch"""
    ingest = {ingest_tuple(c.fmt, ingest_wide(c)) for c in cases if c.ups}
    emit = {emit_tuple(c.fmt, c.siting, emit_wide(c), ref) for c in cases for _, ref in c.emits}
    return ingest, emit


# -- the unnamed 10-bit words --------------------------------------------------------------------------------------------------------

def reshifted(frame, fmt, shift, noise=None):
    """the frame's codes in words of another shift; noise (uint16, cycled): what the bits outside the code hold, else 0"""
    old = CC.FORMATS[fmt][2]
    out = []
    for p in frame:
        w = ((p >> np.uint16(old)) & np.uint16(1023)) << np.uint16(shift)
        if noise is not None:
            w = w | (np.resize(noise, p.shape) & ~np.uint16(1023 << shift))
        out.append(np.ascontiguousarray(w.astype(np.uint16)))
    return tuple(out)


# -- whole pictures ------------------------------------------------------------------------------------------------------------------

COLOURS = [(1.0, 1.0, 1.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)]             # white, blue, red: the top code in Y, in Cb, in Cr


def whole_saturated(fmt, hp, wp):
    """(x [3,3,hp,wp], a frame of zeros, [top^2 * samples of plane p]): picture p saturates plane p in full range; one picture cannot
    saturate two planes (Cb' = 1/2 needs R = G = 0, Cr' = 1/2 needs G = B = 0)"""
    H, W = WHOLE["H"], WHOLE["W"]
    Hc, Wc = CC.chroma_size(H, W, fmt)
    x = np.zeros((3, 3, hp, wp), np.float32)
    for b, rgb in enumerate(COLOURS):
        for ch in range(3):
            x[b, ch] = rgb[ch]
    top = 2 ** CC.bits(fmt) - 1
    zeros = CC.frame(np.zeros((3, H, W), np.int64), np.zeros((3, Hc, Wc), np.int64), np.zeros((3, Hc, Wc), np.int64), fmt)
    return x, zeros, [top * top * H * W, top * top * Hc * Wc, top * top * Hc * Wc]


def whole_tail(fmt, siting, matrix, rng, hp, wp, top, left):
    """(x [2,3,hp,wp], ref): ref is the emit of in-gamut noise; x is that noise with the last luma row of the last picture sent to
    the far end of [0, 1]"""
    H, W, B = WHOLE["H"], WHOLE["W"], WHOLE["B"]
    x = np.random.default_rng(5).uniform(0.2, 0.8, (B, 3, hp, wp)).astype(np.float32)
    ref = CC.emit(x, top, left, H, W, fmt, matrix, rng, siting)
    row = x[B - 1, :, top + H - 1, :]
    x[B - 1, :, top + H - 1, :] = np.where(row > 0.5, np.float32(0), np.float32(1))
    return x, ref

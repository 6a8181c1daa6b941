"""The raw-call cases of tests/test_gpu_chroma_tiles.py's matrix as data, and the ledger of kernel instantiations they reach.  Not a
test file and not a conftest: numpy and the restatements (tests/*_contract.py) only.  tests/test_chroma_tiles_host.py holds the table
to the 24 + 64 instantiations chroma_tiles_hip/pc_chroma_tiles.hip states; tests/test_gpu_chroma_tiles.py runs every case and asserts
that pc_chroma_tiles_plan reports the path the table predicts, so that the ledger is true of the library.

Two rules of the library are restated here, from pc_chroma_tiles.h's text:
  the access path   wide exactly where the float pointer is 16-byte aligned and its strides are multiples of 4, every plane's row
                    stride is a multiple of 4 and the first element an item touches in every plane lies on four elements; for the
                    cut that also needs O a multiple of 8 at sx == 2 (any O at 4:4:4);
  the tuple         (element width, interleaved, SX, SY, WIDE) names the cut kernel, (element width, interleaved, SX, SY, VCO, WIDE,
                    HAS_REF) the stitch kernel; VCO: SY = 2 and siting "topleft".
"""
import collections
import itertools

from tests import chroma_contract as CC

T = 64
MAIN = dict(H=100, W=150, overlaps=(0, 4), matrix="bt709", rng="limited")
OTHER_FORMATS = ["nv16", "p210", "i444", "nv12"]
OTHER_SIZES = [(1, 1), (2, 3), (3, 2), (37, 53), (65, 63), (127, 129)]
OTHER_OVERLAPS = [16, 32]
OTHER_SETTINGS = [("bt601", "full"), ("bt2020", "limited"), ("bt2020", "full"), ("bt709", "full"), ("bt601", "limited")]
#: (with image, with reference) of the stitch calls of a case
ALL_EMITS = ((True, True), (False, True), (True, False))

#: one case: one frame, cut under `ups` and stitched (the whole frame) once per entry of emits.  aligned: the planes are pad4 Views
#: with each plane's first item element on an aligned address, the tile tensor keeps every 16-byte alignment (`variant`) and the
#: cut's destination is aligned; else the planes are loose, the tile tensor lies one float past an allocation start and the cut's
#: destination `dst_offset` floats past an aligned address
Case = collections.namedtuple("Case", "fmt matrix rng siting H W O n aligned variant dst_offset ups emits")


def layout_of(n, aligned):
    return (True, ("contiguous", "loose4")[n % 2], 0) if aligned else (False, "odd", 1 + n % 3)


def cut_wide(c):
    return c.aligned and (CC.sub(c.fmt)[0] == 1 or c.O % 8 == 0)


def stitch_wide(c):
    return c.aligned


def cut_tuple(fmt, wide):
    semi, n, _, sx, sy = CC.FORMATS[fmt]
    return (2 if n == 10 else 1, semi, sx, sy, bool(wide))


def stitch_tuple(fmt, siting, wide, has_ref):
    semi, n, _, sx, sy = CC.FORMATS[fmt]
    return (2 if n == 10 else 1, semi, sx, sy, sy == 2 and CC.SITINGS[siting][1], bool(wide), bool(has_ref))


SUBSAMPLINGS = [(2, 2), (2, 1), (1, 1)]
ALL_CUT = {(es, il, sx, sy, w) for es in (1, 2) for il in (False, True) for sx, sy in SUBSAMPLINGS for w in (False, True)}
ALL_STITCH = {(es, il, sx, sy, vco, w, r) for es in (1, 2) for il in (False, True) for sx, sy in SUBSAMPLINGS
              for vco in ((False, True) if sy == 2 else (False,)) for w in (False, True) for r in (False, True)}


def main_cases(fmt):
    """every siting x overlap at 100 x 150 under both upsamplers, with image, with the sums, and with the sums alone.  The views
    alternate between the two paths so that every siting meets both and O = 0 (the cut's wide path at sx == 2) meets an aligned one"""
    out = []
    for n, ((si, siting), (oi, O)) in enumerate(itertools.product(enumerate(CC.SITINGS), enumerate(MAIN["overlaps"]))):
        out.append(Case(fmt, MAIN["matrix"], MAIN["rng"], siting, MAIN["H"], MAIN["W"], O, n, *layout_of(n, (si + oi) % 2 == 1),
                        tuple(CC.UPSAMPLES), ALL_EMITS))
    return out


def other_cases(fmt):
    """the small, odd and multi-tile sizes with the larger overlaps, the other matrices and full range"""
    out = []
    k = OTHER_FORMATS.index(fmt)
    for n, (H, W) in enumerate(OTHER_SIZES):
        matrix, rng = OTHER_SETTINGS[(n + k) % len(OTHER_SETTINGS)]
        siting = list(CC.SITINGS)[(n + k) % 3]
        out.append(Case(fmt, matrix, rng, siting, H, W, OTHER_OVERLAPS[(n + k) % 2], 100 + n, *layout_of(n, (n + k) % 2 == 0),
                        (CC.UPSAMPLES[n % 2],), ((True, True),)))
    return out


def table():
    return [c for fmt in sorted(CC.FORMATS) for c in main_cases(fmt)] + [c for fmt in OTHER_FORMATS for c in other_cases(fmt)]


def reached(cases):
    """(cut tuples, stitch tuples) the cases launch"""
    cut = {cut_tuple(c.fmt, cut_wide(c)) for c in cases if c.ups}
    stitch = {stitch_tuple(c.fmt, c.siting, stitch_wide(c), ref) for c in cases for _, ref in c.emits}
    return cut, stitch


def names(tuples):
    return sorted("u%d %s %d:%d%s %s%s" % (8 * t[0], "semi" if t[1] else "planar", t[2], t[3], " vco" if len(t) == 7 and t[4] else "",
                                           "wide" if t[-2 if len(t) == 7 else -1] else "narrow", (" ref" if t[-1] else " image") if len(t) == 7 else "")
                  for t in tuples)

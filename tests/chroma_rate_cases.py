"""The raw-call cases of tests/test_gpu_chroma_rate.py's matrix as data, and the ledger of kernel instantiations they reach.  Not a test
file and not a conftest: numpy and the restatements (tests/*_contract.py) only.  tests/test_chroma_rate_host.py holds the table to the
32 instantiations chroma_rate_hip/pc_chroma_rate.hip states; tests/test_gpu_chroma_rate.py runs every case and asserts that
pc_chroma_rate_plan reports the path the table predicts, so that the ledger is true of the library.

Two rules of the library are restated here, from pc_chroma_rate.h's text:
  the access path   wide exactly where the float pointer is 16-byte aligned and its strides are multiples of 4, every plane of the
                    reference lies on four elements with a row stride that is a multiple of 4, and O is a multiple of 8 at sx == 2
                    (any O at 4:4:4);
  the tuple         (element width, interleaved, SX, SY, VCO, WIDE) names the kernel; VCO: SY = 2 and siting "topleft".
"""
import collections
import itertools

from tests import chroma_contract as CC

T = 64
MAIN = dict(H=100, W=150, overlaps=(0, 4), matrix="bt709", rng="limited")
OTHER_FORMATS = ["nv16", "p210", "i444", "nv12"]
OTHER_SIZES = [(1, 1), (2, 3), (3, 2), (65, 63), (127, 129)]
OTHER_OVERLAPS = [16, 32]
OTHER_SETTINGS = [("bt601", "full"), ("bt2020", "limited"), ("bt2020", "full"), ("bt709", "full"), ("bt601", "limited")]

#: one case: one frame against hostile tiles of its whole grid.  aligned: the reference planes are pad4 Views at an allocation start
#: and the tile tensor keeps every 16-byte alignment (`variant`); else the planes are loose and one element in, and the tile tensor
#: lies one float past an allocation start
Case = collections.namedtuple("Case", "fmt matrix rng siting H W O n aligned variant")


def layout_of(n, aligned):
    return (True, ("contiguous", "loose4")[n % 2]) if aligned else (False, "odd")


def wide(c):
    return c.aligned and (CC.sub(c.fmt)[0] == 1 or c.O % 8 == 0)


def kernel_tuple(fmt, siting, is_wide):
    semi, n, _, sx, sy = CC.FORMATS[fmt]
    return (2 if n == 10 else 1, semi, sx, sy, sy == 2 and CC.SITINGS[siting][1], bool(is_wide))


SUBSAMPLINGS = [(2, 2), (2, 1), (1, 1)]
ALL = {(es, il, sx, sy, vco, w) for es in (1, 2) for il in (False, True) for sx, sy in SUBSAMPLINGS
       for vco in ((False, True) if sy == 2 else (False,)) for w in (False, True)}


def main_cases(fmt):
    """every siting x overlap at 100 x 150 (2 x 3 ragged tiles).  The views alternate so that "centre" and "topleft" meet the wide path
    at O = 0, every siting meets the narrow one, and an aligned O = 4 (wide at 4:4:4 alone) is there"""
    out = []
    for n, ((si, siting), (oi, O)) in enumerate(itertools.product(enumerate(CC.SITINGS), enumerate(MAIN["overlaps"]))):
        out.append(Case(fmt, MAIN["matrix"], MAIN["rng"], siting, MAIN["H"], MAIN["W"], O, n, *layout_of(n, (si + oi) % 2 == 0)))
    return out


def other_cases(fmt):
    """the small, odd and multi-tile sizes with the larger overlaps, the other matrices and full range"""
    out = []
    k = OTHER_FORMATS.index(fmt)
    for n, (H, W) in enumerate(OTHER_SIZES):
        matrix, rng = OTHER_SETTINGS[(n + k) % len(OTHER_SETTINGS)]
        siting = list(CC.SITINGS)[(n + k) % 3]
        out.append(Case(fmt, matrix, rng, siting, H, W, OTHER_OVERLAPS[(n + k) % 2], 100 + n, *layout_of(n, (n + k) % 2 == 0)))
    return out


def table():
    return [c for fmt in sorted(CC.FORMATS) for c in main_cases(fmt)] + [c for fmt in OTHER_FORMATS for c in other_cases(fmt)]


def reached(cases):
    """the tuples the cases launch"""
    return {kernel_tuple(c.fmt, c.siting, wide(c)) for c in cases}


def names(tuples):
    return sorted("u%d %s %d:%d%s %s" % (8 * t[0], "semi" if t[1] else "planar", t[2], t[3], " vco" if t[4] else "", "wide" if t[5] else "narrow")
                  for t in tuples)

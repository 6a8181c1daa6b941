"""The raw-call cases of tests/test_gpu_chroma_clips.py's matrix as data, and the ledger of kernel instantiations they reach.  Not a test
file and not a conftest: the restatements (tests/*_contract.py) only.  tests/test_chroma_clips_host.py holds the table to the 24 + 24
instantiations chroma_clips_kernels/pc_chroma_clips.hip states; tests/test_gpu_chroma_clips.py runs every case on both kinds of views
and asserts that pc_chroma_clips_plan reports the path the table predicts, so that the ledger is true of the library.

Two rules of the library are restated here, from pc_chroma_clips.h's text:
  the access path   wide exactly where every plane pointer (of both frames for the changes) lies on four elements, every row stride
                    is a multiple of 4, O is a multiple of 8 at sx == 2 (any O at 4:4:4) and, for the cut, the float pointer is
                    16-byte aligned;
  the tuple         (element width, interleaved, SX, SY, WIDE) names the changes kernel, and the cut kernel likewise.
"""
import collections
import itertools

from tests import chroma_contract as CC

T = 64
MAIN = dict(H=100, W=150, overlaps=(0, 4))
OTHER_FORMATS = ["nv16", "p210", "i444", "nv12"]
OTHER_SIZES = [(1, 1), (2, 3), (3, 2), (37, 53), (65, 63), (127, 129)]
OTHER_OVERLAPS = [16, 32]
SETTINGS = [("bt709", "limited"), ("bt601", "full"), ("bt2020", "limited"), ("bt2020", "full"), ("bt709", "full"), ("bt601", "limited")]
#: the views every case is run on: the planes of both frames aligned with row strides that are multiples of 4 (the cut's floats
#: 16-byte aligned), and every plane one element past such an address with loose row strides (the floats one float past)
ALIGNMENTS = (True, False)

#: one case: a pair of frames (and the cut of lists of tiles of the first) in one format, siting, upsampling and geometry; n numbers
#: it and seeds its data; matrix and rng are the cut's
Case = collections.namedtuple("Case", "fmt siting upsample H W O n matrix rng")


def wide(c, aligned):
    """the access path of the changes and of the cut of case c on aligned / unaligned views"""
    return aligned and (CC.sub(c.fmt)[0] == 1 or c.O % 8 == 0)


def kernel_tuple(fmt, w):
    semi, n, _, sx, sy = CC.FORMATS[fmt]
    return (2 if n == 10 else 1, semi, sx, sy, bool(w))


SUBSAMPLINGS = [(2, 2), (2, 1), (1, 1)]
ALL_KERNELS = {(es, il, sx, sy, w) for es in (1, 2) for il in (False, True) for sx, sy in SUBSAMPLINGS for w in (False, True)}


def main_cases(fmt):
    """every siting x upsampling x overlap at 100 x 150; O = 4 is narrow at sx == 2 whatever the views"""
    out = []
    for n, (siting, up, O) in enumerate(itertools.product(CC.SITINGS, CC.UPSAMPLES, MAIN["overlaps"])):
        out.append(Case(fmt, siting, up, MAIN["H"], MAIN["W"], O, n, *SETTINGS[n % len(SETTINGS)]))
    return out


def other_cases(fmt):
    """the small, odd and multi-tile sizes with the larger overlaps"""
    out = []
    k = OTHER_FORMATS.index(fmt)
    for n, (H, W) in enumerate(OTHER_SIZES):
        out.append(Case(fmt, list(CC.SITINGS)[(n + k) % 3], CC.UPSAMPLES[(n + k // 2) % 2], H, W, OTHER_OVERLAPS[(n + k) % 2], 100 + n,
                        *SETTINGS[(n + k) % len(SETTINGS)]))
    return out


def table():
    return [c for fmt in sorted(CC.FORMATS) for c in main_cases(fmt)] + [c for fmt in OTHER_FORMATS for c in other_cases(fmt)]


def reached(cases):
    """the kernel tuples the cases launch: the changes' and the cut's are the same set, every case runs both on both kinds of views"""
    return {kernel_tuple(c.fmt, wide(c, a)) for c in cases for a in ALIGNMENTS}


def names(tuples):
    return sorted("u%d %s %d:%d %s" % (8 * t[0], "semi" if t[1] else "planar", t[2], t[3], "wide" if t[4] else "narrow") for t in tuples)

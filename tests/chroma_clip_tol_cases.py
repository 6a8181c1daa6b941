"""The raw-call cases of tests/test_gpu_chroma_clip_tol.py's matrix as data, and the ledger of diff_kernel instantiations they reach.
Not a test file and not a conftest.  The case table is section 25's (tests/chroma_clips_cases.py): all twelve formats x three sitings
x two upsamplings at 100 x 150 with O in {0, 4}, and nv16 / p210 / i444 / nv12 at the small, odd and multi-tile sizes with O in
{16, 32}.  tests/test_chroma_clip_tol_host.py holds the table to the 24 instantiations chroma_clip_tol_gpu/pc_chroma_clip_tol.hip
states; tests/test_gpu_chroma_clip_tol.py runs every case on every frame table below and asserts that pc_chroma_clip_tol_plan reports
the path the table predicts, so that the ledger is true of the library.

The access path, restated from pc_chroma_clip_tol.h's text: wide exactly where EVERY frame of the table has every plane pointer on
four elements and every row stride a multiple of 4, and O is a multiple of 8 at sx == 2 (any O at 4:4:4).
"""
from tests import chroma_contract as CC
from tests.chroma_clips_cases import (ALL_KERNELS, OTHER_FORMATS, OTHER_SIZES, T, Case, kernel_tuple, main_cases, names,  # noqa: F401
                                      other_cases, table)

F = 5
#: how the frames of one table lie in memory, frame k taking entry k % 2 (tests.test_gpu_chroma_clips.views' modes): aligned with row
#: strides that are multiples of 4, but different ones; pitched with a stride that is none, next to an aligned one; one element past
#: an allocation start, next to a contiguous one.  By construction only the first table is aligned in every frame, and two
#: neighbours in a table never share a pitch.
TABLES = [(("pad4", 0), ("wider", 0)), (("loose", 0), ("pad4", 0)), (("pad4", 1), ("tight", 0))]
ALIGNED = (True, False, False)


def wide(c, p):
    """the access path of the scan of case c on frame table p"""
    return ALIGNED[p] and (CC.sub(c.fmt)[0] == 1 or c.O % 8 == 0)


def reached(cases):
    """the diff_kernel tuples (element width, interleaved, SX, SY, WIDE) the cases launch: every case runs on every table"""
    return {kernel_tuple(c.fmt, wide(c, p)) for c in cases for p in range(len(TABLES))}

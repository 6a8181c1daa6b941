"""The raw-call cases of tests/test_gpu_chroma_clip_rate.py's matrix as data, and the ledger of kernel instantiations they reach.  Not a
test file and not a conftest: numpy and the restatements (tests/*_contract.py) only.  tests/test_chroma_clip_rate_host.py holds the table
to the 32 instantiations chroma_clip_rate_kernels/pc_chroma_clip_rate.hip states; tests/test_gpu_chroma_clip_rate.py runs every case and
asserts that pc_chroma_clip_rate_plan reports the path the table predicts, so that the ledger is true of the library.

The cases are tests/chroma_rate_cases.py's (the same formats, sitings, sizes, overlaps, matrices and ranges), each over a clip of
three frames and a scattered job list.  Two rules of the library are restated here, from pc_chroma_clip_rate.h's text:
  the access path   wide exactly where the float pointer is 16-byte aligned and its strides are multiples of 4, EVERY frame of the
                    table has every plane on four elements with a row stride that is a multiple of 4, and O is a multiple of 8 at
                    sx == 2 (any O at 4:4:4): one narrow frame makes the whole call narrow;
  the tuple         (element width, interleaved, SX, SY, VCO, WIDE) names the kernel; VCO: SY = 2 and siting "topleft".
"""
import numpy as np

from tests import chroma_contract as CC
from tests.chroma_rate_cases import ALL, OTHER_FORMATS, OTHER_SIZES, Case, T, kernel_tuple, main_cases, names, other_cases, table  # noqa: F401

F = 3
#: the three frames of a table as (View mode, offset in elements): all aligned with row strides that are multiples of 4, but not the
#: same ones; or pitched differently with ONE of them one element past an allocation start among aligned ones
ALIGNED = [("pad4", 0), ("wider", 0), ("pad4", 0)]
MIXED = [("pad4", 0), ("loose", 1), ("wider", 0)]


def frame_modes(c):
    return ALIGNED if c.aligned else MIXED


def frames_wide(modes):
    """every frame of the table has to allow the wide path"""
    return all(mode in ("pad4", "wider") and offset % 4 == 0 for mode, offset in modes)


def wide(c):
    floats = c.variant != "odd"
    return floats and frames_wide(frame_modes(c)) and (CC.sub(c.fmt)[0] == 1 or c.O % 8 == 0)


def reached(cases):
    """the tuples the cases launch"""
    return {kernel_tuple(c.fmt, c.siting, wide(c)) for c in cases}


def job_list(n, seed):
    """jobs over three frames: every tile of frame 2 in descending order, then frames 0 and 1 out of order with a job repeated"""
    g = np.random.default_rng(seed)
    jobs = [(2, t) for t in reversed(range(n))] + [(0, 0), (1, n - 1), (0, 0), (1, int(g.integers(0, n))), (0, int(g.integers(0, n)))]
    assert jobs[n] == jobs[n + 2] and {t for f, t in jobs if f == 2} == set(range(n)) and {f for f, _ in jobs} == set(range(F))
    return jobs

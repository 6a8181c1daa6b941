"""The raw-call cases of tests/test_gpu_chroma_clip_tol_rate.py's matrix as data, their inputs and expected rows, and the ledger of
kernel instantiations they reach.  Not a test file and not a conftest: numpy and the restatements (tests/*_contract.py) only.
tests/test_chroma_clip_tol_rate_host.py holds the table to the 32 instantiations
chroma_clip_tol_rate_gpu/pc_chroma_clip_tol_rate.hip states (16 item shapes on two access paths) and asserts, on the CPU, that the
inputs can tell a kernel that ignores `slots` from one that does not; tests/test_gpu_chroma_clip_tol_rate.py runs every case and
asserts that pc_chroma_clip_tol_rate_plan reports the path the table predicts, so that the ledger is true of the library.

The cases are section 28's (tests/chroma_clip_rate_cases.py: the same formats, sitings, overlaps, matrices, ranges, frame tables and
access rule) at 100 x 150, the four other formats at 65 x 63 and 127 x 129 with O = 16 and 32 and at 100 x 150 with O = 24 and 28,
each over a clip of three frames that differ and a list of runs.  The expected rows of a case are computed once (want) and shared.
"""
import functools

import numpy as np

from tests import chroma_clip_tol_rate_contract as TR
from tests import chroma_contract as CC
from tests import hostile_values as HV
from tests import tiles_contract as TC
from tests.chroma_clip_rate_cases import ALIGNED, MIXED, F, frame_modes, frames_wide, reached, wide  # noqa: F401
from tests.chroma_rate_cases import ALL, OTHER_FORMATS, OTHER_SETTINGS, Case, T, kernel_tuple, layout_of, main_cases, names  # noqa: F401

OTHER_SIZES = [(65, 63), (127, 129)]
OTHER_OVERLAPS = [16, 32]
BAND = dict(H=100, W=150, overlaps=(24, 28))                               # 2 O is no power of two (tests/band_cases.py)


def other_cases(fmt):
    """the odd and multi-tile sizes with the larger overlaps, the other matrices and full range"""
    out = []
    k = OTHER_FORMATS.index(fmt)
    for n, ((H, W), O) in enumerate((hw, O) for hw in OTHER_SIZES for O in OTHER_OVERLAPS):
        matrix, rng = OTHER_SETTINGS[(n + k) % len(OTHER_SETTINGS)]
        out.append(Case(fmt, matrix, rng, list(CC.SITINGS)[(n + k) % 3], H, W, O, 100 + n, *layout_of(n, (n + k) % 2 == 0)))
    return out


def band_cases(fmt):
    """O = 24 (wide where the rest allows it) and O = 28 (narrow at sx == 2), each on an aligned and on a mixed table"""
    out = []
    k = OTHER_FORMATS.index(fmt)
    for n, (O, aligned) in enumerate((O, a) for O in BAND["overlaps"] for a in (True, False)):
        matrix, rng = OTHER_SETTINGS[(n + k + 2) % len(OTHER_SETTINGS)]
        out.append(Case(fmt, matrix, rng, list(CC.SITINGS)[(n + k + 1) % 3], BAND["H"], BAND["W"], O, 200 + n, *layout_of(n, aligned)))
    return out


def table():
    return ([c for fmt in sorted(CC.FORMATS) for c in main_cases(fmt)] + [c for fmt in OTHER_FORMATS for c in other_cases(fmt)]
            + [c for fmt in OTHER_FORMATS for c in band_cases(fmt)])


def hostile(n, seed, size=T):
    """tiles_contract.hostile_tiles with hostile_values.SPECIALS (NaN, +-inf, the largest finites, a denormal, -0.0) planted on top"""
    x = TC.hostile_tiles(n, size, seed)
    flat = x.reshape(-1)
    flat[5::211] = np.resize(HV.SPECIALS, flat[5::211].shape)
    return x


def run_list(n, seed):
    """jobs over three frames: runs of length 1, 2 and 3 in mixed order -- scattered, reversed, over all frames, a frame repeated
    inside a run -- every tile of the grid in descending order, and a tile repeated across jobs with different runs"""
    g = np.random.default_rng(seed)
    patterns = [[2], [0, 1], [1, 2, 0], [1, 1], [2, 0, 2], [0], [2, 1, 0], [0, 2]]
    tile_ids = list(reversed(range(n))) + [0, n - 1, 0, int(g.integers(0, n)), int(g.integers(0, n))]
    runs = [patterns[(m + seed) % len(patterns)] for m in range(len(tile_ids))]
    runs[n], runs[n + 2] = [1, 2, 0], [2, 2]                                          # tile 0 twice, with different runs
    runs[n + 1], runs[n + 3] = [0, 1, 2], [1]
    assert {len(r) for r in runs} == {1, 2, 3} and tile_ids[n] == tile_ids[n + 2] and [0, 1, 2] in runs
    return tile_ids, runs


@functools.lru_cache(maxsize=None)
def inputs(c):
    """-> (the three frames, which differ in every sample's chance; the hostile tiles [n_jobs,3,T,T]; tile_ids; runs)"""
    ny, nx = TC.grid(c.H, c.W, T, c.O)
    tile_ids, runs = run_list(ny * nx, c.H + c.W + c.O + c.n)
    fr = [CC.random_frame(1, c.H, c.W, c.fmt, seed=1000 * c.H + c.W + c.n + 7 * s, garbage=True) for s in range(F)]
    return fr, hostile(len(tile_ids), seed=77 * c.H + c.W + c.n), tile_ids, runs


@functools.lru_cache(maxsize=None)
def want(c):
    """the restatement's rows of case c, computed once"""
    fr, x_np, tile_ids, runs = inputs(c)
    return TR.run_sse(x_np, fr, tile_ids, runs, c.H, c.W, T, c.O, c.fmt, c.matrix, c.rng, c.siting)


def slots_matter(runs, rows):
    """within every run, two entries of different frames have rows that differ in every plane (entries of the same frame are the same
    job): a kernel that ignored `slots`, or read another entry's, could not give these rows.  -> the number of pairs looked at"""
    off = TR.offsets_of(runs)
    pairs = 0
    for m, run in enumerate(runs):
        for a in range(len(run)):
            for b in range(a + 1, len(run)):
                ra, rb = rows[off[m] + a], rows[off[m] + b]
                if run[a] == run[b]:
                    assert ra == rb, (m, run)
                else:
                    assert all(ra[p] != rb[p] for p in range(3)), (m, run, ra, rb)
                    pairs += 1
    return pairs


# -- the codec tests' clips -------------------------------------------------------------------------------------------------------------

H0, W0 = 100, 150                                                          # 2 x 3 tiles of 64 x 64, with and without overlap
N = 6
CODEC_F = 5
CODEC = [("p210", "left"), ("nv12", "topleft"), ("i444", "centre")]


@functools.lru_cache(maxsize=None)
def noisy_clip(fmt, siting):
    """five frames: a smooth frame (its codes lie well inside the code range) with seeded noise of 0 / +1 on every sample of every
    frame, so that static tiles differ from frame to frame by at most one code, and a block that moves through the upper row of tiles"""
    from tests.test_gpu_chroma_tiles import codec_frame
    g = np.random.default_rng(20)
    base = [np.array(c) for c in CC.codes(codec_frame(H0, W0, fmt, siting), fmt)]
    s = 1 << (CC.bits(fmt) - 8)
    sx, sy = CC.sub(fmt)[:2]
    out = []
    for k in range(CODEC_F):
        y, cb, cr = [c + g.integers(0, 2, c.shape) for c in base]
        y[0, 10:30, 10 + 25 * k:30 + 25 * k] = 200 * s
        cb[0, 10 // sy:30 // sy, (10 + 25 * k) // sx:(30 + 25 * k) // sx] = 90 * s
        out.append(CC.frame(y, cb, cr, fmt))
    return out

"""The image-side libraries past T = 128: the case table and the builders of tests/test_image_limits_host.py (no GPU) and
tests/test_gpu_image_limits.py (GPU).  Not a test file and not a conftest: numpy and the restatements (tests/*_contract.py) only.

Four groups of cases (DESIGN.md section 19.1 lists the limit each executes):
  A  the largest tile a library admits per format, every weight meeting the largest error: sums of 58 bits;
  B  T = 576 and T = 1024 on hostile data: 81 (82) and 256 (257) block partials per tile, so that the final reductions, which walk
     a row of partials with a lane stride of 64, make a second and a fourth trip; and tail-only data, whose only non-zero partial
     is the last of the row (and, for the clip libraries, the halo block after it);
  C  whole pictures of 1026 x 1030: more than 256 block partials per picture, sums past 2^32;
  D  the cuts at T = 576 and T = 2048;
  E  clip_tol_rate (section 20), whose partials are per WAVE and per entry: A and B again -- 4096 wave partials per entry at
     T = 2048 (64 trips of its final), 1024 at T = 1024 in P010 (16 trips) -- and runs longer than a wave has lanes.
Expected values are the restatements'; for saturated inputs also the closed forms below in Python ints, and the host test holds
the two to each other.
"""
import functools

import numpy as np

from tests import clip_tol_contract as TOL
from tests import clips_contract as CC
from tests import frame_rate_contract as QC
from tests import frames_contract as FC
from tests import pixels_contract as K
from tests import tiles_contract as TC

# -- the table -----------------------------------------------------------------------------------------------------------------------

#: A, the sum kernels: every sample of tile 4 of the 3 x 3 grid lies in a band on both axes (S = O = T / 2)
RATE_LIMIT = dict(T=2048, O=1024, H=4096, W=4096, tile=4)
#: A, a tile the image clips on both axes, H and W no multiples of 8: 2 x 3 tiles, tile 5 holds 1979 x 1453 pixels
RATE_CLIPPED = dict(T=2048, O=1024, H=3003, W=3501, tile=5)
FRAME_LIMITS = {"nv12": dict(T=2048, O=1024, H=4096, W=4096, tile=4), "i420": dict(T=2048, O=1024, H=4096, W=4096, tile=4),
                "p010": dict(T=1024, O=512, H=2048, W=2048, tile=4)}
#: A, the clip libraries: tile 4 of the 3 x 3 grid has a complete halo ring, 2 * 1026 + 2 * 1024 chroma samples
CLIP_LIMIT = dict(T=2048, O=0, H=4098, W=4098, tile=4)
CLIP_FORMATS = ("nv12", "p010")
#: the jobs of the clip_rate limit case over its two frames: a repeat, both frames, one corner tile
LIMIT_JOBS = [(1, 4), (0, 4), (1, 4), (0, 0)]

#: B: the smallest T whose row of partials needs a second trip, on a frame with odd sizes and clipped edge tiles; (O, wide path?)
SECOND_TRIP = dict(T=576, H=601, W=1101)
SECOND_TRIP_OVERLAPS = [(0, True), (64, True), (4, False)]
FOUR_TRIPS = dict(T=1024, O=0, H=1030, W=1500)                             # 2 x 2 tiles, tile 0 whole, tile 3 clipped to 6 x 476

#: C
WHOLE = dict(H=1026, W=1030, B=2, T=576, O=64)

#: D
CUT_SMALL = dict(T=576, H=601, W=1101)
CUT_LARGE = dict(T=2048, O=0, H=4098, W=4098, rect=(1, 1, 1, 1))

#: the largest T each library's header promises, per element width
T_MAX = {"rate": {8: 2048}, "frame_rate": {8: 2048, 10: 1024}, "clip_rate": {8: 2048, 10: 1024}, "clips": {8: 2048, 10: 2048},
         "clip_tol": {8: 2048, 10: 2048}, "clip_tol_rate": {8: 2048, 10: 1024}}


# -- closed forms, Python ints -------------------------------------------------------------------------------------------------------

def axis_weight_sum(i, n, T, O, length=None):
    """the sum over u < length (default T) of the band numerator of tile i of n: O^2 over a band (1 + 3 + ... + 2 O - 1), den
    elsewhere.  length < T: only for a tile whose upper band the picture cuts away entirely or not at all."""
    L = T if length is None else length
    den = 2 * O if O else 1
    lo = O * O if i > 0 else den * O
    if i < n - 1:
        assert L == T
        return lo + den * (T - 2 * O) + O * O
    return lo + den * (L - O)


def rate_closed(c, e):
    """the weighted sum of e^2 over c's tile, which the image does not clip"""
    ny, nx = TC.grid(c["H"], c["W"], c["T"], c["O"])
    i, j = divmod(c["tile"], nx)
    return e * e * axis_weight_sum(i, ny, c["T"], c["O"]) * axis_weight_sum(j, nx, c["T"], c["O"])


def frame_rate_closed(c, eY, eC):
    """[Y, Cb, Cr]: a chroma weight is the mean of its two luma numerators, so a chroma axis sums to half the luma axis"""
    ny, nx = TC.grid(c["H"], c["W"], c["T"], c["O"])
    i, j = divmod(c["tile"], nx)
    wy, wx = axis_weight_sum(i, ny, c["T"], c["O"]), axis_weight_sum(j, nx, c["T"], c["O"])
    assert wy % 2 == 0 and wx % 2 == 0
    return [eY * eY * wy * wx, eC * eC * (wy // 2) * (wx // 2), eC * eC * (wy // 2) * (wx // 2)]


def top_code(fmt):
    return (1 << FC.bits(fmt)) - 1


def footprint_sizes(c, upsample):
    """[Y, Cb, Cr] samples of the footprint of c's tile, which has all four neighbours and a whole halo ring under linear upsampling"""
    h = CC.halo_of(upsample)
    return [c["T"] ** 2] + [(c["T"] // 2 + 2 * h) ** 2] * 2


# -- A -------------------------------------------------------------------------------------------------------------------------------

def const_tile(T, v, n=1):
    return np.full((n, 3, T, T), v, np.float32)


def rate_saturated(mirror):
    """(x [1,3,T,T], ref chw, the error): zero tiles against 255, or (mirror) ones against 0"""
    c = RATE_LIMIT
    return const_tile(c["T"], 1.0 if mirror else 0.0), np.full((3, c["H"], c["W"]), 0 if mirror else 255, np.uint8), 255


def const_frame(fmt, H, W, y, cb, cr):
    Hc, Wc = FC.chroma_size(H, W)
    return FC.frame(np.full((1, H, W), y, np.int64), np.full((1, Hc, Wc), cb, np.int64), np.full((1, Hc, Wc), cr, np.int64), fmt)


def frame_saturated(fmt, mirror):
    """(x value, frame, eY, eC) in full range: zero tiles (codes 0, co, co) against Y at the top code and chroma 0; or (mirror) ones
    (codes top, co, co) against Y = 0 and chroma at the top code"""
    c = FRAME_LIMITS[fmt]
    _, _, co, _, mx = FC.levels(fmt, "full")
    if mirror:
        return 1.0, const_frame(fmt, c["H"], c["W"], 0, mx, mx), mx, mx - co
    return 0.0, const_frame(fmt, c["H"], c["W"], mx, 0, 0), mx, co


@functools.lru_cache(maxsize=None)
def rate_clipped_case():
    """(x [1,3,T,T] hostile, ref chw random) for RATE_CLIPPED's tile"""
    c = RATE_CLIPPED
    x = TC.hostile_tiles(1, c["T"], seed=5)
    ref = np.random.default_rng(6).integers(0, 256, (3, c["H"], c["W"]), dtype=np.uint8)
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref


def clip_limit_frames(fmt):
    """(all codes 0, all codes at the top, the latter with random low bits where the format has them): frames 0 and 1 differ in every
    sample by the largest difference, frames 1 and 2 in no code"""
    c = CLIP_LIMIT
    top = top_code(fmt)
    f0, f1 = const_frame(fmt, c["H"], c["W"], 0, 0, 0), const_frame(fmt, c["H"], c["W"], top, top, top)
    if fmt == "p010":
        g = np.random.default_rng(10)
        f2 = tuple(p | g.integers(0, 64, p.shape, dtype=np.uint16) for p in f1)
    else:
        f2 = tuple(np.array(p) for p in f1)
    return f0, f1, f2


def boundary_tolerances(fmt):
    """[(max_abs, mse_q10, max_run, every tile reused?)]: the exact boundary, and one less on either number"""
    top = top_code(fmt)
    q = 1024 * top * top
    assert q < TOL.NO_MSE
    return [((top,) * 3, (q,) * 3, 0, True), ((top,) * 3, (q - 1,) * 3, 0, False), ((top - 1,) * 3, (q,) * 3, 0, False)]


# -- B -------------------------------------------------------------------------------------------------------------------------------

def byte_image(H, W, seed):
    """uint8 [3,H,W] as tests/test_gpu_rate.py's: random, every byte value present"""
    a = np.random.default_rng(1000 * H + W + seed).integers(0, 256, (3, H, W), dtype=np.uint8)
    a.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
    return a


def flip(x):
    """a float tile part -> values whose codes all differ from x's: the far end of [0, 1]"""
    return np.where(K.clamp01(x) > np.float32(0.5), np.float32(0.0), np.float32(1.0)).astype(np.float32)


def rate_tail(T, H, W, seed=0):
    """(x_tail, x_equal [1,3,T,T], ref chw): tile 0 (O = 0), which lies inside the image; x_equal is the image's own tile, every error
    zero; x_tail differs from it in the tile's last two rows alone"""
    assert T <= H and T <= W
    ref = byte_image(H, W, seed)
    eq = TC.cut(ref, "chw", T, 0, rect=(0, 0, 1, 1))
    tail = np.array(eq)
    tail[:, :, T - 2:, :] = flip(eq[:, :, T - 2:, :])
    return tail, eq, ref


def frame_tail(fmt, T, H, W, matrix="bt709", rng="limited", seed=0):
    """(x_tail, x_equal [1,3,T,T], frame): tile 0 (O = 0) inside the frame; the frame holds under tile 0 the tile's own codes, every
    error zero; x_tail differs from x_equal in the last two rows alone (one luma row pair, one chroma row)"""
    assert T <= H and T <= W and T % 2 == 0
    eq = TC.hostile_tiles(1, T, seed=seed + 1)
    Y, Cb, Cr = (np.array(c) for c in FC.codes(FC.random_frame(1, H, W, fmt, seed), fmt))
    tY, tCb, tCr = QC.tile_codes(eq[0], T, T, fmt, matrix, rng)
    Y[0, :T, :T], Cb[0, :T // 2, :T // 2], Cr[0, :T // 2, :T // 2] = tY, tCb, tCr
    tail = np.array(eq)
    tail[:, :, T - 2:, :] = flip(eq[:, :, T - 2:, :])
    return tail, eq, FC.frame(Y, Cb, Cr, fmt)


def clip_tail(fmt, T, H, W, halo=True, seed=0):
    """(cur, prev): prev random; cur differs from it in tile 0's last luma row pair and last chroma row (O = 0, the tile inside the
    frame) and, with `halo`, in one Cb sample of the chroma row below the tile: tile 0's halo ring under linear upsampling"""
    assert T < H and T <= W and T % 2 == 0
    prev = FC.random_frame(1, H, W, fmt, seed)
    top = 1 << FC.bits(fmt)
    Y, Cb, Cr = (np.array(c) for c in FC.codes(prev, fmt))
    Y[0, T - 2:T, :T] = (Y[0, T - 2:T, :T] + 1) % top
    Cb[0, T // 2 - 1, :T // 2] = (Cb[0, T // 2 - 1, :T // 2] + top - 1) % top
    Cr[0, T // 2 - 1, :T // 2] = (Cr[0, T // 2 - 1, :T // 2] + top // 2) % top
    if halo:
        Cb[0, T // 2, 100] = (Cb[0, T // 2, 100] + 3) % top
    return FC.frame(Y, Cb, Cr, fmt), prev


def quick_frame(fmt, H, W, seed):
    """a frame of seeded random codes over the whole code range (without random_frame's permutation: for the largest frames)"""
    g = np.random.default_rng(seed)
    Hc, Wc = FC.chroma_size(H, W)
    return FC.frame(*[g.integers(0, 1 << FC.bits(fmt), s, dtype=np.int64) for s in ((1, H, W), (1, Hc, Wc), (1, Hc, Wc))], fmt)


def job_list(n):
    """jobs over two frames, out of order: both frames, a repeat, the whole first tile and the clipped last one"""
    return [(1, n - 1), (0, 0), (1, 1), (0, 0), (0, n - 1)]


def sub_range(n):
    return (1, n - 1) if n > 2 else (n - 1, 1)


# -- C -------------------------------------------------------------------------------------------------------------------------------

def whole_saturated_sum(peak):
    return peak * peak * WHOLE["H"] * WHOLE["W"]


def rows_kept(T, O, H):
    """per tile row of the grid, the local rows of the picture's last two rows (for the tail-only stitches)"""
    ny = TC.axis_tiles(H, T, O)
    S = T - O
    return {i: [r - i * S for r in (H - 2, H - 1) if i * S <= r < i * S + T] for i in range(ny)}


def stitch_tail(x_equal, T, O, H, W):
    """tiles [n,3,T,T] of the whole grid -> the same tiles with the picture's last two rows flipped in every tile that holds them"""
    ny, nx = TC.grid(H, W, T, O)
    out = np.array(x_equal)
    for i, rows in rows_kept(T, O, H).items():
        for r in rows:
            for j in range(nx):
                out[i * nx + j, :, r, :] = flip(x_equal[i * nx + j, :, r, :])
    return out


# -- E: clip_tol_rate ------------------------------------------------------------------------------------------------------------------

#: A: (tile value, tile, run) per job over the table (frame_saturated(fmt, False), frame_saturated(fmt, True), the first again)
RUN_LIMIT_JOBS = [(0.0, 4, [0, 1, 0]), (1.0, 4, [1, 0]), (0.0, 0, [0])]
RUN_LIMIT_MIRRORS = (False, True, False)
#: C: T = 64 on a 100 x 150 picture, three frames; the run lengths of the six jobs, 300 entries in all
LONG_RUNS = dict(T=64, H=100, W=150, O=16, lengths=(70, 1, 2, 33, 64, 130), tiles=(5, 0, 3, 5, 1, 2))


def saturated_errors(fmt, v, mirror):
    """(eY, eC) of a constant tile of value v (codes 0 or top, co, co in full range) against frame_saturated(fmt, mirror)'s frame"""
    _, _, co, _, mx = FC.levels(fmt, "full")
    ty = mx if v else 0
    fy, fc = (0, mx) if mirror else (mx, 0)
    return abs(ty - fy), abs(co - fc)


def run_limit_case(fmt):
    """(frames, tile values, tile_ids, runs, the closed-form rows) of A"""
    c = FRAME_LIMITS[fmt]
    frames = [frame_saturated(fmt, mirror)[1] for mirror in RUN_LIMIT_MIRRORS]
    vals, tile_ids, runs = ([j[k] for j in RUN_LIMIT_JOBS] for k in range(3))
    want = [frame_rate_closed(dict(c, tile=t), *saturated_errors(fmt, v, RUN_LIMIT_MIRRORS[f])) for v, t, run in RUN_LIMIT_JOBS for f in run]
    return frames, vals, tile_ids, runs, want


def run_list(n):
    """runs over two frames in job_list's style: both frames, a repeat inside a run, out of order, the whole first tile twice with
    different runs and the clipped last one"""
    return [n - 1, 0, 1, 0], [[1, 0], [0, 1, 0], [1], [1, 1]]


def run_trip_cases():
    """(T, H, W, O, wide, format): the three overlaps of the second trip in all three formats, the four trips in P010"""
    s, f = SECOND_TRIP, FOUR_TRIPS
    out = [(s["T"], s["H"], s["W"], O, wide, fmt) for O, wide in SECOND_TRIP_OVERLAPS for fmt in FC.FORMATS]
    return out + [(f["T"], f["H"], f["W"], f["O"], True, "p010")]


def long_runs():
    """(tile_ids, runs): six jobs, slots cycling through the three frames with a repeat every fourth entry, each job starting at
    another slot; one run longer than a wave has lanes, one of exactly 64, and 300 entries in all"""
    c = LONG_RUNS
    runs = [[(j - j // 4 + m) % 3 for j in range(n)] for m, n in enumerate(c["lengths"])]
    return list(c["tiles"]), runs


def run_workspace_cases():
    """(T, n_entries) of every clip_tol_rate case of this table"""
    out = [(FRAME_LIMITS[fmt]["T"], sum(len(j[2]) for j in RUN_LIMIT_JOBS)) for fmt in FRAME_LIMITS]
    out += [(c[0], sum(len(r) for r in run_list(4)[1])) for c in run_trip_cases()]
    out += [(SECOND_TRIP["T"], 4), (LONG_RUNS["T"], sum(LONG_RUNS["lengths"]))]
    return out

"""Band weights that are not dyadic: the case table and the builders of tests/test_band_weights_host.py (no GPU) and
tests/test_gpu_band_weights.py (GPU).  Not a test file and not a conftest: numpy and the restatements (tests/*_contract.py) only.

Section 11 of DESIGN.md blends overlapping tiles with the weights (2u+1)/(2 O) and (2(O-1-u)+1)/(2 O): the correctly rounded float32
quotient, one rounded float32 product wy * wx, an fmaf chain.  At O in {4, 16, 32, 64, 512, 1024} every quotient and product is exact
and nothing of that can be seen.  The overlaps of this table are those at which a weight is NOT a float.

A one-ulp error of a weight moves m = w * v by about one ulp, and an 8-bit code only where m * 255 lies within that ulp of a rounding
boundary.  So the data are WITNESS tile sets: gray values chosen, by search on the restatement's own arithmetic, so that the code
they give under the weight as defined differs from the code under a mutant (the weight one ulp up, one ulp down; for a band corner
the product left unrounded, or a rounded multiply and a rounded add in place of the fmaf).  tests/test_band_weights_host.py runs
the mutants through the three restatements on these sets and counts what they see; the search below only proposes.
"""
import contextlib
import functools
import math

import numpy as np

from tests import chroma_tiles_contract as KC
from tests import frame_tiles_contract as GC
from tests import frames_contract as FC
from tests import pixels_contract as K
from tests import tiles_contract as TC

F = np.float32

# -- the table -----------------------------------------------------------------------------------------------------------------------

#: (T, O).  T = 64: S = 52, 44, 36 are no multiples of 8 (the cut and the rate kernels go narrow at sx = 2), S = 40 is (den = 48);
#: T = 128: den = 80 and 96; T = 192: O = T / 2, every interior pixel lies in a band on both axes, den = 192
OVERLAPS = [(64, 12), (64, 20), (64, 24), (64, 28), (128, 40), (128, 48), (192, 96)]
#: the overlaps at which every inexact band coordinate must have a witness for either direction; at O = 96 the list is recorded
COMPLETE = [(T, O) for T, O in OVERLAPS if O <= 48]
#: what every GPU test of the image-side libraries used before: den a power of two, every weight a float
DYADIC = [(64, 4), (64, 16), (64, 32), (128, 64), (1024, 512), (2048, 1024)]

MATRIX, RANGE = "bt709", "full"
#: (library, its parameter, the quantiser the witness sets are searched for): tiles in both roundings; the luma plane of frame_tiles
#: in 8 and 10 bits; chroma_tiles at 4:2:2 left-sited and at 4:4:4 (the same luma rule, other kernels)
LIBRARIES = [("tiles", "nearest", "nearest"), ("tiles", "trunc", "trunc"), ("frame_tiles", "nv12", "y8"), ("frame_tiles", "p010", "y10"),
             ("chroma_tiles", "nv16", "y8"), ("chroma_tiles", "i444", "y8")]
SITING = {"nv16": "left", "i444": "centre"}

#: neighbouring floats of a tie value that are tried, in ulps
DELTAS = np.arange(-8, 9)
#: witnesses kept per band coordinate and direction, and tile sets per band at the most
PER_DIRECTION, MAX_ROUNDS = 64, 2


def numerators(O):
    """the numerator 2u + 1 of the later tile's weight at band coordinate u; the earlier tile's is that of O - 1 - u"""
    return [2 * u + 1 for u in range(O)]


def inexact(num, O):
    """num / (2 O) is no float32: the reduced denominator is no power of two"""
    den = 2 * O // np.gcd(num, 2 * O)
    return den & (den - 1) != 0


def inexact_coordinates(O):
    return [u for u in range(O) if inexact(2 * u + 1, O)]


# -- the quantisers: m (float32, gray) -> code ---------------------------------------------------------------------------------------

def luma_codes(m, fmt):
    """section 13's luma code of gray pixels R = G = B = m, by the restatement itself"""
    m = np.asarray(m, F).reshape(-1)
    x = np.repeat(m[None, None, None, :], 3, axis=1)
    return FC.emit_codes(x, 0, 0, 1, m.size, fmt, MATRIX, RANGE)[0][0, 0]


#: name -> (scale, the boundary between codes k and k + 1 in scaled units is k + edge, the number of boundaries, m -> codes)
QUANTISERS = {
    "nearest": (255, 0.5, 255, lambda m: K.quantise(np.asarray(m, F), "nearest").astype(np.int64)),
    "trunc": (255, 1.0, 255, lambda m: K.quantise(np.asarray(m, F), "trunc").astype(np.int64)),
    "y8": (255, 0.5, 255, lambda m: luma_codes(m, "nv12")),
    "y10": (1023, 0.5, 1023, lambda m: luma_codes(m, "p010")),
}


def ulps(v, d):
    """positive float32 v moved by d ulps"""
    return (np.asarray(v, F).view(np.int32) + np.asarray(d, np.int32)).view(F)


def candidates(wt, q, acc=0.0, ks=None):
    """float32 [..., k, d]: for every boundary k of the quantiser the value v with wt * v + acc on it, and its neighbouring floats;
    NaN where v is not inside (0, 1]"""
    scale, edge, n, _ = QUANTISERS[q]
    ks = np.arange(n) if ks is None else ks
    target = ((ks + edge) / scale - np.asarray(acc, np.float64)[..., None]) / np.asarray(wt, np.float64)[..., None]
    ok = (target > 2.0 ** -20) & (target < 1.5)
    v0 = np.where(ok, target, 0.5).astype(F)
    v = ulps(v0[..., None], DELTAS)
    return np.where(ok[..., None] & (v > 0) & (v <= 1), v, F(np.nan))


@functools.lru_cache(maxsize=None)
def witnesses(num, den, q):
    """(up, down): the float32 values v in (0, 1], ascending, whose code under the weight num / den differs from the code under the
    weight one ulp up / one ulp down; empty when the weight is a float"""
    w = F(num) / F(den)
    if float(w) * den == num:
        return np.zeros(0, F), np.zeros(0, F)
    code = QUANTISERS[q][3]
    v = candidates(w, q).reshape(-1)
    v = np.unique(v[~np.isnan(v)])
    zero = np.zeros_like(v)
    ref = code(TC.fmaf(w, v, zero))
    out = []
    for other in (np.nextafter(w, F(np.inf)), np.nextafter(w, F(0))):
        hit = v[code(TC.fmaf(other, v, zero)) != ref]
        if hit.size > PER_DIRECTION:                                   # spread over the codes
            hit = hit[np.linspace(0, hit.size - 1, PER_DIRECTION).astype(int)]
        hit.setflags(write=False)
        out.append(hit)
    return tuple(out)


def column_values(num, den, q, seed):
    """the values of one band coordinate over the columns of all its rounds: up and down witnesses alternating; for a weight that is
    a float, seeded random values"""
    up, down = witnesses(num, den, q)
    n = max(up.size, down.size)
    if n == 0:
        return np.random.default_rng(seed).uniform(0, 1, 16).astype(F)
    out = np.empty(2 * n, F)
    out[0::2], out[1::2] = np.resize(up if up.size else down, n), np.resize(down if down.size else up, n)
    return out


def rounds(T, O, q):
    """tile sets per band: as many as the coordinate with the most witnesses needs at T columns each, MAX_ROUNDS at the most"""
    most = max(sum(a.size for a in witnesses(n, 2 * O, q)) for n in numerators(O))
    return min(MAX_ROUNDS, max(1, -(-most // T)))


@functools.lru_cache(maxsize=None)
def band_set(T, O, q, axis, side, rnd):
    """(tiles [2,3,T,T], H, W): axis 0 a 2 x 1 grid (H = S + T, W = T), the vertical band; axis 1 its transpose.  side 1: the earlier
    tile is +0.0 and row u < O of the later tile is gray, one value of column_values per column; side 0: the later tile is +0.0 and
    row S + u of the earlier one is gray, under the weight (2 (O - 1 - u) + 1) / (2 O)"""
    S = T - O
    x = np.zeros((2, 3, T, T), F)
    for u in range(O):
        num = 2 * u + 1 if side else 2 * (O - 1 - u) + 1
        vals = column_values(num, 2 * O, q, seed=1000 * O + u)
        row = vals[(rnd * T + np.arange(T)) % vals.size]
        x[side, :, u if side else S + u, :] = row
    if axis == 1:
        x = np.ascontiguousarray(x.transpose(0, 1, 3, 2))
    x.setflags(write=False)
    return (x, S + T, T) if axis == 0 else (x, T, S + T)


def band_sets(T, O, q):
    """every (axis, side, round, tiles, H, W) of one overlap and quantiser"""
    return [(axis, side, r) + band_set(T, O, q, axis, side, r) for axis in (0, 1) for side in (0, 1) for r in range(rounds(T, O, q))]


# -- the corner: the product wy * wx and the fmaf --------------------------------------------------------------------------------------

#: the gray value of the three earlier tiles of the "lit" corner set
LIT = F(0.25)
CORNER_KINDS = ("zero", "lit")


def corner_weights(T, O):
    """float32 [4,O,O]: the weight of tile t of the 2 x 2 grid at the corner pixel (uy, ux), tiles_contract's own"""
    S = T - O
    out = []
    for i in range(2):
        wy = TC.weights(i, 2, T, O)[S:T] if i == 0 else TC.weights(i, 2, T, O)[:O]
        for j in range(2):
            wx = TC.weights(j, 2, T, O)[S:T] if j == 0 else TC.weights(j, 2, T, O)[:O]
            out.append((wy[:, None] * wx[None, :]).astype(F))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def corner_set(T, O, q, kind):
    """(tiles [4,3,T,T], H, W) of a 2 x 2 grid, H = W = S + T; the values that matter lie in the O x O corner of the last tile.
    "zero": three tiles of +0.0, so that m = fl(fl(wy wx) v): values sought under which fl(wy wx v), the product left unrounded,
    gives another code.  "lit": the three earlier tiles hold LIT in the corner, so that the last fmaf adds to a non-zero sum: values
    sought under which fl(fl(w v) + acc) gives another code than fmaf(w, v, acc).  (With three zero tiles that mutant is invisible:
    acc = 0 and fl(fl(w v) + 0) is fmaf(w, v, 0).)  Every cell takes the first candidate that qualifies, else a seeded value."""
    S = T - O
    code = QUANTISERS[q][3]
    n = QUANTISERS[q][2]
    w = corner_weights(T, O)
    g = np.random.default_rng(7 * T + O + len(q))
    ks = np.sort(g.choice(n, 12, replace=False))
    x = np.zeros((4, 3, T, T), F)
    acc = np.zeros((O, O), F)
    if kind == "lit":
        for t in range(3):
            acc = TC.fmaf(w[t], np.full((O, O), LIT, F), acc)
        x[0, :, S:, S:], x[1, :, S:, :O], x[2, :, :O, S:] = LIT, LIT, LIT
    v = candidates(w[3], q, acc, ks).reshape(O, O, -1)
    ok = ~np.isnan(v)
    v = np.where(ok, v, F(0.5))
    wt, a = w[3][..., None], acc[..., None]
    ref = TC.fmaf(np.broadcast_to(wt, v.shape), v, np.broadcast_to(a, v.shape))
    if kind == "zero":                                                 # the float64 product is exact, its product with v nearly
        exact = corner_weights64(T, O)[..., None] * v.astype(np.float64)
        mut = exact.astype(F)
    else:
        mut = ((wt * v).astype(F) + a).astype(F)
    hit = ok & (code(mut.reshape(-1)).reshape(v.shape) != code(ref.reshape(-1)).reshape(v.shape))
    first = np.where(hit.any(axis=2), hit.argmax(axis=2), g.integers(0, v.shape[2], (O, O)))
    x[3, :, :O, :O] = np.take_along_axis(v, first[..., None], axis=2)[..., 0]
    x.setflags(write=False)
    return x, S + T, S + T


def corner_weights64(T, O):
    """float64 [O,O]: the exact product wy * wx of the last tile's two float32 weights (48 bits)"""
    wy = TC.weights(1, 2, T, O)[:O].astype(np.float64)
    return wy[:, None] * wy[None, :]


def corner_window(T, O):
    return (T - O, T - O, O, O)


# -- the three restatements on one tile set ------------------------------------------------------------------------------------------

def render(lib, param, x, H, W, T, O, window=None):
    """the codes the library's restatement gives for tiles x: int64 [h,w] -- red of `tiles`, luma of the two others (the witness sets
    are gray)"""
    if lib == "tiles":
        return TC.stitch(x, H, W, T, O, param, "chw", window=window)[0].astype(np.int64)
    if lib == "frame_tiles":
        return GC.stitch_codes(x, H, W, T, O, param, MATRIX, RANGE, window=window)[0][0]
    return KC.stitch_codes(x, H, W, T, O, param, MATRIX, RANGE, SITING[param], window=window)[0][0]


# -- the mutants: what a kernel could get wrong, put into tiles_contract ---------------------------------------------------------------

MUTANTS = ("up", "down", "unrounded", "unfused")


def moved_weights(real, towards):
    def weights(i, n, T, O):
        w = real(i, n, T, O)
        if O == 0:
            return w
        scaled = w.astype(np.float64) * (2 * O)                        # exact: 24 + 8 bits; the numerator where w is a float
        return np.where(scaled != np.rint(scaled), np.nextafter(w, F(towards)), w).astype(F)
    return weights


def int_of(v):
    """finite float -> (integer, exponent), exactly"""
    m, e = math.frexp(float(v))
    return int(m * (1 << 53)), e - 53


def round32(N, e):
    """the non-negative N * 2^e rounded once to float32, to nearest even (normal range)"""
    drop = N.bit_length() - 24
    if drop <= 0:
        return math.ldexp(N, e)
    q = N >> drop
    rem, half = N - (q << drop), 1 << (drop - 1)
    if rem > half or (rem == half and q & 1):
        q += 1
    assert e + drop > -120
    return math.ldexp(q, e + drop)


def fmaf_unrounded(a, b, c):
    """a * b + c rounded once to float32 for a float64 `a` of up to 48 bits (the exact product of two float32 weights): in
    integers wherever a is no float32 and b is not zero, tiles_contract's fmaf elsewhere"""
    a, b, c = np.broadcast_arrays(np.atleast_1d(np.asarray(a, np.float64)), np.asarray(b, F), np.asarray(c, F))
    a32 = a.astype(F)
    out = np.array(FMAF(a32, b, c))
    for idx in zip(*np.nonzero((a32.astype(np.float64) != a) & (b != 0))):
        (na, ea), (nb, eb), (nc, ec) = int_of(a[idx]), int_of(b[idx]), int_of(c[idx])
        e = min(ea + eb, ec)
        out[idx] = round32(((na * nb) << (ea + eb - e)) + (nc << (ec - e)), e)
    return out


def fmaf_unfused(a, b, c):
    """a rounded float32 multiply, then a rounded float32 add"""
    p = (np.asarray(a, F) * np.asarray(b, F)).astype(F)
    return (p + np.asarray(c, F)).astype(F)


WEIGHTS, PRODUCT, FMAF = TC.weights, TC.product, TC.fmaf


@contextlib.contextmanager
def mutant(name):
    """tiles_contract, and with it the two restatements that blend through it, with one rule broken"""
    if name == "up":
        TC.weights = moved_weights(WEIGHTS, np.inf)
    elif name == "down":
        TC.weights = moved_weights(WEIGHTS, 0)
    elif name == "unrounded":
        TC.product = lambda wy, wx: wy.astype(np.float64)[:, None] * wx.astype(np.float64)[None, :]
        TC.fmaf = fmaf_unrounded
    elif name == "unfused":
        TC.fmaf = fmaf_unfused
    else:
        raise ValueError(name)
    try:
        yield
    finally:
        TC.weights, TC.product, TC.fmaf = WEIGHTS, PRODUCT, FMAF


# -- the hostile matrix at the new overlaps --------------------------------------------------------------------------------------------

#: (T, H, W): two sizes of 2 x 3 and 3 x 3 grids with clipped last tiles at T = 64, one at T = 128
HOSTILE_SIZES = [(64, 100, 150), (64, 127, 129), (128, 200, 300)]


def hostile_cases():
    """(T, O, H, W) of the matrix: every overlap of the table at its T's sizes that leaves more than one tile a side"""
    return [(T, O, H, W) for T, O in OVERLAPS for TT, H, W in HOSTILE_SIZES if TT == T]


def hostile_windows(T, O, H, W, sx=2, sy=2):
    """the whole picture; a window that starts inside the first band on both axes and ends inside the picture; one that ends on the
    picture's odd or even last row and column and starts before a band.  Starts and sizes are multiples of the subsampling."""
    S = T - O
    inside = (S + 2 * sy, S + 2 * sx, min(O + 6, H - S - 2 * sy) // sy * sy, min(O + 10, W - S - 2 * sx) // sx * sx)
    last = (S - 2 * sy, S - 4 * sx, H - S + 2 * sy, W - S + 4 * sx)
    return [(0, 0, H, W), inside, last]

"""chroma_tiles and chroma_rate (section 24) past T = 64: the case table and the builders of
tests/test_chroma_limits_host.py (no GPU) and tests/test_gpu_chroma_limits.py (GPU).  Not a test file and not a conftest: numpy and
the restatements (tests/*_contract.py) only.  The sizes are tests/image_limits.py's (SECOND_TRIP: T = 576 on 601 x 1101, FOUR_TRIPS:
T = 1024 on 1030 x 1500, WHOLE: 1026 x 1030 in 576-tiles at O = 64); what is new is the subsampling, which sets how many block
partials a tile or a picture has, and the siting, which chooses the kernel.

  cut      T = 576 at four overlaps under both upsamplers, and tile (1, 1) alone of a 4098^2 frame at T = 2048;
  stitch   T = 576 at O = 64 and O = 288 (den = 576, no power of two: also a case of tests/band_cases.py's kind) on hostile tiles;
           whole pictures with 518 (4:2:2) and 259 (4:2:0) block partials, hostile and tail-only;
  rate     T = 576 (81 partials per tile at 4:2:0, 162 at 4:2:2 and 4:4:4) and T = 1024 (256 and 512: four and eight trips of
           row_final) on hostile tiles; tail-only tiles; the largest tile at 4:2:0 and 4:2:2 against closed forms in Python ints.
"""
import functools

import numpy as np

from tests import chroma_contract as CC
from tests import chroma_rate_contract as XC
from tests import image_limits as IL
from tests import tiles_contract as TC

# -- the table -----------------------------------------------------------------------------------------------------------------------

SECOND_TRIP, FOUR_TRIPS, WHOLE = IL.SECOND_TRIP, IL.FOUR_TRIPS, IL.WHOLE
#: O at T = 576: image_limits' three and O = T / 2, where S = 288 and every interior pixel lies in a band
OVERLAPS = [0, 64, 4, 288]
#: (format, siting) of the cuts and of the rate cases: 4:2:0 under VCO, 4:2:2 at ten bits, 4:4:4
FORMATS = [("nv12", "topleft"), ("p210", "left"), ("i444", "centre")]
#: the stitches at T = 576
STITCH_FORMATS = [("nv12", "topleft"), ("nv16", "left"), ("p010", "centre")]
STITCH_OVERLAPS = [64, 288]
#: the whole pictures: (format, siting, block partials of the picture)
WHOLE_FORMATS = [("nv16", "left", 518), ("nv12", "topleft", 259)]
#: the rate cases at T = 1024: (format, siting, block partials per tile, trips of row_final's 64 lanes)
RATE_1024 = [("p010", "left", 256, 4), ("p210", "topleft", 512, 8)]
#: the largest tile of chroma_rate at 4:2:0 and 4:2:2: tile 4 of 3 x 3 lies in bands entirely
RATE_LIMIT = dict(T=2048, O=1024, H=4096, W=4096, tile=4)
RATE_LIMIT_FORMATS = [("nv12", "topleft"), ("nv16", "left")]
#: the largest cut: the tile size of image_limits.CUT_LARGE, the largest any library that takes the tiles admits (chroma_rate, 8 bits);
#: pc_chroma_tiles.h itself states no bound but that T * T / 8 fits 31 bits
CUT_LARGE = dict(IL.CUT_LARGE, fmt="nv12", siting="left")

MATRICES = list(CC.MATRICES)


def partials_per_tile(T, fmt):
    """chroma_rate: a work item is sy rows by eight columns, a block 256 items"""
    return T * T // (2048 * CC.sub(fmt)[1])


def stitch_partials(h, w, fmt, x0=0):
    """chroma_tiles.stitch: ceil(h / sy) * (eight-column items of the window) items, 256 to a block"""
    sy = CC.sub(fmt)[1]
    return -(-(-(-h // sy) * (-(-(x0 + w) // 8) - x0 // 8)) // 256)


@functools.lru_cache(maxsize=None)
def hostile(n, T, seed):
    x = TC.hostile_tiles(n, T, seed)
    x.setflags(write=False)
    return x


def settings(k):
    """(matrix, range) cycling with k"""
    return MATRICES[k % 3], CC.RANGES[k % 2]


def sub_rect(ny, nx):
    """a rectangle that does not start at the grid's origin: the last row of tiles from the second column on"""
    return (ny - 1, 1, 1, nx - 1)


# -- tail-only data ------------------------------------------------------------------------------------------------------------------

def last_row_tail(x_equal, T, O, H, W):
    """tiles of the whole grid -> the same with the picture's LAST luma row flipped in every tile that holds it"""
    ny, nx = TC.grid(H, W, T, O)
    S = T - O
    out = np.array(x_equal)
    for i in range(ny):
        r = H - 1 - i * S
        if 0 <= r < T:
            out[i * nx:(i + 1) * nx, :, r, :] = IL.flip(x_equal[i * nx:(i + 1) * nx, :, r, :])
    return out


def rate_tail(fmt, siting, T, H, W, matrix="bt709", rng="limited", seed=0):
    """(x_tail, x_equal [1,3,T,T], frame): tile 0 (O = 0) inside the frame; the frame holds under tile 0 the tile's own rendering
    (chroma_contract's emit of it), every error zero; x_tail differs from x_equal in the tile's last sy rows alone: one luma row
    (pair) and the last chroma row, the last items of the tile's last block"""
    sx, sy = CC.sub(fmt)
    assert T <= H and T <= W
    eq = np.array(hostile(1, T, seed + 1))
    Y, Cb, Cr = (np.array(c) for c in CC.codes(CC.random_frame(1, H, W, fmt, seed), fmt))
    tY, tCb, tCr = XC.tile_codes(eq[0], T, T, fmt, matrix, rng, siting)
    Y[0, :T, :T], Cb[0, :T // sy, :T // sx], Cr[0, :T // sy, :T // sx] = tY, tCb, tCr
    tail = np.array(eq)
    tail[:, :, T - sy:, :] = IL.flip(eq[:, :, T - sy:, :])
    return tail, eq, CC.frame(Y, Cb, Cr, fmt)


# -- the largest tile: closed forms in Python ints -----------------------------------------------------------------------------------

def const_frame(fmt, H, W, y, cb, cr):
    Hc, Wc = CC.chroma_size(H, W, fmt)
    return CC.frame(np.full((1, H, W), y, np.int64), np.full((1, Hc, Wc), cb, np.int64), np.full((1, Hc, Wc), cr, np.int64), fmt)


def rate_saturated(fmt, H, W):
    """(frame, eY, eC) in full range: zero tiles (codes 0, co, co under every siting) against Y at the top code and chroma 0"""
    _, _, co, _, mx = CC.levels(fmt, "full")
    return const_frame(fmt, H, W, mx, 0, 0), mx, co


def rate_closed(c, fmt, eY, eC):
    """[Y, Cb, Cr]: image_limits.frame_rate_closed with the chroma axes halved where the format subsamples them: a chroma weight is
    the mean of its two luma numerators on a subsampled axis, the luma numerator on the other"""
    ny, nx = TC.grid(c["H"], c["W"], c["T"], c["O"])
    i, j = divmod(c["tile"], nx)
    sx, sy = CC.sub(fmt)
    wy, wx = IL.axis_weight_sum(i, ny, c["T"], c["O"]), IL.axis_weight_sum(j, nx, c["T"], c["O"])
    assert wy % sy == 0 and wx % sx == 0
    ch = eC * eC * (wy // sy) * (wx // sx)
    return [eY * eY * wy * wx, ch, ch]

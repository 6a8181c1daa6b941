"""chroma_clips past T = 64: the case table and the builders of tests/test_chroma_clips_limits_host.py (no GPU)
and tests/test_gpu_chroma_clips_limits.py (GPU).  Not a test file and not a conftest: numpy and the restatements (tests/*_contract.py)
only.  The sizes are tests/image_limits.py's (SECOND_TRIP: T = 576 on 601 x 1101, FOUR_TRIPS: T = 1024 on 1030 x 1500, CLIP_LIMIT:
T = 2048 on 4098 x 4098); what is new is the halo ring with four flags, which clips has no counterpart of, and the subsampling, which
sets how many block partials a tile has.

  ring     T = 128 on 300 x 300: the witness samples are ring indices 256 .. 259 and later, the loop's second trip at its smallest
           size; T = 576 on 1300 x 1300: each side of tile 4's ring alone and its four corners, five and seven trips;
  final    T = 576 (82 partials per tile at 4:2:0, 163 at 4:2:2 and 4:4:4), T = 1024 (257 and 513: the ring's partial is the only
           entry of the fifth and of the ninth trip), T = 2048 (1025 and 2049); tail-only pairs;
  cut      the list cut at T = 576 at four overlaps and at T = 2048.

What the kernels do with a sample is stated here a second time, as a LAYOUT MODEL (which block and thread of a tile holds which
sample, which ring index which ring sample) from pc_chroma_clips.hip's head comment and DESIGN.md section 25.  It is used for two
things only: to assert where the witness samples land, and to build MUTANTS -- numpy functions that count as a subtly wrong kernel
would.  tests/test_chroma_clips_limits_host.py asserts that every mutant differs from the restatement on a named case of this table.
The expected values of the GPU tests are the restatement's (tests/chroma_clips_contract.py), never the model's.
"""
import functools

import numpy as np

from tests import chroma_contract as CC
from tests import chroma_limits as CL
from tests import image_limits as IL
from tests import tiles_contract as TC

# -- the table -----------------------------------------------------------------------------------------------------------------------

SECOND_TRIP, FOUR_TRIPS, CLIP_LIMIT = IL.SECOND_TRIP, IL.FOUR_TRIPS, IL.CLIP_LIMIT
OVERLAPS = CL.OVERLAPS                                                     # O at T = 576: 0, 64, 4 and T / 2
FORMATS = CL.FORMATS                                                       # nv12 topleft, p210 left, i444 centre
#: the ring's second trip at its smallest size: tile 4 of 3 x 3
RING_SMALL = dict(T=128, O=0, H=300, W=300, tile=4)
RING_SMALL_FORMATS = ["nv12", "nv16"]
#: each ring side alone: tile 4 of 3 x 3; (format, indices of the ring loop under centre / linear, its trips of 256 threads)
RING_SIDES = dict(T=576, O=0, H=1300, W=1300, tile=4)
RING_SIDES_FORMATS = [("nv12", 1156, 5), ("p210", 1732, 7)]
SIDES = ["above", "below", "left", "right", "corners"]
#: the Cr samples a side pair leaves unchanged at the start of the side (Cb changes in all of them, corners included)
CR_SKIP = 5
#: T = 1024: (format, siting, partials per tile with the ring's, trips of the final's 64 lanes)
FINAL_1024 = [("p010", "left", 257, 5), ("p210", "topleft", 513, 9)]
TAIL_FORMATS = FORMATS + [("p210", "topleft")]
#: the largest tile: (format, siting, chroma samples of tile 4's footprint under linear and under nearest upsampling)
LIMIT_FORMATS = [("nv12", "centre", 1026 * 1026, 1024 * 1024), ("nv12", "topleft", 1025 * 1025, 1024 * 1024),
                 ("p210", "left", 2048 * 1025, 2048 * 1024)]
LIMIT_LUMA = 4194304
#: the list cut at T = 2048: the frame of chroma_limits.CUT_LARGE; tile 8 is a 2 x 2-pixel corner
CUT_LIST_LARGE = dict(CL.CUT_LARGE, tiles=[4, 0, 8, 4], raw=[4, 9, -1, 0])
#: (T, partials per tile at sy = 2, at sy = 1, trips at sy = 2, at sy = 1) as the issue of this table states them
TRIPS = [(576, 82, 163, 2, 3), (1024, 257, 513, 5, 9), (2048, 1025, 2049, 17, 33)]

#: the size cap: no frame of this table is larger, and no list at T = 2048 longer
MAX_FRAME = (4098, 4098)
MAX_LIST_AT_2048 = 4

NT = 256                                                                   # threads of a block: items of an item block
POISON = 0xA5A5A5A5A5A5A5A5                                                # the 64-bit word the GPU tests fill the workspace with


def partials_per_tile(T, fmt):
    """T * T / (2048 sy) item blocks and the ring's"""
    return T * T // (2048 * CC.sub(fmt)[1]) + 1


def trips(partials):
    """of the final's 64 lanes over a row of partials"""
    return -(-partials // 64)


def frames_of_the_table():
    """(H, W) of every case"""
    return [(c["H"], c["W"]) for c in (RING_SMALL, RING_SIDES, SECOND_TRIP, FOUR_TRIPS, CLIP_LIMIT, CUT_LIST_LARGE)]


def workspace_cases():
    """(T, sy, n) of every raw changes call of the table: whole grids, sub-ranges and single tiles"""
    out = set()
    for c, fmts in [(RING_SMALL, RING_SMALL_FORMATS), (RING_SIDES, [f for f, _, _ in RING_SIDES_FORMATS]),
                    (dict(SECOND_TRIP, O=0), [f for f, _ in TAIL_FORMATS]), (FOUR_TRIPS, [f for f, _, _, _ in FINAL_1024]),
                    (CLIP_LIMIT, [f for f, _, _, _ in LIMIT_FORMATS])]:
        n = int(np.prod(TC.grid(c["H"], c["W"], c["T"], c["O"])))
        out |= {(c["T"], CC.sub(f)[1], m) for f in fmts for m in {n, 1, IL.sub_range(n)[1]}}
    for O in OVERLAPS:
        n = int(np.prod(TC.grid(SECOND_TRIP["H"], SECOND_TRIP["W"], SECOND_TRIP["T"], O)))
        out |= {(SECOND_TRIP["T"], CC.sub(f)[1], m) for f, _ in FORMATS for m in {n, 1, IL.sub_range(n)[1]}}
    return sorted(out)


# -- the rule and the layout model ---------------------------------------------------------------------------------------------------

def rule(fmt, siting, upsample):
    """(ylo, yhi, xlo, xhi) as 0 / 1: pc_chroma_clips.h's footprint -- on a subsampled axis hi = 1 for linear upsampling, lo = 1 for
    linear upsampling and a centre-sited axis"""
    sx, sy = CC.sub(fmt)
    hco, vco = CC.SITINGS[siting]
    lin = upsample == "linear"
    return (int(sy == 2 and lin and not vco), int(sy == 2 and lin), int(sx == 2 and lin and not hco), int(sx == 2 and lin))


def tile_geo(H, W, T, O, fmt, tile):
    """the tile's part of the frame (Yt, Xt, hh, ww) and the chroma rectangle its items cover (r0c, r1c, c0c, c1c), inclusive"""
    sx, sy = CC.sub(fmt)
    _, nx = TC.grid(H, W, T, O)
    i, j = divmod(tile, nx)
    Yt, Xt = i * (T - O), j * (T - O)
    hh, ww = min(T, H - Yt), min(T, W - Xt)
    r0c, c0c = Yt // sy, Xt // sx
    return (Yt, Xt, hh, ww), (r0c, r0c + -(-hh // sy) - 1, c0c, c0c + -(-ww // sx) - 1)


def ring(H, W, T, O, fmt, flags, tile, corners=True, right_at=1):
    """the ring block's index space: (row, col, on) arrays over idx < 2 nw + 2 nh -- the chroma row above the items' rectangle, the
    row below (both nw samples, from the column left of it to the column right of it where those sides are on), the column left and
    the column right (nh samples each).  corners / right_at are the mutants' knobs."""
    ylo, yhi, xlo, xhi = flags
    Hc, Wc = CC.chroma_size(H, W, fmt)
    _, (r0c, r1c, c0c, c1c) = tile_geo(H, W, T, O, fmt, tile)
    top, bottom, left, right = bool(ylo and r0c > 0), bool(yhi and r1c < Hc - 1), bool(xlo and c0c > 0), bool(xhi and c1c < Wc - 1)
    cf = c0c - left
    nw, nh = c1c + right - cf + 1, r1c - r0c + 1
    acr, down = np.arange(nw), np.arange(nh)
    row = np.concatenate([np.full(nw, r0c - 1), np.full(nw, r1c + 1), r0c + down, r0c + down])
    col = np.concatenate([cf + acr, cf + acr, np.full(nh, c0c - 1), np.full(nh, c1c + right_at)])
    on = np.concatenate([np.full(nw, top), np.full(nw, bottom), np.full(nh, left), np.full(nh, right)])
    if not corners:
        on[:2 * nw] &= (col[:2 * nw] >= c0c) & (col[:2 * nw] <= c1c)
    return row, col, on


def ring_index(H, W, T, O, fmt, siting, upsample, tile, row, col):
    """the loop index that holds chroma sample (row, col) of the tile's ring, or None"""
    r, c, on = ring(H, W, T, O, fmt, rule(fmt, siting, upsample), tile)
    hit = np.nonzero((r == row) & (c == col) & on)[0]
    assert len(hit) <= 1
    return int(hit[0]) if len(hit) else None


def item_block(T, fmt, y, x):
    """the item block of a tile that holds its luma sample (y, x) -- and the chroma sample (y / sy, x / sx): item (kp, g) = (y / sy,
    x / 8) is number kp * (T / 8) + g of the tile, 256 to a block"""
    sy = CC.sub(fmt)[1]
    return ((y // sy) * (T // 8) + x // 8) // NT


def tile_partials(d, H, W, T, O, fmt, flags, tile, **knobs):
    """the model: d = the three planes' boolean difference maps -> (int [bpt + 1, 3], the tile's row of block partials; bool [bpt],
    whether the block has an active item)"""
    sx, sy = CC.sub(fmt)
    (Yt, Xt, hh, ww), _ = tile_geo(H, W, T, O, fmt, tile)
    G8, bpt = T // 8, T * T // (8 * sy * NT)
    per = []
    for p, (fy, fx) in enumerate([(1, 1), (sy, sx), (sy, sx)]):
        a = np.zeros((T // fy, T // fx), np.int64)
        part = d[p][Yt // fy:Yt // fy + -(-hh // fy), Xt // fx:Xt // fx + -(-ww // fx)]
        a[:part.shape[0], :part.shape[1]] = part
        per.append(a.reshape(T // sy, (sy if p == 0 else 1), G8, -1).sum(axis=(1, 3)).reshape(bpt, NT).sum(axis=1))
    kp, g = np.divmod(np.arange(bpt * NT), G8)
    active = ((sy * kp < hh) & (8 * g < ww)).reshape(bpt, NT).any(axis=1)
    row, col, on = ring(H, W, T, O, fmt, flags, tile, **{k: v for k, v in knobs.items() if k in ("corners", "right_at")})
    limit = knobs.get("ring_limit")
    if limit is not None:
        on = on & (np.arange(len(on)) < limit)
    planes = (2, 1) if knobs.get("ring_swapped") else (1, 2)
    halo = [0, 0, 0]
    for p, q in zip((1, 2), planes):
        halo[p] = int(d[q][row[on], col[on]].sum())
    return np.concatenate([np.stack(per, axis=1), np.array([halo])]), active


#: the mutants: name -> what a wrong kernel of that kind would do, as knobs of the model
MUTANTS = {
    "final_first_64": dict(final_limit=64),            # the final gathers only the first 64 partials of a row
    "ring_first_256": dict(ring_limit=NT),             # the ring loop stops after its first trip
    "swap_lo_hi_y": dict(swap="y"),                    # lo and hi swapped on the vertical axis
    "swap_lo_hi_x": dict(swap="x"),                    # ... on the horizontal axis
    "swap_sitings": dict(swap="sitings"),              # horizontal and vertical siting swapped
    "ring_without_corners": dict(corners=False),
    "right_column_at_c1c": dict(right_at=0),           # the right column read at c1c instead of c1c + 1
    "ring_cb_cr_swapped": dict(ring_swapped=True),
    "inactive_block_unwritten": dict(poison=True),     # a block without an active item leaves the workspace's poison
}


def model_flags(fmt, siting, upsample, swap=None):
    if swap == "sitings":
        hco, vco = CC.SITINGS[siting]
        siting = {(False, False): "centre", (False, True): None, (True, True): "topleft", (True, False): "left"}[(vco, hco)]
        if siting is None:                             # vertically co-sited, horizontally centred: no name, the flags directly
            sx, sy = CC.sub(fmt)
            lin = upsample == "linear"
            return (0, int(sy == 2 and lin), int(sx == 2 and lin), int(sx == 2 and lin))
    ylo, yhi, xlo, xhi = rule(fmt, siting, upsample)
    return {"y": (yhi, ylo, xlo, xhi), "x": (ylo, yhi, xhi, xlo)}.get(swap, (ylo, yhi, xlo, xhi))


def diff_maps(cur, prev, fmt):
    """(the three planes' boolean difference maps of the codes, H, W)"""
    a, b = CC.codes(cur, fmt), CC.codes(prev, fmt)
    return [x[0] != y[0] for x, y in zip(a, b)], a[0].shape[1], a[0].shape[2]


def model_counts(d, H, W, fmt, siting, T, O, upsample, tiles=None, mutant=None):
    """[n][3] Python ints in [0, 2^64): the counts by the layout model from diff_maps' d; mutant: a name of MUTANTS"""
    knobs = dict(MUTANTS[mutant]) if mutant else {}
    flags = model_flags(fmt, siting, upsample, knobs.get("swap"))
    ny, nx = TC.grid(H, W, T, O)
    out = []
    for t in range(ny * nx) if tiles is None else tiles:
        part, active = tile_partials(d, H, W, T, O, fmt, flags, t, **knobs)
        sums = [int(v) for v in part[:knobs.get("final_limit")].sum(axis=0)]
        if knobs.get("poison"):
            sums = [(v + int((~active).sum()) * POISON) % 2 ** 64 for v in sums]
        out.append(sums)
    return out


def model_changes(cur, prev, fmt, siting, T, O, upsample, tiles=None, mutant=None):
    d, H, W = diff_maps(cur, prev, fmt)
    return model_counts(d, H, W, fmt, siting, T, O, upsample, tiles, mutant)


# -- data ----------------------------------------------------------------------------------------------------------------------------

def top_of(fmt):
    return 1 << CC.bits(fmt)


def smooth_frame(fmt, H, W):
    """ramps over the code range"""
    top = top_of(fmt)
    Hc, Wc = CC.chroma_size(H, W, fmt)
    y, x = np.mgrid[0:H, 0:W]
    cy, cx = np.mgrid[0:Hc, 0:Wc]
    return CC.frame(((y + 2 * x) * top // (H + 2 * W))[None], ((2 * cy + cx) * top // (2 * Hc + Wc))[None],
                    ((Hc - cy + cx) * top // (Hc + Wc + 1))[None], fmt)


def changed(codes, fmt, where, plane, k=1):
    """codes (three writable arrays [1, h, w]) with the codes of `plane` at `where` moved by k (0 < k < top): every one differs"""
    top = top_of(fmt)
    assert 0 < k < top
    codes[plane][0][where] = (codes[plane][0][where] + k) % top
    return codes


def codes_of(f, fmt):
    return [np.array(c) for c in CC.codes(f, fmt)]


def below_the_code(f, fmt, seed):
    """the frame with the bits of its 16-bit words outside the code randomised"""
    n, sh = CC.FORMATS[fmt][1:3]
    assert n == 10
    keep = np.uint16((2 ** n - 1) << sh)
    g = np.random.default_rng(seed)
    return tuple((p & keep) | (g.integers(0, 2 ** 16, p.shape).astype(np.uint16) & ~keep) for p in f)


# 1: the ring's second trip at its smallest size

def ring_small_witness(fmt, c=RING_SMALL):
    """[(plane, chroma row, chroma column)] of the samples that differ.  nv12: Cb rows 124 .. 127 of column 128, tile 4's right column
    from loop index 256 on under centre / linear.  nv16: Cb rows 252 .. 255 of column 128 (the last four indices of the loop) and
    Cr rows 252 .. 255 of column 63, tile 4's left column, indices 256 .. 259 under centre / linear."""
    T = c["T"]
    sy = CC.sub(fmt)[1]
    last = range(2 * T // sy - 4, 2 * T // sy)
    out = [(1, r, T // 2 * 2) for r in last]
    return out + ([(2, r, T // 2 - 1) for r in last] if sy == 1 else [])


@functools.lru_cache(maxsize=None)
def ring_small_pair(fmt, kind):
    """(cur, prev): prev smooth or random; cur differs from it in ring_small_witness alone"""
    H, W = RING_SMALL["H"], RING_SMALL["W"]
    prev = smooth_frame(fmt, H, W) if kind == "smooth" else CC.random_frame(1, H, W, fmt, seed=128)
    codes = codes_of(prev, fmt)
    for p, r, col in ring_small_witness(fmt):
        changed(codes, fmt, (r, col), p, 1 + r % 3)
    return CC.frame(*codes, fmt), prev


def ring_small_expect(fmt, siting, upsample):
    """{tile: counts} the table expects; every other tile counts nothing.  At 4:2:0 chroma (127, 128) is also a sample of the row
    above tiles 7 and 8, tile 7's corner"""
    ylo, _, xlo, xhi = rule(fmt, siting, upsample)
    if CC.sub(fmt)[1] == 2:
        return {4: [0, 4 * xhi, 0], 5: [0, 4, 0], 7: [0, ylo * xhi, 0], 8: [0, ylo, 0]}
    return {3: [0, 0, 4], 4: [0, 4 * xhi, 4 * xlo], 5: [0, 4, 0]}


# 2: each ring side alone

def side_samples(fmt, side, c=RING_SIDES):
    """(Cb, Cr): index tuples (rows, cols) of the chroma samples a side pair changes.  Cb: the complete row or column, corners
    included; Cr: the side without its corners and without its first CR_SKIP samples.  "corners": Cb all four, Cr the top left one
    alone (the bottom right one counts under every linear rule of 4:2:0: Cr must not follow it)."""
    _, (r0c, r1c, c0c, c1c) = tile_geo(c["H"], c["W"], c["T"], c["O"], fmt, c["tile"])
    across, down = np.arange(c0c - 1, c1c + 2), np.arange(r0c - 1, r1c + 2)
    if side in ("above", "below"):
        r = r0c - 1 if side == "above" else r1c + 1
        return (np.full(len(across), r), across), (np.full(len(across) - 2 - CR_SKIP, r), across[1 + CR_SKIP:-1])
    if side in ("left", "right"):
        col = c0c - 1 if side == "left" else c1c + 1
        return (down, np.full(len(down), col)), (down[1 + CR_SKIP:-1], np.full(len(down) - 2 - CR_SKIP, col))
    rr, cc = np.array([r0c - 1, r0c - 1, r1c + 1, r1c + 1]), np.array([c0c - 1, c1c + 1, c0c - 1, c1c + 1])
    return (rr, cc), (rr[:1], cc[:1])


@functools.lru_cache(maxsize=None)
def ring_side_prev(fmt, H, W):
    return CC.random_frame(1, H, W, fmt, seed=576)


def ring_side_pair(fmt, side, c=RING_SIDES):
    key = tuple(sorted(c.items()))
    return _ring_side_pair(fmt, side, key)


@functools.lru_cache(maxsize=None)
def _ring_side_pair(fmt, side, key):
    c = dict(key)
    prev = ring_side_prev(fmt, c["H"], c["W"])
    codes = codes_of(prev, fmt)
    cb, cr = side_samples(fmt, side, c)
    changed(codes, fmt, cb, 1, 1)
    changed(codes, fmt, cr, 2, top_of(fmt) // 2)
    return CC.frame(*codes, fmt), prev


def ring_side_expect(fmt, siting, upsample, side, c=RING_SIDES):
    """tile 4's counts, the table's own: side length or 0 per lo / hi"""
    ylo, yhi, xlo, xhi = rule(fmt, siting, upsample)
    _, (r0c, r1c, c0c, c1c) = tile_geo(c["H"], c["W"], c["T"], c["O"], fmt, c["tile"])
    nw, nh = c1c - c0c + 1, r1c - r0c + 1
    return {"above": [0, ylo * (nw + xlo + xhi), ylo * (nw - CR_SKIP)], "below": [0, yhi * (nw + xlo + xhi), yhi * (nw - CR_SKIP)],
            "left": [0, xlo * (nh + ylo + yhi), xlo * (nh - CR_SKIP)], "right": [0, xhi * (nh + ylo + yhi), xhi * (nh - CR_SKIP)],
            "corners": [0, (ylo + yhi) * (xlo + xhi), ylo * xlo]}[side]


# 4: one ring sample of tile 0 at T = 1024

def ring_sample_1024(fmt):
    """(chroma row, chroma column) of one sample of tile 0's ring: the row below at 4:2:0, the column right at 4:2:2"""
    T = FOUR_TRIPS["T"]
    return (T // 2, 100) if CC.sub(fmt)[1] == 2 else (700, T // 2)


@functools.lru_cache(maxsize=None)
def ring_sample_pair(fmt):
    """(cur, prev) on FOUR_TRIPS' frame: random, the Cb sample ring_sample_1024 differs and nothing else"""
    prev = CC.random_frame(1, FOUR_TRIPS["H"], FOUR_TRIPS["W"], fmt, seed=1024, garbage=True)
    codes = changed(codes_of(prev, fmt), fmt, ring_sample_1024(fmt), 1, 7)
    return below_the_code(CC.frame(*codes, fmt), fmt, 3), prev


# 5: tail-only

def tail_halo_sample(fmt, T):
    """the Cb ring sample of tile 0 the tail pair adds with halo=True: (chroma row, column) in the row below for 4:2:0, in the column
    right for 4:2:2, None at 4:4:4 (no ring)"""
    sx, sy = CC.sub(fmt)
    return (T // 2, T // 4 + 1) if sy == 2 else (T // 4 + 1, T // 2) if sx == 2 else None


def tail_pair(fmt, T, H, W, halo, seed=0):
    """(cur, prev): prev random; cur differs from it in tile 0's last sy luma rows and last chroma row (O = 0, the tile inside the
    frame) and, with `halo`, in tail_halo_sample"""
    sx, sy = CC.sub(fmt)
    assert T < H and T < W
    prev = CC.random_frame(1, H, W, fmt, seed, garbage=True)
    codes = codes_of(prev, fmt)
    changed(codes, fmt, (slice(T - sy, T), slice(0, T)), 0, 1)
    changed(codes, fmt, (T // sy - 1, slice(0, T // sx)), 1, top_of(fmt) - 1)
    changed(codes, fmt, (T // sy - 1, slice(0, T // sx)), 2, top_of(fmt) // 2)
    if halo and tail_halo_sample(fmt, T):
        changed(codes, fmt, tail_halo_sample(fmt, T), 1, 3)
    return CC.frame(*codes, fmt), prev


def tail_expect(fmt, siting, upsample, T, halo):
    """tile 0's counts in closed form"""
    sx, sy = CC.sub(fmt)
    _, yhi, _, xhi = rule(fmt, siting, upsample)
    ring_on = (yhi if sy == 2 else xhi) if halo and tail_halo_sample(fmt, T) else 0
    return [sy * T, T // sx + ring_on, T // sx]


# 6: the largest tile

def limit_frames(fmt):
    """(all codes 0, all codes at the top, and at 10 bits the second with other bits below the code)"""
    c = CLIP_LIMIT
    top = top_of(fmt) - 1
    f0, f1 = CL.const_frame(fmt, c["H"], c["W"], 0, 0, 0), CL.const_frame(fmt, c["H"], c["W"], top, top, top)
    return f0, f1, (below_the_code(f1, fmt, 10) if CC.bits(fmt) == 10 else None)


def limit_expect(fmt, siting, upsample, T=CLIP_LIMIT["T"]):
    """tile 4 of 3 x 3 at O = 0 on a (2 T + 2)^2 frame: the whole footprint in closed form"""
    sx, sy = CC.sub(fmt)
    ylo, yhi, xlo, xhi = rule(fmt, siting, upsample)
    ch = (T // sy + ylo + yhi) * (T // sx + xlo + xhi)
    return [T * T, ch, ch]


# 3, 7: the lists of the cut

def cut_lists(n, seed):
    """a scattered list with repeats and the reversed list"""
    g = np.random.default_rng(seed)
    return [[int(v) for v in g.permutation(n)] + [int(v) for v in g.integers(0, n, 3)], list(range(n - 1, -1, -1))]


def all_differ(table):
    """every tile's three counts differ from every other tile's"""
    return len({tuple(r) for r in table}) == len(table)


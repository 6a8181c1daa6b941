"""The three stitch kernels (libpc_tiles.so, libpc_frame_tiles.so, libpc_chroma_tiles.so) at overlaps whose band weights are no
floats, against their restatements: exact equality of planes and integer sums throughout; the one tolerance is the derived bound
of tests/test_gpu_tiles.py on `sse_f`, h * w * 2^-53 * sse_f.

At O in {4, 16, 32, 64, 512, 1024} -- what every other GPU test uses -- 2 O is a power of two, every weight (2u+1)/(2 O) and every
product wy * wx is exact, and a division that is one ulp off, an unrounded product or an unfused multiply-add changes nothing.
tests/band_cases.py has the overlaps at which they are not and the witness tile sets, whose codes sit on rounding ties;
tests/test_band_weights_host.py shows on the CPU that every such error changes a code of these sets.  Here the sets, and hostile
tiles at the same overlaps, go through the kernels on both access paths."""
import numpy as np
import pytest
import torch

from tests import band_cases as BC
from tests import chroma_contract as CC
from tests import chroma_tiles_contract as KC
from tests import frame_tiles_contract as GC
from tests import frames_contract as FC
from tests import test_gpu_chroma_tiles as GK
from tests import test_gpu_frame_tiles as GF
from tests import test_gpu_tiles as GT
from tests import tiles_contract as TC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PATHS = (True, False)                                                      # wide, narrow


def rect_index(nx, rect):
    return [(rect[0] + a) * nx + rect[1] + b for a in range(rect[2]) for b in range(rect[3])]


def full_rect(H, W, T, O):
    return (0, 0) + TC.grid(H, W, T, O)


# -- one stitch of each library against its restatement, image and sums, on the paths asked for ----------------------------------------

def check_tiles(x, H, W, T, O, rounding, win=None, rect=None, paths=PATHS, ref_chw=None, note=None):
    tiles = GT.TL()
    L = tiles.lib()
    win = (0, 0, H, W) if win is None else win
    rect = full_rect(H, W, T, O) if rect is None else rect
    y0, x0, h, w = win
    ref_chw = GT.image(H, W, seed=7) if ref_chw is None else ref_chw
    want = TC.stitch(x, H, W, T, O, rounding, "chw", window=win)
    su, sf = TC.sums(x, H, W, T, O, rounding, ref_chw, "chw", window=win)
    xr = np.ascontiguousarray(x[rect_index(TC.grid(H, W, T, O)[1], rect)])
    bits = None
    for wide in paths:
        layout = "hwc" if wide else "chw"
        xv = GT.float_tiles(xr, "contiguous" if wide else "odd")
        ref = GT.window_of(GT.u8_tensor(GT.in_layout(ref_chw, "chw"), "chw", 0, pad4=True), "chw", win)
        buf, dst = GT.poisoned_destination(h, w, layout, x0, True)
        case = ("tiles", H, W, T, O, rounding, win, rect, wide, note)
        assert tiles.plan(tiles.STITCH, dst, layout, xv, x0, ref, "chw") is wide, case
        rc, sums = GT.stitch_raw(L, xv, H, W, O, rect, win, tiles.ROUNDINGS[rounding], dst, layout, ref, "chw", T=T)
        assert rc == 0, case
        assert torch.equal(dst, torch.from_numpy(GT.in_layout(want, layout)).to(DEV)), case
        dst.fill_(GT.POISON)
        assert (buf == GT.POISON).all(), case
        hs = sums.cpu()
        assert hs[0].tolist() == su, case
        got_f = hs[1].view(torch.float64)
        for c in range(3):
            assert abs(got_f[c].item() - sf[c]) <= h * w * 2.0 ** -53 * sf[c], (case, c, got_f[c].item(), sf[c])
        bits = hs[1].clone() if bits is None else bits
        assert torch.equal(hs[1], bits), case                              # the same bits on both paths


def check_frame_tiles(x, H, W, T, O, fmt, win=None, rect=None, paths=PATHS, matrix=BC.MATRIX, rng=BC.RANGE, note=None):
    win = (0, 0, H, W) if win is None else win
    rect = full_rect(H, W, T, O) if rect is None else rect
    y0, x0, h, w = win
    assert GC.admissible(H, W, win)
    ref = FC.random_frame(1, H, W, fmt, seed=H + W + O)
    want = GC.stitch(x, H, W, T, O, fmt, matrix, rng, window=win)
    want_sums = GC.sums(x, H, W, T, O, fmt, matrix, rng, ref, window=win)
    xr = np.ascontiguousarray(x[rect_index(TC.grid(H, W, T, O)[1], rect)])
    for wide in paths:
        mode = "pad4" if wide else "loose"
        xv = GT.float_tiles(xr, "contiguous" if wide else "odd")
        dstv = GF.frame_views(fmt, h, w, x0 % 8, mode)
        refv = GF.frame_views(fmt, h, w, x0 % 8, mode, GF.window_frame(ref, fmt, win))
        rc, got_wide, sse, ws, need = GF.stitch_raw(xv, fmt, matrix, rng, H, W, O, rect, win, dstv, refv, T=T)
        case = ("frame_tiles", H, W, T, O, fmt, matrix, rng, win, rect, wide, note)
        assert rc == 0 and got_wide == int(wide), case
        GF.check_planes(dstv, want, case)
        GF.check_sums(sse, ws, want_sums, need)


def check_chroma_tiles(x, H, W, T, O, fmt, siting, win=None, rect=None, paths=PATHS, matrix=BC.MATRIX, rng=BC.RANGE, note=None):
    win = (0, 0, H, W) if win is None else win
    rect = full_rect(H, W, T, O) if rect is None else rect
    y0, x0, h, w = win
    assert KC.admissible(H, W, fmt, win)
    ref = CC.random_frame(1, H, W, fmt, seed=H + W + O, garbage=True)
    want = KC.stitch(x, H, W, T, O, fmt, matrix, rng, siting, window=win)
    want_sums = KC.sums(x, H, W, T, O, fmt, matrix, rng, siting, ref, window=win)
    xr = np.ascontiguousarray(x[rect_index(TC.grid(H, W, T, O)[1], rect)])
    for wide in paths:
        xv = GT.float_tiles(xr, "contiguous" if wide else "odd")
        dstv = GK.frame_views(fmt, h, w, x0 % 8, wide)
        refv = GK.frame_views(fmt, h, w, x0 % 8, wide, GK.window_frame(ref, fmt, win))
        rc, got_wide, sse, ws, need = GK.stitch_raw(xv, fmt, matrix, rng, siting, H, W, O, rect, win, dstv, refv, tile=T)
        case = ("chroma_tiles", H, W, T, O, fmt, siting, matrix, rng, win, rect, wide, note)
        assert rc == 0 and got_wide == int(wide), case
        GK.check_planes(dstv, want, case)
        GK.check_sums(sse, ws, want_sums, need)


def check(lib, param, x, H, W, T, O, **kw):
    if lib == "tiles":
        check_tiles(x, H, W, T, O, param, **kw)
    elif lib == "frame_tiles":
        check_frame_tiles(x, H, W, T, O, param, **kw)
    else:
        check_chroma_tiles(x, H, W, T, O, param, BC.SITING[param], **kw)


# -- the witness sets ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lib,param,q", BC.LIBRARIES)
@pytest.mark.parametrize("TO", BC.OVERLAPS)
def test_the_witness_sets_are_the_restatement_exactly(TO, lib, param, q):
    """every band set (either axis, either tile of the band, every round) and both corner sets, whole pictures, both paths: a weight
    one ulp off in either direction, an unrounded product wy * wx or an unfused multiply-add changes a code of these sets in every
    inexact band coordinate (tests/test_band_weights_host.py), so any of them in the kernel fails here"""
    T, O = TO
    for axis, side, r, x, H, W in BC.band_sets(T, O, q):
        check(lib, param, x, H, W, T, O, note=("band", axis, side, r))
    for kind in BC.CORNER_KINDS:
        x, H, W = BC.corner_set(T, O, q, kind)
        check(lib, param, x, H, W, T, O, note=("corner", kind))


@pytest.mark.parametrize("TO", BC.OVERLAPS)
def test_one_row_windows_of_the_band_carry_the_weight_in_their_float_sum(TO):
    """`tiles` alone has a float sum: against an all-zero reference sse_f = sum m^2 over the window.  A window of one band row
    (column) holds one weight: were it one ulp off, every term would move by about 2^-23 relative, the bound is w * 2^-53 relative.
    Every band coordinate of either tile of the band, including those of O = 96 whose small weights leave few codes to tie on."""
    T, O = TO
    S = T - O
    for axis in (0, 1):
        for side in (0, 1):
            x, H, W = BC.band_set(T, O, "nearest", axis, side, 0)
            zero = np.zeros((3, H, W), np.uint8)
            for u in range(O):
                win = (S + u, 0, 1, W) if axis == 0 else (0, S + u, H, 1)
                check_tiles(x, H, W, T, O, "nearest", win, paths=(u % 2 == 0,), ref_chw=zero, note=("row", axis, side, u))


# -- hostile tiles at the new overlaps ---------------------------------------------------------------------------------------------------

CHROMA_SHAPES = [("nv12", "centre"), ("i010", "topleft"), ("nv16", "left"), ("p410", "centre")]
SETTINGS = [("bt601", "limited"), ("bt2020", "full"), ("bt709", "limited")]


@pytest.mark.parametrize("case", BC.hostile_cases())
def test_hostile_tiles_at_the_new_overlaps(case):
    """NaN, +-inf, -0.0, denormals, ties and values outside [0, 1] under weights that are no floats: the whole picture on both paths,
    a window that starts inside a band and one that ends on the picture's last row and column, each from the whole grid on one path
    and from the smallest rectangle that holds it on the other; limited range included"""
    T, O, H, W = case
    ny, nx = TC.grid(H, W, T, O)
    x = TC.hostile_tiles(ny * nx, T, seed=H + W + O)
    configs = [("tiles", r, None) for r in ("nearest", "trunc")] + [("frame_tiles", f, None) for f in FC.FORMATS] + \
              [("chroma_tiles", f, s) for f, s in CHROMA_SHAPES]
    for n, (lib, param, siting) in enumerate(configs):
        sx, sy = (1, 1) if lib == "tiles" else (2, 2) if lib == "frame_tiles" else CC.sub(param)
        matrix, rng = SETTINGS[(n + O // 4) % 3]
        for k, win in enumerate(BC.hostile_windows(T, O, H, W, sx, sy)):
            if lib == "chroma_tiles":
                small = KC.covering(H, W, T, O, KC.halo_window(param, siting, win))
            else:
                small = KC.covering(H, W, T, O, win)
            runs = [(None, PATHS)] if k == 0 else [(None, (k == 1,)), (small, (k != 1,))]
            for rect, paths in runs:
                kw = dict(win=win, rect=rect, paths=paths, note=("hostile", k))
                if lib == "tiles":
                    check_tiles(x, H, W, T, O, param, **kw)
                elif lib == "frame_tiles":
                    check_frame_tiles(x, H, W, T, O, param, matrix=matrix, rng=rng, **kw)
                else:
                    check_chroma_tiles(x, H, W, T, O, param, siting, matrix=matrix, rng=rng, **kw)


# -- the halo pixel of the co-sited filter (blend_px) inside a band --------------------------------------------------------------------

#: O -> lit luma columns X inside a band with X + 1 on an item boundary (a multiple of 8): the item's first chroma sample reads X
#: through blend_px; and rows Y = 2i - 1 inside the band
LIT = {12: dict(cols=[55, 63, 111], rows=[53, 55, 63]), 28: dict(cols=[39, 47, 55, 79], rows=[37, 47, 55, 61])}


@pytest.mark.parametrize("fmt,siting", [("nv12", "left"), ("nv16", "left"), ("p210", "topleft"), ("i010", "topleft")])
def test_a_lit_column_inside_a_band_at_an_item_boundary_reaches_the_sample_right_of_it(fmt, siting):
    """tests/test_gpu_chroma_tiles.py's lit-column case at O = 12 and 28: the column is blue in ONE of its two tiles, so the halo
    pixel's value is that tile's band weight times blue plus the other's times gray.  Whole frame, and windows that start on X + 1.
    (One-ulp sensitivity is not claimed for this path: equality with the restatement is.)"""
    co = CC.levels(fmt, "limited")[2]
    sx, sy = CC.sub(fmt)
    n = 0
    for O, lit in LIT.items():
        S = GK.T - O
        for X in lit["cols"]:
            assert (X + 1) % 8 == 0 and len(TC.covering(X, GK.W1, GK.T, O)) == 2
            for which in (0, -1):
                x, ny, nx = GK.gray_tiles(O)
                GK.light(x, nx, O, 1, X, which)
                aligned, variant = n % 2 == 0, ("contiguous", "odd", "loose4")[n % 3]
                n += 1
                want = GK.halo_case(x, nx, O, fmt, siting, (0, 0, GK.H1, GK.W1), aligned, variant, ("column", X, which))
                cb = CC.codes(want, fmt)[1][0]
                assert (cb[:, (X + 1) // 2] != co).all() and (cb[:, (X - 1) // 2] != co).all()
                assert (np.delete(cb, [(X - 1) // 2, (X + 1) // 2], axis=1) == co).all(), (fmt, siting, O, X)
                for y0, h, w in [(0, GK.H1, GK.W1 - X - 1), (S + sy, 2 * sy, 2 * sx)]:      # the second: inside the horizontal band, too
                    win = (y0, X + 1, h, w)
                    assert KC.admissible(GK.H1, GK.W1, fmt, win)
                    want = GK.halo_case(x, nx, O, fmt, siting, win, n % 2 == 0, ("contiguous", "odd", "loose4")[n % 3], "window")
                    n += 1
                    assert (CC.codes(want, fmt)[1][0][:, 0] != co).all()
                    clamped = KC.stitch_codes(x, GK.H1, GK.W1, GK.T, O, fmt, "bt709", "limited", siting, window=win, frame_edges=False)
                    assert (clamped[1][0][:, 0] == co).all()


@pytest.mark.parametrize("fmt", ["nv12", "p010"])
def test_a_lit_row_inside_a_band_reaches_the_sample_below_it(fmt):
    siting = "topleft"
    co = CC.levels(fmt, "limited")[2]
    n = 0
    for O, lit in LIT.items():
        for Y in lit["rows"]:
            assert Y % 2 == 1 and len(TC.covering(Y, GK.H1, GK.T, O)) == 2
            for which in (0, -1):
                x, ny, nx = GK.gray_tiles(O)
                GK.light(x, nx, O, 0, Y, which)
                aligned, variant = n % 2 == 0, ("contiguous", "odd", "loose4")[n % 3]
                n += 1
                want = GK.halo_case(x, nx, O, fmt, siting, (0, 0, GK.H1, GK.W1), aligned, variant, ("row", Y, which))
                cb = CC.codes(want, fmt)[1][0]
                assert (cb[(Y + 1) // 2] != co).all() and (cb[(Y - 1) // 2] != co).all()
                assert (np.delete(cb, [(Y - 1) // 2, (Y + 1) // 2], axis=0) == co).all(), (fmt, O, Y)
                for x0, h, w in [(0, GK.H1 - Y - 1, GK.W1), (GK.T - O + 2, 4, 6)]:
                    win = (Y + 1, x0, h, w)
                    want = GK.halo_case(x, nx, O, fmt, siting, win, n % 2 == 0, ("contiguous", "odd", "loose4")[n % 3], "window")
                    n += 1
                    assert (CC.codes(want, fmt)[1][0][0] != co).all()
                    clamped = KC.stitch_codes(x, GK.H1, GK.W1, GK.T, O, fmt, "bt709", "limited", siting, window=win, frame_edges=False)
                    assert (clamped[1][0][0] == co).all()


# -- "the bits are the same": the float32 quotient of pc_chroma_tiles.hip and the rounded double quotient of pc_frame_tiles.hip --------

@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_centre_sited_420_is_frame_tiles_on_the_device_where_the_weights_are_no_floats(fmt):
    """the two libraries divide differently and must give the same planes and sums: on the witness sets of their luma quantiser, on
    the corner sets and on hostile tiles, at O = 12, 24 and 28"""
    from progressivecodec_amd import chroma_tiles, frame_tiles
    q = "y10" if fmt == "p010" else "y8"
    T = 64
    for O in (12, 24, 28):
        sets = [(x, H, W) for _, _, _, x, H, W in BC.band_sets(T, O, q)] + [BC.corner_set(T, O, q, kind) for kind in BC.CORNER_KINDS]
        ny, nx = TC.grid(100, 150, T, O)
        sets.append((TC.hostile_tiles(ny * nx, T, seed=O), 100, 150))
        for n, (x_np, H, W) in enumerate(sets):
            f = FC.random_frame(1, H, W, fmt, seed=n)
            planes = tuple(torch.from_numpy(p[0]).to(DEV) for p in f)
            ga, gb = chroma_tiles.grid_of(H, W, T, O), frame_tiles.grid_of(H, W, T, O)
            x = torch.from_numpy(np.array(x_np)).to(DEV)
            S = T - O
            for win in [None, (S + 2, S - 2 if W > T else 2, min(O + 4, H - S - 2), 10)]:
                if win is not None and not GC.admissible(H, W, win):
                    continue
                pa, da = chroma_tiles.stitch_frame(x, ga, fmt, "bt709", "full", window=win, ref=planes)
                pb, db = frame_tiles.stitch_frame(x, gb, fmt, "bt709", "full", window=win, ref=planes)
                assert all(torch.equal(p, r) for p, r in zip(pa, pb)) and torch.equal(da.sse, db.sse), (fmt, O, n, win)
        f = FC.random_frame(1, 100, 150, fmt, seed=3)
        planes = tuple(torch.from_numpy(p[0]).to(DEV) for p in f)
        a, ga = chroma_tiles.cut_frame(planes, fmt, "bt601", "full", "linear", "centre", tile=T, overlap=O)
        b, gb = frame_tiles.cut_frame(planes, fmt, "bt601", "full", "linear", tile=T, overlap=O)
        assert ga == gb and torch.equal(a.view(torch.int32), b.view(torch.int32))

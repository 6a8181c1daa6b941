"""GPU tests of tiled coding of YUV frames of any subsampling and siting (progressivecodec_amd/chroma_tiles.py, libpc_chroma_tiles.so)
against the restatement tests/chroma_tiles_contract.py.  Exact equality throughout: cut tiles bit for bit,
planes and sums as integers.

T = 64 throughout.  The matrix is tests/chroma_tiles_cases.py's table (every case asserts the access path the table predicts); the
halo cases light one luma column or row in ONE tile and look at the chroma sample next to it; the rest are the two paths on the same
data, frame_tiles on the device, the large sums and the codec.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from progressivecodec_amd import chroma_tiles
from tests import chroma_contract as CC
from tests import chroma_tiles_cases as CS
from tests import chroma_tiles_contract as KC
from tests import frames_contract as FC
from tests import tiles_contract as TC
from tests.test_gpu_frames import POISON64, View, same_bits
from tests.test_gpu_tiles import float_tiles
from tests.util import gpu_codec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POL = "point-based-std"
T = CS.T


def KT():
    return chroma_tiles


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def frame_views(fmt, H, W, back=0, aligned=True, data=None):
    """The planes of one frame as Views.  back: the luma columns the frame's first sample lies past an aligned address (the window's
    x0 % 8, so that frame column 8 * floor(x0 / 8) is the aligned one: what the wide path of the stitch needs); the chroma planes lie
    2 * back / sx (semi-planar) or back / sx (planar) elements in.  Not aligned: odd offsets and row strides that are no multiples
    of 4."""
    semi, n, _, sx, _ = CC.FORMATS[fmt]
    Hc, Wc = CC.chroma_size(H, W, fmt)
    dt = np.uint16 if n == 10 else np.uint8
    shapes = [(1, H, W), (1, Hc, Wc, 2)] if semi else [(1, H, W), (1, Hc, Wc), (1, Hc, Wc)]
    odd = 0 if aligned else 1
    cback = 2 * back // sx if semi else back // sx
    offs = [back + odd] + [cback + odd] * (len(shapes) - 1)
    mode = "pad4" if aligned else "loose"
    return [View(s, dt, o, mode, None if data is None else data[i]) for i, (s, o) in enumerate(zip(shapes, offs))]


def struct_of(views):
    from progressivecodec_amd import frames
    return frames._frame_struct([v.t for v in views])


def cut_raw(views, fmt, matrix, rng, up, siting, H, W, O, rect, dst_offset=0, tile=T):
    """pc_chroma_tiles_cut into a NaN-poisoned buffer with guard floats on both sides -> (status, wide as pc_chroma_tiles_plan reports
    it, the [n,3,T,T] result, whether the guards kept their bits)"""
    from progressivecodec_amd import chroma, frames
    kt = KT()
    L = kt.lib()
    k = frames.coefficients(matrix)
    f, (hs, vs) = chroma.FORMATS[fmt], chroma.SITINGS[siting]
    n = rect[2] * rect[3] * 3 * tile * tile
    buf = torch.full((4 + dst_offset + n + 4,), float("nan"), dtype=torch.float32, device=DEV)
    dst = buf[4 + dst_offset:4 + dst_offset + n]
    src = struct_of(views)
    wide = C.c_int(-1)
    assert L.pc_chroma_tiles_plan(kt.CUT, f.layout, f.bits, f.sx, C.byref(src), dst.data_ptr(), 3 * tile * tile, tile * tile, tile, O, 0, None,
                                  C.byref(wide)) == 0
    rc = L.pc_chroma_tiles_cut(C.byref(src), *f, hs, vs, frames.RANGES[rng], frames.UPSAMPLES[up], k.a, k.b, k.c, k.d, H, W, tile, O, *rect,
                               dst.data_ptr(), stream())
    h = buf.cpu().numpy()
    guards = bool(np.isnan(h[:4 + dst_offset]).all() and np.isnan(h[4 + dst_offset + n:]).all())
    return rc, wide.value, h[4 + dst_offset:4 + dst_offset + n].reshape(-1, 3, tile, tile), guards


def stitch_raw(xv, fmt, matrix, rng, siting, H, W, O, rect, win, dst_views, ref_views, tile=T):
    """pc_chroma_tiles_stitch -> (status, wide, the [3,3] sums buffer whose middle row is `sse`, poisoned beforehand, the workspace
    with one more word than needed, the bytes needed)"""
    from progressivecodec_amd import chroma, frames
    kt = KT()
    L = kt.lib()
    k = frames.coefficients(matrix)
    f, (hs, vs) = chroma.FORMATS[fmt], chroma.SITINGS[siting]
    y0, x0, h, w = win
    dst = struct_of(dst_views) if dst_views is not None else None
    ref = struct_of(ref_views) if ref_views is not None else None
    need = L.pc_chroma_tiles_stitch_workspace_size(x0, h, w, f.sy)
    assert need == 24 * -(-(-(-h // f.sy) * (-(-(x0 + w) // 8) - x0 // 8)) // 256)
    ws = torch.full((max(1, need // 8) + 1,), POISON64, dtype=torch.int64, device=DEV)
    sse = torch.full((3, 3), POISON64, dtype=torch.int64, device=DEV)
    wide = C.c_int(-1)
    pd, pr = (C.byref(dst) if dst is not None else None), (C.byref(ref) if ref is not None else None)
    assert L.pc_chroma_tiles_plan(kt.STITCH, f.layout, f.bits, f.sx, pd, xv.data_ptr(), xv.stride(0), xv.stride(1), xv.stride(2), O, x0, pr,
                                  C.byref(wide)) == 0
    rc = L.pc_chroma_tiles_stitch(xv.data_ptr(), xv.stride(0), xv.stride(1), xv.stride(2), H, W, tile, O, *rect, y0, x0, h, w, *f, hs, vs,
                                  frames.RANGES[rng], k.kr, k.kg, k.kb, k.ib, k.ir, pd, pr, ws.data_ptr() if ref is not None else None,
                                  need if ref is not None else 0, sse[1].data_ptr() if ref is not None else None, stream())
    return rc, wide.value, sse.cpu(), ws.cpu(), need


def check_sums(sse, ws, want, need):
    assert sse[0].tolist() == [POISON64] * 3 and sse[2].tolist() == [POISON64] * 3              # the guard words keep their bits
    assert sse[1].tolist() == want
    assert ws[-1].item() == POISON64 and (ws[:need // 8] != POISON64).all()                     # every partial written, none beyond


def check_planes(views, want, case):
    for v, w in zip(views, want):
        got, clean = v.read()
        assert clean and np.array_equal(got, w), case


def window_frame(f, fmt, win):
    """the window of a whole frame of tests/chroma_contract.py, as a frame"""
    return CC.frame(*KC.crop_codes(CC.codes(f, fmt), fmt, win), fmt)


def rect_tiles(x, nx, rect):
    return x[[(rect[0] + a) * nx + rect[1] + b for a in range(rect[2]) for b in range(rect[3])]]


# -- the matrix ----------------------------------------------------------------------------------------------------------------------

def run_matrix(cases):
    """every case: the cut under its upsamplers against the restatement bit for bit, and the stitch of hostile tiles (NaN, +-inf,
    values outside [0, 1]) against a reference with random bits outside its 10-bit codes, with image, with sums, with sums alone"""
    for c in cases:
        H, W, O = c.H, c.W, c.O
        ny, nx = TC.grid(H, W, T, O)
        rect = (0, 0, ny, nx)
        f = CC.random_frame(1, H, W, c.fmt, seed=1000 * H + W + c.n, garbage=True)
        for up in c.ups:
            rc, wide, got, guards = cut_raw(frame_views(c.fmt, H, W, 0, c.aligned, f), c.fmt, c.matrix, c.rng, up, c.siting, H, W, O, rect,
                                            c.dst_offset)
            assert rc == 0 and guards, (c, up)
            assert wide == int(CS.cut_wide(c)), c
            assert not np.isnan(got).any() and same_bits(got, KC.cut(f, c.fmt, c.matrix, c.rng, up, c.siting, T, O)), (c, up)
        x = TC.hostile_tiles(ny * nx, T, seed=77 * H + W + c.n)
        xv = float_tiles(x, c.variant)
        win = (0, 0, H, W)
        want = KC.stitch(x, H, W, T, O, c.fmt, c.matrix, c.rng, c.siting)
        want_sums = KC.sums(x, H, W, T, O, c.fmt, c.matrix, c.rng, c.siting, f)
        refv = frame_views(c.fmt, H, W, 0, c.aligned, f)
        for with_image, with_ref in c.emits:
            dstv = frame_views(c.fmt, H, W, 0, c.aligned) if with_image else None
            rc, wide, sse, ws, need = stitch_raw(xv, c.fmt, c.matrix, c.rng, c.siting, H, W, O, rect, win, dstv, refv if with_ref else None)
            assert rc == 0, c
            assert wide == int(CS.stitch_wide(c)), c
            if with_ref:
                check_sums(sse, ws, want_sums, need)
            else:
                assert (sse == POISON64).all() and (ws == POISON64).all(), c
            if with_image:
                check_planes(dstv, want, c)


@pytest.mark.parametrize("fmt", sorted(CC.FORMATS))
def test_every_format_and_siting_is_the_restatement_exactly(fmt):
    run_matrix(CS.main_cases(fmt))


@pytest.mark.parametrize("fmt", CS.OTHER_FORMATS)
def test_the_other_sizes_overlaps_matrices_and_full_range(fmt):
    run_matrix(CS.other_cases(fmt))


# -- the halo ------------------------------------------------------------------------------------------------------------------------

H1, W1 = 100, 150


def gray_tiles(O):
    ny, nx = TC.grid(H1, W1, T, O)
    return np.full((ny * nx, 3, T, T), 0.5, np.float32), ny, nx


def light(x, nx, O, axis, p, which):
    """paint frame column (axis 1) or row (axis 0) p blue in ONE of the tiles that cover it along that axis (`which`: 0 the first,
    -1 the last), in every tile along the other axis"""
    S = T - O
    L = (H1, W1)[axis]
    i = TC.covering(p, L, T, O)[which]
    for t in range(x.shape[0]):
        ty, tx = divmod(t, nx)
        if (ty, tx)[axis] == i:
            idx = [t, slice(None), slice(None), slice(None)]
            idx[2 + axis] = p - i * S
            x[tuple(idx)] = np.array([0.0, 0.0, 1.0], np.float32)[:, None]


def heavier(p, axis, O):
    """which of the tiles covering p along the axis weighs it with at least 1/2: 0 the first, -1 the last"""
    cover = TC.covering(p, (H1, W1)[axis], T, O)
    return -1 if len(cover) == 1 or 2 * (p - cover[-1] * (T - O)) >= O else 0


def halo_case(x, nx, O, fmt, siting, win, aligned, variant, note, H=H1, W=W1):
    """one stitch of `win` of the H x W frame from the smallest rectangle the halo rule allows, against the restatement"""
    rect = KC.covering(H, W, T, O, KC.halo_window(fmt, siting, win))
    want = KC.stitch(x, H, W, T, O, fmt, "bt709", "limited", siting, window=win)
    ref = CC.random_frame(1, H, W, fmt, seed=5)
    want_sums = KC.sums(x, H, W, T, O, fmt, "bt709", "limited", siting, ref, window=win)
    xv = float_tiles(rect_tiles(x, nx, rect), variant)
    back = win[1] % 8
    dstv = frame_views(fmt, win[2], win[3], back, aligned)
    refv = frame_views(fmt, win[2], win[3], back, aligned, window_frame(ref, fmt, win))
    rc, wide, sse, ws, need = stitch_raw(xv, fmt, "bt709", "limited", siting, H, W, O, rect, win, dstv, refv)
    case = (fmt, siting, O, win, rect, aligned, variant, note)
    assert rc == 0 and wide == int(aligned and variant != "odd"), case
    check_planes(dstv, want, case)
    check_sums(sse, ws, want_sums, need)
    return want


@pytest.mark.parametrize("fmt,siting", [("nv12", "left"), ("nv12", "topleft"), ("nv16", "left"), ("i010", "topleft"), ("p210", "topleft")])
def test_a_lit_column_left_of_a_chroma_sample_reaches_it_and_no_other(fmt, siting):
    """gray tiles in which one luma column is blue in one tile only: it is the sole input of chroma sample (X + 1) / 2 that is not
    gray.  Columns: an item boundary, a block boundary (item 256 of the whole frame is row 13 / 26, columns 72 ..), a tile origin at
    O = 0, inside a band at O = 4 and 32, left of the partial last item; then windows whose first column is X + 1, for
    x0 = 0, 2, 4, 6 (mod 8), from the rectangle that covers the halo-extended window alone"""
    co = CC.levels(fmt, "limited")[2]
    sx, sy = CC.sub(fmt)
    n = 0
    for O in (0, 4, 32):
        S = T - O
        band = {0: [], 4: [S + 1], 32: [S + 1, S + 7, 2 * S + 3]}[O]
        for X in [7, 71, S - 1, 143] + band:
            for which in (0, -1):
                x, ny, nx = gray_tiles(O)
                light(x, nx, O, 1, X, which)
                aligned, variant = n % 2 == 0, ("contiguous", "odd", "loose4")[n % 3]
                n += 1
                want = halo_case(x, nx, O, fmt, siting, (0, 0, H1, W1), aligned, variant, ("column", X, which))
                cb = CC.codes(want, fmt)[1][0]
                assert (cb[:, (X + 1) // 2] != co).all() and (cb[:, (X - 1) // 2] != co).all()      # the sample right of X and X's own
                others = np.delete(cb, [(X - 1) // 2, (X + 1) // 2], axis=1)
                assert (others == co).all(), (fmt, siting, O, X)
        for x0 in (S, 64, 66, 68, 70, 8, 130):
            x, ny, nx = gray_tiles(O)
            light(x, nx, O, 1, x0 - 1, heavier(x0 - 1, 1, O))
            for y0, h, w in [(0, H1, W1 - x0), (sy * 7, 2 * sy, 2 * sx), (H1 - 1 - (H1 - 1) % sy, 1 + (H1 - 1) % sy, 14)]:
                win = (y0, x0, h, w)
                assert KC.admissible(H1, W1, fmt, win)
                aligned, variant = n % 2 == 0, ("contiguous", "odd", "loose4")[n % 3]
                n += 1
                want = halo_case(x, nx, O, fmt, siting, win, aligned, variant, "window")
                assert (CC.codes(want, fmt)[1][0][:, 0] != co).all()
                # a stitch that clamped its filter at the window's edge would not see the column
                clamped = KC.stitch_codes(x, H1, W1, T, O, fmt, "bt709", "limited", siting, window=win, frame_edges=False)
                assert (clamped[1][0][:, 0] == co).all()


@pytest.mark.parametrize("fmt", ["nv12", "i010", "p010"])
def test_a_lit_row_above_a_chroma_sample_reaches_it_and_no_other(fmt):
    """the same along columns, under "topleft": rows 2i - 1 at a block boundary, a tile origin, inside a band, and above a window"""
    siting = "topleft"
    co = CC.levels(fmt, "limited")[2]
    n = 0
    for O in (0, 4, 32):
        S = T - O
        band = {0: [], 4: [S + 1], 32: [S + 1, S + 7]}[O]
        for Y in [25, S - 1, 97] + band:
            for which in (0, -1):
                x, ny, nx = gray_tiles(O)
                light(x, nx, O, 0, Y, which)
                aligned, variant = n % 2 == 0, ("contiguous", "odd", "loose4")[n % 3]
                n += 1
                want = halo_case(x, nx, O, fmt, siting, (0, 0, H1, W1), aligned, variant, ("row", Y, which))
                cb = CC.codes(want, fmt)[1][0]
                assert (cb[(Y + 1) // 2] != co).all() and (cb[(Y - 1) // 2] != co).all()
                assert (np.delete(cb, [(Y - 1) // 2, (Y + 1) // 2], axis=0) == co).all(), (fmt, O, Y)
        for y0 in (S, 66, 26):
            x, ny, nx = gray_tiles(O)
            light(x, nx, O, 0, y0 - 1, heavier(y0 - 1, 0, O))
            for x0, h, w in [(0, H1 - y0, W1), (S, 4, 6), (70, 2, W1 - 70)]:
                win = (y0, x0, h, w)
                aligned, variant = n % 2 == 0, ("contiguous", "odd", "loose4")[n % 3]
                n += 1
                want = halo_case(x, nx, O, fmt, siting, win, aligned, variant, "window")
                assert (CC.codes(want, fmt)[1][0][0] != co).all()
                clamped = KC.stitch_codes(x, H1, W1, T, O, fmt, "bt709", "limited", siting, window=win, frame_edges=False)
                assert (clamped[1][0][0] == co).all()


@pytest.mark.parametrize("fmt,siting", [("nv12", "left"), ("nv12", "topleft"), ("i010", "topleft"), ("nv16", "left"), ("p210", "topleft")])
def test_windows_that_end_on_an_odd_edge_under_a_halo(fmt, siting):
    """a 99 x 131 frame: a window with x0 > 0 and y0 > 0 that ends on the odd last row and column has, in one item, a halo column or
    row, a missing second row and a missing right neighbour; hostile tiles, every overlap, both paths, window starts at
    x0 = 0, 2, 4, 6 (mod 8), from the rectangle that covers the halo-extended window alone"""
    H, W = 99, 131
    sx, sy = CC.sub(fmt)
    n = 0
    for O in (0, 4, 32):
        S = T - O
        ny, nx = TC.grid(H, W, T, O)
        x = TC.hostile_tiles(ny * nx, T, seed=O + len(fmt))
        for y0, x0 in [(S, S), (2 * sy, 66), (S + 2 * sy, 68), (H - 1 - (H - 1) % sy, 70), (0, 122), (S, 0)]:
            win = (y0, x0, H - y0, W - x0)
            assert KC.admissible(H, W, fmt, win) and ((H - y0) % sy or sy == 1) and (W - x0) % sx
            aligned, variant = n % 2 == 0, ("contiguous", "odd", "loose4")[n % 3]
            n += 1
            halo_case(x, nx, O, fmt, siting, win, aligned, variant, "odd edge", H, W)


def test_the_rectangle_must_hold_the_halo():
    """x0 = S at O = 0: the window's own tiles do not do under "left" at 4:2:0; they do under "centre" and at 4:4:4"""
    kt = KT()
    from progressivecodec_amd import tiles
    O, win = 0, (0, 64, 64, 64)
    x, ny, nx = gray_tiles(O)
    g = tiles.grid_of(H1, W1, T, O)
    own = g.covering(win)
    assert own == (0, 1, 1, 1) and kt.covering(g, win, "nv12", "left") == (0, 0, 1, 2) and kt.covering(g, win, "i444", "left") == own
    xt = torch.from_numpy(rect_tiles(x, nx, own)).to(DEV)
    with pytest.raises(ValueError, match="halo"):
        kt.stitch_frame(xt, g.with_rect(own), "nv12", siting="left", window=win)
    dstv = frame_views("nv12", 64, 64)
    assert stitch_raw(xt, "nv12", "bt709", "limited", "left", H1, W1, O, own, win, dstv, None)[0] == -1
    assert kt.lib().pc_chroma_tiles_last_hip_error() == 0 and all(v.read()[1] for v in dstv)
    for fmt, siting in [("nv12", "centre"), ("i444", "left"), ("i444", "topleft")]:
        got = kt.stitch_frame(xt, g.with_rect(own), fmt, siting=siting, window=win)
        want = KC.stitch(x, H1, W1, T, O, fmt, "bt709", "limited", siting, window=win)
        assert all(np.array_equal(a.cpu().numpy(), b[0]) for a, b in zip(got, want)), (fmt, siting)


# -- frame_tiles on the device -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_centre_sited_420_is_frame_tiles_on_the_device(fmt):
    from progressivecodec_amd import frame_tiles
    kt = KT()
    H, W = 100, 150
    f = FC.random_frame(1, H, W, fmt, seed=3)
    planes = tuple(torch.from_numpy(p[0]).to(DEV) for p in f)
    for O in (0, 4, 16):
        a, ga = kt.cut_frame(planes, fmt, "bt601", "full", "linear", "centre", tile=T, overlap=O)
        b, gb = frame_tiles.cut_frame(planes, fmt, "bt601", "full", "linear", tile=T, overlap=O)
        assert ga == gb and torch.equal(a.view(torch.int32), b.view(torch.int32))
        x = torch.from_numpy(TC.hostile_tiles(ga.n, T, seed=O)).to(DEV)
        for win in [None, (2, 66, 40, 30), (98, 148, 2, 2)]:
            (pa, da), (pb, db) = kt.stitch_frame(x, ga, fmt, "bt601", "full", window=win, ref=planes), \
                frame_tiles.stitch_frame(x, gb, fmt, "bt601", "full", window=win, ref=planes)
            assert all(torch.equal(p, q) for p, q in zip(pa, pb)) and torch.equal(da.sse, db.sse), (fmt, O, win)


# -- both paths on the same data -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,siting", [("nv16", "left"), ("p210", "topleft"), ("i444", "centre"), ("nv12", "topleft"), ("i010", "left")])
def test_wide_and_narrow_agree_on_the_same_data(fmt, siting):
    """one frame and one tile set under every alignment: aligned, pitched and offset planes; aligned, strided and misaligned tiles"""
    H, W = 65, 150
    sx, sy = CC.sub(fmt)
    f = CC.random_frame(1, H, W, fmt, seed=9, garbage=True)
    for O in (0, 4, 16):
        ny, nx = TC.grid(H, W, T, O)
        rect = (0, 0, ny, nx)
        cuts = {}
        for aligned, dst_offset in [(True, 0), (True, 2), (False, 0), (False, 3)]:
            rc, wide, got, guards = cut_raw(frame_views(fmt, H, W, 0, aligned, f), fmt, "bt2020", "limited", "linear", siting, H, W, O, rect, dst_offset)
            assert rc == 0 and guards and wide == int(aligned and dst_offset == 0 and (sx == 1 or O % 8 == 0))
            cuts[(aligned, dst_offset)] = got
        first = cuts[(True, 0)]
        assert all(same_bits(first, g) for g in cuts.values())
        x = TC.hostile_tiles(ny * nx, T, seed=O)
        seen = set()
        for win in [(0, 0, H, W), (sy * 3, 70, H - sy * 3, 50), (0, 8, 2 * sy, 24)]:
            outs = []
            for aligned in (True, False):
                for variant in ("contiguous", "loose4", "odd"):
                    back = win[1] % 8
                    dstv = frame_views(fmt, win[2], win[3], back, aligned)
                    refv = frame_views(fmt, win[2], win[3], back, aligned, window_frame(f, fmt, win))
                    rc, wide, sse, ws, need = stitch_raw(float_tiles(x, variant), fmt, "bt2020", "limited", siting, H, W, O, rect, win, dstv, refv)
                    assert rc == 0 and wide == int(aligned and variant != "odd")
                    seen.add(wide)
                    outs.append(([v.read()[0] for v in dstv], sse[1].tolist()))
            assert all(o[1] == outs[0][1] and all(np.array_equal(a, b) for a, b in zip(o[0], outs[0][0])) for o in outs), (fmt, O, win)
        assert seen == {0, 1}


# -- large sums ----------------------------------------------------------------------------------------------------------------------

def test_large_sums_reach_the_closed_form_and_the_last_row_counts():
    """one 1026 x 1030 p410 frame in 512-tiles at O = 0: 1026 * 129 = 132354 items, 517 full blocks and one of 2 items, so 518 block
    partials: the final's threads make several trips and the last partial is a nearly empty block's"""
    kt = KT()
    H, W, TT = 1026, 1030, 512
    ny, nx = TC.grid(H, W, TT, 0)
    assert (ny, nx) == (3, 3) and divmod(H * -(-W // 8), 256) == (517, 2)
    assert kt.lib().pc_chroma_tiles_stitch_workspace_size(0, H, W, 1) == 24 * 518
    zeros = tuple(torch.zeros(s, dtype=torch.uint16, device=DEV) for s in [(H, W), (H, W, 2)])
    g = None
    for p, rgb in enumerate([(1.0, 1.0, 1.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)]):
        x = torch.empty((9, 3, TT, TT), dtype=torch.float32, device=DEV)
        for ch in range(3):
            x[:, ch] = rgb[ch]
        g = kt.grid_of(H, W, TT, 0) if g is None else g
        d = kt.stitch_frame(x, g, "p410", "bt709", "full", ref=zeros, image=False)
        assert d.sse.cpu().tolist()[0][p] == 1023 ** 2 * 1026 * 1030 == 1105950916620, p
    # a frame that differs from its reference in the last row alone
    x = torch.full((9, 3, TT, TT), 0.25, dtype=torch.float32, device=DEV)
    frame = kt.stitch_frame(x, g, "p410", "bt709", "full")
    x2 = x.clone()
    x2[6:, :, H - 1 - 2 * TT, :] = 0.75                                     # frame row 1025 is row 1 of the tiles of grid row 2
    d = kt.stitch_frame(x2, g, "p410", "bt709", "full", ref=frame, image=False)
    yq = [int(np.rint(np.float32(v) * np.float32(1023))) for v in (0.25, 0.75)]
    assert d.sse.cpu().tolist()[0] == [(yq[1] - yq[0]) ** 2 * W, 0, 0]


# -- through the codec ---------------------------------------------------------------------------------------------------------------

QUALITIES = [0, 0.5]


@functools.lru_cache(maxsize=None)
def codec_frame(H, W, fmt, siting):
    g = np.random.default_rng(H + W)
    lo = torch.from_numpy(g.uniform(0.1, 0.9, (1, 3, 8, 8)).astype(np.float32))
    x = torch.nn.functional.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False).numpy()
    return CC.emit(x, 0, 0, H, W, fmt, "bt709", "limited", siting)


def on_device(f):
    return tuple(torch.from_numpy(p[0]).to(DEV) for p in f)


def decoded_tiles(inner, n, lv):
    from progressivecodec_amd import container, tiles
    net = gpu_codec()
    hd = tiles.parse_tiled(inner)
    outs = []
    for t in range(n):
        strings, shape, qs, _, pol = container.unpack(tiles.tile_bytes(inner, hd, t)[0], levels=[lv])
        outs.append(net.decompress(strings[0], shape, qs[0], pol)["x_hat"].cpu().numpy()[0])
    return np.stack(outs)


@pytest.mark.parametrize("fmt,siting,hw,O", [("p210", "left", (100, 150), 0), ("i444", "centre", (65, 63), 16)])
def test_encode_and_decode_through_the_codec(fmt, siting, hw, O):
    kt = KT()
    net = gpu_codec()
    H, W = hw
    f = codec_frame(H, W, fmt, siting)
    buf = kt.encode_frame_tiled(net, on_device(f), QUALITIES, fmt, siting=siting, tile=T, overlap=O, mask_pol=POL)
    assert kt.encode_frame_tiled(net, on_device(f), QUALITIES, fmt, siting=siting, tile=T, overlap=O, mask_pol=POL, max_tiles_per_call=1) == buf
    hd = kt.parse_frame_tiled(buf)
    g = hd["tiled"]["grid"]
    assert (hd["fmt"], hd["siting"], hd["H"], hd["W"], g.T, g.O) == (fmt, siting, H, W, T, O)
    x = decoded_tiles(hd["inner"], g.n, 1)
    xt = torch.from_numpy(x).to(DEV)
    S = T - O
    whole = kt.decode_frame_tiled(net, buf)
    assert all(torch.equal(a, b) for a, b in zip(whole, kt.stitch_frame(xt, g, fmt, siting=siting)))
    assert all(np.array_equal(a.cpu().numpy(), b[0]) for a, b in zip(whole, KC.stitch(x, H, W, T, O, fmt, "bt709", "limited", siting)))
    region = (0, S, H, W - S)
    got = kt.decode_frame_tiled(net, buf, region=region)
    want = KC.stitch(x, H, W, T, O, fmt, "bt709", "limited", siting, window=region)
    assert all(np.array_equal(a.cpu().numpy(), b[0]) for a, b in zip(got, want))
    if fmt == "p210":                                             # the 4:2:2 master straight to left-sited NV12, whole and a region
        for reg in (None, (2, S, 40, 20)):
            got = kt.decode_frame_tiled(net, buf, region=reg, fmt="nv12", siting="left")
            want = KC.stitch(x, H, W, T, O, "nv12", "bt709", "limited", "left", window=reg)
            assert got[0].dtype == torch.uint8 and all(np.array_equal(a.cpu().numpy(), b[0]) for a, b in zip(got, want)), reg


def test_a_one_tile_frame_holds_encode_frames_blob_and_pck1_holds_pcg1s_inner_container():
    from progressivecodec_amd import chroma, frame_tiles, tiles
    kt = KT()
    net = gpu_codec()
    f = codec_frame(64, 64, "nv16", "left")
    buf = kt.encode_frame_tiled(net, on_device(f), QUALITIES, "nv16", siting="left", tile=T, overlap=0, mask_pol=POL)
    pch = chroma.encode_frame(net, on_device(f), QUALITIES, "nv16", siting="left", mask_pol=POL)
    hd = kt.parse_frame_tiled(buf)
    assert tiles.tile_bytes(hd["inner"], hd["tiled"], 0)[0] == chroma.parse_frame(pch)["blob"]
    # for centre-sited nv12, i420 and p010 the PCT1 container inside PCK1 is the one inside PCG1, byte for byte
    for fmt in FC.FORMATS:
        f = codec_frame(100, 150, fmt, "centre")
        a = kt.encode_frame_tiled(net, on_device(f), QUALITIES, fmt, tile=T, overlap=16, mask_pol=POL)
        b = frame_tiles.encode_frame_tiled(net, on_device(f), QUALITIES, fmt, tile=T, overlap=16, mask_pol=POL)
        assert kt.parse_frame_tiled(a)["inner"] == frame_tiles.parse_frame_tiled(b)["inner"] and a[:4] == b"PCK1" and b[:4] == b"PCG1", fmt
        assert all(torch.equal(p, q) for p, q in zip(kt.decode_frame_tiled(net, a, level=0), frame_tiles.decode_frame_tiled(net, b, level=0))), fmt

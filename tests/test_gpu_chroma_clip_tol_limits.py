"""chroma_clip_tol (libpc_chroma_clip_tol.so) on the GPU past T = 64 (DESIGN.md section 19.1's row for section 29), at the smallest
shapes that reach each path: the halo ring's loop making its second trip (T = 128) and every side of the ring alone (T = 576);
decide_kernel's gather making 2, 3, 17 and 33 trips over rows of 82, 163, 1025 and 2049 block partials; and the largest sums -- a
2048 x 2048 one-tile i410 pair of all-0 against all-1023 codes, where 32-bit wave sums would overflow if the bounds stated in
pc_chroma_clip_tol.hip were wrong.  The frames and witnesses are tests/chroma_clips_limits.py's where they fit (the item and the ring
lay samples out as section 25's do; tests/test_chroma_clips_limits_host.py holds that table to the restatement).  Every comparison is
exact equality of integers against the restatement (tests/chroma_clip_tol_contract.py) or a closed form; every raw call asserts its
status, that the workspace was written exactly where the call may, and the access path pc_chroma_clip_tol_plan reports."""
import itertools

import numpy as np
import pytest

from tests import chroma_clip_tol_contract as TOL
from tests import chroma_clips_limits as XL
from tests import chroma_contract as CC
from tests import chroma_limits as CL
from tests import tiles_contract as TC
from tests.test_gpu_chroma_clip_tol import CT, check, scan_raw
from tests.test_gpu_chroma_clips import frame_pair, views

pytestmark = pytest.mark.gpu

NO = TOL.NO_MSE
RULES = list(itertools.product(CC.SITINGS, CC.UPSAMPLES))
#: how the frames of a table lie in memory, frame k taking entry k % 2: aligned but pitched differently (wide where O and sx allow);
#: one element past an allocation start with loose rows, next to an aligned one (narrow)
TABLES = {True: (("pad4", 0), ("wider", 0)), False: (("loose", 1), ("pad4", 0))}


def ids(v):
    return "-".join(str(a) for a in v) if isinstance(v, tuple) else str(v)


def device_table(fmt, H, W, clip, aligned):
    return [views(fmt, H, W, *TABLES[aligned][k % 2], f) for k, f in enumerate(clip)]


def run(table, clip, fmt, siting, up, H, W, T, O, aligned, tol=((0, 0, 0), (NO,) * 3, 0), want=None, note=None):
    """one raw scan against the restatement (or `want`) -> the restatement's (source, stats)"""
    ct = CT()
    n = int(np.prod(TC.grid(H, W, T, O)))
    wide = ct.plan(table, fmt, overlap=O)
    assert wide is (aligned and (CC.sub(fmt)[0] == 1 or O % 8 == 0)), (note, aligned)
    want = TOL.scan(clip, fmt, siting, T, O, up, *tol) if want is None else want
    rc, source, stats, ws_ok = scan_raw(table, fmt, siting, up, H, W, O, tol, n, T_=T)
    assert rc == 0 and ws_ok, (note, siting, up, aligned)
    check(source, stats, want, (note, siting, up, aligned))
    return want


def counts(stats_row):
    return [[s[0] for s in tile] for tile in stats_row]


# -- the halo ring -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", XL.RING_SMALL_FORMATS)
def test_ring_second_trip_at_its_smallest_size(fmt):
    """T = 128, tile 4 of 300 x 300: frame 1 differs from frame 0 in the samples the ring's loop reaches from index 256 on; frame 2 is
    frame 0 again, judged against frame 1 where the tile was recoded.  Tile 4 holds them under the rules that have that side"""
    c = XL.RING_SMALL
    H, W, T, O = c["H"], c["W"], c["T"], c["O"]
    cur, prev = XL.ring_small_pair(fmt, "random")
    clip = [prev, cur, prev]
    for aligned in (True, False):
        table = device_table(fmt, H, W, clip, aligned)
        for siting, up in RULES:
            want = run(table, clip, fmt, siting, up, H, W, T, O, aligned, note=fmt)
            expect = XL.ring_small_expect(fmt, siting, up)
            assert counts(want[1][1]) == [expect.get(t, [0, 0, 0]) for t in range(9)] and want[1][1][4][1][0] == (4 if up == "linear" else 0)
            assert want[0][1] == [1 if t in expect and expect[t] != [0, 0, 0] else 0 for t in range(9)] and want[0][2] == [2 * s for s in want[0][1]]
            # the witnesses move by at most three codes: a tolerance of three takes them back in, the evidence stays
            again = run(table, clip, fmt, siting, up, H, W, T, O, aligned, ((3, 3, 3), (NO,) * 3, 0), note=fmt)
            assert again[0] == [[0] * 9] * 3 and again[1][1] == want[1][1]


@pytest.mark.parametrize("side", XL.SIDES)
@pytest.mark.parametrize("fmt", [f for f, _, _ in XL.RING_SIDES_FORMATS])
def test_each_ring_side_alone(fmt, side):
    """T = 576, tile 4 of 1300 x 1300: the frames differ in one side of tile 4's ring alone, in Cb everywhere and in Cr in fewer
    samples; the loop covers up to 1156 (nv12) and 1732 (p210) indices.  Side length or 0 per lo / hi, under every rule"""
    c = XL.RING_SIDES
    H, W, T, O = c["H"], c["W"], c["T"], c["O"]
    cur, prev = XL.ring_side_pair(fmt, side)
    clip = [prev, cur]
    for aligned in (True, False):
        table = device_table(fmt, H, W, clip, aligned)
        for siting, up in RULES:
            want = run(table, clip, fmt, siting, up, H, W, T, O, aligned, note=(fmt, side))
            assert counts(want[1][1])[4] == XL.ring_side_expect(fmt, siting, up, side), (side, siting, up)


# -- the decide kernel's gather ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs", XL.FORMATS, ids=ids)
def test_decide_second_and_third_trip_at_576(fs):
    """601 x 1101 in 576-tiles: 82 block partials per tile at 4:2:0 (two trips of the wave's 64 lanes), 163 at 4:2:2 and 4:4:4
    (three); frames that differ in a few hundred samples of every plane, so that every tile's nine numbers differ from every other
    tile's; zero tolerance and one that the MSE condition alone decides"""
    fmt, siting = fs
    T, H, W = (XL.SECOND_TRIP[k] for k in ("T", "H", "W"))
    assert (XL.partials_per_tile(T, fmt), XL.trips(XL.partials_per_tile(T, fmt))) == ((82, 2) if CC.sub(fmt)[1] == 2 else (163, 3))
    cur, prev = frame_pair(fmt, H, W, "few", 576)
    clip = [prev, cur, cur]
    top = (1 << CC.bits(fmt)) - 1
    for O in (0, 4):
        for aligned in (True, False):
            table = device_table(fmt, H, W, clip, aligned)
            for up in CC.UPSAMPLES:
                want = run(table, clip, fmt, siting, up, H, W, T, O, aligned, note=(fs, O))
                assert XL.all_differ([sum(tile, []) for tile in want[1][1]]) and want[0][2] == want[0][1] == [1] * len(want[0][1])
                loose = run(table, clip, fmt, siting, up, H, W, T, O, aligned, ((top,) * 3, (TOL.mse_q10(top * top / 3000), NO, NO), 0), note=(fs, O))
                assert loose[1][1] == want[1][1]


def tail_clip(fmt, T):
    """one T x T tile: frame 1 differs from frame 0 in a few hundred samples; frame 2 differs from frame 1 in the tile's last sy luma
    rows and last chroma row alone, so that of the row of partials only the last item block's is non-zero"""
    sx, sy = CC.sub(fmt)
    cur, prev = frame_pair(fmt, T, T, "few", T)
    codes = XL.codes_of(cur, fmt)
    XL.changed(codes, fmt, (slice(T - sy, T), slice(0, T)), 0, 1)
    XL.changed(codes, fmt, (T // sy - 1, slice(0, T // sx)), 1, XL.top_of(fmt) - 1)
    XL.changed(codes, fmt, (T // sy - 1, slice(0, T // sx)), 2, XL.top_of(fmt) // 2)
    return [prev, cur, CC.frame(*codes, fmt)]


@pytest.mark.parametrize("fs", [("nv12", "topleft"), ("p210", "left")], ids=ids)
def test_decide_seventeen_and_thirty_three_trips_at_2048(fs):
    """T = 2048 on a 2048 x 2048 frame, one tile: 1025 block partials at 4:2:0 (17 trips), 2049 at 4:2:2 (33).  Frame 1 differs from
    frame 0 in a few hundred samples spread over the row of partials; frame 2 from frame 1 in the tile's last rows alone: the only
    non-zero partial is the last item block's, an entry of the last full trip"""
    fmt, siting = fs
    T = 2048
    sx, sy = CC.sub(fmt)
    assert (XL.partials_per_tile(T, fmt), XL.trips(XL.partials_per_tile(T, fmt))) == ((1025, 17) if sy == 2 else (2049, 33))
    clip = tail_clip(fmt, T)
    top = XL.top_of(fmt)
    for aligned in (True, False):
        table = device_table(fmt, T, T, clip, aligned)
        want = run(table, clip, fmt, siting, "linear", T, T, T, 0, aligned, note=fs)
        assert want[0] == [[0], [1], [2]] and all(0 < s[0] <= 300 for s in want[1][1][0])
        assert counts(want[1][2]) == [[sy * T, T // sx, T // sx]]
        # reused under a tolerance: frame 2 is then judged against frame 0, both differences at once
        both = run(table, clip, fmt, siting, "linear", T, T, T, 0, aligned, ((top - 1,) * 3, (NO,) * 3, 0), note=fs)
        assert both[0] == [[0]] * 3 and both[1][1] == want[1][1] and both[1][2] != want[1][2]


# -- the largest sums ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("aligned", (True, False))
def test_largest_sums_at_2048(aligned):
    """a 2048 x 2048 one-tile i410 pair, all codes 0 against all codes 1023, F = 2: every count is 2048^2, every sse 2048^2 * 1023^2
    (> 2^41) and every maxabs 1023, by closed form.  A wave of the item blocks holds 64 * 8 samples of a plane, 64 * 8 * 1023^2 < 2^31;
    the MSE condition is decided at its exact boundary, 1024 * 1023^2 against mse_q10"""
    fmt, T = "i410", 2048
    clip = [CL.const_frame(fmt, T, T, 0, 0, 0), CL.const_frame(fmt, T, T, 1023, 1023, 1023)]
    full = [[T * T, T * T * 1023 * 1023, 1023]] * 3
    assert 2 ** 41 < T * T * 1023 * 1023 < 2 ** 43 and 17 * 1023 * 1023 < 2 ** 25 and 64 * 17 * 1023 * 1023 < 2 ** 31 < 64 * 17 * 1023 * 1023 * 2
    assert TOL.nsamp(0, T, T, T, 0, fmt, "centre", "linear") == [T * T] * 3
    table = device_table(fmt, T, T, clip, aligned)
    zero = [[[0, 0, 0]] * 3]
    bound = 1024 * 1023 * 1023                                                        # < 2^30
    for tol, src in [(((0, 0, 0), (NO,) * 3, 0), 1), (((1023,) * 3, (NO,) * 3, 0), 0), (((1023,) * 3, (bound,) * 3, 0), 0),
                     (((1023,) * 3, (bound, bound - 1, bound), 0), 1), (((1023, 1023, 1022), (NO,) * 3, 0), 1)]:
        assert TOL.close(full, [T * T] * 3, tol[0], tol[1]) is (src == 0)
        run(table, clip, fmt, "centre", "linear", T, T, T, 0, aligned, tol, want=([[0], [src]], [zero, [full]]), note=tol)

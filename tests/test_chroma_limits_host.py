"""tests/chroma_limits.py without a GPU: the table does what it claims.  The rows of block partials are as long as the cases say
(from the two libraries' own workspace-size functions); the closed forms of the largest-tile case are the restatement's values at a
small T and have the widths the case is there for; the tail-only data are non-zero through their last rows alone."""
import numpy as np
import pytest

from tests import chroma_contract as CC
from tests import chroma_limits as CL
from tests import chroma_rate_contract as XC
from tests import chroma_tiles_contract as KC
from tests import image_limits as IL
from tests import tiles_contract as TC


def sizes():
    from progressivecodec_amd import chroma_rate, chroma_tiles
    return chroma_tiles.lib().pc_chroma_tiles_stitch_workspace_size, chroma_rate.lib().pc_chroma_rate_workspace_size


def test_the_rows_of_partials_are_as_long_as_the_cases_say():
    stitch_size, rate_size = sizes()
    T = CL.SECOND_TRIP["T"]
    per_tile = {fmt: CL.partials_per_tile(T, fmt) for fmt, _ in CL.FORMATS}
    assert per_tile == {"nv12": 81, "p210": 162, "i444": 162}                              # a second and a third trip of 64 lanes
    for fmt, _ in CL.FORMATS:
        sy = CC.sub(fmt)[1]
        for n in (1, 4, 6):
            assert rate_size(T, sy, n) == 24 * n * per_tile[fmt]
        assert rate_size(512, sy, 1) == 24 * 128 // sy                                      # the tile size before: one trip, or two
    for fmt, _, partials, trips in CL.RATE_1024:
        assert CL.partials_per_tile(CL.FOUR_TRIPS["T"], fmt) == partials and -(-partials // 64) == trips
        assert rate_size(CL.FOUR_TRIPS["T"], CC.sub(fmt)[1], 4) == 24 * 4 * partials
    assert TC.grid(*(CL.FOUR_TRIPS[k] for k in "HWTO")) == (2, 2)
    c = CL.RATE_LIMIT
    for fmt, _ in CL.RATE_LIMIT_FORMATS:
        assert c["T"] == XC.max_tile(fmt) and rate_size(c["T"], CC.sub(fmt)[1], 1) == 24 * CL.partials_per_tile(c["T"], fmt) > 0
        assert rate_size(c["T"] + 64, CC.sub(fmt)[1], 1) == 0
    assert TC.grid(*(c[k] for k in "HWTO")) == (3, 3) and c["O"] == c["T"] // 2
    # the stitches: whole pictures past 256 partials (a second and a third trip of the final's 256 threads), and the 601 x 1101 one
    H, W = CL.WHOLE["H"], CL.WHOLE["W"]
    for fmt, _, partials in CL.WHOLE_FORMATS:
        assert CL.stitch_partials(H, W, fmt) == partials and stitch_size(0, H, W, CC.sub(fmt)[1]) == 24 * partials
    assert TC.grid(H, W, CL.WHOLE["T"], CL.WHOLE["O"]) == (2, 2)
    H, W = CL.SECOND_TRIP["H"], CL.SECOND_TRIP["W"]
    for fmt, _ in CL.STITCH_FORMATS:
        assert stitch_size(0, H, W, CC.sub(fmt)[1]) == 24 * CL.stitch_partials(H, W, fmt)
    assert [TC.grid(H, W, T, O) for O in CL.OVERLAPS] == [(2, 2), (2, 3), (2, 2), (2, 3)]
    assert all(O in CL.OVERLAPS for O in CL.STITCH_OVERLAPS) and 2 * 288 & (2 * 288 - 1)     # den = 576 is no power of two
    assert CL.CUT_LARGE["T"] == 2048 and TC.grid(*(CL.CUT_LARGE[k] for k in "HWTO")) == (3, 3)


@pytest.mark.parametrize("fmt,siting", [("nv12", "topleft"), ("nv16", "left"), ("i444", "centre"), ("p210", "topleft")])
def test_the_closed_forms_are_the_restatement_at_a_small_tile(fmt, siting):
    """the same grid shape as the limit case, T = 64, O = 32 on 128 x 128: tile 4 in bands entirely, and the corner and edge tiles"""
    c = dict(T=64, O=32, H=128, W=128)
    assert TC.grid(128, 128, 64, 32) == (3, 3)
    frame, eY, eC = CL.rate_saturated(fmt, 128, 128)
    x = np.zeros((9, 3, 64, 64), np.float32)
    got = XC.tile_sse(x, 128, 128, 64, 32, fmt, "bt709", "full", siting, frame)
    assert got == [CL.rate_closed(dict(c, tile=t), fmt, eY, eC) for t in range(9)]
    sx, sy = CC.sub(fmt)
    assert got[4][1] * sx * sy * eY * eY == got[4][0] * eC * eC


def test_the_largest_tiles_sums_have_the_widths_the_case_is_there_for():
    c = CL.RATE_LIMIT
    for fmt, _ in CL.RATE_LIMIT_FORMATS:
        frame, eY, eC = CL.rate_saturated(fmt, 64, 64)
        assert (eY, eC) == (255, 128)
        closed = CL.rate_closed(c, fmt, eY, eC)
        assert closed[0] == 285982974384537600 == IL.frame_rate_closed(c, eY, eC)[0] and 2 ** 54 <= closed[0] < 2 ** 60
        assert closed[1] == closed[2] == (2 ** 54 if fmt == "nv12" else 2 ** 55)            # 4:2:2: wy * (wx / 2)
    assert CL.rate_closed(c, "nv12", 255, 128) == IL.frame_rate_closed(c, 255, 128)


@pytest.mark.parametrize("fmt,siting", CL.FORMATS + [("p210", "topleft")])
def test_rate_tail_only_comes_from_the_last_rows_alone(fmt, siting):
    T, H, W = (CL.SECOND_TRIP[k] for k in ("T", "H", "W"))
    sx, sy = CC.sub(fmt)
    tail, eq, frame = CL.rate_tail(fmt, siting, T, H, W)
    assert np.array_equal(tail[:, :, :T - sy].view(np.uint32), eq[:, :, :T - sy].view(np.uint32))
    want = XC.tile_sse(tail, H, W, T, 0, fmt, "bt709", "limited", siting, frame)
    assert all(v > 0 for v in want[0]) and XC.tile_sse(eq, H, W, T, 0, fmt, "bt709", "limited", siting, frame) == [[0, 0, 0]]
    y, cb, cr = XC.tile_codes(tail[0], T, T, fmt, "bt709", "limited", siting)
    ey, ecb, ecr = XC.tile_codes(eq[0], T, T, fmt, "bt709", "limited", siting)
    assert (y[:T - sy] == ey[:T - sy]).all() and (cb[:T // sy - 1] == ecb[:T // sy - 1]).all() and (cr[:T // sy - 1] == ecr[:T // sy - 1]).all()
    assert want[0] == [int(((y[T - sy:] - ey[T - sy:]) ** 2).sum()), int(((cb[-1] - ecb[-1]) ** 2).sum()), int(((cr[-1] - ecr[-1]) ** 2).sum())]


@pytest.mark.parametrize("fmt,siting,partials", CL.WHOLE_FORMATS)
def test_whole_picture_tail_pairs_differ_in_the_last_luma_row_alone(fmt, siting, partials):
    H, W, T, O = (CL.WHOLE[k] for k in ("H", "W", "T", "O"))
    sx, sy = CC.sub(fmt)
    eq = CL.hostile(4, T, 3)
    tail = CL.last_row_tail(eq, T, O, H, W)
    assert np.array_equal(tail[:2].view(np.uint32), eq[:2].view(np.uint32)) and not np.array_equal(tail[2:].view(np.uint32), eq[2:].view(np.uint32))
    ref = KC.stitch(eq, H, W, T, O, fmt, "bt709", "limited", siting)
    got = KC.stitch_codes(tail, H, W, T, O, fmt, "bt709", "limited", siting)
    want = CC.codes(ref, fmt)
    assert (got[0][0, :H - 1] == want[0][0, :H - 1]).all() and (got[0][0, H - 1] != want[0][0, H - 1]).any()
    assert all((g[0, :-1] == w[0, :-1]).all() for g, w in zip(got[1:], want[1:]))             # the last chroma row alone
    sums = KC.sums(tail, H, W, T, O, fmt, "bt709", "limited", siting, ref)
    assert sums[0] > 0 and KC.sums(eq, H, W, T, O, fmt, "bt709", "limited", siting, ref) == [0, 0, 0]
    # the last row's 129 items are the last of the picture: block 258 exactly at 4:2:0, blocks 516 and 517 at 4:2:2 -- partials that
    # only the final's second and third trip gather
    items_per_row = -(-W // 8)
    first, last = (-(-H // sy) - 1) * items_per_row // 256, (-(-H // sy) * items_per_row - 1) // 256
    assert last == partials - 1 and first == (258 if sy == 2 else 516) and first >= 256

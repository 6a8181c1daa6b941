"""chroma_tiles (libpc_chroma_tiles.so) and chroma_rate (libpc_chroma_rate.so) on the GPU past T = 64 (tests/chroma_limits.py holds
the table; DESIGN.md section 19.1 the limits): the cut at T = 576 and T = 2048, the stitch at T = 576 and of whole pictures with 259
and 518 block partials, and chroma_rate's finals making their later trips -- 81 and 162 partials per tile at T = 576, 256 and 512 at
T = 1024 -- on hostile data and on tail-only data, and its largest tile at 4:2:0 and 4:2:2.  Every comparison is exact equality of
integers or bits against the restatements (tests/chroma_tiles_contract.py, tests/chroma_rate_contract.py); the largest tile against
closed forms in Python ints that tests/test_chroma_limits_host.py holds to the restatement at a small T."""
import numpy as np
import pytest
import torch

from tests import chroma_contract as CC
from tests import chroma_limits as CL
from tests import chroma_rate_contract as XC
from tests import chroma_tiles_contract as KC
from tests import image_limits as IL
from tests import tiles_contract as TC
from tests.test_gpu_band_weights import check_chroma_tiles
from tests.test_gpu_chroma_rate import sse_raw
from tests.test_gpu_chroma_tiles import cut_raw, frame_views
from tests.test_gpu_frames import same_bits
from tests.test_gpu_image_limits import need_memory
from tests.test_gpu_rate import check_out, float_tiles

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def ids(v):
    return "-".join(str(a) for a in v) if isinstance(v, tuple) else str(v)


# -- the cut -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("O", CL.OVERLAPS)
@pytest.mark.parametrize("fs", CL.FORMATS, ids=ids)
def test_cut_at_576(fs, O):
    """the 601 x 1101 frame in 576-tiles: the whole grid from aligned planes (wide where O is a multiple of 8, or at 4:4:4) and a
    rectangle that starts elsewhere from offset planes into a misaligned destination (narrow), under both upsamplers"""
    fmt, siting = fs
    T, H, W = (CL.SECOND_TRIP[k] for k in ("T", "H", "W"))
    ny, nx = TC.grid(H, W, T, O)
    sx = CC.sub(fmt)[0]
    matrix, rng = CL.settings(O // 4 + len(fmt))
    f = CC.random_frame(1, H, W, fmt, seed=O + 1, garbage=True)
    rect = CL.sub_rect(ny, nx)
    for up in CC.UPSAMPLES:
        want = KC.cut(f, fmt, matrix, rng, up, siting, T, O)
        rc, wide, got, guards = cut_raw(frame_views(fmt, H, W, 0, True, f), fmt, matrix, rng, up, siting, H, W, O, (0, 0, ny, nx), tile=T)
        assert rc == 0 and guards and wide == int(sx == 1 or O % 8 == 0), (fs, O, up)
        assert same_bits(got, want), (fs, O, up)
        rc, wide, got, guards = cut_raw(frame_views(fmt, H, W, 0, False, f), fmt, matrix, rng, up, siting, H, W, O, rect, 3, tile=T)
        assert rc == 0 and guards and wide == 0, (fs, O, up, rect)
        idx = [(rect[0] + a) * nx + rect[1] + b for a in range(rect[2]) for b in range(rect[3])]
        assert same_bits(got, want[idx]), (fs, O, up, rect)


def test_cut_at_2048():
    """tile (1, 1) alone of a 4098 x 4098 left-sited NV12 frame, whose chroma taps reach into its neighbours, on both paths"""
    need_memory(400 << 20)
    c = CL.CUT_LARGE
    H, W, T, O, rect, fmt, siting = (c[k] for k in ("H", "W", "T", "O", "rect", "fmt", "siting"))
    g = np.random.default_rng(12)
    Hc, Wc = CC.chroma_size(H, W, fmt)
    f = CC.frame(*[g.integers(0, 256, s, dtype=np.int64) for s in ((1, H, W), (1, Hc, Wc), (1, Hc, Wc))], fmt)
    want = KC.cut(f, fmt, "bt709", "limited", "linear", siting, T, O, rect)
    for aligned in (True, False):
        rc, wide, got, guards = cut_raw(frame_views(fmt, H, W, 0, aligned, f), fmt, "bt709", "limited", "linear", siting, H, W, O, rect, tile=T)
        assert rc == 0 and guards and wide == int(aligned)
        assert same_bits(got, want), aligned
        del got


# -- the stitch ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("O", CL.STITCH_OVERLAPS)
@pytest.mark.parametrize("fs", CL.STITCH_FORMATS, ids=ids)
def test_stitch_at_576_on_hostile_tiles(fs, O):
    """image and sums of the whole 601 x 1101 frame on both paths, and a window from the rectangle that just covers it.  O = 288:
    S = 288, den = 576 -- weights that are no floats in every band"""
    fmt, siting = fs
    T, H, W = (CL.SECOND_TRIP[k] for k in ("T", "H", "W"))
    ny, nx = TC.grid(H, W, T, O)
    x = np.array(CL.hostile(ny * nx, T, O + 5))
    matrix, rng = CL.settings(O // 64 + len(fmt))
    check_chroma_tiles(x, H, W, T, O, fmt, siting, matrix=matrix, rng=rng)
    S = T - O
    win = (S + 2, S + 6, 24, W - S - 6)
    rect = KC.covering(H, W, T, O, KC.halo_window(fmt, siting, win))
    check_chroma_tiles(x, H, W, T, O, fmt, siting, win=win, rect=rect, paths=(O == 64,), matrix=matrix, rng=rng)


@pytest.mark.parametrize("kind", ["hostile", "tail"])
@pytest.mark.parametrize("fsp", CL.WHOLE_FORMATS, ids=ids)
def test_stitch_whole_picture_sums(fsp, kind):
    """1026 x 1030 in 576-tiles at O = 64: 518 block partials at 4:2:2, 259 at 4:2:0 (check_sums holds the workspace to them): the
    final's 256 threads make a third and a second trip.  Hostile tiles against a random frame; and tiles that differ from the
    reference's in the last luma row alone, whose items are the last block's"""
    from progressivecodec_amd import chroma_tiles
    fmt, siting, partials = fsp
    H, W, T, O = (CL.WHOLE[k] for k in ("H", "W", "T", "O"))
    assert chroma_tiles.lib().pc_chroma_tiles_stitch_workspace_size(0, H, W, CC.sub(fmt)[1]) == 24 * partials
    eq = np.array(CL.hostile(4, T, 3))
    if kind == "hostile":
        check_chroma_tiles(eq, H, W, T, O, fmt, siting, matrix="bt2020", rng="limited")
        return
    tail = CL.last_row_tail(eq, H=H, W=W, T=T, O=O)
    ref = KC.stitch(eq, H, W, T, O, fmt, "bt709", "limited", siting)
    want = KC.sums(tail, H, W, T, O, fmt, "bt709", "limited", siting, ref)
    assert want[0] > 0 and any(want[1:])
    g = chroma_tiles.grid_of(H, W, T, O)
    planes = tuple(torch.from_numpy(np.ascontiguousarray(p[0])).to(DEV) for p in ref)
    for x_np, w in ((tail, want), (eq, [0, 0, 0])):
        xt = torch.from_numpy(x_np).to(DEV)
        out, d = chroma_tiles.stitch_frame(xt, g, fmt, "bt709", "limited", siting, ref=planes)
        assert d.sse.dtype == torch.int64 and d.sse.tolist() == [w], (fsp, kind)
        only = chroma_tiles.stitch_frame(float_tiles(x_np, "odd", T), g, fmt, "bt709", "limited", siting, ref=planes, image=False)
        assert only.sse.tolist() == [w], (fsp, kind, "narrow")
    assert all(np.array_equal(p.cpu().numpy(), r[0]) for p, r in zip(out, ref))              # the equal tiles give the reference back


# -- chroma_rate ---------------------------------------------------------------------------------------------------------------------

def rate_case(x_np, H, W, T, O, fmt, siting, matrix, rng, f, ranges, note):
    """the tiles x_np holds (the whole grid) against frame f on both paths, over the given (first, count) ranges"""
    want = XC.tile_sse(x_np, H, W, T, O, fmt, matrix, rng, siting, f)
    sx = CC.sub(fmt)[0]
    seen = set()
    for aligned in (True, False):
        xv = float_tiles(x_np, "contiguous" if aligned else "odd", T)
        refv = frame_views(fmt, H, W, 0, aligned, f)
        for first, m in ranges:
            rc, wide, buf, ws_ok = sse_raw(xv[first:first + m], H, W, O, first, fmt, rng, matrix, siting, refv, T)
            assert rc == 0 and ws_ok, (note, aligned, first, m)
            assert wide == int(aligned and (sx == 1 or O % 8 == 0)), (note, aligned)
            seen.add(wide)
            check_out(buf, want[first:first + m], (note, aligned, first, m))
    return want, seen


@pytest.mark.parametrize("O", CL.OVERLAPS)
@pytest.mark.parametrize("fs", CL.FORMATS, ids=ids)
def test_rate_later_trips_at_576_on_hostile_tiles(fs, O):
    """81 block partials per tile at 4:2:0 (the third row of the VCO path at depth), 162 at 4:2:2 and 4:4:4: row_final's second and
    third trip on partials that all differ; the whole grid, a sub-range and every tile alone, both paths"""
    fmt, siting = fs
    T, H, W = (CL.SECOND_TRIP[k] for k in ("T", "H", "W"))
    ny, nx = TC.grid(H, W, T, O)
    n = ny * nx
    x_np = np.array(CL.hostile(n, T, H + O))
    matrix, rng = CL.settings(O // 4 + len(siting))
    f = CC.random_frame(1, H, W, fmt, seed=T + O, garbage=True)
    ranges = [(0, n), IL.sub_range(n)] + [(t, 1) for t in range(n)]
    want, seen = rate_case(x_np, H, W, T, O, fmt, siting, matrix, rng, f, ranges, (fs, O))
    assert seen == ({0, 1} if CC.sub(fmt)[0] == 1 or O % 8 == 0 else {0})
    assert len({tuple(r) for r in want}) == n


@pytest.mark.parametrize("fsp", CL.RATE_1024, ids=ids)
def test_rate_four_and_eight_trips_at_1024(fsp):
    """T = 1024, O = 0 on 1030 x 1500: 256 partials per tile in p010, 512 in p210; tile 3 is clipped to 6 x 476, so that most of its
    blocks hold no active item and still write their zeros"""
    need_memory(300 << 20)
    fmt, siting, partials, trips = fsp
    T, H, W, O = (CL.FOUR_TRIPS[k] for k in ("T", "H", "W", "O"))
    assert CL.partials_per_tile(T, fmt) == partials
    x_np = np.array(CL.hostile(4, T, 11))
    f = CC.random_frame(1, H, W, fmt, seed=T, garbage=True)
    want, seen = rate_case(x_np, H, W, T, O, fmt, siting, "bt601", "limited", f, [(0, 4), (3, 1), (1, 2)], fsp)
    assert seen == {0, 1} and all(v > 0 for row in want for v in row)


@pytest.mark.parametrize("fs", CL.FORMATS + [("p210", "topleft")], ids=ids)
def test_rate_tail_only(fs):
    """the frame holds the tile's own rendering, so every error is zero; the tile's last sy rows are then flipped: of the row of 81 or
    162 partials only the last is non-zero, which only the final's last trip gathers"""
    fmt, siting = fs
    T, H, W = (CL.SECOND_TRIP[k] for k in ("T", "H", "W"))
    tail, eq, frame = CL.rate_tail(fmt, siting, T, H, W)
    want, _ = rate_case(tail, H, W, T, 0, fmt, siting, "bt709", "limited", frame, [(0, 1)], (fs, "tail"))
    assert all(v > 0 for v in want[0])
    zero, _ = rate_case(eq, H, W, T, 0, fmt, siting, "bt709", "limited", frame, [(0, 1)], (fs, "equal"))
    assert zero == [[0, 0, 0]]


@pytest.mark.parametrize("fs", CL.RATE_LIMIT_FORMATS, ids=ids)
def test_rate_largest_tile_meets_the_largest_error(fs):
    """T = 2048, O = 1024, tile 4 of a 4096 x 4096 frame in full range: zero tiles against Y at the top code and chroma 0.  Luma
    65025 * (2^21)^2, 58 bits; chroma 128^2 * 2^20 * 2^20 = 2^54 at 4:2:0 and 2^55 at 4:2:2, where the sum is wy * (wx / 2)"""
    need_memory(400 << 20)
    from progressivecodec_amd import chroma_rate
    fmt, siting = fs
    c = CL.RATE_LIMIT
    H, W, T, O, t = (c[k] for k in ("H", "W", "T", "O", "tile"))
    frame, eY, eC = CL.rate_saturated(fmt, H, W)
    want = [CL.rate_closed(c, fmt, eY, eC)]
    assert want[0][0] == 285982974384537600 and want[0][1] == (2 ** 54 if CC.sub(fmt)[1] == 2 else 2 ** 55)
    x_np = IL.const_tile(T, 0.0)
    for aligned in (True, False):
        xv = float_tiles(x_np, "contiguous" if aligned else "odd", T)
        refv = frame_views(fmt, H, W, 0, aligned, frame)
        rc, wide, buf, ws_ok = sse_raw(xv, H, W, O, t, fmt, "full", "bt709", siting, refv, T)
        assert rc == 0 and ws_ok and wide == int(aligned), (fs, aligned)
        check_out(buf, want, (fs, aligned))
        if aligned:
            got = chroma_rate.frame_tile_distortion(xv, chroma_rate.grid_of(H, W, T, O), tuple(v.t[0] for v in refv), fmt, "bt709", "full", siting,
                                                    first_tile=t)
            assert got.dtype == torch.int64 and got.tolist() == want                        # 58 bits reach Python
        del xv, refv

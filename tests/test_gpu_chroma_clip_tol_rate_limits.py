"""pc_chroma_clip_tol_rate_sse_runs past T = 64 and past short runs (progressivecodec_amd/chroma_clip_tol_rate.py,
libpc_chroma_clip_tol_rate.so; DESIGN.md section 19.1's row): tiles whose wave partials take the final's later trips, the largest
tiles of either depth against saturated frames (closed forms), a tile clipped to a few rows, tiles whose error lies in their last rows
alone, the refusal of T + 64, and one job with 130 entries beside one with 1.  Every raw call asserts its status, the poisoned
workspace (every partial written, nothing after them -- or, refused, none at all) and the path plan reports: plan is host only and
looks at pointers, strides and the overlap alone, so it answers for a call that is refused for its tile size as well; every
comparison is exact equality of integers."""
import numpy as np
import pytest
import torch

from tests import chroma_clip_tol_rate_cases as CS
from tests import chroma_clip_tol_rate_contract as TR
from tests import chroma_contract as CC
from tests import chroma_limits as CL
from tests import chroma_rate_contract as XC
from tests.test_gpu_chroma_clip_rate_limits import random_planes
from tests.test_gpu_chroma_clip_tol_rate import CR, CTR, DEV, expanded_on_the_gpu, runs_raw
from tests.test_gpu_chroma_clips import views
from tests.test_gpu_chroma_tiles import on_device
from tests.test_gpu_rate import POISON64, check_out, float_tiles

pytestmark = pytest.mark.gpu


def batched(planes):
    return [[p[None] for p in ps] for ps in planes]


@pytest.mark.parametrize("fmt,siting,partials,trips", [("nv12", "topleft", 324, 6), ("p210", "left", 648, 11), ("i444", "centre", 648, 11)])
def test_tiles_of_576_take_the_finals_later_trips(fmt, siting, partials, trips):
    """T = 576 on 601 x 1101: 4 * 576 * 576 / (2048 sy) wave partials per entry, so the final's 64 lanes make six trips (sy = 2, the
    row above read: VCO) or eleven; a whole tile, the tile of 25 rows and the corner of 25 x 525, hostile values, runs of 1, 2 and 3"""
    ctr = CTR()
    size, H, W, O = 576, 601, 1101, 0
    sy = CC.sub(fmt)[1]
    assert 4 * (size * size // (2048 * sy)) == partials and -(-partials // 64) == trips
    g = ctr.grid_of(H, W, size, O)
    assert (g.ny, g.nx) == (2, 2)
    fr = [CC.random_frame(1, H, W, fmt, seed=576 + s, garbage=True) for s in range(3)]
    tile_ids, runs = [0, 3, 2], [[1], [2, 0], [0, 1, 2]]
    x_np = CS.hostile(3, seed=576, size=size)
    want = TR.run_sse(x_np, fr, tile_ids, runs, H, W, size, O, fmt, "bt709", "limited", siting)
    assert CS.slots_matter(runs, want) == 4
    x = torch.from_numpy(x_np).to(DEV)
    planes = [on_device(f) for f in fr]
    odd = torch.zeros(x.numel() + 1, dtype=torch.float32, device=DEV)[1:].view(x.shape)
    odd.copy_(x)
    for xv, modes, wide in ((x, CS.ALIGNED, True), (odd, CS.MIXED, False)):
        table = [views(fmt, H, W, *m, f) for m, f in zip(modes, fr)]
        assert ctr.plan(xv, table, fmt, overlap=O) is wide
        rc, buf, ws_ok = runs_raw(xv, H, W, O, fmt, "limited", "bt709", siting, table, tile_ids, runs, size)
        assert rc == 0 and ws_ok
        check_out(buf, want, (fmt, wide))
    assert expanded_on_the_gpu(x, g, planes, tile_ids, runs, fmt, "bt709", "limited", siting) == want


@pytest.mark.parametrize("fmt,siting", CL.FORMATS)
def test_tail_only_tiles_at_576(fmt, siting):
    """the frame holds tile 0's own rendering, so every error of the equal tile is zero; the tail tile differs from it in its last sy
    rows alone.  Each against the frame twice, a second, different frame in the table: of an entry's 324 or 648 wave partials only
    the last block's four are non-zero, all at or after index 4 bpt - 4, which the final's sixth or eleventh trip gathers"""
    ctr = CTR()
    T, H, W = (CL.SECOND_TRIP[k] for k in ("T", "H", "W"))
    sy = CC.sub(fmt)[1]
    assert (T, H, W) == (576, 601, 1101) and (4 * (T * T // (2048 * sy)) - 4) // 64 == (5 if sy == 2 else 10)
    tail, eq, frame = CL.rate_tail(fmt, siting, T, H, W)
    row = XC.tile_sse(tail, H, W, T, 0, fmt, "bt709", "limited", siting, frame)[0]
    want = [row, row, [0, 0, 0], [0, 0, 0]]
    assert all(v > 0 for v in row)
    other = CC.random_frame(1, H, W, fmt, seed=77, garbage=True)
    for variant, modes in (("contiguous", CS.ALIGNED), ("odd", CS.MIXED)):
        x = float_tiles(np.concatenate([tail, eq]), variant, T)
        table = [views(fmt, H, W, *m, f) for m, f in zip(modes, (frame, other))]
        assert ctr.plan(x, table, fmt, overlap=0) is (variant == "contiguous")
        rc, buf, ws_ok = runs_raw(x, H, W, 0, fmt, "limited", "bt709", siting, table, [0, 0], [[0, 0], [0, 0]], T)
        assert rc == 0 and ws_ok
        check_out(buf, want, (fmt, variant))
        rc, buf, ws_ok = runs_raw(x, H, W, 0, fmt, "limited", "bt709", siting, table, [0, 0], [[0, 1], [1, 0]], T)      # the other frame: no zero row
        assert rc == 0 and ws_ok and buf[1].tolist() == row and buf[4].tolist() == [0, 0, 0] and all(v > 0 for v in buf[2].tolist() + buf[3].tolist())


def test_a_tile_of_1024_clipped_to_6_by_476():
    ctr = CTR()
    fmt, siting, size = "p210", "left", 1024
    H, W = size + 6, size + 476
    g = ctr.grid_of(H, W, size, 0)
    assert (g.ny, g.nx) == (2, 2) and size == ctr.max_tile(fmt)
    planes = [random_planes(fmt, H, W, seed=s) for s in (5, 6, 7)]
    gen = torch.Generator(device=DEV).manual_seed(7)
    x = torch.rand((2, 3, size, size), generator=gen, device=DEV) * 1.5 - 0.25
    tile_ids, runs = [3, 0], [[2, 0, 1], [1, 2]]
    assert ctr.plan(x, batched(planes), fmt, overlap=0)
    rc, buf, ws_ok = runs_raw(x, H, W, 0, fmt, "limited", "bt709", siting, batched(planes), tile_ids, runs, size)
    assert rc == 0 and ws_ok
    want = expanded_on_the_gpu(x, g, planes, tile_ids, runs, fmt, "bt709", "limited", siting)
    check_out(buf, want, "clipped")
    assert CS.slots_matter(runs, want) == 4 and all(v > 0 for row in want for v in row)
    assert want[3][0] > want[0][0] * 100                                    # 6 x 476 samples against 1024 x 1024


@pytest.mark.parametrize("fmt,siting,size", [("nv12", "topleft", 2048), ("nv16", "left", 2048), ("p210", "left", 1024)])
def test_the_largest_tiles_against_saturated_frames(fmt, siting, size):
    """one tile of the largest size the depth allows, all zeros and all ones, against a frame of the top code and a frame of code 0 at
    full range and O = 0 (every weight is 1): a zero tile is Y = 0, Cb = Cr = the chroma offset; a one tile Y = top, Cb = Cr = the
    offset.  The sums in closed form, and chroma_clip_rate's value of the expanded job"""
    ctr = CTR()
    H = W = size
    semi, bits, sh, sx, sy = CC.FORMATS[fmt]
    top, co = (1 << bits) - 1, 1 << (bits - 1)
    dt = np.uint16 if bits == 10 else np.uint8
    Hc, Wc = CC.chroma_size(H, W, fmt)
    shapes = [(H, W), (Hc, Wc, 2)] if semi else [(H, W), (Hc, Wc), (Hc, Wc)]
    planes = [tuple(torch.from_numpy(np.full(s, v << sh, dt)).to(DEV) for s in shapes) for v in (top, 0)]
    x = torch.stack([torch.zeros((3, size, size), device=DEV), torch.ones((3, size, size), device=DEV)])
    tile_ids, runs = [0, 0], [[0, 1, 0], [1, 0]]
    nY, nC = H * W, Hc * Wc
    want = [[top * top * nY, (top - co) ** 2 * nC, (top - co) ** 2 * nC], [0, co * co * nC, co * co * nC],
            [top * top * nY, (top - co) ** 2 * nC, (top - co) ** 2 * nC],
            [top * top * nY, co * co * nC, co * co * nC], [0, (top - co) ** 2 * nC, (top - co) ** 2 * nC]]
    assert max(v for row in want for v in row) < 2 ** 60 and size == ctr.max_tile(fmt)
    g = ctr.grid_of(H, W, size, 0)
    assert ctr.plan(x, batched(planes), fmt, overlap=0)
    rc, buf, ws_ok = runs_raw(x, H, W, 0, fmt, "full", "bt709", siting, batched(planes), tile_ids, runs, size)
    assert rc == 0 and ws_ok
    check_out(buf, want, (fmt, size))
    assert expanded_on_the_gpu(x, g, planes, tile_ids, runs, fmt, "bt709", "full", siting) == want
    assert CR().tile_distortion_jobs(x[:1], g, planes, [(0, 0)], fmt, "bt709", "full", siting).tolist() == want[:1]


@pytest.mark.parametrize("fmt,size", [("nv12", 2112), ("p210", 1088)])
def test_a_tile_64_past_the_largest_is_refused(fmt, size):
    ctr = CTR()
    H = W = size + 40
    planes = [random_planes(fmt, H, W, seed=1)]
    x = torch.zeros((1, 3, size, size), dtype=torch.float32, device=DEV)
    L = ctr.lib()
    assert L.pc_chroma_clip_tol_rate_workspace_size(2112, CC.sub(fmt)[1], 1) == 0 and L.pc_chroma_clip_tol_rate_workspace_size(2048, 1, 1) == 96 * 2048
    with pytest.raises(ValueError, match="at most %d" % (size - 64)):
        ctr.tile_distortion_runs(x, ctr.grid_of(H, W, size, 0), planes, [0], [[0]], fmt, siting="left")
    with pytest.raises(ValueError, match="at most %d" % (size - 64)):
        ctr.encode_clip_to_size(None, planes, [0], 10 ** 9, fmt, siting="left", tile=size)
    assert ctr.plan(x, batched(planes), fmt, overlap=0) is True                # host only: the path such a call would take, were it not refused
    rc, buf, ws_ok = runs_raw(x, H, W, 0, fmt, "limited", "bt709", "left", batched(planes), [0], [[0]], size)
    torch.cuda.synchronize()
    assert rc == -1 and (buf == POISON64).all() and ws_ok


@pytest.mark.parametrize("fmt,siting", [("nv12", "topleft"), ("p210", "left"), ("i444", "centre")])
def test_a_job_of_130_entries_beside_a_job_of_1(fmt, siting):
    """the entry loop far past the frames of the table: 130 entries over three frames in a seeded order, then a job of one"""
    ctr = CTR()
    H, W, O = 100, 150, 16
    fr = [CC.random_frame(1, H, W, fmt, seed=130 + s, garbage=True) for s in range(3)]
    g = np.random.default_rng(130)
    tile_ids, runs = [4, 1], [[int(v) for v in g.integers(0, 3, 130)], [2]]
    x_np = CS.hostile(2, seed=130)
    per_frame = TR.run_sse(x_np, fr, tile_ids, [[0, 1, 2], [2]], H, W, CS.T, O, fmt, "bt709", "limited", siting)
    assert CS.slots_matter([[0, 1, 2]], per_frame[:3]) == 3
    want = [per_frame[f] for f in runs[0]] + [per_frame[3]]
    planes = [on_device(f) for f in fr]
    x = torch.from_numpy(x_np).to(DEV)
    assert ctr.plan(x, batched(planes), fmt, overlap=O) is False               # rows of 150 elements: no multiple of 4
    rc, buf, ws_ok = runs_raw(x, H, W, O, fmt, "limited", "bt709", siting, batched(planes), tile_ids, runs)
    assert rc == 0 and ws_ok
    check_out(buf, want, fmt)
    got, off = ctr.tile_distortion_runs(x, ctr.grid_of(H, W, CS.T, O), planes, tile_ids, runs, fmt, siting=siting)
    assert got.tolist() == want and off == [0, 130, 131]

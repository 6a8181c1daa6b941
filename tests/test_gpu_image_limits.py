"""The image-side libraries on the GPU past T = 128 (tests/image_limits.py holds the table; DESIGN.md section 19.1 the limits): the
largest tile each library admits per format with every weight meeting the largest error; the second and the fourth trip of every
final reduction on hostile data, and tail-only data whose only non-zero partials are the last of their row; whole pictures with more
than 256 block partials and sums past 2^32; the cuts at T = 576 and T = 2048; and clip_tol_rate's largest tiles, the trips of its
final over an entry's wave partials, and runs longer than a wave has lanes.  Every comparison is exact equality of integers,
bits or bytes against the restatements (tests/*_contract.py) -- for saturated inputs against the closed forms that
tests/test_image_limits_host.py holds to the restatements; the one float64 sum is held to test_gpu_pixels.py's bound.  A case codes
one tile, or a few, of its grid (first_tile / rect / the job list), so that none holds more than about 0.25 GB on the device."""
import functools

import numpy as np
import pytest
import torch

from tests import clip_rate_contract as RC2
from tests import clip_tol_contract as TOL
from tests import clip_tol_rate_contract as TRC
from tests import clips_contract as CC
from tests import frame_rate_contract as QC
from tests import frame_tiles_contract as GC
from tests import frames_contract as FC
from tests import image_limits as IL
from tests import pixels_contract as K
from tests import rate_contract as RC
from tests import tiles_contract as TC
from tests.test_gpu_clip_rate import jobs_raw
from tests.test_gpu_clip_tol import check as check_scan
from tests.test_gpu_clip_tol import clip_codes, scan_raw
from tests.test_gpu_clip_tol_rate import runs_raw
from tests.test_gpu_clips import changes_raw, frame_pair, views
from tests.test_gpu_frame_rate import ref_views
from tests.test_gpu_frame_rate import sse_raw as frame_sse_raw
from tests.test_gpu_rate import check_out, float_tiles, in_layout, sse_raw, u8_tensor

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
#: the planes of two frames of a table: aligned with row strides that are multiples of 4, but different ones (wide where the overlap
#: allows it); pitched with a stride that is none next to one an element past an allocation start (narrow)
ALIGNED = [("pad4", 0), ("wider", 0), ("pad4", 0)]
MIXED = [("loose", 0), ("pad4", 1), ("tight", 0)]


def need_memory(nbytes):
    free = torch.cuda.mem_get_info(DEV)[0]
    if free < nbytes + (1 << 30):
        pytest.skip(f"{free >> 20} MiB of device memory free, the case needs {nbytes >> 20} MiB and 1024 MiB to spare")


def mods():
    from progressivecodec_amd import clip_rate, clip_tol, clip_tol_rate, clips, frame_rate, frame_tiles, frames, pixels, rate, tiles
    return dict(rate=rate, frame_rate=frame_rate, clip_rate=clip_rate, clips=clips, clip_tol=clip_tol, pixels=pixels, frames=frames,
                tiles=tiles, frame_tiles=frame_tiles, clip_tol_rate=clip_tol_rate)


def planes_of(f):
    """a frame of the restatement as unbatched cuda planes"""
    return tuple(torch.from_numpy(np.ascontiguousarray(p[0])).to(DEV) for p in f)


def table_of(fmt, H, W, modes, frames):
    return [views(fmt, H, W, *m, f) for m, f in zip(modes, frames)]


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(t, want_np):
    return torch.equal(bits(t), torch.from_numpy(np.ascontiguousarray(want_np).view(np.int32)).to(t.device).view(t.shape))


# -- A: the largest admitted tile, the largest error ---------------------------------------------------------------------------------

@pytest.mark.parametrize("mirror", [False, True], ids=["zeros-against-255", "ones-against-0"])
def test_rate_largest_tile_meets_the_largest_error(mirror):
    """T = 2048, O = 1024: tile 4 of 3 x 3 lies in bands entirely; every weight times 255^2: 65025 * (2^21)^2, 58 bits, per channel"""
    need_memory(300 << 20)
    rate = mods()["rate"]
    c = IL.RATE_LIMIT
    H, W, T, O, t = (c[k] for k in ("H", "W", "T", "O", "tile"))
    x_np, ref_chw, e = IL.rate_saturated(mirror)
    want = [[IL.rate_closed(c, e)] * 3]
    assert want[0][0] == 285982974384537600
    for variant, lay in [("contiguous", "chw"), ("odd", "hwc")]:
        x = float_tiles(x_np, variant, T)
        ref = u8_tensor(in_layout(ref_chw, lay), lay, pad4=True)
        assert rate.plan(x, ref, lay) is (variant == "contiguous")
        for rounding in ("nearest", "trunc"):
            rc, buf = sse_raw(rate.lib(), x, H, W, O, t, rate.ROUNDINGS[rounding], ref, lay, T)
            assert rc == 0, (variant, rounding)
            check_out(buf, want, (variant, lay, rounding))
        got = rate.tile_distortion(x, rate.grid_of(H, W, T, O), ref, first_tile=t, ref_layout=lay)      # 58 bits reach Python
        assert got.dtype == torch.int64 and got.tolist() == want
        del x, ref


def test_rate_largest_tile_clipped_by_the_image():
    """T = 2048 on a 3003 x 3501 image: tile 5 holds 1979 x 1453 pixels, neither a multiple of 8; hostile data, both paths"""
    need_memory(200 << 20)
    rate = mods()["rate"]
    c = IL.RATE_CLIPPED
    H, W, T, O, t = (c[k] for k in ("H", "W", "T", "O", "tile"))
    x_np, ref_chw = IL.rate_clipped_case()
    want = RC.tile_sse(x_np, H, W, T, O, "nearest", ref_chw, "chw", first_tile=t)
    print("rate, clipped tile at T = 2048:", want)
    assert all(2 ** 54 <= v < 2 ** 60 for v in want[0])
    for variant, lay, loose in [("contiguous", "chw", False), ("odd", "hwc", True)]:
        x = float_tiles(np.array(x_np), variant, T)
        ref = u8_tensor(in_layout(np.array(ref_chw), lay), lay, loose=loose, pad4=not loose)
        assert rate.plan(x, ref, lay) is (variant == "contiguous")
        rc, buf = sse_raw(rate.lib(), x, H, W, O, t, 0, ref, lay, T)
        assert rc == 0
        check_out(buf, want, (variant, lay))
        del x, ref


@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_frame_rate_largest_tile_meets_the_largest_error(fmt):
    """nv12 / i420 at T = 2048, p010 at T = 1024, O = T / 2, full range: Y at the top code and chroma 0 against zero tiles, and the
    mirror; the next tile size is refused for the format"""
    need_memory(300 << 20)
    fq = mods()["frame_rate"]
    c = IL.FRAME_LIMITS[fmt]
    H, W, T, O, t = (c[k] for k in ("H", "W", "T", "O", "tile"))
    for mirror in (False, True):
        v, frame, eY, eC = IL.frame_saturated(fmt, mirror)
        want = [IL.frame_rate_closed(c, eY, eC)]
        x_np = IL.const_tile(T, v)
        for variant, rv in [("contiguous", ("pad4", 0)), ("odd", ("loose", 0))]:
            x = float_tiles(x_np, variant, T)
            rt = [w.t for w in ref_views(fmt, H, W, *rv, frame)]
            assert fq.plan(x, rt, fmt, overlap=O) is (variant == "contiguous")
            rc, buf, ws_ok = frame_sse_raw(x, H, W, O, t, fmt, "full", "bt709", rt, T)
            assert rc == 0 and ws_ok, (fmt, mirror, variant)
            check_out(buf, want, (fmt, mirror, variant))
            if variant == "contiguous":
                got = fq.frame_tile_distortion(x, fq.grid_of(H, W, T, O), tuple(p[0] for p in rt), fmt, "bt709", "full", first_tile=t)
                assert got.tolist() == want
            del x, rt
    # one tile size on, the call refuses: no launch, nothing written
    big = T + 64
    x = torch.zeros((1, 3, big, big), device=DEV)
    rt = [w.t for w in ref_views(fmt, H, W, "pad4", 0, frame)]
    rc, buf, ws_ok = frame_sse_raw(x, H, W, 0, 0, fmt, "full", "bt709", rt, big)
    torch.cuda.synchronize()
    assert rc == -1 and ws_ok and (buf == -0x5A5A5A5A5A5A5A5B).all()


@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_clip_rate_largest_tile_jobs_are_frame_rates_values(fmt):
    """the same two frames as a clip; jobs with a repeat, both frames and a corner tile: each row is that (frame, tile)'s value"""
    need_memory(500 << 20)
    cr, fq = mods()["clip_rate"], mods()["frame_rate"]
    c = IL.FRAME_LIMITS[fmt]
    H, W, T, O = (c[k] for k in ("H", "W", "T", "O"))
    sat = [IL.frame_saturated(fmt, mirror) for mirror in (False, True)]
    clip = [s[1] for s in sat]
    jobs = IL.LIMIT_JOBS
    want = [IL.frame_rate_closed(dict(c, tile=t), sat[f][2], sat[f][3]) for f, t in jobs]
    x_np = np.concatenate([IL.const_tile(T, sat[f][0]) for f, _ in jobs])
    g = cr.grid_of(H, W, T, O)
    for modes, variant in [(ALIGNED, "contiguous"), (MIXED, "odd")]:
        x = float_tiles(x_np, variant, T)
        table = table_of(fmt, H, W, modes, clip)
        assert cr.plan(x, table, fmt, overlap=O) is (variant == "contiguous")
        rc, buf, ws_ok = jobs_raw(x, H, W, O, fmt, "full", "bt709", table, jobs, T)
        assert rc == 0 and ws_ok, (fmt, variant)
        check_out(buf, want, (fmt, variant))
        if variant == "contiguous":
            frames = [tuple(p[0] for p in ts) for ts in table]
            assert cr.tile_distortion_jobs(x, g, frames, jobs, fmt, "bt709", "full").tolist() == want
            for m in (0, 1, 3):
                f, t = jobs[m]
                assert fq.frame_tile_distortion(x[m:m + 1], g, frames[f], fmt, "bt709", "full", first_tile=t).tolist() == [want[m]]
        del x, table
    big = T + 64
    x = torch.zeros((1, 3, big, big), device=DEV)
    rc, buf, ws_ok = jobs_raw(x, H, W, 0, fmt, "full", "bt709", table_of(fmt, H, W, ALIGNED, clip), [(0, 0)], big)
    torch.cuda.synchronize()
    assert rc == -1 and ws_ok and (buf == -0x5A5A5A5A5A5A5A5B).all()


@pytest.mark.parametrize("fmt", IL.CLIP_FORMATS)
def test_clips_largest_tile_counts_its_whole_footprint(fmt):
    """T = 2048, O = 0 on 4098 x 4098: tile 4 with a complete halo ring; all 0 against all top code counts the footprint, identical
    frames and frames that differ below the code count nothing"""
    need_memory(400 << 20)
    cl = mods()["clips"]
    c = IL.CLIP_LIMIT
    H, W, T, O, t = (c[k] for k in ("H", "W", "T", "O", "tile"))
    f0, f1, f2 = IL.clip_limit_frames(fmt)
    for modes in (ALIGNED, MIXED):
        v0, v1, v2 = table_of(fmt, H, W, modes, (f0, f1, f2))
        assert cl.plan(cl.CHANGES, v1, fmt, other=v0, overlap=O) is (modes is ALIGNED)
        for up in FC.UPSAMPLES:
            want = CC.tile_changes(f1, f0, fmt, T, O, up)
            assert want[t] == IL.footprint_sizes(c, up)
            rc, buf, ws_ok = changes_raw(v1, v0, fmt, up, H, W, O, 0, 9, size=T)
            assert rc == 0 and ws_ok, (fmt, up)
            check_out(buf, want, (fmt, up, "grid"))
            rc, buf, ws_ok = changes_raw(v1, v0, fmt, up, H, W, O, t, 1, size=T)
            assert rc == 0 and ws_ok
            check_out(buf, [IL.footprint_sizes(c, up)], (fmt, up, "tile 4"))
            for a, b in ((v2, v1), (v0, v0)):                                  # low bits only (P010); the same frame
                rc, buf, ws_ok = changes_raw(a, b, fmt, up, H, W, O, 0, 9, size=T)
                assert rc == 0 and ws_ok
                check_out(buf, [[0, 0, 0]] * 9, (fmt, up, "equal"))
        if modes is ALIGNED:
            got = cl.tile_changes(tuple(p[0] for p in v1), tuple(p[0] for p in v0), fmt, T, O, "linear", first_tile=t, n_tiles=1)
            assert got.tolist() == [[4194304, 1052676, 1052676]]
        del v0, v1, v2


@pytest.mark.parametrize("fmt", IL.CLIP_FORMATS)
def test_clip_tol_largest_tile_decides_at_the_exact_boundary(fmt):
    """the same frames and a third equal to frame 1: every tile's stats are (n, n top^2, top) per plane; max_abs = top with mse_q10 =
    1024 top^2 reuses every tile, one less on either recodes every tile, and step 2 then compares against the anchor step 1 moved"""
    need_memory(400 << 20)
    ct = mods()["clip_tol"]
    c = IL.CLIP_LIMIT
    H, W, T, O, t = (c[k] for k in ("H", "W", "T", "O", "tile"))
    clip = IL.clip_limit_frames(fmt)
    top = IL.top_code(fmt)
    zeros = [[[0, 0, 0]] * 3] * 9
    for modes in (ALIGNED, MIXED):
        table = table_of(fmt, H, W, modes, clip)
        assert ct.plan(table, fmt, overlap=O) is (modes is ALIGNED)
        for up in FC.UPSAMPLES if modes is ALIGNED else ("linear",):
            stats1 = [[[n, n * top * top, top] for n in TOL.nsamp(k, H, W, T, O, up)] for k in range(9)]
            assert stats1[t][0] == [T * T, T * T * top * top, top]
            for max_abs, q10, max_run, reused in IL.boundary_tolerances(fmt):
                want = ([[0] * 9] * 3, [zeros, stats1, stats1]) if reused else ([[0] * 9, [1] * 9, [1] * 9], [zeros, stats1, zeros])
                rc, source, stats, ws_ok = scan_raw(table, fmt, up, H, W, O, (max_abs, q10, max_run), 9, T_=T)
                assert rc == 0 and ws_ok, (fmt, up, max_abs, q10)
                check_scan(source, stats, want, (fmt, up, max_abs, q10))
        if modes is ALIGNED:
            max_abs, q10, _, _ = IL.boundary_tolerances(fmt)[1]
            tol = ct.Tolerance(max_abs[0])._replace(mse_q10=q10)
            source, stats = ct.scan_clip([tuple(p[0] for p in ts) for ts in table], fmt, tol, T, O, "linear")
            assert source.tolist() == [[0] * 9, [1] * 9, [1] * 9] and stats[1, t, 0].tolist() == [T * T, T * T * top * top, top]
        del table


# -- B: the later trips of the final reductions ------------------------------------------------------------------------------------------

def trip_cases():
    """(id, T, H, W, O, wide, format): the second trip at three overlaps, the four trips once"""
    s, f = IL.SECOND_TRIP, IL.FOUR_TRIPS
    out = [(s["T"], s["H"], s["W"], O, wide, FC.FORMATS[k]) for k, (O, wide) in enumerate(IL.SECOND_TRIP_OVERLAPS)]
    return out + [(f["T"], f["H"], f["W"], f["O"], True, "p010")]


TRIPS = pytest.mark.parametrize("case", trip_cases(), ids=lambda c: f"T{c[0]}-O{c[3]}-{c[5]}")


@functools.lru_cache(maxsize=None)
def hostile(n, T, seed):
    x = TC.hostile_tiles(n, T, seed)
    x.setflags(write=False)
    return x


@TRIPS
def test_rate_later_trips_on_hostile_data(case):
    T, H, W, O, wide, _ = case
    rate = mods()["rate"]
    ny, nx = TC.grid(H, W, T, O)
    n = ny * nx
    x_np = np.array(hostile(n, T, H + O))
    ref_chw = IL.byte_image(H, W, 7)
    want = RC.tile_sse(x_np, H, W, T, O, "nearest", ref_chw, "chw")
    variant, lay = ("contiguous", "chw") if wide else ("odd", "hwc")
    x = float_tiles(x_np, variant, T)
    ref = u8_tensor(in_layout(ref_chw, lay), lay, loose=not wide, pad4=wide)
    assert rate.plan(x, ref, lay) is wide
    first, m = IL.sub_range(n)
    for a, k in ((0, n), (first, m)):
        rc, buf = sse_raw(rate.lib(), x[a:a + k], H, W, O, a, 0, ref, lay, T)
        assert rc == 0
        check_out(buf, want[a:a + k], (case, a, k))
    want_t = RC.tile_sse(x_np[n - 1:], H, W, T, O, "trunc", ref_chw, "chw", first_tile=n - 1)
    assert rate.tile_distortion(x[n - 1:], rate.grid_of(H, W, T, O), ref, first_tile=n - 1, ref_layout=lay, rounding="trunc").tolist() == want_t


@TRIPS
def test_frame_rate_later_trips_on_hostile_data(case):
    T, H, W, O, wide, fmt = case
    fq = mods()["frame_rate"]
    ny, nx = TC.grid(H, W, T, O)
    n = ny * nx
    x_np = np.array(hostile(n, T, H + O))
    f = FC.random_frame(1, H, W, fmt, seed=T + O)
    want = QC.tile_sse(x_np, H, W, T, O, fmt, "bt601", "limited", f)
    x = float_tiles(x_np, "contiguous" if wide else "odd", T)
    rt = [v.t for v in ref_views(fmt, H, W, "pad4" if wide else "loose", 0, f)]
    assert fq.plan(x, rt, fmt, overlap=O) is wide
    first, m = IL.sub_range(n)
    for a, k in ((0, n), (first, m)):
        rc, buf, ws_ok = frame_sse_raw(x[a:a + k], H, W, O, a, fmt, "limited", "bt601", rt, T)
        assert rc == 0 and ws_ok
        check_out(buf, want[a:a + k], (case, a, k))
    assert fq.frame_tile_distortion(x, fq.grid_of(H, W, T, O), tuple(p[0] for p in rt), fmt, "bt601", "limited").tolist() == want


@TRIPS
def test_clip_rate_later_trips_on_hostile_data(case):
    T, H, W, O, wide, fmt = case
    cr = mods()["clip_rate"]
    ny, nx = TC.grid(H, W, T, O)
    jobs = IL.job_list(ny * nx)
    x_np = np.array(hostile(len(jobs), T, W + O))
    clip = [FC.random_frame(1, H, W, fmt, seed=T + O + s) for s in range(2)]
    want = RC2.job_sse(x_np, clip, jobs, H, W, T, O, fmt, "bt2020", "full")
    assert want[1] != want[3] and jobs[1] == jobs[3]                           # the same job on another tile's floats
    x = float_tiles(x_np, "contiguous" if wide else "odd", T)
    table = table_of(fmt, H, W, ALIGNED if wide else MIXED, clip)
    assert cr.plan(x, table, fmt, overlap=O) is wide
    rc, buf, ws_ok = jobs_raw(x, H, W, O, fmt, "full", "bt2020", table, jobs, T)
    assert rc == 0 and ws_ok
    check_out(buf, want, case)
    rc, buf, ws_ok = jobs_raw(x[1:4], H, W, O, fmt, "full", "bt2020", table, jobs[1:4], T)
    assert rc == 0 and ws_ok
    check_out(buf, want[1:4], (case, "sub-list"))


@TRIPS
def test_clips_later_trips_on_hostile_data(case):
    T, H, W, O, wide, fmt = case
    cl = mods()["clips"]
    ny, nx = TC.grid(H, W, T, O)
    n = ny * nx
    first, m = IL.sub_range(n)
    for kind in ("few", "all"):
        cur, prev = frame_pair(fmt, H, W, kind, seed=T + O)
        cv, pv = table_of(fmt, H, W, ALIGNED if wide else MIXED, (cur, prev))
        assert cl.plan(cl.CHANGES, cv, fmt, other=pv, overlap=O) is wide
        for up in FC.UPSAMPLES:
            want = CC.tile_changes(cur, prev, fmt, T, O, up)
            assert kind == "few" or all(all(row) for row in want)
            for a, k in ((0, n), (first, m)):
                rc, buf, ws_ok = changes_raw(cv, pv, fmt, up, H, W, O, a, k, size=T)
                assert rc == 0 and ws_ok
                check_out(buf, want[a:a + k], (case, kind, up, a, k))
        got = cl.tile_changes(tuple(p[0] for p in cv), tuple(p[0] for p in pv), fmt, T, O, "linear")
        assert got.tolist() == CC.tile_changes(cur, prev, fmt, T, O, "linear")


@TRIPS
def test_clip_tol_later_trips_on_hostile_data(case):
    T, H, W, O, wide, fmt = case
    ct = mods()["clip_tol"]
    ny, nx = TC.grid(H, W, T, O)
    n = ny * nx
    for kind in ("noise", "few"):
        clip, _, tols = clip_codes(fmt, H, W, kind, seed=T + O)
        table = [views(fmt, H, W, *(ALIGNED if wide else MIXED)[k % 2], f) for k, f in enumerate(clip)]
        assert ct.plan(table, fmt, overlap=O) is wide
        for j, tol in enumerate(tols):
            up = FC.UPSAMPLES[(j + 1) % 2]
            want = TOL.scan(clip, fmt, T, O, up, *tol)
            rc, source, stats, ws_ok = scan_raw(table, fmt, up, H, W, O, tol, n, T_=T)
            assert rc == 0 and ws_ok, (case, kind, j)
            check_scan(source, stats, want, (case, kind, j))


# tail-only: the decoded tile is the original everywhere but in its last two rows, so only the tile's last block partial (number 80
# of 81) is non-zero, and the result is, only if the later trips are gathered

def test_rate_tail_only():
    rate = mods()["rate"]
    T, H, W = (IL.SECOND_TRIP[k] for k in ("T", "H", "W"))
    tail, eq, ref_chw = IL.rate_tail(T, H, W)
    want = RC.tile_sse(tail, H, W, T, 0, "nearest", ref_chw, "chw")
    assert all(v > 0 for v in want[0])
    for variant, lay in [("contiguous", "chw"), ("odd", "hwc")]:
        ref = u8_tensor(in_layout(ref_chw, lay), lay, pad4=True)
        for x_np, w in ((tail, want), (eq, [[0, 0, 0]])):
            rc, buf = sse_raw(rate.lib(), float_tiles(x_np, variant, T), H, W, 0, 0, 0, ref, lay, T)
            assert rc == 0
            check_out(buf, w, (variant, lay))


@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_frame_rate_and_clip_rate_tail_only(fmt):
    fq, cr = mods()["frame_rate"], mods()["clip_rate"]
    T, H, W = (IL.SECOND_TRIP[k] for k in ("T", "H", "W"))
    tail, eq, frame = IL.frame_tail(fmt, T, H, W)
    want = QC.tile_sse(tail, H, W, T, 0, fmt, "bt709", "limited", frame)
    assert all(v > 0 for v in want[0])
    other = FC.random_frame(1, H, W, fmt, seed=77)
    for variant, rv, modes in [("contiguous", ("pad4", 0), ALIGNED), ("odd", ("loose", 0), MIXED)]:
        rt = [v.t for v in ref_views(fmt, H, W, *rv, frame)]
        for x_np, w in ((tail, want), (eq, [[0, 0, 0]])):
            rc, buf, ws_ok = frame_sse_raw(float_tiles(x_np, variant, T), H, W, 0, 0, fmt, "limited", "bt709", rt, T)
            assert rc == 0 and ws_ok
            check_out(buf, w, (fmt, variant))
        # as jobs: the tail tile, the equal tile, the tail tile again, all against frame 1 of the table
        x = float_tiles(np.concatenate([tail, eq, tail]), variant, T)
        rc, buf, ws_ok = jobs_raw(x, H, W, 0, fmt, "limited", "bt709", table_of(fmt, H, W, modes, (other, frame)), [(1, 0)] * 3, T)
        assert rc == 0 and ws_ok
        check_out(buf, [want[0], [0, 0, 0], want[0]], (fmt, variant, "jobs"))


@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_clips_and_clip_tol_tail_only(fmt):
    """the frames differ in tile 0's last row pair and last chroma row, and in one Cb sample of its halo ring: partial 80 and the halo
    block's, number 81, the last of the row"""
    T, H, W = (IL.SECOND_TRIP[k] for k in ("T", "H", "W"))
    n = 4
    cur, prev = IL.clip_tail(fmt, T, H, W)
    inner, _ = IL.clip_tail(fmt, T, H, W, halo=False)
    for modes in (ALIGNED, MIXED):
        cv, pv, iv = table_of(fmt, H, W, modes, (cur, prev, inner))
        for a, up in ((cv, "linear"), (cv, "nearest"), (iv, "linear")):
            f = cur if a is cv else inner
            want = CC.tile_changes(f, prev, fmt, T, 0, up)
            assert want[0] == [2 * T, T // 2 + (1 if a is cv and up == "linear" else 0), T // 2]
            rc, buf, ws_ok = changes_raw(a, pv, fmt, up, H, W, 0, 0, n, size=T)
            assert rc == 0 and ws_ok
            check_out(buf, want, (fmt, up))
            rc, buf, ws_ok = changes_raw(a, pv, fmt, up, H, W, 0, 0, 1, size=T)
            assert rc == 0 and ws_ok
            check_out(buf, want[:1], (fmt, up, "tile 0"))
        rc, buf, ws_ok = changes_raw(pv, pv, fmt, "linear", H, W, 0, 0, n, size=T)
        assert rc == 0 and ws_ok
        check_out(buf, [[0, 0, 0]] * n, fmt)
        # the scan: a tolerance of nothing recodes tiles 0 and 2 (the rows below the tile are tile 2's own); a tolerance that lets the
        # halo's difference of 3 through but not the tile's own still recodes tile 0
        top = IL.top_code(fmt)
        for tol in [((0, 0, 0), (TOL.NO_MSE,) * 3, 0), ((top, 3, top), (TOL.NO_MSE,) * 3, 0), ((top,) * 3, (TOL.NO_MSE,) * 3, 0)]:
            for up in FC.UPSAMPLES:
                want = TOL.scan([prev, cur, inner], fmt, T, 0, up, *tol)
                rc, source, stats, ws_ok = scan_raw([pv, cv, iv], fmt, up, H, W, 0, tol, n, T_=T)
                assert rc == 0 and ws_ok
                check_scan(source, stats, want, (fmt, up, tol))
        assert TOL.scan([prev, cur], fmt, T, 0, "linear")[1][1][0][1][0] == T // 2 + 1


# -- C: whole pictures with more than 256 block partials, sums past 2^32 ---------------------------------------------------------------------

def close_enough(got, want, H, W):
    """test_gpu_pixels.py's bound for the float64 sum"""
    return abs(got - want) <= H * W * 2.0 ** -53 * want


@functools.lru_cache(maxsize=None)
def whole_planes():
    """(x_equal, x_tail [B,3,Hp,Wp], geometry): hostile planes, and the same with the last two rows of the last picture flipped"""
    H, W, B = IL.WHOLE["H"], IL.WHOLE["W"], IL.WHOLE["B"]
    hp, wp, top, left = K.geometry(H, W)
    eq = K.hostile_planes(np.stack([IL.byte_image(H, W, s) for s in range(B)]), hp, wp, top, left, seed=2)
    tail = np.array(eq)
    tail[B - 1, :, top + H - 2:top + H] = IL.flip(eq[B - 1, :, top + H - 2:top + H])
    return eq, tail, (hp, wp, top, left)


@pytest.mark.parametrize("kind", ["hostile", "saturated", "tail"])
def test_pixels_whole_picture_sums(kind):
    pixels = mods()["pixels"]
    H, W, B = IL.WHOLE["H"], IL.WHOLE["W"], IL.WHOLE["B"]
    eq, tail, (hp, wp, top, left) = whole_planes()
    geom = pixels.padding(H, W)
    assert (geom.Hp, geom.Wp, geom.top, geom.left) == (hp, wp, top, left)
    if kind == "hostile":
        x_np, ref = eq, np.stack([IL.byte_image(H, W, 10 + s) for s in range(B)])
    elif kind == "saturated":
        x_np, ref = np.zeros_like(eq), np.full((B, 3, H, W), 255, np.uint8)
    else:
        x_np, ref = tail, K.emit(eq, top, left, H, W, "nearest", "chw")
    su, sf = K.sums(x_np, top, left, H, W, "nearest", ref, "chw")
    if kind == "saturated":
        assert su == [[IL.whole_saturated_sum(255)] * 3] * B and su[0][0] > 2 ** 32
    if kind == "tail":
        assert su[0] == [0, 0, 0] and all(v > 0 for v in su[1])
    xt, rt = torch.from_numpy(x_np).to(DEV), torch.from_numpy(ref).to(DEV)
    for layout in ("chw", "hwc"):
        rl = rt if layout == "chw" else rt.permute(0, 2, 3, 1).contiguous()
        out, d = pixels.from_model_output(xt, geom, layout, "nearest", ref=rl, ref_layout=layout)
        assert torch.equal(out.cpu(), torch.from_numpy(K.emit(x_np, top, left, H, W, "nearest", layout))), (kind, layout)
        assert d.sse_u8.dtype == torch.int64 and d.sse_u8.tolist() == su, (kind, layout)
        got_f = d.sse_f.tolist()
        assert all(close_enough(got_f[b][c], sf[b][c], H, W) for b in range(B) for c in range(3)), (kind, layout, got_f, sf)
    only = pixels.from_model_output(xt[1:], geom, ref=rt[1:], ref_layout="chw", image=False)
    assert only.sse_u8.tolist() == su[1:]


@pytest.mark.parametrize("kind", ["hostile-nv12", "hostile-i420", "hostile-p010", "saturated-nv12", "saturated-p010", "tail-i420"])
def test_frames_whole_picture_sums(kind):
    frames, pixels = mods()["frames"], mods()["pixels"]
    kind, fmt = kind.split("-")
    H, W, B = IL.WHOLE["H"], IL.WHOLE["W"], IL.WHOLE["B"]
    eq, tail, (hp, wp, top, left) = whole_planes()
    geom = pixels.padding(H, W)
    matrix, rng = ("bt709", "full") if kind == "saturated" else ("bt601", "limited")
    if kind == "hostile":
        ref = FC.random_frame(B, H, W, fmt, seed=5)
        x_np = FC.hostile_planes(ref, fmt, matrix, rng, hp, wp, top, left, seed=6)
    elif kind == "saturated":
        mx = IL.top_code(fmt)
        x_np, ref = np.zeros_like(eq), tuple(np.repeat(p, B, axis=0) for p in IL.const_frame(fmt, H, W, mx, 0, 0))
    else:
        x_np, ref = tail, FC.emit(eq, top, left, H, W, fmt, matrix, rng)
    want = FC.sums(x_np, top, left, H, W, fmt, matrix, rng, ref)
    if kind == "saturated":
        assert all(row[0] == IL.whole_saturated_sum(IL.top_code(fmt)) and min(row) > 2 ** 32 for row in want)
    if kind == "tail":
        assert want[0] == [0, 0, 0] and all(v > 0 for v in want[1])
    xt = torch.from_numpy(x_np).to(DEV)
    rt = tuple(torch.from_numpy(np.ascontiguousarray(p)).to(DEV) for p in ref)
    out, d = frames.from_model_output(xt, geom, fmt, matrix, rng, ref=rt)
    assert d.sse.dtype == torch.int64 and d.sse.tolist() == want, kind
    assert all(np.array_equal(p.cpu().numpy(), w) for p, w in zip(out, FC.emit(x_np, top, left, H, W, fmt, matrix, rng)))
    only = frames.from_model_output(xt[1:], geom, fmt, matrix, rng, ref=tuple(p[1:] for p in rt), image=False)
    assert only.sse.tolist() == want[1:]


@functools.lru_cache(maxsize=None)
def whole_tiles():
    """(x_equal, x_tail [4,3,T,T]) of the 2 x 2 grid: hostile tiles, and the same with the picture's last two rows flipped"""
    H, W, T, O = (IL.WHOLE[k] for k in ("H", "W", "T", "O"))
    eq = np.array(hostile(4, T, 3))
    return eq, IL.stitch_tail(eq, T, O, H, W)


@pytest.mark.parametrize("kind", ["hostile", "saturated", "tail"])
def test_tiles_stitch_whole_picture_sums(kind):
    tiles = mods()["tiles"]
    H, W, T, O = (IL.WHOLE[k] for k in ("H", "W", "T", "O"))
    eq, tail = whole_tiles()
    if kind == "hostile":
        x_np, ref = eq, IL.byte_image(H, W, 4)
    elif kind == "saturated":
        x_np, ref = np.zeros_like(eq), np.full((3, H, W), 255, np.uint8)
    else:
        x_np, ref = tail, TC.stitch(eq, H, W, T, O, "nearest", "chw")
    su, sf = TC.sums(x_np, H, W, T, O, "nearest", ref, "chw")
    if kind == "saturated":
        assert su == [IL.whole_saturated_sum(255)] * 3
    if kind == "tail":
        assert all(v > 0 for v in su)
    g = tiles.grid_of(H, W, T, O)
    xt, rt = torch.from_numpy(x_np).to(DEV), torch.from_numpy(ref).to(DEV)
    for layout in ("chw", "hwc"):
        rl = rt if layout == "chw" else rt.permute(1, 2, 0).contiguous()
        out, d = tiles.stitch(xt, g, None, layout, "nearest", ref=rl, ref_layout=layout)
        assert torch.equal(out.cpu(), torch.from_numpy(TC.stitch(x_np, H, W, T, O, "nearest", layout))), (kind, layout)
        assert d.sse_u8.dtype == torch.int64 and d.sse_u8.tolist() == [su], (kind, layout)
        got_f = d.sse_f.tolist()[0]
        assert all(close_enough(got_f[c], sf[c], H, W) for c in range(3)), (kind, layout, got_f, sf)


@pytest.mark.parametrize("kind", ["hostile-nv12", "hostile-i420", "hostile-p010", "saturated-nv12", "saturated-p010", "tail-p010"])
def test_frame_tiles_stitch_whole_picture_sums(kind):
    ft = mods()["frame_tiles"]
    kind, fmt = kind.split("-")
    H, W, T, O = (IL.WHOLE[k] for k in ("H", "W", "T", "O"))
    eq, tail = whole_tiles()
    matrix, rng = ("bt709", "full") if kind == "saturated" else ("bt2020", "limited")
    if kind == "hostile":
        x_np, ref = eq, FC.random_frame(1, H, W, fmt, seed=8)
    elif kind == "saturated":
        x_np, ref = np.zeros_like(eq), IL.const_frame(fmt, H, W, IL.top_code(fmt), 0, 0)
    else:
        x_np, ref = tail, GC.stitch(eq, H, W, T, O, fmt, matrix, rng)
    want = GC.sums(x_np, H, W, T, O, fmt, matrix, rng, ref)
    if kind == "saturated":
        assert want[0] == IL.whole_saturated_sum(IL.top_code(fmt)) and min(want) > 2 ** 32
    if kind == "tail":
        assert all(v > 0 for v in want)
    g = mods()["tiles"].grid_of(H, W, T, O)
    xt = torch.from_numpy(x_np).to(DEV)
    out, d = ft.stitch_frame(xt, g, fmt, matrix, rng, ref=planes_of(ref))
    assert d.sse.dtype == torch.int64 and d.sse.tolist() == [want], kind
    assert all(np.array_equal(p.cpu().numpy(), w[0]) for p, w in zip(out, GC.stitch(x_np, H, W, T, O, fmt, matrix, rng)))


# -- D: the cuts at large T ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("O", [0, 64, 4])
def test_cuts_at_576(O):
    """tiles.cut, frame_tiles.cut_frame and clips.cut_tiles of the 601 x 1101 picture: the whole grid, and a scattered list"""
    tiles, ft, cl = mods()["tiles"], mods()["frame_tiles"], mods()["clips"]
    T, H, W = (IL.CUT_SMALL[k] for k in ("T", "H", "W"))
    ny, nx = TC.grid(H, W, T, O)
    img = IL.byte_image(H, W, O)
    for layout in ("chw", "hwc"):
        x, g = tiles.cut(torch.from_numpy(in_layout(img, layout)).to(DEV), T, O, layout)
        assert (g.ny, g.nx) == (ny, nx) and same_bits(x, TC.cut(img, "chw", T, O)), (O, layout)
    idx = [ny * nx - 1, 0, 1, ny * nx - 1, nx]
    for k, fmt in enumerate(FC.FORMATS):
        f = FC.random_frame(1, H, W, fmt, seed=O + k)
        matrix, rng, up = list(FC.MATRICES)[k], FC.RANGES[k % 2], FC.UPSAMPLES[(k + O // 4) % 2]
        want = GC.cut(f, fmt, matrix, rng, up, T, O)
        for planes in (planes_of(f), tuple(v[0] for v in views(fmt, H, W, "loose", 1, f))):
            x, g = ft.cut_frame(planes, fmt, matrix, rng, up, T, O)
            assert same_bits(x, want), (O, fmt)
            assert same_bits(cl.cut_tiles(planes, fmt, idx, matrix, rng, up, T, O), want[idx]), (O, fmt)


def test_tiles_cut_at_2048():
    """tile (1, 1) alone of a 4098 x 4098 image"""
    need_memory(300 << 20)
    tiles = mods()["tiles"]
    c = IL.CUT_LARGE
    H, W, T, O, rect = (c[k] for k in ("H", "W", "T", "O", "rect"))
    img = np.random.default_rng(11).integers(0, 256, (3, H, W), dtype=np.uint8)
    want = TC.cut(img, "chw", T, O, rect)
    for layout in ("chw", "hwc"):
        x, g = tiles.cut(torch.from_numpy(in_layout(img, layout)).to(DEV), T, O, layout, rect=rect)
        assert g.rect == rect and same_bits(x, want), layout
        del x


def test_frame_cuts_at_2048():
    """tile (1, 1) alone of a 4098 x 4098 P010 frame, whose chroma taps reach into all of its neighbours: frame_tiles.cut_frame of the
    rectangle and clips.cut_tiles of the index, from aligned and from pitched planes"""
    need_memory(400 << 20)
    ft, cl = mods()["frame_tiles"], mods()["clips"]
    c = IL.CUT_LARGE
    H, W, T, O, rect = (c[k] for k in ("H", "W", "T", "O", "rect"))
    f = IL.quick_frame("p010", H, W, seed=12)
    want = GC.cut(f, "p010", "bt709", "limited", "linear", T, O, rect)
    for planes in (planes_of(f), tuple(v[0] for v in views("p010", H, W, "loose", 1, f))):
        x, g = ft.cut_frame(planes, "p010", "bt709", "limited", "linear", T, O, rect=rect)
        assert same_bits(x, want)
        del x
        assert same_bits(cl.cut_tiles(planes, "p010", [4], "bt709", "limited", "linear", T, O), want)


# -- E: clip_tol_rate: the largest tile, the later trips of its final over an entry's wave partials, long runs ------------------------------

def expanded_rows(x, g, planes, tile_ids, runs, fmt, matrix, rng):
    """clip_rate.tile_distortion_jobs of the expanded job list, a job's entries at a time (at T = 2048 a tile is 50 MB)"""
    cr = mods()["clip_rate"]
    out = []
    for m, (t, run) in enumerate(zip(tile_ids, runs)):
        for a in range(0, len(run), 64):
            part = run[a:a + 64]
            rep = x[m:m + 1].expand(len(part), -1, -1, -1).contiguous()
            out += cr.tile_distortion_jobs(rep, g, planes, [(f, t) for f in part], fmt, matrix, rng).tolist()
            del rep
    return out


@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_clip_tol_rate_largest_tile_runs_are_frame_rates_values(fmt):
    """nv12 / i420 at T = 2048 (4096 wave partials per entry, 64 trips of the final), p010 at T = 1024 (1024, 16 trips), O = T / 2, full
    range: zero and one tiles against both saturated frames, a frame twice in a run, a corner tile; every row is the closed form of
    its (tile value, frame) pair and clip_rate's value of the expanded job; the next tile size is refused for the format"""
    need_memory(500 << 20)
    ctr = mods()["clip_tol_rate"]
    c = IL.FRAME_LIMITS[fmt]
    H, W, T, O = (c[k] for k in ("H", "W", "T", "O"))
    clip, vals, tile_ids, runs, want = IL.run_limit_case(fmt)
    x_np = np.concatenate([IL.const_tile(T, v) for v in vals])
    for modes, variant in [(ALIGNED, "contiguous"), (MIXED, "odd")]:
        x = float_tiles(x_np, variant, T)
        table = table_of(fmt, H, W, modes, clip)
        assert ctr.plan(x, table, fmt, overlap=O) is (variant == "contiguous")
        rc, buf, ws_ok = runs_raw(x, H, W, O, fmt, "full", "bt709", table, tile_ids, runs, T)
        assert rc == 0 and ws_ok, (fmt, variant)
        check_out(buf, want, (fmt, variant))
        if variant == "contiguous":
            frames = [tuple(p[0] for p in ts) for ts in table]
            g = ctr.grid_of(H, W, T, O)
            got, off = ctr.tile_distortion_runs(x, g, frames, tile_ids, runs, fmt, "bt709", "full")
            assert got.dtype == torch.int64 and got.tolist() == want and off == [0, 3, 5, 6]          # 58 bits reach Python
            assert expanded_rows(x, g, frames, tile_ids, runs, fmt, "bt709", "full") == want
        del x, table
    big = T + 64
    x = torch.zeros((1, 3, big, big), device=DEV)
    rc, buf, ws_ok = runs_raw(x, H, W, 0, fmt, "full", "bt709", table_of(fmt, H, W, ALIGNED, clip), [0], [[0]], big)
    torch.cuda.synchronize()
    assert rc == -1 and ws_ok and (buf == -0x5A5A5A5A5A5A5A5B).all()


@pytest.mark.parametrize("case", IL.run_trip_cases(), ids=lambda c: f"T{c[0]}-O{c[3]}-{c[5]}")
def test_clip_tol_rate_later_trips_on_hostile_data(case):
    """T = 576: 324 wave partials per entry, six trips; T = 1024: 1024, sixteen; tile 3 of the latter is clipped to 6 x 476, so that
    most of its blocks hold no active item and still write their zeros"""
    T, H, W, O, wide, fmt = case
    ctr = mods()["clip_tol_rate"]
    ny, nx = TC.grid(H, W, T, O)
    tile_ids, runs = IL.run_list(ny * nx)
    off = TRC.offsets_of(runs)
    x_np = np.array(hostile(len(tile_ids), T, W + O))
    clip = [FC.random_frame(1, H, W, fmt, seed=T + O + s) for s in range(2)]
    want = TRC.run_sse(x_np, clip, tile_ids, runs, H, W, T, O, fmt, "bt2020", "full")
    assert want[off[1]] != want[off[3]] and tile_ids[1] == tile_ids[3] and runs[1][0] != runs[3][0]
    x = float_tiles(x_np, "contiguous" if wide else "odd", T)
    table = table_of(fmt, H, W, ALIGNED if wide else MIXED, clip)
    assert ctr.plan(x, table, fmt, overlap=O) is wide
    rc, buf, ws_ok = runs_raw(x, H, W, O, fmt, "full", "bt2020", table, tile_ids, runs, T)
    assert rc == 0 and ws_ok
    check_out(buf, want, case)
    rc, buf, ws_ok = runs_raw(x[1:3], H, W, O, fmt, "full", "bt2020", table, tile_ids[1:3], runs[1:3], T)
    assert rc == 0 and ws_ok
    check_out(buf, want[off[1]:off[3]], (case, "sub-list"))
    frames = [tuple(p[0] for p in ts) for ts in table]
    assert expanded_rows(x, ctr.grid_of(H, W, T, O), frames, tile_ids, runs, fmt, "bt2020", "full") == want


@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_clip_tol_rate_tail_only(fmt):
    """the tail tile and the equal tile, each against the frame twice: of an entry's 324 wave partials only the last block's four
    are non-zero, which the final's sixth trip gathers"""
    T, H, W = (IL.SECOND_TRIP[k] for k in ("T", "H", "W"))
    tail, eq, frame = IL.frame_tail(fmt, T, H, W)
    row = QC.tile_sse(tail, H, W, T, 0, fmt, "bt709", "limited", frame)[0]
    want = [row, row, [0, 0, 0], [0, 0, 0]]
    assert all(v > 0 for v in row)
    other = FC.random_frame(1, H, W, fmt, seed=77)
    for variant, modes in [("contiguous", ALIGNED), ("odd", MIXED)]:
        x = float_tiles(np.concatenate([tail, eq]), variant, T)
        table = table_of(fmt, H, W, modes, (frame, other))
        rc, buf, ws_ok = runs_raw(x, H, W, 0, fmt, "limited", "bt709", table, [0, 0], [[0, 0], [0, 0]], T)
        assert rc == 0 and ws_ok
        check_out(buf, want, (fmt, variant))


@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_clip_tol_rate_long_runs_and_many_entries(fmt):
    """T = 64, 100 x 150, three frames, six jobs of 70, 1, 2, 33, 64 and 130 entries: the entry loop runs past a wave's lanes, and
    the final has 300 rows"""
    ctr = mods()["clip_tol_rate"]
    c = IL.LONG_RUNS
    T, H, W, O = (c[k] for k in ("T", "H", "W", "O"))
    tile_ids, runs = IL.long_runs()
    off = TRC.offsets_of(runs)
    x_np = np.array(hostile(len(tile_ids), T, 300))
    clip = [FC.random_frame(1, H, W, fmt, seed=300 + s) for s in range(3)]
    want = TRC.run_sse(x_np, clip, tile_ids, runs, H, W, T, O, fmt, "bt601", "limited")
    assert len(want) == 300 and all(any(want[off[m] + j] != want[off[m]] for j in range(64, len(runs[m]))) for m in (0, 5))
    g = ctr.grid_of(H, W, T, O)
    for modes, variant in [(ALIGNED, "contiguous"), (MIXED, "odd")]:
        x = float_tiles(x_np, variant, T)
        table = table_of(fmt, H, W, modes, clip)
        assert ctr.plan(x, table, fmt, overlap=O) is (variant == "contiguous")
        rc, buf, ws_ok = runs_raw(x, H, W, O, fmt, "limited", "bt601", table, tile_ids, runs, T)
        assert rc == 0 and ws_ok, (fmt, variant)
        check_out(buf, want, (fmt, variant))
        frames = [tuple(p[0] for p in ts) for ts in table]
        got, goff = ctr.tile_distortion_runs(x, g, frames, tile_ids, runs, fmt, "bt601", "limited")
        assert got.shape == (300, 3) and got.tolist() == want and goff == off
        if variant == "contiguous":
            assert expanded_rows(x, g, frames, tile_ids, runs, fmt, "bt601", "limited") == want

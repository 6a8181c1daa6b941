"""Rate-controlled clips on the GPU (progressivecodec_amd/clip_rate.py, libpc_clip_rate.so) against their restatement
(tests/clip_rate_contract.py): the distortion sums of scattered (frame, tile) jobs exactly, on both access paths, against
tests/frame_rate_contract.tile_sse and against frame_rate.frame_tile_distortion of the same tile; and encode_clip_to_size / decode_clip
through the codec and a PCS2 container.  Every comparison is exact equality of integers, bits or bytes.  T = 64 throughout (one case
at 128): the smallest tile, so that the frames stay small while every branch is taken."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import clip_rate_contract as RC2
from tests import clips_contract as CC
from tests import frame_rate_contract as QC
from tests import frames_contract as FC
from tests import rate_contract as RC
from tests import tiles_contract as TC
from tests.test_gpu_clips import clip_of, views
from tests.test_gpu_frame_rate import saturated
from tests.test_gpu_rate import POISON64, check_out, float_tiles
from tests.util import gpu_codec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POL = "point-based-std"
T = 64
SIZES = [(1, 1), (65, 63), (100, 150), (127, 129)]
OVERLAPS = [0, 4, 16, 32]
BAND_OVERLAPS = [24, 28]                                                    # 2 O is no power of two (tests/band_cases.py)
MATS = list(FC.MATRICES)
#: the three frames of a table as views: all aligned with row strides that are multiples of 4 (the wide path's), or pitched
#: differently with one of them one element past an allocation start (narrow, whichever frame a job names)
ALIGNED = [("pad4", 0), ("wider", 0), ("pad4", 0)]
MIXED = [("loose", 0), ("pad4", 1), ("pad4", 0)]


def CR():
    from progressivecodec_amd import clip_rate
    return clip_rate


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def jobs_raw(x, H, W, O, fmt, rng, matrix, table, jobs, size=T, over=None):
    """pc_clip_rate_sse_jobs on the tiles x holds, the jobs written to the device as they are -> (status, the [n + 2, 3] buffer whose
    rows 1 .. n are `out`, poisoned beforehand, whether every partial of the workspace and no word after it was written -- or, for a
    refused call, none at all).  table: per frame the list of batched plane tensors.  over: arguments to replace, by name."""
    from progressivecodec_amd import frames
    L = CR().lib()
    n = len(jobs)
    buf = torch.full((n + 2, 3), POISON64, dtype=torch.int64, device=DEV)
    need = L.pc_clip_rate_workspace_size(size, n)
    ws = torch.full((need // 8 + 1,), POISON64, dtype=torch.int64, device=DEV)
    k = frames.coefficients(matrix)
    host = (frames.Frame * len(table))(*[frames._frame_struct(list(ts)) for ts in table])
    dtab = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(DEV)
    djobs = torch.tensor(jobs, dtype=torch.int32).reshape(-1, 2).to(DEV)
    a = dict(x=x.data_ptr(), sxt=x.stride(0), sxc=x.stride(1), sxh=x.stride(2), H=H, W=W, T=size, O=O, fmt=frames.FORMATS.get(fmt, fmt),
             range=frames.RANGES.get(rng, rng), kr=k.kr, kg=k.kg, kb=k.kb, ib=k.ib, ir=k.ir, frames_host=host, frames_dev=dtab.data_ptr(),
             n_frames=len(table), jobs=djobs.data_ptr(), n_jobs=n, ws=ws.data_ptr(), nbytes=need, out=buf[1:].data_ptr(), stream=stream())
    a.update(over or {})
    rc = L.pc_clip_rate_sse_jobs(*a.values())
    h = ws.cpu()
    return rc, buf, bool(h[-1] == POISON64 and ((h[:-1] != POISON64).all() if rc == 0 else (h == POISON64).all()))


def job_list(n, seed):
    """jobs over three frames: every tile of frame 2 in descending order, then frames 0 and 1 out of order with a job repeated"""
    g = np.random.default_rng(seed)
    jobs = [(2, t) for t in reversed(range(n))] + [(0, 0), (1, n - 1), (0, 0), (1, int(g.integers(0, n))), (0, int(g.integers(0, n)))]
    assert jobs[n] == jobs[n + 2] and {t for f, t in jobs if f == 2} == set(range(n))
    return jobs


def kernel_matrix(hw, overlaps):
    """every overlap x format x range against the restatement and against frame_tile_distortion of the same tile and frame; a table
    of three frames with different contents, once all aligned (wide where the floats and the overlap allow it) and once with mixed
    pitches and an offset pointer (narrow); the jobs out of frame order, with a repeat, covering every tile of one frame; the Python
    call on a list, on batched planes and on a side stream."""
    cr = CR()
    from progressivecodec_amd import frame_rate
    H, W = hw
    seen = set()
    for O in overlaps:
        ny, nx = TC.grid(H, W, T, O)
        n = ny * nx
        jobs = job_list(n, H + W + O)
        x_np = TC.hostile_tiles(len(jobs), T, seed=H + W + O)
        xs = {v: float_tiles(x_np, v) for v in ("contiguous", "odd")}
        g = cr.grid_of(H, W, T, O)
        for k, fmt in enumerate(FC.FORMATS):
            fr = [FC.random_frame(1, H, W, fmt, seed=1000 * H + W + O + 10 * k + s) for s in range(3)]
            tables = {"aligned": [views(fmt, H, W, *m, f) for m, f in zip(ALIGNED, fr)], "mixed": [views(fmt, H, W, *m, f) for m, f in zip(MIXED, fr)]}
            planes = [tuple(torch.from_numpy(p[0]).to(DEV) for p in f) for f in fr]
            for rng in FC.RANGES:
                matrix = MATS[(k + O // 4 + (rng == "full")) % 3]
                want = RC2.job_sse(x_np, fr, jobs, H, W, T, O, fmt, matrix, rng)
                for tname, variant in (("aligned", "contiguous"), ("mixed", "contiguous"), ("aligned", "odd"), ("mixed", "odd")):
                    expect = tname == "aligned" and variant == "contiguous" and O % 8 == 0
                    wide = cr.plan(xs[variant], tables[tname], fmt, overlap=O)
                    case = (H, W, O, fmt, rng, tname, variant)
                    assert wide is expect, case
                    seen.add(wide)
                    rc, buf, ws_ok = jobs_raw(xs[variant], H, W, O, fmt, rng, matrix, tables[tname], jobs)
                    assert rc == 0 and ws_ok, case
                    check_out(buf, want, case)
                if rng == "limited":
                    # the existing call on the same tile and frame: the same integers
                    for m, (f, t) in enumerate(jobs):
                        one = frame_rate.frame_tile_distortion(xs["contiguous"][m:m + 1], g, planes[f], fmt, matrix, rng, first_tile=t)
                        assert one.tolist() == [want[m]], (H, W, O, fmt, m, f, t)
                    # a sub-list, and one job alone, on either path
                    for tname, variant in (("aligned", "contiguous"), ("mixed", "odd")):
                        rc, buf, ws_ok = jobs_raw(xs[variant][1:n + 2], H, W, O, fmt, rng, matrix, tables[tname], jobs[1:n + 2])
                        assert rc == 0 and ws_ok
                        check_out(buf, want[1:n + 2], (H, W, O, fmt, tname, "sub-list"))
                        rc, buf, ws_ok = jobs_raw(xs[variant][n:n + 1], H, W, O, fmt, rng, matrix, tables[tname], jobs[n:n + 1])
                        assert rc == 0 and ws_ok
                        check_out(buf, want[n:n + 1], (H, W, O, fmt, tname, "alone"))
                else:
                    # the Python call: a list of pitched frames; batched planes; channels last in memory (copied); a side stream
                    got = cr.tile_distortion_jobs(xs["odd"], g, [tuple(v[0] for v in ts) for ts in tables["mixed"]], jobs, fmt, matrix, rng)
                    assert got.dtype == torch.int64 and got.shape == (len(jobs), 3) and got.device.type == "cuda" and got.tolist() == want
                    batched = tuple(torch.stack(ps) for ps in zip(*planes))
                    cl = xs["contiguous"].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
                    assert cr.tile_distortion_jobs(cl, g, batched, torch.tensor(jobs), fmt, matrix, rng).tolist() == want
                    side = torch.cuda.Stream(DEV)
                    side.wait_stream(torch.cuda.current_stream(DEV))
                    with torch.cuda.stream(side):
                        got_s = cr.tile_distortion_jobs(xs["contiguous"][-2:], g, planes, jobs[-2:], fmt, matrix, rng)
                    side.synchronize()
                    assert got_s.tolist() == want[-2:]
    assert seen == {True, False}


@pytest.mark.parametrize("hw", SIZES)
def test_kernel_matrix_exact_on_both_paths(hw):
    kernel_matrix(hw, OVERLAPS)


def test_kernel_matrix_at_overlaps_whose_band_quotients_are_no_floats():
    """O = 24 (S = 40, den = 48: the wide path where there is one) and O = 28 (S = 36, den = 56: narrow at 4:2:0) on one picture.  The
    sums weigh with the integer numerators 2u + 1, which are exact whatever 2 O is; what is new is the band geometry."""
    kernel_matrix((100, 150), BAND_OVERLAPS)


@pytest.mark.parametrize("fmt", ["nv12", "i420", "p010"])
def test_jobs_out_of_range_give_zeros_and_touch_nothing(fmt):
    """a job whose slot is -1 or n_frames, or whose tile is -1 or ny * nx (and the far ends of int32), written straight through the C
    call: 0, 0, 0, its neighbours intact, every partial written, nothing outside out or the workspace"""
    cr = CR()
    H, W = 100, 150
    for O in (0, 16):
        n = 6
        fr = [FC.random_frame(1, H, W, fmt, seed=40 + s + O) for s in range(3)]
        good = [(1, 4), (0, 0), (2, 5), (1, 1), (0, 3), (2, 2), (1, 5), (0, 5), (2, 0), (1, 0)]
        bad = {1: (-1, 0), 3: (3, 0), 4: (0, -1), 6: (0, n), 7: (2 ** 31 - 1, 2), 8: (-2 ** 31, 2), 9: (1, 2 ** 31 - 1)}
        jobs = [bad.get(m, j) for m, j in enumerate(good)] + [(2, -2 ** 31), (-1, -1), (3, n), (1, 3)]
        x_np = TC.hostile_tiles(len(jobs), T, seed=O + 9)
        valid = [m for m, (f, t) in enumerate(jobs) if 0 <= f < 3 and 0 <= t < n]
        assert valid == [0, 2, 5, len(jobs) - 1]
        full = RC2.job_sse(x_np[valid], fr, [jobs[m] for m in valid], H, W, T, O, fmt, "bt709", "limited")
        want = [[0, 0, 0]] * len(jobs)
        for m, row in zip(valid, full):
            want[m] = row
            assert any(row)
        for modes, variant in ((ALIGNED, "contiguous"), (MIXED, "odd")):
            table = [views(fmt, H, W, *m, f) for m, f in zip(modes, fr)]
            x = float_tiles(x_np, variant)
            assert cr.plan(x, table, fmt, overlap=O) is (variant == "contiguous")
            rc, buf, ws_ok = jobs_raw(x, H, W, O, fmt, "limited", "bt709", table, jobs)
            assert rc == 0 and ws_ok
            check_out(buf, want, (fmt, O, variant))


def test_refused_calls_launch_nothing():
    cr = CR()
    L = cr.lib()
    H, W, O = 100, 150, 16
    jobs = [(1, 5), (0, 0), (2, 3), (0, 0), (1, 2)]
    x = torch.rand(len(jobs), 3, T, T, device=DEV)
    for fmt in ("nv12", "p010"):
        table = [views(fmt, H, W, *m, FC.random_frame(1, H, W, fmt, seed=s)) for s, m in enumerate(ALIGNED)]
        big = lambda size: dict(size=size, O=0, sxt=3 * size * size, sxc=size * size, sxh=size)                         # noqa: E731
        bads = [dict(T=96), dict(T=0), big(4096), dict(O=6), dict(O=36), dict(O=-4), dict(fmt=3), dict(fmt=-1), dict(range=2), dict(range=-1),
                dict(n_jobs=0), dict(n_jobs=-1), dict(n_frames=0), dict(n_frames=-1), dict(nbytes=L.pc_clip_rate_workspace_size(T, 5) - 1),
                dict(x=None), dict(frames_host=None), dict(frames_dev=None), dict(jobs=None), dict(ws=None), dict(out=None), dict(H=0)]
        if fmt == "p010":
            bads.append(big(2048))
        for kw in bads:
            kw = dict(kw)
            size = kw.pop("size", T)
            rc, buf, ws_ok = jobs_raw(x, H, W, kw.pop("O", O), fmt, "limited", "bt709", table, jobs, size, over=kw)
            torch.cuda.synchronize()
            assert rc == -1 and (buf == POISON64).all() and ws_ok, (fmt, kw)
        rc, buf, ws_ok = jobs_raw(x, H, W, O, fmt, "limited", "bt709", table, jobs)                                    # unspoilt, it goes through
        assert rc == 0 and ws_ok and (buf[1:-1] != POISON64).all() and (buf[0] == POISON64).all() and (buf[-1] == POISON64).all()
    with pytest.raises(cr.ClipRateError, match="PC_ERR_ARG"):
        raise cr.ClipRateError(-1, "pc_clip_rate_sse_jobs")


@pytest.mark.parametrize("fmt", ["nv12", "p010"])
def test_the_largest_weights_meet_the_largest_error(fmt):
    H, W, size, O = 200, 250, 128, 64                                  # S = 64: 3 x 3 tiles, every interior pixel in a band
    assert TC.grid(H, W, size, O) == (3, 3)
    f, eY, eC = saturated(H, W, fmt)
    other = FC.random_frame(1, H, W, fmt, seed=8)
    jobs = [(1, t) for t in (4, 8, 0, 3, 7, 1, 5, 2, 6)] + [(0, 4)]
    x_np = np.zeros((len(jobs), 3, size, size), np.float32)
    every = QC.tile_sse(x_np[:9], H, W, size, O, fmt, "bt709", "full", f)
    want = [every[t] for _, t in jobs[:9]] + QC.tile_sse(x_np[:1], H, W, size, O, fmt, "bt709", "full", other, first_tile=4)
    assert want == RC2.job_sse(x_np, [other, f], jobs, H, W, size, O, fmt, "bt709", "full")
    den = RC.den_of(O)
    Hc, Wc = FC.chroma_size(H, W)
    assert sum(w[0] for w in want[:9]) == eY * eY * den * den * H * W                                 # the weights partition den^2 per sample
    assert sum(w[1] for w in want[:9]) == sum(w[2] for w in want[:9]) == eC * eC * den * den * Hc * Wc
    assert want[0][0] == eY * eY * int(RC.weights_int(1, 3, size, O).sum()) ** 2
    assert want[0][1] == eC * eC * sum(QC.chroma_weights(1, 3, size, O)) ** 2
    for modes, variant in [(ALIGNED, "contiguous"), (ALIGNED, "odd"), (MIXED, "contiguous")]:
        x = float_tiles(x_np, variant, size)
        table = [views(fmt, H, W, *m, fr) for m, fr in zip(modes, (other, f))]
        assert CR().plan(x, table, fmt, overlap=O) is (variant == "contiguous" and modes is ALIGNED)
        rc, buf, ws_ok = jobs_raw(x, H, W, O, fmt, "full", "bt709", table, jobs, size)
        assert rc == 0 and ws_ok
        check_out(buf, want, (variant, modes))


def test_offsets_past_2_to_the_31():
    """two jobs whose tiles lie a tile stride past 2^31 bytes apart, the second against a frame whose last luma rows lie past 2^31
    bytes, inside one untouched allocation: every offset is 64-bit, the job's tile offset and the table's frame included"""
    cr = CR()
    BIG = 2 ** 31 + 4096                                                   # tile stride in bytes
    ROW = 2 ** 26 + 64                                                     # luma row stride in bytes: row 32 starts past 2^31
    need = 2 * BIG + (16 << 20)
    free_mem = torch.cuda.mem_get_info(DEV)[0]
    if free_mem < need + (1 << 30):
        pytest.skip(f"{free_mem >> 20} MiB of device memory free, the strided views need {need >> 20} MiB")
    buf = torch.empty(need, dtype=torch.uint8, device=DEV)
    H, W, O = 40, 100, 0                                                   # 1 x 2 tiles
    fr = [FC.random_frame(1, H, W, "nv12", seed=31 + s) for s in range(2)]
    y = torch.as_strided(buf, (1, H, W), (H * ROW, ROW, 1), 8 << 20)
    y.copy_(torch.from_numpy(fr[1][0]))
    table = [[torch.from_numpy(p).to(DEV) for p in fr[0]], [y, torch.from_numpy(fr[1][1]).to(DEV)]]
    assert 39 * ROW > 2 ** 31
    jobs = [(0, 1), (1, 1)]
    x_np = TC.hostile_tiles(2, T, seed=32)
    want = RC2.job_sse(x_np, fr, jobs, H, W, T, O, "nv12", "bt709", "limited")
    xv = torch.as_strided(buf.view(torch.float32), (2, 3, T, T), (BIG // 4, T * T, T, 1), (1 << 20) // 4)
    xv.copy_(torch.from_numpy(x_np))
    assert cr.plan(xv, table, "nv12")
    rc, out, ws_ok = jobs_raw(xv, H, W, O, "nv12", "limited", "bt709", table, jobs)
    assert rc == 0 and ws_ok
    check_out(out, want, "wide")
    odd = torch.as_strided(buf.view(torch.float32), (2, 3, T, T), (BIG // 4, T * T, T, 1), (4 << 20) // 4 + 1)      # apart from xv and y
    odd.copy_(torch.from_numpy(x_np))
    assert not cr.plan(odd, table, "nv12")
    rc, out, ws_ok = jobs_raw(odd, H, W, O, "nv12", "limited", "bt709", table, jobs)
    assert rc == 0 and ws_ok
    check_out(out, want, "narrow")
    assert cr.tile_distortion_jobs(xv, cr.grid_of(H, W, T, O), [tuple(t[0] for t in ts) for ts in table], jobs, "nv12").tolist() == want


# -- through the codec ---------------------------------------------------------------------------------------------------------------

QUALITIES = [0, 0.5, 10]
H0, W0 = 100, 150                                                          # 2 x 3 tiles of 64 x 64, with and without overlap
N = 6
CASES = [(fmt, O) for fmt in ("nv12", "p010") for O in (0, 16)]


def device_clip(fmt):
    return [tuple(torch.from_numpy(p[0]).to(DEV) for p in f) for f in clip_of(fmt)]


def encode(fmt, O, frames, target, **kw):
    return CR().encode_clip_to_size(gpu_codec(), frames, QUALITIES, target, fmt, tile=T, overlap=O, mask_pol=POL, **kw)


@functools.lru_cache(maxsize=None)
def free(fmt, O):
    """the clip without a budget to speak of: (bytes, plan); the plan's tables do not depend on the budget"""
    return encode(fmt, O, device_clip(fmt), 10 ** 9)


def fixed_of(F):
    return 42 + 16 * F * N


def bounds(plan, F):
    return fixed_of(F) + sum(min(r) for r in plan.rates), fixed_of(F) + sum(max(r) for r in plan.rates)


@functools.lru_cache(maxsize=None)
def alone(fmt, O, f, t, l):
    """tile t of frame f cut and coded alone at level l, and the model's own output for it decoded alone"""
    from progressivecodec_amd import container, frame_tiles
    net = gpu_codec()
    x, _ = frame_tiles.cut_frame(device_clip(fmt)[f], fmt, tile=T, overlap=O, rect=(t // 3, t % 3, 1, 1))
    datas = net.compress_levels(x, [QUALITIES[l]], mask_pol=POL)
    b = container.pack([datas[0]["strings"]], datas[0]["shape"], [float(QUALITIES[l])], image_size=(T, T), mask_pol=POL)
    strings, shape, qs, _, pol = container.unpack(b, levels=[0])
    return b, net.decompress(strings[0], shape, qs[0], pol)["x_hat"][0]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("fmt,O", CASES)
def test_encode_clip_to_size_and_decode_clip(fmt, O):
    from progressivecodec_amd import container, frame_rate, frame_tiles
    cr = CR()
    net = gpu_codec()
    clip = clip_of(fmt)
    F = len(clip)
    frames = device_clip(fmt)
    g = cr.grid_of(H0, W0, T, O)
    free_buf, plan0 = free(fmt, O)
    # the source table, the items and the weights are the restatement's
    source = CC.source_table(clip, fmt, T, O, "linear")
    items, runs = RC2.items_of(source)
    weights = RC2.weights(source)
    assert plan0.source == source and plan0.items == items and plan0.weights == weights == [len(r) for r in runs]
    assert (plan0.n_coded, plan0.n_reused) == (len(items), F * N - len(items)) and 6 < len(items) < F * N and plan0.den == (2 * O if O else 1)
    # rates and dists are those of the tile cut, coded and decoded alone, measured against the frame it was coded for
    rates, dists, pd = plan0.rates, plan0.dists, plan0.plane_dists
    assert len(rates) == len(dists) == len(pd) == len(items) and all(len(r) == 3 for r in rates + dists + pd)
    for i, (f, t) in enumerate(items):
        for l in range(3):
            b, x = alone(fmt, O, f, t, l)
            assert rates[i][l] == len(b), (i, l)
            assert pd[i][l] == frame_rate.frame_tile_distortion(x[None], g, frames[f], fmt, first_tile=t).tolist()[0], (i, l)
            assert dists[i][l] == sum(pd[i][l])
    lo, hi = bounds(plan0, F)
    assert lo < hi
    with pytest.raises(ValueError, match=rf"\b{lo}\b"):
        encode(fmt, O, frames, lo - 1)
    other = "nv12" if fmt == "p010" else "p010"
    for target in (lo, lo + (hi - lo) // 3, lo + 2 * (hi - lo) // 3, hi):
        buf, plan = encode(fmt, O, frames, target)
        assert isinstance(buf, bytes) and len(buf) == plan.container_bytes <= target, target
        assert (plan.source, plan.items, plan.weights, plan.rates, plan.dists, plan.plane_dists) == (source, items, weights, rates, dists, pd)
        levels = plan.levels
        assert levels == RC.allocate(rates, dists, RC2.budget(target, F, N), weights), target
        assert len(buf) == RC2.container_bytes(rates, levels, F, N)
        assert plan.sse == RC2.frame_sse(source, pd, levels) and plan.predicted == RC2.predicted(source, dists, levels)
        blobs = [[alone(fmt, O, f, t, levels[items.index((f, t))])[0] if source[f][t] == f else None for t in range(N)] for f in range(F)]
        hd = cr.parse_clip(buf)
        assert buf == RC2.pack_clip(blobs, source, H0, W0, T, O, fmt, "bt709", "limited", "linear", hd["contract"])
        assert hd["contract"] == container.build_contract_id()
        if target == hi:
            assert all(dists[i][l] == min(dists[i]) for i, l in enumerate(levels)) and (buf, plan) == (free_buf, plan0)
        # every frame is decode_frame_tiled of its own container, bit for bit
        per_frame = [cr.frame_container(buf, k) for k in range(F)]
        want = [frame_tiles.decode_frame_tiled(net, b) for b in per_frame]
        assert all(same(a, b) for a, b in zip(cr.decode_clip(net, buf), want)), target
        decoded = lambda k: torch.stack([alone(fmt, O, source[k][t], t, levels[items.index((source[k][t], t))])[1] for t in range(N)])   # noqa: E731
        if O == 0:                                                         # the plan's table is the decoded frame's exact per-plane SSE
            for k in range(F):
                assert frame_tiles.stitch_frame(decoded(k), g, fmt, ref=frames[k], image=False).sse[0].tolist() == plan.sse[k], (target, k)
        if target == lo + 2 * (hi - lo) // 3:
            for k in range(F):
                assert same(cr.decode_clip(net, buf, frames=[k], level=0)[0], want[k]), k
            for dkw in [dict(region=(40, 90, 30, 30)), dict(level=0, region=(60, 60, 8, 8), fmt=other), dict(max_tiles_per_call=1),
                        dict(max_tiles_per_call=4)]:
                got = cr.decode_clip(net, buf, **dkw)
                assert all(same(a, frame_tiles.decode_frame_tiled(net, b, **dkw)) for a, b in zip(got, per_frame)), dkw
            part = cr.decode_clip(net, buf, frames=[3, 1, 1], max_tiles_per_call=1)
            assert len(part) == 3 and same(part[0], want[3]) and same(part[1], want[1]) and same(part[2], want[1])
            # the reuse identity: a reused item's decoded tile leaves the same three sums in every frame that shows it
            for i, ((f, t), run) in enumerate(zip(items, runs)):
                x = alone(fmt, O, f, t, levels[i])[1][None]
                for k in run:
                    assert frame_rate.frame_tile_distortion(x, g, frames[k], fmt, first_tile=t).tolist()[0] == pd[i][levels[i]], (i, k)
            assert any(len(run) > 1 for run in runs)
    with pytest.raises(container.ContainerError, match="level must be -1 or 0"):
        cr.decode_clip(net, free_buf, level=1)


@pytest.mark.parametrize("fmt,O", CASES)
def test_bytes_and_plan_do_not_depend_on_the_layout(fmt, O):
    clip = clip_of(fmt)
    frames = device_clip(fmt)
    lo, hi = bounds(free(fmt, O)[1], len(clip))
    target = lo + (hi - lo) // 3
    buf, plan = encode(fmt, O, frames, target)
    for per_call in (1, 4, 32):
        assert encode(fmt, O, frames, target, max_tiles_per_call=per_call) == (buf, plan), per_call
    batched = tuple(torch.stack(ps) for ps in zip(*frames))
    assert encode(fmt, O, batched, target) == (buf, plan)
    pitched = [tuple(v[0] for v in views(fmt, H0, W0, "loose", 1, f)) for f in clip]
    assert encode(fmt, O, pitched, target, max_tiles_per_call=4) == (buf, plan)


@pytest.mark.parametrize("fmt,O", CASES)
def test_a_clip_of_one_frame_is_the_frame_call(fmt, O):
    """the clip's fixed overhead is 42 + 16 n bytes, the frame's 43 with the 16 in its rates: at target and target + 1 the allocator
    sees the same problem"""
    from progressivecodec_amd import frame_rate
    cr = CR()
    frame = device_clip(fmt)[0]
    fbuf0, fplan0 = frame_rate.encode_frame_tiled_to_size(gpu_codec(), frame, QUALITIES, 10 ** 9, fmt, tile=T, overlap=O, mask_pol=POL)
    lo, hi = 43 + sum(min(r) for r in fplan0.rates), 43 + sum(max(r) for r in fplan0.rates)
    for target in (lo - 1, (lo + hi) // 2 - 1, hi - 1):
        buf, plan = encode(fmt, O, [frame], target)
        fbuf, fplan = frame_rate.encode_frame_tiled_to_size(gpu_codec(), frame, QUALITIES, target + 1, fmt, tile=T, overlap=O, mask_pol=POL)
        assert cr.frame_container(buf, 0) == fbuf, target
        assert plan.levels == fplan.levels and plan.plane_dists == fplan.plane_dists and plan.sse == [fplan.sse]
        assert plan.rates == [[v - 16 for v in r] for r in fplan.rates] and len(buf) == len(fbuf) - 1
        assert plan.source == [[0] * N] and plan.items == [(0, t) for t in range(N)] and plan.weights == [1] * N
    with pytest.raises(ValueError, match=rf"\b{lo - 1}\b"):
        encode(fmt, O, [frame], lo - 2)


@pytest.mark.parametrize("fmt,O", CASES)
def test_a_static_clip(fmt, O):
    cr = CR()
    frame = device_clip(fmt)[0]
    still = [frame] * 3
    big, plan_big = encode(fmt, O, still, 10 ** 9)
    assert plan_big.source == [[0] * N] * 3 and plan_big.items == [(0, t) for t in range(N)] and plan_big.weights == [3] * N
    assert (plan_big.n_coded, plan_big.n_reused) == (N, 2 * N)
    lo, hi = bounds(plan_big, 3)
    for target in (lo, (lo + hi) // 2):
        buf, plan = encode(fmt, O, still, target)
        single, splan = encode(fmt, O, [frame], target - 16 * 2 * N)
        assert plan.levels == splan.levels and plan.rates == splan.rates and plan.plane_dists == splan.plane_dists
        assert plan.sse == splan.sse * 3 and plan.predicted == 3 * splan.predicted
        # a uniform scale of the importance changes nothing
        assert encode(fmt, O, still, target, importance=[7] * N) == (buf, plan._replace(weights=[21] * N))
        assert encode(fmt, O, still, target, frame_weights=[Fraction(1, 3)] * 3)[0] == buf
        # the payload is stored once: three equal rows of the table in front of the single frame's payload
        hd, hs = cr.parse_clip(buf), cr.parse_clip(single)
        assert hd["table"][0] == hd["table"][1] == hd["table"][2] and len(buf) == len(single) + 16 * 2 * N == RC2.container_bytes(plan.rates, plan.levels, 3, N)
        assert buf[hd["payload_start"]:] == single[hs["payload_start"]:]
        assert all(cr.frame_container(buf, k) == cr.frame_container(single, 0) for k in range(3))
    # without reuse: eighteen items of weight 1, every tile stored again
    target = (lo + hi) // 2 + 2 * (hi - fixed_of(3))
    every, plan_all = encode(fmt, O, still, target, reuse=False)
    assert plan_all.source == [[f] * N for f in range(3)] and plan_all.items == [(f, t) for f in range(3) for t in range(N)]
    assert plan_all.weights == [1] * 18 and (plan_all.n_coded, plan_all.n_reused) == (18, 0) and len(every) == plan_all.container_bytes <= target
    assert plan_all.rates == plan_big.rates * 3 and plan_all.plane_dists == plan_big.plane_dists * 3
    assert plan_all.levels == RC.allocate(plan_all.rates, plan_all.dists, RC2.budget(target, 3, N), [1] * 18)


@pytest.mark.parametrize("fmt,O", CASES)
def test_frame_weights_and_importance_are_passed_on(fmt, O):
    clip = clip_of(fmt)
    F = len(clip)
    frames = device_clip(fmt)
    plan0 = free(fmt, O)[1]
    lo, hi = bounds(plan0, F)
    target = lo + (hi - lo) // 3
    fw = [Fraction(1, 3), 2, 5, 1, 7][:F]
    imp = [1, 1, Fraction(1, 1000), 1, 10 ** 6, 1]
    for kw in (dict(frame_weights=fw), dict(importance=imp), dict(importance=[imp[:3], imp[3:]], frame_weights=fw), dict(plane_weights=(1, 0, 0))):
        plan = encode(fmt, O, frames, target, **kw)[1]
        flat = kw.get("importance")
        flat = [v for row in flat for v in row] if flat and isinstance(flat[0], list) else flat
        weights = RC2.weights(plan0.source, flat, kw.get("frame_weights"))
        pw = kw.get("plane_weights", (1, 1, 1))
        dists = [[sum(w * v for w, v in zip(pw, row)) for row in item] for item in plan0.plane_dists]
        assert plan.weights == weights and plan.rates == plan0.rates and plan.plane_dists == plan0.plane_dists and plan.dists == dists
        assert plan.levels == RC.allocate(plan0.rates, dists, RC2.budget(target, F, N), weights), kw
        assert plan.container_bytes <= target

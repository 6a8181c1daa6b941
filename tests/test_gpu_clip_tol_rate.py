"""Tolerant rate-controlled clips on the GPU (progressivecodec_amd/clip_tol_rate.py, libpc_clip_tol_rate.so) against their restatement
(tests/clip_tol_rate_contract.py): the distortion sums of decoded tiles against every frame of their runs exactly, on both access
paths, against tests/clip_rate_contract.job_sse and against clip_rate.tile_distortion_jobs of the expanded job list with the tile
repeated; and encode_clip_to_size through the codec into a PCS2 container that clip_rate's decoders read.  Every comparison is exact
equality of integers, bits or bytes.  T = 64 throughout (one case at 128, one at 576): the smallest tile, so that the frames stay small
while every branch is taken; the largest tiles, the later trips of the final and the long runs are in tests/test_gpu_image_limits.py."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import clip_rate_contract as RC2
from tests import clip_tol_contract as TOL
from tests import clip_tol_rate_contract as TRC
from tests import frames_contract as FC
from tests import rate_contract as RC
from tests import tiles_contract as TC
from tests.test_gpu_clip_rate import ALIGNED, MIXED
from tests.test_gpu_clips import clip_of, views
from tests.test_gpu_frame_rate import codec_frame, saturated
from tests.test_gpu_rate import POISON64, check_out, float_tiles
from tests.util import gpu_codec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POL = "point-based-std"
T = 64
SIZES = [(65, 63), (100, 150), (127, 129)]
OVERLAPS = [0, 4, 16, 32]
BAND_OVERLAPS = [24, 28]                                                    # 2 O is no power of two (tests/band_cases.py)
MATS = list(FC.MATRICES)


def CTR():
    from progressivecodec_amd import clip_tol_rate
    return clip_tol_rate


def CR():
    from progressivecodec_amd import clip_rate
    return clip_rate


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def runs_raw(x, H, W, O, fmt, rng, matrix, table, tile_ids, runs, size=T, over=None, dev_offsets=None):
    """pc_clip_tol_rate_sse_runs on the tiles x holds, the tiles and slots written to the device as they are -> (status, the
    [n_entries + 2, 3] buffer whose rows 1 .. n_entries are `out`, poisoned beforehand, whether every partial of the workspace and no
    word after it was written -- or, for a refused call, none at all).  table: per frame the list of batched plane tensors.  over:
    arguments to replace, by name.  dev_offsets: what the device's copy of the offsets holds instead of the host's."""
    from progressivecodec_amd import frames
    L = CTR().lib()
    n = len(tile_ids)
    off = TRC.offsets_of(runs)
    ne = off[-1]
    buf = torch.full((ne + 2, 3), POISON64, dtype=torch.int64, device=DEV)
    need = L.pc_clip_tol_rate_workspace_size(size, ne)
    assert need == (TRC.workspace_size(size, ne) if size <= 2048 else 0)
    ws = torch.full((need // 8 + 1,), POISON64, dtype=torch.int64, device=DEV)
    k = frames.coefficients(matrix)
    host = (frames.Frame * len(table))(*[frames._frame_struct(list(ts)) for ts in table])
    dtab = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(DEV)
    dtiles = torch.tensor(tile_ids, dtype=torch.int32).to(DEV)
    doff = torch.tensor(off if dev_offsets is None else dev_offsets, dtype=torch.int32).to(DEV)
    dslots = torch.tensor([s for run in runs for s in run], dtype=torch.int32).to(DEV)
    a = dict(x=x.data_ptr(), sxt=x.stride(0), sxc=x.stride(1), sxh=x.stride(2), H=H, W=W, T=size, O=O, fmt=frames.FORMATS.get(fmt, fmt),
             range=frames.RANGES.get(rng, rng), kr=k.kr, kg=k.kg, kb=k.kb, ib=k.ib, ir=k.ir, frames_host=host, frames_dev=dtab.data_ptr(),
             n_frames=len(table), tiles=dtiles.data_ptr(), offsets_host=(C.c_int32 * (n + 1))(*off), offsets_dev=doff.data_ptr(),
             slots=dslots.data_ptr(), n_jobs=n, n_entries=ne, ws=ws.data_ptr(), nbytes=need, out=buf[1:].data_ptr(), stream=stream())
    a.update(over or {})
    rc = L.pc_clip_tol_rate_sse_runs(*a.values())
    h = ws.cpu()
    return rc, buf, bool(h[-1] == POISON64 and ((h[:-1] != POISON64).all() if rc == 0 else (h == POISON64).all()))


def run_list(n, seed):
    """jobs over three frames: run lengths 1, 2 and 3 in mixed order, every tile of the grid in descending order, a tile repeated
    across jobs, and a frame repeated inside a run"""
    g = np.random.default_rng(seed)
    patterns = [[2], [0, 1], [1, 2, 0], [1, 1], [2, 0, 2], [0]]
    tile_ids = list(reversed(range(n))) + [0, n - 1, 0, int(g.integers(0, n)), int(g.integers(0, n))]
    runs = [patterns[(m + seed) % 6] for m in range(len(tile_ids))]
    runs[n], runs[n + 2] = [1, 2, 0], [2, 2]                                          # tile 0 twice, with different runs
    assert {len(r) for r in runs} == {1, 2, 3} and tile_ids[n] == tile_ids[n + 2]
    return tile_ids, runs


def expanded_on_the_gpu(x, g, planes, tile_ids, runs, fmt, matrix, rng):
    """the sequence the run kernel replaces: the tile of every entry repeated, one clip_rate job per entry"""
    jobs, owner = TRC.expanded(tile_ids, runs)
    rep = x.index_select(0, torch.tensor(owner, device=DEV))
    return CR().tile_distortion_jobs(rep, g, planes, jobs, fmt, matrix, rng).tolist()


def kernel_matrix(hw, overlaps):
    """every overlap x format x range against the restatement and against clip_rate.tile_distortion_jobs of the expanded job list; a
    table of three frames with different contents, once all aligned (wide where the floats and the overlap allow it) and once with
    mixed pitches and an offset pointer (narrow); the Python call on a list, on batched planes and on a side stream."""
    ctr = CTR()
    H, W = hw
    seen = set()
    for O in overlaps:
        ny, nx = TC.grid(H, W, T, O)
        n = ny * nx
        tile_ids, runs = run_list(n, H + W + O)
        off = TRC.offsets_of(runs)
        x_np = TC.hostile_tiles(len(tile_ids), T, seed=H + W + O)
        xs = {v: float_tiles(x_np, v) for v in ("contiguous", "odd")}
        g = ctr.grid_of(H, W, T, O)
        for k, fmt in enumerate(FC.FORMATS):
            fr = [FC.random_frame(1, H, W, fmt, seed=1000 * H + W + O + 10 * k + s) for s in range(3)]
            tables = {"aligned": [views(fmt, H, W, *m, f) for m, f in zip(ALIGNED, fr)], "mixed": [views(fmt, H, W, *m, f) for m, f in zip(MIXED, fr)]}
            planes = [tuple(torch.from_numpy(p[0]).to(DEV) for p in f) for f in fr]
            for rng in FC.RANGES:
                matrix = MATS[(k + O // 4 + (rng == "full")) % 3]
                want = TRC.run_sse(x_np, fr, tile_ids, runs, H, W, T, O, fmt, matrix, rng)
                assert len(want) == off[-1]
                assert expanded_on_the_gpu(xs["contiguous"], g, planes, tile_ids, runs, fmt, matrix, rng) == want
                for tname, variant in (("aligned", "contiguous"), ("mixed", "contiguous"), ("aligned", "odd"), ("mixed", "odd")):
                    expect = tname == "aligned" and variant == "contiguous" and O % 8 == 0
                    wide = ctr.plan(xs[variant], tables[tname], fmt, overlap=O)
                    case = (H, W, O, fmt, rng, tname, variant)
                    assert wide is expect, case
                    assert wide is CR().plan(xs[variant], tables[tname], fmt, overlap=O)
                    seen.add(wide)
                    rc, buf, ws_ok = runs_raw(xs[variant], H, W, O, fmt, rng, matrix, tables[tname], tile_ids, runs)
                    assert rc == 0 and ws_ok, case
                    check_out(buf, want, case)
                if rng == "limited":
                    # a sub-list, and one job alone, on either path
                    for tname, variant in (("aligned", "contiguous"), ("mixed", "odd")):
                        rc, buf, ws_ok = runs_raw(xs[variant][1:n + 2], H, W, O, fmt, rng, matrix, tables[tname], tile_ids[1:n + 2], runs[1:n + 2])
                        assert rc == 0 and ws_ok
                        check_out(buf, want[off[1]:off[n + 2]], (H, W, O, fmt, tname, "sub-list"))
                        rc, buf, ws_ok = runs_raw(xs[variant][n:n + 1], H, W, O, fmt, rng, matrix, tables[tname], tile_ids[n:n + 1], runs[n:n + 1])
                        assert rc == 0 and ws_ok
                        check_out(buf, want[off[n]:off[n + 1]], (H, W, O, fmt, tname, "alone"))
                else:
                    # the Python call: a list of pitched frames; batched planes; channels last in memory (copied); a side stream
                    got, goff = ctr.tile_distortion_runs(xs["odd"], g, [tuple(v[0] for v in ts) for ts in tables["mixed"]], tile_ids, runs, fmt, matrix, rng)
                    assert got.dtype == torch.int64 and got.shape == (off[-1], 3) and got.device.type == "cuda" and got.tolist() == want and goff == off
                    batched = tuple(torch.stack(ps) for ps in zip(*planes))
                    cl = xs["contiguous"].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
                    assert ctr.tile_distortion_runs(cl, g, batched, torch.tensor(tile_ids), [tuple(r) for r in runs], fmt, matrix, rng)[0].tolist() == want
                    side = torch.cuda.Stream(DEV)
                    side.wait_stream(torch.cuda.current_stream(DEV))
                    with torch.cuda.stream(side):
                        got_s = ctr.tile_distortion_runs(xs["contiguous"][-2:], g, planes, tile_ids[-2:], runs[-2:], fmt, matrix, rng)[0]
                    side.synchronize()
                    assert got_s.tolist() == want[off[-3]:]
    assert seen == {True, False}


@pytest.mark.parametrize("hw", SIZES)
def test_kernel_matrix_exact_on_both_paths(hw):
    kernel_matrix(hw, OVERLAPS)


def test_kernel_matrix_at_overlaps_whose_band_quotients_are_no_floats():
    """O = 24 (S = 40, den = 48: the wide path where there is one) and O = 28 (S = 36, den = 56: narrow at 4:2:0) on one picture.  The
    sums weigh with the integer numerators 2u + 1, which are exact whatever 2 O is; what is new is the band geometry."""
    kernel_matrix((100, 150), BAND_OVERLAPS)


@pytest.mark.parametrize("fmt", ["nv12", "p010"])
def test_four_blocks_per_job_at_128(fmt):
    H, W, size, O = 200, 250, 128, 16                                      # 2 x 3 tiles, S = 112
    assert TC.grid(H, W, size, O) == (2, 3)
    fr = [FC.random_frame(1, H, W, fmt, seed=128 + s) for s in range(3)]
    tile_ids, runs = [5, 0, 4, 5], [[0, 2], [1], [2, 1, 0], [1, 1]]
    x_np = TC.hostile_tiles(4, size, seed=128)
    want = TRC.run_sse(x_np, fr, tile_ids, runs, H, W, size, O, fmt, "bt709", "limited")
    for modes, variant in [(ALIGNED, "contiguous"), (MIXED, "odd")]:
        x = float_tiles(x_np, variant, size)
        table = [views(fmt, H, W, *m, f) for m, f in zip(modes, fr)]
        assert CTR().plan(x, table, fmt, overlap=O) is (variant == "contiguous")
        rc, buf, ws_ok = runs_raw(x, H, W, O, fmt, "limited", "bt709", table, tile_ids, runs, size)
        assert rc == 0 and ws_ok
        check_out(buf, want, (fmt, variant))


def test_six_trips_of_the_final_at_576():
    """T = 576: 81 blocks per job, 324 wave partials per entry, so the final's 64 lanes make six trips (the last one partial)"""
    H, W, size, O, fmt = 600, 700, 576, 0, "nv12"
    assert TC.grid(H, W, size, O) == (2, 2) and 4 * (size * size // 4096) == 324
    fr = [FC.random_frame(1, H, W, fmt, seed=576 + s) for s in range(2)]
    tile_ids, runs = [3, 0], [[1, 0], [0, 1]]
    x_np = TC.hostile_tiles(2, size, seed=576)
    want = TRC.run_sse(x_np, fr, tile_ids, runs, H, W, size, O, fmt, "bt709", "limited")
    table = [views(fmt, H, W, *m, f) for m, f in zip(ALIGNED, fr)]
    x = float_tiles(x_np, "contiguous", size)
    assert CTR().plan(x, table, fmt, overlap=O)
    rc, buf, ws_ok = runs_raw(x, H, W, O, fmt, "limited", "bt709", table, tile_ids, runs, size)
    assert rc == 0 and ws_ok
    check_out(buf, want, "576")
    planes = [tuple(torch.from_numpy(p[0]).to(DEV) for p in f) for f in fr]
    assert expanded_on_the_gpu(x, CTR().grid_of(H, W, size, O), planes, tile_ids, runs, fmt, "bt709", "limited") == want


@pytest.mark.parametrize("fmt", ["nv12", "i420", "p010"])
def test_entries_out_of_range_give_zeros_and_touch_nothing(fmt):
    """an entry whose slot is -1 or n_frames, a job whose tile is -1 or ny * nx (and the far ends of int32), written straight through
    the C call: 0, 0, 0 for exactly those rows, their neighbours intact, every partial written, nothing outside out or the workspace;
    and device offsets beyond [0, n_entries] are clamped"""
    ctr = CTR()
    H, W = 100, 150
    for O in (0, 16):
        n = 6
        fr = [FC.random_frame(1, H, W, fmt, seed=40 + s + O) for s in range(3)]
        tile_ids = [4, -1, 5, n, 2, 2 ** 31 - 1, -2 ** 31, 3, 0]
        runs = [[1, -1, 0], [0, 1], [3, 2], [0], [2 ** 31 - 1, 2, -2 ** 31], [1], [2, 0], [0, 3, 1], [-1]]
        x_np = TC.hostile_tiles(len(tile_ids), T, seed=O + 9)
        jobs, owner = TRC.expanded(tile_ids, runs)
        valid = [e for e, (f, t) in enumerate(jobs) if 0 <= f < 3 and 0 <= t < n]
        assert valid == [0, 2, 6, 9, 14, 16]
        full = RC2.job_sse(x_np[[owner[e] for e in valid]], fr, [jobs[e] for e in valid], H, W, T, O, fmt, "bt709", "limited")
        want = [[0, 0, 0]] * len(jobs)
        for e, row in zip(valid, full):
            want[e] = row
            assert any(row)
        off = TRC.offsets_of(runs)
        for modes, variant in ((ALIGNED, "contiguous"), (MIXED, "odd")):
            table = [views(fmt, H, W, *m, f) for m, f in zip(modes, fr)]
            x = float_tiles(x_np, variant)
            assert ctr.plan(x, table, fmt, overlap=O) is (variant == "contiguous")
            rc, buf, ws_ok = runs_raw(x, H, W, O, fmt, "limited", "bt709", table, tile_ids, runs)
            assert rc == 0 and ws_ok
            check_out(buf, want, (fmt, O, variant))
            # what the device's offsets hold beyond [0, n_entries] is clamped: the same entries, nothing outside
            rc, buf, ws_ok = runs_raw(x, H, W, O, fmt, "limited", "bt709", table, tile_ids, runs, dev_offsets=[-7] + off[1:-1] + [2 ** 31 - 1])
            assert rc == 0 and ws_ok
            check_out(buf, want, (fmt, O, variant, "clamped"))


def test_refused_calls_launch_nothing():
    ctr = CTR()
    L = ctr.lib()
    H, W, O = 100, 150, 16
    tile_ids, runs = [5, 0, 3, 0, 2], [[1], [0, 2], [2, 1, 0], [0], [1, 1]]
    x = torch.rand(len(tile_ids), 3, T, T, device=DEV)
    off = lambda *v: (C.c_int32 * len(v))(*v)                                         # noqa: E731
    for fmt in ("nv12", "p010"):
        table = [views(fmt, H, W, *m, FC.random_frame(1, H, W, fmt, seed=s)) for s, m in enumerate(ALIGNED)]
        big = lambda size: dict(size=size, O=0, sxt=3 * size * size, sxc=size * size, sxh=size)                         # noqa: E731
        bads = [dict(T=96), dict(T=0), big(4096), dict(O=6), dict(O=36), dict(O=-4), dict(fmt=3), dict(fmt=-1), dict(range=2), dict(range=-1),
                dict(n_jobs=0), dict(n_jobs=-1), dict(n_entries=0), dict(n_entries=4), dict(n_entries=10), dict(n_frames=0), dict(n_frames=-1),
                dict(nbytes=L.pc_clip_tol_rate_workspace_size(T, 9) - 1),
                dict(offsets_host=off(1, 1, 3, 6, 7, 9)), dict(offsets_host=off(0, 1, 1, 6, 7, 9)), dict(offsets_host=off(0, 1, 3, 6, 7, 8)),
                dict(offsets_host=off(0, 3, 1, 6, 7, 9)), dict(offsets_host=None),
                dict(x=None), dict(frames_host=None), dict(frames_dev=None), dict(tiles=None), dict(offsets_dev=None), dict(slots=None),
                dict(ws=None), dict(out=None), dict(H=0)]
        if fmt == "p010":
            bads.append(big(2048))
        for kw in bads:
            kw = dict(kw)
            size = kw.pop("size", T)
            rc, buf, ws_ok = runs_raw(x, H, W, kw.pop("O", O), fmt, "limited", "bt709", table, tile_ids, runs, size, over=kw)
            torch.cuda.synchronize()
            assert rc == -1 and (buf == POISON64).all() and ws_ok, (fmt, kw)
        rc, buf, ws_ok = runs_raw(x, H, W, O, fmt, "limited", "bt709", table, tile_ids, runs)                          # unspoilt, it goes through
        assert rc == 0 and ws_ok and (buf[1:-1] != POISON64).all() and (buf[0] == POISON64).all() and (buf[-1] == POISON64).all()
    with pytest.raises(ctr.ClipTolRateError, match="PC_ERR_ARG"):
        raise ctr.ClipTolRateError(-1, "pc_clip_tol_rate_sse_runs")


@pytest.mark.parametrize("fmt", ["nv12", "p010"])
def test_the_largest_weights_meet_the_largest_error_twice(fmt):
    """the saturated frame twice in every run: both entries are the largest sums the contract allows, and equal"""
    H, W, size, O = 200, 250, 128, 64                                  # S = 64: 3 x 3 tiles, every interior pixel in a band
    assert TC.grid(H, W, size, O) == (3, 3)
    f, eY, eC = saturated(H, W, fmt)
    other = FC.random_frame(1, H, W, fmt, seed=8)
    tile_ids = [4, 8, 0, 3, 7, 1, 5, 2, 6, 4]
    runs = [[1, 1]] * 9 + [[0, 1, 0]]
    x_np = np.zeros((len(tile_ids), 3, size, size), np.float32)
    want = TRC.run_sse(x_np, [other, f], tile_ids, runs, H, W, size, O, fmt, "bt709", "full")
    den = RC.den_of(O)
    Hc, Wc = FC.chroma_size(H, W)
    for j in (0, 1):
        assert sum(w[0] for w in want[j:18:2]) == eY * eY * den * den * H * W                         # the weights partition den^2 per sample
        assert sum(w[1] for w in want[j:18:2]) == sum(w[2] for w in want[j:18:2]) == eC * eC * den * den * Hc * Wc
    assert want[0] == want[1] == want[19] and want[18] == want[20] != want[19]
    assert want[0][0] == eY * eY * int(RC.weights_int(1, 3, size, O).sum()) ** 2
    for modes, variant in [(ALIGNED, "contiguous"), (ALIGNED, "odd"), (MIXED, "contiguous")]:
        x = float_tiles(x_np, variant, size)
        table = [views(fmt, H, W, *m, fr) for m, fr in zip(modes, (other, f))]
        assert CTR().plan(x, table, fmt, overlap=O) is (variant == "contiguous" and modes is ALIGNED)
        rc, buf, ws_ok = runs_raw(x, H, W, O, fmt, "full", "bt709", table, tile_ids, runs, size)
        assert rc == 0 and ws_ok
        check_out(buf, want, (variant, modes))


# -- through the codec ---------------------------------------------------------------------------------------------------------------

QUALITIES = [0, 0.5, 10]
H0, W0 = 100, 150                                                          # 2 x 3 tiles of 64 x 64, with and without overlap
N = 6
F = 5
CASES = [(fmt, O) for fmt in ("nv12", "p010") for O in (0, 16)]


@functools.lru_cache(maxsize=None)
def noisy_clip(fmt):
    """five frames: a smooth frame (its codes lie well inside the code range) with seeded noise of 0 / +1 on every sample of every
    frame, so that static tiles differ from frame to frame by at most one code, and a block that moves through the upper row of tiles"""
    g = np.random.default_rng(20)
    base = [np.array(c) for c in FC.codes(codec_frame(fmt), fmt)]
    s = 1 << (FC.bits(fmt) - 8)
    out = []
    for k in range(F):
        y, cb, cr = [c + g.integers(0, 2, c.shape) for c in base]
        y[0, 10:30, 10 + 25 * k:30 + 25 * k] = 200 * s
        cb[0, 5:15, (10 + 25 * k) // 2:(30 + 25 * k) // 2] = 90 * s
        out.append(FC.frame(y, cb, cr, fmt))
    return out


def device_frames(clip):
    return [tuple(torch.from_numpy(p[0]).to(DEV) for p in f) for f in clip]


def encode(fmt, O, frames, target, **kw):
    kw.setdefault("tolerance", CTR().Tolerance(max_abs=1))
    return CTR().encode_clip_to_size(gpu_codec(), frames, QUALITIES, target, fmt, tile=T, overlap=O, mask_pol=POL, **kw)


@functools.lru_cache(maxsize=None)
def free(fmt, O):
    """the noisy clip without a budget to speak of: (bytes, plan); the plan's tables do not depend on the budget"""
    return encode(fmt, O, device_frames(noisy_clip(fmt)), 10 ** 9)


def fixed_of(n_frames):
    return 42 + 16 * n_frames * N


def bounds(plan, n_frames):
    return fixed_of(n_frames) + sum(min(r) for r in plan.rates), fixed_of(n_frames) + sum(max(r) for r in plan.rates)


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def true_sse(decoded, frame, fmt):
    """per plane the squared error of a decoded frame (unbatched cuda planes) against a frame of the restatement, in the frames' codes"""
    got = FC.codes(tuple(p.cpu().numpy()[None] for p in decoded), fmt)
    return [int(((a - b) ** 2).sum()) for a, b in zip(got, FC.codes(frame, fmt))]


@pytest.mark.parametrize("fmt,O", CASES)
def test_encode_clip_to_size_on_a_noisy_clip(fmt, O):
    from progressivecodec_amd import container, frame_tiles
    ctr = CTR()
    net = gpu_codec()
    clip = noisy_clip(fmt)
    frames = device_frames(clip)
    free_buf, plan0 = free(fmt, O)
    # the source table is the tolerant scan's; the exact test reuses nothing on this clip
    source, stats = TOL.scan(clip, fmt, T, O, "linear", (1, 1, 1))
    assert plan0.source == source and plan0.stats == stats and plan0.worst == TOL.worst(source, stats) == [1, 1, 1]
    assert TOL.scan(clip, fmt, T, O, "linear")[0] == [[k] * N for k in range(F)]
    items, runs = RC2.items_of(source)
    assert (plan0.items, plan0.runs) == (items, runs) and (plan0.n_coded, plan0.n_reused) == (len(items), F * N - len(items))
    assert N < len(items) < F * N and max(len(r) for r in runs) == F and plan0.den == (2 * O if O else 1)
    assert plan0.weights == [1] * len(items) and plan0.frame_scale == 1
    rates, pd = plan0.rates, plan0.plane_dists
    assert len(rates) == len(pd) == len(items) and all(len(r) == 3 for r in rates) and all(len(v) == 3 for v in pd)
    assert all(len(per_frame) == len(run) and all(len(d) == 3 for d in per_frame) for row, run in zip(pd, runs) for per_frame in row)
    assert plan0.dists == TRC.dists(pd, runs)
    # a reused tile's error differs from frame to frame: the reuse identity of section 17 does not hold here
    assert any(len({tuple(d) for d in per_frame}) > 1 for row in pd for per_frame in row)
    lo, hi = bounds(plan0, F)
    assert lo < hi
    with pytest.raises(ValueError, match=rf"\b{lo}\b"):
        encode(fmt, O, frames, lo - 1)
    identity_differs = False
    for target in (lo, lo + (hi - lo) // 3, lo + 2 * (hi - lo) // 3, hi):
        buf, plan = encode(fmt, O, frames, target)
        assert isinstance(buf, bytes) and len(buf) == plan.container_bytes <= target, target
        assert (plan.source, plan.items, plan.runs, plan.weights, plan.rates, plan.dists, plan.plane_dists) == (source, items, runs, plan0.weights, rates, plan0.dists, pd)
        levels = plan.levels
        assert levels == RC.allocate(rates, plan.dists, RC2.budget(target, F, N), plan.weights), target
        assert len(buf) == TRC.container_bytes(rates, levels, F, N)
        assert plan.sse == TRC.frame_sse(source, pd, levels) and plan.predicted == TRC.predicted(pd, levels) == sum(sum(row) for row in plan.sse)
        if target == hi:
            assert (buf, plan) == (free_buf, plan0)
        # clip_rate's decoders read it: the table aliases exactly where the scan reused, every frame is decode_frame_tiled of its own
        hd = ctr.parse_clip(buf)
        assert hd["contract"] == container.build_contract_id() and hd["F"] == F and buf[:4] == b"PCS2"
        for k in range(F):
            for t in range(N):
                assert hd["table"][k][t] == hd["table"][source[k][t]][t]
                assert all((hd["table"][k][t] == hd["table"][j][t]) == (source[k][t] == source[j][t]) for j in range(F)), (k, t)
        got = ctr.decode_clip(net, buf)
        for k in range(F):
            assert same(got[k], frame_tiles.decode_frame_tiled(net, ctr.frame_container(buf, k))), (target, k)
        if O == 0:
            # the plan's table is the decoded frame's exact per-plane SSE against the frame that was shown
            for k in range(F):
                assert true_sse(got[k], clip[k], fmt) == plan.sse[k], (target, k)
            by_identity = [[sum(pd[items.index((source[k][t], t))][levels[items.index((source[k][t], t))]][0][p] for t in range(N)) for p in range(3)]
                           for k in range(F)]
            identity_differs = identity_differs or by_identity != plan.sse
    assert O != 0 or identity_differs


@pytest.mark.parametrize("fmt,O", CASES)
def test_bytes_and_plan_do_not_depend_on_the_layout(fmt, O):
    clip = noisy_clip(fmt)
    frames = device_frames(clip)
    lo, hi = bounds(free(fmt, O)[1], F)
    target = lo + (hi - lo) // 3
    buf, plan = encode(fmt, O, frames, target)
    for per_call in (1, 4, 32):
        assert encode(fmt, O, frames, target, max_tiles_per_call=per_call) == (buf, plan), per_call
    batched = tuple(torch.stack(ps) for ps in zip(*frames))
    assert encode(fmt, O, batched, target) == (buf, plan)
    pitched = [tuple(v[0] for v in views(fmt, H0, W0, "loose", 1, f)) for f in clip]
    assert encode(fmt, O, pitched, target, max_tiles_per_call=4) == (buf, plan)


@pytest.mark.parametrize("fmt,O", CASES)
def test_zero_tolerance_and_max_run_1_are_clip_rates(fmt, O):
    """on the exact clip of tests/test_gpu_clips: Tolerance() gives clip_rate.encode_clip_to_size byte for byte, with its levels,
    rates, sse and predicted; Tolerance(max_run=1) the bytes of reuse=False"""
    ctr, cr = CTR(), CR()
    frames = device_frames(clip_of(fmt))
    n_frames = len(frames)
    args = dict(tile=T, overlap=O, mask_pol=POL)
    big, plan_big = cr.encode_clip_to_size(gpu_codec(), frames, QUALITIES, 10 ** 9, fmt, **args)
    lo, hi = bounds(plan_big, n_frames)
    fw = [Fraction(1, 3), 2, 0.5, 1, 7][:n_frames]
    imp = [1, 1, Fraction(1, 1000), 1, 10 ** 6, 1]
    for target, kw in [(lo, {}), (lo + (hi - lo) // 3, {}), (lo + 2 * (hi - lo) // 3, dict(frame_weights=fw, importance=imp, plane_weights=(2, 1, 1))), (hi, {})]:
        want, wplan = cr.encode_clip_to_size(gpu_codec(), frames, QUALITIES, target, fmt, **args, **kw)
        buf, plan = ctr.encode_clip_to_size(gpu_codec(), frames, QUALITIES, target, fmt, tolerance=ctr.Tolerance(), **args, **kw)
        assert buf == want, (target, kw)
        assert (plan.source, plan.items, plan.levels, plan.rates, plan.sse, plan.predicted) == (wplan.source, wplan.items, wplan.levels, wplan.rates, wplan.sse, wplan.predicted)
        assert (plan.n_coded, plan.n_reused, plan.container_bytes, plan.den) == (wplan.n_coded, wplan.n_reused, wplan.container_bytes, wplan.den)
        assert plan.worst == [0, 0, 0] and any(len(r) > 1 for r in plan.runs)
        # the reuse identity: every frame of a run leaves the same sums, which are clip_rate's
        assert [[[per_frame[0]] * len(per_frame) for per_frame in row] for row in plan.plane_dists] == plan.plane_dists
        assert [[per_frame[0] for per_frame in row] for row in plan.plane_dists] == wplan.plane_dists
        # weights . dists is M times clip_rate's
        assert all(w * d == plan.frame_scale * ww * dd for w, row, ww, wrow in zip(plan.weights, plan.dists, wplan.weights, wplan.dists)
                   for d, dd in zip(row, wrow))
    lo, hi = bounds(cr.encode_clip_to_size(gpu_codec(), frames, QUALITIES, 10 ** 9, fmt, reuse=False, **args)[1], n_frames)
    target = (lo + hi) // 2
    want, wplan = cr.encode_clip_to_size(gpu_codec(), frames, QUALITIES, target, fmt, reuse=False, **args)
    buf, plan = ctr.encode_clip_to_size(gpu_codec(), frames, QUALITIES, target, fmt, tolerance=ctr.Tolerance(max_run=1), **args)
    assert buf == want and plan.runs == [[f] for f, _ in plan.items] and plan.n_reused == 0 and plan.levels == wplan.levels
    assert plan.sse == wplan.sse and plan.predicted == wplan.predicted


@pytest.mark.parametrize("fmt,O", CASES)
def test_frame_weights_and_importance_are_passed_on(fmt, O):
    frames = device_frames(noisy_clip(fmt))
    plan0 = free(fmt, O)[1]
    lo, hi = bounds(plan0, F)
    target = lo + (hi - lo) // 3
    fw = [Fraction(1, 3), 2, 0.5, 1, 7]
    imp = [1, 1, Fraction(1, 1000), 1, 10 ** 6, 1]
    for kw in (dict(frame_weights=fw), dict(importance=imp), dict(importance=[imp[:3], imp[3:]], frame_weights=fw), dict(plane_weights=(1, 0, 0))):
        buf, plan = encode(fmt, O, frames, target, **kw)
        flat = kw.get("importance")
        flat = [v for row in flat for v in row] if flat and isinstance(flat[0], list) else flat
        weights = TRC.weights(plan0.items, flat)
        pw = kw.get("plane_weights", (1, 1, 1))
        dists = TRC.dists(plan0.plane_dists, plan0.runs, pw, kw.get("frame_weights"), F)
        assert plan.frame_scale == TRC.frame_scale(kw.get("frame_weights"), F)[0] == (6 if "frame_weights" in kw else 1)
        assert plan.weights == weights and plan.rates == plan0.rates and plan.plane_dists == plan0.plane_dists and plan.dists == dists
        assert plan.levels == RC.allocate(plan0.rates, dists, RC2.budget(target, F, N), weights), kw
        assert plan.predicted == TRC.predicted(plan0.plane_dists, plan.levels, pw) and plan.sse == TRC.frame_sse(plan0.source, plan0.plane_dists, plan.levels)
        assert len(buf) == plan.container_bytes <= target

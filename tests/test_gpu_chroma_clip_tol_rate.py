"""Tolerant rate-controlled clips of YUV frames of any subsampling and siting on the GPU (progressivecodec_amd/chroma_clip_tol_rate.py,
libpc_chroma_clip_tol_rate.so) against their restatement (tests/chroma_clip_tol_rate_contract.py): the distortion sums of decoded
tiles against every frame of their runs exactly, on both access paths, against chroma_clip_rate.tile_distortion_jobs of the expanded
job list with the tile repeated and, for centre-sited 4:2:0, against clip_tol_rate.tile_distortion_runs; and encode_clip_to_size
through the codec into a PCL2 container that chroma_clip_rate's decoders read.  Every comparison is exact equality of integers, bits
or bytes.  T = 64 throughout (one test at 128), clips of three frames for the kernel and of five for the codec; the largest tiles, the
later trips of the final and the long runs are in tests/test_gpu_chroma_clip_tol_rate_limits.py.  The matrix is
tests/chroma_clip_tol_rate_cases.py's table; every case asserts the access path the table predicts."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import chroma_clip_tol_contract as TOL
from tests import chroma_clip_tol_rate_cases as CS
from tests import chroma_clip_tol_rate_contract as TR
from tests import chroma_contract as CC
from tests import frames_contract as FC
from tests import rate_contract as RC
from tests import tiles_contract as TC
from tests.clip_rate_contract import items_of
from tests.test_gpu_chroma_clips import clip_of, views
from tests.test_gpu_chroma_tiles import on_device
from tests.test_gpu_rate import POISON64, check_out, float_tiles
from tests.util import gpu_codec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POL = "point-based-std"
T = CS.T


def CTR():
    from progressivecodec_amd import chroma_clip_tol_rate
    return chroma_clip_tol_rate


def CR():
    from progressivecodec_amd import chroma_clip_rate
    return chroma_clip_rate


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def runs_raw(x, H, W, O, fmt, rng, matrix, siting, table, tile_ids, runs, size=T, over=None, dev_offsets=None):
    """pc_chroma_clip_tol_rate_sse_runs on the tiles x holds, the tiles and slots written to the device as they are -> (status, the
    [n_entries + 2, 3] buffer whose rows 1 .. n_entries are `out`, poisoned beforehand, whether every partial of the workspace and no
    word after it was written -- or, for a refused call, none at all).  table: per frame the list of batched plane tensors.  over:
    arguments to replace, by name.  dev_offsets: what the device's copy of the offsets holds instead of the host's."""
    from progressivecodec_amd import chroma, frames
    L = CTR().lib()
    n = len(tile_ids)
    off = TR.offsets_of(runs)
    ne = off[-1]
    f, (hs, vs) = chroma.FORMATS[fmt], chroma.SITINGS[siting]
    buf = torch.full((ne + 2, 3), POISON64, dtype=torch.int64, device=DEV)
    need = L.pc_chroma_clip_tol_rate_workspace_size(size, f.sy, ne)
    assert need == (TR.workspace_size(size, f.sy, ne) if size <= 2048 else 0)
    ws = torch.full((need // 8 + 1,), POISON64, dtype=torch.int64, device=DEV)
    k = frames.coefficients(matrix)
    host = (frames.Frame * len(table))(*[frames._frame_struct(list(ts)) for ts in table])
    dtab = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(DEV)
    dtiles = torch.tensor(tile_ids, dtype=torch.int32).to(DEV)
    doff = torch.tensor(off if dev_offsets is None else dev_offsets, dtype=torch.int32).to(DEV)
    dslots = torch.tensor([s for run in runs for s in run], dtype=torch.int32).to(DEV)
    a = dict(x=x.data_ptr(), sxt=x.stride(0), sxc=x.stride(1), sxh=x.stride(2), H=H, W=W, T=size, O=O, layout=f.layout, bits=f.bits,
             shift=f.shift, sx=f.sx, sy=f.sy, hsite=hs, vsite=vs, range=frames.RANGES.get(rng, rng), kr=k.kr, kg=k.kg, kb=k.kb, ib=k.ib, ir=k.ir,
             frames_host=host, frames_dev=dtab.data_ptr(), n_frames=len(table), tiles=dtiles.data_ptr(),
             offsets_host=(C.c_int32 * (n + 1))(*off), offsets_dev=doff.data_ptr(), slots=dslots.data_ptr(), n_jobs=n, n_entries=ne,
             ws=ws.data_ptr(), nbytes=need, out=buf[1:].data_ptr(), stream=stream())
    a.update(over or {})
    rc = L.pc_chroma_clip_tol_rate_sse_runs(*a.values())
    h = ws.cpu()
    return rc, buf, bool(h[-1] == POISON64 and ((h[:-1] != POISON64).all() if rc == 0 else (h == POISON64).all()))


def expanded_on_the_gpu(x, g, planes, tile_ids, runs, fmt, matrix, rng, siting):
    """the sequence the run kernel replaces: the tile of every entry repeated, one chroma_clip_rate job per entry"""
    jobs, owner = TR.expanded(tile_ids, runs)
    rep = x.index_select(0, torch.tensor(owner, device=DEV))
    return CR().tile_distortion_jobs(rep, g, planes, jobs, fmt, matrix, rng, siting).tolist()


# -- 1. the matrix -------------------------------------------------------------------------------------------------------------------

def run_matrix(cases):
    """every case: hostile tiles against three frames that differ, with random bits outside their 10-bit codes, pitched differently;
    runs scattered, reversed, repeated, of length 1 and over all three frames; the restatement, the expanded job list on the device, a
    sub-list and one job alone; the Python call on a list of pitched frames, on batched planes and on a side stream"""
    ctr = CTR()
    for c in cases:
        H, W, O = c.H, c.W, c.O
        ny, nx = TC.grid(H, W, T, O)
        n = ny * nx
        fr, x_np, tile_ids, runs = CS.inputs(c)
        want = CS.want(c)
        off = TR.offsets_of(runs)
        assert len(want) == off[-1]
        xv = float_tiles(x_np, c.variant)
        table = [views(c.fmt, H, W, *m, f) for m, f in zip(CS.frame_modes(c), fr)]
        assert ctr.plan(xv, table, c.fmt, overlap=O) is CS.wide(c) is CR().plan(xv, table, c.fmt, overlap=O), c
        if not c.aligned:                                                  # one narrow frame makes the whole call narrow
            assert ctr.plan(float_tiles(x_np, "contiguous"), table, c.fmt, overlap=O) is False, c
        rc, buf, ws_ok = runs_raw(xv, H, W, O, c.fmt, c.rng, c.matrix, c.siting, table, tile_ids, runs)
        assert rc == 0 and ws_ok, c
        check_out(buf, want, c)
        # a sub-list, and one job alone
        rc, buf, ws_ok = runs_raw(xv[1:n + 2], H, W, O, c.fmt, c.rng, c.matrix, c.siting, table, tile_ids[1:n + 2], runs[1:n + 2])
        assert rc == 0 and ws_ok
        check_out(buf, want[off[1]:off[n + 2]], (c, "sub-list"))
        rc, buf, ws_ok = runs_raw(xv[n:n + 1], H, W, O, c.fmt, c.rng, c.matrix, c.siting, table, tile_ids[n:n + 1], runs[n:n + 1])
        assert rc == 0 and ws_ok
        check_out(buf, want[off[n]:off[n + 1]], (c, "alone"))
        # the sequence it replaces, on the device: the same integers
        g = ctr.grid_of(H, W, T, O)
        planes = [on_device(f) for f in fr]
        assert expanded_on_the_gpu(xv, g, planes, tile_ids, runs, c.fmt, c.matrix, c.rng, c.siting) == want, c
        # the Python call
        pitched = [tuple(v[0] for v in ts) for ts in table]
        got, goff = ctr.tile_distortion_runs(xv, g, pitched, tile_ids, runs, c.fmt, c.matrix, c.rng, c.siting)
        assert got.dtype == torch.int64 and got.shape == (off[-1], 3) and got.device.type == "cuda" and got.tolist() == want and goff == off, c
        if c.n % 3 == 0:
            batched = tuple(torch.stack(ps) for ps in zip(*planes))
            cl = torch.from_numpy(x_np).to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
            assert ctr.tile_distortion_runs(cl, g, batched, torch.tensor(tile_ids), [tuple(r) for r in runs], c.fmt, c.matrix, c.rng,
                                            c.siting)[0].tolist() == want, c
            side = torch.cuda.Stream(DEV)
            side.wait_stream(torch.cuda.current_stream(DEV))
            with torch.cuda.stream(side):
                got_s = ctr.tile_distortion_runs(xv[-2:], g, planes, tile_ids[-2:], runs[-2:], c.fmt, c.matrix, c.rng, c.siting)[0]
            side.synchronize()
            assert got_s.tolist() == want[off[-3]:], c


@pytest.mark.parametrize("fmt", sorted(CC.FORMATS))
def test_every_format_and_siting_is_the_restatement_exactly(fmt):
    run_matrix(CS.main_cases(fmt))


@pytest.mark.parametrize("fmt", CS.OTHER_FORMATS)
def test_the_other_sizes_overlaps_matrices_and_full_range(fmt):
    run_matrix(CS.other_cases(fmt))


@pytest.mark.parametrize("fmt", CS.OTHER_FORMATS)
def test_overlaps_whose_band_quotients_are_no_floats(fmt):
    """O = 24 (S = 40, den = 48) and O = 28 (S = 36, den = 56: narrow at sx == 2): the sums weigh with the integer numerators 2u + 1,
    which are exact whatever 2 O is; what is new is the band geometry"""
    run_matrix(CS.band_cases(fmt))


# -- 2. the other kernel tests -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_centre_sited_420_is_clip_tol_rate_on_the_device(fmt):
    from progressivecodec_amd import clip_tol_rate
    ctr = CTR()
    H, W = 100, 150
    fr = [FC.random_frame(1, H, W, fmt, seed=3 + s) for s in range(3)]
    planes = [on_device(f) for f in fr]
    for O in (0, 16):
        g = ctr.grid_of(H, W, T, O)
        tile_ids, runs = CS.run_list(g.n, O)
        x = torch.from_numpy(CS.hostile(len(tile_ids), seed=O)).to(DEV)
        for matrix, rng in [("bt601", "full"), ("bt709", "limited")]:
            a, aoff = ctr.tile_distortion_runs(x, g, planes, tile_ids, runs, fmt, matrix, rng)
            b, boff = clip_tol_rate.tile_distortion_runs(x, g, planes, tile_ids, runs, fmt, matrix, rng)
            assert torch.equal(a, b) and aoff == boff and a.sum().item() > 0, (fmt, O, matrix, rng)
            assert CS.slots_matter(runs, a.tolist()) > 0


@pytest.mark.parametrize("fmt,siting", [("nv12", "topleft"), ("p210", "left"), ("i444", "centre")])
def test_a_job_spans_several_blocks_at_128(fmt, siting):
    H, W, size, O = 200, 250, 128, 16                                      # 2 x 3 tiles, S = 112; 4 or 8 blocks per job
    assert TC.grid(H, W, size, O) == (2, 3)
    fr = [CC.random_frame(1, H, W, fmt, seed=128 + s, garbage=True) for s in range(3)]
    tile_ids, runs = [5, 0, 4, 5], [[0, 2], [1], [2, 1, 0], [1, 1]]
    x_np = CS.hostile(4, seed=128, size=size)
    want = TR.run_sse(x_np, fr, tile_ids, runs, H, W, size, O, fmt, "bt709", "limited", siting)
    assert CS.slots_matter(runs, want) == 4
    for modes, variant in [(CS.ALIGNED, "contiguous"), (CS.MIXED, "odd")]:
        x = float_tiles(x_np, variant, size)
        table = [views(fmt, H, W, *m, f) for m, f in zip(modes, fr)]
        assert CTR().plan(x, table, fmt, overlap=O) is (variant == "contiguous")
        rc, buf, ws_ok = runs_raw(x, H, W, O, fmt, "limited", "bt709", siting, table, tile_ids, runs, size)
        assert rc == 0 and ws_ok
        check_out(buf, want, (fmt, variant))


@pytest.mark.parametrize("fmt,siting", [("nv12", "topleft"), ("p210", "left"), ("i444", "centre")])
def test_entries_out_of_range_give_zeros_and_touch_nothing(fmt, siting):
    """an entry whose slot is -1 or n_frames, a job whose tile is -1 or ny * nx (and the far ends of int32), written straight through
    the C call: 0, 0, 0 for exactly those rows, their neighbours intact, every partial written, nothing outside out or the workspace;
    and device offsets beyond [0, n_entries] are clamped"""
    ctr = CTR()
    H, W = 100, 150
    for O in (0, 16):
        n = 6
        fr = [CC.random_frame(1, H, W, fmt, seed=40 + s + O, garbage=True) for s in range(3)]
        tile_ids = [4, -1, 5, n, 2, 2 ** 31 - 1, -2 ** 31, 3, 0]
        runs = [[1, -1, 0], [0, 1], [3, 2], [0], [2 ** 31 - 1, 2, -2 ** 31], [1], [2, 0], [0, 3, 1], [-1]]
        x_np = CS.hostile(len(tile_ids), seed=O + 9)
        jobs, owner = TR.expanded(tile_ids, runs)
        valid = [e for e, (f, t) in enumerate(jobs) if 0 <= f < 3 and 0 <= t < n]
        assert valid == [0, 2, 6, 9, 14, 16]
        want = [[0, 0, 0]] * len(jobs)
        for e in valid:
            want[e] = TR.run_sse(x_np[owner[e]:owner[e] + 1], fr, [jobs[e][1]], [[jobs[e][0]]], H, W, T, O, fmt, "bt709", "limited", siting)[0]
            assert any(want[e])
        off = TR.offsets_of(runs)
        for modes, variant in ((CS.ALIGNED, "contiguous"), (CS.MIXED, "odd")):
            table = [views(fmt, H, W, *m, f) for m, f in zip(modes, fr)]
            x = float_tiles(x_np, variant)
            assert ctr.plan(x, table, fmt, overlap=O) is (variant == "contiguous")
            rc, buf, ws_ok = runs_raw(x, H, W, O, fmt, "limited", "bt709", siting, table, tile_ids, runs)
            assert rc == 0 and ws_ok
            check_out(buf, want, (fmt, O, variant))
            # what the device's offsets hold beyond [0, n_entries] is clamped: the same entries, nothing outside
            rc, buf, ws_ok = runs_raw(x, H, W, O, fmt, "limited", "bt709", siting, table, tile_ids, runs,
                                      dev_offsets=[-7] + off[1:-1] + [2 ** 31 - 1])
            assert rc == 0 and ws_ok
            check_out(buf, want, (fmt, O, variant, "clamped"))


def test_refused_calls_launch_nothing():
    ctr = CTR()
    L = ctr.lib()
    H, W, O = 100, 150, 16
    tile_ids, runs = [5, 0, 3, 0, 2], [[1], [0, 2], [2, 1, 0], [0], [1, 1]]
    x = torch.rand(len(tile_ids), 3, T, T, device=DEV)
    off = lambda *v: (C.c_int32 * len(v))(*v)                                         # noqa: E731
    for fmt in ("nv12", "p210", "i444"):
        sy = CC.sub(fmt)[1]
        table = [views(fmt, H, W, *m, CC.random_frame(1, H, W, fmt, seed=s)) for s, m in enumerate(CS.ALIGNED)]
        assert ctr.plan(x, table, fmt, overlap=O) is True                      # host only: the path of the unspoilt call; a refused call takes none
        big = lambda size: dict(size=size, O=0, sxt=3 * size * size, sxc=size * size, sxh=size)                         # noqa: E731
        bads = [dict(T=96), dict(T=0), big(4096), dict(O=6), dict(O=36), dict(O=-4), dict(layout=2), dict(bits=9), dict(shift=3), dict(sx=1, sy=2),
                dict(hsite=2), dict(vsite=-1), dict(range=2), dict(range=-1), dict(n_jobs=0), dict(n_jobs=-1), dict(n_entries=0),
                dict(n_entries=4), dict(n_entries=10), dict(n_frames=0), dict(n_frames=-1),
                dict(nbytes=L.pc_chroma_clip_tol_rate_workspace_size(T, sy, 9) - 1),
                dict(offsets_host=off(1, 1, 3, 6, 7, 9)), dict(offsets_host=off(0, 1, 1, 6, 7, 9)), dict(offsets_host=off(0, 1, 3, 6, 7, 8)),
                dict(offsets_host=off(0, 3, 1, 6, 7, 9)), dict(offsets_host=None),
                dict(x=None), dict(frames_host=None), dict(frames_dev=None), dict(tiles=None), dict(offsets_dev=None), dict(slots=None),
                dict(ws=None), dict(out=None), dict(H=0)]
        if fmt == "p210":
            bads.append(big(2048))
        for kw in bads:
            kw = dict(kw)
            size = kw.pop("size", T)
            rc, buf, ws_ok = runs_raw(x, H, W, kw.pop("O", O), fmt, "limited", "bt709", "left", table, tile_ids, runs, size, over=kw)
            torch.cuda.synchronize()
            assert rc == -1 and (buf == POISON64).all() and ws_ok, (fmt, kw)
        rc, buf, ws_ok = runs_raw(x, H, W, O, fmt, "limited", "bt709", "left", table, tile_ids, runs)                   # unspoilt, it goes through
        assert rc == 0 and ws_ok and (buf[1:-1] != POISON64).all() and (buf[0] == POISON64).all() and (buf[-1] == POISON64).all()
    with pytest.raises(ctr.ChromaClipTolRateError, match="PC_ERR_ARG"):
        raise ctr.ChromaClipTolRateError(-1, "pc_chroma_clip_tol_rate_sse_runs")


# -- 3. through the codec ------------------------------------------------------------------------------------------------------------

QUALITIES = [0, 0.5, 10]
H0, W0, N, F = CS.H0, CS.W0, CS.N, CS.CODEC_F
CASES = [(fmt, siting, O) for fmt, siting in CS.CODEC for O in (0, 16)]


@functools.lru_cache(maxsize=None)
def device_noisy(fmt, siting):
    return [on_device(f) for f in CS.noisy_clip(fmt, siting)]


def encode(fmt, siting, O, frames, target, **kw):
    kw.setdefault("tolerance", CTR().Tolerance(max_abs=1))
    return CTR().encode_clip_to_size(gpu_codec(), frames, QUALITIES, target, fmt, siting=siting, tile=T, overlap=O, mask_pol=POL, **kw)


@functools.lru_cache(maxsize=None)
def free(fmt, siting, O):
    """the noisy clip without a budget to speak of: (bytes, plan); the plan's tables do not depend on the budget"""
    return encode(fmt, siting, O, device_noisy(fmt, siting), 10 ** 9)


def fixed_of(n_frames):
    return 47 + 16 * n_frames * N


def bounds(plan, n_frames):
    return fixed_of(n_frames) + sum(min(r) for r in plan.rates), fixed_of(n_frames) + sum(max(r) for r in plan.rates)


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def true_sse(decoded, frame, fmt):
    """per plane the squared error of a decoded frame (unbatched cuda planes) against a frame of the restatement, in the frames' codes:
    independent of the kernels"""
    got = CC.codes(tuple(p.cpu().numpy()[None] for p in decoded), fmt)
    return [int(((np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)) ** 2).sum()) for a, b in zip(got, CC.codes(frame, fmt))]


@pytest.mark.parametrize("fmt,siting,O", CASES)
def test_encode_clip_to_size_on_a_noisy_clip(fmt, siting, O):
    from progressivecodec_amd import chroma_rate, chroma_tiles, container
    ctr = CTR()
    net = gpu_codec()
    clip = CS.noisy_clip(fmt, siting)
    frames = device_noisy(fmt, siting)
    g = ctr.grid_of(H0, W0, T, O)
    free_buf, plan0 = free(fmt, siting, O)
    # the source table is the tolerant scan's; the exact test reuses nothing on this clip
    source, stats = TOL.scan(clip, fmt, siting, T, O, "linear", (1, 1, 1))
    assert plan0.source == source and plan0.stats == stats and plan0.worst == TOL.worst(source, stats) == [1, 1, 1]
    items, runs = items_of(source)
    assert (plan0.items, plan0.runs) == (items, runs) and (plan0.n_coded, plan0.n_reused) == (len(items), F * N - len(items))
    assert N < len(items) < F * N and max(len(r) for r in runs) == F and plan0.den == (2 * O if O else 1)
    assert plan0.weights == [1] * len(items) and plan0.frame_scale == 1
    assert plan0.sse_exact is chroma_rate.sse_exact(g, fmt, siting) is (O == 0 and siting == "centre")
    rates, pd = plan0.rates, plan0.plane_dists
    assert len(rates) == len(pd) == len(items) and all(len(r) == 3 for r in rates) and all(len(v) == 3 for v in pd)
    assert all(len(per_frame) == len(run) and all(len(d) == 3 for d in per_frame) for row, run in zip(pd, runs) for per_frame in row)
    assert plan0.dists == TR.dists(pd, runs)
    # a reused tile's error differs from frame to frame: the reuse identity of section 28 does not hold here
    assert any(len({tuple(d) for d in per_frame}) > 1 for row in pd for per_frame in row)
    lo, hi = bounds(plan0, F)
    assert lo < hi
    with pytest.raises(ValueError, match=rf"\b{lo}\b"):
        encode(fmt, siting, O, frames, lo - 1)
    identity_differs = False
    for target in (lo, lo + (hi - lo) // 3, hi):
        buf, plan = encode(fmt, siting, O, frames, target)
        assert isinstance(buf, bytes) and buf[:4] == b"PCL2" and len(buf) == plan.container_bytes <= target, target
        assert (plan.source, plan.items, plan.runs, plan.weights, plan.rates, plan.dists, plan.plane_dists) == \
            (source, items, runs, plan0.weights, rates, plan0.dists, pd)
        levels = plan.levels
        assert levels == RC.allocate(rates, plan.dists, TR.budget(target, F, N), plan.weights), target
        assert len(buf) == TR.container_bytes(rates, levels, F, N)
        assert plan.sse == TR.frame_sse(source, pd, levels) and plan.predicted == TR.predicted(pd, levels) == sum(sum(row) for row in plan.sse)
        if target == hi:
            assert (buf, plan) == (free_buf, plan0)
        # chroma_clip_rate's decoders read it: the table aliases exactly where the scan reused, every frame is decode_frame_tiled of its own
        hd = ctr.parse_clip(buf)
        assert hd["contract"] == container.build_contract_id() and hd["F"] == F and (hd["fmt"], hd["siting"]) == (fmt, siting)
        for k in range(F):
            for t in range(N):
                assert hd["table"][k][t] == hd["table"][source[k][t]][t]
                assert all((hd["table"][k][t] == hd["table"][j][t]) == (source[k][t] == source[j][t]) for j in range(F)), (k, t)
        got = ctr.decode_clip(net, buf)
        assert len(got) == F and all(same(a, b) for a, b in zip(got, CR().decode_clip(net, buf)))
        for k in range(F):
            assert same(got[k], chroma_tiles.decode_frame_tiled(net, ctr.frame_container(buf, k))), (target, k)
        if O == 0:
            # the plan's luma column is the decoded frame's exact SSE against the frame that was shown; every plane where sse_exact
            for k in range(F):
                sse = true_sse(got[k], clip[k], fmt)
                assert sse[0] == plan.sse[k][0] and (sse == plan.sse[k] or not plan.sse_exact), (target, k)
            # what the reuse identity would give: every frame of a run charged the item's sums against the frame it was coded for
            anchor = lambda k, t: pd[items.index((source[k][t], t))][levels[items.index((source[k][t], t))]][0]       # noqa: E731
            by_identity = [[sum(anchor(k, t)[p] for t in range(N)) for p in range(3)] for k in range(F)]
            identity_differs = identity_differs or any(by_identity[k][0] != plan.sse[k][0] for k in range(F))
    assert O != 0 or identity_differs
    assert O != 0 or fmt != "i444" or plan0.sse_exact


@pytest.mark.parametrize("fmt,siting,O", CASES)
def test_bytes_and_plan_do_not_depend_on_the_layout(fmt, siting, O):
    clip = CS.noisy_clip(fmt, siting)
    frames = device_noisy(fmt, siting)
    lo, hi = bounds(free(fmt, siting, O)[1], F)
    target = lo + (hi - lo) // 3
    buf, plan = encode(fmt, siting, O, frames, target)
    for per_call in (1, 4):
        assert encode(fmt, siting, O, frames, target, max_tiles_per_call=per_call) == (buf, plan), per_call
    batched = tuple(torch.stack(ps) for ps in zip(*frames))
    assert encode(fmt, siting, O, batched, target) == (buf, plan)
    pitched = [tuple(v[0] for v in views(fmt, H0, W0, "loose", 1, f)) for f in clip]
    assert encode(fmt, siting, O, pitched, target, max_tiles_per_call=5) == (buf, plan)


@pytest.mark.parametrize("fmt,siting,O", CASES)
def test_zero_tolerance_and_max_run_1_are_chroma_clip_rates(fmt, siting, O):
    """on the exact clip of tests/test_gpu_chroma_clips: Tolerance() gives chroma_clip_rate.encode_clip_to_size byte for byte, with its
    levels, rates, sse and predicted; Tolerance(max_run=1) the bytes of reuse=False"""
    ctr, cr = CTR(), CR()
    frames = [on_device(f) for f in clip_of(fmt, siting)]
    n_frames = len(frames)
    args = dict(siting=siting, tile=T, overlap=O, mask_pol=POL)
    big, plan_big = cr.encode_clip_to_size(gpu_codec(), frames, QUALITIES, 10 ** 9, fmt, **args)
    lo, hi = bounds(plan_big, n_frames)
    fw = [Fraction(1, 3), 2, 0.5, 1, 7][:n_frames]
    imp = [1, 1, Fraction(1, 1000), 1, 10 ** 6, 1]
    for target, kw in [(lo + (hi - lo) // 3, {}), (lo + 2 * (hi - lo) // 3, dict(frame_weights=fw, importance=imp, plane_weights=(2, 1, 1))), (hi, {})]:
        want, wplan = cr.encode_clip_to_size(gpu_codec(), frames, QUALITIES, target, fmt, **args, **kw)
        buf, plan = ctr.encode_clip_to_size(gpu_codec(), frames, QUALITIES, target, fmt, tolerance=ctr.Tolerance(), **args, **kw)
        assert buf == want, (target, kw)
        assert (plan.source, plan.items, plan.levels, plan.rates, plan.sse, plan.predicted) == \
            (wplan.source, wplan.items, wplan.levels, wplan.rates, wplan.sse, wplan.predicted)
        assert (plan.n_coded, plan.n_reused, plan.container_bytes, plan.den, plan.sse_exact) == \
            (wplan.n_coded, wplan.n_reused, wplan.container_bytes, wplan.den, wplan.sse_exact)
        assert plan.worst == [0, 0, 0] and any(len(r) > 1 for r in plan.runs)
        # the reuse identity: every frame of a run leaves the same sums, which are chroma_clip_rate's
        assert [[[per_frame[0]] * len(per_frame) for per_frame in row] for row in plan.plane_dists] == plan.plane_dists
        assert [[per_frame[0] for per_frame in row] for row in plan.plane_dists] == wplan.plane_dists
        assert all(w * d == plan.frame_scale * ww * dd for w, row, ww, wrow in zip(plan.weights, plan.dists, wplan.weights, wplan.dists)
                   for d, dd in zip(row, wrow))
    lo, hi = bounds(cr.encode_clip_to_size(gpu_codec(), frames, QUALITIES, 10 ** 9, fmt, reuse=False, **args)[1], n_frames)
    target = (lo + hi) // 2
    want, wplan = cr.encode_clip_to_size(gpu_codec(), frames, QUALITIES, target, fmt, reuse=False, **args)
    buf, plan = ctr.encode_clip_to_size(gpu_codec(), frames, QUALITIES, target, fmt, tolerance=ctr.Tolerance(max_run=1), **args)
    assert buf == want and plan.runs == [[f] for f, _ in plan.items] and plan.n_reused == 0 and plan.levels == wplan.levels
    assert plan.sse == wplan.sse and plan.predicted == wplan.predicted


@pytest.mark.parametrize("O", [0, 16])
def test_centre_sited_nv12_is_clip_tol_rate_s_encoder(O):
    """the levels, rates, plane_dists and every tile's blob are clip_tol_rate.encode_clip_to_size's; the containers differ in their
    headers (47 bytes against 42) and so in every offset"""
    from progressivecodec_amd import clip_rate, clip_tol_rate
    ctr = CTR()
    frames = device_noisy("nv12", "centre")
    plan0 = free("nv12", "centre", O)[1]
    lo, hi = bounds(plan0, F)
    for target in (lo + (hi - lo) // 3, hi):
        buf, plan = encode("nv12", "centre", O, frames, target)
        obuf, oplan = clip_tol_rate.encode_clip_to_size(gpu_codec(), frames, QUALITIES, target - 5, "nv12", tile=T, overlap=O, mask_pol=POL,
                                                        tolerance=ctr.Tolerance(max_abs=1))
        assert plan[:-1] == oplan._replace(container_bytes=len(buf)) and len(buf) == len(obuf) + 5 and plan.n_reused > 0
        hd, ohd = ctr.parse_clip(buf), clip_tol_rate.parse_clip(obuf)
        for k in range(F):
            for t in range(N):
                assert ctr.tile_blob(buf, hd, k, t)[0] == clip_rate.tile_blob(obuf, ohd, k, t)[0], (k, t)


@pytest.mark.parametrize("fmt,siting,O", CASES[:2] + CASES[3:4])
def test_frame_weights_and_importance_are_passed_on(fmt, siting, O):
    frames = device_noisy(fmt, siting)
    plan0 = free(fmt, siting, O)[1]
    lo, hi = bounds(plan0, F)
    target = lo + (hi - lo) // 3
    fw = [Fraction(1, 3), 2, 0.5, 1, 7]
    imp = [1, 1, Fraction(1, 1000), 1, 10 ** 6, 1]
    for kw in (dict(frame_weights=fw), dict(importance=[imp[:3], imp[3:]], frame_weights=fw), dict(plane_weights=(1, 0, 0))):
        buf, plan = encode(fmt, siting, O, frames, target, **kw)
        flat = imp if "importance" in kw else None
        weights = TR.weights(plan0.items, flat)
        pw = kw.get("plane_weights", (1, 1, 1))
        dists = TR.dists(plan0.plane_dists, plan0.runs, pw, kw.get("frame_weights"), F)
        assert plan.frame_scale == TR.frame_scale(kw.get("frame_weights"), F)[0] == (6 if "frame_weights" in kw else 1)
        assert plan.weights == weights and plan.rates == plan0.rates and plan.plane_dists == plan0.plane_dists and plan.dists == dists
        assert plan.levels == RC.allocate(plan0.rates, dists, TR.budget(target, F, N), weights), kw
        assert plan.predicted == TR.predicted(plan0.plane_dists, plan.levels, pw) and plan.sse == TR.frame_sse(plan0.source, plan0.plane_dists, plan.levels)
        assert len(buf) == plan.container_bytes <= target

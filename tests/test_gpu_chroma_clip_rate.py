"""Rate-controlled clips of YUV frames of any subsampling and siting on the GPU (progressivecodec_amd/chroma_clip_rate.py,
libpc_chroma_clip_rate.so) against their restatement (tests/chroma_clip_rate_contract.py): the distortion sums of scattered (frame, tile)
jobs exactly, on both access paths, against chroma_rate.frame_tile_distortion of the same tile and frame and against
clip_rate.tile_distortion_jobs on the device; and encode_clip_to_size / decode_clip through the codec and a PCL2 container.  Every
comparison is exact equality of integers, bits or bytes.  T = 64 throughout, clips of three frames for the kernel and of six for the
codec.  The matrix is tests/chroma_clip_rate_cases.py's table; every case asserts the access path the table predicts."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import chroma_clip_rate_cases as JS
from tests import chroma_clip_rate_contract as JC
from tests import chroma_clips_contract as CK
from tests import chroma_contract as CC
from tests import frames_contract as FC
from tests import hostile_values as HV
from tests import rate_contract as RC
from tests import tiles_contract as TC
from tests.test_gpu_chroma_clips import clip_of, other_bits, views
from tests.test_gpu_chroma_tiles import on_device
from tests.test_gpu_rate import POISON64, check_out, float_tiles
from tests.util import gpu_codec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POL = "point-based-std"
T = JS.T


def CR():
    from progressivecodec_amd import chroma_clip_rate
    return chroma_clip_rate


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def hostile(n, seed, size=T):
    """tiles_contract.hostile_tiles with hostile_values.SPECIALS (NaN, +-inf, the largest finites, a denormal, -0.0) planted on top"""
    x = TC.hostile_tiles(n, size, seed)
    flat = x.reshape(-1)
    flat[5::211] = np.resize(HV.SPECIALS, flat[5::211].shape)
    return x


def jobs_raw(x, H, W, O, fmt, rng, matrix, siting, table, jobs, size=T, over=None):
    """pc_chroma_clip_rate_sse_jobs on the tiles x holds, the jobs written to the device as they are -> (status, the [n + 2, 3] buffer
    whose rows 1 .. n are `out`, poisoned beforehand, whether every partial of the workspace and no word after it was written -- or,
    for a refused call, none at all).  table: per frame the list of batched plane tensors.  over: arguments to replace, by name."""
    from progressivecodec_amd import chroma, frames
    L = CR().lib()
    n = len(jobs)
    f, (hs, vs) = chroma.FORMATS[fmt], chroma.SITINGS[siting]
    buf = torch.full((n + 2, 3), POISON64, dtype=torch.int64, device=DEV)
    need = L.pc_chroma_clip_rate_workspace_size(size, f.sy, n)
    assert need == (24 * n * (size * size // (2048 * f.sy)) if size <= 2048 else 0)
    ws = torch.full((need // 8 + 1,), POISON64, dtype=torch.int64, device=DEV)
    k = frames.coefficients(matrix)
    host = (frames.Frame * len(table))(*[frames._frame_struct(list(ts)) for ts in table])
    dtab = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(DEV)
    djobs = torch.tensor(jobs, dtype=torch.int32).reshape(-1, 2).to(DEV)
    a = dict(x=x.data_ptr(), sxt=x.stride(0), sxc=x.stride(1), sxh=x.stride(2), H=H, W=W, T=size, O=O, layout=f.layout, bits=f.bits,
             shift=f.shift, sx=f.sx, sy=f.sy, hsite=hs, vsite=vs, range=frames.RANGES.get(rng, rng), kr=k.kr, kg=k.kg, kb=k.kb, ib=k.ib, ir=k.ir,
             frames_host=host, frames_dev=dtab.data_ptr(), n_frames=len(table), jobs=djobs.data_ptr(), n_jobs=n, ws=ws.data_ptr(), nbytes=need,
             out=buf[1:].data_ptr(), stream=stream())
    a.update(over or {})
    rc = L.pc_chroma_clip_rate_sse_jobs(*a.values())
    h = ws.cpu()
    return rc, buf, bool(h[-1] == POISON64 and ((h[:-1] != POISON64).all() if rc == 0 else (h == POISON64).all()))


def clip3(c):
    return [CC.random_frame(1, c.H, c.W, c.fmt, seed=1000 * c.H + c.W + c.n + 7 * s, garbage=True) for s in range(JS.F)]


# -- 1. the matrix -------------------------------------------------------------------------------------------------------------------

def run_matrix(cases):
    """every case: hostile tiles against three frames with random bits outside their 10-bit codes, pitched differently; the jobs
    scattered, reversed, repeated and from all three frames; the restatement, the frame call on the device, a sub-list and one job
    alone; the Python call on a list of pitched frames, on batched planes and on a side stream"""
    cr = CR()
    from progressivecodec_amd import chroma_rate
    for c in cases:
        H, W, O = c.H, c.W, c.O
        ny, nx = TC.grid(H, W, T, O)
        n = ny * nx
        jobs = JS.job_list(n, H + W + O + c.n)
        fr = clip3(c)
        x_np = hostile(len(jobs), seed=77 * H + W + c.n)
        want = JC.job_sse(x_np, fr, jobs, H, W, T, O, c.fmt, c.matrix, c.rng, c.siting)
        xv = float_tiles(x_np, c.variant)
        table = [views(c.fmt, H, W, *m, f) for m, f in zip(JS.frame_modes(c), fr)]
        assert cr.plan(xv, table, c.fmt, overlap=O) is JS.wide(c), c
        if not c.aligned:                                                  # one narrow frame makes the whole call narrow
            assert cr.plan(float_tiles(x_np, "contiguous"), table, c.fmt, overlap=O) is False, c
        rc, buf, ws_ok = jobs_raw(xv, H, W, O, c.fmt, c.rng, c.matrix, c.siting, table, jobs)
        assert rc == 0 and ws_ok, c
        check_out(buf, want, c)
        # a sub-list, and one job alone
        rc, buf, ws_ok = jobs_raw(xv[1:n + 2], H, W, O, c.fmt, c.rng, c.matrix, c.siting, table, jobs[1:n + 2])
        assert rc == 0 and ws_ok
        check_out(buf, want[1:n + 2], (c, "sub-list"))
        rc, buf, ws_ok = jobs_raw(xv[n:n + 1], H, W, O, c.fmt, c.rng, c.matrix, c.siting, table, jobs[n:n + 1])
        assert rc == 0 and ws_ok
        check_out(buf, want[n:n + 1], (c, "alone"))
        # the call it replaces, on the device: the same integers
        g = cr.grid_of(H, W, T, O)
        planes = [on_device(f) for f in fr]
        for m, (f, t) in enumerate(jobs):
            one = chroma_rate.frame_tile_distortion(xv[m:m + 1], g, planes[f], c.fmt, c.matrix, c.rng, c.siting, first_tile=t)
            assert one.tolist() == [want[m]], (c, m, f, t)
        # the Python call
        pitched = [tuple(v[0] for v in ts) for ts in table]
        got = cr.tile_distortion_jobs(xv, g, pitched, jobs, c.fmt, c.matrix, c.rng, c.siting)
        assert got.dtype == torch.int64 and got.shape == (len(jobs), 3) and got.device.type == "cuda" and got.tolist() == want, c
        if c.n % 3 == 0:
            batched = tuple(torch.stack(ps) for ps in zip(*planes))
            cl = torch.from_numpy(x_np).to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
            assert cr.tile_distortion_jobs(cl, g, batched, torch.tensor(jobs), c.fmt, c.matrix, c.rng, c.siting).tolist() == want, c
            side = torch.cuda.Stream(DEV)
            side.wait_stream(torch.cuda.current_stream(DEV))
            with torch.cuda.stream(side):
                got_s = cr.tile_distortion_jobs(xv[-2:], g, planes, jobs[-2:], c.fmt, c.matrix, c.rng, c.siting)
            side.synchronize()
            assert got_s.tolist() == want[-2:], c


@pytest.mark.parametrize("fmt", sorted(CC.FORMATS))
def test_every_format_and_siting_is_the_restatement_exactly(fmt):
    run_matrix(JS.main_cases(fmt))


@pytest.mark.parametrize("fmt", JS.OTHER_FORMATS)
def test_the_other_sizes_overlaps_matrices_and_full_range(fmt):
    run_matrix(JS.other_cases(fmt))


# -- 2. the other kernel tests -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_centre_sited_420_is_clip_rate_on_the_device(fmt):
    from progressivecodec_amd import clip_rate
    cr = CR()
    H, W = 100, 150
    fr = [FC.random_frame(1, H, W, fmt, seed=3 + s) for s in range(3)]
    planes = [on_device(f) for f in fr]
    for O in (0, 16):
        g = cr.grid_of(H, W, T, O)
        jobs = JS.job_list(g.n, O)
        x = torch.from_numpy(hostile(len(jobs), seed=O)).to(DEV)
        for matrix, rng in [("bt601", "full"), ("bt709", "limited")]:
            a = cr.tile_distortion_jobs(x, g, planes, jobs, fmt, matrix, rng)
            b = clip_rate.tile_distortion_jobs(x, g, planes, jobs, fmt, matrix, rng)
            assert torch.equal(a, b) and a.sum().item() > 0, (fmt, O, matrix, rng)


@pytest.mark.parametrize("fmt,siting", [("nv12", "topleft"), ("p210", "left"), ("i444", "centre")])
def test_jobs_out_of_range_give_zeros_and_touch_nothing(fmt, siting):
    """a job whose slot is -1 or n_frames, or whose tile is -1 or ny * nx (and the far ends of int32), written straight through the C
    call: 0, 0, 0, its neighbours intact, every partial written, nothing outside out or the workspace"""
    cr = CR()
    H, W = 100, 150
    for O in (0, 16):
        n = 6
        fr = [CC.random_frame(1, H, W, fmt, seed=40 + s + O, garbage=True) for s in range(3)]
        good = [(1, 4), (0, 0), (2, 5), (1, 1), (0, 3), (2, 2), (1, 5), (0, 5), (2, 0), (1, 0)]
        bad = {1: (-1, 0), 3: (3, 0), 4: (0, -1), 6: (0, n), 7: (2 ** 31 - 1, 2), 8: (-2 ** 31, 2), 9: (1, 2 ** 31 - 1)}
        jobs = [bad.get(m, j) for m, j in enumerate(good)] + [(2, -2 ** 31), (-1, -1), (3, n), (1, 3)]
        x_np = hostile(len(jobs), seed=O + 9)
        valid = [m for m, (f, t) in enumerate(jobs) if 0 <= f < 3 and 0 <= t < n]
        assert valid == [0, 2, 5, len(jobs) - 1]
        full = JC.job_sse(x_np[valid], fr, [jobs[m] for m in valid], H, W, T, O, fmt, "bt709", "limited", siting)
        want = [[0, 0, 0]] * len(jobs)
        for m, row in zip(valid, full):
            want[m] = row
            assert any(row)
        for modes, variant in ((JS.ALIGNED, "contiguous"), (JS.MIXED, "odd")):
            table = [views(fmt, H, W, *m, f) for m, f in zip(modes, fr)]
            x = float_tiles(x_np, variant)
            assert cr.plan(x, table, fmt, overlap=O) is (variant == "contiguous")
            rc, buf, ws_ok = jobs_raw(x, H, W, O, fmt, "limited", "bt709", siting, table, jobs)
            assert rc == 0 and ws_ok
            check_out(buf, want, (fmt, O, variant))


def test_refused_calls_launch_nothing():
    cr = CR()
    L = cr.lib()
    H, W, O = 100, 150, 16
    jobs = [(1, 5), (0, 0), (2, 3), (0, 0), (1, 2)]
    x = torch.rand(len(jobs), 3, T, T, device=DEV)
    for fmt in ("nv12", "p210", "i444"):
        sy = CC.sub(fmt)[1]
        table = [views(fmt, H, W, *m, CC.random_frame(1, H, W, fmt, seed=s)) for s, m in enumerate(JS.ALIGNED)]
        big = lambda size: dict(size=size, O=0, sxt=3 * size * size, sxc=size * size, sxh=size)                         # noqa: E731
        bads = [dict(T=96), dict(T=0), big(4096), dict(O=6), dict(O=36), dict(O=-4), dict(layout=2), dict(bits=9), dict(shift=3), dict(sx=1, sy=2),
                dict(hsite=2), dict(vsite=-1), dict(range=2), dict(range=-1), dict(n_jobs=0), dict(n_jobs=-1), dict(n_frames=0),
                dict(n_frames=-1), dict(nbytes=L.pc_chroma_clip_rate_workspace_size(T, sy, 5) - 1), dict(x=None), dict(frames_host=None),
                dict(frames_dev=None), dict(jobs=None), dict(ws=None), dict(out=None), dict(H=0)]
        if fmt == "p210":
            bads.append(big(2048))
        for kw in bads:
            kw = dict(kw)
            size = kw.pop("size", T)
            rc, buf, ws_ok = jobs_raw(x, H, W, kw.pop("O", O), fmt, "limited", "bt709", "left", table, jobs, size, over=kw)
            torch.cuda.synchronize()
            assert rc == -1 and (buf == POISON64).all() and ws_ok, (fmt, kw)
        rc, buf, ws_ok = jobs_raw(x, H, W, O, fmt, "limited", "bt709", "left", table, jobs)                            # unspoilt, it goes through
        assert rc == 0 and ws_ok and (buf[1:-1] != POISON64).all() and (buf[0] == POISON64).all() and (buf[-1] == POISON64).all()
    with pytest.raises(cr.ChromaClipRateError, match="PC_ERR_ARG"):
        raise cr.ChromaClipRateError(-1, "pc_chroma_clip_rate_sse_jobs")


@pytest.mark.parametrize("fmt,siting", [("nv12", "centre"), ("nv12", "topleft"), ("p210", "left"), ("i444", "centre")])
def test_the_reuse_identity_on_the_device(fmt, siting):
    """two frames that differ only outside tile (1, 1)'s footprint -- every sample of every plane outside it changed -- give that
    tile's job the same three integers against either; one more sample changed inside the measured part and they differ"""
    cr = CR()
    H, W, O = 100, 150, 16
    g = cr.grid_of(H, W, T, O)
    t = 1 * g.nx + 1
    half = 1 << (CC.bits(fmt) - 1)
    for up in ("linear", "nearest"):
        lu, ch = CK.footprint(1, 1, H, W, T, O, fmt, siting, up)
        a = [np.array(c) for c in CC.codes(CC.random_frame(1, H, W, fmt, seed=11), fmt)]
        b = [c ^ half for c in a]
        for p, box in enumerate((lu, ch, ch)):
            b[p][0, box[0]:box[1], box[2]:box[3]] = a[p][0, box[0]:box[1], box[2]:box[3]]
        fa, fb = CC.frame(*a, fmt), CC.frame(*b, fmt)
        assert CK.tile_changes(fb, fa, fmt, siting, T, O, up, t, 1) == [[0, 0, 0]]
        x = torch.from_numpy(hostile(1, seed=5)).to(DEV).repeat(3, 1, 1, 1)   # one decoded tile, measured three times
        got = cr.tile_distortion_jobs(x, g, [on_device(fa), on_device(fb)], [(0, t), (1, t), (1, t - 1)], fmt, siting=siting)
        assert got[0].tolist() == got[1].tolist() and any(got[0].tolist()), (fmt, siting, up)
        c = [np.array(v) for v in b]
        c[1][0, ch[1] - 1, ch[3] - 2] ^= half                              # a chroma cell of the tile itself
        got2 = cr.tile_distortion_jobs(x[:1], g, [on_device(CC.frame(*c, fmt))], [(0, t)], fmt, siting=siting)
        assert got2[0, 1].item() != got[0, 1].item() and got2[0, 0].item() == got[0, 0].item()


# -- 3. through the codec ------------------------------------------------------------------------------------------------------------

QUALITIES = [0, 0.5, 10]
H0, W0 = 100, 150                                                          # 2 x 3 tiles of 64 x 64, with and without overlap
N = 6
CODEC = [("p210", "left"), ("nv12", "topleft"), ("i444", "centre")]
CASES = [(fmt, siting, O) for fmt, siting in CODEC for O in (0, 16)]
OTHER = {("p210", "left"): ("nv12", "left"), ("nv12", "topleft"): ("p210", "left"), ("i444", "centre"): ("nv12", "topleft"),
         ("nv12", "centre"): ("i444", "centre")}


@functools.lru_cache(maxsize=None)
def clip6(fmt, siting):
    """test_gpu_chroma_clips.clip_of's four frames (a smooth frame; one luma sample changed; the same again; one Cb sample changed),
    then that frame again with other bits outside its codes, then a frame whose luma sample (70, 120) changed"""
    c = clip_of(fmt, siting)
    last = [np.array(p) for p in CC.codes(c[3], fmt)]
    last[0][0, 70, 120] ^= 1 << (CC.bits(fmt) - 1)
    return list(c) + [other_bits(c[3], fmt, np.random.default_rng(9)), CC.frame(*last, fmt)]


@functools.lru_cache(maxsize=None)
def device_clip(fmt, siting):
    return [on_device(f) for f in clip6(fmt, siting)]


def encode(fmt, siting, O, frames, target, **kw):
    return CR().encode_clip_to_size(gpu_codec(), frames, QUALITIES, target, fmt, siting=siting, tile=T, overlap=O, mask_pol=POL, **kw)


@functools.lru_cache(maxsize=None)
def free(fmt, siting, O):
    """the clip without a budget to speak of: (bytes, plan); the plan's tables do not depend on the budget"""
    return encode(fmt, siting, O, device_clip(fmt, siting), 10 ** 9)


def fixed_of(F):
    return 47 + 16 * F * N


def bounds(plan, F):
    return fixed_of(F) + sum(min(r) for r in plan.rates), fixed_of(F) + sum(max(r) for r in plan.rates)


@functools.lru_cache(maxsize=None)
def alone(fmt, siting, O, f, t, l):
    """tile t of frame f cut and coded alone at level l, and the model's own output for it decoded alone"""
    from progressivecodec_amd import chroma_tiles, container
    net = gpu_codec()
    x, _ = chroma_tiles.cut_frame(device_clip(fmt, siting)[f], fmt, siting=siting, tile=T, overlap=O, rect=(t // 3, t % 3, 1, 1))
    datas = net.compress_levels(x, [QUALITIES[l]], mask_pol=POL)
    b = container.pack([datas[0]["strings"]], datas[0]["shape"], [float(QUALITIES[l])], image_size=(T, T), mask_pol=POL)
    strings, shape, qs, _, pol = container.unpack(b, levels=[0])
    return b, net.decompress(strings[0], shape, qs[0], pol)["x_hat"][0]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("fmt,siting,O", CASES)
def test_encode_clip_to_size_and_decode_clip(fmt, siting, O):
    from progressivecodec_amd import chroma_rate, chroma_tiles, container
    cr = CR()
    net = gpu_codec()
    clip = clip6(fmt, siting)
    F = len(clip)
    frames = device_clip(fmt, siting)
    g = cr.grid_of(H0, W0, T, O)
    free_buf, plan0 = free(fmt, siting, O)
    source = CK.source_table(clip, fmt, siting, T, O, "linear")
    items, runs = JC.items_of(source)
    weights = JC.weights(source)
    assert F == 6 and plan0.source == source and plan0.items == items and plan0.weights == weights == [len(r) for r in runs]
    assert (plan0.n_coded, plan0.n_reused) == (len(items), F * N - len(items)) and 6 < len(items) < F * N and plan0.den == (2 * O if O else 1)
    assert plan0.sse_exact is chroma_rate.sse_exact(g, fmt, siting) is (O == 0 and siting == "centre")
    # rates and plane_dists are those of the tile cut, coded and decoded alone, measured against the frame it was coded for
    rates, dists, pd = plan0.rates, plan0.dists, plan0.plane_dists
    assert len(rates) == len(dists) == len(pd) == len(items) and all(len(r) == 3 for r in rates + dists + pd)
    for i, (f, t) in enumerate(items):
        for l in range(3):
            b, x = alone(fmt, siting, O, f, t, l)
            assert rates[i][l] == len(b), (i, l)
            assert pd[i][l] == chroma_rate.frame_tile_distortion(x[None], g, frames[f], fmt, siting=siting, first_tile=t).tolist()[0], (i, l)
            assert dists[i][l] == sum(pd[i][l])
    lo, hi = bounds(plan0, F)
    assert lo < hi
    with pytest.raises(ValueError, match=rf"\b{lo}\b"):
        encode(fmt, siting, O, frames, lo - 1)
    ofmt, ositing = OTHER[(fmt, siting)]
    for target in (lo, lo + (hi - lo) // 3, hi):
        buf, plan = encode(fmt, siting, O, frames, target)
        assert isinstance(buf, bytes) and buf[:4] == b"PCL2" and len(buf) == plan.container_bytes <= target, target
        assert (plan.source, plan.items, plan.weights, plan.rates, plan.dists, plan.plane_dists) == (source, items, weights, rates, dists, pd)
        levels = plan.levels
        assert levels == RC.allocate(rates, dists, JC.budget(target, F, N), weights), target
        assert len(buf) == JC.container_bytes(rates, levels, F, N)
        assert plan.sse == JC.frame_sse(source, pd, levels) and plan.predicted == JC.predicted(source, dists, levels)
        blobs = [[alone(fmt, siting, O, f, t, levels[items.index((f, t))])[0] if source[f][t] == f else None for t in range(N)] for f in range(F)]
        hd = cr.parse_clip(buf)
        assert buf == JC.pack_clip(blobs, source, H0, W0, T, O, fmt, "bt709", "limited", "linear", siting, hd["contract"])
        assert hd["contract"] == container.build_contract_id()
        if target == hi:
            assert all(dists[i][l] == min(dists[i]) for i, l in enumerate(levels)) and (buf, plan) == (free_buf, plan0)
        # every frame is decode_frame_tiled of its own container, bit for bit
        per_frame = [cr.frame_container(buf, k) for k in range(F)]
        shown = lambda k: [blobs[source[k][t]][t] for t in range(N)]                                                  # noqa: E731
        assert all(per_frame[k] == JC.frame_container(shown(k), H0, W0, T, O, fmt, "bt709", "limited", "linear", siting, hd["contract"])
                   for k in range(F))
        want = [chroma_tiles.decode_frame_tiled(net, b) for b in per_frame]
        assert all(same(a, b) for a, b in zip(cr.decode_clip(net, buf), want)), target
        decoded = lambda k: torch.stack([alone(fmt, siting, O, source[k][t], t, levels[items.index((source[k][t], t))])[1] for t in range(N)])   # noqa: E731
        if O == 0:                                                         # luma always; chroma where the plan says so
            for k in range(F):
                sse = chroma_tiles.stitch_frame(decoded(k), g, fmt, siting=siting, ref=frames[k], image=False).sse[0].tolist()
                assert sse[0] == plan.sse[k][0] and (sse == plan.sse[k] or not plan.sse_exact), (target, k)
        if target == lo + (hi - lo) // 3:
            for dkw in [dict(region=(64, 64, 30, 40)), dict(level=0, region=(64, 64, 30, 40), fmt=ofmt, siting=ositing), dict(max_tiles_per_call=1)]:
                got = cr.decode_clip(net, buf, **dkw)
                assert all(same(a, chroma_tiles.decode_frame_tiled(net, b, **dkw)) for a, b in zip(got, per_frame)), dkw
            part = cr.decode_clip(net, buf, frames=[3, 1, 1], max_tiles_per_call=1)
            assert len(part) == 3 and same(part[0], want[3]) and same(part[1], want[1]) and same(part[2], want[1])
            # the reuse identity: a reused item's decoded tile leaves the same three sums in every frame that shows it
            for i, ((f, t), run) in enumerate(zip(items, runs)):
                x = alone(fmt, siting, O, f, t, levels[i])[1][None]
                for k in run:
                    assert chroma_rate.frame_tile_distortion(x, g, frames[k], fmt, siting=siting, first_tile=t).tolist()[0] == pd[i][levels[i]], (i, k)
            assert any(len(run) > 1 for run in runs)
    with pytest.raises(container.ContainerError, match="level must be -1 or 0"):
        cr.decode_clip(net, free_buf, level=1)


@pytest.mark.parametrize("fmt,siting,O", CASES)
def test_bytes_and_plan_do_not_depend_on_the_layout(fmt, siting, O):
    clip = clip6(fmt, siting)
    frames = device_clip(fmt, siting)
    lo, hi = bounds(free(fmt, siting, O)[1], len(clip))
    target = lo + (hi - lo) // 3
    buf, plan = encode(fmt, siting, O, frames, target)
    for per_call in (1, 4):
        assert encode(fmt, siting, O, frames, target, max_tiles_per_call=per_call) == (buf, plan), per_call
    batched = tuple(torch.stack(ps) for ps in zip(*frames))
    assert encode(fmt, siting, O, batched, target) == (buf, plan)
    pitched = [tuple(v[0] for v in views(fmt, H0, W0, "loose", 1, f)) for f in clip]
    assert encode(fmt, siting, O, pitched, target, max_tiles_per_call=5) == (buf, plan)


@pytest.mark.parametrize("fmt,siting,O", CASES)
def test_a_clip_of_one_frame_is_the_frame_call(fmt, siting, O):
    """the clip's fixed overhead is 47 + 16 n bytes, the frame's 48 with the 16 in its rates: at target and target + 1 the allocator
    sees the same problem"""
    from progressivecodec_amd import chroma_rate
    cr = CR()
    frame = device_clip(fmt, siting)[0]
    kw = dict(siting=siting, tile=T, overlap=O, mask_pol=POL)
    fbuf0, fplan0 = chroma_rate.encode_frame_tiled_to_size(gpu_codec(), frame, QUALITIES, 10 ** 9, fmt, **kw)
    lo, hi = 48 + sum(min(r) for r in fplan0.rates), 48 + sum(max(r) for r in fplan0.rates)
    for target in (lo - 1, (lo + hi) // 2 - 1, hi - 1):
        buf, plan = encode(fmt, siting, O, [frame], target)
        fbuf, fplan = chroma_rate.encode_frame_tiled_to_size(gpu_codec(), frame, QUALITIES, target + 1, fmt, **kw)
        assert cr.frame_container(buf, 0) == fbuf, target
        assert plan.levels == fplan.levels and plan.plane_dists == fplan.plane_dists and plan.sse == [fplan.sse]
        assert plan.sse_exact is fplan.sse_exact
        assert plan.rates == [[v - 16 for v in r] for r in fplan.rates] and len(buf) == len(fbuf) - 1
        assert plan.source == [[0] * N] and plan.items == [(0, t) for t in range(N)] and plan.weights == [1] * N
    with pytest.raises(ValueError, match=rf"\b{lo - 1}\b"):
        encode(fmt, siting, O, [frame], lo - 2)


@pytest.mark.parametrize("fmt,siting,O", CASES)
def test_a_static_clip_stores_each_tile_once(fmt, siting, O):
    cr = CR()
    frame = device_clip(fmt, siting)[0]
    still = [frame] * 3
    big, plan_big = encode(fmt, siting, O, still, 10 ** 9)
    assert plan_big.source == [[0] * N] * 3 and plan_big.items == [(0, t) for t in range(N)] and plan_big.weights == [3] * N
    assert (plan_big.n_coded, plan_big.n_reused) == (N, 2 * N)
    lo, hi = bounds(plan_big, 3)
    target = (lo + hi) // 2
    buf, plan = encode(fmt, siting, O, still, target)
    single, splan = encode(fmt, siting, O, [frame], target - 16 * 2 * N)
    assert plan.levels == splan.levels and plan.rates == splan.rates and plan.plane_dists == splan.plane_dists
    assert plan.sse == splan.sse * 3 and plan.predicted == 3 * splan.predicted
    hd, hs = cr.parse_clip(buf), cr.parse_clip(single)
    assert hd["table"][0] == hd["table"][1] == hd["table"][2] and len(buf) == len(single) + 16 * 2 * N == JC.container_bytes(plan.rates, plan.levels, 3, N)
    assert buf[hd["payload_start"]:] == single[hs["payload_start"]:]
    assert all(cr.frame_container(buf, k) == cr.frame_container(single, 0) for k in range(3))
    every, plan_all = encode(fmt, siting, O, still, target + 2 * (hi - fixed_of(3)), reuse=False)
    assert plan_all.source == [[f] * N for f in range(3)] and plan_all.weights == [1] * 18 and (plan_all.n_coded, plan_all.n_reused) == (18, 0)
    assert plan_all.rates == plan_big.rates * 3 and plan_all.plane_dists == plan_big.plane_dists * 3


@pytest.mark.parametrize("fmt,siting,O", CASES)
def test_frame_weights_and_importance_reach_the_allocator(fmt, siting, O):
    F = 6
    frames = device_clip(fmt, siting)
    plan0 = free(fmt, siting, O)[1]
    lo, hi = bounds(plan0, F)
    target = lo + (hi - lo) // 3
    fw = [Fraction(1, 3), 2, 5, 1, 7, 3]
    imp = [1, 1, Fraction(1, 1000), 1, 10 ** 6, 1]
    for kw in (dict(frame_weights=fw), dict(importance=[imp[:3], imp[3:]], frame_weights=fw), dict(plane_weights=(1, 0, 0))):
        plan = encode(fmt, siting, O, frames, target, **kw)[1]
        flat = imp if "importance" in kw else None
        weights = JC.weights(plan0.source, flat, kw.get("frame_weights"))
        pw = kw.get("plane_weights", (1, 1, 1))
        dists = [[sum(w * v for w, v in zip(pw, row)) for row in item] for item in plan0.plane_dists]
        assert plan.weights == weights and plan.rates == plan0.rates and plan.plane_dists == plan0.plane_dists and plan.dists == dists
        assert plan.levels == RC.allocate(plan0.rates, dists, JC.budget(target, F, N), weights), kw
        assert plan.container_bytes <= target


@pytest.mark.parametrize("O", [0, 16])
def test_centre_sited_nv12_is_clip_rate_s_encoder(O):
    """the levels, rates, plane_dists and every tile's blob are clip_rate.encode_clip_to_size's; the containers differ in their headers
    (47 bytes against 42) and so in every offset"""
    from progressivecodec_amd import clip_rate
    cr = CR()
    frames = device_clip("nv12", "centre")
    F = len(frames)
    plan0 = free("nv12", "centre", O)[1]
    lo, hi = bounds(plan0, F)
    for target in (lo + (hi - lo) // 3, hi):
        buf, plan = encode("nv12", "centre", O, frames, target)
        obuf, oplan = clip_rate.encode_clip_to_size(gpu_codec(), frames, QUALITIES, target - 5, "nv12", tile=T, overlap=O, mask_pol=POL)
        assert plan[:-1] == oplan._replace(container_bytes=len(buf)) and len(buf) == len(obuf) + 5
        hd, ohd = cr.parse_clip(buf), clip_rate.parse_clip(obuf)
        for k in range(F):
            for t in range(N):
                assert cr.tile_blob(buf, hd, k, t)[0] == clip_rate.tile_blob(obuf, ohd, k, t)[0], (k, t)

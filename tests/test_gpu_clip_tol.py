"""Tolerant clips on the GPU (progressivecodec_amd/clip_tol.py, libpc_clip_tol.so) against their restatement
(tests/clip_tol_contract.py): the scan's source table and all nine numbers of every tile of every frame, on both access paths, and
clip_tol.encode_clip through the codec against clips.encode_clip / clips.decode_clip.  Every comparison is exact equality of integers
or bytes.  T = 64 throughout: the smallest tile, so that the frames stay small while every branch (one tile, several tiles, partial
last tiles with odd edges, a halo on every side or on none) is taken."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import clip_tol_contract as TOL
from tests import clips_contract as CC
from tests import frames_contract as FC
from tests import tiles_contract as TC
from tests.test_gpu_clips import views
from tests.util import gpu_codec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POL = "point-based-std"
T = 64
F = 5
SIZES = [(1, 1), (2, 2), (64, 64), (65, 63), (100, 150), (127, 129)]
OVERLAPS = [0, 4, 16, 32]
NO = TOL.NO_MSE
POISON32 = -0x5A5A5A5B                                                     # 0xA5A5A5A5
POISON64 = -0x5A5A5A5A5A5A5A5B
#: how the frames of one table lie in memory, frame k taking entry k % 2: aligned with row strides that are multiples of 4, but
#: different ones; pitched with a stride that is none, next to an aligned one; one element past an allocation start, next to a
#: contiguous one.  By construction only the first table is wide, and two neighbours in a table never share a pitch.
TABLES = [(("pad4", 0), ("wider", 0)), (("loose", 0), ("pad4", 0)), (("pad4", 1), ("tight", 0))]


def CT():
    from progressivecodec_amd import clip_tol
    return clip_tol


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def planes_of(f):
    return tuple(torch.from_numpy(p[0]).to(DEV) for p in f)


def clip_codes(fmt, H, W, kind, seed):
    """F frames from one random frame -> (the frames, a, the tolerances to scan it under as (max_abs, mse_q10, max_run)).
    "noise": every sample of frames 1 .. moves by at most a = 3 from frame 0 (and in the larger planes some sample by exactly a);
    "ramp": every code rises by 1 per frame; "few": a few hundred random large changes per frame, on top of the frame before."""
    g = np.random.default_rng(seed)
    top = 1 << FC.bits(fmt)
    Hc, Wc = FC.chroma_size(H, W)
    shapes = ((1, H, W), (1, Hc, Wc), (1, Hc, Wc))
    a = 3
    base = [g.integers(F + a, top - F - a, s, dtype=np.int64) for s in shapes]
    clip = [base]
    for k in range(1, F):
        if kind == "noise":
            clip.append([c + g.integers(-a, a + 1, c.shape) for c in base])
        elif kind == "ramp":
            clip.append([c + k for c in base])
        else:
            nxt = [np.array(c) for c in clip[-1]]
            for c in nxt:
                flat = c.reshape(-1)
                idx = g.choice(flat.size, min(flat.size, 300), replace=False)
                flat[idx] = (flat[idx] + 1 + g.integers(0, top - 1, idx.size)) % top
            clip.append(nxt)
    frames = [FC.frame(*c, fmt) for c in clip]
    if fmt == "p010":                                                      # low bits on top of the later frames: they change no code
        frames = [frames[0]] + [tuple(p | g.integers(0, 64, p.shape).astype(np.uint16) for p in f) for f in frames[1:]]
    if kind == "noise":
        tols = [((a,) * 3, (NO,) * 3, 0), ((a - 1,) * 3, (NO,) * 3, 0), ((a,) * 3, (TOL.mse_q10(4), TOL.mse_q10(3.9), TOL.mse_q10(4.1)), 3)]
    elif kind == "ramp":
        tols = [((2, 2, 2), (NO,) * 3, 0), ((3, 1, 3), (NO, NO, 1024), 0)]
    else:
        tols = [((0, 0, 0), (NO,) * 3, 0), ((top - 1,) * 3, (TOL.mse_q10(top * top / 3000), NO, NO), 2)]
    return frames, a, tols


def scan_raw(table, fmt, up, H, W, O, tol, n, n_frames=None, nbytes=None, T_=T):
    """pc_clip_tol_scan -> (status, source int32 [F + 2, n] and stats int64 [F + 2, n, 3, 3] whose rows 1 .. F are the call's,
    poisoned beforehand, whether the workspace was written exactly where the call may: every partial (if a step ran) and every anchor,
    and no byte after them -- or, for a refused call, none at all).  table: per frame its planes as batched views."""
    from progressivecodec_amd import frames
    ct = CT()
    L = ct.lib()
    nf = len(table) if n_frames is None else n_frames
    rows = max(nf, 0) + 2
    source = torch.full((rows, n), POISON32, dtype=torch.int32, device=DEV)
    stats = torch.full((rows, n, 3, 3), POISON64, dtype=torch.int64, device=DEV)
    need = L.pc_clip_tol_workspace_size(T_, n)
    ws = torch.full((need // 8 + 2,), POISON64, dtype=torch.int64, device=DEV)
    host, dev = ct._frame_table(table, torch.device(DEV))
    rc = L.pc_clip_tol_scan(host, dev.data_ptr(), nf, frames.FORMATS.get(fmt, fmt), frames.UPSAMPLES.get(up, up), H, W, T_, O,
                            (C.c_int * 3)(*tol[0]), (C.c_int * 3)(*tol[1]), tol[2], ws.data_ptr(), need if nbytes is None else nbytes,
                            source[1:].data_ptr(), stats[1:].data_ptr(), stream())
    h = ws.cpu().view(torch.int32)
    npart = 18 * n * (T_ * T_ // 4096 + 1)                                 # 32-bit words of partials; then n of anchors
    if rc != 0:
        ws_ok = bool((h == POISON32).all())
    else:
        part = h[:npart]
        ws_ok = bool((h[npart:npart + n] != POISON32).all() and (h[npart + n:] == POISON32).all()
                     and ((part != POISON32).all() if nf > 1 else (part == POISON32).all()))
    del dev
    return rc, source, stats, ws_ok


def check(source, stats, want, case):
    """the guard rows keep their bits, the rows between are the restatement's"""
    s, st = source.cpu(), stats.cpu()
    assert (s[0] == POISON32).all() and (s[-1] == POISON32).all() and (st[0] == POISON64).all() and (st[-1] == POISON64).all(), case
    assert s[1:-1].tolist() == want[0], case
    assert st[1:-1].tolist() == want[1], case


@pytest.mark.parametrize("hw", SIZES)
def test_scan_exact_on_both_paths(hw):
    """every overlap x format x upsampling against the restatement, for clips of noise within a tolerance, a ramp and random large
    changes; the frame tables aligned, pitched and offset by one element, the frames of a table pitched differently; source, stats and
    the workspace poisoned.  Wide exactly where pc_clip_tol_plan says."""
    ct = CT()
    H, W = hw
    seen = set()
    for O in OVERLAPS:
        ny, nx = TC.grid(H, W, T, O)
        n = ny * nx
        for i, fmt in enumerate(FC.FORMATS):
            for kind in ("noise", "ramp", "few"):
                clip, a, tols = clip_codes(fmt, H, W, kind, seed=1000 * H + W + O + i)
                tables = [[views(fmt, H, W, *tb[k % 2], clip[k]) for k in range(F)] for tb in TABLES]
                for up in FC.UPSAMPLES:
                    for j, tol in enumerate(tols):
                        want = TOL.scan(clip, fmt, T, O, up, *tol)
                        if kind == "noise" and j == 0:
                            assert want[0] == [[0] * n] * F                # within a of the anchor, frame 0, however long the run
                        if kind == "noise" and j == 1:                     # recoded in every tile that drew an a, and only there
                            drew = [any(m[2] == a for m in want[1][1][t]) for t in range(n)]
                            assert [s == 1 for s in want[0][1]] == drew and (any(drew) or H * W < 64)
                        if kind == "ramp" and j == 0:
                            assert want[0] == [[v] * n for v in [0, 0, 0, 3, 3]]
                        for p, table in enumerate(tables):
                            expect = p == 0 and O % 8 == 0
                            wide = ct.plan(table, fmt, overlap=O)
                            assert wide is expect, (H, W, O, fmt, p)
                            seen.add(wide)
                            case = (H, W, O, fmt, kind, up, j, p)
                            rc, source, stats, ws_ok = scan_raw(table, fmt, up, H, W, O, tol, n)
                            assert rc == 0 and ws_ok, case
                            check(source, stats, want, case)
    assert seen == {True, False}


def test_refused_scans_launch_nothing():
    ct = CT()
    H, W, O = 100, 150, 16
    for fmt in ("nv12", "p010"):
        clip, _, tols = clip_codes(fmt, H, W, "few", seed=3)
        table = [views(fmt, H, W, *TABLES[1][k % 2], clip[k]) for k in range(F)]
        top = (1 << FC.bits(fmt)) - 1
        ok = dict(fmt=fmt, up="linear", H=H, W=W, O=O, tol=tols[1], n=6)
        need = ct.lib().pc_clip_tol_workspace_size(T, 6)
        for kw in [dict(O=6), dict(nbytes=need - 1), dict(fmt=3), dict(fmt=-1), dict(up=2), dict(up=-1), dict(H=0), dict(n_frames=0), dict(T_=96),
                   dict(tol=((top + 1, 0, 0), (NO,) * 3, 0)), dict(tol=((0, 0, 0), (NO + 1, 0, 0), 0)), dict(tol=((0, 0, 0), (0, 0, 0), -1))]:
            rc, source, stats, ws_ok = scan_raw(table, **dict(ok, **kw))
            torch.cuda.synchronize()
            assert rc == -1 and (source == POISON32).all() and (stats == POISON64).all() and ws_ok, (fmt, kw)
        rc, source, stats, ws_ok = scan_raw(table, **ok)                                   # unspoilt, it goes through
        assert rc == 0 and ws_ok
        check(source, stats, TOL.scan(clip, fmt, T, O, "linear", *tols[1]), fmt)
    with pytest.raises(ct.ClipTolError, match="PC_ERR_ARG"):
        raise ct.ClipTolError(-1, "pc_clip_tol_scan")


def test_halo_recodes_under_linear_only():
    """a flat frame; one changed chroma sample in the halo row above tile (1, 1), in the halo column to its left and in the one to its
    right: tile (1, 1) is recoded under linear upsampling and not under nearest"""
    ct = CT()
    H, W, O = 100, 150, 16                                                 # S = 48: tile (1, 1) holds chroma rows 24 .. 49, columns 24 .. 55
    Hc, Wc = FC.chroma_size(H, W)
    for fmt in FC.FORMATS:
        flat = [np.full(s, 90, np.int64) for s in ((1, H, W), (1, Hc, Wc), (1, Hc, Wc))]
        f0 = FC.frame(*flat, fmt)
        for p, (row, col) in [(1, (23, 40)), (2, (30, 23)), (1, (30, 56)), (2, (23, 23))]:
            c = [np.array(q) for q in flat]
            c[p][0, row, col] += 1
            clip = [f0, FC.frame(*c, fmt)]
            for up, recoded in (("linear", 1), ("nearest", 0)):
                want = TOL.scan(clip, fmt, T, O, up)
                assert want[0][1][4] == recoded and want[1][1][4][p] == [recoded] * 3
                source, stats = ct.scan_clip([planes_of(f) for f in clip], fmt, ct.Tolerance(), T, O, up)
                assert source.tolist() == want[0] and stats.tolist() == want[1], (fmt, p, row, col, up)
                # a tolerance of one code takes the halo back in
                source, _ = ct.scan_clip([planes_of(f) for f in clip], fmt, ct.Tolerance(1), T, O, up)
                assert source.tolist() == [[0] * 6] * 2


def test_equalities_one_frame_zero_tolerance_and_max_run_1():
    from progressivecodec_amd import clips
    ct = CT()
    for fmt, (H, W), O, up in [("nv12", (100, 150), 16, "linear"), ("i420", (127, 129), 0, "nearest"), ("p010", (65, 63), 4, "linear")]:
        n = int(np.prod(TC.grid(H, W, T, O)))
        clip, _, _ = clip_codes(fmt, H, W, "few", seed=H)
        clip = clip[:3] + [clip[2]] + clip[3:]                             # a frame that repeats the one before it
        frames = [planes_of(f) for f in clip]
        # F = 1: row 0 and nothing else
        for mode, off in (("pad4", 0), ("loose", 1)):
            rc, source, stats, ws_ok = scan_raw([views(fmt, H, W, mode, off, clip[0])], fmt, up, H, W, O, ((1, 1, 1), (NO,) * 3, 0), n)
            assert rc == 0 and ws_ok
            check(source, stats, ([[0] * n], [[[[0, 0, 0]] * 3] * n]), fmt)
        source, stats = ct.scan_clip(frames[:1], fmt, ct.Tolerance(5), T, O, up)
        assert source.dtype == torch.int32 and stats.dtype == torch.int64 and source.device.type == "cuda" and stats.device.type == "cuda"
        assert source.tolist() == [[0] * n] and stats.shape == (1, n, 3, 3) and not stats.any()
        # tolerance 0: section 16's source table, from section 16's kernel
        counts = clips.clip_changes(frames, fmt, T, O, up)
        want = clips.source_table((counts != 0).any(dim=2).tolist())
        source, stats = ct.scan_clip(frames, fmt, ct.Tolerance(), T, O, up)
        assert source.shape == (len(clip), n) and stats.shape == (len(clip), n, 3, 3)
        assert source.tolist() == want == CC.source_table(clip, fmt, T, O, up) == TOL.scan(clip, fmt, T, O, up)[0]
        assert source[3].tolist() == source[2].tolist() and any(s == 1 for s in want[1])
        assert stats[1, :, :, 0].tolist() == counts[0].tolist()            # against frame 0 the counts are section 16's
        batched = tuple(torch.stack(ps) for ps in zip(*frames))
        sb, stb = ct.scan_clip(batched, fmt, ct.Tolerance(), T, O, up)
        assert torch.equal(sb, source) and torch.equal(stb, stats)
        # on a second stream
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            ss, sst = ct.scan_clip(frames, fmt, ct.Tolerance(), T, O, up)
        side.synchronize()
        assert torch.equal(ss, source) and torch.equal(sst, stats)
        # max_run = 1 codes everything, whatever the tolerance
        for tol in (ct.Tolerance(max_run=1), ct.Tolerance((1 << FC.bits(fmt)) - 1, max_run=1)):
            source, stats = ct.scan_clip(frames, fmt, tol, T, O, up)
            assert source.tolist() == [[k] * n for k in range(len(clip))]
            assert stats.tolist() == TOL.scan(clip, fmt, T, O, up, tol.max_abs, tol.mse_q10, 1)[1]
        with pytest.raises(ValueError, match="at most 255" if fmt != "p010" else "max_abs"):
            ct.scan_clip(frames, fmt, ct.Tolerance(256) if fmt != "p010" else ct.Tolerance(1024), T, O, up)


# -- through the codec ---------------------------------------------------------------------------------------------------------------

QUALITIES = [0, 0.5]
CODEC_CLIPS = [("nv12", 100, 150, 16), ("p010", 65, 63, 4)]               # 2 x 3 tiles, S = 48; 2 x 1 tiles, S = 60


@functools.lru_cache(maxsize=None)
def smooth_frame(fmt, H, W):
    """a smooth frame (the codec's synthetic weights are not meant for noise; any frame does)"""
    g = np.random.default_rng(H + W)
    lo = torch.from_numpy(g.uniform(0.2, 0.8, (1, 3, 8, 8)).astype(np.float32))
    x = torch.nn.functional.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False).numpy()
    return FC.emit(x, 0, 0, H, W, fmt, "bt709", "limited")


def exact_clip(fmt, H, W):
    """four frames: one luma sample changes for frame 1, nothing for frame 2, one Cb sample for frame 3"""
    sh = 6 if fmt == "p010" else 0
    f0 = tuple(np.array(p) for p in smooth_frame(fmt, H, W))
    f1 = tuple(np.array(p) for p in f0)
    f1[0][0, 10, 10] ^= 0x80 << sh
    f3 = tuple(np.array(p) for p in f1)
    f3[1][0, 23, 20, 0] ^= 0x80 << sh
    return [f0, f1, f1, f3]


def noisy_clip(fmt, H, W):
    """four frames: the smooth frame (its codes lie well inside the code range), then three times that frame plus seeded noise of
    -1, 0, +1 on every sample -- every frame within one code of frame 0, two later frames up to two codes apart"""
    g = np.random.default_rng(7)
    base = [np.array(c) for c in FC.codes(smooth_frame(fmt, H, W), fmt)]
    return [FC.frame(*base, fmt)] + [FC.frame(*[c + g.integers(-1, 2, c.shape) for c in base], fmt) for _ in range(3)]


@pytest.mark.parametrize("case", CODEC_CLIPS, ids=lambda c: c[0])
def test_encode_clip_through_the_codec(case):
    from progressivecodec_amd import clips, frame_tiles
    ct = CT()
    fmt, H, W, O = case
    net = gpu_codec()
    n = int(np.prod(TC.grid(H, W, T, O)))
    kw = dict(tile=T, overlap=O, upsample="linear", mask_pol=POL)
    same = lambda a, b: len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))                           # noqa: E731
    # tolerance 0 is clips.encode_clip, byte for byte
    clip = exact_clip(fmt, H, W)
    frames = [planes_of(f) for f in clip]
    buf0, plan0 = clips.encode_clip(net, frames, QUALITIES, fmt, **kw)
    buf, plan = ct.encode_clip(net, frames, QUALITIES, fmt, tolerance=ct.Tolerance(), **kw)
    assert isinstance(buf, bytes) and buf == buf0 and plan[:4] == tuple(plan0) and 0 < plan.n_reused < 4 * n
    assert plan.stats == TOL.scan(clip, fmt, T, O, "linear")[1] and plan.worst == [0, 0, 0]
    # +-1 noise: the exact test reuses nothing, a tolerance of one code every tile of frames 1 - 3
    clip = noisy_clip(fmt, H, W)
    frames = [planes_of(f) for f in clip]
    exact, plan_exact = clips.encode_clip(net, frames, QUALITIES, fmt, **kw)
    assert (plan_exact.n_coded, plan_exact.n_reused) == (4 * n, 0)
    every, plan_every = clips.encode_clip(net, frames, QUALITIES, fmt, reuse=False, **kw)
    assert every == exact and plan_every.source == plan_exact.source
    hd = clips.parse_clip(every)
    blobs = [[clips.clip_tile_bytes(every, hd, f, t)[0] for t in range(n)] for f in range(4)]
    for tol, source in [(ct.Tolerance(1), [[0] * n] * 4), (ct.Tolerance(1, max_run=2), [[0] * n, [0] * n, [2] * n, [3] * n]),     # frame 3 is two codes from its anchor, frame 2
                        (ct.Tolerance((1, 0, 1)), None)]:
        buf, plan = ct.encode_clip(net, frames, QUALITIES, fmt, tolerance=tol, **kw)
        want = TOL.scan(clip, fmt, T, O, "linear", *tol)
        assert plan.source == want[0] and plan.stats == want[1] and plan.worst == TOL.worst(*want)
        n_coded = sum(s == f for f, row in enumerate(plan.source) for s in row)
        assert (plan.n_coded, plan.n_reused, plan.container_bytes) == (n_coded, 4 * n - n_coded, len(buf))
        if source is not None:
            assert plan.source == source and plan.worst == [1, 1, 1] and len(buf) < len(exact)
        else:
            assert plan.n_reused == 0 and buf == exact                     # Cb moved by a code in every footprint
        # the container: the blobs of reuse=False, selected by plan.source
        assert buf == clips.pack_clip(blobs, plan.source, H, W, T, O, fmt, "bt709", "limited", "linear")
        assert buf == CC.pack_clip(blobs, plan.source, H, W, T, O, fmt, "bt709", "limited", "linear", hd["contract"])
        # clips.decode_clip reads it, and frame k is decode_frame_tiled of its own container
        got = clips.decode_clip(net, buf)
        assert len(got) == 4
        for k in range(4):
            assert same(got[k], frame_tiles.decode_frame_tiled(net, clips.frame_container(buf, k))), k
            assert clips.frame_container(buf, k) == clips.frame_container(every, plan.source[k][0]) or len(set(plan.source[k])) > 1
        if source is not None and tol.max_run == 2:
            # the bytes and the plan depend neither on max_tiles_per_call nor on how the frames lie in memory
            for per_call in (1, 5, 32):
                assert ct.encode_clip(net, frames, QUALITIES, fmt, tolerance=tol, max_tiles_per_call=per_call, **kw) == (buf, plan), per_call
            batched = tuple(torch.stack(ps) for ps in zip(*frames))
            assert ct.encode_clip(net, batched, QUALITIES, fmt, tolerance=tol, **kw) == (buf, plan)
            pitched = [tuple(v[0] for v in views(fmt, H, W, "loose", 1, f)) for f in clip]
            assert ct.encode_clip(net, pitched, QUALITIES, fmt, tolerance=tol, **kw) == (buf, plan)

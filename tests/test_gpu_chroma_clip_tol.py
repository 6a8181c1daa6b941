"""Tolerant clips of YUV frames of any subsampling and siting on the GPU (progressivecodec_amd/chroma_clip_tol.py,
libpc_chroma_clip_tol.so) against their restatement (tests/chroma_clip_tol_contract.py): the scan's source table and all nine numbers
of every tile of every frame, on both access paths, and chroma_clip_tol.encode_clip through the codec against chroma_clips.encode_clip /
decode_clip.  Every comparison is exact equality of integers or bytes.  T = 64 and F = 5 throughout.  The matrix is
tests/chroma_clip_tol_cases.py's table (section 25's); every case asserts the access path the table predicts."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import chroma_clip_tol_cases as CS
from tests import chroma_clip_tol_contract as TOL
from tests import chroma_clips_contract as CK
from tests import chroma_contract as CC
from tests import clip_tol_contract as TOL18
from tests import frames_contract as FC
from tests import tiles_contract as TC
from tests.test_gpu_chroma_clips import other_bits, views
from tests.test_gpu_chroma_tiles import codec_frame, on_device
from tests.util import gpu_codec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POL = "point-based-std"
T = CS.T
F = CS.F
NO = TOL.NO_MSE
POISON32 = -0x5A5A5A5B                                                     # 0xA5A5A5A5
POISON64 = -0x5A5A5A5A5A5A5A5B


def CT():
    from progressivecodec_amd import chroma_clip_tol
    return chroma_clip_tol


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


@functools.lru_cache(maxsize=None)
def clip_codes(fmt, H, W, kind, seed):
    """F frames from one random frame -> (the frames, a, the tolerances to scan it under as (max_abs, mse_q10, max_run)): section 18's
    three kinds with its tolerances per kind.  "noise": every sample of frames 1 .. moves by at most a = 3 from frame 0; "ramp": every
    code rises by 1 per frame; "few": a few hundred random large changes per frame, on top of the frame before.  For the 16-bit
    formats the bits outside the code are random in the later frames: they change no code."""
    g = np.random.default_rng(seed)
    top = 1 << CC.bits(fmt)
    Hc, Wc = CC.chroma_size(H, W, fmt)
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
    frames = [CC.frame(*c, fmt) for c in clip]
    frames = [frames[0]] + [other_bits(f, fmt, g) for f in frames[1:]]
    if kind == "noise":
        tols = [((a,) * 3, (NO,) * 3, 0), ((a - 1,) * 3, (NO,) * 3, 0), ((a,) * 3, (TOL.mse_q10(4), TOL.mse_q10(3.9), TOL.mse_q10(4.1)), 3)]
    elif kind == "ramp":
        tols = [((2, 2, 2), (NO,) * 3, 0), ((3, 1, 3), (NO, NO, 1024), 0)]
    else:
        tols = [((0, 0, 0), (NO,) * 3, 0), ((top - 1,) * 3, (TOL.mse_q10(top * top / 3000), NO, NO), 2)]
    return frames, a, tols


@functools.lru_cache(maxsize=None)
def clip_tables(fmt, H, W, kind, seed):
    clip = clip_codes(fmt, H, W, kind, seed)[0]
    return [[views(fmt, H, W, *tb[k % 2], clip[k]) for k in range(F)] for tb in CS.TABLES]


def scan_raw(table, fmt, siting, up, H, W, O, tol, n, n_frames=None, nbytes=None, T_=T, **raw):
    """pc_chroma_clip_tol_scan -> (status, source int32 [F + 2, n] and stats int64 [F + 2, n, 3, 3] whose rows 1 .. F are the call's,
    poisoned beforehand, whether the workspace was written exactly where the call may: every partial (if a step ran) and every anchor,
    and no byte after them -- or, for a refused call, none at all).  table: per frame its planes as batched views.  raw: format,
    siting or upsampling integers that replace the names', and null pointers, for the calls that are to be refused."""
    from progressivecodec_amd import chroma, clips, frames
    L = CT().lib()
    f = dict(chroma.FORMATS[fmt]._asdict(), hsite=chroma.SITINGS[siting][0], vsite=chroma.SITINGS[siting][1], up=frames.UPSAMPLES.get(up, up))
    f.update({k: v for k, v in raw.items() if k in f})
    nf = len(table) if n_frames is None else n_frames
    rows = max(nf, 0) + 2
    source = torch.full((rows, n), POISON32, dtype=torch.int32, device=DEV)
    stats = torch.full((rows, n, 3, 3), POISON64, dtype=torch.int64, device=DEV)
    sy = chroma.FORMATS[fmt].sy
    need = L.pc_chroma_clip_tol_workspace_size(T_, sy, n) or L.pc_chroma_clip_tol_workspace_size(T, sy, n)
    ws = torch.full((need // 8 + 2,), POISON64, dtype=torch.int64, device=DEV)
    host, dev = clips._frame_table(table, torch.device(DEV))
    rc = L.pc_chroma_clip_tol_scan(host if not raw.get("no_host") else None, dev.data_ptr() if not raw.get("no_dev") else None, nf, *f.values(),
                                   H, W, T_, O, (C.c_int * 3)(*tol[0]), (C.c_int * 3)(*tol[1]), tol[2],
                                   ws.data_ptr() if not raw.get("no_ws") else None, need if nbytes is None else nbytes,
                                   source[1:].data_ptr() if not raw.get("no_source") else None,
                                   stats[1:].data_ptr() if not raw.get("no_stats") else None, stream())
    torch.cuda.synchronize()
    h = ws.cpu().view(torch.int32)
    npart = 18 * n * (T_ * T_ // (2048 * sy) + 1)                          # 32-bit words of partials; then n of anchors
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


# -- the case table ------------------------------------------------------------------------------------------------------------------

def run_scans(cases):
    ct = CT()
    seen = set()
    for c in cases:
        ny, nx = TC.grid(c.H, c.W, T, c.O)
        n = ny * nx
        seed = 1000 * c.H + c.W
        for kind in ("noise", "ramp", "few"):
            clip, a, tols = clip_codes(c.fmt, c.H, c.W, kind, seed)
            tables = clip_tables(c.fmt, c.H, c.W, kind, seed)
            for j, tol in enumerate(tols):
                want = TOL.scan(clip, c.fmt, c.siting, T, c.O, c.upsample, *tol)
                if kind == "noise" and j == 0:
                    assert want[0] == [[0] * n] * F                        # within a of the anchor, frame 0, however long the run
                if kind == "ramp" and j == 0:
                    assert want[0] == [[v] * n for v in [0, 0, 0, 3, 3]]
                for p, table in enumerate(tables):
                    wide = ct.plan(table, c.fmt, overlap=c.O)
                    assert wide is CS.wide(c, p), (c, p)
                    seen.add(CS.kernel_tuple(c.fmt, wide))
                    rc, source, stats, ws_ok = scan_raw(table, c.fmt, c.siting, c.upsample, c.H, c.W, c.O, tol, n)
                    assert rc == 0 and ws_ok, (c, kind, j, p)
                    check(source, stats, want, (c, kind, j, p))
    return seen


@pytest.mark.parametrize("fmt", sorted(CC.FORMATS))
def test_scan_of_every_format_siting_and_upsampling(fmt):
    """100 x 150 with O in {0, 4}: clips of noise within a tolerance, a ramp and random large changes under section 18's tolerances;
    the frame tables aligned, pitched and offset by one element, the frames of a table pitched differently; source, stats and the
    workspace poisoned, with guard rows.  Wide exactly where pc_chroma_clip_tol_plan says."""
    cases = CS.main_cases(fmt)
    assert run_scans(cases) == CS.reached(cases) == {CS.kernel_tuple(fmt, False), CS.kernel_tuple(fmt, True)}


@pytest.mark.parametrize("fmt", CS.OTHER_FORMATS)
def test_scan_at_the_other_sizes_and_overlaps(fmt):
    cases = CS.other_cases(fmt)
    assert run_scans(cases) == CS.reached(cases)


def test_bits_outside_the_code_change_nothing():
    """16-bit formats: later frames that differ from frame 0 in the bits outside the code alone"""
    ct = CT()
    H, W, O = 100, 150, 4
    for fmt, siting in (("p210", "left"), ("i410", "centre"), ("p010", "topleft"), ("i010", "left")):
        g = np.random.default_rng(5)
        f0 = CC.random_frame(1, H, W, fmt, seed=9)
        clip = [f0] + [other_bits(f0, fmt, g) for _ in range(2)]
        assert any((a != b).any() for a, b in zip(clip[0], clip[1]))
        n = int(np.prod(TC.grid(H, W, T, O)))
        assert TOL.scan(clip, fmt, siting, T, O, "linear") == ([[0] * n] * 3, [[[[0, 0, 0]] * 3] * n] * 3)
        source, stats = ct.scan_clip([on_device(f) for f in clip], fmt, ct.Tolerance(), siting, T, O, "linear")
        assert source.tolist() == [[0] * n] * 3 and not stats.any(), fmt


# -- the halo ------------------------------------------------------------------------------------------------------------------------

def one_sample_clip(fmt, H, W, plane, where):
    """a smooth frame and the same frame with one sample changed"""
    prev = codec_frame(H, W, fmt, "centre")
    codes = [np.array(c) for c in CC.codes(prev, fmt)]
    codes[plane][0][where] ^= 1 << (CC.bits(fmt) - 1)
    return [prev, CC.frame(*codes, fmt)]


#: (format, the changed Cb sample, [(siting, upsampling, the tiles recoded)]): T = 64, O = 0, 100 x 150 is 2 x 3 tiles; tile (0, 1)
#: starts at chroma column 32 of a 4:2:2 frame and tile (1, 0), number 3, at chroma row 32 of a 4:2:0 one
HALO = [
    ("p210", (10, 31), [("centre", "linear", [0, 1]), ("left", "linear", [0]), ("topleft", "linear", [0]), ("centre", "nearest", [0]),
                        ("left", "nearest", [0])]),
    ("p210", (10, 32), [("centre", "linear", [0, 1]), ("left", "linear", [0, 1]), ("topleft", "linear", [0, 1]), ("centre", "nearest", [1]),
                        ("left", "nearest", [1])]),
    ("nv12", (31, 10), [("centre", "linear", [0, 3]), ("left", "linear", [0, 3]), ("topleft", "linear", [0]), ("centre", "nearest", [0]),
                        ("topleft", "nearest", [0])]),
    ("nv12", (32, 10), [("centre", "linear", [0, 3]), ("left", "linear", [0, 3]), ("topleft", "linear", [0, 3]), ("centre", "nearest", [3]),
                        ("topleft", "nearest", [3])]),
]


def test_the_halo_rule_on_the_device():
    """one Cb sample changed, zero tolerance: the tiles recoded are those whose footprint holds it under the siting and the upsampling.
    The restatement's table is the authority, and gives exactly this."""
    ct = CT()
    H, W, O = 100, 150, 0
    for fmt, where, rows in HALO:
        clip = one_sample_clip(fmt, H, W, 1, where)
        frames = [on_device(f) for f in clip]
        for siting, up, recoded in rows:
            want = TOL.scan(clip, fmt, siting, T, O, up)
            assert [t for t, s in enumerate(want[0][1]) if s == 1] == recoded, (fmt, where, siting, up)
            assert all(want[1][1][t][1][0] == 1 and want[1][1][t][0] == [0, 0, 0] for t in recoded)
            source, stats = ct.scan_clip(frames, fmt, ct.Tolerance(), siting, T, O, up)
            assert source.tolist() == want[0] and stats.tolist() == want[1], (fmt, where, siting, up)


# -- equalities ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_centre_sited_420_is_clip_tol_on_the_device(fmt):
    from progressivecodec_amd import clip_tol
    ct = CT()
    H, W = 100, 150
    for kind in ("noise", "ramp", "few"):
        clip, _, tols = clip_codes(fmt, H, W, kind, 77)
        frames = [on_device(f) for f in clip]
        for O, up in ((0, "linear"), (4, "nearest"), (16, "linear")):
            for tol in tols:
                tl = ct.Tolerance(tol[0], [None if q == NO else q / 1024 for q in tol[1]], tol[2] or None)
                assert (tl.max_abs, tl.mse_q10, tl.max_run) == tol
                ours = ct.scan_clip(frames, fmt, tl, "centre", T, O, up)
                theirs = clip_tol.scan_clip(frames, fmt, tl, T, O, up)
                assert torch.equal(ours[0], theirs[0]) and torch.equal(ours[1], theirs[1]), (fmt, kind, O, up, tol)
                want = TOL18.scan(clip, fmt, T, O, up, *tol)
                assert ours[0].tolist() == want[0] and ours[1].tolist() == want[1]


def test_equalities_one_frame_zero_tolerance_and_max_run_1():
    from progressivecodec_amd import chroma_clips, clips
    ct = CT()
    for fmt, siting, (H, W), O, up in [("p210", "left", (100, 150), 16, "linear"), ("i444", "centre", (127, 129), 0, "nearest"),
                                       ("nv12", "topleft", (65, 63), 4, "linear")]:
        n = int(np.prod(TC.grid(H, W, T, O)))
        clip = list(clip_codes(fmt, H, W, "few", H)[0])
        clip = clip[:3] + [clip[2]] + clip[3:]                             # a frame that repeats the one before it
        frames = [on_device(f) for f in clip]
        # F = 1: row 0 and the anchors, and the partials untouched
        for mode, off in (("pad4", 0), ("loose", 1)):
            rc, source, stats, ws_ok = scan_raw([views(fmt, H, W, mode, off, clip[0])], fmt, siting, up, H, W, O, ((1, 1, 1), (NO,) * 3, 0), n)
            assert rc == 0 and ws_ok
            check(source, stats, ([[0] * n], [[[[0, 0, 0]] * 3] * n]), fmt)
        source, stats = ct.scan_clip(frames[:1], fmt, ct.Tolerance(5), siting, T, O, up)
        assert source.dtype == torch.int32 and stats.dtype == torch.int64 and source.device.type == "cuda" and stats.device.type == "cuda"
        assert source.tolist() == [[0] * n] and stats.shape == (1, n, 3, 3) and not stats.any()
        # tolerance 0: section 25's source table, from section 25's kernel; the counts are changes_item's wherever the anchor is the
        # previous frame
        counts = chroma_clips.clip_changes(frames, fmt, siting, T, O, up)
        want = clips.source_table((counts != 0).any(dim=2).tolist())
        source, stats = ct.scan_clip(frames, fmt, ct.Tolerance(), siting, T, O, up)
        assert source.shape == (len(clip), n) and stats.shape == (len(clip), n, 3, 3)
        assert source.tolist() == want == CK.source_table(clip, fmt, siting, T, O, up) == TOL.scan(clip, fmt, siting, T, O, up)[0]
        assert source[3].tolist() == source[2].tolist() and any(s == 1 for s in want[1])
        assert stats[1, :, :, 0].tolist() == counts[0].tolist()
        tied = 0
        for k in range(1, len(clip)):
            for t in range(n):
                if want[k - 1][t] == k - 1:
                    assert stats[k, t, :, 0].tolist() == counts[k - 1, t].tolist(), (fmt, k, t)
                    tied += 1
        assert tied > n
        batched = tuple(torch.stack(ps) for ps in zip(*frames))
        sb, stb = ct.scan_clip(batched, fmt, ct.Tolerance(), siting, T, O, up)
        assert torch.equal(sb, source) and torch.equal(stb, stats)
        # max_run = 1 codes everything, whatever the tolerance
        for tol in (ct.Tolerance(max_run=1), ct.Tolerance((1 << CC.bits(fmt)) - 1, max_run=1)):
            source, stats = ct.scan_clip(frames, fmt, tol, siting, T, O, up)
            assert source.tolist() == [[k] * n for k in range(len(clip))]
            assert stats.tolist() == TOL.scan(clip, fmt, siting, T, O, up, tol.max_abs, tol.mse_q10, 1)[1]
        if CC.bits(fmt) == 8:
            with pytest.raises(ValueError, match="at most 255"):
                ct.scan_clip(frames, fmt, ct.Tolerance(256), siting, T, O, up)


def test_refused_scans_launch_nothing():
    ct = CT()
    H, W, O = 100, 150, 16
    for fmt, siting in (("nv16", "left"), ("p010", "topleft"), ("i444", "centre")):
        from progressivecodec_amd import chroma
        clip, _, tols = clip_codes(fmt, H, W, "few", 3)
        table = clip_tables(fmt, H, W, "few", 3)[1]
        top = (1 << CC.bits(fmt)) - 1
        ok = dict(fmt=fmt, siting=siting, up="linear", H=H, W=W, O=O, tol=tols[1], n=6)
        need = ct.lib().pc_chroma_clip_tol_workspace_size(T, chroma.FORMATS[fmt].sy, 6)
        for kw in [dict(T_=96), dict(T_=32), dict(T_=4096, O=0), dict(O=6), dict(O=36), dict(O=-4), dict(nbytes=need - 1), dict(nbytes=0),
                   dict(layout=2), dict(bits=9), dict(shift=3), dict(sx=3), dict(sy=0), dict(hsite=2), dict(vsite=-1), dict(up=2), dict(up=-1),
                   dict(no_host=1), dict(no_dev=1), dict(no_ws=1), dict(no_source=1), dict(no_stats=1), dict(H=0), dict(n_frames=0),
                   dict(tol=((top + 1, 0, 0), (NO,) * 3, 0)), dict(tol=((0, 0, 0), (NO + 1, 0, 0), 0)), dict(tol=((0, 0, 0), (0, 0, 0), -1))]:
            rc, source, stats, ws_ok = scan_raw(table, **dict(ok, **kw))
            assert rc == -1 and (source == POISON32).all() and (stats == POISON64).all() and ws_ok, (fmt, kw)
        rc, source, stats, ws_ok = scan_raw(table, **ok)                                   # unspoilt, it goes through
        assert rc == 0 and ws_ok
        check(source, stats, TOL.scan(clip, fmt, siting, T, O, "linear", *tols[1]), fmt)
    with pytest.raises(ct.ChromaClipTolError, match="PC_ERR_ARG"):
        raise ct.ChromaClipTolError(-1, "pc_chroma_clip_tol_scan")


# -- through the codec ---------------------------------------------------------------------------------------------------------------

QUALITIES = [0, 0.5]
H0, W0, O0 = 100, 150, 16                                                  # 2 x 3 tiles of 64 x 64, S = 48
CODEC = [("p210", "left"), ("nv12", "topleft"), ("i444", "centre")]


@functools.lru_cache(maxsize=None)
def codec_clips(fmt, siting):
    """-> (the noise-free clip, the noisy one).  Noise-free: a smooth frame; luma sample (10, 10) changed by half the range; that
    frame again; the Cb sample at chroma (23, 40) changed.  Noisy: seeded noise of 0 / +1 on every sample of every frame on top."""
    half = 1 << (CC.bits(fmt) - 1)
    c0 = [np.array(c) for c in CC.codes(codec_frame(H0, W0, fmt, siting), fmt)]
    c1 = [np.array(c) for c in c0]
    c1[0][0, 10, 10] ^= half
    c3 = [np.array(c) for c in c1]
    c3[1][0, 23, 40] ^= half
    clean = [c0, c1, c1, c3]
    g = np.random.default_rng(7)
    top = (1 << CC.bits(fmt)) - 1
    noisy = [[np.minimum(c + g.integers(0, 2, c.shape), top) for c in f] for f in clean]
    return [CC.frame(*c, fmt) for c in clean], [CC.frame(*c, fmt) for c in noisy]


@pytest.mark.parametrize("fmt,siting", CODEC)
def test_encode_clip_through_the_codec(fmt, siting):
    from progressivecodec_amd import chroma_clips, chroma_tiles
    ct = CT()
    net = gpu_codec()
    clean, noisy = codec_clips(fmt, siting)
    n, nf = 6, 4
    kw = dict(siting=siting, tile=T, overlap=O0, upsample="linear", mask_pol=POL)
    same = lambda a, b: len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))                           # noqa: E731
    # Tolerance() is chroma_clips.encode_clip, byte for byte
    frames = [on_device(f) for f in clean]
    buf0, plan0 = chroma_clips.encode_clip(net, frames, QUALITIES, fmt, **kw)
    buf, plan = ct.encode_clip(net, frames, QUALITIES, fmt, tolerance=ct.Tolerance(), **kw)
    table = CK.source_table(clean, fmt, siting, T, O0, "linear")
    assert isinstance(buf, bytes) and buf == buf0 and plan[:4] == tuple(plan0) and plan.source == table and 0 < plan.n_reused < nf * n
    assert plan.stats == TOL.scan(clean, fmt, siting, T, O0, "linear")[1] and plan.worst == [0, 0, 0]
    # 0 / +1 noise: the exact test reuses next to nothing, a tolerance of one code gives the noise-free clip's table
    frames = [on_device(f) for f in noisy]
    every, plan_every = chroma_clips.encode_clip(net, frames, QUALITIES, fmt, reuse=False, **kw)
    assert plan_every.source == [[f] * n for f in range(nf)]
    assert CK.source_table(noisy, fmt, siting, T, O0, "linear") == plan_every.source
    hd = chroma_clips.parse_clip(every)
    blobs = [[chroma_clips.clip_tile_bytes(every, hd, f, t)[0] for t in range(n)] for f in range(nf)]
    tol = ct.Tolerance(1)
    buf, plan = ct.encode_clip(net, frames, QUALITIES, fmt, tolerance=tol, **kw)
    want = TOL.scan(noisy, fmt, siting, T, O0, "linear", *tol)
    assert plan.source == want[0] == table and plan.stats == want[1] and plan.worst == TOL.worst(*want) == [1, 1, 1]
    n_coded = sum(s == f for f, row in enumerate(table) for s in row)
    assert (plan.n_coded, plan.n_reused, plan.container_bytes) == (n_coded, nf * n - n_coded, len(buf)) and len(buf) < len(every)
    # the container: the blobs of reuse=False, selected by plan.source
    assert buf == chroma_clips.pack_clip(blobs, plan.source, H0, W0, T, O0, fmt, "bt709", "limited", "linear", siting)
    assert buf == CK.pack_clip(blobs, plan.source, H0, W0, T, O0, fmt, "bt709", "limited", "linear", siting, hd["contract"])
    # the bytes and the plan depend neither on max_tiles_per_call nor on how the frames lie in memory
    assert ct.encode_clip(net, frames, QUALITIES, fmt, tolerance=tol, max_tiles_per_call=5, **kw) == (buf, plan)
    pitched = [tuple(v[0] for v in views(fmt, H0, W0, "loose", 1, f)) for f in noisy]
    assert ct.encode_clip(net, pitched, QUALITIES, fmt, tolerance=tol, **kw) == (buf, plan)
    # chroma_clips.decode_clip reads it, and frame k is decode_frame_tiled of its own container
    got = chroma_clips.decode_clip(net, buf)
    assert len(got) == nf
    for k in range(nf):
        assert same(got[k], chroma_tiles.decode_frame_tiled(net, chroma_clips.frame_container(buf, k))), k

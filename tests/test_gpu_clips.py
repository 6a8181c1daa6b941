"""Clips of YUV 4:2:0 frames on the GPU (progressivecodec_amd/clips.py, libpc_clips.so) against their restatement
(tests/clips_contract.py): the change counts over every tile's footprint, the cut of a list of tiles against frame_tiles.cut_frame and
tests/frame_tiles_contract.cut, both on both access paths, and encode_clip / decode_clip through the codec against the per-frame
encode_frame_tiled / decode_frame_tiled.  Every comparison is exact equality of integers, bits or bytes.  T = 64 throughout: the
smallest tile, so that the frames stay small while every branch (one tile, several tiles, partial last tiles with odd edges, a halo
on every side or on none) is taken."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import clips_contract as CC
from tests import frame_tiles_contract as GC
from tests import frames_contract as FC
from tests import tiles_contract as TC
from tests.test_gpu_frame_rate import codec_frame
from tests.test_gpu_frames import View, poison_of, up4
from tests.test_gpu_rate import POISON64, check_out
from tests.util import gpu_codec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POL = "point-based-std"
T = 64
SIZES = [(1, 1), (2, 2), (64, 64), (65, 63), (100, 150), (127, 129)]
OVERLAPS = [0, 4, 16, 32]
MATS = list(FC.MATRICES)
#: (cur, prev) as views: both aligned with row strides that are multiples of 4, but different ones; cur pitched with a stride that is
#: none; cur one element past an allocation start.  By construction only the first is wide, and cur and prev never share a pitch.
PAIRS = [(("pad4", 0), ("wider", 0)), (("loose", 0), ("pad4", 0)), (("pad4", 1), ("tight", 0))]


def CL():
    from progressivecodec_amd import clips
    return clips


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def plane_shapes(fmt, H, W):
    Hc, Wc = FC.chroma_size(H, W)
    return [(1, H, W), (1, Hc, Wc), (1, Hc, Wc)] if fmt == "i420" else [(1, H, W), (1, Hc, Wc, 2)]


def views(fmt, H, W, mode, offset, data):
    """the planes of a frame as cuda views `offset` elements past an allocation start; mode "wider": aligned rows eight elements (and
    a multiple of 4) longer than "pad4" would make them"""
    dt = np.uint16 if fmt == "p010" else np.uint8
    out = []
    for i, s in enumerate(plane_shapes(fmt, H, W)):
        if mode != "wider":
            out.append(View(s, dt, offset, mode, data[i]).t)
            continue
        rowlen = int(np.prod(s[2:]))
        sr = up4(rowlen) + 8
        host = np.full(s[1] * sr + 16, poison_of(dt), dt)
        strides = (s[1] * sr, sr, 2, 1) if len(s) == 4 else (s[1] * sr, sr, 1)
        np.lib.stride_tricks.as_strided(host, s, [v * host.itemsize for v in strides])[...] = data[i]
        out.append(torch.as_strided(torch.from_numpy(host).to(DEV), s, strides))
    return out


def frame_pair(fmt, H, W, kind, seed):
    """(cur, prev): prev random over the whole code range; cur differs from it in nothing ("none"), in a few hundred random samples of
    every plane ("few") or in every sample ("all"); for P010 cur's low six bits are random on top, which changes no code"""
    prev = FC.random_frame(1, H, W, fmt, seed)
    g = np.random.default_rng(seed + 1)
    top = 1 << FC.bits(fmt)
    codes = [np.array(c) for c in FC.codes(prev, fmt)]
    for c in codes:
        flat = c.reshape(-1)
        if kind == "all":
            flat[:] = (flat + 1 + g.integers(0, top - 1, flat.size)) % top
        elif kind == "few":
            idx = g.choice(flat.size, min(flat.size, 300), replace=False)
            flat[idx] = (flat[idx] + 1 + g.integers(0, top - 1, idx.size)) % top
    cur = FC.frame(*codes, fmt)
    if fmt == "p010":
        cur = tuple(p | g.integers(0, 64, p.shape).astype(np.uint16) for p in cur)
    return cur, prev


def changes_raw(cur, prev, fmt, up, H, W, O, first, n, nbytes=None, size=T):
    """pc_clips_tile_changes -> (status, the [n + 2, 3] buffer whose rows 1 .. n are `out`, poisoned beforehand, whether every partial
    of the workspace and no word after it was written -- or, for a refused call, none at all).  fmt and up: names, or raw ids for the
    calls that are to be refused."""
    from progressivecodec_amd import frames
    L = CL().lib()
    buf = torch.full((max(n, 0) + 2, 3), POISON64, dtype=torch.int64, device=DEV)
    need = L.pc_clips_changes_workspace_size(size, n)
    ws = torch.full((need // 8 + 1,), POISON64, dtype=torch.int64, device=DEV)
    a, b = frames._frame_struct(list(cur)), frames._frame_struct(list(prev))
    rc = L.pc_clips_tile_changes(C.byref(a), C.byref(b), frames.FORMATS.get(fmt, fmt), frames.UPSAMPLES.get(up, up), H, W, size, O, first, n,
                                 ws.data_ptr(), need if nbytes is None else nbytes, buf[1:].data_ptr(), stream())
    h = ws.cpu()
    return rc, buf, bool(h[-1] == POISON64 and ((h[:-1] != POISON64).all() if rc == 0 else (h == POISON64).all()))


@pytest.mark.parametrize("hw", SIZES)
def test_change_counts_exact_on_both_paths(hw):
    """every overlap x format x upsampling against the restatement, for frame pairs that differ in nothing, in a few hundred samples
    and in everything; the planes aligned, pitched and offset by one element, cur and prev pitched differently; sub-ranges and every
    tile alone; out and the workspace poisoned.  Wide exactly where pc_clips_plan's preconditions hold."""
    cl = CL()
    H, W = hw
    seen = set()
    for O in OVERLAPS:
        ny, nx = TC.grid(H, W, T, O)
        n = ny * nx
        ranges = [(0, n)] + ([(1, n - 1), (n // 2, 1)] if n > 1 else [])
        for k, fmt in enumerate(FC.FORMATS):
            for kind in ("few", "none", "all"):
                cur, prev = frame_pair(fmt, H, W, kind, seed=1000 * H + W + O + k)
                pairs = [(views(fmt, H, W, *pc, cur), views(fmt, H, W, *pp, prev)) for pc, pp in PAIRS]
                for up in FC.UPSAMPLES:
                    want = CC.tile_changes(cur, prev, fmt, T, O, up)
                    if kind == "none":
                        assert want == [[0, 0, 0]] * n
                    elif kind == "all":
                        fp = [CC.footprint(t // nx, t % nx, H, W, T, O, up) for t in range(n)]
                        assert want == [[(lu[1] - lu[0]) * (lu[3] - lu[2])] + [(ch[1] - ch[0]) * (ch[3] - ch[2])] * 2 for lu, ch in fp]
                    for p, (cv, pv) in enumerate(pairs):
                        expect = p == 0 and O % 8 == 0
                        wide = cl.plan(cl.CHANGES, cv, fmt, other=pv, overlap=O)
                        assert wide is expect, (H, W, O, fmt, p)
                        seen.add(wide)
                        for first, m in ranges if kind == "few" else ranges[:1]:
                            case = (H, W, O, fmt, kind, up, p, first, m)
                            rc, buf, ws_ok = changes_raw(cv, pv, fmt, up, H, W, O, first, m)
                            assert rc == 0 and ws_ok, case
                            check_out(buf, want[first:first + m], case)
                    if kind == "few" and up == "linear":
                        for t in range(n):                                 # every tile alone, on either path
                            for cv, pv in pairs[::2]:
                                rc, buf, ws_ok = changes_raw(cv, pv, fmt, up, H, W, O, t, 1)
                                assert rc == 0 and ws_ok
                                check_out(buf, want[t:t + 1], (H, W, O, fmt, t))
                    if kind == "few":
                        # the Python calls: unbatched planes, a plane whose innermost stride is not 1 (copied), a sub-range on a
                        # second stream, and the clip call on a list and on batched planes
                        pl = lambda f: tuple(torch.from_numpy(p[0]).to(DEV) for p in f)                            # noqa: E731
                        got = cl.tile_changes(tuple(v[0] for v in pairs[1][0]), pl(prev), fmt, T, O, up)
                        assert got.dtype == torch.int64 and got.shape == (n, 3) and got.device.type == "cuda" and got.tolist() == want
                        wider = torch.from_numpy(np.repeat(cur[0][0], 2, axis=1)).to(DEV)[:, ::2]
                        assert cl.tile_changes((wider,) + pl(cur)[1:], pl(prev), fmt, T, O, up).tolist() == want
                        side = torch.cuda.Stream(DEV)
                        side.wait_stream(torch.cuda.current_stream(DEV))
                        with torch.cuda.stream(side):
                            got_s = cl.tile_changes(pl(cur), pl(prev), fmt, T, O, up, first_tile=n - 1)
                        side.synchronize()
                        assert got_s.tolist() == want[n - 1:]
                        back = CC.tile_changes(prev, cur, fmt, T, O, up)
                        assert back == want
                        clip = cl.clip_changes([pl(prev), pl(cur), pl(cur), pl(prev)], fmt, T, O, up)
                        assert clip.shape == (3, n, 3) and clip.tolist() == [want, [[0, 0, 0]] * n, back]
                        batched = tuple(torch.stack([a, b, b, a]) for a, b in zip(pl(prev), pl(cur)))
                        assert torch.equal(cl.clip_changes(batched, fmt, T, O, up), clip)
                        assert cl.clip_changes([pl(cur)], fmt, T, O, up).shape == (0, n, 3)
                        if n > 1:
                            assert cl.clip_changes(batched, fmt, T, O, up, first_tile=1, n_tiles=n - 1).tolist() == [r[1:] for r in clip.tolist()]
    assert seen == {True, False}


def test_refused_change_calls_launch_nothing():
    cl = CL()
    L = cl.lib()
    H, W, O = 100, 150, 16
    for fmt in ("nv12", "p010"):
        cur, prev = frame_pair(fmt, H, W, "few", seed=3)
        cv, pv = views(fmt, H, W, "pad4", 0, cur), views(fmt, H, W, "loose", 0, prev)
        ok = dict(fmt=fmt, up="linear", H=H, W=W, O=O, first=0, n=6)
        for kw in [dict(first=1), dict(first=-1), dict(O=6), dict(nbytes=L.pc_clips_changes_workspace_size(T, 6) - 1), dict(fmt=3), dict(fmt=-1),
                   dict(up=2), dict(up=-1), dict(H=0), dict(n=7)]:
            rc, buf, ws_ok = changes_raw(cv, pv, **dict(ok, **kw))
            torch.cuda.synchronize()
            assert rc == -1 and (buf == POISON64).all() and ws_ok, (fmt, kw)
        rc, buf, ws_ok = changes_raw(cv, pv, **ok)                                         # unspoilt, it goes through
        assert rc == 0 and ws_ok and (buf[1:-1] != POISON64).all() and (buf[0] == POISON64).all() and (buf[-1] == POISON64).all()
    with pytest.raises(cl.ClipsError, match="PC_ERR_ARG"):
        raise cl.ClipsError(-1, "pc_clips_tile_changes")


# -- the cut of a list ---------------------------------------------------------------------------------------------------------------

NAN_BITS = 0x7FC00ABC


def float_buffer(n_floats, offset):
    """a NaN-patterned float32 buffer and the contiguous view of n_floats floats `offset` floats past its (256-byte aligned) start"""
    buf = torch.full((offset + n_floats + 8,), NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    return buf, buf[offset:offset + n_floats]


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("hw", SIZES)
def test_cut_of_a_list_is_the_cut_of_each_rectangle_bit_for_bit(hw):
    """every tile in order, a permuted list with repeats, against frame_tiles.cut_frame and the restatement; source planes aligned,
    pitched and offset, the destination 16-byte aligned and one float past it; out= into a slice of a larger buffer"""
    from progressivecodec_amd import frame_tiles, frames
    cl = CL()
    L = cl.lib()
    H, W = hw
    seen = set()
    for O in OVERLAPS:
        ny, nx = TC.grid(H, W, T, O)
        n = ny * nx
        g = np.random.default_rng(H * W + O)
        order = [int(v) for v in g.permutation(n)] + [int(v) for v in g.integers(0, n, 3)]
        for k, fmt in enumerate(FC.FORMATS):
            f = FC.random_frame(1, H, W, fmt, seed=7 * H + W + O + k)
            planes = tuple(torch.from_numpy(p[0]).to(DEV) for p in f)
            for up in FC.UPSAMPLES:
                matrix, rng = MATS[(k + O // 4 + (up == "linear")) % 3], FC.RANGES[(k + O // 4) % 2]
                want_np = GC.cut(f, fmt, matrix, rng, up, T, O)
                want = torch.from_numpy(want_np).to(DEV)
                whole, _ = frame_tiles.cut_frame(planes, fmt, matrix, rng, up, T, O)
                assert torch.equal(bits(whole), bits(want))
                one, _ = frame_tiles.cut_frame(planes, fmt, matrix, rng, up, T, O, rect=(order[0] // nx, order[0] % nx, 1, 1))
                coef = frames.coefficients(matrix)
                for (mode, off), foff in [(("pad4", 0), 0), (("loose", 0), 0), (("pad4", 1), 0), (("pad4", 0), 1)]:
                    src = views(fmt, H, W, mode, off, f)
                    for idx in (list(range(n)), order):
                        m = len(idx)
                        store, dst = float_buffer(m * 3 * T * T, 4 + foff)
                        dst = dst.view(m, 3, T, T)
                        expect = (mode, off, foff) == ("pad4", 0, 0) and O % 8 == 0
                        wide = cl.plan(cl.CUT, src, fmt, f32=dst, overlap=O)
                        assert wide is expect, (H, W, O, fmt, mode, off, foff)
                        seen.add(wide)
                        got = cl.cut_tiles(tuple(v[0] for v in src), fmt, idx, matrix, rng, up, T, O, out=dst)
                        assert got is dst
                        case = (H, W, O, fmt, up, mode, off, foff, m)
                        assert torch.equal(bits(dst), bits(want[idx])), case
                        assert torch.equal(bits(dst[0]), bits(one[0])) or idx is not order, case
                        h = store.view(torch.int32)
                        assert (h[:4 + foff] == NAN_BITS).all() and (h[4 + foff + dst.numel():] == NAN_BITS).all(), case
                # without out=, and an index list as a tensor
                got = cl.cut_tiles(planes, fmt, torch.tensor(order), matrix, rng, up, T, O)
                assert got.shape == (len(order), 3, T, T) and got.dtype == torch.float32 and torch.equal(bits(got), bits(want[order]))
                # an index outside the grid, written straight through the C call: a tile of +0.0f and no access outside the frame
                raw = [order[0], n, -1, 2 ** 31 - 1, -2 ** 31, order[-1]]
                didx = torch.tensor(raw, dtype=torch.int32, device=DEV)
                for mode, foff in (("pad4", 0), ("loose", 1)):
                    held = views(fmt, H, W, mode, 0, f)
                    src = frames._frame_struct(held)
                    store, dst = float_buffer(len(raw) * 3 * T * T, 4 + foff)
                    rc = L.pc_clips_cut_list(C.byref(src), frames.FORMATS[fmt], frames.RANGES[rng], frames.UPSAMPLES[up], coef.a, coef.b, coef.c,
                                             coef.d, H, W, T, O, didx.data_ptr(), len(raw), dst.data_ptr(), stream())
                    assert rc == 0
                    d = bits(dst.view(len(raw), 3, T, T))
                    assert torch.equal(d[0], bits(want[raw[0]])) and torch.equal(d[5], bits(want[raw[5]])) and (d[1:5] == 0).all()
                    h = store.view(torch.int32)
                    assert (h[:4 + foff] == NAN_BITS).all() and (h[4 + foff + dst.numel():] == NAN_BITS).all()
                    del held
    assert seen == {True, False}


def test_refused_cut_calls_launch_nothing():
    from progressivecodec_amd import frames
    cl = CL()
    L = cl.lib()
    H, W, O = 100, 150, 16
    f = FC.random_frame(1, H, W, "nv12", seed=2)
    held = views("nv12", H, W, "pad4", 0, f)
    src = frames._frame_struct(held)
    k = frames.coefficients("bt709")
    didx = torch.tensor([0, 5], dtype=torch.int32, device=DEV)
    store, dst = float_buffer(2 * 3 * T * T, 4)
    ok = dict(fmt=0, range=0, up=1, a=k.a, b=k.b, c=k.c, d=k.d, H=H, W=W, T=T, O=O, tiles=didx.data_ptr(), n=2, dst=dst.data_ptr())
    for kw in [dict(fmt=3), dict(range=2), dict(up=2), dict(T=96), dict(O=6), dict(n=0), dict(n=-1), dict(tiles=None), dict(dst=None), dict(H=0)]:
        assert L.pc_clips_cut_list(C.byref(src), *dict(ok, **kw).values(), stream()) == -1, kw
    torch.cuda.synchronize()
    assert (store.view(torch.int32) == NAN_BITS).all()
    assert L.pc_clips_cut_list(C.byref(src), *ok.values(), stream()) == 0
    torch.cuda.synchronize()
    assert (bits(dst) != NAN_BITS).all()
    del held
    with pytest.raises(ValueError, match="tile index 6"):
        cl.cut_tiles(tuple(torch.from_numpy(p[0]).to(DEV) for p in f), "nv12", [0, 6], tile=T, overlap=O)


# -- through the codec ---------------------------------------------------------------------------------------------------------------

QUALITIES = [0, 0.5]
H0, W0, O0 = 100, 150, 16                                                  # 2 x 3 tiles of 64 x 64, S = 48


@functools.lru_cache(maxsize=None)
def clip_of(fmt):
    """frame 0: a smooth frame; frame 1: luma sample (10, 10) changed; frame 2: frame 1; frame 3: the Cb sample at chroma (23, 40)
    changed -- the halo row of tile (1, 1); P010: a fifth frame that differs from frame 3 in the low six bits only"""
    sh = 6 if fmt == "p010" else 0
    f0 = tuple(np.array(p) for p in codec_frame(fmt))
    f1 = tuple(np.array(p) for p in f0)
    f1[0][0, 10, 10] ^= 0x80 << sh
    f2 = tuple(np.array(p) for p in f1)
    f3 = tuple(np.array(p) for p in f2)
    f3[1][0, 23, 40, 0] ^= 0x80 << sh
    out = [f0, f1, f2, f3]
    if fmt == "p010":
        g = np.random.default_rng(4)
        out.append(tuple(p | g.integers(0, 64, p.shape).astype(np.uint16) for p in f3))
    return out


@pytest.mark.parametrize("fmt", ["nv12", "p010"])
@pytest.mark.parametrize("up", ["linear", "nearest"])
def test_encode_clip_and_decode_clip_are_the_per_frame_calls(up, fmt):
    from progressivecodec_amd import frame_tiles, tiles
    cl = CL()
    net = gpu_codec()
    clip = clip_of(fmt)
    F = len(clip)
    frames = [tuple(torch.from_numpy(p[0]).to(DEV) for p in f) for f in clip]
    kw = dict(tile=T, overlap=O0, upsample=up, mask_pol=POL)
    # only tile (0, 0) is recoded for frame 1 and nothing for frame 2; for frame 3 tile (0, 1) and, through its halo row alone and
    # under linear upsampling only, tile (1, 1); low bits recode nothing
    f3 = [1, 3, 0, 0, 3 if up == "linear" else 0, 0]
    source = [[0] * 6, [1, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], f3] + ([f3] if F == 5 else [])
    assert CC.source_table(clip, fmt, T, O0, up) == source
    buf, plan = cl.encode_clip(net, frames, QUALITIES, fmt, **kw)
    assert isinstance(buf, bytes) and plan.source == source and plan.container_bytes == len(buf)
    n_coded = sum(s == f for f, row in enumerate(source) for s in row)
    assert (plan.n_coded, plan.n_reused) == (n_coded, 6 * F - n_coded) and n_coded == (9 if up == "linear" else 8)
    every, plan_all = cl.encode_clip(net, frames, QUALITIES, fmt, reuse=False, **kw)
    assert plan_all.source == [[f] * 6 for f in range(F)] and (plan_all.n_coded, plan_all.n_reused) == (6 * F, 0) and len(every) == plan_all.container_bytes
    # 1. every frame's container is encode_frame_tiled's, byte for byte, with and without reuse
    alone = [frame_tiles.encode_frame_tiled(net, f, QUALITIES, fmt, **kw) for f in frames]
    for k in range(F):
        assert cl.frame_container(buf, k) == alone[k] == cl.frame_container(every, k), k
    # 4. the container is the layout's: 42 bytes, the table, the coded tiles' blobs -- the restatement's bytes from the per-frame blobs
    blobs = []
    for b in alone:
        hd = frame_tiles.parse_frame_tiled(b)
        blobs.append([tiles.tile_bytes(hd["inner"], hd["tiled"], t)[0] for t in range(6)])
    contract = cl.parse_clip(buf)["contract"]
    assert buf == CC.pack_clip(blobs, source, H0, W0, T, O0, fmt, "bt709", "limited", up, contract)
    assert len(buf) == CC.container_bytes(blobs, source) == 42 + 16 * 6 * F + sum(len(blobs[f][t]) for f in range(F) for t in range(6) if source[f][t] == f)
    assert every == CC.pack_clip(blobs, plan_all.source, H0, W0, T, O0, fmt, "bt709", "limited", up, contract)
    assert len(every) == 42 + 16 * 6 * F + sum(len(b) for row in blobs for b in row)
    # the bytes depend neither on max_tiles_per_call nor on how the frames lie in memory
    for per_call in (1, 4):
        assert cl.encode_clip(net, frames, QUALITIES, fmt, max_tiles_per_call=per_call, **kw) == (buf, plan), per_call
    batched = tuple(torch.stack(ps) for ps in zip(*frames))
    assert cl.encode_clip(net, batched, QUALITIES, fmt, **kw) == (buf, plan)
    pitched = [tuple(v[0] for v in views(fmt, H0, W0, "loose", 1, f)) for f in clip]
    assert cl.encode_clip(net, pitched, QUALITIES, fmt, **kw) == (buf, plan)
    # 2. every frame decodes to decode_frame_tiled of its own container: every level, a region, another format
    other = "nv12" if fmt == "p010" else "p010"
    same = lambda a, b: len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))                           # noqa: E731
    for dkw in [dict(level=0), dict(), dict(region=(40, 40, 30, 50)), dict(level=0, region=(60, 60, 8, 8), fmt=other)]:
        want = [frame_tiles.decode_frame_tiled(net, alone[k], **dkw) for k in range(F)]
        got = cl.decode_clip(net, buf, **dkw)
        assert len(got) == F and all(same(g, w) for g, w in zip(got, want)), dkw
        if not dkw:
            assert all(same(g, w) for g, w in zip(cl.decode_clip(net, every), want))
            assert all(same(g, w) for g, w in zip(cl.decode_clip(net, buf, max_tiles_per_call=4), want))
            part = cl.decode_clip(net, buf, frames=[3, 1, 1], max_tiles_per_call=1)
            assert len(part) == 3 and same(part[0], want[3]) and same(part[1], want[1]) and same(part[2], want[1])
            assert same(want[1], want[2]) and (F == 4 or same(want[3], want[4]))

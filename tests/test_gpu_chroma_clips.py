"""Clips of YUV frames of any subsampling and siting on the GPU (progressivecodec_amd/chroma_clips.py, libpc_chroma_clips.so) against
their restatement (tests/chroma_clips_contract.py): the change counts over every tile's footprint, the cut of a list of tiles against
chroma_tiles.cut_frame, both on both access paths, and encode_clip / decode_clip through the codec against the per-frame
encode_frame_tiled / decode_frame_tiled.  Every comparison is exact equality of integers, bits or bytes.  T = 64 throughout.  The
matrix is tests/chroma_clips_cases.py's table; every case asserts the access path the table predicts."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import chroma_clips_cases as CS
from tests import chroma_clips_contract as CK
from tests import chroma_contract as CC
from tests import clips_contract as SC
from tests import frames_contract as FC
from tests import tiles_contract as TC
from tests.test_gpu_chroma_tiles import codec_frame, on_device
from tests.test_gpu_frames import POISON64, View, poison_of, up4
from tests.test_gpu_rate import check_out
from tests.util import gpu_codec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POL = "point-based-std"
T = CS.T
NAN_BITS = 0x7FC00ABC


def KC():
    from progressivecodec_amd import chroma_clips
    return chroma_clips


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def plane_shapes(fmt, H, W):
    Hc, Wc = CC.chroma_size(H, W, fmt)
    return [(1, H, W), (1, Hc, Wc, 2)] if CC.FORMATS[fmt][0] else [(1, H, W), (1, Hc, Wc), (1, Hc, Wc)]


def views(fmt, H, W, mode, offset, data):
    """the planes of a frame as cuda views `offset` elements past an allocation start; tests.test_gpu_frames.View's modes, and
    "wider": aligned rows eight elements (and a multiple of 4) longer than "pad4" would make them"""
    dt = np.uint16 if CC.bits(fmt) == 10 else np.uint8
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


#: (cur, prev) per entry of CS.ALIGNMENTS: both aligned with row strides that are multiples of 4, but different ones; cur one element
#: past an allocation start with a loose row stride next to an aligned prev.  The two frames of a pair never share a pitch.
PAIR = {True: (("pad4", 0), ("wider", 0)), False: (("loose", 1), ("pad4", 0))}


def other_bits(planes, fmt, g):
    """the frame with the bits of its 16-bit words outside the code randomised; an 8-bit frame has none"""
    _, n, sh = CC.FORMATS[fmt][:3]
    if n != 10:
        return planes
    keep = np.uint16((2 ** n - 1) << sh)
    return tuple((p & keep) | (g.integers(0, 2 ** 16, p.shape).astype(np.uint16) & ~keep) for p in planes)


@functools.lru_cache(maxsize=None)
def frame_pair(fmt, H, W, kind, seed):
    """(cur, prev): prev random over the whole code range; cur differs from it in a few hundred random samples of every plane ("few"),
    in every sample ("all") or in no code ("outside"); for the 10-bit formats cur's bits outside the codes are random on top, which
    changes no code"""
    prev = CC.random_frame(1, H, W, fmt, seed)
    g = np.random.default_rng(seed + 1)
    top = 1 << CC.bits(fmt)
    codes = [np.array(c) for c in CC.codes(prev, fmt)]
    for c in codes:
        flat = c.reshape(-1)
        if kind == "all":
            flat[:] = (flat + 1 + g.integers(0, top - 1, flat.size)) % top
        elif kind == "few":
            idx = g.choice(flat.size, min(flat.size, 300), replace=False)
            flat[idx] = (flat[idx] + 1 + g.integers(0, top - 1, idx.size)) % top
    return other_bits(CC.frame(*codes, fmt), fmt, g), prev


def kinds_of(fmt):
    return ("few", "all") + (("outside",) if CC.bits(fmt) == 10 else ())


@functools.lru_cache(maxsize=None)
def pair_views(fmt, H, W, kind, seed, aligned):
    cur, prev = frame_pair(fmt, H, W, kind, seed)
    (cm, co), (pm, po) = PAIR[aligned]
    return views(fmt, H, W, cm, co, cur), views(fmt, H, W, pm, po, prev)


def changes_raw(cur, prev, fmt, siting, up, H, W, O, first, n, nbytes=None, size=T, **raw):
    """pc_chroma_clips_tile_changes -> (status, the [n + 2, 3] buffer whose rows 1 .. n are `out`, poisoned beforehand, whether every
    partial of the workspace and no word after it was written -- or, for a refused call, none at all).  raw: format, siting or
    upsampling integers that replace the names', and null pointers, for the calls that are to be refused."""
    from progressivecodec_amd import chroma, frames
    L = KC().lib()
    f = dict(chroma.FORMATS[fmt]._asdict(), hsite=chroma.SITINGS[siting][0], vsite=chroma.SITINGS[siting][1], up=frames.UPSAMPLES.get(up, up))
    f.update({k: v for k, v in raw.items() if k in f})
    buf = torch.full((max(n, 0) + 2, 3), POISON64, dtype=torch.int64, device=DEV)
    # the workspace of the tile size the call is made with; of the module's where the library has none for it (a call to be refused)
    need = (L.pc_chroma_clips_changes_workspace_size(size, chroma.FORMATS[fmt].sy, max(n, 1))
            or L.pc_chroma_clips_changes_workspace_size(T, chroma.FORMATS[fmt].sy, max(n, 1)))
    ws =torch.full((need // 8 + 1,), POISON64, dtype=torch.int64, device=DEV)
    a, b = frames._frame_struct(list(cur)), frames._frame_struct(list(prev))
    rc = L.pc_chroma_clips_tile_changes(C.byref(a) if not raw.get("no_cur") else None, C.byref(b) if not raw.get("no_prev") else None, *f.values(),
                                        H, W, size, O, first, n, ws.data_ptr() if not raw.get("no_ws") else None,
                                        need if nbytes is None else nbytes, buf[1:].data_ptr() if not raw.get("no_out") else None, stream())
    torch.cuda.synchronize()
    h = ws.cpu()
    return rc, buf, bool(h[-1] == POISON64 and ((h[:-1] != POISON64).all() if rc == 0 else (h == POISON64).all()))


def float_buffer(n_floats, offset):
    """a NaN-patterned float32 buffer and the contiguous view of n_floats floats `offset` floats past its (256-byte aligned) start"""
    buf = torch.full((offset + n_floats + 8,), NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    return buf, buf[offset:offset + n_floats]


def bits(t):
    return t.contiguous().view(torch.int32)


def guards_kept(store, offset, numel):
    h = store.view(torch.int32)
    return bool((h[:offset] == NAN_BITS).all() and (h[offset + numel:] == NAN_BITS).all())


# -- the change counts ---------------------------------------------------------------------------------------------------------------

def run_changes(cases):
    kc = KC()
    seen = set()
    for c in cases:
        ny, nx = TC.grid(c.H, c.W, T, c.O)
        n = ny * nx
        ranges = [(0, n)] + ([(1, n - 1), (n // 2, 1)] if n > 1 else [])
        seed = 1000 * c.H + c.W
        for kind in kinds_of(c.fmt):
            cur, prev = frame_pair(c.fmt, c.H, c.W, kind, seed)
            want = CK.tile_changes(cur, prev, c.fmt, c.siting, T, c.O, c.upsample)
            if kind == "outside":
                assert want == [[0, 0, 0]] * n and any((a != b).any() for a, b in zip(cur, prev))
            elif kind == "all":
                assert want == CK.footprint_sizes(c.H, c.W, T, c.O, c.fmt, c.siting, c.upsample)
            for aligned in CS.ALIGNMENTS:
                cv, pv = pair_views(c.fmt, c.H, c.W, kind, seed, aligned)
                wide = kc.plan(kc.CHANGES, cv, c.fmt, other=pv, overlap=c.O)
                assert wide is CS.wide(c, aligned), (c, aligned)
                seen.add(CS.kernel_tuple(c.fmt, wide))
                for first, m in ranges if kind == "few" else ranges[:1]:
                    rc, buf, ws_ok = changes_raw(cv, pv, c.fmt, c.siting, c.upsample, c.H, c.W, c.O, first, m)
                    assert rc == 0 and ws_ok, (c, kind, aligned, first, m)
                    check_out(buf, want[first:first + m], (c, kind, aligned, first, m))
                if kind == "few":
                    for t in range(n):                             # every tile alone
                        rc, buf, ws_ok = changes_raw(cv, pv, c.fmt, c.siting, c.upsample, c.H, c.W, c.O, t, 1)
                        assert rc == 0 and ws_ok
                        check_out(buf, want[t:t + 1], (c, aligned, t))
            if kind == "few":                                      # the Python call, on unbatched planes
                got = kc.tile_changes(on_device(cur), on_device(prev), c.fmt, c.siting, T, c.O, c.upsample)
                assert got.dtype == torch.int64 and got.shape == (n, 3) and got.device.type == "cuda" and got.tolist() == want, c
    return seen


@pytest.mark.parametrize("fmt", sorted(CC.FORMATS))
def test_change_counts_of_every_format_siting_and_upsampling(fmt):
    """100 x 150 with O in {0, 4}: frame pairs that differ in a few hundred samples, in everything (the counts are the footprint's
    sizes) and, at 10 bits, outside their codes alone (all counts zero); aligned views and views offset by one element, the two
    frames pitched differently; the whole grid, sub-ranges and every tile alone; out and the workspace poisoned"""
    cases = CS.main_cases(fmt)
    assert run_changes(cases) == CS.reached(cases) == {CS.kernel_tuple(fmt, False), CS.kernel_tuple(fmt, True)}


@pytest.mark.parametrize("fmt", CS.OTHER_FORMATS)
def test_change_counts_at_the_other_sizes_and_overlaps(fmt):
    cases = CS.other_cases(fmt)
    assert run_changes(cases) == CS.reached(cases)


def one_sample_pair(fmt, H, W, plane, where):
    """a smooth frame and the same frame with one sample changed"""
    prev = codec_frame(H, W, fmt, "centre")
    codes = [np.array(c) for c in CC.codes(prev, fmt)]
    codes[plane][0][where] ^= 1 << (CC.bits(fmt) - 1)
    return CC.frame(*codes, fmt), prev


def test_the_halo_rule_on_the_device():
    """one Cb sample changed.  p210 at chroma column 23 (luma row 10): tile column 1 starts at chroma column 24 and reads column 23
    under "centre" alone.  nv12 at chroma (23, 40): tile (1, 1) starts at chroma row 24 and reads row 23 under "centre" / linear
    alone.  The restatement's table is the authority, and gives exactly this."""
    kc = KC()
    H, W, O = 100, 150, 16
    tiles_counted = lambda counts: [t for t, c in enumerate(counts) if c != [0, 0, 0]]                                 # noqa: E731
    cur, prev = one_sample_pair("p210", H, W, 1, (10, 23))
    for siting, up, want in [("centre", "linear", [0, 1]), ("left", "linear", [0]), ("topleft", "linear", [0]), ("centre", "nearest", [0])]:
        table = CK.tile_changes(cur, prev, "p210", siting, T, O, up)
        assert tiles_counted(table) == want and all(table[t] == [0, 1, 0] for t in want)
        assert kc.tile_changes(on_device(cur), on_device(prev), "p210", siting, T, O, up).tolist() == table, (siting, up)
    cur, prev = one_sample_pair("nv12", H, W, 1, (23, 40))
    for siting, up, want in [("centre", "linear", [1, 4]), ("topleft", "linear", [1]), ("left", "linear", [1, 4]), ("centre", "nearest", [1]),
                             ("topleft", "nearest", [1])]:
        table = CK.tile_changes(cur, prev, "nv12", siting, T, O, up)
        assert tiles_counted(table) == want and all(table[t] == [0, 1, 0] for t in want)
        for aligned in CS.ALIGNMENTS:
            (cm, co), (pm, po) = PAIR[aligned]
            rc, buf, ws_ok = changes_raw(views("nv12", H, W, cm, co, cur), views("nv12", H, W, pm, po, prev), "nv12", siting, up, H, W, O, 0, 6)
            assert rc == 0 and ws_ok
            check_out(buf, table, (siting, up, aligned))


@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_centre_sited_420_is_clips_on_the_device(fmt):
    from progressivecodec_amd import clips
    kc = KC()
    H, W = 100, 150
    cur, prev = frame_pair(fmt, H, W, "few", 77)
    a, b = on_device(cur), on_device(prev)
    for O, up in itertools.product((0, 4, 16), CC.UPSAMPLES):
        ours = kc.tile_changes(a, b, fmt, "centre", T, O, up)
        assert torch.equal(ours, clips.tile_changes(a, b, fmt, T, O, up)) and ours.tolist() == SC.tile_changes(cur, prev, fmt, T, O, up)
        n = ours.shape[0]
        idx = list(range(n - 1, -1, -1)) + [0, n - 1]
        x = kc.cut_tiles(a, fmt, idx, "bt601", "full", up, "centre", T, O)
        assert torch.equal(bits(x), bits(clips.cut_tiles(a, fmt, idx, "bt601", "full", up, T, O))), (fmt, O, up)


def test_refused_change_calls_launch_nothing():
    kc = KC()
    L = kc.lib()
    H, W, O = 100, 150, 16
    for fmt, siting in (("nv16", "left"), ("p010", "topleft"), ("i444", "centre")):
        from progressivecodec_amd import chroma
        cur, prev = frame_pair(fmt, H, W, "few", 3)
        cv, pv = views(fmt, H, W, "pad4", 0, cur), views(fmt, H, W, "loose", 0, prev)
        ok = dict(fmt=fmt, siting=siting, up="linear", H=H, W=W, O=O, first=0, n=6)
        need = L.pc_chroma_clips_changes_workspace_size(T, chroma.FORMATS[fmt].sy, 6)
        for kw in [dict(size=96), dict(size=32), dict(size=4096, O=0), dict(O=6), dict(O=36), dict(O=-4), dict(nbytes=need - 1), dict(nbytes=0),
                   dict(layout=2), dict(bits=9), dict(shift=3), dict(sx=3), dict(sy=0), dict(hsite=2), dict(vsite=-1), dict(up=2), dict(up=-1),
                   dict(no_cur=1), dict(no_prev=1), dict(no_ws=1), dict(no_out=1), dict(first=1), dict(first=-1), dict(H=0), dict(n=7), dict(n=0)]:
            rc, buf, ws_ok = changes_raw(cv, pv, **dict(ok, **kw))
            assert rc == -1 and (buf == POISON64).all() and ws_ok, (fmt, kw)
        rc, buf, ws_ok = changes_raw(cv, pv, **ok)                                         # unspoilt, it goes through
        assert rc == 0 and ws_ok and (buf[1:-1] != POISON64).all() and (buf[0] == POISON64).all() and (buf[-1] == POISON64).all()
    with pytest.raises(kc.ChromaClipsError, match="PC_ERR_ARG"):
        raise kc.ChromaClipsError(-1, "pc_chroma_clips_tile_changes")


def test_clip_changes_is_the_tile_changes_of_each_pair():
    kc = KC()
    H, W, O = 100, 150, 16
    for fmt, siting, up in [("p210", "left", "linear"), ("nv12", "topleft", "linear"), ("i410", "centre", "nearest")]:
        cur, prev = frame_pair(fmt, H, W, "few", 11)
        other = frame_pair(fmt, H, W, "all", 11)[0]
        clip = [on_device(f) for f in (prev, cur, cur, other, prev)]
        each = [kc.tile_changes(clip[k + 1], clip[k], fmt, siting, T, O, up) for k in range(4)]
        assert [e.tolist() for e in each] == [CK.tile_changes(b, a, fmt, siting, T, O, up) for a, b in zip((prev, cur, cur, other), (cur, cur, other, prev))]
        got = kc.clip_changes(clip, fmt, siting, T, O, up)
        assert got.shape == (4, 6, 3) and got.dtype == torch.int64 and torch.equal(got, torch.stack(each)) and not got[1].any()
        batched = tuple(torch.stack(ps) for ps in zip(*clip))
        assert torch.equal(kc.clip_changes(batched, fmt, siting, T, O, up), got)
        assert torch.equal(kc.clip_changes(batched, fmt, siting, T, O, up, first_tile=1, n_tiles=4), got[:, 1:5])
        assert kc.clip_changes(clip[:1], fmt, siting, T, O, up).shape == (0, 6, 3)


# -- the cut of a list ---------------------------------------------------------------------------------------------------------------

def run_cuts(cases):
    from progressivecodec_amd import chroma, chroma_tiles, frames
    kc = KC()
    L = kc.lib()
    seen = set()
    for c in cases:
        ny, nx = TC.grid(c.H, c.W, T, c.O)
        n = ny * nx
        f = CC.random_frame(1, c.H, c.W, c.fmt, seed=7 * c.H + c.W + c.n, garbage=True)
        planes = on_device(f)
        want = torch.cat([chroma_tiles.cut_frame(planes, c.fmt, c.matrix, c.rng, c.upsample, c.siting, T, c.O, rect=(t // nx, t % nx, 1, 1))[0]
                          for t in range(n)])
        g = np.random.default_rng(c.H * c.W + c.n)
        lists = [[int(v) for v in g.permutation(n)] + [int(v) for v in g.integers(0, n, 3)], list(range(n - 1, -1, -1))]
        for aligned in CS.ALIGNMENTS:
            (mode, off), _ = PAIR[aligned]
            src = views(c.fmt, c.H, c.W, mode, off, f)
            foff = 4 if aligned else 5                             # floats past an allocation start: 16-byte aligned or not
            for idx in lists:
                m = len(idx)
                store, dst = float_buffer(m * 3 * T * T, foff)     # a slice of a larger buffer
                dst = dst.view(m, 3, T, T)
                wide = kc.plan(kc.CUT, src, c.fmt, f32=dst, overlap=c.O)
                assert wide is CS.wide(c, aligned), (c, aligned)
                seen.add(CS.kernel_tuple(c.fmt, wide))
                got = kc.cut_tiles(tuple(v[0] for v in src), c.fmt, idx, c.matrix, c.rng, c.upsample, c.siting, T, c.O, out=dst)
                assert got is dst and torch.equal(bits(dst), bits(want[idx])), (c, aligned, m)
                assert guards_kept(store, foff, dst.numel()), (c, aligned)
        if c.n % 4 == 0:
            # an index outside the grid, written straight through the C call: a tile of +0.0f, nothing else touched
            raw = [n - 1, n, -1, 2 ** 31 - 1, -2 ** 31, 0]
            didx = torch.tensor(raw, dtype=torch.int32, device=DEV)
            coef = frames.coefficients(c.matrix)
            for aligned in CS.ALIGNMENTS:
                (mode, off), _ = PAIR[aligned]
                held = views(c.fmt, c.H, c.W, mode, off, f)
                src = frames._frame_struct(held)
                foff = 4 if aligned else 5
                store, dst = float_buffer(len(raw) * 3 * T * T, foff)
                rc = L.pc_chroma_clips_cut_list(C.byref(src), *chroma.FORMATS[c.fmt], *chroma.SITINGS[c.siting], frames.RANGES[c.rng],
                                                frames.UPSAMPLES[c.upsample], coef.a, coef.b, coef.c, coef.d, c.H, c.W, T, c.O, didx.data_ptr(),
                                                len(raw), dst.data_ptr(), stream())
                torch.cuda.synchronize()
                assert rc == 0
                d = bits(dst.view(len(raw), 3, T, T))
                assert torch.equal(d[0], bits(want[n - 1])) and torch.equal(d[5], bits(want[0])) and (d[1:5] == 0).all(), (c, aligned)
                assert guards_kept(store, foff, dst.numel()), (c, aligned)
                del held
        got = kc.cut_tiles(planes, c.fmt, torch.tensor(lists[0]), c.matrix, c.rng, c.upsample, c.siting, T, c.O)      # without out=
        assert got.shape == (len(lists[0]), 3, T, T) and got.dtype == torch.float32 and torch.equal(bits(got), bits(want[lists[0]]))
    return seen


@pytest.mark.parametrize("fmt", sorted(CC.FORMATS))
def test_cut_of_a_list_is_the_cut_of_each_rectangle_bit_for_bit(fmt):
    """scattered lists with repeats and reversed lists against the single-rectangle cuts of chroma_tiles.cut_frame; source planes
    aligned, and pitched and offset; the destination a slice of a larger buffer, 16-byte aligned and one float past it"""
    cases = CS.main_cases(fmt)
    assert run_cuts(cases) == CS.reached(cases)


@pytest.mark.parametrize("fmt", CS.OTHER_FORMATS)
def test_cut_of_a_list_at_the_other_sizes_and_overlaps(fmt):
    cases = CS.other_cases(fmt)
    assert run_cuts(cases) == CS.reached(cases)


def test_refused_cut_calls_launch_nothing():
    from progressivecodec_amd import chroma, frames
    kc = KC()
    L = kc.lib()
    H, W, O = 100, 150, 16
    f = CC.random_frame(1, H, W, "p210", seed=2)
    held = views("p210", H, W, "pad4", 0, f)
    src = frames._frame_struct(held)
    k = frames.coefficients("bt709")
    didx = torch.tensor([0, 5], dtype=torch.int32, device=DEV)
    store, dst = float_buffer(2 * 3 * T * T, 4)
    ok = dict(chroma.FORMATS["p210"]._asdict(), hsite=1, vsite=0, range=0, up=1, a=k.a, b=k.b, c=k.c, d=k.d, H=H, W=W, T=T, O=O,
              tiles=didx.data_ptr(), n=2, dst=dst.data_ptr())
    for kw in [dict(layout=2), dict(bits=8), dict(shift=4), dict(sx=3), dict(sy=2, sx=1), dict(hsite=2), dict(vsite=2), dict(range=2), dict(up=2),
               dict(T=96), dict(T=4096, O=0), dict(O=6), dict(O=36), dict(n=0), dict(n=-1), dict(tiles=None), dict(dst=None), dict(H=0)]:
        assert L.pc_chroma_clips_cut_list(C.byref(src), *dict(ok, **kw).values(), stream()) == -1, kw
    assert L.pc_chroma_clips_cut_list(None, *ok.values(), stream()) == -1
    torch.cuda.synchronize()
    assert (store.view(torch.int32) == NAN_BITS).all()
    assert L.pc_chroma_clips_cut_list(C.byref(src), *ok.values(), stream()) == 0
    torch.cuda.synchronize()
    assert (bits(dst) != NAN_BITS).all() and guards_kept(store, 4, dst.numel())
    del held
    with pytest.raises(ValueError, match="tile index 6"):
        kc.cut_tiles(on_device(f), "p210", [0, 6], tile=T, overlap=O)


# -- through the codec ---------------------------------------------------------------------------------------------------------------

QUALITIES = [0, 0.5]
H0, W0, O0 = 100, 150, 16                                                  # 2 x 3 tiles of 64 x 64, S = 48
#: the stored format and siting -> another output format and siting
OTHER = {("p210", "left"): ("nv12", "left"), ("nv12", "topleft"): ("p210", "left"), ("i444", "centre"): ("nv12", "topleft")}


@functools.lru_cache(maxsize=None)
def clip_of(fmt, siting):
    """frame 0: a smooth frame; frame 1: luma sample (10, 10) changed; frame 2: frame 1; frame 3: the Cb sample at chroma (23, 40)
    changed, and for the 10-bit format the bits outside the codes on top"""
    half = 1 << (CC.bits(fmt) - 1)
    c0 = [np.array(c) for c in CC.codes(codec_frame(H0, W0, fmt, siting), fmt)]
    c1 = [np.array(c) for c in c0]
    c1[0][0, 10, 10] ^= half
    c3 = [np.array(c) for c in c1]
    c3[1][0, 23, 40] ^= half
    f0, f1, f3 = (CC.frame(*c, fmt) for c in (c0, c1, c3))
    return [f0, f1, tuple(np.array(p) for p in f1), other_bits(f3, fmt, np.random.default_rng(4))]


@pytest.mark.parametrize("fmt,siting", list(OTHER))
def test_encode_clip_and_decode_clip_are_the_per_frame_calls(fmt, siting):
    from progressivecodec_amd import chroma_tiles, tiles
    kc = KC()
    net = gpu_codec()
    clip = clip_of(fmt, siting)
    F = len(clip)
    frames = [on_device(f) for f in clip]
    kw = dict(siting=siting, tile=T, overlap=O0, mask_pol=POL)
    source = CK.source_table(clip, fmt, siting, T, O0, "linear")
    assert source[:3] == [[0] * 6, [1, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0]] and 3 in source[3] and 0 in source[3]
    buf, plan = kc.encode_clip(net, frames, QUALITIES, fmt, **kw)
    assert isinstance(buf, bytes) and plan.source == source and plan.container_bytes == len(buf)
    n_coded = sum(s == f for f, row in enumerate(source) for s in row)
    assert (plan.n_coded, plan.n_reused) == (n_coded, 6 * F - n_coded) and 7 < n_coded < 6 * F
    every, plan_all = kc.encode_clip(net, frames, QUALITIES, fmt, reuse=False, **kw)
    assert plan_all.source == [[f] * 6 for f in range(F)] and (plan_all.n_coded, plan_all.n_reused) == (6 * F, 0) and len(every) == plan_all.container_bytes
    # every frame's container is encode_frame_tiled's, byte for byte, with and without reuse
    alone = [chroma_tiles.encode_frame_tiled(net, f, QUALITIES, fmt, **kw) for f in frames]
    for k in range(F):
        assert kc.frame_container(buf, k) == alone[k] == kc.frame_container(every, k), k
    # the container is the layout's: the restatement's bytes from the per-frame blobs
    blobs = []
    for b in alone:
        hd = chroma_tiles.parse_frame_tiled(b)
        blobs.append([tiles.tile_bytes(hd["inner"], hd["tiled"], t)[0] for t in range(6)])
    contract = kc.parse_clip(buf)["contract"]
    assert buf == CK.pack_clip(blobs, source, H0, W0, T, O0, fmt, "bt709", "limited", "linear", siting, contract)
    assert every == CK.pack_clip(blobs, plan_all.source, H0, W0, T, O0, fmt, "bt709", "limited", "linear", siting, contract)
    assert len(every) == 47 + 16 * 6 * F + sum(len(b) for row in blobs for b in row) > len(buf)
    # the bytes depend neither on max_tiles_per_call nor on how the frames lie in memory
    for per_call in (1, 4, 32):
        assert kc.encode_clip(net, frames, QUALITIES, fmt, max_tiles_per_call=per_call, **kw) == (buf, plan), per_call
    batched = tuple(torch.stack(ps) for ps in zip(*frames))
    assert kc.encode_clip(net, batched, QUALITIES, fmt, **kw) == (buf, plan)
    pitched = [tuple(v[0] for v in views(fmt, H0, W0, "loose", 1, f)) for f in clip]
    assert kc.encode_clip(net, pitched, QUALITIES, fmt, **kw) == (buf, plan)
    # every frame decodes to decode_frame_tiled of its own container: every level, a region with a halo (under a co-sited axis column
    # 63 and row 63 are other tiles' than the region's first), another output format and siting
    ofmt, ositing = OTHER[(fmt, siting)]
    same = lambda a, b: len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))                           # noqa: E731
    for dkw in [dict(level=0), dict(), dict(region=(64, 64, 30, 40)), dict(level=0, region=(64, 64, 30, 40), fmt=ofmt, siting=ositing)]:
        want = [chroma_tiles.decode_frame_tiled(net, alone[k], **dkw) for k in range(F)]
        got = kc.decode_clip(net, buf, **dkw)
        assert len(got) == F and all(same(g, w) for g, w in zip(got, want)), dkw
        if not dkw:
            assert all(same(g, w) for g, w in zip(kc.decode_clip(net, every), want))
            part = kc.decode_clip(net, buf, frames=[3, 1, 1], max_tiles_per_call=1)
            assert len(part) == 3 and same(part[0], want[3]) and same(part[1], want[1]) and same(part[2], want[1])
            assert same(want[1], want[2])

"""Tiled coding of YUV 4:2:0 frames without a GPU: the properties DESIGN.md section 14 promises, on the restatement
(tests/frame_tiles_contract.py) alone; libpc_frame_tiles.so's C ABI up to the first device call; progressivecodec_amd.frame_tiles'
argument checks; and the PCG1 container up to the model."""
import ctypes as C
import functools
import itertools
import os
import re
import struct

import numpy as np
import pytest
import torch

from tests import frame_tiles_contract as GC
from tests import frames_contract as FC
from tests import image_shared
from tests import tiles_contract as TC
from tests.test_frames_host import fake_frame
from tests.test_tiles_host import blob, pct1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 64
SIZES = [(65, 63), (100, 150), (127, 129)]
OVERLAPS = [0, 4, 16, 32]
MATS = list(FC.MATRICES)


def _lib():
    from progressivecodec_amd import frame_tiles
    return frame_tiles, frame_tiles.lib()


# -- the contract's properties -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def hostile(H, W, O):
    ny, nx = TC.grid(H, W, T, O)
    x = TC.hostile_tiles(ny * nx, T, seed=H * 1000 + W + O)
    x.setflags(write=False)
    return x


def windows(H, W, seed):
    """the whole frame, the last odd (or last two) rows and columns, a 2 x 2 window, and seeded random admissible windows"""
    g = np.random.default_rng(seed)
    out = [(0, 0, H, W), (H - 1 - (H - 1) % 2, 0, H - (H - 1 - (H - 1) % 2), W), (0, W - 1 - (W - 1) % 2, H, W - (W - 1 - (W - 1) % 2)),
           (2 * (H // 4), 2 * (W // 4), 2, 2)]
    while len(out) < 9:
        y0, x0 = 2 * int(g.integers(0, H // 2)), 2 * int(g.integers(0, W // 2))
        h = H - y0 if g.integers(0, 3) == 0 else 2 * int(g.integers(1, (H - y0) // 2 + 1)) if H - y0 >= 2 else H - y0
        w = W - x0 if g.integers(0, 3) == 0 else 2 * int(g.integers(1, (W - x0) // 2 + 1)) if W - x0 >= 2 else W - x0
        out.append((y0, x0, h, w))
    assert all(GC.admissible(H, W, win) for win in out)
    return out


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("O", OVERLAPS)
def test_an_admissible_windows_stitch_is_the_crop_of_the_whole_frames(hw, O):
    from progressivecodec_amd import tiles
    H, W = hw
    x = hostile(H, W, O)
    grid = tiles.grid_of(H, W, T, O)
    n = 0
    for k, fmt in enumerate(FC.FORMATS):
        matrix, rng = MATS[(k + O // 4) % 3], FC.RANGES[(k + H) % 2]
        whole = GC.stitch_codes(x, H, W, T, O, fmt, matrix, rng)
        for win in windows(H, W, seed=H + W + O + k):
            got = GC.stitch_codes(x, H, W, T, O, fmt, matrix, rng, window=win)
            want = GC.crop_codes(whole, win)
            assert all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got, want)), (hw, O, fmt, win)
            # and the same from the smallest rectangle that covers the window
            ty0, tx0, nty, ntx = rect = grid.covering(win)
            sub = x[[(ty0 + a) * grid.nx + tx0 + b for a in range(nty) for b in range(ntx)]]
            got = GC.stitch_codes(sub, H, W, T, O, fmt, matrix, rng, rect=rect, window=win)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (hw, O, fmt, win, rect)
            n += 1
    assert n == 27


def test_the_rule_is_needed():
    """a window that starts on an odd row, or ends on an odd row inside the frame, has 2 x 2 cells that are not the frame's"""
    H, W, O = 100, 150, 16
    x = hostile(H, W, O)
    whole = GC.stitch_codes(x, H, W, T, O, "nv12", "bt709", "limited")
    for win in [(31, 20, 20, 40), (30, 20, 21, 40)]:
        assert not GC.admissible(H, W, win)
        with pytest.raises(ValueError, match="admissible"):
            GC.stitch_codes(x, H, W, T, O, "nv12", "bt709", "limited", window=win)
        got = GC.stitch_codes(x, H, W, T, O, "nv12", "bt709", "limited", window=win, check=False)
        want = GC.crop_codes(whole, win)
        assert np.array_equal(got[0], want[0])                                    # luma is per pixel: the crop
        assert got[1].shape != want[1].shape or not np.array_equal(got[1], want[1])
    # what the rule admits and what it refuses
    assert GC.admissible(5, 7, (4, 6, 1, 1)) and GC.admissible(5, 7, (0, 0, 5, 7)) and GC.admissible(6, 8, (2, 2, 2, 4))
    for bad in [(1, 0, 2, 2), (0, 1, 2, 2), (0, 0, 3, 2), (0, 0, 2, 3), (0, 0, 1, 1), (2, 2, 1, 2)]:
        assert not GC.admissible(6, 8, bad), bad


@pytest.mark.parametrize("fmt,matrix,rng,up", list(itertools.product(FC.FORMATS, FC.MATRICES, FC.RANGES, FC.UPSAMPLES)))
def test_gray_frames_return_every_nominal_luma_code_through_cut_and_stitch(fmt, matrix, rng, up):
    yo, ys, co, cs, mx = FC.levels(fmt, rng)
    lo, hi = (yo, yo + ys) if rng == "limited" else (0, mx)
    vals = np.arange(lo, hi + 1)
    H, W = 70, 91                                                                  # 2 x 2 tiles, an odd width: a clamped chroma column
    Y = np.resize(vals, (1, H, W))
    assert set(Y.ravel().tolist()) == set(vals.tolist())
    Hc, Wc = FC.chroma_size(H, W)
    f = FC.frame(Y, np.full((1, Hc, Wc), co), np.full((1, Hc, Wc), co), fmt)
    for O in (4, 32):
        tiles = GC.cut(f, fmt, matrix, rng, up, T, O)
        assert tiles.shape[0] == 4
        back = GC.stitch_codes(tiles, H, W, T, O, fmt, matrix, rng)
        assert (back[0] == Y).all() and (back[1] == co).all() and (back[2] == co).all(), O


@pytest.mark.parametrize("fmt,matrix,rng", list(itertools.product(FC.FORMATS, FC.MATRICES, FC.RANGES)))
def test_constant_cell_frames_round_trip_under_nearest_upsampling(fmt, matrix, rng):
    """frames of in-gamut RGB constant per 2 x 2 cell: nearest upsampling repeats each chroma sample over its cell, the 2 x 2 mean
    returns it, and the band weights of two tiles that agree sum to one within an ulp -- every code of all three planes comes back"""
    for (H, W), O in itertools.product([(100, 150), (65, 63)], [0, 4, 32]):
        g = np.random.default_rng(H + O)
        cells = g.uniform(0.2, 0.8, (1, 3, -(-H // 2), -(-W // 2)))
        x = np.repeat(np.repeat(cells, 2, axis=2), 2, axis=3)[:, :, :H, :W].astype(np.float32)
        f = FC.emit(x, 0, 0, H, W, fmt, matrix, rng)
        tiles = GC.cut(f, fmt, matrix, rng, "nearest", T, O)
        back = GC.stitch_codes(tiles, H, W, T, O, fmt, matrix, rng)
        for got, want in zip(back, FC.codes(f, fmt)):
            assert np.array_equal(got, want), (H, W, O)


def test_a_one_tile_frame_cuts_to_the_ingest():
    for (fmt, matrix, rng, up) in itertools.product(FC.FORMATS, ["bt601"], FC.RANGES, FC.UPSAMPLES):
        f = FC.random_frame(1, 64, 64, fmt, seed=4)
        got = GC.cut(f, fmt, matrix, rng, up, 64, 0)
        want = FC.ingest(f, fmt, matrix, rng, up, 64, 64, 0, 0)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # a tile is the crop of the whole frame's ingest: its chroma taps reach into the neighbouring tile
    f = FC.random_frame(1, 100, 150, "nv12", seed=5)
    whole = FC.rgb(f, "nv12", "bt709", "limited", "linear")[0]
    tiles = GC.cut(f, "nv12", "bt709", "limited", "linear", 64, 4, rect=(1, 1, 1, 2))
    assert np.array_equal(tiles[0, :, :40, :64].view(np.uint32), whole[:, 60:100, 60:124].view(np.uint32)) and (tiles[0, :, 40:] == 0).all()
    assert np.array_equal(tiles[1, :, :40, :30].view(np.uint32), whole[:, 60:100, 120:150].view(np.uint32)) and (tiles[1, :, :, 30:] == 0).all()


# -- the library, no device ----------------------------------------------------------------------------------------------------------

def test_library_exports_every_declared_function():
    ft, L = _lib()
    hdr = open(os.path.join(ROOT, "progressivecodec_amd", "frame_tiles_csrc", "pc_frame_tiles.h")).read()
    declared = re.findall(r"PC_API\s+[\w\s\*]+?\b(pc_\w+)\s*\(", hdr)
    assert len(declared) == 6 and sorted(declared) == sorted(ft.EXPORTS)
    for name in declared:
        getattr(L, name)
    assert L.pc_frame_tiles_strerror(-1).decode() and L.pc_frame_tiles_strerror(-6).decode() and L.pc_frame_tiles_last_hip_error() == 0
    # a library of its own: no other library of the project is linked, and the codec's source hash does not cover it
    import bench
    import inspect
    assert "frame_tiles" not in inspect.getsource(bench.source_hash)
    mk = image_shared.build_rule("frame_tiles")                                             # image_csrc/lib.mk, which the library's Makefile includes
    assert "-ffp-contract=off" in mk and not re.search(r"-lpc|libpc(odec|_pixels|_tiles|_rate|_metrics|_frames)\b", mk)
    top = open(os.path.join(ROOT, "progressivecodec_amd", "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\bframe_tiles\b", top, re.M) and re.search(r"^\.PHONY:.*\bframe_tiles\b", top, re.M)
    assert "$(MAKE) -C ../frame_tiles_csrc clean" in top
    # the frame is the one record of image_csrc/pc_yuv_frame.h, as pc_frames.h's is: frames.Frame serves both libraries
    image_shared.assert_frame_is_shared(hdr, "pc_ft_frame")


def test_workspace_size_is_the_documented_formula():
    _, L = _lib()
    for x0, h, w in [(0, 1, 1), (0, 64, 64), (2, 2, 2), (6, 3, 3), (6, 2, 2), (8, 127, 129), (14, 100, 131), (0, 1080, 1920), (0, 2160, 3840)]:
        items = -(-h // 2) * (-(-(x0 + w) // 8) - x0 // 8)
        assert L.pc_frame_tiles_stitch_workspace_size(x0, h, w) == 24 * -(-items // 256), (x0, h, w)
    for bad in [(-2, 4, 4), (0, 0, 4), (0, 4, 0), (0, -1, 4), (2 ** 31 - 2, 4, 4), (0, 2 ** 31 - 1, 2 ** 31 - 1)]:
        assert L.pc_frame_tiles_stitch_workspace_size(*bad) == 0, bad


def test_plan_is_host_only_and_each_precondition_is_broken_alone():
    """made-up pointer values: nothing may be dereferenced or launched (there is no GPU here)"""
    from progressivecodec_amd import frames
    ft, L = _lib()
    Fp = 0x7000_0100_0000
    H, W = 96, 160
    FS = (3 * T * T, T * T, T)

    def plan(op, fmt, fr, f32=Fp, fs=FS, O=0, x0=0, ref=None):
        wide = C.c_int(-1)
        rc = L.pc_frame_tiles_plan(op, frames.FORMATS[fmt], C.byref(fr) if fr is not None else None, f32, *fs, O, x0,
                                   C.byref(ref) if ref is not None else None, C.byref(wide))
        return rc, wide.value

    def shifted(fmt, back):
        """the window's frame whose column 8 * floor(x0 / 8) is aligned: every plane `back` luma columns into an aligned one"""
        es = 2 if fmt == "p010" else 1
        f = fake_frame(frames, fmt, H, W)
        f.y += back * es
        if fmt == "i420":
            f.u += back // 2
            f.v += back // 2
        else:
            f.u += back * es
        return f
    for fmt in FC.FORMATS:
        es = 2 if fmt == "p010" else 1
        ok = fake_frame(frames, fmt, H, W)
        for op in (ft.CUT, ft.STITCH):
            assert plan(op, fmt, ok) == (0, 1)
            for off in (4, 8, 12):
                assert plan(op, fmt, ok, f32=Fp + off) == (0, 0)                                # the floats: 16-byte aligned
            for k in range(3):
                fs = list(FS)
                fs[k] += 2
                assert plan(op, fmt, ok, fs=tuple(fs)) == (0, 0)                                # their strides: multiples of 4
            names = ["y", "u"] + (["v"] if fmt == "i420" else [])
            for nm in names:
                for off in (1, 2, 3):
                    bad = fake_frame(frames, fmt, H, W)
                    setattr(bad, nm, getattr(bad, nm) + off * es)                               # each plane: aligned to four elements
                    assert plan(op, fmt, bad) == (0, 0), (fmt, nm, off)
                bad = fake_frame(frames, fmt, H, W)
                setattr(bad, nm + "_row", getattr(bad, nm + "_row") + 2)                        # each row stride: a multiple of 4
                assert plan(op, fmt, bad) == (0, 0), (fmt, nm)
                free = fake_frame(frames, fmt, H, W)
                setattr(free, nm + "_batch", getattr(free, nm + "_batch") + 1)                  # one frame per call: no batch stride counts
                assert plan(op, fmt, free) == (0, 1), (fmt, nm)
        # the cut: O a multiple of 8 -- with O = 4 a tile's first chroma column is 2 mod 4 in the frame; the stitch does not care
        for O, wide in [(0, 1), (8, 1), (16, 1), (32, 1), (4, 0), (12, 0), (20, 0), (28, 0)]:
            assert plan(ft.CUT, fmt, ok, O=O) == (0, wide), (fmt, O)
            assert plan(ft.STITCH, fmt, ok, O=O) == (0, 1), (fmt, O)
        assert plan(ft.CUT, fmt, ok, x0=6) == (0, 1) and plan(ft.CUT, fmt, ok, x0=-3) == (0, 1)      # ignored by the cut
        # the stitch: items are aligned to 8 frame columns, so it is the address of column 8 * floor(x0 / 8) that counts
        for x0 in (0, 8, 16, 160):
            assert plan(ft.STITCH, fmt, ok, x0=x0) == (0, 1)
        for x0 in (2, 4, 6, 10, 12, 14):
            assert plan(ft.STITCH, fmt, ok, x0=x0) == (0, 1 if (fmt != "i420" and x0 % 4 == 0) else 0), (fmt, x0)
            assert plan(ft.STITCH, fmt, shifted(fmt, x0 % 8), x0=x0) == (0, 1), (fmt, x0)
            assert plan(ft.STITCH, fmt, shifted(fmt, x0 % 8), x0=x0, ref=ok) == (0, 1 if (fmt != "i420" and x0 % 4 == 0) else 0), (fmt, x0)
            assert plan(ft.STITCH, fmt, None, x0=x0, ref=shifted(fmt, x0 % 8)) == (0, 1), (fmt, x0)
        # the reference frame counts for the stitch alone; the destination may be absent there
        loose = fake_frame(frames, fmt, H, W, pad=2)
        assert plan(ft.STITCH, fmt, ok, ref=loose) == (0, 0) and plan(ft.CUT, fmt, ok, ref=loose) == (0, 1)
        assert plan(ft.STITCH, fmt, None, ref=ok) == (0, 1) and plan(ft.STITCH, fmt, None, ref=loose) == (0, 0)
        assert plan(ft.STITCH, fmt, None)[0] == -1 and plan(ft.CUT, fmt, None, ref=ok)[0] == -1
        assert plan(2, fmt, ok)[0] == -1 and plan(-1, fmt, ok)[0] == -1
        assert plan(ft.STITCH, fmt, ok, x0=-2)[0] == -1 and plan(ft.STITCH, fmt, ok, x0=3)[0] == -1 and plan(ft.CUT, fmt, ok, O=-4)[0] == -1
        assert plan(ft.STITCH, fmt, ok, f32=None)[0] == -1
        nul = fake_frame(frames, fmt, H, W)
        nul.u = None
        assert plan(ft.STITCH, fmt, nul)[0] == -1 and plan(ft.CUT, fmt, nul)[0] == -1
        assert L.pc_frame_tiles_plan(0, frames.FORMATS[fmt], C.byref(ok), Fp, 4, 4, 4, 0, 0, None, None) == -1
    wide = C.c_int(-1)
    assert L.pc_frame_tiles_plan(0, 3, C.byref(fake_frame(frames, "nv12", H, W)), Fp, 4, 4, 4, 0, 0, None, C.byref(wide)) == -1
    f = fake_frame(frames, "nv12", H, W)
    assert plan(ft.STITCH, "nv12", f) == (0, 1) and plan(ft.STITCH, "i420", f)[0] == -1      # an I420 frame needs its V pointer


def test_every_argument_error_returns_before_the_device():
    """fake device pointers: every call below must return PC_ERR_ARG without touching them (no GPU here)"""
    from progressivecodec_amd import frames
    ft, L = _lib()
    Fp, Wk, S = 0x7000_0100_0000, 0x7000_0200_0000, 0x7000_0300_0000
    H, W, O = 100, 150, 16                                                        # 2 x 3 tiles, S = 48
    k = frames.coefficients("bt709")
    for fmt in FC.FORMATS:
        fid = frames.FORMATS[fmt]
        fr = lambda h=H, w=W, **kw: fake_frame(frames, fmt, h, w, **kw)                          # noqa: E731

        def broken(field, value, h=H, w=W):
            f = fr(h, w)
            setattr(f, field, value)
            return f

        def bad_frames(h, w):
            out = [broken("y", None, h, w), broken("u", None, h, w), broken("y_row", w - 1, h, w),
                   broken("u_row", (2 * -(-w // 2) if fmt != "i420" else -(-w // 2)) - 1, h, w)]
            if fmt == "i420":
                out += [broken("v", None, h, w), broken("v_row", -(-w // 2) - 1, h, w)]
            if fmt == "p010":
                out += [broken("y", fr(h, w).y + 1, h, w), broken("u", fr(h, w).u + 1, h, w)]   # a 16-bit plane on an odd address
            return out
        ok = dict(src=fr(), fmt=fid, range=0, up=1, a=k.a, b=k.b, c=k.c, d=k.d, H=H, W=W, T=T, O=O, ty0=0, tx0=0, nty=2, ntx=3, dst=Fp, stream=None)
        bads = [dict(src=f) for f in bad_frames(H, W)] + [
            dict(fmt=3), dict(fmt=-1), dict(range=2), dict(range=-1), dict(up=2), dict(up=-1), dict(H=0), dict(W=0), dict(H=-5),
            dict(T=0), dict(T=32), dict(T=96), dict(T=-64), dict(O=-4), dict(O=2), dict(O=36), dict(dst=None), dict(dst=Fp + 2),
            dict(ty0=-1), dict(tx0=-1), dict(nty=0), dict(ntx=0), dict(nty=3), dict(ntx=4), dict(ty0=1, nty=2), dict(tx0=2, ntx=2),
            dict(H=2 ** 31 - 1, W=2 ** 31 - 1, nty=1, ntx=1)]
        for bad in bads:
            a = dict(ok, **bad)
            src = a.pop("src")
            assert L.pc_frame_tiles_cut(C.byref(src), *a.values()) == -1, (fmt, bad)
        assert L.pc_frame_tiles_cut(None, *list(ok.values())[1:]) == -1

        y0, x0, h, w = 40, 50, 30, 60                                             # rows of tiles 0 and 1, columns of tiles 0, 1 and 2
        nbytes = L.pc_frame_tiles_stitch_workspace_size(x0, h, w)
        assert nbytes == 24 * -(-(15 * (-(-110 // 8) - 6)) // 256)
        sok = dict(x=Fp, sxt=3 * T * T, sxc=T * T, sxh=T, H=H, W=W, T=T, O=O, ty0=0, tx0=0, nty=2, ntx=3, y0=y0, x0=x0, h=h, w=w, fmt=fid,
                   range=0, kr=k.kr, kg=k.kg, kb=k.kb, ib=k.ib, ir=k.ir, dst=fr(h, w, base=0x7100_0000_0000), ref=fr(h, w), ws=Wk,
                   nbytes=nbytes, sse=S, stream=None)
        sbads = [dict(dst=f) for f in bad_frames(h, w)] + [dict(ref=f) for f in bad_frames(h, w)] + [
            dict(x=None), dict(x=Fp + 1), dict(sxh=T - 1), dict(sxc=0), dict(sxt=0), dict(fmt=3), dict(fmt=-1), dict(range=2), dict(range=-1),
            dict(H=0), dict(W=0), dict(T=32), dict(T=96), dict(O=2), dict(O=36), dict(O=-4),
            dict(ty0=-1), dict(nty=3), dict(ntx=4), dict(nty=0),                                           # a rectangle outside the grid
            dict(y0=-2), dict(x0=-2), dict(h=0), dict(w=0), dict(y0=80, h=22), dict(x0=100, w=52),        # a window outside the frame
            dict(y0=41), dict(x0=51), dict(h=31), dict(w=61), dict(y0=41, h=59), dict(x0=51, w=99),        # an inadmissible window
            dict(ty0=1, nty=1), dict(nty=1), dict(tx0=1, ntx=2), dict(ntx=2), dict(tx0=1, ntx=1),          # a covering tile is missing
            dict(dst=None, ref=None), dict(ws=None), dict(ws=Wk + 4), dict(sse=None), dict(sse=S + 4), dict(nbytes=nbytes - 1), dict(nbytes=0)]
        for bad in sbads:
            a = dict(sok, **bad)
            args = [C.byref(v) if isinstance(v, frames.Frame) else v for v in a.values()]
            assert L.pc_frame_tiles_stitch(*args) == -1, (fmt, bad)


def test_python_rejects_before_any_device_call(monkeypatch):
    from progressivecodec_amd import frame_tiles as ft

    def touched(*a, **k):
        raise AssertionError("the device was reached")
    for name in ("device", "current_stream", "synchronize", "current_device", "_lazy_init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.setattr(ft, "lib", touched)
    y, uv, u = torch.zeros(6, 10, dtype=torch.uint8), torch.zeros(3, 5, 2, dtype=torch.uint8), torch.zeros(3, 5, dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU"):
        ft.cut_frame((y, uv), "nv12", tile=64)
    with pytest.raises(ValueError, match="GPU"):
        ft.cut_frame((y, u, u), "i420", tile=64)
    with pytest.raises(ValueError, match="GPU"):
        ft.cut_frame((y.to(torch.uint16), uv.to(torch.uint16)), "p010", tile=64)
    with pytest.raises(ValueError, match="one frame"):
        ft.cut_frame((torch.stack([y, y]), torch.stack([uv, uv])), "nv12", tile=64)
    with pytest.raises(ValueError, match="fmt"):
        ft.cut_frame((y, uv), "nv21")
    with pytest.raises(ValueError, match="matrix"):
        ft.cut_frame((y, uv), "nv12", matrix="bt470")
    with pytest.raises(ValueError, match="range"):
        ft.cut_frame((y, uv), "nv12", range="tv")
    with pytest.raises(ValueError, match="upsample"):
        ft.cut_frame((y, uv), "nv12", upsample="cubic")
    with pytest.raises(ValueError, match="2 planes"):
        ft.cut_frame((y, u, u), "nv12")
    with pytest.raises(TypeError, match="uint16"):
        ft.cut_frame((y, uv), "p010")
    with pytest.raises(ValueError, match="UV must be"):
        ft.cut_frame((y, uv[:2]), "nv12")
    g = ft.grid_of(100, 150, 64, 16)
    x = torch.zeros(6, 3, 64, 64)
    with pytest.raises(ValueError, match="GPU"):
        ft.stitch_frame(x, g, "nv12")
    with pytest.raises(ValueError, match="image=False"):
        ft.stitch_frame(x, g, "nv12", image=False)
    with pytest.raises(TypeError, match="float32"):
        ft.stitch_frame(x.double(), g, "nv12")
    with pytest.raises(ValueError, match="x_hat_tiles must be"):
        ft.stitch_frame(x[:5], g, "nv12")
    with pytest.raises(ValueError, match="outside"):
        ft.stitch_frame(x, g, "nv12", window=(0, 0, 102, 150))
    for win in [(1, 0, 2, 2), (0, 1, 2, 2), (0, 0, 3, 2), (0, 0, 2, 3), (41, 51, 59, 99)]:
        with pytest.raises(ValueError, match="admissible"):
            ft.stitch_frame(x, g, "nv12", window=win)
    with pytest.raises(ValueError, match="needs the tiles"):
        ft.stitch_frame(x[:1], g.with_rect((0, 0, 1, 1)), "nv12", window=(0, 0, 50, 20))
    with pytest.raises(ValueError, match="the grid of"):
        ft.stitch_frame(x, g._replace(ny=3, nty=3), "nv12")
    with pytest.raises(ValueError, match="fmt"):
        ft.stitch_frame(x, g, "yuyv")
    with pytest.raises(ValueError, match="range"):
        ft.stitch_frame(x, g, "nv12", range="pc")
    yy, uu = torch.zeros(100, 150, dtype=torch.uint8), torch.zeros(50, 75, 2, dtype=torch.uint8)
    with pytest.raises(ValueError, match="ref: UV must be"):
        ft.stitch_frame(x, g, "nv12", ref=(yy, uu[:2]))
    with pytest.raises(ValueError, match="ref must be on a GPU"):
        ft.stitch_frame(x, g, "nv12", ref=(yy, uu))
    with pytest.raises(ValueError, match="GPU"):
        ft.encode_frame_tiled(None, (y, uv), [0, 1], "nv12", tile=64)
    with pytest.raises(ValueError, match="max_tiles_per_call"):
        ft.encode_frame_tiled(None, (y, uv), [0, 1], "nv12", tile=64, max_tiles_per_call=0)
    assert ft.admissible((4, 6, 1, 1), 5, 7) and not ft.admissible((4, 6, 1, 1), 6, 8)


# -- PCG1 ----------------------------------------------------------------------------------------------------------------------------

def test_pcg1_round_trip():
    from progressivecodec_amd import container, tiles
    from progressivecodec_amd import frame_tiles as ft
    ALL = list(itertools.product(FC.FORMATS, FC.MATRICES, FC.RANGES, FC.UPSAMPLES))
    for (fmt, matrix, rng, up), (H, W, O) in zip(ALL, itertools.cycle([(100, 150, 16), (1, 1, 0), (64, 64, 0), (65, 63, 4)])):
        inner, _ = pct1(H, W, T, O)
        buf = ft.pack_frame_tiled(inner, fmt, matrix, rng, up)
        assert buf[:4] == b"PCG1" and buf[4] == 1 and len(buf) == 10 + len(inner) == ft.HEADER_BYTES + len(inner)
        assert buf[10:] == inner and buf[9] == FC.bits(fmt)
        assert tuple(buf[5:9]) == (FC.FORMATS.index(fmt), ["bt601", "bt709", "bt2020"].index(matrix), FC.RANGES.index(rng), FC.UPSAMPLES.index(up))
        hd = ft.parse_frame_tiled(buf)
        assert (hd["fmt"], hd["matrix"], hd["range"], hd["upsample"], hd["bits"], hd["H"], hd["W"]) == (fmt, matrix, rng, up, FC.bits(fmt), H, W)
        assert hd["inner"] == inner and hd["tiled"] == tiles.parse_tiled(inner)
        assert ft.parse_frame_tiled(bytearray(buf))["inner"] == inner and ft.parse_frame_tiled(memoryview(buf))["W"] == W
    # a PCT2 container is taken as it is, too
    inner2 = tiles.pack_tiled([blob(T, t, qualities=(0.5,)) for t in range(6)], 100, 150, T, 16, contract=1, per_tile_levels=True)
    assert ft.parse_frame_tiled(ft.pack_frame_tiled(inner2, "p010", "bt2020", "full", "nearest"))["tiled"]["magic"] == b"PCT2"
    with pytest.raises(container.ContainerError, match="does not parse"):
        ft.pack_frame_tiled(blob(64, 1), "nv12", "bt709", "limited", "linear")
    with pytest.raises(ValueError, match="fmt"):
        ft.pack_frame_tiled(inner, "nv21", "bt709", "limited", "linear")


def test_pcg1_every_malformed_container_raises_before_the_model(monkeypatch):
    from progressivecodec_amd import container, tiles
    from progressivecodec_amd import frame_tiles as ft
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    inner, blobs = pct1(100, 150, T, 16)
    buf = ft.pack_frame_tiled(inner, "p010", "bt2020", "limited", "linear")

    def patched(off, fmt, *vals):
        b = bytearray(buf)
        struct.pack_into(fmt, b, off, *vals)
        return bytes(b)
    cases = [(b"PCG2" + buf[4:], "not a PCG1"), (b"PCF1" + buf[4:], "not a PCG1"), (inner, "not a PCG1"), (b"", "not a PCG1"), (b"PCG", "not a PCG1"),
             (patched(4, "B", 2), "version"), (patched(4, "B", 0), "version"),
             (patched(5, "B", 3), "corrupt"), (patched(6, "B", 3), "corrupt"), (patched(7, "B", 2), "corrupt"), (patched(8, "B", 2), "corrupt"),
             (patched(5, "B", 255), "corrupt"), (patched(9, "B", 8), "10|bits"), (patched(9, "B", 12), "bits"), (patched(5, "B", 0), "bits"),
             (buf[:10], "does not parse"), (buf[:10] + b"PCB1" + buf[14:], "does not parse"), (buf[:30], "does not parse"),
             (patched(10 + 4, "B", 2), "does not parse"),                                        # the inner version
             (patched(10 + 9, "I", 200), "does not parse"),                                      # the inner H: another grid
             (buf[:10 + tiles.HEADER_BYTES + 16 * 6 - 1], "does not parse")]                     # the inner table is cut short
    for n in range(4, 10):
        cases.append((buf[:n], "truncated"))
    for bad, msg in cases:
        with pytest.raises(container.ContainerError, match=msg):
            ft.parse_frame_tiled(bad)
        with pytest.raises(container.ContainerError, match=msg):
            ft.decode_frame_tiled(None, bad)
    # refusals that need the region, the tiles or the level
    for region in [(1, 0, 2, 2), (0, 1, 2, 2), (0, 0, 3, 2), (0, 0, 2, 3), (0, 0, 101, 150), (-2, 0, 4, 4), (0, 0, 0, 2), "all"]:
        with pytest.raises(container.ContainerError, match="admissible|outside|region"):
            ft.decode_frame_tiled(None, buf, region=region)
    for level in (2, -3):
        with pytest.raises(container.ContainerError, match="no level"):
            ft.decode_frame_tiled(None, buf, level=level)
    with pytest.raises(ValueError, match="fmt"):
        ft.decode_frame_tiled(None, buf, fmt="nv21")
    with pytest.raises(ValueError, match="max_tiles_per_call"):
        ft.decode_frame_tiled(None, buf, max_tiles_per_call=0)
    # a tile whose container is for another tile size, or coded otherwise than its neighbours
    wrong = tiles.pack_tiled(blobs[:5] + [blob(128, 5)], 100, 150, T, 16, contract=1)
    with pytest.raises(container.ContainerError, match="tile 5"):
        ft.decode_frame_tiled(None, ft.pack_frame_tiled(wrong, "nv12", "bt709", "full", "nearest"))
    mixed = tiles.pack_tiled(blobs[:5] + [blob(T, 5, qualities=(0, 0.75))], 100, 150, T, 16, contract=1)
    with pytest.raises(container.ContainerError, match="was coded as"):
        ft.decode_frame_tiled(None, ft.pack_frame_tiled(mixed, "nv12", "bt709", "full", "nearest"))
    with pytest.raises(container.ContainerError, match="contract"):
        monkeypatch.setattr(container, "build_contract_id", lambda: 2)
        ft.decode_frame_tiled(None, buf)
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    # a container cut off inside its payload is refused where a missing tile is needed, before the model
    hd = tiles.parse_tiled(inner)
    cut = buf[:10 + hd["table"][3][0] + hd["table"][3][1]]
    with pytest.raises(container.ContainerError, match="tile 4"):
        ft.decode_frame_tiled(None, cut)
    with pytest.raises(container.ContainerError, match="tile 4"):
        ft.decode_frame_tiled(None, cut, region=(70, 64, 30, 32))
    # nothing above is wrong with a good container: with a model (here: none) the decode goes on to use it
    with pytest.raises(AttributeError):
        ft.decode_frame_tiled(None, buf)
    with pytest.raises(AttributeError):
        ft.decode_frame_tiled(None, cut, level=0, region=(4, 6, 20, 30), fmt="nv12")


def test_the_shared_helper_keeps_decode_tiled_as_it_was(monkeypatch):
    """tiles.decode_tiled and decode_frame_tiled read the same tiles through tiles._decode_region_tiles"""
    from progressivecodec_amd import container, tiles
    from progressivecodec_amd import frame_tiles as ft
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    inner, _ = pct1(100, 150, T, 16)
    seen = []

    class Model:
        def decompress(self, strings, shape, q, mask_pol):
            seen.append((len(strings[1]), tuple(shape), q, mask_pol))
            raise KeyError("far enough")
    for region, n in [((4, 6, 20, 30), 1), ((60, 60, 8, 8), 4), (None, 6)]:
        del seen[:]
        with pytest.raises(KeyError):
            tiles.decode_tiled(Model(), inner, level=1, region=region)
        with pytest.raises(KeyError):
            ft.decode_frame_tiled(Model(), ft.pack_frame_tiled(inner, "i420", "bt601", "full", "linear"), level=1, region=region)
        assert seen == [(n, (1, 1), 0.5, "point-based-std")] * 2, (region, seen)
    del seen[:]
    with pytest.raises(KeyError):
        tiles._decode_region_tiles(Model(), inner, 0, (60, 60, 8, 8), 3)
    assert [s[0] for s in seen] == [3]

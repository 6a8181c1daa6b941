"""Tiled image coding without a GPU: the numpy restatement (tests/tiles_contract.py) against its own definition and against
tests/pixels_contract.py, and libpc_tiles.so's C ABI, progressivecodec_amd.tiles and the PCT1 container up to the first device call:
the grid, exports, the plan, every argument error, every Python-side rejection, packing, parsing, truncation and corruption."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest
import torch

from tests import pixels_contract as K
from tests import tiles_contract as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(T, O) for T in (64, 128) for O in (0, 4, 16, T // 2)]


def lengths(T, O):
    return [1, T - 1, T, T + 1, 2 * T - O, 2 * T - O + 1, 3 * T]


def _lib():
    from progressivecodec_amd import tiles
    return tiles, tiles.lib()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# -- geometry ------------------------------------------------------------------------------------------------------------------------

def test_grid_covers_the_axis_and_equals_the_library_and_python():
    tiles, L = _lib()
    for T, O in GEOMETRIES:
        S = T - O
        for length in lengths(T, O):
            n = TC.axis_tiles(length, T, O)
            count = np.zeros(length, int)
            for i in range(n):
                count[i * S:i * S + T] += 1
            assert count.min() >= 1 and count.max() <= 2, (T, O, length)                  # covered; at most two tiles per axis
            assert (n - 1) * S < length, (T, O, length)                                   # the last tile starts inside the image
            assert n == 1 or (n - 2) * S + T < length, (T, O, length)                     # and is needed
            for p in range(length):
                assert len(TC.covering(p, length, T, O)) == count[p]
            ny, nx = C.c_int(-1), C.c_int(-1)
            assert L.pc_tiles_grid(length, 7, T, O, C.byref(ny), C.byref(nx)) == 0 and (ny.value, nx.value) == (n, 1)
            assert L.pc_tiles_grid(T + 1, length, T, O, C.byref(ny), C.byref(nx)) == 0 and (ny.value, nx.value) == (2, n)
            g = tiles.grid_of(length, T + 1, T, O)
            assert (g.ny, g.nx, g.rect, g.S) == (n, 2, (0, 0, n, 2), S)
    assert TC.grid(2160, 3840, 512, 0) == (5, 8) and TC.grid(2160, 3840, 512, 32) == (5, 8) and TC.grid(100, 150, 64, 16) == (2, 3)


def test_grid_refuses_what_the_geometry_excludes():
    tiles, L = _lib()
    ny, nx = C.c_int(0), C.c_int(0)
    for bad in [(0, 5, 64, 0), (5, 0, 64, 0), (-1, 5, 64, 0), (5, 5, 0, 0), (5, 5, 32, 0), (5, 5, 96, 0), (5, 5, -64, 0), (5, 5, 64, -4),
                (5, 5, 64, 2), (5, 5, 64, 36), (5, 5, 128, 68), (2 ** 31 - 1, 2 ** 31 - 1, 64, 0)]:
        assert L.pc_tiles_grid(*bad, C.byref(ny), C.byref(nx)) == -1, bad
        with pytest.raises(ValueError):
            tiles.grid_of(*bad)
        if bad[0] < 2 ** 31 - 1:
            with pytest.raises(ValueError):
                TC.grid(*bad)
    assert L.pc_tiles_grid(5, 5, 64, 0, None, C.byref(nx)) == -1 and L.pc_tiles_grid(5, 5, 64, 0, C.byref(ny), None) == -1
    assert L.pc_tiles_grid(2 ** 31 - 1, 1, 64, 32, C.byref(ny), C.byref(nx)) == 0 and ny.value == -(-(2 ** 31 - 1 - 64) // 32) + 1


def test_region_tile_sets_at_band_edges():
    tiles, _ = _lib()
    g = tiles.grid_of(100, 150, 64, 16)                               # S = 48: rows of tiles at 0, 48; columns at 0, 48, 96
    assert (g.ny, g.nx) == (2, 3)
    assert g.covering((0, 0, 100, 150)) == (0, 0, 2, 3)
    assert g.covering((0, 0, 48, 48)) == (0, 0, 1, 1)                 # ends on the band's first pixel: tile 0 alone
    assert g.covering((0, 0, 49, 48)) == (0, 0, 2, 1) and g.covering((0, 0, 48, 49)) == (0, 0, 1, 2)
    assert g.covering((63, 63, 1, 1)) == (0, 0, 2, 2)                 # the band's last pixel: both tiles
    assert g.covering((64, 64, 1, 1)) == (1, 1, 1, 1)                 # one past the band: the later tile alone
    assert g.covering((64, 64, 36, 32)) == (1, 1, 1, 1) and g.covering((64, 64, 36, 33)) == (1, 1, 1, 2)
    assert g.covering((99, 149, 1, 1)) == (1, 2, 1, 1) and g.covering((50, 100, 5, 5)) == (0, 1, 2, 2)
    g0 = tiles.grid_of(100, 150, 64, 0)
    assert g0.covering((63, 63, 1, 1)) == (0, 0, 1, 1) and g0.covering((63, 63, 2, 2)) == (0, 0, 2, 2) and g0.covering((64, 128, 1, 1)) == (1, 2, 1, 1)
    for gg in (g, g0):                                                # against the definition, pixel by pixel
        for y0, x0, h, w in [(0, 0, 1, 1), (47, 95, 2, 2), (40, 90, 30, 30), (63, 111, 1, 2), (10, 10, 80, 130)]:
            ys = sorted({i for p in range(y0, y0 + h) for i in TC.covering(p, 100, 64, gg.O)})
            xs = sorted({i for p in range(x0, x0 + w) for i in TC.covering(p, 150, 64, gg.O)})
            assert gg.covering((y0, x0, h, w)) == (ys[0], xs[0], len(ys), len(xs))
    for bad in [(0, 0, 101, 1), (0, 0, 1, 151), (-1, 0, 1, 1), (0, 0, 0, 1), (100, 0, 1, 1), (0, 1, 2)]:
        with pytest.raises(ValueError):
            g.covering(bad)


# -- weights -------------------------------------------------------------------------------------------------------------------------

def test_weights_sum_to_one_mirror_each_other_and_are_one_outside_bands():
    for T, O in GEOMETRIES:
        S = T - O
        for n in (1, 2, 3):
            for i in range(n):
                w = TC.weights(i, n, T, O)
                lo = O if i > 0 else 0
                hi = S if i < n - 1 else T
                assert (bits(w[lo:hi]) == bits(np.float32(1.0))).all(), (T, O, n, i)
                if i > 0:
                    prev = TC.weights(i - 1, n, T, O)
                    for u in range(O):
                        a, b = w[u], prev[S + u]
                        assert a == np.float32(np.float64(2 * u + 1) / np.float64(2 * O))              # the correctly rounded quotient
                        assert abs(np.float64(a) + np.float64(b) - 1.0) <= 2.0 ** -24, (T, O, u)      # one float32 ulp of 1 (below it)
                        assert bits(a) == bits(prev[S + O - 1 - u]) and bits(b) == bits(w[O - 1 - u])   # reflection of the band
                        assert 0 < a < 1 and 0 < b < 1


def test_fmaf_is_the_fused_operation():
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a = rng.uniform(0, 1, 4000).astype(np.float32)
    b = rng.uniform(0, 1, 4000).astype(np.float32)
    c = rng.uniform(0, 1, 4000).astype(np.float32)
    b[:50] = np.float32(1e-40)
    c[50:100] = 0
    a[100:150] = np.float32(2.0 ** -12)
    b[100:150] = np.float32(1 + 2.0 ** -12)                          # products that land on float32 midpoints
    c[100:150] = np.float32(1.0)
    got = TC.fmaf(a, b, c)

    def rn32(fr):                                                    # the exact rational rounded once: the nearest of the float32
        f = np.float32(float(fr))                                    # neighbours of a first guess, a tie going to the even one
        cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
        return min(cands, key=lambda c: (abs(Fraction(float(c)) - fr), int(bits(np.array([c]))[0]) & 1))
    for k in list(range(0, 150)) + list(range(150, 4000, 11)):
        want = rn32(Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k])))
        assert bits(np.array([got[k]]))[0] == bits(np.array([want]))[0], k
    one = np.float32(1.0)
    v = np.array([0.0, 0.25, 1.0, 1e-40, 0.3], np.float32)
    assert np.array_equal(bits(TC.fmaf(one, v, np.float32(0))), bits(v))


def image(H, W, seed=0):
    a = np.random.default_rng(1000 * H + W + seed).integers(0, 256, (3, H, W), dtype=np.uint8)
    flat = a.reshape(-1)
    n = min(256, flat.size)
    flat[:n] = np.arange(n, dtype=np.uint8)
    return a


@pytest.mark.parametrize("hw", [(1, 1), (65, 63), (100, 150), (127, 129)])
def test_cut_then_stitch_gives_the_image_back(hw):
    """O = 0: exactly, both roundings.  O > 0, proved: a band value is m = sum_t w_t v with at most four tiles; each w_t carries at most
    three roundings (two quotients, one product), the exact weights sum to 1, and each of at most four fmaf rounds a value <= 1 + 2^-21
    once, so |m - v| <= (3 + 4) * 2^-24 * (1 + 2^-20) < 2^-21, and |255 m - b| < 255 * 2^-21 + 2^-16 < 2^-12 for the byte b: rounding
    to nearest gives b exactly, truncation gives b or b - 1 and never more than b."""
    H, W = hw
    img = image(H, W)
    for O in (0, 4, 16, 32):
        t = TC.cut(img, "chw", 64, O)
        assert t.shape == (np.prod(TC.grid(H, W, 64, O)), 3, 64, 64)
        near, down = TC.stitch(t, H, W, 64, O, "nearest", "chw"), TC.stitch(t, H, W, 64, O, "trunc", "chw")
        assert np.array_equal(near, img), O
        m = TC.blend(t, H, W, 64, O)
        assert np.abs(m.astype(np.float64) - K.unit(img).astype(np.float64)).max() < 2.0 ** -21
        if O == 0:
            assert np.array_equal(down, img) and np.array_equal(bits(m), bits(K.unit(img)))
        else:
            d = img.astype(int) - down.astype(int)
            assert d.min() >= 0 and d.max() <= 1, O
        assert np.array_equal(TC.stitch(t, H, W, 64, O, "nearest", "hwc"), img.transpose(1, 2, 0))
        su, sf = TC.sums(t, H, W, 64, O, "nearest", img, "chw")
        assert su == [0, 0, 0] and max(sf) <= 3 * H * W * 2.0 ** -42


def test_where_one_tile_covers_a_pixel_the_value_is_that_tile_clamped():
    H, W, T, O = 100, 150, 64, 16
    x = TC.hostile_tiles(6, T, 5)
    m = TC.blend(x, H, W, T, O)
    S = T - O
    for i, j, ys, xs in [(0, 0, slice(0, 48), slice(0, 48)), (1, 2, slice(64, 100), slice(112, 150)), (0, 1, slice(0, 48), slice(64, 96))]:
        want = K.clamp01(x[i * 3 + j, :, ys.start - i * S:ys.stop - i * S, xs.start - j * S:xs.stop - j * S])
        got = m[:, ys, xs]
        assert np.array_equal(got, want)                                                  # as values: -0.0 == +0.0
        assert np.array_equal(bits(got)[want != 0], bits(want)[want != 0])                # bit for bit where it is not a zero
    assert not np.isnan(m).any() and m.min() >= 0 and m.max() <= 1 + 2.0 ** -21


@pytest.mark.parametrize("rounding", ["nearest", "trunc"])
def test_without_overlap_the_stitch_is_the_emit_of_every_tile_pasted_in_place(rounding):
    H, W, T = 100, 150, 64
    x = TC.hostile_tiles(6, T, 9)
    want = np.zeros((3, 128, 192), np.uint8)
    for i in range(2):
        for j in range(3):
            want[:, i * T:(i + 1) * T, j * T:(j + 1) * T] = K.emit(x[i * 3 + j][None], 0, 0, T, T, rounding, "chw")[0]
    assert np.array_equal(TC.stitch(x, H, W, T, 0, rounding, "chw"), want[:, :H, :W])
    win = (30, 60, 50, 70)
    assert np.array_equal(TC.stitch(x, H, W, T, 0, rounding, "hwc", window=win), want[:, 30:80, 60:130].transpose(1, 2, 0))
    sub = x[[1, 2, 4, 5]]                                                                 # the rectangle (0, 1, 2, 2) holds that window
    assert np.array_equal(TC.stitch(sub, H, W, T, 0, rounding, "chw", rect=(0, 1, 2, 2), window=(30, 64, 50, 66)), want[:, 30:80, 64:130])
    with pytest.raises(ValueError):
        TC.stitch(sub, H, W, T, 0, rounding, "chw", rect=(0, 1, 2, 2), window=win)
    ref = image(H, W, 3)
    su, sf = TC.sums(x, H, W, T, 0, rounding, ref, "chw", window=win)
    su2, sf2 = K.sums(_paste(x, T)[None], 30, 60, 50, 70, rounding, ref[None, :, 30:80, 60:130], "chw")
    assert su == su2[0] and sf == sf2[0]


def _paste(x, T):
    out = np.zeros((3, 2 * T, 3 * T), np.float32)
    for i in range(2):
        for j in range(3):
            out[:, i * T:(i + 1) * T, j * T:(j + 1) * T] = x[i * 3 + j]
    return out


# -- the library, no device ----------------------------------------------------------------------------------------------------------

def test_library_exports_every_declared_function():
    tiles, L = _lib()
    hdr = open(os.path.join(ROOT, "progressivecodec_amd", "tiles_csrc", "pc_tiles.h")).read()
    declared = re.findall(r"PC_API\s+[\w\s\*]+?\b(pc_\w+)\s*\(", hdr)
    assert len(declared) == 7 and sorted(declared) == sorted(tiles.EXPORTS)
    for name in declared:
        getattr(L, name)
    assert L.pc_tiles_strerror(-1).decode() and L.pc_tiles_strerror(-6).decode() and L.pc_tiles_last_hip_error() == 0


def test_workspace_size():
    _, L = _lib()
    for x0, h, w in [(0, 1, 1), (0, 2160, 3840), (3, 1, 2), (3, 7, 5), (1, 100, 4), (4, 100, 4), (2, 4097, 1), (5, 300, 4099)]:
        groups = -(-(x0 + w) // 4) - x0 // 4
        assert L.pc_tiles_stitch_workspace_size(x0, h, w) == 48 * -(-(h * groups) // 1024), (x0, h, w)
    for bad in [(-1, 4, 4), (0, 0, 4), (0, 4, 0), (2 ** 31 - 1, 1, 1)]:
        assert L.pc_tiles_stitch_workspace_size(*bad) == 0


def _plan(L, op, u8, layout, sp, sr, f32, ft, fc, fh, x0=0, ref=None, rl=0, rp=0, rr=0):
    wide = C.c_int(-1)
    return L.pc_tiles_plan(op, u8, layout, sp, sr, f32, ft, fc, fh, x0, ref, rl, rp, rr, C.byref(wide)), wide.value


def test_plan_is_host_only_and_reports_the_path():
    """made-up pointer values: nothing may be dereferenced or launched (there is no GPU here)"""
    _, L = _lib()
    HWC, CHW, CUT, ST = 0, 1, 0, 1
    A, Fp, R = 0x7000_0000_1000, 0x7000_0100_0000, 0x7000_0200_0000
    T, H, W = 64, 100, 152
    fs = (3 * T * T, T * T, T)
    ok = lambda *a, **k: _plan(L, *a, **k)
    assert ok(CUT, A, HWC, 0, 3 * W, Fp, *fs) == (0, 1)
    for off in (1, 2, 3):
        assert ok(CUT, A + off, HWC, 0, 3 * W, Fp, *fs) == (0, 0) and ok(CUT, A + off, CHW, H * W, W, Fp, *fs) == (0, 0)
    assert ok(CUT, A, HWC, 0, 3 * W + 1, Fp, *fs) == (0, 0) and ok(CUT, A, HWC, 77, 3 * W, Fp, *fs) == (0, 1)    # s_plane ignored
    assert ok(CUT, A, HWC, 0, 3 * 150, Fp, *fs) == (0, 0) and ok(CUT, A, HWC, 0, 3 * 150 + 2, Fp, *fs) == (0, 1)
    assert ok(CUT, A, CHW, H * W, W, Fp, *fs) == (0, 1) and ok(CUT, A, CHW, H * W + 2, W, Fp, *fs) == (0, 0)
    assert ok(CUT, A, CHW, H * W, W, Fp + 4, *fs) == (0, 0)
    assert ok(CUT, A, HWC, 0, 3 * W, Fp, *fs, 3, R + 1, HWC, 0, 3 * W) == (0, 1)                                   # cut: x0 and ref ignored
    # stitch: the address of image column 4 * (x0 / 4) is what must be aligned
    assert ok(ST, A, HWC, 0, 3 * W, Fp, *fs, 0) == (0, 1) and ok(ST, A, HWC, 0, 3 * W, Fp, *fs, 4) == (0, 1)
    assert ok(ST, A, HWC, 0, 3 * W, Fp, *fs, 1) == (0, 0) and ok(ST, A + 3, HWC, 0, 3 * W, Fp, *fs, 1) == (0, 1)
    assert ok(ST, A + 2, HWC, 0, 3 * W, Fp, *fs, 2) == (0, 1) and ok(ST, A + 1, HWC, 0, 3 * W, Fp, *fs, 3) == (0, 1)
    assert ok(ST, A, CHW, H * W, W, Fp, *fs, 1) == (0, 0) and ok(ST, A + 1, CHW, H * W, W, Fp, *fs, 1) == (0, 1)
    assert ok(ST, A + 3, CHW, H * W, W, Fp, *fs, 7) == (0, 1) and ok(ST, A + 3, CHW, H * W + 1, W, Fp, *fs, 7) == (0, 0)
    assert ok(ST, A, HWC, 0, 3 * W, Fp + 8, *fs, 0) == (0, 0) and ok(ST, A, HWC, 0, 3 * W, Fp, fs[0] + 2, fs[1], fs[2], 0) == (0, 0)
    assert ok(ST, A, HWC, 0, 3 * W, Fp, fs[0], fs[1], T + 4, 0) == (0, 1) and ok(ST, A, HWC, 0, 3 * W, Fp, fs[0], fs[1], T + 1, 0) == (0, 0)
    assert ok(ST, A, HWC, 0, 3 * W, Fp, *fs, 0, R, CHW, H * W, W) == (0, 1) and ok(ST, A, HWC, 0, 3 * W, Fp, *fs, 0, R + 2, CHW, H * W, W) == (0, 0)
    assert ok(ST, A + 3, HWC, 0, 3 * W, Fp, *fs, 1, R + 1, CHW, H * W, W) == (0, 1)
    assert ok(ST, None, 0, 0, 0, Fp, *fs, 0, R, HWC, 0, 3 * W) == (0, 1) and ok(ST, None, 0, 0, 0, Fp, *fs, 0, R + 1, HWC, 0, 3 * W) == (0, 0)
    # refusals
    assert ok(2, A, HWC, 0, 3 * W, Fp, *fs)[0] == -1 and ok(-1, A, HWC, 0, 3 * W, Fp, *fs)[0] == -1
    assert ok(CUT, None, HWC, 0, 3 * W, Fp, *fs)[0] == -1 and ok(ST, None, HWC, 0, 3 * W, Fp, *fs)[0] == -1
    assert ok(CUT, None, 0, 0, 0, Fp, *fs, 0, R, HWC, 0, 3 * W)[0] == -1
    assert ok(CUT, A, 2, 0, 3 * W, Fp, *fs)[0] == -1 and ok(ST, A, HWC, 0, 3 * W, None, *fs)[0] == -1
    assert ok(ST, A, HWC, 0, 3 * W, Fp, *fs, -1)[0] == -1 and ok(ST, A, HWC, 0, 3 * W, Fp, *fs, 0, R, 5, 0, 3 * W)[0] == -1
    assert L.pc_tiles_plan(CUT, A, HWC, 0, 3 * W, Fp, *fs, 0, None, 0, 0, 0, None) == -1


def test_every_argument_error_returns_before_the_device():
    """fake device pointers: every call below must return PC_ERR_ARG without touching them (no GPU here)"""
    _, L = _lib()
    A, Fp, Wk, S = 0x7000_0000_1000, 0x7000_0100_0000, 0x7000_0200_0000, 0x7000_0300_0000
    H, W, T, O = 100, 150, 64, 16                                     # 2 x 3 tiles, S = 48
    cut = dict(src=A, layout=0, sp=0, sr=3 * W, H=H, W=W, T=T, O=O, ty0=0, tx0=0, nty=2, ntx=3, dst=Fp, stream=None)
    for bad in [dict(src=None), dict(dst=None), dict(dst=Fp + 2), dict(layout=2), dict(layout=-1), dict(H=0), dict(W=0), dict(T=0), dict(T=32),
                dict(T=96), dict(O=-4), dict(O=2), dict(O=36), dict(ty0=-1), dict(tx0=-1), dict(nty=0), dict(ntx=0), dict(nty=3), dict(ntx=4),
                dict(ty0=1, nty=2), dict(tx0=2, ntx=2), dict(sr=3 * W - 1), dict(layout=1, sp=0, sr=W), dict(layout=1, sp=H * W, sr=W - 1)]:
        assert L.pc_tiles_cut_u8(*dict(cut, **bad).values()) == -1, bad
    y0, x0, h, w = 10, 20, 80, 100
    nbytes = L.pc_tiles_stitch_workspace_size(x0, h, w)
    st = dict(x=Fp, sxt=3 * T * T, sxc=T * T, sxh=T, H=H, W=W, T=T, O=O, ty0=0, tx0=0, nty=2, ntx=3, y0=y0, x0=x0, h=h, w=w, rounding=0,
              dst=A, dl=0, dp=0, dr=3 * w, ref=A + 0x100000, rl=1, rp=h * W, rr=W, ws=Wk, nbytes=nbytes, su=S, sf=S + 64, stream=None)
    for bad in [dict(x=None), dict(x=Fp + 1), dict(sxh=T - 1), dict(sxc=0), dict(sxt=0), dict(H=0), dict(W=0), dict(T=32), dict(T=96), dict(O=2),
                dict(O=36), dict(ty0=-1), dict(nty=0), dict(ntx=0), dict(nty=3), dict(ntx=4), dict(y0=-1), dict(x0=-1), dict(h=0), dict(w=0),
                dict(y0=21), dict(x0=51), dict(h=91), dict(w=131), dict(rounding=2), dict(rounding=-1), dict(dl=2), dict(rl=7), dict(dr=3 * w - 1),
                dict(dl=1, dp=h * w - 1, dr=w), dict(ws=None), dict(ws=Wk + 4), dict(su=None), dict(sf=None), dict(su=S + 4), dict(sf=S + 68),
                dict(nbytes=nbytes - 1), dict(nbytes=0), dict(rr=w - 1), dict(rp=0), dict(dst=None, ref=None),
                # tiles that cover the window and are not in the rectangle: row 1 (y0 + h > 64), column 0 (x0 < 64), column 2 (x0 + w > 96)
                dict(nty=1), dict(ty0=1, nty=1), dict(tx0=1, ntx=2), dict(ntx=2), dict(tx0=1, ntx=1)]:
        assert L.pc_tiles_stitch_u8(*dict(st, **bad).values()) == -1, bad
    # the band decides: a window that ends at image row 47 needs tile row 0 alone, one that ends at row 48 (in the band) both
    assert L.pc_tiles_stitch_u8(*dict(st, nty=1, y0=0, h=49).values()) == -1
    assert L.pc_tiles_stitch_u8(*dict(st, ty0=1, nty=1, y0=63, h=2).values()) == -1      # row 63 is the band's last: tile row 0 covers it


def test_python_rejects_before_any_device_call(monkeypatch):
    from progressivecodec_amd import container, tiles

    def touched(*a, **k):
        raise AssertionError("the device was reached")
    for name in ("device", "current_stream", "synchronize", "current_device", "_lazy_init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    hwc = torch.zeros(5, 7, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU"):
        tiles.cut(hwc, 64)
    with pytest.raises(ValueError, match="GPU"):
        tiles.cut(hwc.permute(2, 0, 1), 64, layout="chw")
    with pytest.raises(ValueError, match="layout"):
        tiles.cut(hwc, 64, layout="nhwc")
    with pytest.raises(TypeError, match="uint8"):
        tiles.cut(hwc.float(), 64)
    with pytest.raises(TypeError, match="tensor"):
        tiles.cut(hwc.numpy(), 64)
    with pytest.raises(ValueError, match="one image"):
        tiles.cut(hwc[None], 64)
    with pytest.raises(ValueError, match="3 channels"):
        tiles.cut(hwc, 64, layout="chw")
    with pytest.raises(ValueError, match="GPU"):
        tiles.encode_tiled(None, hwc, [0], tile=64)
    with pytest.raises(ValueError, match="max_tiles_per_call"):
        tiles.encode_tiled(None, hwc, [0], tile=64, max_tiles_per_call=0)
    monkeypatch.setattr(tiles, "lib", touched)
    # a "cuda" image cannot be made here: the geometry checks are reached through grid_of, which cut calls before any device call
    for bad in [dict(tile=0), dict(tile=100), dict(tile=-64), dict(tile=64, overlap=2), dict(tile=64, overlap=36), dict(tile=64, overlap=-4)]:
        with pytest.raises(ValueError, match="tile|overlap"):
            tiles.grid_of(5, 7, **bad)
    g = tiles.grid_of(100, 150, 64, 16)
    with pytest.raises(ValueError, match="rect"):
        g.with_rect((0, 0, 3, 1))
    with pytest.raises(ValueError, match="rect"):
        g.with_rect((1, 2, 1, 2))
    x = torch.zeros(6, 3, 64, 64)
    with pytest.raises(ValueError, match="GPU"):
        tiles.stitch(x, g)
    with pytest.raises(ValueError, match="GPU"):
        tiles.stitch(x, g, ref=torch.zeros(100, 150, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="rounding"):
        tiles.stitch(x, g, rounding="floor")
    with pytest.raises(ValueError, match="layout"):
        tiles.stitch(x, g, layout="cwh")
    with pytest.raises(TypeError, match="float32"):
        tiles.stitch(x.double(), g)
    with pytest.raises(TypeError, match="tensor"):
        tiles.stitch(x.numpy(), g)
    with pytest.raises(ValueError, match="x_hat_tiles must be"):
        tiles.stitch(x[:5], g)
    with pytest.raises(ValueError, match="x_hat_tiles must be"):
        tiles.stitch(x[:, :, :63], g)
    with pytest.raises(ValueError, match="outside"):
        tiles.stitch(x, g, window=(0, 0, 101, 150))
    with pytest.raises(ValueError, match="outside"):
        tiles.stitch(x, g, window=(0, 149, 1, 2))
    with pytest.raises(ValueError, match="needs the tiles"):
        tiles.stitch(x[:2], g.with_rect((0, 0, 1, 2)), window=(0, 0, 49, 10))
    with pytest.raises(ValueError, match="grid"):
        tiles.stitch(x, g._replace(ny=3))
    with pytest.raises(ValueError, match="overlap"):
        tiles.stitch(x, g._replace(O=6))
    with pytest.raises(ValueError, match="image=False"):
        tiles.stitch(x, g, image=False)
    with pytest.raises(TypeError, match="uint8"):
        tiles.stitch(x, g, ref=torch.zeros(100, 150, 3))
    with pytest.raises(ValueError, match="layout"):
        tiles.decode_tiled(None, b"", layout="x")
    with pytest.raises(ValueError, match="rounding"):
        tiles.decode_tiled(None, b"", rounding="x")
    with pytest.raises(ValueError, match="max_tiles_per_call"):
        tiles.decode_tiled(None, b"", max_tiles_per_call=0)
    with pytest.raises(container.ContainerError):
        tiles.decode_tiled(None, b"nope")


# -- PCT1 ----------------------------------------------------------------------------------------------------------------------------

def blob(T, tag, contract=1, qualities=(0, 0.5)):
    """a PCB1 container of made-up strings for one T x T tile"""
    from progressivecodec_amd import container
    y = [[bytes([tag, s]) * (1 + s % 3)] for s in range(20)]
    levels = [[y[:10] if q == 0 else y, [bytes([tag])]] for q in qualities]
    return container.pack(levels, (T // 64, T // 64), list(qualities), image_size=(T, T), contract=contract)


def pct1(H=100, W=150, T=64, O=16, contract=1):
    from progressivecodec_amd import tiles
    ny, nx = TC.grid(H, W, T, O)
    blobs = [blob(T, t, contract) for t in range(ny * nx)]
    return tiles.pack_tiled(blobs, H, W, T, O, contract=contract), blobs


def test_pct1_round_trip():
    from progressivecodec_amd import container, tiles
    buf, blobs = pct1()
    hd = tiles.parse_tiled(buf)
    g = hd["grid"]
    assert (g.H, g.W, g.T, g.O, g.ny, g.nx) == (100, 150, 64, 16, 2, 3) and hd["contract"] == 1
    assert hd["payload_start"] == 33 + 16 * 6 == tiles.HEADER_BYTES + 96 and len(buf) == hd["payload_start"] + sum(map(len, blobs))
    assert buf[:4] == b"PCT1" and buf[4] == 1
    off = hd["payload_start"]
    for t, b in enumerate(blobs):
        assert hd["table"][t] == (off, len(b))
        tb, th = tiles.tile_bytes(buf, hd, t)
        assert tb == b and th["image_size"] == (64, 64)
        assert container.unpack(tb, levels=[1], expect_contract=1)[0][0][1] == [bytes([t])]
        off += len(b)
    assert tiles.parse_tiled(memoryview(buf))["table"] == hd["table"]
    with pytest.raises(container.ContainerError, match="6 tile containers"):
        tiles.pack_tiled(blobs[:5], 100, 150, 64, 16, contract=1)


def test_pct1_truncation_at_every_boundary():
    from progressivecodec_amd import container, tiles
    buf, blobs = pct1()
    hd = tiles.parse_tiled(buf)
    for n in list(range(0, hd["payload_start"])):                                         # anywhere inside the header or the table
        with pytest.raises(container.ContainerError):
            tiles.parse_tiled(buf[:n])
    for k in range(6):
        off, n = hd["table"][k]
        for end, whole in [(off, k - 1), (off + 1, k - 1), (off + n - 1, k - 1), (off + n, k)]:
            part = tiles.parse_tiled(buf[:end])                                           # the header and the table are there
            for t in range(6):
                if t <= whole:
                    assert tiles.tile_bytes(buf[:end], part, t)[0] == blobs[t]
                else:
                    with pytest.raises(container.ContainerError, match="truncated"):
                        tiles.tile_bytes(buf[:end], part, t)
    # through decode_tiled: the error comes before the model (None) is touched
    cut = buf[:hd["table"][4][0] + 3]
    with pytest.raises(container.ContainerError, match="tile 4"):
        tiles.decode_tiled(None, cut, region=(70, 60, 10, 10))
    with pytest.raises(container.ContainerError, match="tile 4"):
        tiles.decode_tiled(None, cut)


def test_pct1_corruption_is_refused():
    from progressivecodec_amd import container, tiles
    buf, blobs = pct1()
    hd = tiles.parse_tiled(buf)

    def patched(pos, fmt, value):
        b = bytearray(buf)
        struct.pack_into(fmt, b, pos, value)
        return bytes(b)
    with pytest.raises(container.ContainerError, match="not a PCT1"):
        tiles.parse_tiled(b"PCB1" + buf[4:])
    with pytest.raises(container.ContainerError, match="version"):
        tiles.parse_tiled(patched(4, "<B", 2))
    # header fields: H at 9, W at 13, T at 17, O at 21, ny at 25, nx at 29
    for pos, value in [(9, 0), (9, 129), (13, 49), (13, 2 ** 32 - 1), (17, 0), (17, 32), (17, 128), (21, 2), (21, 36), (25, 3),
                       (25, 0), (29, 2), (29, 2 ** 31)]:
        with pytest.raises(container.ContainerError, match="corrupt header"):
            tiles.parse_tiled(patched(pos, "<I", value))
    # a changed contract id: the tiles no longer agree with the container
    bad = patched(5, "<I", 7)
    with pytest.raises(container.ContainerError, match="contract"):
        tiles.tile_bytes(bad, tiles.parse_tiled(bad), 0)
    with pytest.raises(container.ContainerError, match="contract"):
        tiles.decode_tiled(None, bad)
    # table entries: tile 2's offset at 33 + 32, its length at 33 + 40
    for pos, value in [(65, 0), (65, hd["payload_start"] - 1), (65, len(buf)), (65, 2 ** 63), (73, len(buf)), (73, 2 ** 64 - 1)]:
        b = patched(pos, "<Q", value)
        with pytest.raises(container.ContainerError, match="tile 2"):
            tiles.tile_bytes(b, tiles.parse_tiled(b), 2)
        assert tiles.tile_bytes(b, tiles.parse_tiled(b), 1)[0] == blobs[1]                # the other tiles are not affected
        with pytest.raises(container.ContainerError):
            tiles.decode_tiled(None, b)
    b = patched(65, "<Q", hd["table"][2][0] + 1)                                          # inside the buffer, not at a container
    with pytest.raises(container.ContainerError):
        tiles.tile_bytes(b, tiles.parse_tiled(b), 2)
    # a tile whose PCB1 header disagrees with T
    wrong = tiles.pack_tiled(blobs[:5] + [blob(128, 5)], 100, 150, 64, 16, contract=1)
    with pytest.raises(container.ContainerError, match="not a 64x64 tile"):
        tiles.tile_bytes(wrong, tiles.parse_tiled(wrong), 5)
    with pytest.raises(container.ContainerError, match="not a 64x64 tile"):
        tiles.decode_tiled(None, wrong, region=(99, 149, 1, 1))
    with pytest.raises(ValueError, match="outside"):
        tiles.decode_tiled(None, buf, region=(0, 0, 101, 1))

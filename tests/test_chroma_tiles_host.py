"""Host-only checks of tiled coding of YUV frames of any subsampling and siting: the restatement
tests/chroma_tiles_contract.py against section 14's and section 21's, the C ABI of libpc_chroma_tiles.so up to the first device call,
the PCK1 container, the library's structure and the ledger of kernel instantiations."""
import ctypes as C
import glob
import inspect
import itertools
import os
import re
import struct

import numpy as np
import pytest
import torch

from progressivecodec_amd import chroma_tiles
from tests import chroma_contract as CC
from tests import chroma_tiles_cases as CS
from tests import chroma_tiles_contract as KC
from tests import frame_tiles_contract as GC
from tests import frames_contract as FC
from tests import image_shared
from tests import tiles_contract as TC
from tests.test_chroma_host import fake_frame
from tests.test_image_shared_host import DEFINITIONS
from tests.test_tiles_host import blob, pct1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "progressivecodec_amd")
DIR = os.path.join(PKG, "chroma_tiles_hip")
T = 64
SETTINGS = [("bt709", "limited"), ("bt601", "full"), ("bt2020", "limited")]


def _lib():
    """the module and its library; a library that is not built is an ImportError, as for every other one"""
    return chroma_tiles, chroma_tiles.lib()


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(p, q) for p, q in zip(a, b))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# -- 1. identity with section 14 -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", [(65, 63), (100, 150), (127, 129)])
@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_centre_sited_420_is_section_14_bit_for_bit(hw, fmt):
    H, W = hw
    for n, O in enumerate([0, 4, 16, 32]):
        matrix, rng = SETTINGS[n % 3]
        f = FC.random_frame(1, H, W, fmt, seed=H + n)
        for up in FC.UPSAMPLES:
            assert same_bits(KC.cut(f, fmt, matrix, rng, up, "centre", T, O), GC.cut(f, fmt, matrix, rng, up, T, O))
        ny, nx = TC.grid(H, W, T, O)
        x = TC.hostile_tiles(ny * nx, T, seed=W + n)
        S = T - O
        for win in [None, (2, min(S, 32), 20, W - min(S, 32)), (H - 1 - (H - 1) % 2, 6, 1 + (H - 1) % 2, 10)]:
            assert same(KC.stitch_codes(x, H, W, T, O, fmt, matrix, rng, "centre", window=win), GC.stitch_codes(x, H, W, T, O, fmt, matrix, rng, window=win))
            assert KC.sums(x, H, W, T, O, fmt, matrix, rng, "centre", f, window=win) == GC.sums(x, H, W, T, O, fmt, matrix, rng, f, window=win)


# -- 2. a tile is the crop of the whole frame's ingest -------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", sorted(CC.FORMATS))
def test_every_tile_is_the_crop_of_the_whole_frames_ingest(fmt):
    H, W = 100, 150
    f = CC.random_frame(1, H, W, fmt, seed=11, garbage=True)
    for siting, up, O in itertools.product(CC.SITINGS, CC.UPSAMPLES, (0, 4)):
        S = T - O
        whole = CC.ingest(f, fmt, "bt709", "limited", up, siting, H + T, W + T, 0, 0)[0]       # +0.0 beyond the frame
        ny, nx = TC.grid(H, W, T, O)
        tiles = KC.cut(f, fmt, "bt709", "limited", up, siting, T, O)
        assert tiles.shape == (ny * nx, 3, T, T)
        for i, j in itertools.product(range(ny), range(nx)):
            assert same_bits(tiles[i * nx + j], np.ascontiguousarray(whole[:, i * S:i * S + T, j * S:j * S + T])), (siting, up, O, i, j)
        assert same_bits(KC.cut(f, fmt, "bt709", "limited", up, siting, T, O, rect=(ny - 1, 1, 1, nx - 1)), tiles[(ny - 1) * nx + 1:])


# -- 3. a single tile is section 21 --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", sorted(CC.FORMATS))
def test_the_stitch_of_one_tile_is_section_21s_emit(fmt):
    for n, ((H, W), siting) in enumerate(itertools.product([(1, 1), (2, 3), (3, 2), (37, 53)], CC.SITINGS)):
        matrix, rng = SETTINGS[n % 3]
        x = TC.hostile_tiles(1, T, seed=n)
        assert same(KC.stitch_codes(x, H, W, T, 4 * (n % 3), fmt, matrix, rng, siting), CC.emit_codes(x, 0, 0, H, W, fmt, matrix, rng, siting))


# -- 4. a window is the crop, from the smallest rectangle the halo rule allows -------------------------------------------------------

def windows(H, W, O, fmt, seed):
    """admissible windows: the whole frame, the last row and column (the odd ones of a 127 x 129 frame), one chroma sample, x0 = S and
    y0 = S (the halo lies in the previous tile alone at O = 0, in a band otherwise), x0 = 2, 4, 6 (mod 8), and seeded random ones"""
    sx, sy = CC.sub(fmt)
    S = T - O
    out = [(0, 0, H, W), ((H - 1) // sy * sy, (W - 1) // sx * sx, H - (H - 1) // sy * sy, W - (W - 1) // sx * sx), (sy * 9, sx * 5, sy, sx),
           (0, S, H, W - S), (S, 0, H - S, W), (S, S, 2 * sy, 2 * sx), (S + 2, S + 2, 8, 8),
           (S, S, H - S, W - S), (S + 2, 70, H - S - 2, W - 70)]      # ending on the frame's last row and column (odd ones at 127 x 129)
    out += [(sy * 3, 64 + k, 6, 12) for k in (2, 4, 6)] + [(sy * 3, 8 + k, 6, W - 8 - k) for k in (2, 6)]
    g = np.random.default_rng(seed)
    while len(out) < 22:
        y0, x0 = int(g.integers(0, H // sy)) * sy, int(g.integers(0, W // sx)) * sx
        h = H - y0 if g.random() < 0.3 else min(int(g.integers(1, 20)) * sy, H - y0)
        w = W - x0 if g.random() < 0.3 else min(int(g.integers(1, 20)) * sx, W - x0)
        if (h % sy == 0 or y0 + h == H) and (w % sx == 0 or x0 + w == W):
            out.append((y0, x0, h, w))
    assert all(KC.admissible(H, W, fmt, w) for w in out)
    return out


@pytest.mark.parametrize("hw", [(100, 150), (127, 129)])
@pytest.mark.parametrize("fmt", ["nv12", "nv16", "p210", "i444", "i010"])
@pytest.mark.parametrize("siting", ["left", "topleft"])
def test_an_admissible_windows_stitch_is_the_crop_of_the_whole_frames(fmt, siting, hw):
    """also on a frame with an odd last row and column: a window with x0 > 0 or y0 > 0 that ends there has a halo, a missing second
    row and a missing right neighbour at once"""
    H, W = hw
    sx, sy = CC.sub(fmt)
    hco, vco = sx == 2, sy == 2 and siting == "topleft"
    differs = 0
    for n, O in enumerate([0, 4, 16, 32]):
        matrix, rng = SETTINGS[n % 3]
        S = T - O
        ny, nx = TC.grid(H, W, T, O)
        x = TC.hostile_tiles(ny * nx, T, seed=31 * n + len(fmt))
        ref = CC.random_frame(1, H, W, fmt, seed=n)
        whole = KC.stitch_codes(x, H, W, T, O, fmt, matrix, rng, siting)
        for win in windows(H, W, O, fmt, seed=n):
            rect = KC.covering(H, W, T, O, KC.halo_window(fmt, siting, win))
            idx = [(rect[0] + a) * nx + rect[1] + b for a in range(rect[2]) for b in range(rect[3])]
            got = KC.stitch_codes(x[idx], H, W, T, O, fmt, matrix, rng, siting, rect=rect, window=win)
            want = KC.crop_codes(whole, fmt, win)
            assert same(got, want), (O, win, rect)
            assert KC.sums(x[idx], H, W, T, O, fmt, matrix, rng, siting, ref, rect=rect, window=win) == \
                [int(((g - r) ** 2).sum()) for g, r in zip(want, KC.crop_codes(CC.codes(ref, fmt), fmt, win))]
            # a stitch that clamped its filter at the window's edge is another function wherever there is a halo
            if any(KC.halo(fmt, siting, win)):
                differs += not same(KC.stitch_codes(x, H, W, T, O, fmt, matrix, rng, siting, window=win, frame_edges=False), want)
        # the halo costs a tile row / column exactly where the window starts on a tile origin at O = 0
        own = KC.covering(H, W, T, O, (S, S, 8, 8))
        ext = KC.covering(H, W, T, O, KC.halo_window(fmt, siting, (S, S, 8, 8)))
        assert ext == ((own[0] - (vco and O == 0), own[1] - (hco and O == 0), own[2] + (vco and O == 0), own[3] + (hco and O == 0)))
    assert differs > 20 if hco else differs == 0


def test_the_halo_rule_refuses_the_windows_own_rectangle():
    """x0 = S at O = 0 under "left" at 4:2:0: the tile column left of the window is needed; not under "centre", not at 4:4:4"""
    H, W, O = 100, 150, 0
    ny, nx = TC.grid(H, W, T, O)
    x = TC.hostile_tiles(ny * nx, T, seed=1)
    win = (0, 64, 64, 64)
    own = KC.covering(H, W, T, O, win)
    assert own == (0, 1, 1, 1)
    with pytest.raises(ValueError, match="not in the rectangle"):
        KC.stitch_codes(x[[1]], H, W, T, O, "nv12", "bt709", "limited", "left", rect=own, window=win)
    for fmt, siting in [("nv12", "centre"), ("i444", "left"), ("i444", "topleft")]:
        assert same(KC.stitch_codes(x[[1]], H, W, T, O, fmt, "bt709", "limited", siting, rect=own, window=win),
                    KC.crop_codes(KC.stitch_codes(x, H, W, T, O, fmt, "bt709", "limited", siting), fmt, win))
    # and Python's own rule says the same before any device call
    kt, _ = _lib()
    from progressivecodec_amd import tiles
    g = tiles.grid_of(H, W, T, O)
    assert kt.covering(g, win, "nv12", "left") == (0, 0, 1, 2) and kt.covering(g, win, "nv12", "centre") == own == kt.covering(g, win, "i444", "left")
    assert kt.covering(g, (64, 64, 36, 64), "nv12", "topleft") == (0, 0, 2, 2) and kt.covering(g, (64, 64, 36, 64), "nv16", "topleft") == (1, 0, 1, 2)
    for O2 in (4, 16, 32):                                        # inside a band the previous tile covers x0 already
        g2 = tiles.grid_of(H, W, T, O2)
        S = T - O2
        assert kt.covering(g2, (S, S, 8, 8), "nv12", "topleft") == g2.covering((S, S, 8, 8))


def test_the_admissibility_rule_is_needed():
    """one inadmissible window per rule: its stitch (the window as the picture) is not the crop"""
    H, W, O = 100, 150, 16
    ny, nx = TC.grid(H, W, T, O)
    x = TC.hostile_tiles(ny * nx, T, seed=2)
    kt, _ = _lib()
    for fmt, bad in [("nv12", (1, 0, 4, 8)), ("nv12", (0, 1, 4, 8)), ("nv12", (0, 0, 3, 8)), ("nv12", (0, 0, 4, 7)), ("nv16", (0, 3, 5, 8)),
                     ("nv16", (3, 0, 5, 9))]:
        assert not KC.admissible(H, W, fmt, bad) and not kt.admissible(bad, H, W, fmt)
        with pytest.raises(ValueError, match="admissible"):
            KC.stitch_codes(x, H, W, T, O, fmt, "bt709", "limited", "left", window=bad)
        got = KC.stitch_codes(x, H, W, T, O, fmt, "bt709", "limited", "left", window=bad, check=False)
        whole = KC.stitch_codes(x, H, W, T, O, fmt, "bt709", "limited", "left")
        y0, x0, h, w = bad
        sx, sy = CC.sub(fmt)
        hc, wc = CC.chroma_size(h, w, fmt)
        crop = whole[1][:, y0 // sy:y0 // sy + hc, x0 // sx:x0 // sx + wc]
        assert got[1].shape != crop.shape or not np.array_equal(got[1], crop), (fmt, bad)
    for win in [(1, 3, 5, 7), (99, 149, 1, 1)]:                   # at 4:4:4 every window is admissible, at 4:2:2 every y0 and h
        assert KC.admissible(H, W, "i444", win) and kt.admissible(win, H, W, "p410")
    assert KC.admissible(H, W, "nv16", (3, 2, 5, 8)) and kt.admissible((3, 2, 5, 8), H, W, "p210") and not kt.admissible((3, 2, 5, 7), H, W, "p210")


# -- 5. gray frames ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", sorted(CC.FORMATS))
def test_gray_frames_return_every_nominal_luma_code_through_cut_and_stitch(fmt):
    H, W = 70, 150
    for siting, O in itertools.product(CC.SITINGS, (4, 32)):
        for rng in CC.RANGES:
            yo, ys, co, _, mx = CC.levels(fmt, rng)
            Hc, Wc = CC.chroma_size(H, W, fmt)
            lo, hi = (yo, yo + ys) if rng == "limited" else (0, mx)
            Y = (lo + np.arange(H * W) % (hi - lo + 1)).reshape(1, H, W)
            f = CC.frame(Y, np.full((1, Hc, Wc), co), np.full((1, Hc, Wc), co), fmt)
            tiles = KC.cut(f, fmt, "bt709", rng, "linear", siting, T, O)
            got = KC.stitch_codes(tiles, H, W, T, O, fmt, "bt709", rng, siting)
            assert np.array_equal(got[0], Y) and (got[1] == co).all() and (got[2] == co).all(), (siting, O, rng)


# -- 6. round trips ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", sorted(CC.FORMATS))
def test_cut_then_stitch_gives_the_frame_back(fmt):
    """at 4:4:4 every frame whose colours lie in gamut; for the subsampled formats under "nearest" with chroma constant over the frame"""
    H, W = 67, 130
    sx, sy = CC.sub(fmt)
    g = np.random.default_rng(4)
    for n, (siting, O) in enumerate(itertools.product(CC.SITINGS, (0, 4, 32))):
        yo, ys, co, cs, mx = CC.levels(fmt, "limited")
        Hc, Wc = CC.chroma_size(H, W, fmt)
        Y = g.integers(yo + ys // 4, yo + 3 * ys // 4, (1, H, W))
        if (sx, sy) == (1, 1):
            Cb, Cr = (g.integers(co - cs // 16, co + cs // 16, (1, Hc, Wc)) for _ in range(2))
        else:
            Cb, Cr = (np.full((1, Hc, Wc), co + d) for d in ((n + 1) * 3, -(n + 2) * 2))
        f = CC.frame(Y, Cb, Cr, fmt)
        tiles = KC.cut(f, fmt, "bt709", "limited", "nearest", siting, T, O)
        assert same(KC.stitch_codes(tiles, H, W, T, O, fmt, "bt709", "limited", siting), (Y, Cb, Cr)), (siting, O)


# -- 7. the C ABI up to the first device call ----------------------------------------------------------------------------------------

def test_workspace_size_is_the_documented_formula():
    _, L = _lib()
    for x0, h, w, sy in [(0, 1, 1, 1), (0, 100, 150, 2), (6, 3, 9, 1), (64, 64, 64, 2), (2, 2160, 3838, 1), (0, 2160, 3840, 2), (14, 7, 1, 2)]:
        items = -(-h // sy) * (-(-(x0 + w) // 8) - x0 // 8)
        assert L.pc_chroma_tiles_stitch_workspace_size(x0, h, w, sy) == 24 * -(-items // 256), (x0, h, w, sy)
    for bad in [(-1, 4, 4, 1), (0, 0, 4, 2), (0, 4, 0, 1), (0, 4, 4, 0), (0, 4, 4, 3), (2 ** 31 - 8, 4, 16, 1), (0, 2 ** 31 - 1, 2 ** 31 - 1, 1)]:
        assert L.pc_chroma_tiles_stitch_workspace_size(*bad) == 0, bad


def test_plan_is_host_only_and_each_precondition_is_broken_alone():
    """made-up pointer values: nothing may be dereferenced or launched (there is no GPU here)"""
    kt, L = _lib()
    from progressivecodec_amd import chroma
    Fp = 0x7000_0100_0000
    H, W = 96, 160
    fs0 = (3 * T * T, T * T, T)

    def plan(op, fmt, fr, f32=Fp, fs=fs0, O=0, x0=0, ref=None, sx=None):
        wide = C.c_int(-1)
        f = chroma.FORMATS[fmt]
        rc = L.pc_chroma_tiles_plan(op, f.layout, f.bits, f.sx if sx is None else sx, C.byref(fr) if fr is not None else None, f32, *fs, O, x0,
                                    C.byref(ref) if ref is not None else None, C.byref(wide))
        return rc, wide.value
    for fmt in sorted(chroma.FORMATS):
        f_ = chroma.FORMATS[fmt]
        es = 2 if f_.bits == 10 else 1
        planar = f_.layout == chroma.PLANAR
        ok = fake_frame(chroma, fmt, H, W)
        for op in (kt.CUT, kt.STITCH):
            assert plan(op, fmt, ok) == (0, 1)
            for off in (4, 8, 12):
                assert plan(op, fmt, ok, f32=Fp + off) == (0, 0)
            for k in range(3):
                fs = list(fs0)
                fs[k] += 2
                assert plan(op, fmt, ok, fs=tuple(fs)) == (0, 0)
            for nm in ["y", "u"] + (["v"] if planar else []):
                for off in (1, 2, 3):
                    bad = fake_frame(chroma, fmt, H, W)
                    setattr(bad, nm, getattr(bad, nm) + off * es)
                    assert plan(op, fmt, bad) == (0, 0), (fmt, nm, off)
                bad = fake_frame(chroma, fmt, H, W)
                setattr(bad, nm + "_row", getattr(bad, nm + "_row") + 2)
                assert plan(op, fmt, bad) == (0, 0), (fmt, nm)
                bad = fake_frame(chroma, fmt, H, W)                                         # the batch strides are not looked at
                setattr(bad, nm + "_batch", getattr(bad, nm + "_batch") + 1)
                assert plan(op, fmt, bad) == (0, 1), (fmt, nm)
        # the cut: O a multiple of 8 where a chroma sample spans two luma columns, any O at 4:4:4
        for O in (8, 16, 32):
            assert plan(kt.CUT, fmt, ok, O=O) == (0, 1)
        for O in (4, 12, 20):
            assert plan(kt.CUT, fmt, ok, O=O) == (0, int(f_.sx == 1)), (fmt, O)
            assert plan(kt.STITCH, fmt, ok, O=O) == (0, 1)
        assert plan(kt.CUT, fmt, ok, O=-4)[0] == -1 and plan(kt.CUT, fmt, ok, x0=3, ref=ok) == (0, 1)     # the cut ignores x0 and ref
        # the stitch: frame column 8 * floor(x0 / 8) is the aligned one
        for x0 in range(0, 24, f_.sx):
            k = x0 % 8
            at = fake_frame(chroma, fmt, H, W)
            at.y += k * es
            cb = (2 * k // f_.sx) if not planar else k // f_.sx
            at.u += cb * es
            if planar:
                at.v += cb * es
            assert plan(kt.STITCH, fmt, at, x0=x0) == (0, 1), (fmt, x0)
            assert plan(kt.STITCH, fmt, None, x0=x0, ref=at) == (0, 1)
            if k % 4:
                assert plan(kt.STITCH, fmt, ok, x0=x0) == (0, 0), (fmt, x0)
                assert plan(kt.STITCH, fmt, at, x0=x0, ref=ok) == (0, 0)
        if f_.sx == 2:
            assert plan(kt.STITCH, fmt, ok, x0=3)[0] == -1
        assert plan(kt.STITCH, fmt, ok, x0=-2)[0] == -1
        loose = fake_frame(chroma, fmt, H, W, pad=2)
        assert plan(kt.STITCH, fmt, ok, ref=loose) == (0, 0) and plan(kt.STITCH, fmt, None, ref=loose) == (0, 0)
        assert plan(kt.STITCH, fmt, None)[0] == -1 and plan(kt.CUT, fmt, None, ref=ok)[0] == -1
        assert plan(2, fmt, ok)[0] == -1 and plan(-1, fmt, ok)[0] == -1 and plan(kt.STITCH, fmt, ok, f32=None)[0] == -1
        assert plan(kt.CUT, fmt, ok, sx=3)[0] == -1 and plan(kt.CUT, fmt, ok, sx=0)[0] == -1
        nul = fake_frame(chroma, fmt, H, W)
        nul.u = None
        assert plan(kt.STITCH, fmt, nul)[0] == -1
    ok, wide = fake_frame(chroma, "nv12", H, W), C.c_int(-1)
    for layout, bits in [(2, 8), (-1, 8), (0, 9), (1, 12), (1, 16)]:
        assert L.pc_chroma_tiles_plan(0, layout, bits, 2, C.byref(ok), Fp, 4, 4, 4, 0, 0, None, C.byref(wide)) == -1
    assert L.pc_chroma_tiles_plan(0, 1, 8, 2, C.byref(ok), Fp, 4, 4, 4, 0, 0, None, None) == -1
    assert plan(kt.STITCH, "i420", ok)[0] == -1                                               # a planar frame needs its V plane


def test_every_argument_error_returns_before_the_device():
    """fake device pointers: every call below must return PC_ERR_ARG without touching them (no GPU here)"""
    kt, L = _lib()
    from progressivecodec_amd import chroma, frames
    Fp, Wk, Sp = 0x7000_0100_0000, 0x7000_0200_0000, 0x7000_0300_0000
    H, W, O = 100, 150, 16                                          # S = 48: a 2 x 3 grid
    k = chroma.coefficients("bt709")
    for fmt in sorted(chroma.FORMATS):
        f_ = chroma.FORMATS[fmt]
        planar = f_.layout == chroma.PLANAR
        Wc = chroma.chroma_size(H, W, fmt)[1]
        fr = lambda w=W, **kw: fake_frame(chroma, fmt, H, w, **kw)                              # noqa: E731

        def broken(field, value, w=W):
            f = fr(w)
            setattr(f, field, value)
            return f
        fbads = [dict(layout=2), dict(layout=-1), dict(bits=9), dict(bits=16), dict(shift=1), dict(shift=6 if f_.bits == 8 else 4), dict(sx=3),
                 dict(sx=0), dict(sy=0), dict(sx=1, sy=2), dict(hsite=2), dict(hsite=-1), dict(vsite=2), dict(range=2), dict(range=-1)]
        geo = [dict(H=0), dict(W=0), dict(T=0), dict(T=96), dict(T=-64), dict(O=-4), dict(O=6), dict(O=36), dict(ty0=-1), dict(tx0=-1), dict(nty=0),
               dict(ntx=0), dict(ty0=1, nty=2), dict(tx0=2, ntx=2), dict(nty=3), dict(ntx=4)]
        cok = dict(src=fr(), layout=f_.layout, bits=f_.bits, shift=f_.shift, sx=f_.sx, sy=f_.sy, hsite=1, vsite=1, range=0, up=1, a=k.a, b=k.b,
                   c=k.c, d=k.d, H=H, W=W, T=T, O=O, ty0=0, tx0=0, nty=2, ntx=3, dst=Fp, stream=None)
        bad_src = [broken("y", None), broken("u", None), broken("y_row", W - 1), broken("u_row", (Wc if planar else 2 * Wc) - 1)]
        if planar:
            bad_src += [broken("v", None), broken("v_row", Wc - 1)]
        if f_.bits == 10:
            bad_src += [broken("y", fr().y + 1), broken("u", fr().u + 1)]
        for bad in [dict(src=f) for f in bad_src] + fbads + geo + [dict(up=2), dict(up=-1), dict(dst=None), dict(dst=Fp + 2)]:
            a = dict(cok, **bad)
            src = a.pop("src")
            assert L.pc_chroma_tiles_cut(C.byref(src), *a.values()) == -1, (fmt, bad)
        assert L.pc_chroma_tiles_cut(None, *list(cok.values())[1:]) == -1

        y0, x0, h, w = 2 * f_.sy, 52, 40, 60
        wf = lambda **kw: fake_frame(chroma, fmt, h, w, **kw)                                   # noqa: E731
        wc = chroma.chroma_size(h, w, fmt)[1]
        nbytes = L.pc_chroma_tiles_stitch_workspace_size(x0, h, w, f_.sy)
        assert nbytes > 0
        sok = dict(x=Fp, sxt=3 * T * T, sxc=T * T, sxh=T, H=H, W=W, T=T, O=O, ty0=0, tx0=0, nty=2, ntx=3, y0=y0, x0=x0, h=h, w=w, layout=f_.layout,
                   bits=f_.bits, shift=f_.shift, sx=f_.sx, sy=f_.sy, hsite=1, vsite=1, range=0, kr=k.kr, kg=k.kg, kb=k.kb, ib=k.ib, ir=k.ir,
                   dst=wf(base=0x7100_0000_0000), ref=wf(), ws=Wk, nbytes=nbytes, sse=Sp, stream=None)

        def wbroken(field, value):
            f = wf()
            setattr(f, field, value)
            return f
        bad_win = [wbroken("y", None), wbroken("u", None), wbroken("y_row", w - 1), wbroken("u_row", (wc if planar else 2 * wc) - 1),
                   wbroken("y_row", 2 ** 31), wbroken("u_row", 2 ** 31)]
        if planar:
            bad_win += [wbroken("v", None), wbroken("v_row", wc - 1), wbroken("v_row", 2 ** 31)]
        if f_.bits == 10:
            bad_win += [wbroken("y", wf().y + 1)]
        windows = [dict(y0=-2), dict(x0=-2), dict(h=0), dict(w=0), dict(y0=H - 2, h=4), dict(x0=W - 2, w=4)]
        if f_.sx == 2:
            windows += [dict(x0=x0 + 1), dict(w=w + 1)]
        if f_.sy == 2:
            windows += [dict(y0=y0 + 1), dict(h=h + 1)]
        # the rectangle against the window: x 52 .. 111 lies in tile columns 0 (band 48 .. 63), 1 and 2; its rows in tile row 0
        rects = [dict(tx0=1, ntx=2), dict(ntx=2), dict(ty0=1, nty=1)]
        halo = []
        if f_.sx == 2:                                              # at O = 0 the halo of x0 = 64, column 63, is tile column 0's alone
            halo += [dict(x0=64, w=40, O=0, tx0=1, ntx=2)]
        if f_.sy == 2:
            halo += [dict(y0=64, h=36, O=0, ty0=1, nty=1)]
        ebads = ([dict(dst=f) for f in bad_win] + [dict(ref=f) for f in bad_win] + fbads + geo + windows + rects + halo +
                 [dict(x=None), dict(x=Fp + 1), dict(sxh=T - 1), dict(sxc=0), dict(sxt=0), dict(dst=None, ref=None), dict(ws=None), dict(ws=Wk + 4),
                  dict(sse=None), dict(sse=Sp + 4), dict(nbytes=nbytes - 1), dict(nbytes=0)])
        for bad in ebads:
            a = dict(sok, **bad)
            args = [C.byref(v) if isinstance(v, frames.Frame) else v for v in a.values()]
            assert L.pc_chroma_tiles_stitch(*args) == -1, (fmt, bad)
    assert L.pc_chroma_tiles_last_hip_error() == 0


def test_python_rejects_before_any_device_call(monkeypatch):
    from progressivecodec_amd import chroma_tiles as kt
    from progressivecodec_amd import tiles

    def touched(*a, **k):
        raise AssertionError("the device was reached")
    for name in ("device", "current_stream", "synchronize", "current_device", "_lazy_init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.setattr(kt, "lib", touched)
    y, uv, u = torch.zeros(6, 10, dtype=torch.uint8), torch.zeros(6, 5, 2, dtype=torch.uint8), torch.zeros(6, 10, dtype=torch.uint8)
    for planes, fmt in [((y, uv), "nv16"), ((y, u, u), "i444"), ((y.to(torch.uint16), uv.to(torch.uint16)), "p210")]:
        with pytest.raises(ValueError, match="GPU"):
            kt.cut_frame(planes, fmt, siting="left", tile=64)
    with pytest.raises(ValueError, match="fmt"):
        kt.cut_frame((y, uv), "nv21")
    with pytest.raises(ValueError, match="siting"):
        kt.cut_frame((y, uv), "nv16", siting="top")
    with pytest.raises(ValueError, match="one frame"):
        kt.cut_frame((y[None].repeat(2, 1, 1), uv[None].repeat(2, 1, 1, 1)), "nv16")
    with pytest.raises(ValueError, match="GPU"):
        kt.encode_frame_tiled(None, (y, uv), [0], "nv16", siting="left", tile=64)
    g = tiles.grid_of(100, 150, 64, 0)
    x = torch.zeros(g.n, 3, 64, 64)
    with pytest.raises(ValueError, match="GPU"):
        kt.stitch_frame(x, g, "nv16", siting="topleft")
    with pytest.raises(ValueError, match="image=False"):
        kt.stitch_frame(x, g, "nv16", image=False)
    with pytest.raises(ValueError, match="admissible"):
        kt.stitch_frame(x, g, "nv16", window=(0, 1, 4, 4))
    with pytest.raises(ValueError, match="halo"):
        kt.stitch_frame(x[1:2], g.with_rect((0, 1, 1, 1)), "nv16", siting="left", window=(0, 64, 64, 64))
    with pytest.raises(ValueError, match="GPU"):                                               # the same tiles do under "centre"
        kt.stitch_frame(x[1:2], g.with_rect((0, 1, 1, 1)), "nv16", siting="centre", window=(0, 64, 64, 64))
    with pytest.raises(ValueError, match="ref must be on a GPU"):
        kt.stitch_frame(x, g, "nv16", ref=(torch.zeros(100, 150, dtype=torch.uint8), torch.zeros(100, 75, 2, dtype=torch.uint8)))
    assert issubclass(kt.ChromaTilesError, kt._imagelib.ImageLibError)
    assert list(inspect.signature(kt.cut_frame).parameters) == ["planes", "fmt", "matrix", "range", "upsample", "siting", "tile", "overlap", "rect"]
    assert list(inspect.signature(kt.stitch_frame).parameters) == ["x_hat_tiles", "grid", "fmt", "matrix", "range", "siting", "window", "ref", "image"]
    assert inspect.signature(kt.cut_frame).parameters["siting"].default == "centre"


# -- 8. PCK1 -------------------------------------------------------------------------------------------------------------------------

def test_pck1_round_trip():
    from progressivecodec_amd import chroma, container, frame_tiles, tiles
    from progressivecodec_amd import chroma_tiles as kt
    params = itertools.product(sorted(chroma.FORMATS), chroma.SITINGS, CC.MATRICES, CC.RANGES, CC.UPSAMPLES)
    inners = {s: pct1(*s)[0] for s in [(100, 150, T, 16), (1, 1, T, 0), (64, 64, T, 0), (65, 63, T, 4)]}
    for (fmt, siting, matrix, rng, up), key in zip(params, itertools.cycle(inners)):
        inner = inners[key]
        buf = kt.pack_frame_tiled(inner, fmt, matrix, rng, up, siting)
        f, (hs, vs) = chroma.FORMATS[fmt], chroma.SITINGS[siting]
        assert buf[:4] == b"PCK1" and buf[4] == 1 and len(buf) == 15 + len(inner) == kt.HEADER_BYTES + len(inner) and buf[15:] == inner
        assert tuple(buf[5:15]) == (f.layout, f.shift, f.sx, f.sy, hs, vs, chroma._MATRIX_ID[matrix], chroma.RANGES[rng], chroma.UPSAMPLES[up], f.bits)
        hd = kt.parse_frame_tiled(buf)
        assert (hd["fmt"], hd["siting"], hd["matrix"], hd["range"], hd["upsample"], hd["bits"], hd["H"], hd["W"]) == \
            (fmt, siting, matrix, rng, up, f.bits) + key[:2]
        assert hd["inner"] == inner and hd["tiled"] == tiles.parse_tiled(inner)
        assert kt.parse_frame_tiled(bytearray(buf))["inner"] == inner and kt.parse_frame_tiled(memoryview(buf))["W"] == key[1]
    inner = inners[(100, 150, T, 16)]
    inner2 = tiles.pack_tiled([blob(T, t, qualities=(0.5,)) for t in range(6)], 100, 150, T, 16, contract=1, per_tile_levels=True)
    assert kt.parse_frame_tiled(kt.pack_frame_tiled(inner2, "p210", "bt2020", "full", "nearest", "left"))["tiled"]["magic"] == b"PCT2"
    with pytest.raises(container.ContainerError, match="does not parse"):
        kt.pack_frame_tiled(blob(64, 1), "nv16", "bt709", "limited", "linear", "left")
    with pytest.raises(ValueError, match="fmt"):
        kt.pack_frame_tiled(inner, "nv21", "bt709", "limited", "linear", "left")
    with pytest.raises(ValueError, match="siting"):
        kt.pack_frame_tiled(inner, "nv16", "bt709", "limited", "linear", "bottom")
    # PCK1, PCG1 and PCH1 do not read each other
    pck = kt.pack_frame_tiled(inner, "nv12", "bt709", "limited", "linear", "centre")
    pcg = frame_tiles.pack_frame_tiled(inner, "nv12", "bt709", "limited", "linear")
    with pytest.raises(container.ContainerError, match="not a PCG1"):
        frame_tiles.parse_frame_tiled(pck)
    with pytest.raises(container.ContainerError, match="not a PCK1"):
        kt.parse_frame_tiled(pcg)
    with pytest.raises(container.ContainerError, match="not a PCH1"):
        chroma.parse_frame(pck)
    assert frame_tiles.MAGIC == b"PCG1" and frame_tiles.HEADER_BYTES == 10 and chroma.MAGIC == b"PCH1" and chroma.HEADER_BYTES == 23


def test_pck1_every_malformed_container_raises_before_the_model(monkeypatch):
    from progressivecodec_amd import chroma, container, frame_tiles, tiles
    from progressivecodec_amd import chroma_tiles as kt
    from tests.test_frames_host import pcb1
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    inner, blobs = pct1(100, 150, T, 16)
    buf = kt.pack_frame_tiled(inner, "p210", "bt2020", "limited", "linear", "left")
    # offsets: 4 version, 5 layout, 6 shift, 7 sx, 8 sy, 9 hsite, 10 vsite, 11 matrix, 12 range, 13 upsample, 14 bits, 15 the inner container
    assert tuple(buf[4:15]) == (1, 1, 6, 2, 1, 1, 0, 2, 0, 1, 10)

    def patched(off, fmt, *vals):
        b = bytearray(buf)
        struct.pack_into(fmt, b, off, *vals)
        return bytes(b)
    pcg = frame_tiles.pack_frame_tiled(inner, "p010", "bt2020", "limited", "linear")
    pch = chroma.pack_frame(pcb1(100, 150), "p210", "bt2020", "limited", "linear", "left", 100, 150)
    cases = [(b"PCK2" + buf[4:], "not a PCK1"), (pcg, "not a PCK1"), (pch, "not a PCK1"), (inner, "not a PCK1"), (b"", "not a PCK1"), (b"PCK", "not a PCK1"),
             (patched(4, "B", 2), "version"), (patched(4, "B", 0), "version"),
             (patched(5, "B", 2), "corrupt"), (patched(5, "B", 0), "corrupt"),                   # planar with shift 6 is none of the twelve
             (patched(6, "B", 0), "corrupt"), (patched(6, "B", 4), "corrupt"), (patched(7, "B", 0), "corrupt"), (patched(7, "B", 4), "corrupt"),
             (patched(8, "B", 0), "corrupt"), (patched(8, "B", 3), "corrupt"), (patched(9, "B", 2), "corrupt"),
             (patched(9, "BB", 0, 1), "corrupt"),                                               # (centre, co-sited) is no siting
             (patched(10, "B", 7), "corrupt"), (patched(11, "B", 3), "corrupt"), (patched(12, "B", 2), "corrupt"), (patched(13, "B", 2), "corrupt"),
             (patched(14, "B", 8), "corrupt"), (patched(14, "B", 12), "bits"), (patched(14, "B", 0), "bits"),
             (buf[:15], "does not parse"), (buf[:15] + b"PCB1" + buf[19:], "does not parse"), (buf[:35], "does not parse"),
             (patched(15 + 4, "B", 2), "does not parse"),                                        # the inner version
             (patched(15 + 9, "I", 200), "does not parse"),                                      # the inner H: another grid
             (buf[:15 + tiles.HEADER_BYTES + 16 * 6 - 1], "does not parse")]                    # the inner table is cut short
    for n in range(4, 15):
        cases.append((buf[:n], "truncated"))
    for bad, msg in cases:
        with pytest.raises(container.ContainerError, match=msg):
            kt.parse_frame_tiled(bad)
        with pytest.raises(container.ContainerError, match=msg):
            kt.decode_frame_tiled(None, bad)
    # refusals that need the region or the level: 4:2:2 takes every y0 and h, and no odd x0 or w
    for region in [(0, 1, 2, 2), (0, 0, 2, 3), (0, 0, 101, 150), (-2, 0, 4, 4), (0, 0, 0, 2), "all"]:
        with pytest.raises(container.ContainerError, match="admissible|outside|region"):
            kt.decode_frame_tiled(None, buf, region=region)
    for region in [(1, 0, 2, 2), (0, 0, 3, 2)]:                   # ... which the stored format takes and NV12 does not
        with pytest.raises(container.ContainerError, match="admissible"):
            kt.decode_frame_tiled(None, buf, region=region, fmt="nv12")
        with pytest.raises(AttributeError):
            kt.decode_frame_tiled(None, buf, region=region)
    for level in (2, -3):
        with pytest.raises(container.ContainerError, match="no level"):
            kt.decode_frame_tiled(None, buf, level=level)
    with pytest.raises(ValueError, match="fmt"):
        kt.decode_frame_tiled(None, buf, fmt="nv21")
    with pytest.raises(ValueError, match="siting"):
        kt.decode_frame_tiled(None, buf, siting="middle")
    with pytest.raises(ValueError, match="max_tiles_per_call"):
        kt.decode_frame_tiled(None, buf, max_tiles_per_call=0)
    with pytest.raises(container.ContainerError, match="contract"):
        monkeypatch.setattr(container, "build_contract_id", lambda: 2)
        kt.decode_frame_tiled(None, buf)
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    with pytest.raises(AttributeError):                            # nothing is wrong with a good container: the decode goes on to the model
        kt.decode_frame_tiled(None, buf)


def test_a_region_decodes_exactly_the_tiles_of_its_halo_extended_window(monkeypatch):
    from progressivecodec_amd import container
    from progressivecodec_amd import chroma_tiles as kt
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    seen = []

    class Model:
        def decompress(self, strings, shape, q, mask_pol):
            seen.append([z[0] for z in strings[1]])                # a tile's z string is its tag: its index in the grid
            raise KeyError("far enough")

    def tiles_of(buf, region, **kw):
        del seen[:]
        with pytest.raises(KeyError):
            kt.decode_frame_tiled(Model(), buf, level=1, region=region, **kw)
        assert len(seen) == 1
        return seen[0]
    inner0 = pct1(100, 150, T, 0)[0]                                # 2 x 3 tiles, S = 64
    left = kt.pack_frame_tiled(inner0, "nv12", "bt709", "limited", "linear", "left")
    assert tiles_of(left, (0, 64, 64, 64)) == [0, 1]               # the halo column 63 is tile 0's
    assert tiles_of(left, (0, 64, 64, 64), siting="centre") == [1] and tiles_of(left, (0, 64, 64, 64), fmt="i444") == [1]
    assert tiles_of(left, (64, 64, 36, 64)) == [3, 4] and tiles_of(left, (64, 64, 36, 64), siting="topleft") == [0, 1, 3, 4]
    assert tiles_of(left, (64, 0, 36, 64), siting="topleft") == [0, 3] and tiles_of(left, (64, 0, 36, 64), fmt="nv16", siting="topleft") == [3]
    assert tiles_of(left, (0, 66, 10, 10)) == [1] and tiles_of(left, None) == [0, 1, 2, 3, 4, 5]
    inner16 = pct1(100, 150, T, 16)[0]                              # 2 x 3 tiles, S = 48: column 47 is tile 0's alone, 48 .. 63 a band
    band = kt.pack_frame_tiled(inner16, "p210", "bt2020", "limited", "linear", "topleft")
    assert tiles_of(band, (0, 48, 40, 16)) == [0, 1] and tiles_of(band, (0, 50, 40, 14)) == [0, 1] and tiles_of(band, (0, 64, 40, 16)) == [0, 1]
    assert tiles_of(band, (0, 66, 40, 16)) == [1] and tiles_of(band, (0, 64, 40, 16), fmt="p410") == [1]
    assert tiles_of(band, (0, 48, 40, 16), max_tiles_per_call=1) == [0]


def test_the_container_does_not_depend_on_max_tiles_per_call(monkeypatch):
    """_tilecodec.encode_items against a fake model and a fake cut: the PCK1 bytes are the same however the tiles are chunked"""
    from progressivecodec_amd import chroma_tiles as kt
    from progressivecodec_amd import container, tiles
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    g = tiles.grid_of(100, 150, T, 16)
    chunks = []

    class Model:
        def compress_levels(self, x, qualities, mask_pol):
            chunks.append(len(x))
            return [{"strings": [[[bytes([t, s]) for t in x] for s in range(10 if q == 0 else 20)], [bytes([t]) for t in x]], "shape": (1, 1)}
                    for q in qualities]
    monkeypatch.setattr(kt, "cut_frame", lambda planes, *a, **k: (list(range(g.n)), g))
    bufs = []
    for per_call in (1, 5, 32):
        del chunks[:]
        bufs.append(kt.encode_frame_tiled(Model(), None, [0, 0.5], "p210", siting="left", tile=T, overlap=16, max_tiles_per_call=per_call))
        assert chunks == [min(per_call, g.n - a) for a in range(0, g.n, per_call)]
    assert bufs[0] == bufs[1] == bufs[2] and bufs[0][:4] == b"PCK1"
    hd = kt.parse_frame_tiled(bufs[0])
    assert (hd["fmt"], hd["siting"], hd["H"], hd["W"]) == ("p210", "left", 100, 150) and len(hd["tiled"]["table"]) == g.n


# -- 9. structure --------------------------------------------------------------------------------------------------------------------

def test_the_thirteenth_library_keeps_the_rules_of_the_twelve():
    kt, L = _lib()
    from progressivecodec_amd import chroma
    hdr = open(os.path.join(DIR, "pc_chroma_tiles.h")).read()
    declared = re.findall(r"PC_API\s+[\w\s\*]+?\b(pc_\w+)\s*\(", hdr)
    assert len(declared) == 6 and sorted(declared) == sorted(kt.EXPORTS)
    for name in declared:
        getattr(L, name)
    assert L.pc_chroma_tiles_strerror(-1).decode() and L.pc_chroma_tiles_strerror(-6).decode() and L.pc_chroma_tiles_last_hip_error() == 0
    assert kt.LIB_PATH == os.path.join(PKG, "libpc_chroma_tiles.so")
    assert issubclass(kt.ChromaTilesError, kt._imagelib.ImageLibError)
    mk = image_shared.uncommented(os.path.join(DIR, "Makefile"))
    assert mk == "NAME := chroma_tiles\ninclude ../image_csrc/lib.mk\n"
    top = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\bchroma_tiles\b", top, re.M) and re.search(r"^\.PHONY:.*\bchroma_tiles\b", top, re.M)
    assert "$(MAKE) -C ../chroma_tiles_hip clean" in top and re.search(r"^chroma_tiles:\n\t\$\(MAKE\) -C \.\./chroma_tiles_hip$", top, re.M)
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(DIR, "*")) if not p.endswith((".o", ".so")))
    assert names == ["Makefile", "pc_chroma_tiles.h", "pc_chroma_tiles.hip"]
    assert len(glob.glob(os.path.join(PKG, "*_csrc", "*.hip"))) == len(image_shared.LIBS) == 10
    src = open(os.path.join(DIR, "pc_chroma_tiles.hip")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert '#include "pc_image_host.h"' in src and "pc_chroma.h" not in code and "pc_frame_tiles.h" not in code
    for name, pattern in DEFINITIONS.items():
        assert not re.search(pattern, code), name
    shared = ("HIPCHK", "g_last_hip", "Planes", "load4", "store4", "store8", "Levels", "IngestCoef", "EmitCoef",
              "emit_px", "clampi", "clamp01", "block_reduce", "gather_partials", "plane_wide", "f32_wide", "upsample_ok", "cdiv", "F32",
              "geo_of", "rect_ok", "first_tile", "last_tile",
              "ingest_item", "Taps", "taps_of", "code_of", "word_of", "Fmt", "format_of", "with_format", "picture_ok", "site_ok", "depth_levels")
    for name in shared:
        assert re.search(r"\b%s\b" % name, code), name
        assert not re.search(r"\b(struct|void|int|bool|unsigned|float|define)\s+%s\b\s*[({]" % name, code), name
    image_shared.assert_frame_is_shared(hdr, "pc_cht_frame")
    found = dict(re.findall(r"\b(PC_CHT_(?:LIMITED|FULL|NEAREST|LINEAR)) = (\w+)", hdr))
    assert found == {"PC_CHT_" + k: "PC_YUV_" + k for k in ("LIMITED", "FULL", "NEAREST", "LINEAR")}
    assert "PC_YUV_" not in re.sub(r"PC_YUV_(LIMITED|FULL|NEAREST|LINEAR|NV12|P010)\b", "", hdr + code)
    values = dict((k, int(v)) for k, v in re.findall(r"\b(PC_CHT_\w+) = (\d+)", hdr))
    assert values == {"PC_CHT_PLANAR": chroma.PLANAR, "PC_CHT_SEMIPLANAR": chroma.SEMIPLANAR, "PC_CHT_CENTRE": chroma.CENTRE,
                      "PC_CHT_COSITED": chroma.COSITED, "PC_CHT_CUT": kt.CUT, "PC_CHT_STITCH": kt.STITCH}
    assert not re.search(r"\batomic(Add|CAS|Exch|Max|Min|Or|And)\b|\basm\b|__asm|__shared__|__syncthreads|__builtin_amdgcn", code)
    import bench
    assert "chroma" not in inspect.getsource(bench.source_hash) and "_hip" not in inspect.getsource(bench.source_hash)
    from progressivecodec_amd import _imagelib
    assert "thirteen" in _imagelib.__doc__ and "chroma_tiles" in _imagelib.__doc__


# -- 10. the ledger ------------------------------------------------------------------------------------------------------------------

def test_every_instantiation_is_launched():
    """pc_chroma_tiles.hip: "24 cut kernels, 64 stitch kernels".  The tuples the table reaches are exactly those; a case taken away
    shows here by the names of the kernels nothing launches any more"""
    src = open(os.path.join(DIR, "pc_chroma_tiles.hip")).read()
    assert "24 cut kernels, 64 stitch kernels" in src
    assert len(CS.ALL_CUT) == 24 and len(CS.ALL_STITCH) == 64
    table = CS.table()
    assert len(table) == 12 * 6 + 4 * 6 and len(set(table)) == len(table)
    cut, stitch = CS.reached(table)
    assert cut == CS.ALL_CUT, "never launched: %s" % CS.names(CS.ALL_CUT - cut)
    assert stitch == CS.ALL_STITCH, "never launched: %s" % CS.names(CS.ALL_STITCH - stitch)
    # the cases the issue names: all twelve formats x three sitings at 100 x 150 with O in {0, 4}; four formats at the other sizes
    assert {(c.fmt, c.siting, c.O) for c in table if (c.H, c.W) == (100, 150)} == set(itertools.product(CC.FORMATS, CC.SITINGS, (0, 4)))
    assert {(c.fmt, c.H, c.W) for c in table if c.n >= 100} == set((f, H, W) for f in CS.OTHER_FORMATS for H, W in CS.OTHER_SIZES)
    assert {c.O for c in table if c.n >= 100} == {16, 32} and {(c.matrix, c.rng) for c in table if c.n >= 100} == set(CS.OTHER_SETTINGS)
    # both paths for every siting of every format
    for fmt, siting in itertools.product(CC.FORMATS, CC.SITINGS):
        assert {CS.stitch_wide(c) for c in table if (c.fmt, c.siting) == (fmt, siting) and c.n < 100} == {False, True}
    # the ledger notices a case that leaves
    less = [c for c in table if not (c.fmt == "i010" and c.siting == "topleft" and not c.aligned)]
    assert CS.ALL_STITCH - CS.reached(less)[1] == {(2, False, 2, 2, True, False, False), (2, False, 2, 2, True, False, True)}
    assert CS.names([(2, False, 2, 2, True, False, False)]) == ["u16 planar 2:2 vco narrow image"]

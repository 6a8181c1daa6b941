"""The chroma layer (4:2:0 / 4:2:2 / 4:4:4, centre / left / top-left siting) without a GPU: the restatement
(tests/chroma_contract.py) against tests/frames_contract.py where the two must agree, against what a siting means, against the round
trips the contract promises and against the float64 formulas; libpc_chroma.so's C ABI up to the first device call; the PCH1 container
up to the model; and the structure of the twelfth image-side library (the rules of the eleven, sections 19 and 20)."""
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

from tests import chroma_cases as CS
from tests import chroma_contract as CC
from tests import frames_contract as FC
from tests import image_shared
from tests import pixels_contract as K
from tests.test_frames_host import pcb1
from tests.test_image_shared_host import DEFINITIONS
from tests.test_tiles_host import blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "progressivecodec_amd")
DIR = os.path.join(PKG, "chroma_hip")
U = 2.0 ** -24                                   # the unit roundoff of float32
SIZES = [(1, 1), (2, 3), (3, 2), (37, 53)]
SUBSAMPLED = [f for f in CC.FORMATS if CC.sub(f) != (1, 1)]
FULL_RES = [f for f in CC.FORMATS if CC.sub(f) == (1, 1)]


def _lib():
    from progressivecodec_amd import chroma
    return chroma, chroma.lib()


def same_frames(a, b):
    return len(a) == len(b) and all(p.dtype == q.dtype and p.shape == q.shape and (p == q).all() for p, q in zip(a, b))


# -- 1. agreement with frames on 4:2:0 centre ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,matrix,rng", list(itertools.product(FC.FORMATS, FC.MATRICES, FC.RANGES)))
def test_restatement_is_frames_at_420_centre(fmt, matrix, rng):
    assert fmt in CC.FORMATS and CC.sub(fmt) == (2, 2) and CC.levels(fmt, rng) == FC.levels(fmt, rng)
    for n, (H, W) in enumerate(SIZES):
        hp, wp, top, left = 64, 64, 3 + n, 5 + n
        f = FC.random_frame(2, H, W, fmt, seed=11 + n)
        assert same_frames(CC.frame(*CC.codes(f, fmt), fmt), f)
        for up in FC.UPSAMPLES:
            want = FC.ingest(f, fmt, matrix, rng, up, hp, wp, top, left)
            got = CC.ingest(f, fmt, matrix, rng, up, "centre", hp, wp, top, left)
            assert got.dtype == np.float32 and (got.view(np.uint32) == want.view(np.uint32)).all(), (H, W, up)
        for x in (FC.hostile_planes(f, fmt, matrix, rng, hp, wp, top, left, seed=3 + n),
                  np.random.default_rng(n).uniform(-0.2, 1.2, (2, 3, hp, wp)).astype(np.float32)):
            want = FC.emit_codes(x, top, left, H, W, fmt, matrix, rng)
            got = CC.emit_codes(x, top, left, H, W, fmt, matrix, rng, "centre")
            assert all((g == w).all() for g, w in zip(got, want)), (H, W)
            assert same_frames(CC.emit(x, top, left, H, W, fmt, matrix, rng, "centre"), FC.emit(x, top, left, H, W, fmt, matrix, rng))
            assert CC.sums(x, top, left, H, W, fmt, matrix, rng, "centre", f) == FC.sums(x, top, left, H, W, fmt, matrix, rng, f)


# -- 2. tap weights ------------------------------------------------------------------------------------------------------------------

def test_tap_weights_sum_to_4_per_axis_and_16_per_pixel():
    for N, odd, sub, linear, co in itertools.product((1, 2, 3, 4, 5), (0, 1), (False, True), (False, True), (False, True)):
        L = (2 * N - odd if sub else N)                          # luma samples that N chroma samples serve
        for r in range(L):
            (i0, w0), (i1, w1) = CC.taps(r, N, sub, linear, co)
            assert w0 + w1 == 4 and w0 > 0 and w1 >= 0 and 0 <= i0 < N and 0 <= i1 < N, (N, L, r, sub, linear, co)
            assert i0 == (r >> 1 if sub else r) and abs(i1 - i0) <= 1
            if not sub or not linear:
                assert (w0, w1) == (4, 0)
    for fmt, siting, up in itertools.product(("nv12", "nv16", "nv24"), CC.SITINGS, CC.UPSAMPLES):
        for H, W in [(1, 1), (2, 2), (3, 5), (6, 4), (9, 10)]:
            Hc, Wc = CC.chroma_size(H, W, fmt)
            assert (CC.upsample16(np.ones((1, Hc, Wc), np.int64), H, W, fmt, up, siting) == 16).all()
            big = CC.upsample16(np.full((1, Hc, Wc), 1023, np.int64), H, W, fmt, up, siting)
            assert big.max() == 16 * 1023


# -- 3. siting is what it claims -----------------------------------------------------------------------------------------------------

def test_a_ramp_lands_where_the_siting_says():
    c0, Hc, Wc = 100, 6, 9
    H, W = 2 * Hc, 2 * Wc
    q = np.arange(2, W - 2)                                      # interior: no tap is clamped
    ramp_x = np.broadcast_to(c0 + 4 * np.arange(Wc), (1, Hc, Wc)).astype(np.int64)
    ramp_y = np.broadcast_to((c0 + 4 * np.arange(Hc))[:, None], (1, Hc, Wc)).astype(np.int64)
    for fmt in ("nv12", "nv16"):
        C = ramp_x[:, :CC.chroma_size(H, W, fmt)[0]] if fmt == "nv12" else np.broadcast_to(c0 + 4 * np.arange(Wc), (1, H, Wc)).astype(np.int64)
        for siting, shift in (("left", 0), ("topleft", 0), ("centre", -16)):
            got = CC.upsample16(C, H, W, fmt, "linear", siting)
            assert (got[:, :, q] == 16 * (c0 + 2 * q) + shift).all(), (fmt, siting)
    for siting, shift in (("topleft", 0), ("left", -16), ("centre", -16)):
        got = CC.upsample16(ramp_y, H, W, "nv12", "linear", siting)
        r = np.arange(2, H - 2)
        assert (got[:, r, :] == (16 * (c0 + 2 * r) + shift)[None, :, None]).all(), siting
    # 4:2:2 has no vertical axis to site: left and topleft are one
    g = np.random.default_rng(0).integers(0, 256, (1, H, Wc))
    assert (CC.upsample16(g, H, W, "nv16", "linear", "left") == CC.upsample16(g, H, W, "nv16", "linear", "topleft")).all()
    g = np.random.default_rng(0).integers(0, 256, (1, H, W))
    for siting in CC.SITINGS:
        assert (CC.upsample16(g, H, W, "nv24", "linear", siting) == 16 * g).all()
    # the emit: u = 4 q along a row; v s = 8 j co-sited (the sample lies on luma 2j) and 8 j + 2 centred (on luma 2j + 1/2)
    p = np.broadcast_to((4.0 * np.arange(W)).astype(np.float32), (1, 3, W)).copy()
    j = np.arange(1, Wc - 1)
    h, scale = CC.axis_filter(p, 2, True, True)
    assert scale == 4 and (h[:, :, j] * np.float32(1 / scale) == 8 * j).all()
    h, scale = CC.axis_filter(p, 2, True, False)
    assert scale == 2 and (h[:, :, j] * np.float32(1 / scale) == 8 * j + 2).all()
    h, scale = CC.axis_filter(p, 2, False, True)
    assert scale == 1 and h is p
    # and vertically, through the whole emit: the same planes transposed give the transposed chroma under topleft, not under left
    pt = np.ascontiguousarray(p.transpose(0, 2, 1))
    h, scale = CC.axis_filter(pt, 1, True, True)
    assert scale == 4 and (h[:, j, :] * np.float32(0.25) == 8 * j[None, :, None]).all()


# -- 4. luma round trip --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", sorted(CC.FORMATS))
def test_gray_frames_return_every_nominal_luma_code(fmt):
    for matrix, rng, up, siting in itertools.product(CC.MATRICES, CC.RANGES, CC.UPSAMPLES, CC.SITINGS):
        yo, ys, co, cs, mx = CC.levels(fmt, rng)
        lo, hi = (yo, yo + ys) if rng == "limited" else (0, mx)
        vals = np.arange(lo, hi + 1)
        side = int(np.ceil(np.sqrt(vals.size)))
        Y = np.resize(vals, (1, side, side + 1))                                  # every code, odd width: a clamped chroma column too
        Hc, Wc = CC.chroma_size(side, side + 1, fmt)
        f = CC.frame(Y, np.full((1, Hc, Wc), co), np.full((1, Hc, Wc), co), fmt)
        x = CC.ingest(f, fmt, matrix, rng, up, siting, 64, 64, 3, 7)
        assert (x[0, 0] == x[0, 1]).all() and (x[0, 1] == x[0, 2]).all()          # no chroma: R = G = B = y'
        back = CC.emit_codes(x, 3, 7, side, side + 1, fmt, matrix, rng, siting)
        assert (back[0] == Y).all(), (matrix, rng, up, siting)


# -- 5. and 6. chroma round trips ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FULL_RES)
def test_444_round_trip_is_exact(fmt):
    """no resampling at 4:4:4: a frame that came out of the emit (in-gamut RGB, so no clamp acts) goes through ingest and emit
    unchanged, whatever the siting and the upsampler say"""
    H, W, hp, wp, top, left = 37, 53, 64, 64, 13, 5
    for n, (matrix, rng) in enumerate(itertools.product(CC.MATRICES, CC.RANGES)):
        x0 = np.random.default_rng(n).uniform(0.2, 0.8, (2, 3, hp, wp)).astype(np.float32)
        f = CC.emit(x0, top, left, H, W, fmt, matrix, rng, "centre")
        for siting, up in itertools.product(CC.SITINGS, CC.UPSAMPLES):
            x = CC.ingest(f, fmt, matrix, rng, up, siting, hp, wp, top, left)
            assert same_frames(CC.emit(x, top, left, H, W, fmt, matrix, rng, siting), f), (matrix, rng, siting, up)
            assert CC.sums(x, top, left, H, W, fmt, matrix, rng, siting, f) == [[0, 0, 0]] * 2


@pytest.mark.parametrize("fmt", SUBSAMPLED)
def test_flat_chroma_round_trip_is_exact(fmt):
    """chroma constant over a frame survives any of the filters: nearest replication in, a mean of equal values out"""
    H, W, hp, wp, top, left = 37, 53, 64, 64, 13, 5
    s = 2 ** (CC.bits(fmt) - 8)
    for n, (matrix, rng, siting) in enumerate(itertools.product(CC.MATRICES, CC.RANGES, CC.SITINGS)):
        g = np.random.default_rng(n)
        yo, ys, co, cs, mx = CC.levels(fmt, rng)
        Hc, Wc = CC.chroma_size(H, W, fmt)
        Y = g.integers(yo + 3 * ys // 10, yo + 7 * ys // 10, (2, H, W))
        cb, cr = g.integers(co - 20 * s, co + 20 * s, (2, 2, 1, 1))
        f0 = CC.frame(Y, np.broadcast_to(cb, (2, Hc, Wc)), np.broadcast_to(cr, (2, Hc, Wc)), fmt)
        f = CC.emit(CC.ingest(f0, fmt, matrix, rng, "nearest", siting, hp, wp, top, left), top, left, H, W, fmt, matrix, rng, siting)
        _, fb, fr = CC.codes(f, fmt)
        assert (fb == fb[:, :1, :1]).all() and (fr == fr[:, :1, :1]).all()
        x = CC.ingest(f, fmt, matrix, rng, "nearest", siting, hp, wp, top, left)
        win = x[:, :, top:top + H, left:left + W]
        assert win.min() > 0 and win.max() < 1                                    # in gamut: no clamp acts
        assert same_frames(CC.emit(x, top, left, H, W, fmt, matrix, rng, siting), f), (matrix, rng, siting)


# -- 7. the restatement against float64 ----------------------------------------------------------------------------------------------

def ideal_rgb(planes, fmt, matrix, rng, upsample, siting):
    yo, ys, co, cs, _ = CC.levels(fmt, rng)
    a, b, c, d = CC.coefficients64(matrix)[:4]
    Y, Cb, Cr = CC.codes(planes, fmt)
    H, W = Y.shape[1:]
    y = (Y - yo) / float(ys)
    cb = (CC.upsample16(Cb, H, W, fmt, upsample, siting) - 16 * co) / (16.0 * cs)
    cr = (CC.upsample16(Cr, H, W, fmt, upsample, siting) - 16 * co) / (16.0 * cs)
    return np.clip(np.stack([y + cr * a, y - cb * b - cr * c, y + cb * d], axis=1), 0.0, 1.0)


def ideal_filter(p, axis, subsampled, cosited):
    if not subsampled:
        return p
    N = p.shape[axis]
    j = np.arange(-(-N // 2))
    b, c = np.take(p, 2 * j, axis=axis), np.take(p, np.minimum(2 * j + 1, N - 1), axis=axis)
    if not cosited:
        return (b + c) / 2
    return (np.take(p, np.maximum(2 * j - 1, 0), axis=axis) + 2 * b + c) / 4


@pytest.mark.parametrize("fmt,siting", [(f, s) for f in ("nv12", "p210", "i444", "i010", "nv16", "p410") for s in CC.SITINGS])
def test_restatement_stays_within_the_rounding_bound_of_the_float64_formulas(fmt, siting):
    """Bounds, from the roundings alone (u = 2^-24; each float32 operation errs by at most u times its result, each rounded
    coefficient by u times itself; the clamp and the exact integer chroma add nothing).

    Ingest.  c16 is an exact integer for every siting (at most 16 * 1023 < 2^24), so the bound is section 13's, derived in
    tests/test_frames_host.py, with the same constants: u max(2 ym + 4 cm a, 2 ym + 4 cm d, 3 ym + 5 cm b + 4 cm c), times 1.01.

    Emit.  Luma as in section 13: <= 7u (2^n - 1) before rintf.  Chroma: each u = Cb' cs carries 5.1u cs and |u| <= cs / 2
    (tests/test_frames_host.py).  The filter is a sum of the u values with weights that add up to S = scale_h * scale_v, times
    s = 1 / S, which is exact, so the errors the inputs bring are at most 5.1u cs after the scale, for every siting.  What the sums
    add, for the co-sited [1, 2, 1] on both axes (9 terms, S = 16), the largest case:
      a row:    a + c rounds once, at most u cs (|a + c| <= cs);  b + b is exact;  their sum rounds once, at most u 2 cs
                (|h| <= 2 cs):  3u cs per h;
      a column: the three h bring 3u cs with weights 1, 2, 1: 12u cs;  ha + hc rounds at most u 4 cs;  hb + hb is exact;  the last
                sum at most u 8 cs (|v| <= 8 cs):  24u cs in all, 1.5u cs after the scale s = 1/16.
    Centre siting on an axis has one rounding where co-sited has two (12u cs / 8 = 1.5u cs for the four terms of 4:2:0: section
    13's 4 * 5.1 + 4 = 24.4 over 4 is 6.1u cs), an axis that is not subsampled has none.  So v s carries at most 5.1u cs + 1.5u cs
    = 6.6u cs, and adding co rounds once more, at most u (2^n - 1): the constant of a chroma code is 7.6 where section 13 has 7.1,
    still below the 8 the assertion uses.  Both code bounds: the half-width of rintf, 1/2, plus 8u (2^n - 1)."""
    g = np.random.default_rng(9)
    H, W, top, left = 37, 53, 13, 5
    for matrix, rng in itertools.product(CC.MATRICES, CC.RANGES):
        yo, ys, co, cs, mx = CC.levels(fmt, rng)
        a, b, c, d = CC.coefficients64(matrix)[:4]
        ym = max(mx - yo, yo) / ys
        cm = max(mx - co, co) / cs
        bound = 1.01 * U * max(2 * ym + 4 * cm * a, 2 * ym + 4 * cm * d, 3 * ym + 5 * cm * b + 4 * cm * c)
        assert bound < 8 * U * 1.3
        f = CC.random_frame(2, H, W, fmt, seed=5)
        for up in CC.UPSAMPLES:
            got = CC.rgb(f, fmt, matrix, rng, up, siting).astype(np.float64)
            err = np.abs(got - ideal_rgb(f, fmt, matrix, rng, up, siting)).max()
            assert err <= bound, (up, err, bound)
        x = g.uniform(-0.1, 1.1, (2, 3, 64, 64)).astype(np.float32)
        kr, kg, kb, ib, ir = CC.coefficients64(matrix)[4:]
        cl = np.clip(x[:, :, top:top + H, left:left + W].astype(np.float64), 0, 1)
        Yf = kr * cl[:, 0] + kg * cl[:, 1] + kb * cl[:, 2]
        ideal = [Yf * ys + yo]
        sx, sy = CC.sub(fmt)
        hco, vco = CC.SITINGS[siting]
        for Cp in ((cl[:, 2] - Yf) * ib, (cl[:, 0] - Yf) * ir):
            ideal.append(ideal_filter(ideal_filter(Cp * cs, 2, sx == 2, hco), 1, sy == 2, vco) + co)
        for p, (got, want) in enumerate(zip(CC.emit_codes(x, top, left, H, W, fmt, matrix, rng, siting), ideal)):
            assert got.shape == want.shape
            err = np.abs(got - np.clip(want, 0, mx)).max()
            print(f"{fmt} {siting} {matrix} {rng} plane {p}: |code - float64| <= {err:.6f}")
            assert err <= 0.5 + 8 * U * mx


# -- 8. the bits of a 16-bit word outside the code -----------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [f for f in sorted(CC.FORMATS) if CC.bits(f) == 10])
def test_bits_outside_the_code_are_ignored_on_input_and_zero_on_output(fmt):
    H, W = 9, 11
    sh = CC.FORMATS[fmt][2]
    clean, dirty = CC.random_frame(2, H, W, fmt, seed=4), CC.random_frame(2, H, W, fmt, seed=4, garbage=True)
    assert not same_frames(clean, dirty) and all((a == b).all() for a, b in zip(CC.codes(clean, fmt), CC.codes(dirty, fmt)))
    assert all(p.dtype == np.uint16 for p in clean) and all((p & ~np.uint16(1023 << sh) == 0).all() for p in clean)
    for siting, up in itertools.product(CC.SITINGS, CC.UPSAMPLES):
        a = CC.ingest(clean, fmt, "bt709", "limited", up, siting, 64, 64, 1, 2)
        b = CC.ingest(dirty, fmt, "bt709", "limited", up, siting, 64, 64, 1, 2)
        assert (a.view(np.uint32) == b.view(np.uint32)).all()
        x = CC.hostile_planes(dirty, fmt, "bt709", "limited", siting, 64, 64, 1, 2, seed=1)
        out = CC.emit(x, 1, 2, H, W, fmt, "bt709", "limited", siting)
        assert all(p.dtype == np.uint16 and (p & ~np.uint16(1023 << sh) == 0).all() for p in out)
        assert CC.sums(x, 1, 2, H, W, fmt, "bt709", "limited", siting, dirty) == CC.sums(x, 1, 2, H, W, fmt, "bt709", "limited", siting, clean)


# -- the C ABI up to the first device call -------------------------------------------------------------------------------------------

def fake_frame(chroma, fmt, H, W, base=0x7000_0000_1000, pad=0):
    from progressivecodec_amd import frames
    f_ = chroma.FORMATS[fmt]
    Hc, Wc = chroma.chroma_size(H, W, fmt)
    es = 2 if f_.bits == 10 else 1
    f = frames.Frame()
    f.y, f.y_batch, f.y_row = base, H * (W + pad), W + pad
    if f_.layout == chroma.PLANAR:
        f.u, f.u_batch, f.u_row = base + 0x100_0000 * es, Hc * (Wc + pad), Wc + pad
        f.v, f.v_batch, f.v_row = base + 0x200_0000 * es, Hc * (Wc + pad), Wc + pad
    else:
        f.u, f.u_batch, f.u_row = base + 0x100_0000 * es, Hc * (2 * Wc + pad), 2 * Wc + pad
    return f


def test_formats_sitings_and_sizes():
    chroma, L = _lib()
    assert sorted(chroma.FORMATS) == sorted(CC.FORMATS) and len(chroma.FORMATS) == 12
    for name, f in chroma.FORMATS.items():
        assert (f.layout == chroma.SEMIPLANAR, f.bits, f.shift, f.sx, f.sy) == CC.FORMATS[name]
        for H, W in [(1, 1), (2, 3), (37, 53), (64, 64)]:
            assert chroma.chroma_size(H, W, name) == CC.chroma_size(H, W, name) == (-(-H // f.sy), -(-W // f.sx))
    assert {k: (bool(h), bool(v)) for k, (h, v) in chroma.SITINGS.items()} == CC.SITINGS
    assert inspect.signature(chroma.to_model_input).parameters["siting"].default == "centre"
    assert inspect.signature(chroma.from_model_output).parameters["siting"].default == "centre"
    for B, H, W, sy in [(1, 1, 1, 1), (3, 64, 64, 2), (1, 127, 129, 1), (2, 1080, 1920, 2), (1, 2160, 3840, 1)]:
        items = -(-H // sy) * -(-W // 8)
        assert L.pc_chroma_emit_workspace_size(B, H, W, sy) == 24 * B * -(-items // 256), (B, H, W, sy)
    for bad in [(0, 4, 4, 1), (1, 0, 4, 2), (1, 4, 0, 1), (-1, 4, 4, 2), (1, 4, 4, 0), (1, 4, 4, 3), (1, 2 ** 31 - 1, 2 ** 31 - 1, 1)]:
        assert L.pc_chroma_emit_workspace_size(*bad) == 0, bad


def test_plan_is_host_only_and_each_precondition_is_broken_alone():
    """made-up pointer values: nothing may be dereferenced or launched (there is no GPU here); pc_frames_plan's rule for every format"""
    chroma, L = _lib()
    Fp = 0x7000_0100_0000
    H, W = 96, 160

    def plan(op, fmt, fr, f32=Fp, fs=(3 * 128 * 192, 128 * 192, 192), left=16, ref=None):
        wide = C.c_int(-1)
        f = chroma.FORMATS[fmt]
        rc = L.pc_chroma_plan(op, f.layout, f.bits, C.byref(fr) if fr is not None else None, f32, *fs, left,
                              C.byref(ref) if ref is not None else None, C.byref(wide))
        return rc, wide.value
    for fmt in sorted(chroma.FORMATS):
        f_ = chroma.FORMATS[fmt]
        es = 2 if f_.bits == 10 else 1
        ok = fake_frame(chroma, fmt, H, W)
        for op in (chroma.INGEST, chroma.EMIT):
            assert plan(op, fmt, ok) == (0, 1)
            for off in (4, 8, 12):
                assert plan(op, fmt, ok, f32=Fp + off) == (0, 0)
            for k in range(3):
                fs = [3 * 128 * 192, 128 * 192, 192]
                fs[k] += 2
                assert plan(op, fmt, ok, fs=tuple(fs)) == (0, 0)
            for nm in ["y", "u"] + (["v"] if f_.layout == chroma.PLANAR else []):
                for off in (1, 2, 3):
                    bad = fake_frame(chroma, fmt, H, W)
                    setattr(bad, nm, getattr(bad, nm) + off * es)
                    assert plan(op, fmt, bad) == (0, 0), (fmt, nm, off)
                for st in ("_batch", "_row"):
                    bad = fake_frame(chroma, fmt, H, W)
                    setattr(bad, nm + st, getattr(bad, nm + st) + 2)
                    assert plan(op, fmt, bad) == (0, 0), (fmt, nm, st)
        fs196 = (3 * 128 * 196, 128 * 196, 196)
        assert plan(chroma.INGEST, fmt, ok, fs=fs196) == (0, 0) and plan(chroma.EMIT, fmt, ok, fs=fs196) == (0, 1)
        for left in (0, 8):
            assert plan(chroma.INGEST, fmt, ok, left=left) == (0, 1)
        for left in (1, 2, 4, 12, 21):
            assert plan(chroma.INGEST, fmt, ok, left=left) == (0, 0)
        for left, w in ((4, 1), (12, 1), (1, 0), (2, 0), (6, 0), (21, 0)):
            assert plan(chroma.EMIT, fmt, ok, left=left) == (0, w)
        loose = fake_frame(chroma, fmt, H, W, pad=2)
        assert plan(chroma.EMIT, fmt, ok, ref=loose) == (0, 0) and plan(chroma.INGEST, fmt, ok, ref=loose) == (0, 1)
        assert plan(chroma.EMIT, fmt, None, ref=ok) == (0, 1) and plan(chroma.EMIT, fmt, None, ref=loose) == (0, 0)
        assert plan(chroma.EMIT, fmt, None)[0] == -1 and plan(chroma.INGEST, fmt, None, ref=ok)[0] == -1
        assert plan(2, fmt, ok)[0] == -1 and plan(-1, fmt, ok)[0] == -1 and plan(chroma.EMIT, fmt, ok, left=-4)[0] == -1
        assert plan(chroma.EMIT, fmt, ok, f32=None)[0] == -1
        nul = fake_frame(chroma, fmt, H, W)
        nul.u = None
        assert plan(chroma.EMIT, fmt, nul)[0] == -1
    ok, wide = fake_frame(chroma, "nv12", H, W), C.c_int(-1)
    for layout, bits in [(2, 8), (-1, 8), (0, 9), (1, 12), (1, 16)]:
        assert L.pc_chroma_plan(0, layout, bits, C.byref(ok), Fp, 4, 4, 4, 0, None, C.byref(wide)) == -1
    assert L.pc_chroma_plan(0, 1, 8, C.byref(ok), Fp, 4, 4, 4, 0, None, None) == -1
    assert plan(chroma.EMIT, "nv12", ok) == (0, 1) and plan(chroma.EMIT, "i420", ok)[0] == -1          # a planar frame needs its V plane


def test_every_argument_error_returns_before_the_device():
    """fake device pointers: every call below must return PC_ERR_ARG without touching them (no GPU here)"""
    chroma, L = _lib()
    Fp, Wk, S = 0x7000_0100_0000, 0x7000_0200_0000, 0x7000_0300_0000
    B, H, W, Hp, Wp, top, left = 2, 100, 150, 128, 192, 14, 21
    k = chroma.coefficients("bt709")
    for fmt in sorted(chroma.FORMATS):
        f_ = chroma.FORMATS[fmt]
        Hc, Wc = chroma.chroma_size(H, W, fmt)
        planar = f_.layout == chroma.PLANAR
        fr = lambda **kw: fake_frame(chroma, fmt, H, W, **kw)                                   # noqa: E731

        def broken(field, value):
            f = fr()
            setattr(f, field, value)
            return f
        bad_frames = [broken("y", None), broken("u", None), broken("y_row", W - 1), broken("u_row", (Wc if planar else 2 * Wc) - 1),
                      broken("y_batch", 0), broken("u_batch", 0)]
        if planar:
            bad_frames += [broken("v", None), broken("v_row", Wc - 1), broken("v_batch", 0)]
        if f_.bits == 10:
            bad_frames += [broken("y", fr().y + 1), broken("u", fr().u + 1)]                    # a 16-bit plane on an odd address
        fbads = [dict(layout=2), dict(layout=-1), dict(bits=9), dict(bits=16), dict(shift=1), dict(shift=6 if f_.bits == 8 else 4),
                 dict(sx=3), dict(sx=0), dict(sy=0), dict(sx=1, sy=2), dict(hsite=2), dict(hsite=-1), dict(vsite=2), dict(range=2),
                 dict(range=-1), dict(B=0), dict(H=0), dict(W=0), dict(top=-1), dict(left=-1), dict(top=Hp - H + 1), dict(left=Wp - W + 1)]
        ok = dict(src=fr(), layout=f_.layout, bits=f_.bits, shift=f_.shift, sx=f_.sx, sy=f_.sy, hsite=1, vsite=1, range=0, up=1, a=k.a,
                  b=k.b, c=k.c, d=k.d, B=B, H=H, W=W, dst=Fp, Hp=Hp, Wp=Wp, top=top, left=left, stream=None)
        bads = [dict(src=f) for f in bad_frames] + fbads + [
            dict(up=2), dict(up=-1), dict(H=-5), dict(dst=None), dict(dst=Fp + 2), dict(Hp=H + top - 1), dict(Wp=W + left - 1),
            dict(H=2 ** 31 - 1, W=2 ** 31 - 1, Hp=2 ** 31 - 1, Wp=2 ** 31 - 1, top=0, left=0)]
        for bad in bads:
            a = dict(ok, **bad)
            src = a.pop("src")
            assert L.pc_chroma_ingest(C.byref(src), *a.values()) == -1, (fmt, bad)
        assert L.pc_chroma_ingest(None, *list(ok.values())[1:]) == -1

        nbytes = L.pc_chroma_emit_workspace_size(B, H, W, f_.sy)
        assert nbytes > 0
        eok = dict(x=Fp, sxb=3 * Hp * Wp, sxc=Hp * Wp, sxh=Wp, Hp=Hp, Wp=Wp, top=top, left=left, B=B, H=H, W=W, layout=f_.layout,
                   bits=f_.bits, shift=f_.shift, sx=f_.sx, sy=f_.sy, hsite=1, vsite=0, range=0, kr=k.kr, kg=k.kg, kb=k.kb, ib=k.ib, ir=k.ir,
                   dst=fr(base=0x7100_0000_0000), ref=fr(), ws=Wk, nbytes=nbytes, sse=S, stream=None)
        short_y = broken("y_batch", (H - 1) * W + W - 1)                 # a destination must also be nested; a reference need not
        ebads = [dict(dst=f) for f in bad_frames + [short_y]] + [dict(ref=f) for f in bad_frames] + fbads + [
            dict(x=None), dict(x=Fp + 1), dict(sxh=Wp - 1), dict(sxc=0), dict(sxb=0), dict(dst=None, ref=None),
            dict(ws=None), dict(ws=Wk + 4), dict(sse=None), dict(sse=S + 4), dict(nbytes=nbytes - 1), dict(nbytes=0),
            dict(H=2 ** 31 - 1, W=2 ** 31 - 1, Hp=2 ** 31 - 1, Wp=2 ** 31 - 1, sxh=2 ** 31 - 1, top=0, left=0, nbytes=10 ** 12)]
        from progressivecodec_amd import frames
        for bad in ebads:
            a = dict(eok, **bad)
            args = [C.byref(v) if isinstance(v, frames.Frame) else v for v in a.values()]
            assert L.pc_chroma_emit(*args) == -1, (fmt, bad)
    assert L.pc_chroma_last_hip_error() == 0


def test_python_rejects_before_any_device_call(monkeypatch):
    from progressivecodec_amd import chroma, pixels

    def touched(*a, **k):
        raise AssertionError("the device was reached")
    for name in ("device", "current_stream", "synchronize", "current_device", "_lazy_init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.setattr(chroma, "lib", touched)
    y, uv, u = torch.zeros(6, 10, dtype=torch.uint8), torch.zeros(6, 5, 2, dtype=torch.uint8), torch.zeros(6, 10, dtype=torch.uint8)
    for planes, fmt in [((y, uv), "nv16"), ((y, u, u), "i444"), ((y.to(torch.uint16), uv.to(torch.uint16)), "p210"),
                        ((y.to(torch.uint16), u.to(torch.uint16), u.to(torch.uint16)), "i410")]:
        with pytest.raises(ValueError, match="GPU"):
            chroma.to_model_input(planes, fmt, siting="left")
    with pytest.raises(ValueError, match="fmt"):
        chroma.to_model_input((y, uv), "nv21")
    with pytest.raises(ValueError, match="siting"):
        chroma.to_model_input((y, uv), "nv16", siting="top")
    with pytest.raises(ValueError, match="matrix"):
        chroma.to_model_input((y, uv), "nv16", matrix="bt470")
    with pytest.raises(ValueError, match="range"):
        chroma.to_model_input((y, uv), "nv16", range="tv")
    with pytest.raises(ValueError, match="upsample"):
        chroma.to_model_input((y, uv), "nv16", upsample="cubic")
    with pytest.raises(ValueError, match="2 planes"):
        chroma.to_model_input((y, u, u), "nv24")
    with pytest.raises(ValueError, match="3 planes"):
        chroma.to_model_input((y, uv), "i422")
    with pytest.raises(TypeError, match="uint16"):
        chroma.to_model_input((y, uv), "p210")
    with pytest.raises(TypeError, match="uint8"):
        chroma.to_model_input((y.to(torch.uint16), uv), "nv16")
    with pytest.raises(ValueError, match="UV must be"):
        chroma.to_model_input((y, uv), "nv12")                                               # 4:2:2 chroma for a 4:2:0 name
    with pytest.raises(ValueError, match="U must be"):
        chroma.to_model_input((y, u[:, :5], u), "i444")
    geom = pixels.padding(6, 10)
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match="GPU"):
        chroma.from_model_output(x, geom, "nv16", siting="topleft")
    with pytest.raises(ValueError, match="image=False"):
        chroma.from_model_output(x, geom, "nv16", image=False)
    with pytest.raises(ValueError, match="siting"):
        chroma.from_model_output(x, geom, "nv16", siting="right")
    with pytest.raises(ValueError, match="ref: UV must be"):
        chroma.from_model_output(x, geom, "nv16", ref=(y, uv[:3]))
    with pytest.raises(ValueError, match="ref must be on a GPU"):
        chroma.from_model_output(x, geom, "nv16", ref=(y, uv))
    with pytest.raises(ValueError, match="GPU"):
        chroma.encode_frame(None, (y, uv), [0, 1], "nv16", siting="left")
    d = chroma.Distortion(torch.tensor([[0, 4, 255 * 255 * 30]]), 6, 10, "nv16")
    assert d.psnr_y() == [float("inf")] and abs(d.psnr_cb()[0] - CC.psnr(4, 30, 255)) < 1e-12 and d.psnr_cr() == [0.0]
    assert chroma.Distortion(torch.tensor([[0, 1023 ** 2 * 60, 0]]), 6, 10, "p410").psnr_cb() == [0.0]


# -- 9. PCH1 -------------------------------------------------------------------------------------------------------------------------

def test_pch1_round_trip():
    from progressivecodec_amd import chroma, container, frames
    params = itertools.product(sorted(chroma.FORMATS), chroma.SITINGS, CC.MATRICES, CC.RANGES, CC.UPSAMPLES)
    inners = {s: pcb1(*s) for s in [(100, 150), (1, 1), (64, 64), (2160, 3840)]}
    for (fmt, siting, matrix, rng, up), (H, W) in zip(params, itertools.cycle(inners)):
        inner = inners[(H, W)]
        buf = chroma.pack_frame(inner, fmt, matrix, rng, up, siting, H, W)
        f, (hs, vs) = chroma.FORMATS[fmt], chroma.SITINGS[siting]
        assert buf[:4] == b"PCH1" and buf[4] == 1 and len(buf) == 23 + len(inner) == chroma.HEADER_BYTES + len(inner)
        assert tuple(buf[5:11]) == (f.layout, f.shift, f.sx, f.sy, hs, vs) and buf[14] == f.bits == CC.bits(fmt)
        assert buf[23:] == inner and struct.unpack_from("<II", buf, 15) == (H, W)
        hd = chroma.parse_frame(buf)
        assert (hd["fmt"], hd["siting"], hd["matrix"], hd["range"], hd["upsample"], hd["bits"], hd["H"], hd["W"]) == \
            (fmt, siting, matrix, rng, up, f.bits, H, W)
        assert hd["blob"] == inner and hd["pcb1"] == container.parse_header(inner)
        assert chroma.parse_frame(bytearray(buf))["blob"] == inner and chroma.parse_frame(memoryview(buf))["W"] == W
    with pytest.raises(container.ContainerError, match="holds a 64x64"):
        chroma.pack_frame(blob(64, 1), "nv16", "bt709", "limited", "linear", "left", 64, 63)
    with pytest.raises(ValueError, match="fmt"):
        chroma.pack_frame(blob(64, 1), "nv21", "bt709", "limited", "linear", "left", 64, 64)
    with pytest.raises(ValueError, match="siting"):
        chroma.pack_frame(blob(64, 1), "nv16", "bt709", "limited", "linear", "bottom", 64, 64)
    # PCF1 and PCH1 do not read each other
    pcf = frames.pack_frame(inners[(64, 64)], "nv12", "bt709", "limited", "linear", 64, 64)
    with pytest.raises(container.ContainerError, match="not a PCH1"):
        chroma.parse_frame(pcf)
    with pytest.raises(container.ContainerError, match="not a PCF1"):
        frames.parse_frame(chroma.pack_frame(inners[(64, 64)], "nv12", "bt709", "limited", "linear", "centre", 64, 64))
    assert frames.MAGIC == b"PCF1" and frames.HEADER_BYTES == 18


def test_pch1_every_malformed_header_raises_before_the_model(monkeypatch):
    from progressivecodec_amd import chroma, container
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    inner = pcb1(100, 150)
    buf = chroma.pack_frame(inner, "p210", "bt2020", "limited", "linear", "left", 100, 150)
    # offsets: 4 version, 5 layout, 6 shift, 7 sx, 8 sy, 9 hsite, 10 vsite, 11 matrix, 12 range, 13 upsample, 14 bits, 15 H, 19 W
    assert tuple(buf[4:15]) == (1, 1, 6, 2, 1, 1, 0, 2, 0, 1, 10)

    def patched(off, fmt, *vals):
        b = bytearray(buf)
        struct.pack_into(fmt, b, off, *vals)
        return bytes(b)
    cases = [(b"PCH2" + buf[4:], "not a PCH1"), (b"PCF1" + buf[4:], "not a PCH1"), (b"PCB1" + buf[4:], "not a PCH1"), (inner, "not a PCH1"),
             (b"", "not a PCH1"), (b"PCH", "not a PCH1"), (patched(4, "B", 2), "version"), (patched(4, "B", 0), "version"),
             (patched(5, "B", 2), "corrupt"), (patched(5, "B", 0), "corrupt"),                   # planar with shift 6 is none of the twelve
             (patched(6, "B", 0), "corrupt"), (patched(6, "B", 4), "corrupt"), (patched(7, "B", 0), "corrupt"), (patched(7, "B", 4), "corrupt"),
             (patched(8, "B", 0), "corrupt"), (patched(8, "B", 3), "corrupt"), (patched(9, "B", 2), "corrupt"),
             (patched(9, "BB", 0, 1), "corrupt"),                                               # (centre, co-sited) is no siting
             (patched(10, "B", 7), "corrupt"), (patched(11, "B", 3), "corrupt"), (patched(12, "B", 2), "corrupt"), (patched(13, "B", 2), "corrupt"),
             (patched(14, "B", 8), "corrupt"), (patched(14, "B", 12), "bits"), (patched(14, "B", 0), "bits"),
             (patched(15, "I", 0), "size"), (patched(19, "I", 0), "size"), (patched(15, "I", 101), "PCB1 blob 100x150"),
             (patched(19, "I", 2 ** 32 - 1), "PCB1 blob"), (buf[:23], "does not parse"), (buf[:23] + b"PCB2" + buf[27:], "does not parse"),
             (buf[:45], "does not parse")]
    for n in range(4, 23):
        cases.append((buf[:n], "truncated"))
    for bad, msg in cases:
        with pytest.raises(container.ContainerError, match=msg):
            chroma.parse_frame(bad)
        with pytest.raises(container.ContainerError, match=msg):
            chroma.decode_frame(None, bad)
    for level in (2, -3):
        with pytest.raises(container.ContainerError, match="no level"):
            chroma.decode_frame(None, buf, level=level)
    wrong = container.pack([[[[b"x"]] * 10, [b"z"]]], (1, 1), [0], image_size=(100, 150), contract=1)
    with pytest.raises(container.ContainerError, match="shape"):
        chroma.decode_frame(None, chroma.pack_frame(wrong, "nv16", "bt709", "limited", "linear", "left", 100, 150))
    with pytest.raises(ValueError, match="fmt"):
        chroma.decode_frame(None, buf, fmt="nv21")
    with pytest.raises(ValueError, match="siting"):
        chroma.decode_frame(None, buf, siting="middle")


# -- 10. structure -------------------------------------------------------------------------------------------------------------------

def test_the_twelfth_library_keeps_the_rules_of_the_eleven():
    chroma, L = _lib()
    hdr = open(os.path.join(DIR, "pc_chroma.h")).read()
    declared = re.findall(r"PC_API\s+[\w\s\*]+?\b(pc_\w+)\s*\(", hdr)
    assert len(declared) == 6 and sorted(declared) == sorted(chroma.EXPORTS)
    for name in declared:
        getattr(L, name)
    assert L.pc_chroma_strerror(-1).decode() and L.pc_chroma_strerror(-6).decode() and L.pc_chroma_last_hip_error() == 0
    assert chroma.LIB_PATH == os.path.join(PKG, "libpc_chroma.so")
    assert issubclass(chroma.ChromaError, chroma._imagelib.ImageLibError)
    # its Makefile is its name and the shared rule, which is the rule of the eleven, unchanged
    mk = image_shared.uncommented(os.path.join(DIR, "Makefile"))
    assert mk == "NAME := chroma\ninclude ../image_csrc/lib.mk\n"
    rule = image_shared.build_rule("frames")
    assert "-ffp-contract=off" in rule and not re.search(r"-lpc|libpc(?!_\$\(NAME\)\.so)", rule)
    top = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\bchroma\b", top, re.M) and re.search(r"^\.PHONY:.*\bchroma\b", top, re.M)
    assert "$(MAKE) -C ../chroma_hip clean" in top and re.search(r"^chroma:\n\t\$\(MAKE\) -C \.\./chroma_hip$", top, re.M)
    # the directory holds the Makefile, the header and one source; it is not one of the *_csrc the structure tests of the ten count
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(DIR, "*")) if not p.endswith((".o", ".so")))
    assert names == ["Makefile", "pc_chroma.h", "pc_chroma.hip"]
    assert len(glob.glob(os.path.join(PKG, "*_csrc", "*.hip"))) == len(image_shared.LIBS) == 10
    # the source reaches the shared names through the host header and restates none of them
    src = open(os.path.join(DIR, "pc_chroma.hip")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert '#include "pc_image_host.h"' in src
    for name, pattern in DEFINITIONS.items():
        assert not re.search(pattern, code), name
    shared = ("HIPCHK", "g_last_hip", "Planes", "load4", "store4", "store8", "Levels", "IngestCoef", "EmitCoef",
              "emit_px", "clampi", "block_reduce", "gather_partials", "plane_wide", "f32_wide", "upsample_ok", "cdiv", "F32",
              "ingest_item", "Taps", "taps_of", "code_of", "word_of", "Fmt", "format_of", "with_format", "site_ok", "depth_levels")
    for name in shared:
        assert re.search(r"\b%s\b" % name, code), name
        assert not re.search(r"\b(struct|void|int|bool|unsigned|float|define)\s+%s\b\s*[({]" % name, code), name
    # the frame is the one record of image_csrc/pc_yuv_frame.h, the enum names that mean the same alias the shared values, and the
    # shared header has gained no value
    image_shared.assert_frame_is_shared(hdr, "pc_ch_frame")
    found = dict(re.findall(r"\b(PC_CH_(?:LIMITED|FULL|NEAREST|LINEAR)) = (\w+)", hdr))
    assert found == {"PC_CH_" + k: "PC_YUV_" + k for k in ("LIMITED", "FULL", "NEAREST", "LINEAR")}
    assert "PC_YUV_" not in re.sub(r"PC_YUV_(LIMITED|FULL|NEAREST|LINEAR|NV12|P010)\b", "", hdr + code)
    values = dict((k, int(v)) for k, v in re.findall(r"\b(PC_CH_\w+) = (\d+)", hdr))
    assert values == {"PC_CH_PLANAR": chroma.PLANAR, "PC_CH_SEMIPLANAR": chroma.SEMIPLANAR, "PC_CH_CENTRE": chroma.CENTRE,
                      "PC_CH_COSITED": chroma.COSITED, "PC_CH_INGEST": chroma.INGEST, "PC_CH_EMIT": chroma.EMIT}
    # plain C++ kernels: no atomics, no inline assembly; LDS only inside the shared reduction
    assert not re.search(r"\batomic(Add|CAS|Exch|Max|Min|Or|And)\b|\basm\b|__asm|__shared__|__syncthreads|__builtin_amdgcn", code)
    # a library of its own: the codec's source hash does not cover it
    import bench
    assert "chroma" not in inspect.getsource(bench.source_hash) and "_hip" not in inspect.getsource(bench.source_hash)


# -- 11. the case table of the GPU matrices and the ledger of instantiations ---------------------------------------------------------

def old_loops(fmt, matrix, rng, sizes):
    """the loops tests/test_gpu_chroma.py's run_matrix had before it read tests/chroma_cases.py, restated once: per position
    (siting, size, left, offset, mode, float variant, the ingest's destination offset, [(with image, with reference)])"""
    out = []
    for n, (siting, (H, W)) in enumerate(itertools.product(CC.SITINGS, sizes)):
        left0 = K.geometry(H, W)[3]
        narrow = n % 2 == 0
        left, offset, mode, variant = (left0, 1 + n % 3, "loose", "odd") if narrow else (left0 // 8 * 8, 0, "pad4", ("contiguous", "loose4")[n % 4 // 2])
        emits = [(True, True)] + ([(False, True), (True, False)] if (H, W) == (37, 53) else [])
        out.append(CS.Case(fmt, matrix, rng, siting, H, W, n, left, offset, mode, variant, int(narrow), ("nearest", "linear"), tuple(emits)))
    return out


def old_cases():
    sizes = [(1, 1), (2, 3), (3, 2), (37, 53), (64, 64), (67, 130)]
    out = [c for fmt in sorted(CC.FORMATS) for c in old_loops(fmt, "bt709", "limited", sizes)]
    for fmt in ["nv16", "p210", "i444"]:
        for matrix, rng in [("bt601", "full"), ("bt2020", "limited"), ("bt2020", "full"), ("bt709", "full"), ("bt601", "limited")]:
            out += old_loops(fmt, matrix, rng, [(37, 53), (3, 2)])
    return out


def names(tuples):
    return sorted("u%d %s %d:%d%s %s%s" % (8 * t[0], "semi" if t[1] else "planar", t[2], t[3], " vco" if len(t) == 7 and t[4] else "",
                                           "wide" if t[-2 if len(t) == 7 else -1] else "narrow", (" ref" if t[-1] else " image") if len(t) == 7 else "")
                  for t in tuples)


def test_the_table_runs_at_least_what_the_loops_ran():
    table, old = CS.table(), old_cases()
    assert len(old) == 12 * 18 + 3 * 5 * 6 and set(old) <= set(table) and len(set(table)) == len(table)
    assert set(CC.UPSAMPLES) == {"nearest", "linear"}
    added = [c for c in table if c not in set(old)]
    assert len(added) == 12 * 4 and all(c.emits == ((True, False),) and not c.ups and not CS.emit_wide(c) for c in added)
    assert {(c.fmt, c.siting, c.H, c.W) for c in added} == {(f, s, H, W) for f in CC.FORMATS for s in ("centre", "topleft") for H, W in [(37, 53), (3, 2)]}
    # positions alternate between the paths, and the rule agrees with what the loops asserted case by case: narrow at even positions
    for c in table:
        assert CS.emit_wide(c) is (c.n % 2 == 1) and (not c.ups or CS.ingest_wide(c) is (c.n % 2 == 1)), c
    # the rule itself, each precondition broken alone
    c = next(c for c in table if c.n % 2 == 1 and (c.H, c.W) == (37, 53))
    assert CS.emit_wide(c) and CS.ingest_wide(c)
    assert not CS.emit_wide(c._replace(variant="odd")) and not CS.emit_wide(c._replace(left=c.left + 2)) and CS.emit_wide(c._replace(left=c.left + 4))
    assert not CS.ingest_wide(c._replace(left=c.left + 4)) and not CS.ingest_wide(c._replace(dst_offset=1)) and not CS.ingest_wide(c._replace(offset=2))
    assert not CS.emit_wide(c, ref=(0, "loose")) and not CS.emit_wide(c, dst=(1, "pad4")) and CS.emit_wide(c, ref=(4, "pad4"))


def test_every_instantiation_is_launched():
    """pc_chroma.hip: "24 ingest kernels, 64 emit kernels".  The tuples the table reaches are exactly those; a case taken away shows
    here by the names of the kernels nothing launches any more"""
    src = open(os.path.join(DIR, "pc_chroma.hip")).read()
    assert "24 ingest kernels, 64 emit kernels" in src
    assert len(CS.ALL_INGEST) == 24 and len(CS.ALL_EMIT) == 64
    ingest, emit = CS.reached(CS.table())
    assert ingest == CS.ALL_INGEST, "never launched: %s" % names(CS.ALL_INGEST - ingest)
    assert emit == CS.ALL_EMIT, "never launched: %s" % names(CS.ALL_EMIT - emit)
    # what the loops reached before the table: every ingest kernel, and all but 13 of the emit kernels -- the narrow emit without
    # a reference ran for nv16, p210 and i444 alone
    ingest0, emit0 = CS.reached(old_cases())
    missing = CS.ALL_EMIT - emit0
    print("not launched by the loops:", names(missing))
    assert ingest0 == CS.ALL_INGEST and len(emit0) == 51 and len(missing) == 13
    assert all(not t[5] and not t[6] for t in missing) and sum(t[3] == 2 for t in missing) == 8
    assert {t for t in CS.ALL_EMIT if not t[5] and not t[6]} - missing == {(1, True, 2, 1, False, False, False), (2, True, 2, 1, False, False, False),
                                                                         (1, False, 1, 1, False, False, False)}
    # the ledger notices a case that leaves
    table = CS.table()
    less = [c for c in table if not (c.fmt == "i010" and c.siting == "topleft" and c.emits == ((True, False),))]
    assert CS.ALL_EMIT - CS.reached(less)[1] == {(2, False, 2, 2, True, False, False)}
    assert names([(2, False, 2, 2, True, False, False)]) == ["u16 planar 2:2 vco narrow image"]


def test_the_unnamed_10_bit_words():
    chroma, _ = _lib()
    named = {(f.layout, f.bits, f.shift) for f in chroma.FORMATS.values()}
    for fmt, shift in CS.UNNAMED:
        f = chroma.FORMATS[fmt]
        assert f.bits == 10 and shift in (0, 6) and (f.layout, 10, shift) not in named and (f.layout, 10, 6 - shift) in named
        fr = CC.random_frame(1, 5, 7, fmt, seed=1)
        noise = np.arange(1, 2 ** 16, 257, dtype=np.uint16)
        w = CS.reshifted(fr, fmt, shift, noise)
        assert all(((a >> shift) & 1023 == c).all() for a, c in zip(w, [p >> f.shift & 1023 for p in fr]))
        assert any((a & ~np.uint16(1023 << shift)).any() for a in w)
        assert same_frames(tuple(a & np.uint16(1023 << shift) for a in w), CS.reshifted(fr, fmt, shift))
    assert len({(chroma.FORMATS[fmt].layout, chroma.FORMATS[fmt].sx, chroma.FORMATS[fmt].sy) for fmt, _ in CS.UNNAMED}) == 6


def test_whole_pictures_have_the_partials_and_the_sums_the_cases_are_there_for():
    _, L = _lib()
    H, W, B = CS.WHOLE["H"], CS.WHOLE["W"], CS.WHOLE["B"]
    hp, wp, top, left = K.geometry(H, W)
    assert (hp, wp) == (1088, 1088) and hp * -(-wp // 8) == 578 * 256
    assert {CC.sub(f) for f, _ in CS.WHOLE_FORMATS} == {(2, 2), (2, 1)} and all(s != "centre" for _, s in CS.WHOLE_FORMATS)
    for b in (B, 3):
        assert L.pc_chroma_emit_workspace_size(b, H, W, 2) == 24 * 259 * b and L.pc_chroma_emit_workspace_size(b, H, W, 1) == 24 * 518 * b
    # the last chroma row's items are exactly the last block at 4:2:0, and lie in the last two blocks at 4:2:2
    G = -(-W // 8)
    assert (513 * G - G) // 256 == 258 and (513 * G - G) % 256 == 0 and (1026 * G - G) // 256 == 516 and -(-1026 * G // 256) == 518
    for fmt, siting in CS.WHOLE_FORMATS:
        x, zeros, closed = CS.whole_saturated(fmt, 64, 64)
        small = x[:, :, :4, :8]
        codes = CC.emit_codes(small, 0, 0, 4, 8, fmt, "bt709", "full", siting)
        t = 2 ** CC.bits(fmt) - 1
        assert [int(codes[p][p].min()) for p in range(3)] == [t, t, t] == [int(codes[p][p].max()) for p in range(3)]
        Hc, Wc = CC.chroma_size(H, W, fmt)
        assert closed == [t * t * H * W, t * t * Hc * Wc, t * t * Hc * Wc] and min(closed) > 2 ** 32
    x, zeros, closed = CS.whole_saturated("i420", hp, wp)
    assert closed == [68717119500, 17179279875, 17179279875]
    got = CC.sums(x, top, left, H, W, "i420", "bt709", "full", "left", zeros)
    assert [got[p][p] for p in range(3)] == closed


@pytest.mark.parametrize("fmt,siting", CS.WHOLE_FORMATS)
def test_whole_picture_tail_differs_in_the_last_rows_alone(fmt, siting):
    H, W, B = CS.WHOLE["H"], CS.WHOLE["W"], CS.WHOLE["B"]
    hp, wp, top, left = K.geometry(H, W)
    left = left // 4 * 4
    x, ref = CS.whole_tail(fmt, siting, "bt601", "limited", hp, wp, top, left)
    got, want = CC.emit_codes(x, top, left, H, W, fmt, "bt601", "limited", siting), CC.codes(ref, fmt)
    for p in range(3):
        assert (got[p][:, :-1] == want[p][:, :-1]).all() and (got[p][0] == want[p][0]).all()    # every sum over the rows above is zero
    sums = CC.sums(x, top, left, H, W, fmt, "bt601", "limited", siting, ref)
    assert sums[0] == [0, 0, 0] and all(v > 0 for v in sums[1])

"""The YUV 4:2:0 layer without a GPU: the restatement (tests/frames_contract.py) against the published coefficients and the float64
formulas, the round trips the contract promises, libpc_frames.so's C ABI up to the first device call, progressivecodec_amd.frames'
argument checks, and the PCF1 container up to the model."""
import ctypes as C
import itertools
import os
import re
import struct

import numpy as np
import pytest
import torch

from tests import frames_contract as FC
from tests import image_shared
from tests.test_tiles_host import blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24                                   # the unit roundoff of float32
ALL = list(itertools.product(FC.FORMATS, FC.MATRICES, FC.RANGES, FC.UPSAMPLES))


def _lib():
    from progressivecodec_amd import frames
    return frames, frames.lib()


# -- coefficients --------------------------------------------------------------------------------------------------------------------

def test_coefficients_are_the_published_ones_and_what_python_passes():
    from progressivecodec_amd import frames
    # BT.601 / BT.709 / BT.2020 as every table of them prints the YCbCr -> RGB factors (four or five decimals)
    published = {"bt601": (1.402, 0.344136, 0.714136, 1.772), "bt709": (1.5748, 0.187324, 0.468124, 1.8556),
                 "bt2020": (1.4746, 0.164553, 0.571353, 1.8814)}
    for m, (kr, kb) in FC.MATRICES.items():
        a, b, c, d, kr_, kg, kb_, ib, ir = FC.coefficients64(m)
        # Kg = 1 - Kr - Kb: two float64 roundings there and two in the sum, each at most 2^-53
        assert abs(kr + kg + kb - 1.0) <= 2.0 ** -51 and (kr_, kb_) == (kr, kb) and kg == 1.0 - kr - kb
        for got, want in zip((a, b, c, d), published[m]):
            assert abs(got - want) < 5e-7, (m, got, want)
        assert abs(ib * d - 1) < 1e-15 and abs(ir * a - 1) < 1e-15
        # white and black have no chroma: the G row reproduces y when R = G = B
        assert abs(kr * a - c * kg) < 1e-15 and abs(kb * d - b * kg) < 1e-15
        k32 = frames.coefficients(m)
        assert frames.MATRICES[m] == (kr, kb)
        for got, want, want64 in zip(k32, FC.coefficients(m), FC.coefficients64(m)):
            assert np.float32(got).view(np.uint32) == want.view(np.uint32) and float(want) == got
            assert abs(got - want64) <= abs(want64) * U
    for fmt in FC.FORMATS:
        for rng in FC.RANGES:
            assert frames.levels(fmt, rng) == FC.levels(fmt, rng)
    assert FC.levels("nv12", "limited") == (16, 219, 128, 224, 255) and FC.levels("p010", "limited") == (64, 876, 512, 896, 1023)
    assert FC.levels("i420", "full") == (0, 255, 128, 255, 255) and FC.levels("p010", "full") == (0, 1023, 512, 1023, 1023)


# -- the restatement against float64 -------------------------------------------------------------------------------------------------

def ideal_rgb(planes, fmt, matrix, rng, upsample):
    yo, ys, co, cs, _ = FC.levels(fmt, rng)
    a, b, c, d = FC.coefficients64(matrix)[:4]
    Y, Cb, Cr = FC.codes(planes, fmt)
    H, W = Y.shape[1:]
    y = (Y - yo) / float(ys)
    cb = (FC.upsample16(Cb, H, W, upsample) - 16 * co) / (16.0 * cs)
    cr = (FC.upsample16(Cr, H, W, upsample) - 16 * co) / (16.0 * cs)
    return np.clip(np.stack([y + cr * a, y - cb * b - cr * c, y + cb * d], axis=1), 0.0, 1.0)


@pytest.mark.parametrize("fmt,matrix,rng", list(itertools.product(FC.FORMATS, FC.MATRICES, FC.RANGES)))
def test_restatement_stays_within_the_rounding_bound_of_the_float64_formulas(fmt, matrix, rng):
    """Bounds, from the roundings alone (u = 2^-24; each float32 operation errs by at most u times its result, each rounded
    coefficient by u times itself; the clamp and the exact integer chroma add nothing).

    Ingest.  With ym = max |y'| and cm = max |cb'|, |cr'| over the code range: y' carries u ym; a product cr' k carries 3u cm k (the
    quotient, the coefficient, the product); a sum carries u times its size.  R = y' + cr' a:  u (ym + 3 cm a + (ym + cm a));  B
    likewise with d;  G = (y' - cb' b) - cr' c:  u (ym + 3 cm b + (ym + cm b) + 3 cm c + (ym + cm b + cm c)).  The test takes the
    largest of the three, times 1.01 for the second-order terms.

    Emit.  With R, G, B in [0, 1] and Kr + Kg + Kb = 1: Y' carries 2u (the three products, coefficient and product) + 2u (two sums
    of at most 1) = 4u; Y' ys + yo then u (4 ys + ys + (ys + yo)) <= 7u (2^n - 1).  Cb' = (B - Y') ib carries (4u + u) ib + 2u / 2
    <= 4.6u (ib, ir <= 0.7133 and |Cb'| <= 1/2); u = Cb' cs carries 5.1u cs; the three sums of four such terms, each at most
    cs / 2, carry 4 * 5.1u cs + u (cs + cs + 2 cs); a quarter of that (exact) is 6.1u cs, and adding co rounds once more:
    <= 7.1u (2^n - 1).  Both code bounds: the half-width of rintf, 1/2, plus 8u (2^n - 1)."""
    yo, ys, co, cs, mx = FC.levels(fmt, rng)
    a, b, c, d = FC.coefficients64(matrix)[:4]
    ym = max(mx - yo, yo) / ys
    cm = max(mx - co, co) / cs
    bound = 1.01 * U * max(2 * ym + 4 * cm * a, 2 * ym + 4 * cm * d, 3 * ym + 5 * cm * b + 4 * cm * c)
    assert bound < 8 * U * 1.3
    f = FC.random_frame(2, 37, 53, fmt, seed=5)
    for up in FC.UPSAMPLES:
        got = FC.rgb(f, fmt, matrix, rng, up).astype(np.float64)
        err = np.abs(got - ideal_rgb(f, fmt, matrix, rng, up)).max()
        assert err <= bound, (up, err, bound)
    # emit: the codes against the float64 values before rounding
    g = np.random.default_rng(9)
    x = g.uniform(-0.1, 1.1, (2, 3, 64, 64)).astype(np.float32)
    H, W, top, left = 37, 53, 13, 5
    kr, kg, kb, ib, ir = FC.coefficients64(matrix)[4:]
    cl = np.clip(x[:, :, top:top + H, left:left + W].astype(np.float64), 0, 1)
    Yf = kr * cl[:, 0] + kg * cl[:, 1] + kb * cl[:, 2]
    ideal = [Yf * ys + yo]
    for Cp in ((cl[:, 2] - Yf) * ib, (cl[:, 0] - Yf) * ir):
        p = np.pad(Cp * cs, ((0, 0), (0, H & 1), (0, W & 1)), mode="edge")
        ideal.append((p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2]) / 4 + co)
    for got, want in zip(FC.emit_codes(x, top, left, H, W, fmt, matrix, rng), ideal):
        assert np.abs(got - np.clip(want, 0, mx)).max() <= 0.5 + 8 * U * mx


# -- round trips ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,matrix,rng,up", ALL)
def test_gray_frames_return_every_nominal_luma_code(fmt, matrix, rng, up):
    yo, ys, co, cs, mx = FC.levels(fmt, rng)
    lo, hi = (yo, yo + ys) if rng == "limited" else (0, mx)
    vals = np.arange(lo, hi + 1)
    side = int(np.ceil(np.sqrt(vals.size)))
    Y = np.resize(vals, (1, side, side + 1))                                      # every code, odd width: a clamped chroma column too
    assert set(Y.ravel().tolist()) == set(vals.tolist())
    Hc, Wc = FC.chroma_size(side, side + 1)
    f = FC.frame(Y, np.full((1, Hc, Wc), co), np.full((1, Hc, Wc), co), fmt)
    x = FC.ingest(f, fmt, matrix, rng, up, 64, 64, 3, 7)
    assert (x[0, 0] == x[0, 1]).all() and (x[0, 1] == x[0, 2]).all()              # no chroma: R = G = B = y'
    back = FC.emit_codes(x, 3, 7, side, side + 1, fmt, matrix, rng)
    assert (back[0] == Y).all()


def test_chroma_round_trip_figures(capsys):
    """not gated: what emit(ingest(f)) does to the chroma (and luma) codes of random in-gamut 128x128 bt709 frames.  "cells": RGB in
    [0.2, 0.8], drawn per 2x2 cell, so that every chroma sample stands for four equal pixels and no pixel of f leaves the RGB cube;
    "smooth": RGB noise at 1/8 resolution, bilinearly enlarged.  Nearest repeats each sample and loses only the two roundings; linear
    blurs across cells, which the 2x2 mean does not undo."""
    g = np.random.default_rng(3)
    cells = np.repeat(np.repeat(g.uniform(0.2, 0.8, (1, 3, 64, 64)), 2, axis=2), 2, axis=3).astype(np.float32)
    lo = torch.from_numpy(g.uniform(0.1, 0.9, (1, 3, 16, 16)).astype(np.float32))
    smooth = torch.nn.functional.interpolate(lo, size=(128, 128), mode="bilinear", align_corners=False).numpy()
    lines = []
    for (name, x), fmt, rng, up in itertools.product((("cells", cells), ("smooth", smooth)), ("nv12", "p010"), FC.RANGES, FC.UPSAMPLES):
        f = FC.emit(x, 0, 0, 128, 128, fmt, "bt709", rng)
        back = FC.emit_codes(FC.ingest(f, fmt, "bt709", rng, up, 128, 128, 0, 0), 0, 0, 128, 128, fmt, "bt709", rng)
        want = FC.codes(f, fmt)
        d = np.abs(np.stack(back[1:]) - np.stack(want[1:]))
        dy = np.abs(back[0] - want[0])
        lines.append(f"  {name:6s} {fmt} {rng:7s} {up:7s}: chroma max {d.max():3d} mean {d.mean():7.4f} codes; luma max {dy.max():3d} mean {dy.mean():.4f}")
    with capsys.disabled():
        print("\nchroma round trip emit(ingest(f)):\n" + "\n".join(lines))


def test_chroma_weights_sum_to_16_and_the_taps_stay_inside():
    for n in (1, 2, 3, 4, 7):
        for r in range(2 * n - 1, 2 * n + 1):
            if r < 1:
                continue
            for q in range(r):
                i0, i1 = FC.taps(q, n)
                assert i0 == q // 2 and 0 <= i1 < n and abs(i1 - i0) <= 1
                assert i1 == i0 + (1 if q % 2 else -1) or (q == 0 and i1 == 0) or (q == r - 1 and i1 == n - 1 == i0)
    for H, W in itertools.product((1, 2, 3), repeat=2):
        Hc, Wc = FC.chroma_size(H, W)
        # a constant plane stays constant: the four weights sum to 16 at every pixel, clamped taps included
        assert (FC.upsample16(np.full((1, Hc, Wc), 7), H, W, "linear") == 16 * 7).all()
        assert (FC.upsample16(np.full((1, Hc, Wc), 7), H, W, "nearest") == 16 * 7).all()
        # each chroma sample alone: its weights over the luma grid, summed over all samples, are 16 per pixel
        tot = np.zeros((H, W), np.int64)
        for i, j in itertools.product(range(Hc), range(Wc)):
            one = np.zeros((1, Hc, Wc), np.int64)
            one[0, i, j] = 1
            w = FC.upsample16(one, H, W, "linear")[0]
            assert w.min() >= 0 and set(np.unique(w).tolist()) <= {0, 1, 3, 4, 9, 12, 16}
            tot += w
        assert (tot == 16).all()
    C4 = np.arange(6).reshape(1, 2, 3)
    up = FC.upsample16(C4, 4, 6, "linear")[0]
    assert up[0, 0] == 16 * 0 and up[1, 1] == 9 * 0 + 3 * 1 + 3 * 3 + 4 and up[2, 3] == 9 * 4 + 3 * 5 + 3 * 1 + 2 and up[3, 5] == 16 * 5


# -- the library, no device ----------------------------------------------------------------------------------------------------------

def test_library_exports_every_declared_function():
    frames, L = _lib()
    hdr = open(os.path.join(ROOT, "progressivecodec_amd", "frames_csrc", "pc_frames.h")).read()
    declared = re.findall(r"PC_API\s+[\w\s\*]+?\b(pc_\w+)\s*\(", hdr)
    assert len(declared) == 6 and sorted(declared) == sorted(frames.EXPORTS)
    for name in declared:
        getattr(L, name)
    assert L.pc_frames_strerror(-1).decode() and L.pc_frames_strerror(-6).decode() and L.pc_frames_last_hip_error() == 0
    # a library of its own: no other library of the project is linked, and the codec's source hash does not cover it
    import bench
    import inspect
    assert "frames" not in inspect.getsource(bench.source_hash)
    mk = image_shared.build_rule("frames")                                             # image_csrc/lib.mk, which the library's Makefile includes
    assert "-ffp-contract=off" in mk and not re.search(r"-lpc|libpc(odec|_pixels|_tiles|_rate|_metrics)", mk)


def fake_frame(frames, fmt, H, W, base=0x7000_0000_1000, pad=0):
    Hc, Wc = FC.chroma_size(H, W)
    es = 2 if fmt == "p010" else 1
    f = frames.Frame()
    f.y, f.y_batch, f.y_row = base, H * (W + pad), W + pad
    if fmt == "i420":
        f.u, f.u_batch, f.u_row = base + 0x100_0000, Hc * (Wc + pad), Wc + pad
        f.v, f.v_batch, f.v_row = base + 0x200_0000, Hc * (Wc + pad), Wc + pad
    else:
        f.u, f.u_batch, f.u_row = base + 0x100_0000 * es, Hc * (2 * Wc + pad), 2 * Wc + pad
    return f


def test_workspace_size():
    _, L = _lib()
    for B, H, W in [(1, 1, 1), (3, 64, 64), (1, 127, 129), (2, 1080, 1920), (1, 2160, 3840)]:
        items = -(-H // 2) * -(-W // 8)
        assert L.pc_frames_emit_workspace_size(B, H, W) == 24 * B * -(-items // 256), (B, H, W)
    for bad in [(0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, 2 ** 31 - 1, 2 ** 31 - 1)]:
        assert L.pc_frames_emit_workspace_size(*bad) == 0, bad


def test_plan_is_host_only_and_each_precondition_is_broken_alone():
    """made-up pointer values: nothing may be dereferenced or launched (there is no GPU here)"""
    frames, L = _lib()
    Fp = 0x7000_0100_0000
    H, W = 96, 160

    def plan(op, fmt, fr, f32=Fp, fs=(3 * 128 * 192, 128 * 192, 192), left=16, ref=None):
        wide = C.c_int(-1)
        rc = L.pc_frames_plan(op, frames.FORMATS[fmt], C.byref(fr) if fr is not None else None, f32, *fs, left,
                              C.byref(ref) if ref is not None else None, C.byref(wide))
        return rc, wide.value
    for fmt in FC.FORMATS:
        es = 2 if fmt == "p010" else 1
        ok = fake_frame(frames, fmt, H, W)
        for op in (frames.INGEST, frames.EMIT):
            assert plan(op, fmt, ok) == (0, 1)
            for off in (4, 8, 12):
                assert plan(op, fmt, ok, f32=Fp + off) == (0, 0)                               # the floats: 16-byte aligned
            for k in range(3):
                fs = [3 * 128 * 192, 128 * 192, 192]
                fs[k] += 2
                assert plan(op, fmt, ok, fs=tuple(fs)) == (0, 0)                               # their strides: multiples of 4
            names = ["y", "u"] + (["v"] if fmt == "i420" else [])
            for nm in names:
                for off in (1, 2, 3):
                    bad = fake_frame(frames, fmt, H, W)
                    setattr(bad, nm, getattr(bad, nm) + off * es)                              # each plane: aligned to four elements
                    assert plan(op, fmt, bad) == (0, 0), (fmt, nm, off)
                for st in ("_batch", "_row"):
                    bad = fake_frame(frames, fmt, H, W)
                    setattr(bad, nm + st, getattr(bad, nm + st) + 2)                           # each stride: a multiple of 4
                    assert plan(op, fmt, bad) == (0, 0), (fmt, nm, st)
        assert plan(frames.INGEST, fmt, ok, left=8) == (0, 1) and plan(frames.INGEST, fmt, ok, left=0) == (0, 1)
        fs196 = (3 * 128 * 196, 128 * 196, 196)                                                 # Wp a multiple of 4, not of 8
        assert plan(frames.INGEST, fmt, ok, fs=fs196) == (0, 0) and plan(frames.EMIT, fmt, ok, fs=fs196) == (0, 1)
        for left in (1, 2, 4, 12, 21):
            assert plan(frames.INGEST, fmt, ok, left=left) == (0, 0)                           # ingest: left a multiple of 8
        assert plan(frames.EMIT, fmt, ok, left=4) == (0, 1) and plan(frames.EMIT, fmt, ok, left=12) == (0, 1)
        for left in (1, 2, 6, 21):
            assert plan(frames.EMIT, fmt, ok, left=left) == (0, 0)                             # emit: a multiple of 4
        # the reference frame counts for the emit alone; the destination may be absent there
        loose = fake_frame(frames, fmt, H, W, pad=2)
        assert plan(frames.EMIT, fmt, ok, ref=loose) == (0, 0) and plan(frames.INGEST, fmt, ok, ref=loose) == (0, 1)
        assert plan(frames.EMIT, fmt, None, ref=ok) == (0, 1) and plan(frames.EMIT, fmt, None, ref=loose) == (0, 0)
        assert plan(frames.EMIT, fmt, None)[0] == -1 and plan(frames.INGEST, fmt, None, ref=ok)[0] == -1
        assert plan(2, fmt, ok)[0] == -1 and plan(-1, fmt, ok)[0] == -1 and plan(frames.EMIT, fmt, ok, left=-4)[0] == -1
        assert plan(frames.EMIT, fmt, ok, f32=None)[0] == -1
        nul = fake_frame(frames, fmt, H, W)
        nul.u = None
        assert plan(frames.EMIT, fmt, nul)[0] == -1
        assert L.pc_frames_plan(0, frames.FORMATS[fmt], C.byref(ok), Fp, 4, 4, 4, 0, None, None) == -1
    wide = C.c_int(-1)
    assert L.pc_frames_plan(0, 3, C.byref(fake_frame(frames, "nv12", H, W)), Fp, 4, 4, 4, 0, None, C.byref(wide)) == -1
    # an I420 frame whose V pointer is missing is refused; NV12 does not look at it
    f = fake_frame(frames, "nv12", H, W)
    assert plan(frames.EMIT, "nv12", f) == (0, 1) and plan(frames.EMIT, "i420", f)[0] == -1


def test_every_argument_error_returns_before_the_device():
    """fake device pointers: every call below must return PC_ERR_ARG without touching them (no GPU here)"""
    frames, L = _lib()
    Fp, Wk, S = 0x7000_0100_0000, 0x7000_0200_0000, 0x7000_0300_0000
    B, H, W, Hp, Wp, top, left = 2, 100, 150, 128, 192, 14, 21
    k = frames.coefficients("bt709")
    for fmt in FC.FORMATS:
        fid = frames.FORMATS[fmt]
        fr = lambda **kw: fake_frame(frames, fmt, H, W, **kw)                                   # noqa: E731

        def broken(field, value):
            f = fr()
            setattr(f, field, value)
            return f
        ok = dict(src=fr(), fmt=fid, range=0, up=1, a=k.a, b=k.b, c=k.c, d=k.d, B=B, H=H, W=W, dst=Fp, Hp=Hp, Wp=Wp, top=top, left=left, stream=None)
        bad_frames = [broken("y", None), broken("u", None), broken("y_row", W - 1), broken("u_row", (150 if fmt != "i420" else 75) - 1),
                      broken("y_batch", 0), broken("u_batch", 0)]
        if fmt == "i420":
            bad_frames += [broken("v", None), broken("v_row", 74), broken("v_batch", 0)]
        if fmt == "p010":
            bad_frames += [broken("y", fr().y + 1), broken("u", fr().u + 1)]                    # a 16-bit plane on an odd address
        bads = [dict(src=f) for f in bad_frames] + [
            dict(fmt=3), dict(fmt=-1), dict(range=2), dict(range=-1), dict(up=2), dict(up=-1), dict(B=0), dict(H=0), dict(W=0), dict(H=-5),
            dict(dst=None), dict(dst=Fp + 2), dict(Hp=H + top - 1), dict(Wp=W + left - 1), dict(top=-1), dict(left=-1), dict(top=Hp - H + 1),
            dict(left=Wp - W + 1), dict(H=2 ** 31 - 1, W=2 ** 31 - 1, Hp=2 ** 31 - 1, Wp=2 ** 31 - 1, top=0, left=0)]
        for bad in bads:
            a = dict(ok, **bad)
            src = a.pop("src")
            assert L.pc_frames_ingest(C.byref(src), *a.values()) == -1, (fmt, bad)
        assert L.pc_frames_ingest(None, *list(ok.values())[1:]) == -1

        nbytes = L.pc_frames_emit_workspace_size(B, H, W)
        eok = dict(x=Fp, sxb=3 * Hp * Wp, sxc=Hp * Wp, sxh=Wp, Hp=Hp, Wp=Wp, top=top, left=left, B=B, H=H, W=W, fmt=fid, range=0, kr=k.kr,
                   kg=k.kg, kb=k.kb, ib=k.ib, ir=k.ir, dst=fr(base=0x7100_0000_0000), ref=fr(), ws=Wk, nbytes=nbytes, sse=S, stream=None)
        # a destination must also be nested: a batch stride shorter than one picture's rows is refused for dst, not for ref
        short_y = broken("y_batch", (H - 1) * W + W - 1)
        ebads = [dict(dst=f) for f in bad_frames + [short_y]] + [dict(ref=f) for f in bad_frames] + [
            dict(x=None), dict(x=Fp + 1), dict(sxh=Wp - 1), dict(sxc=0), dict(sxb=0), dict(fmt=3), dict(fmt=-1), dict(range=2), dict(B=0),
            dict(H=0), dict(W=0), dict(top=-1), dict(left=-1), dict(top=Hp - H + 1), dict(left=Wp - W + 1), dict(dst=None, ref=None),
            dict(ws=None), dict(ws=Wk + 4), dict(sse=None), dict(sse=S + 4), dict(nbytes=nbytes - 1), dict(nbytes=0),
            dict(H=2 ** 31 - 1, W=2 ** 31 - 1, Hp=2 ** 31 - 1, Wp=2 ** 31 - 1, sxh=2 ** 31 - 1, top=0, left=0, nbytes=10 ** 12)]
        for bad in ebads:
            a = dict(eok, **bad)
            args = [C.byref(v) if isinstance(v, frames.Frame) else v for v in a.values()]
            assert L.pc_frames_emit(*args) == -1, (fmt, bad)


def test_python_rejects_before_any_device_call(monkeypatch):
    from progressivecodec_amd import frames, pixels

    def touched(*a, **k):
        raise AssertionError("the device was reached")
    for name in ("device", "current_stream", "synchronize", "current_device", "_lazy_init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.setattr(frames, "lib", touched)
    y, uv, u = torch.zeros(6, 10, dtype=torch.uint8), torch.zeros(3, 5, 2, dtype=torch.uint8), torch.zeros(3, 5, dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU"):
        frames.to_model_input((y, uv), "nv12")
    with pytest.raises(ValueError, match="GPU"):
        frames.to_model_input((y, u, u), "i420")
    with pytest.raises(ValueError, match="GPU"):
        frames.to_model_input((y.to(torch.uint16), uv.to(torch.uint16)), "p010")
    with pytest.raises(ValueError, match="fmt"):
        frames.to_model_input((y, uv), "nv21")
    with pytest.raises(ValueError, match="matrix"):
        frames.to_model_input((y, uv), "nv12", matrix="bt470")
    with pytest.raises(ValueError, match="range"):
        frames.to_model_input((y, uv), "nv12", range="tv")
    with pytest.raises(ValueError, match="upsample"):
        frames.to_model_input((y, uv), "nv12", upsample="cubic")
    with pytest.raises(ValueError, match="2 planes"):
        frames.to_model_input((y, u, u), "nv12")
    with pytest.raises(ValueError, match="3 planes"):
        frames.to_model_input((y, uv), "i420")
    with pytest.raises(TypeError, match="uint16"):
        frames.to_model_input((y, uv), "p010")
    with pytest.raises(TypeError, match="uint8"):
        frames.to_model_input((y.float(), uv), "nv12")
    with pytest.raises(TypeError, match="tensor"):
        frames.to_model_input((y, uv.numpy()), "nv12")
    with pytest.raises(ValueError, match="UV must be"):
        frames.to_model_input((y, uv[:2]), "nv12")
    with pytest.raises(ValueError, match="U must be"):
        frames.to_model_input((y, u[:, :4], u), "i420")
    with pytest.raises(ValueError, match="V must be"):
        frames.to_model_input((y[None], u[None], u), "i420")
    with pytest.raises(ValueError, match="Y must be"):
        frames.to_model_input((y[0], uv), "nv12")
    with pytest.raises(ValueError, match="empty"):
        frames.to_model_input((y[:0], uv[:0]), "nv12")
    geom = pixels.padding(6, 10)
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match="GPU"):
        frames.from_model_output(x, geom, "nv12")
    with pytest.raises(ValueError, match="image=False"):
        frames.from_model_output(x, geom, "nv12", image=False)
    with pytest.raises(TypeError, match="float32"):
        frames.from_model_output(x.double(), geom, "nv12")
    with pytest.raises(ValueError, match="x_hat must be"):
        frames.from_model_output(x[:, :, :63], geom, "nv12")
    with pytest.raises(ValueError, match="outside"):
        frames.from_model_output(x, geom._replace(top=60), "nv12")
    with pytest.raises(ValueError, match="ref: UV must be"):
        frames.from_model_output(x, geom, "nv12", ref=(y, uv[:2]))
    with pytest.raises(ValueError, match="ref must be on a GPU"):
        frames.from_model_output(x, geom, "nv12", ref=(y, uv))
    with pytest.raises(ValueError, match="fmt"):
        frames.from_model_output(x, geom, "yuyv")
    with pytest.raises(ValueError, match="range"):
        frames.from_model_output(x, geom, "nv12", range="pc")
    with pytest.raises(ValueError, match="GPU"):
        frames.encode_frame(None, (y, uv), [0, 1], "nv12")
    d = frames.Distortion(torch.tensor([[0, 4, 255 * 255 * 15]]), 6, 10, 8)
    assert d.psnr_y() == [float("inf")] and abs(d.psnr_cb()[0] - FC.psnr(4, 15, 255)) < 1e-12 and d.psnr_cr() == [0.0]
    assert frames.Distortion(torch.tensor([[1023 ** 2 * 60, 0, 0]]), 6, 10, 10).psnr_y() == [0.0]


# -- PCF1 ----------------------------------------------------------------------------------------------------------------------------

def pcb1(H, W, qualities=(0, 0.5)):
    from progressivecodec_amd import container
    from progressivecodec_amd.pixels import padding
    g = padding(H, W)
    y = [[bytes([7, s]) * (1 + s % 3)] for s in range(20)]
    lv = [[y[:10] if q == 0 else y, [bytes([7])]] for q in qualities]
    return container.pack(lv, (g.Hp // 64, g.Wp // 64), list(qualities), image_size=(H, W), contract=1)


def test_pcf1_round_trip():
    from progressivecodec_amd import container, frames
    for (fmt, matrix, rng, up), (H, W) in zip(ALL, itertools.cycle([(100, 150), (1, 1), (64, 64), (2160, 3840)])):
        inner = pcb1(H, W)
        buf = frames.pack_frame(inner, fmt, matrix, rng, up, H, W)
        assert buf[:4] == b"PCF1" and buf[4] == 1 and len(buf) == 18 + len(inner) == frames.HEADER_BYTES + len(inner)
        assert buf[18:] == inner and struct.unpack_from("<II", buf, 10) == (H, W) and buf[9] == FC.bits(fmt)
        hd = frames.parse_frame(buf)
        assert (hd["fmt"], hd["matrix"], hd["range"], hd["upsample"], hd["bits"], hd["H"], hd["W"]) == (fmt, matrix, rng, up, FC.bits(fmt), H, W)
        assert hd["blob"] == inner and hd["pcb1"] == container.parse_header(inner)
        assert frames.parse_frame(bytearray(buf))["blob"] == inner and frames.parse_frame(memoryview(buf))["W"] == W
    with pytest.raises(container.ContainerError, match="holds a 64x64"):
        frames.pack_frame(blob(64, 1), "nv12", "bt709", "limited", "linear", 64, 63)
    with pytest.raises(ValueError, match="fmt"):
        frames.pack_frame(blob(64, 1), "nv21", "bt709", "limited", "linear", 64, 64)


def test_pcf1_every_malformed_header_raises_before_the_model(monkeypatch):
    from progressivecodec_amd import container, frames
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    inner = pcb1(100, 150)
    buf = frames.pack_frame(inner, "p010", "bt2020", "limited", "linear", 100, 150)

    def patched(off, fmt, *vals):
        b = bytearray(buf)
        struct.pack_into(fmt, b, off, *vals)
        return bytes(b)
    cases = [(b"PCF2" + buf[4:], "not a PCF1"), (b"PCB1" + buf[4:], "not a PCF1"), (inner, "not a PCF1"), (b"", "not a PCF1"), (b"PCF", "not a PCF1"),
             (patched(4, "B", 2), "version"), (patched(4, "B", 0), "version"),
             (patched(5, "B", 3), "corrupt"), (patched(6, "B", 3), "corrupt"), (patched(7, "B", 2), "corrupt"), (patched(8, "B", 2), "corrupt"),
             (patched(5, "B", 255), "corrupt"), (patched(9, "B", 8), "10|bits"), (patched(9, "B", 12), "bits"), (patched(5, "B", 0), "bits"),
             (patched(10, "I", 0), "size"), (patched(14, "I", 0), "size"), (patched(10, "I", 101), "PCB1 blob 100x150"),
             (patched(14, "I", 2 ** 32 - 1), "PCB1 blob"), (buf[:18], "does not parse"), (buf[:18] + b"PCB2" + buf[22:], "does not parse"),
             (buf[:40], "does not parse")]
    for n in range(4, 18):
        cases.append((buf[:n], "truncated"))
    for bad, msg in cases:
        with pytest.raises(container.ContainerError, match=msg):
            frames.parse_frame(bad)
        with pytest.raises(container.ContainerError, match=msg):
            frames.decode_frame(None, bad)
    # refusals that need the inner header: the level, the latent shape
    for level in (2, -3):
        with pytest.raises(container.ContainerError, match="no level"):
            frames.decode_frame(None, buf, level=level)
    wrong = container.pack([[[[b"x"]] * 10, [b"z"]]], (1, 1), [0], image_size=(100, 150), contract=1)
    with pytest.raises(container.ContainerError, match="header shape"):
        frames.decode_frame(None, frames.pack_frame(wrong, "nv12", "bt709", "full", "nearest", 100, 150))
    with pytest.raises(ValueError, match="fmt"):
        frames.decode_frame(None, buf, fmt="nv21")
    with pytest.raises(container.ContainerError, match="contract"):
        monkeypatch.setattr(container, "build_contract_id", lambda: 2)
        frames.decode_frame(None, buf)
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    # nothing above is wrong with a good container: with a model (here: none) the decode goes on to use it
    with pytest.raises(AttributeError):
        frames.decode_frame(None, buf)
    with pytest.raises(AttributeError):
        frames.decode_frame(None, buf, level=0, fmt="nv12")
    # a payload cut short still parses (the header is whole) and is refused when its level is read
    with pytest.raises(container.ContainerError, match="truncated payload"):
        frames.decode_frame(None, buf[:-1])

"""Tolerant rate-controlled clips of YUV frames of any subsampling and siting without a GPU: the restatement of DESIGN.md section 30
(tests/chroma_clip_tol_rate_contract.py) against section 20's for centre-sited 4:2:0; libpc_chroma_clip_tol_rate.so's C ABI up to the
first device call; progressivecodec_amd.chroma_clip_tol_rate's refusals; encode_clip_to_size against a fake model; the structure of
the eighteenth image-side library; the ledger of kernel instantiations; and the conditions under which the GPU tests' own inputs can
tell a right kernel from a wrong one.  Every comparison is exact equality of integers or bytes."""
import contextlib
import ctypes as C
import glob
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import chroma_clip_tol_contract as TOL
from tests import chroma_clip_tol_rate_cases as CS
from tests import chroma_clip_tol_rate_contract as TR
from tests import chroma_contract as CC
from tests import chroma_limits as CL
from tests import clip_tol_rate_contract as TRC
from tests import frames_contract as FC
from tests import image_shared
from tests import rate_contract as RC
from tests import tiles_contract as TC
from tests.clip_rate_contract import items_of
from tests.test_chroma_host import fake_frame
from tests.test_image_shared_host import DEFINITIONS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "progressivecodec_amd")
DIR = os.path.join(PKG, "chroma_clip_tol_rate_gpu")
T = 64


def _lib():
    """the module and its library; a library that is not built is an ImportError, as for every other one"""
    from progressivecodec_amd import chroma_clip_tol_rate
    return chroma_clip_tol_rate, chroma_clip_tol_rate.lib()


# -- the restatement -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_centre_sited_420_is_section_20(fmt):
    for (H, W), O in [((100, 150), 0), ((65, 63), 16), ((127, 129), 32)]:
        ny, nx = TC.grid(H, W, T, O)
        tile_ids, runs = CS.run_list(ny * nx, H + O)
        fr = [FC.random_frame(1, H, W, fmt, seed=H + s) for s in range(3)]
        x = CS.hostile(len(tile_ids), seed=W + O)
        for matrix, rng in [("bt709", "limited"), ("bt601", "full")]:
            got = TR.run_sse(x, fr, tile_ids, runs, H, W, T, O, fmt, matrix, rng, "centre")
            assert got == TRC.run_sse(x, fr, tile_ids, runs, H, W, T, O, fmt, matrix, rng) and len(got) == TR.offsets_of(runs)[-1]
            assert CS.slots_matter(runs, got) > 0


def test_the_allocation_s_numbers():
    assert TR.budget(10 ** 4, 5, 6) == 10 ** 4 - 47 - 16 * 30 and TR.container_bytes([[5, 9]] * 3, [0, 1, 1], 4, 6) == 47 + 16 * 24 + 5 + 9 + 9
    assert TR.budget(1000, 4, 6) == TRC.RC2.budget(1000, 4, 6) - 5                   # 47 bytes of header where section 20 has 42
    assert (TR.frame_scale, TR.dists, TR.weights, TR.frame_sse, TR.predicted) == (TRC.frame_scale, TRC.dists, TRC.weights, TRC.frame_sse, TRC.predicted)
    from progressivecodec_amd import chroma_clip_rate, chroma_clips
    assert (chroma_clips.HEADER_BYTES, chroma_clip_rate.ENTRY_BYTES, chroma_clip_rate.MAGIC) == (TR.HEADER_BYTES, TR.ENTRY_BYTES, TR.MAGIC)


# -- the library, no device ------------------------------------------------------------------------------------------------------------

def test_workspace_size_is_24_bytes_per_wave_and_entry():
    _, L = _lib()
    from progressivecodec_amd import clip_tol_rate
    for size, n in [(64, 1), (64, 7), (128, 9), (512, 40), (576, 4), (1024, 3), (2048, 2)]:
        for sy in (1, 2):
            assert L.pc_chroma_clip_tol_rate_workspace_size(size, sy, n) == TR.workspace_size(size, sy, n) == 96 * n * (size * size // (2048 * sy))
        assert L.pc_chroma_clip_tol_rate_workspace_size(size, 2, n) == clip_tol_rate.lib().pc_clip_tol_rate_workspace_size(size, n)
    assert L.pc_chroma_clip_tol_rate_workspace_size(64, 2, 1) == 96 and L.pc_chroma_clip_tol_rate_workspace_size(64, 1, 3) == 576
    for bad in [(0, 1, 1), (32, 1, 1), (96, 2, 1), (-64, 1, 1), (2112, 1, 1), (4096, 2, 1), (64, 1, 0), (64, 2, -1), (64, 0, 1), (64, 3, 1),
                (2048, 1, 2 ** 31 - 1), (2048, 2, 2 ** 21), (2048, 1, 2 ** 20)]:
        assert L.pc_chroma_clip_tol_rate_workspace_size(*bad) == 0, bad
    assert L.pc_chroma_clip_tol_rate_workspace_size(2048, 1, 2 ** 20 - 1) == 96 * 2048 * (2 ** 20 - 1)


def table_of(fs):
    from progressivecodec_amd import frames
    return (frames.Frame * len(fs))(*fs)


def test_plan_is_host_only_and_each_precondition_is_broken_alone():
    """made-up pointer values: nothing may be dereferenced or launched (there is no GPU here); pc_chroma_clip_rate_plan's rule, and
    one misaligned frame among aligned ones makes the whole table narrow"""
    from progressivecodec_amd import chroma, chroma_clip_rate
    _, L = _lib()
    Fp = 0x7000_0100_0000
    H, W, st = 96, 160, (3 * T * T, T * T, T)

    def plan(fmt, fs, x=Fp, strides=st, O=0, n=None, sx=None, fn=L.pc_chroma_clip_tol_rate_plan):
        wide = C.c_int(-1)
        f = chroma.FORMATS[fmt]
        rc = fn(x, *strides, O, f.layout, f.bits, f.sx if sx is None else sx, table_of(fs) if fs else None, len(fs) if n is None else n, C.byref(wide))
        return rc, wide.value
    for fmt in sorted(chroma.FORMATS):
        f_ = chroma.FORMATS[fmt]
        es = 2 if f_.bits == 10 else 1
        planar = f_.layout == chroma.PLANAR
        good = lambda: [fake_frame(chroma, fmt, H, W), fake_frame(chroma, fmt, H, W, base=0x7100_0000_1000, pad=4),      # noqa: E731
                        fake_frame(chroma, fmt, H, W, base=0x7200_0000_1000, pad=8)]
        assert plan(fmt, good()) == (0, 1) and plan(fmt, good()[:1]) == (0, 1)
        cases = [dict(x=Fp + off) for off in (4, 8, 12)]
        for i in range(3):
            bad_st = list(st)
            bad_st[i] += 2
            cases.append(dict(strides=bad_st))
        cases += [dict(O=O) for O in (0, 8, 16, 32, 4, 12, 20, 28)]
        for kw in cases:
            got = plan(fmt, good(), **kw)
            assert got == plan(fmt, good(), fn=chroma_clip_rate.lib().pc_chroma_clip_rate_plan, **kw)      # the same rule
            assert got == (0, int(set(kw) == {"O"} and (kw["O"] % 8 == 0 or f_.sx == 1))), (fmt, kw)
        for slot in range(3):
            for nm in ["y", "u"] + (["v"] if planar else []):
                for off in (1, 2, 3):
                    fs = good()
                    setattr(fs[slot], nm, getattr(fs[slot], nm) + off * es)           # each plane of each frame: aligned to four elements
                    assert plan(fmt, fs) == (0, 0), (fmt, slot, nm, off)
                    assert plan(fmt, fs[:slot] + fs[slot + 1:]) == (0, 1)             # without that frame the table is wide
                fs = good()
                setattr(fs[slot], nm + "_row", getattr(fs[slot], nm + "_row") + 2)    # each row stride: a multiple of 4
                assert plan(fmt, fs) == (0, 0), (fmt, slot, nm)
                fs = good()
                setattr(fs[slot], nm + "_batch", getattr(fs[slot], nm + "_batch") + 1)                # no batch stride counts
                assert plan(fmt, fs) == (0, 1)
                fs = good()
                setattr(fs[slot], nm, None)
                assert plan(fmt, fs)[0] == -1, (fmt, slot, nm)
        assert plan(fmt, good(), O=-4)[0] == -1 and plan(fmt, [])[0] == -1 and plan(fmt, good(), n=0)[0] == -1 and plan(fmt, good(), n=-1)[0] == -1
        assert plan(fmt, good(), x=None)[0] == -1 and plan(fmt, good(), sx=3)[0] == -1 and plan(fmt, good(), sx=0)[0] == -1
        assert L.pc_chroma_clip_tol_rate_plan(Fp, *st, 0, f_.layout, f_.bits, f_.sx, table_of(good()), 3, None) == -1
    ok, wide = table_of([fake_frame(chroma, "nv12", H, W)]), C.c_int(-1)
    for layout, bits in [(2, 8), (-1, 8), (0, 9), (1, 12), (1, 16)]:
        assert L.pc_chroma_clip_tol_rate_plan(Fp, *st, 0, layout, bits, 2, ok, 1, C.byref(wide)) == -1
    assert plan("nv12", [fake_frame(chroma, "nv12", H, W)]) == (0, 1) and plan("i420", [fake_frame(chroma, "nv12", H, W)])[0] == -1


def offsets(*vals):
    return (C.c_int32 * len(vals))(*vals)


def test_every_argument_error_returns_before_the_device():
    """fake device pointers: every call below must return PC_ERR_ARG without touching them (no GPU here); each precondition is broken
    alone"""
    from progressivecodec_amd import chroma, frames
    _, L = _lib()
    Fp, Wk, S, Tl, Tb, Of, Sl = (0x7000_0100_0000, 0x7000_0200_0000, 0x7000_0300_0000, 0x7000_0400_0000, 0x7000_0500_0000, 0x7000_0600_0000,
                                 0x7000_0700_0000)
    H, W, O = 100, 150, 16                                                            # 2 x 3 tiles, S = 48
    k = frames.coefficients("bt709")
    for fmt in sorted(chroma.FORMATS):
        f_ = chroma.FORMATS[fmt]
        planar = f_.layout == chroma.PLANAR
        Wc = chroma.chroma_size(H, W, fmt)[1]

        def table(slot=None, field=None, value=None):
            fs = [fake_frame(chroma, fmt, H, W), fake_frame(chroma, fmt, H, W, base=0x7100_0000_1000, pad=3),
                  fake_frame(chroma, fmt, H, W, base=0x7200_0000_1000)]
            if slot is not None:
                setattr(fs[slot], field, value)
            return table_of(fs)
        bad_tables = [None]
        for slot in range(3):                                                         # a bad frame anywhere in the table
            bad_tables += [table(slot, "y", None), table(slot, "u", None), table(slot, "y_row", W - 1),
                           table(slot, "u_row", (Wc if planar else 2 * Wc) - 1)]
            if planar:
                bad_tables += [table(slot, "v", None), table(slot, "v_row", Wc - 1)]
            if f_.bits == 10:
                bad_tables += [table(slot, "y", 0x7000_0000_1001), table(slot, "u", 0x7000_0200_1001)]
        nbytes = L.pc_chroma_clip_tol_rate_workspace_size(T, f_.sy, 9)
        assert nbytes == 96 * 9 * 2 // f_.sy
        ok = dict(x=Fp, sxt=3 * T * T, sxc=T * T, sxh=T, H=H, W=W, T=T, O=O, layout=f_.layout, bits=f_.bits, shift=f_.shift, sx=f_.sx, sy=f_.sy,
                  hsite=1, vsite=0, range=0, kr=k.kr, kg=k.kg, kb=k.kb, ib=k.ib, ir=k.ir, frames_host=table(), frames_dev=Tb, n_frames=3, tiles=Tl,
                  offsets_host=offsets(0, 1, 3, 6, 7, 9), offsets_dev=Of, slots=Sl, n_jobs=5, n_entries=9, ws=Wk, nbytes=nbytes, out=S, stream=None)
        big = lambda size: dict(T=size, O=0, sxt=3 * size ** 2, sxc=size ** 2, sxh=size)                                # noqa: E731
        bads = [dict(frames_host=t) for t in bad_tables] + [
            dict(H=0), dict(W=0), dict(H=-5), dict(T=0), dict(T=32), dict(T=96), dict(T=-64), big(4096), big(2112),
            dict(O=2), dict(O=6), dict(O=36), dict(O=-4), dict(layout=2), dict(layout=-1), dict(bits=9), dict(bits=16), dict(shift=1),
            dict(shift=6 if f_.bits == 8 else 4), dict(sx=3), dict(sx=0), dict(sy=0), dict(sy=3), dict(sx=1, sy=2), dict(hsite=2), dict(hsite=-1),
            dict(vsite=2), dict(vsite=-1), dict(range=2), dict(range=-1),
            dict(x=None), dict(x=Fp + 2), dict(sxh=T - 1), dict(sxc=0), dict(sxt=0),
            dict(frames_dev=None), dict(frames_dev=Tb + 4), dict(n_frames=0), dict(n_frames=-1),
            dict(tiles=None), dict(tiles=Tl + 2), dict(offsets_dev=None), dict(offsets_dev=Of + 2), dict(slots=None), dict(slots=Sl + 2),
            dict(offsets_host=None),
            dict(offsets_host=offsets(1, 2, 3, 6, 7, 9)),                             # does not start at 0
            dict(offsets_host=offsets(0, 1, 1, 6, 7, 9)),                             # a job without an entry
            dict(offsets_host=offsets(0, 1, 3, 2, 7, 9)),                             # falls
            dict(offsets_host=offsets(0, 1, 3, 6, 7, 8)),                             # ends before n_entries
            dict(offsets_host=offsets(0, 1, 3, 6, 7, 10)),                            # ends after it
            dict(offsets_host=offsets(0, 1, 3, 6, 9, 9)),                             # the last job without an entry
            dict(offsets_host=offsets(-1, 1, 3, 6, 7, 9)),
            dict(n_jobs=0), dict(n_jobs=-1), dict(n_jobs=2 ** 31 - 1), dict(n_jobs=4), dict(n_jobs=10, n_entries=9),
            dict(n_entries=0), dict(n_entries=-1), dict(n_entries=4), dict(n_entries=8), dict(n_entries=10), dict(n_entries=2 ** 31 - 1),
            dict(ws=None), dict(ws=Wk + 4), dict(out=None), dict(out=S + 4), dict(nbytes=nbytes - 1), dict(nbytes=0)]
        if f_.bits == 10:
            bads += [dict(big(2048), nbytes=L.pc_chroma_clip_tol_rate_workspace_size(2048, f_.sy, 9)),
                     dict(big(1088), nbytes=L.pc_chroma_clip_tol_rate_workspace_size(1088, f_.sy, 9))]
        for bad in bads:
            assert L.pc_chroma_clip_tol_rate_sse_runs(*dict(ok, **bad).values()) == -1, (fmt, {k_: v for k_, v in bad.items() if k_ != "frames_host"})
    assert L.pc_chroma_clip_tol_rate_last_hip_error() == 0


# -- the Python layer ------------------------------------------------------------------------------------------------------------------

def _no_device(monkeypatch):
    from progressivecodec_amd import chroma_clip_rate, chroma_clip_tol, chroma_clips, clip_rate, clip_tol_rate, clips
    ctr, _ = _lib()

    def touched(*a, **k):
        raise AssertionError("the device was reached")
    for name in ("device", "current_stream", "synchronize", "current_device", "_lazy_init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    for mod in (ctr, chroma_clip_rate, chroma_clip_tol, chroma_clips, clip_rate, clip_tol_rate, clips):
        monkeypatch.setattr(mod, "lib", touched)
    monkeypatch.setattr(ctr, "_scan", touched)
    return ctr


def test_python_rejects_before_any_device_call(monkeypatch):
    from progressivecodec_amd import chroma_clip_rate, clip_tol, clip_tol_rate
    ctr = _no_device(monkeypatch)
    y, uv, u = torch.zeros(100, 150, dtype=torch.uint8), torch.zeros(100, 75, 2, dtype=torch.uint8), torch.zeros(100, 150, dtype=torch.uint8)
    f = (y, uv)
    p = (y.to(torch.uint16), uv.to(torch.uint16))
    x = torch.zeros(2, 3, 64, 64)
    g = ctr.grid_of(100, 150, 64, 16)
    for planes, fmt in [(f, "nv16"), ((y, u, u), "i444"), (p, "p210")]:
        with pytest.raises(ValueError, match="GPU"):
            ctr.tile_distortion_runs(x, g, [planes, planes], [0, 5], [[0], [1, 0]], fmt, siting="left")
        for kw in (dict(), dict(tolerance=ctr.Tolerance(1))):
            with pytest.raises(ValueError, match="GPU"):
                ctr.encode_clip_to_size(None, [planes, planes], [0, 1], 10 ** 6, fmt, siting="left", tile=64, **kw)
        with pytest.raises(ValueError, match="GPU"):
            ctr.encode_clip_to_size(None, tuple(torch.stack([t, t]) for t in planes), [0, 1], 10 ** 6, fmt, tile=64)
    dist = lambda **kw: ctr.tile_distortion_runs(x, g, [f, f], [0, 5], [[0], [1, 0]], **dict(dict(fmt="nv16"), **kw))     # noqa: E731
    enc = lambda **kw: ctr.encode_clip_to_size(None, [f], [0], 10 ** 6, **dict(dict(fmt="nv16"), **kw))                  # noqa: E731
    for fn in (dist, enc):
        for kw, msg in [(dict(fmt="nv21"), "fmt"), (dict(matrix="bt470"), "matrix"), (dict(range="tv"), "range"), (dict(siting="top"), "siting")]:
            with pytest.raises(ValueError, match=msg):
                fn(**kw)
    for kw, msg in [(dict(upsample="cubic"), "upsample"), (dict(max_tiles_per_call=0), "max_tiles_per_call must be at least 1"),
                    (dict(plane_weights=(1, 1)), "plane_weights"), (dict(plane_weights=(0, 0, 0)), "plane_weights"),
                    (dict(plane_weights=(1, -1, 1)), "plane_weights")]:
        with pytest.raises(ValueError, match=msg):
            enc(**kw)
    with pytest.raises(ValueError, match="at least one level"):
        ctr.encode_clip_to_size(None, [f], [], 10 ** 6, "nv16")
    with pytest.raises(ValueError, match="the grid of a 100x150 frame is 2x3"):
        ctr.tile_distortion_runs(x, g._replace(nx=4), [f], [0], [[0]], "nv16")
    with pytest.raises(ValueError, match="at most 1024"):
        ctr.tile_distortion_runs(x, ctr.grid_of(3000, 3000, 2048, 0), [p], [0], [[0]], "p210")
    with pytest.raises(TypeError, match="uint16"):
        dist(fmt="p210")
    for bad in ([], (), None, "clip"):
        with pytest.raises(ValueError, match="non-empty list"):
            ctr.tile_distortion_runs(x, g, bad, [0], [[0]], "nv16")
        with pytest.raises(ValueError, match="non-empty list"):
            ctr.encode_clip_to_size(None, bad, [0], 10 ** 6, "nv16")
    with pytest.raises(ValueError, match="got one frame"):
        ctr.encode_clip_to_size(None, f, [0], 10 ** 6, "nv16")
    with pytest.raises(ValueError, match="fmt"):
        ctr.plan(x, [], "nv21")
    assert issubclass(ctr.ChromaClipTolRateError, ctr._imagelib.ImageLibError) and ctr.LIB_PATH == os.path.join(PKG, "libpc_chroma_clip_tol_rate.so")
    sig = lambda fn: list(inspect.signature(fn).parameters)                                                               # noqa: E731
    assert sig(ctr.tile_distortion_runs) == ["x_hat_tiles", "grid", "frames", "tiles", "runs", "fmt", "matrix", "range", "siting"]
    assert sig(ctr.plan) == ["x_hat_tiles", "frames", "fmt", "overlap"]
    assert sig(ctr.encode_clip_to_size) == ["model", "frames", "qualities", "target_bytes", "fmt", "matrix", "range", "upsample", "siting", "tile",
                                            "overlap", "mask_pol", "tolerance", "plane_weights", "importance", "frame_weights", "max_tiles_per_call"]
    d = inspect.signature(ctr.encode_clip_to_size).parameters
    assert (d["siting"].default, d["tile"].default, d["overlap"].default, d["tolerance"].default, d["max_tiles_per_call"].default) == \
        ("centre", 512, 0, ctr.Tolerance(), 32)
    # decoding needs nothing new; the plan is section 20's with sse_exact
    assert (ctr.decode_clip, ctr.frame_container, ctr.parse_clip, ctr.tile_blob) == \
        (chroma_clip_rate.decode_clip, chroma_clip_rate.frame_container, chroma_clip_rate.parse_clip, chroma_clip_rate.tile_blob)
    assert ctr.Tolerance is clip_tol.Tolerance and ctr.ChromaClipTolRatePlan._fields == clip_tol_rate.ClipTolRatePlan._fields + ("sse_exact",)


def test_python_checks_that_need_a_frame_that_passes(monkeypatch):
    """the checks behind the frames' own, tiles and runs among them with clip_tol_rate's texts: nothing may reach the device"""
    from progressivecodec_amd import clip_tol_rate
    ctr = _no_device(monkeypatch)
    y, uv = torch.zeros(100, 150, dtype=torch.uint8), torch.zeros(100, 75, 2, dtype=torch.uint8)
    f = (y, uv)
    monkeypatch.setattr(ctr, "_clip_frames", lambda frames, fmt: ([[t.unsqueeze(0) for t in p] for p in frames], 100, 150))
    g = ctr.grid_of(100, 150, 64, 16)
    x = torch.zeros(2, 3, 64, 64)
    assert ctr._runs is clip_tol_rate._runs and ctr._offsets is clip_tol_rate._offsets
    for tiles, runs, msg in [([], [], "at least one tile"), ([0, 1], [[0]], "one list of frames per tile, 2 in all"), ([0, 6], [[0], [0]], "lies outside"),
                             ([0, -1], [[0], [0]], "lies outside"), ([0, 1], [[0], [2]], "lies outside"), ([0, 1], [[0], [0, -1]], "lies outside"),
                             ([0, 1.0], [[0], [0]], "a tile is an int"), ([0, True], [[0], [0]], "a tile is an int"), ([0, 1], [[0], []], "non-empty list"),
                             ([0, 1], [[0], 1], "non-empty list"), ([0, 1], [[0], [0.0]], "non-empty list"), (torch.tensor([0, 6]), [[0], [1]], "lies outside")]:
        with pytest.raises(ValueError, match=msg):
            ctr.tile_distortion_runs(x, g, [f, f], tiles, runs, "nv16")
    with pytest.raises(ValueError, match="one tile per entry of tiles"):
        ctr.tile_distortion_runs(x, g, [f, f], [0], [[0, 1]], "nv16")
    monkeypatch.setattr(ctr, "_clip_frames", lambda frames, fmt: ([[t.unsqueeze(0) for t in p] for p in frames], 64, 64))
    with pytest.raises(ValueError, match="frames must be 100x150 frames"):
        ctr.tile_distortion_runs(x, g, [f, f], [0, 1], [[0], [1]], "nv16")
    monkeypatch.setattr(ctr, "_clip_frames", lambda frames, fmt: ([[t.unsqueeze(0) for t in p] for p in frames], 100, 150))
    enc = lambda fmt="nv16", **kw: ctr.encode_clip_to_size(None, [f, f, f], [0, 1], 10 ** 6, fmt, **dict(dict(tile=64, overlap=16), **kw))     # noqa: E731
    for kw, msg in [(dict(tile=96), "multiple of 64"), (dict(overlap=6), "overlap"), (dict(tile=4096, overlap=0), "at most 2048"),
                    (dict(fmt="p210", tile=2048, overlap=0), "at most 1024"), (dict(importance=[1] * 5), "importance needs one number per tile of the 2x3 grid"),
                    (dict(frame_weights=[1, 1]), "frame_weights needs one number per frame"),
                    (dict(tolerance=None), "tolerance must be a clip_tol.Tolerance"), (dict(tolerance=(1, 1, 1)), "tolerance must be a clip_tol.Tolerance"),
                    (dict(tolerance=ctr.Tolerance(256)), "max_abs must be at most 255"),
                    (dict(frame_weights=[1, 0, 1]), "frame_weights needs one positive number per frame, 3 in all"),
                    (dict(importance=[1, 1, 1, 0, 1, 1]), "importance needs one positive number per tile, 6 in all")]:
        with pytest.raises(ValueError, match=msg):
            enc(**kw)
    with pytest.raises(AssertionError, match="the device was reached"):             # nothing above is wrong with good arguments
        enc()


# -- through a fake model ------------------------------------------------------------------------------------------------------------

SOURCE = [[0] * 6, [1, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [1, 3, 0, 0, 3, 0]]


def test_encode_against_a_fake_model(monkeypatch):
    """one scan; the items are chunked across frames, one sse_runs call per level and chunk over tables uploaded once, each chunk's
    offsets rebased to 0, one workspace sized for the chunk with the most entries; the bytes and the plan do not depend on the
    chunking; the budget is target - 47 - 16 F n, and a target below the minimum names it"""
    from progressivecodec_amd import container
    ctr, _ = _lib()
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    items, runs = items_of(SOURCE)
    tags = [16 * f + t for f, t in items]
    off = TR.offsets_of(runs)
    assert tags == [0, 1, 2, 3, 4, 5, 16, 49, 52] and off[-1] == 24
    chunks, measured, asked, uploads, base = [], [], [], [], []
    stats = torch.zeros(4, 6, 3, 3, dtype=torch.int64)
    stats[1, 2, 1], stats[2, 3, 2], stats[3, 5, 0] = torch.tensor([7, 7, 1]), torch.tensor([9, 36, 2]), torch.tensor([1, 9, 3])

    class Model:
        def compress_levels(self, x, qualities, mask_pol):
            chunks.append(list(x))
            return [{"strings": [[[bytes([t, s]) * (1 + (s + t) % 3 + 2 * l) for t in x] for s in range(10 if q == 0 else 20)], [bytes([t]) for t in x]],
                     "shape": (1, 1)} for l, q in enumerate(qualities)]

        def decompress_levels(self, strings, shape, qualities, mask_pol):
            return [{"x_hat": torch.full((len(s[1]), 3, T, T), float(l))} for l, s in enumerate(strings)]

    def scan(fs, fmt, siting, g, upsample, tol):
        asked.append((fmt, siting, upsample, tuple(g)[:4], tol))
        return torch.tensor(SOURCE, dtype=torch.int32), stats

    def cut_of(fs, g, work, *a):
        assert a == ("p210", "bt2020", "limited", "linear", "left")
        return lambda a_, b_: [16 * f + t for f, t in work[a_:a_ + b_]]

    def sse_runs_into(L, x, g, fmt, siting, rng, k, host, table, F, tiles_ptr, offsets_host, offsets_ptr, slots_ptr, n, ne, ws, nbytes, out, stream):
        words = uploads[-1]
        level = int(x[0, 0, 0, 0].item())
        first, at_off, at_slot = (tiles_ptr - base[0]) // 4, (offsets_ptr - base[0]) // 4, (slots_ptr - base[0]) // 4
        host_off = list(offsets_host)
        assert words[at_off:at_off + n + 1] == host_off and host_off[0] == 0 and host_off[-1] == ne       # rebased, the same bytes on both sides
        measured.append((first, n, ne, level, F, nbytes, at_slot - (9 + sum(len(c) + 1 for c in chunks_of[-1]))))
        for m in range(n):
            for j in range(host_off[m], host_off[m + 1]):
                tile, slot = words[first + m], words[at_slot + j]
                out[j] = torch.tensor([1000 * (3 - level) + 100 * slot + tile, 10 * (3 - level) + slot, 3 - level])
    real_tensor = torch.tensor
    chunks_of = []

    def tensor(data, *a, **k):
        t = real_tensor(data, *a, **k)
        if k.get("dtype") == torch.int32 and t.dim() == 1 and len(data) > 9:
            base[:] = [t.data_ptr()]
            uploads.append(t.tolist())
            keep.append(t)
        return t
    keep = []
    fake_lib = types.SimpleNamespace(pc_chroma_clip_tol_rate_workspace_size=lambda T_, sy, n: 96 * n * (T_ * T_ // (2048 * sy)))
    monkeypatch.setattr(ctr, "_clip_frames", lambda frames, fmt: ([[torch.zeros(1)]] * 4, 100, 150))
    monkeypatch.setattr(ctr, "_scan", scan)
    monkeypatch.setattr(ctr, "_cut_of", cut_of)
    monkeypatch.setattr(ctr, "_frame_table", lambda fs, dev: ("host", torch.zeros(1)))
    monkeypatch.setattr(ctr, "_sse_runs_into", sse_runs_into)
    monkeypatch.setattr(ctr, "lib", lambda: fake_lib)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev: types.SimpleNamespace(cuda_stream=0))
    monkeypatch.setattr(torch, "tensor", tensor)
    tol = ctr.Tolerance(2, max_run=4)
    kw = dict(matrix="bt2020", siting="left", tile=T, overlap=16, tolerance=tol)
    outs = []
    for per_call in (1, 4, 32):
        del chunks[:], measured[:], asked[:], uploads[:]
        bounds = [(a, min(a + per_call, 9)) for a in range(0, 9, per_call)]
        chunks_of.append([items[a:b] for a, b in bounds])
        buf, plan = ctr.encode_clip_to_size(Model(), None, [0, 0.5, 10], 10 ** 6, "p210", max_tiles_per_call=per_call, **kw)
        assert chunks == [tags[a:b] for a, b in bounds] and asked == [("p210", "left", "linear", (100, 150, T, 16), tol)]
        most = max(off[b] - off[a] for a, b in bounds)
        assert measured == [(a, b - a, off[b] - off[a], l, 4, 96 * most * 2, off[a]) for a, b in bounds for l in range(3)]
        # one upload: the tiles, every chunk's offsets rebased to 0, the slots
        assert uploads == [[t for _, t in items] + [off[m] - off[a] for a, b in bounds for m in range(a, b + 1)] + [k for run in runs for k in run]]
        outs.append((buf, plan))
    assert outs[0] == outs[1] == outs[2]
    buf, plan = outs[0]
    assert plan.source == SOURCE and plan.items == items and plan.runs == runs and plan.weights == [1] * 9 and plan.den == 32 and plan.frame_scale == 1
    assert plan.plane_dists == [[[[1000 * (3 - l) + 100 * k + t, 10 * (3 - l) + k, 3 - l] for k in run] for l in range(3)] for (_, t), run in zip(items, runs)]
    assert plan.dists == TR.dists(plan.plane_dists, runs) and plan.sse_exact is False and plan.stats == stats.tolist() and plan.worst == [3, 1, 2]
    assert (plan.n_coded, plan.n_reused, plan.container_bytes) == (9, 15, len(buf)) and plan.levels == [2] * 9
    assert plan.sse == TR.frame_sse(SOURCE, plan.plane_dists, plan.levels) and plan.predicted == TR.predicted(plan.plane_dists, plan.levels)
    hd = ctr.parse_clip(buf)
    blobs = [[ctr.tile_blob(buf, hd, f, t)[0] if s == f else None for t, s in enumerate(row)] for f, row in enumerate(SOURCE)]
    from tests import chroma_clip_rate_contract as JC
    assert buf == JC.pack_clip(blobs, SOURCE, 100, 150, T, 16, "p210", "bt2020", "limited", "linear", "left", 1) and buf[:4] == b"PCL2"
    assert [len(blobs[f][t]) for f, t in items] == [r[2] for r in plan.rates]
    # the budget arithmetic: 47 bytes of header, 16 per frame and tile
    fixed = 47 + 16 * 4 * 6
    lo, hi = fixed + sum(min(r) for r in plan.rates), fixed + sum(max(r) for r in plan.rates)
    assert hi == len(buf) and lo < hi
    for target in (lo, (lo + hi) // 2, hi - 1, hi):
        chunks_of.append([items])
        b, p = ctr.encode_clip_to_size(Model(), None, [0, 0.5, 10], target, "p210", **kw)
        assert p.levels == RC.allocate(plan.rates, plan.dists, target - fixed, plan.weights) == RC.allocate(plan.rates, plan.dists, TR.budget(target, 4, 6),
                                                                                                           plan.weights)
        assert len(b) == TR.container_bytes(plan.rates, p.levels, 4, 6) <= target
        assert p.sse == TR.frame_sse(SOURCE, plan.plane_dists, p.levels) and p.predicted == TR.predicted(plan.plane_dists, p.levels)
    with pytest.raises(ValueError, match=rf"target_bytes = {lo - 1} is below the minimum of {lo} bytes: {fixed} bytes of header and table"):
        ctr.encode_clip_to_size(Model(), None, [0, 0.5, 10], lo - 1, "p210", **kw)
    # importance reaches the allocator as exact fractions, the frame weights inside the distortions
    seen = []
    monkeypatch.setattr(ctr.clip_rate, "allocate", lambda rates, dists, budget, weights: seen.append((budget, weights, dists)) or [0] * len(rates))
    fw = [1, 0.5, 1, 3]
    ctr.encode_clip_to_size(Model(), None, [0, 0.5, 10], hi, "p210", importance=[[1, 2, 3], [4, 5, 6]], frame_weights=fw, plane_weights=(2, 1, 0), **kw)
    assert seen == [(hi - fixed, [1, 2, 3, 4, 5, 6, 1, 2, 5], TR.dists(plan.plane_dists, runs, (2, 1, 0), fw, 4))]


# -- structure -----------------------------------------------------------------------------------------------------------------------

def function_body(text, start):
    """the text between the braces that open at or after `start`"""
    start = text.index("{", start)
    depth = 0
    for i in range(start, len(text)):
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        if depth == 0:
            return text[start + 1:i]
    raise AssertionError("unbalanced braces")


def _code(path):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S))


SHARED_NAMES = ("emit_px", "load4", "clampi", "code_of", "axis_weight", "planes_of", "Levels", "EmitCoef", "Measure", "Grid", "geo_of", "format_of",
                "with_format", "picture_ok", "site_ok", "depth_levels", "f32_wide", "plane_wide", "wave_reduce", "row_final", "HIPCHK")


def test_the_eighteenth_library_keeps_the_rules_of_the_seventeen():
    ctr, L = _lib()
    from progressivecodec_amd import chroma
    hdr = open(os.path.join(DIR, "pc_chroma_clip_tol_rate.h")).read()
    declared = re.findall(r"PC_API\s+[\w\s\*]+?\b(pc_\w+)\s*\(", hdr)
    assert len(declared) == 5 and sorted(declared) == sorted(ctr.EXPORTS)
    for name in declared:
        getattr(L, name)
    assert L.pc_chroma_clip_tol_rate_strerror(-1).decode() and L.pc_chroma_clip_tol_rate_strerror(-6).decode()
    assert "offsets" in L.pc_chroma_clip_tol_rate_strerror(-1).decode() and L.pc_chroma_clip_tol_rate_last_hip_error() == 0
    # the directory holds the header and the source alone: no Makefile; csrc/Makefile drives it straight through the shared rule
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(DIR, "*")) if not p.endswith((".o", ".so")))
    assert names == ["pc_chroma_clip_tol_rate.h", "pc_chroma_clip_tol_rate.hip"] and not DIR.endswith(("_csrc", "_hip", "_kernels"))
    top = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\bchroma_clip_tol_rate\b", top, re.M) and re.search(r"^\.PHONY:.*\bchroma_clip_tol_rate\b", top, re.M)
    assert re.search(r"^chroma_clip_tol_rate:\n\t\$\(MAKE\) -C \.\./chroma_clip_tol_rate_gpu -f \.\./image_csrc/lib\.mk NAME=chroma_clip_tol_rate$", top, re.M)
    assert "\t$(MAKE) -C ../chroma_clip_tol_rate_gpu -f ../image_csrc/lib.mk NAME=chroma_clip_tol_rate clean\n" in top
    bare = image_shared.uncommented(os.path.join(PKG, "csrc", "Makefile"))
    assert len(re.findall(r"\bchroma_clip_tol_rate\b(?!_)", bare)) == 5 and len(re.findall(r"chroma_clip_tol_rate_gpu", bare)) == 2
    # the pins of the earlier libraries' tests stay true
    assert len(re.findall(r"\bchroma_clip_tol\b(?!_)", bare)) == 5 and len(re.findall(r"chroma_clip_tol_gpu", bare)) == 2
    rule = image_shared.uncommented(os.path.join(PKG, "image_csrc", "lib.mk"))
    assert "-ffp-contract=off" in rule and not re.search(r"-lpc|libpc(odec|_\w+)\b", rule)
    assert re.search(r"^OUT\s*:=\s*\.\./libpc_\$\(NAME\)\.so$", rule, re.M) and re.search(r"^SHARED\s*:=\s*\$\(wildcard \.\./image_csrc/\*\.h\)$", rule, re.M)
    assert len(glob.glob(os.path.join(PKG, "*_csrc", "*.hip"))) == len(image_shared.LIBS) == 10
    assert len(glob.glob(os.path.join(PKG, "*_hip", "*.hip"))) == 4 and len(glob.glob(os.path.join(PKG, "*_kernels", "*.hip"))) == 2
    assert len(glob.glob(os.path.join(PKG, "*", "Makefile"))) == 17 and len(glob.glob(os.path.join(PKG, "*_gpu", "*.hip"))) == 2
    src = open(os.path.join(DIR, "pc_chroma_clip_tol_rate.hip")).read()
    code = _code(os.path.join(DIR, "pc_chroma_clip_tol_rate.hip"))
    for inc in ("pc_image_host.h", "pc_reduce.h", "pc_tile_grid.h", "pc_yuv_device.h", "pc_chroma_items.h", "pc_chroma_sse_item.h"):
        assert '#include "%s"' % inc in src, inc
    for other in ("pc_chroma.h", "pc_chroma_rate.h", "pc_chroma_clip_rate.h", "pc_clip_tol_rate.h", "pc_chroma_clip_tol.h", "pc_yuv_items.h"):
        assert '"%s"' % other not in code, other
    # the shared names are used, not defined; the item's two halves have one user and are defined here, under names of their own
    for name, pattern in DEFINITIONS.items():
        assert not re.search(pattern, code), name
    for name in SHARED_NAMES:
        assert re.search(r"\b%s\b" % name, code), name
        assert not re.search(r"\b(struct|void|int|bool|unsigned|float|define|constexpr int)\s+%s\b\s*[({=]" % name, code), name
    shared = "".join(_code(p) for p in glob.glob(os.path.join(PKG, "image_csrc", "*.h")))
    for name in ("run_row", "run_emit", "run_compare", "held_code", "Held", "Tables", "sse_runs_kernel", "run_blocks_of", "partial_bytes"):
        assert re.search(r"\b%s\b" % name, code) and not re.search(r"\b%s\b" % name, shared), name
    assert "sse_item<" not in code and "weighted_row<" not in code and "block_reduce" not in code and "code_of<T>" in code and ">> SH" not in code
    for path in ("chroma_rate_hip/pc_chroma_rate.hip", "chroma_clip_rate_kernels/pc_chroma_clip_rate.hip"):
        assert "sse_runs" not in open(os.path.join(PKG, path)).read()
    image_shared.assert_frame_is_shared(hdr, "pc_cctr_frame")
    values = dict((k, int(v)) for k, v in re.findall(r"\b(PC_CCTR_\w+) = (\d+)[,\s]", hdr))
    assert values == {"PC_CCTR_PLANAR": chroma.PLANAR, "PC_CCTR_SEMIPLANAR": chroma.SEMIPLANAR, "PC_CCTR_CENTRE": chroma.CENTRE,
                      "PC_CCTR_COSITED": chroma.COSITED}
    assert dict(re.findall(r"\b(PC_CCTR_(?:LIMITED|FULL)) = (\w+)", hdr)) == {"PC_CCTR_LIMITED": "PC_YUV_LIMITED", "PC_CCTR_FULL": "PC_YUV_FULL"}
    assert code.count("static_assert(PC_CCTR_") == 2 and "LAYOUT_SEMIPLANAR" in code and "SITE_COSITED" in code
    # plain C++: no inline assembly, no builtins, no atomics, no LDS, no barrier
    assert not re.search(r"\batomic(Add|CAS|Exch|Max|Min|Or|And)\b|\basm\b|__asm|__shared__|__syncthreads|__builtin_|__shfl", code)
    # two kernels in the text (32 + 1 instantiations), two launch sites, every refusal before the first of them
    assert "32 sse_runs kernels and the final" in src and len(re.findall(r"__global__", code)) == 2
    call = function_body(code, code.index('extern "C" int pc_chroma_clip_tol_rate_sse_runs('))
    assert call.count("hipLaunchKernelGGL(") == 2 == code.count("hipLaunchKernelGGL(") and "hipLaunchKernelGGL(final_kernel" in call
    assert call.rindex("return PC_ERR_ARG") < call.index("hipLaunchKernelGGL(") and not re.search(r"hipMalloc|hipFree|Synchronize|hipMemcpy|hipMemset", code)
    # one function decides the access path: the call and the exported plan both go through it
    assert len(re.findall(r"\bwide_path\(", code)) == 3
    assert "wide_path(" in call and "wide_path(" in function_body(code, code.index('extern "C" int pc_chroma_clip_tol_rate_plan('))
    # the entry loop: no branch leaves it before the wave's write, and the write is lane 0's
    kernel = function_body(code, code.index("void sse_runs_kernel("))
    loop = function_body(kernel, kernel.index("for (int e = e0; e < e1; ++e)"))
    assert not re.search(r"\b(break|continue|return|goto)\b", loop) and loop.index("wave_reduce<Sum>(su)") < loop.index("(threadIdx.x & 63) == 0")
    assert "clampi(tb.offsets[m], 0, tb.n_entries)" in kernel and "clampi(tb.offsets[(int64_t)m + 1], 0, tb.n_entries)" in kernel
    assert "slot >= 0 && slot < tb.n_frames" in loop and "tg >= 0 && tg < gr.ny * gr.nx" in kernel
    # the width arguments stand next to the code
    for text in ("each term < 2^11 * 2^16 (8 bits), 2^10 * 2^20 (10 bits)", "< T * T / 8 <= 2^19", "T^4 * 255^2 < 2^60", "T^4 * 1023^2 < 2^60"):
        assert text in src, text
    import bench
    assert "chroma" not in inspect.getsource(bench.source_hash) and "_gpu" not in inspect.getsource(bench.source_hash)
    from progressivecodec_amd import _imagelib, chroma_clip_rate, chroma_clip_tol
    for m in (_imagelib, chroma_clip_rate, chroma_clip_tol):
        assert "chroma_clip_tol_rate" in m.__doc__, m.__name__


def test_own_c_calls_and_no_copied_body():
    """section 26's rule for a ported layer: what another module already does is called there, never restated here"""
    ctr, _ = _lib()
    from progressivecodec_amd import chroma_clip_rate, chroma_clip_tol, chroma_clips, clip_rate, clip_tol_rate
    text = re.sub(r'"""[\s\S]*?"""', "", inspect.getsource(ctr))                     # the code without its docstrings
    for call in ("clip_rate._to_size_arguments(", "_tolerance(tolerance, fmt)", "_scan(fs, fmt, siting, g, upsample, tol)", "items_of(source)",
                 "frame_scale(frame_weights, F)", "item_importance(", "_offsets(runs)", "_runs(tiles, runs, len(fs), full)",
                 "_tilecodec.encode_items(", "_cut_of(fs, g, items, fmt, matrix, range, upsample, siting)", "clip_rate._allocate_and_pack(",
                 "header_bytes=HEADER_BYTES", "pack_clip(*a, siting)", "chroma_rate.sse_exact(g, fmt, siting)", "_frame_table(fs, dev)"):
        assert call in text, call
    for own in ("def _runs", "def _offsets", "def frame_scale", "def item_importance", "def items_of", "def pack_clip", "def parse_clip", "def decode_clip",
                "def frame_container", "def tile_blob", "def _scan", "def _tolerance", "class Tolerance", "allocate(", "container.pack", "compress_levels("):
        assert own not in text, own
    assert (ctr._scan, ctr._tolerance) == (chroma_clip_tol._scan, chroma_clip_tol._tolerance) and ctr._cut_of is chroma_clips._cut_of
    assert (ctr.frame_scale, ctr.item_importance, ctr.items_of) == (clip_tol_rate.frame_scale, clip_tol_rate.item_importance, clip_rate.items_of)
    assert ctr.pack_clip is chroma_clip_rate.pack_clip and ctr.HEADER_BYTES == 47
    for name in ctr.EXPORTS[:3]:
        assert "L." + name + "(" in text or "lib()." + name + "(" in text, name
    assert not re.search(r"pc_chroma_clip_rate_|pc_clip_tol_rate_|pc_chroma_clip_tol_(?!rate)", text)


# -- the ledger and the GPU tests' own inputs ----------------------------------------------------------------------------------------------

def test_every_instantiation_is_launched():
    """pc_chroma_clip_tol_rate.hip: "32 sse_runs kernels": 16 item shapes on two access paths.  The tuples the table reaches are exactly
    those; a case taken away shows here by the name of the kernel nothing launches any more"""
    assert len(CS.ALL) == 32 and len({t[:5] for t in CS.ALL}) == 16
    table = CS.table()
    assert len(table) == 12 * 6 + 4 * 4 + 4 * 4 and len(set(table)) == len(table)
    got = CS.reached(table)
    assert got == CS.ALL, "never launched: %s" % CS.names(CS.ALL - got)
    assert {(c.fmt, c.siting, c.O) for c in table if (c.H, c.W) == (100, 150) and c.n < 100} == {(f, s, O) for f in CC.FORMATS for s in CC.SITINGS for O in (0, 4)}
    assert {(c.fmt, c.H, c.W, c.O) for c in table if 100 <= c.n < 200} == {(f, H, W, O) for f in CS.OTHER_FORMATS for H, W in [(65, 63), (127, 129)] for O in (16, 32)}
    assert {(c.fmt, c.H, c.W, c.O) for c in table if c.n >= 200} == {(f, 100, 150, O) for f in CS.OTHER_FORMATS for O in (24, 28)}
    assert CS.OTHER_FORMATS == ["nv16", "p210", "i444", "nv12"] and (CS.T, CS.F) == (64, 3)
    for fmt in CS.OTHER_FORMATS:                                     # O = 28 is narrow at sx == 2 even on an aligned table; O = 24 is not
        assert {CS.wide(c) for c in CS.band_cases(fmt) if c.O == 28 and c.aligned} == {CC.sub(fmt)[0] == 1}
        assert {CS.wide(c) for c in CS.band_cases(fmt) if c.O == 24} == {True, False}
    less = [c for c in table if not (c.fmt == "i010" and c.siting == "topleft" and c.O == 0)]
    gone = CS.ALL - CS.reached(less)
    assert len(gone) == 1 and next(iter(gone))[:5] == (2, False, 2, 2, True)


def test_the_kernel_matrix_can_tell_a_kernel_that_ignores_its_slots():
    """conditions on the GPU tests' inputs, from the restatement: in every run of the matrix, entries of different frames have rows
    that differ in every plane, so rows copied from another entry of the run, or measured against another frame, cannot pass; every
    case has runs of every length, over all frames, reversed and repeated"""
    pairs = 0
    for c in CS.table():
        fr, x_np, tile_ids, runs = CS.inputs(c)
        ny, nx = TC.grid(c.H, c.W, T, c.O)
        assert sorted(set(tile_ids)) == list(range(ny * nx)) and len(tile_ids) == ny * nx + 5 and {len(r) for r in runs} == {1, 2, 3}
        assert any(sorted(r) == [0, 1, 2] for r in runs) and any(len(set(r)) < len(r) for r in runs) and any(r != sorted(r) for r in runs)
        assert not np.isfinite(x_np).all() and x_np.shape == (len(tile_ids), 3, T, T)
        assert all(any((np.asarray(a) != np.asarray(b)).any() for a, b in zip(fr[i], fr[j])) for i in range(3) for j in range(i))
        want = CS.want(c)
        assert len(want) == TR.offsets_of(runs)[-1] and all(0 <= v < 2 ** 60 for row in want for v in row)
        pairs += CS.slots_matter(runs, want)
    assert pairs > 5 * len(CS.table())


@pytest.mark.parametrize("fmt,siting", CS.CODEC + [("nv12", "centre")])
def test_the_codec_tests_clips_are_reused_under_the_tolerance_alone(fmt, siting):
    """the noisy clips under Tolerance(max_abs=1): tiles are reused, the longest run has at least three frames, the largest difference
    of a reused tile is one code in every plane; the exact test reuses nothing"""
    clip = CS.noisy_clip(fmt, siting)
    assert len(clip) == CS.CODEC_F == 5
    for O in (0, 16):
        source, stats = TOL.scan(clip, fmt, siting, T, O, "linear", (1, 1, 1))
        items, runs = items_of(source)
        n_reused = 5 * CS.N - len(items)
        assert n_reused > 0 and max(len(r) for r in runs) >= 3 and TOL.worst(source, stats) == [1, 1, 1], (fmt, siting, O)
        assert TOL.scan(clip, fmt, siting, T, O, "linear")[0] == [[k] * CS.N for k in range(5)]


@pytest.mark.parametrize("fmt,siting", CL.FORMATS)
def test_the_tail_only_tiles_err_in_their_last_rows_alone(fmt, siting):
    """the limits suite's tail case: the tail tile is the equal tile up to its last sy rows, bit for bit; against the frame that holds
    the equal tile's rendering the restatement gives [row, row, 0, 0] with row > 0 in every plane, and every code the two tiles
    differ in lies in the last sy luma rows and the last chroma row -- the last items of the tile's last block"""
    from tests import chroma_rate_contract as XC
    size, H, W = (CL.SECOND_TRIP[k] for k in ("T", "H", "W"))
    sx, sy = CC.sub(fmt)
    tail, eq, frame = CL.rate_tail(fmt, siting, size, H, W)
    assert np.array_equal(tail[:, :, :size - sy].view(np.uint32), eq[:, :, :size - sy].view(np.uint32))
    other = CC.random_frame(1, H, W, fmt, seed=77, garbage=True)
    rows = TR.run_sse(np.concatenate([tail, eq]), [frame, other], [0, 0], [[0, 0], [0, 0]], H, W, size, 0, fmt, "bt709", "limited", siting)
    assert rows[0] == rows[1] and all(v > 0 for v in rows[0]) and rows[2:] == [[0, 0, 0], [0, 0, 0]]
    y, cb, cr = XC.tile_codes(tail[0], size, size, fmt, "bt709", "limited", siting)
    ey, ecb, ecr = XC.tile_codes(eq[0], size, size, fmt, "bt709", "limited", siting)
    assert (y[:size - sy] == ey[:size - sy]).all() and (cb[:size // sy - 1] == ecb[:size // sy - 1]).all() and (cr[:size // sy - 1] == ecr[:size // sy - 1]).all()
    bpt = size * size // (2048 * sy)
    first_item_of_the_last_rows = (size // sy - 1) * (size // 8)
    assert first_item_of_the_last_rows // 256 == bpt - 1 and (4 * bpt - 4) // 64 == -(-4 * bpt // 64) - 1       # the last block; the final's last trip

"""Tolerant rate-controlled clips without a GPU: the structure of the eleventh image-side library (the same rules as the ten,
DESIGN.md sections 19 and 20); libpc_clip_tol_rate.so's C ABI up to the first device call; the restatement of section 20
(tests/clip_tol_rate_contract.py) on hand-made tables, with the argument that the scaled allocation is clip_rate's; and
progressivecodec_amd.clip_tol_rate's argument checks."""
import ctypes as C
import glob
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import clip_rate_contract as RC2
from tests import clip_tol_rate_contract as TRC
from tests import frames_contract as FC
from tests import image_shared
from tests import rate_contract as RC
from tests.test_clips_host import SOURCE
from tests.test_frames_host import fake_frame
from tests.test_image_shared_host import DEFINITIONS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "progressivecodec_amd")
DIR = os.path.join(PKG, "clip_tol_rate_hip")
T = 64


def _lib():
    from progressivecodec_amd import clip_tol_rate
    return clip_tol_rate, clip_tol_rate.lib()


# -- structure -----------------------------------------------------------------------------------------------------------------------

def test_the_eleventh_library_keeps_the_rules_of_the_ten():
    ctr, L = _lib()
    hdr = open(os.path.join(DIR, "pc_clip_tol_rate.h")).read()
    declared = re.findall(r"PC_API\s+[\w\s\*]+?\b(pc_\w+)\s*\(", hdr)
    assert len(declared) == 5 and sorted(declared) == sorted(ctr.EXPORTS)
    for name in declared:
        getattr(L, name)
    assert L.pc_clip_tol_rate_strerror(-1).decode() and L.pc_clip_tol_rate_strerror(-6).decode() and L.pc_clip_tol_rate_last_hip_error() == 0
    assert ctr.LIB_PATH == os.path.join(PKG, "libpc_clip_tol_rate.so")
    # its Makefile is its name and the shared rule, which is the rule of the ten, unchanged
    mk = image_shared.uncommented(os.path.join(DIR, "Makefile"))
    assert mk == "NAME := clip_tol_rate\ninclude ../image_csrc/lib.mk\n"
    rule = image_shared.build_rule("clip_rate")
    assert "-ffp-contract=off" in rule and not re.search(r"-lpc|libpc(?!_\$\(NAME\)\.so)", rule)
    top = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\bclip_tol_rate\b", top, re.M) and re.search(r"^\.PHONY:.*\bclip_tol_rate\b", top, re.M)
    assert "$(MAKE) -C ../clip_tol_rate_hip clean" in top and re.search(r"^clip_tol_rate:\n\t\$\(MAKE\) -C \.\./clip_tol_rate_hip$", top, re.M)
    # the directory holds the Makefile, the header and one source; it is not one of the *_csrc the structure tests of the ten count
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(DIR, "*")) if not p.endswith((".o", ".so")))
    assert names == ["Makefile", "pc_clip_tol_rate.h", "pc_clip_tol_rate.hip"]
    assert len(glob.glob(os.path.join(PKG, "*_csrc", "*.hip"))) == len(image_shared.LIBS) == 10
    # the source reaches the shared names through the host header and restates none of them
    src = open(os.path.join(DIR, "pc_clip_tol_rate.hip")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert '#include "pc_image_host.h"' in src
    for name, pattern in DEFINITIONS.items():
        assert not re.search(pattern, code), name
    for name in ("emit_px", "emit_chroma", "axis_weight", "planes_of", "wave_reduce", "row_final", "pair_blocks_of", "frame_wide", "f32_wide"):
        assert re.search(r"\b%s\b" % name, code) and not re.search(r"\b(void|int|bool|unsigned|Planes<T>)\s+%s\s*\(" % name, code), name
    # the frame is the one record of image_csrc/pc_yuv_frame.h, the enum names alias the shared values
    image_shared.assert_frame_is_shared(hdr, "pc_ctr_frame")
    found = dict(re.findall(r"\b(PC_CTR_(?:NV12|I420|P010|LIMITED|FULL)) = (\w+)", hdr))
    assert found == {"PC_CTR_" + k: "PC_YUV_" + k for k in ("NV12", "I420", "P010", "LIMITED", "FULL")}
    # no atomics, no inline assembly, no LDS in the kernels
    assert not re.search(r"\batomic(Add|CAS|Exch|Max|Min|Or|And)\b|\basm\b|__asm|__shared__|__syncthreads", code)
    # a library of its own: the codec's source hash does not cover it
    import bench
    assert "clip_tol_rate" not in inspect.getsource(bench.source_hash) and "_hip" not in inspect.getsource(bench.source_hash)


def test_workspace_size_is_24_bytes_per_wave_and_entry():
    _, L = _lib()
    for size, n in [(64, 1), (64, 7), (128, 9), (512, 40), (576, 4), (1024, 3), (2048, 2)]:
        assert L.pc_clip_tol_rate_workspace_size(size, n) == TRC.workspace_size(size, n) == 96 * n * (size * size // 4096)
    for bad in [(0, 1), (32, 1), (96, 1), (-64, 1), (4096, 1), (64, 0), (64, -1), (2048, 2 ** 31 - 1)]:
        assert L.pc_clip_tol_rate_workspace_size(*bad) == 0, bad


def table_of(frames, fs):
    return (frames.Frame * len(fs))(*fs)


def test_plan_is_host_only_and_each_precondition_is_broken_alone():
    """made-up pointer values: nothing may be dereferenced or launched (there is no GPU here); pc_clip_rate_plan's rule"""
    from progressivecodec_amd import clip_rate, frames
    _, L = _lib()
    Fp = 0x7000_0100_0000
    H, W, st = 96, 160, (3 * T * T, T * T, T)

    def plan(fmt, fs, x=Fp, strides=st, O=0, n=None, fn=L.pc_clip_tol_rate_plan):
        wide = C.c_int(-1)
        tab = table_of(frames, fs) if fs else None
        rc = fn(x, *strides, O, frames.FORMATS.get(fmt, fmt), tab, len(fs) if n is None else n, C.byref(wide))
        return rc, wide.value
    for fmt in FC.FORMATS:
        es = 2 if fmt == "p010" else 1
        good = lambda: [fake_frame(frames, fmt, H, W), fake_frame(frames, fmt, H, W, base=0x7100_0000_1000, pad=4),      # noqa: E731
                        fake_frame(frames, fmt, H, W, base=0x7200_0000_1000, pad=8)]
        assert plan(fmt, good()) == (0, 1) and plan(fmt, good()[:1]) == (0, 1)
        cases = [dict(x=Fp + off) for off in (4, 8, 12)]
        for i in range(3):
            bad_st = list(st)
            bad_st[i] += 2
            cases.append(dict(strides=bad_st))
        cases += [dict(O=O) for O in (0, 8, 16, 32, 4, 12, 20, 28)]
        for kw in cases:
            got = plan(fmt, good(), **kw)
            assert got == plan(fmt, good(), fn=clip_rate.lib().pc_clip_rate_plan, **kw)          # the same rule
            assert got == (0, int(set(kw) == {"O"} and kw["O"] % 8 == 0)), (fmt, kw)
        for slot in range(3):
            for nm in ["y", "u"] + (["v"] if fmt == "i420" else []):
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
        assert plan(fmt, good(), x=None)[0] == -1
        assert L.pc_clip_tol_rate_plan(Fp, *st, 0, frames.FORMATS[fmt], table_of(frames, good()), 3, None) == -1
    assert plan(3, [fake_frame(frames, "nv12", H, W)])[0] == -1 and plan(-1, [fake_frame(frames, "nv12", H, W)])[0] == -1
    assert plan("nv12", [fake_frame(frames, "nv12", H, W)]) == (0, 1) and plan("i420", [fake_frame(frames, "nv12", H, W)])[0] == -1


def offsets(*vals):
    return (C.c_int32 * len(vals))(*vals)


def test_every_argument_error_returns_before_the_device():
    """fake device pointers: every call below must return PC_ERR_ARG without touching them (no GPU here)"""
    from progressivecodec_amd import frames
    _, L = _lib()
    Fp, Wk, S, Tl, Tb, Of, Sl = (0x7000_0100_0000, 0x7000_0200_0000, 0x7000_0300_0000, 0x7000_0400_0000, 0x7000_0500_0000, 0x7000_0600_0000,
                                 0x7000_0700_0000)
    H, W, O = 100, 150, 16                                                            # 2 x 3 tiles, S = 48
    k = frames.coefficients("bt709")
    for fmt in FC.FORMATS:
        fid = frames.FORMATS[fmt]

        def table(slot=None, field=None, value=None):
            fs = [fake_frame(frames, fmt, H, W), fake_frame(frames, fmt, H, W, base=0x7100_0000_1000, pad=3),
                  fake_frame(frames, fmt, H, W, base=0x7200_0000_1000)]
            if slot is not None:
                setattr(fs[slot], field, value)
            return table_of(frames, fs)
        bad_tables = [None]
        for slot in range(3):                                                         # a bad frame anywhere in the table
            bad_tables += [table(slot, "y", None), table(slot, "u", None), table(slot, "y_row", W - 1),
                           table(slot, "u_row", (2 * 75 if fmt != "i420" else 75) - 1)]
            if fmt == "i420":
                bad_tables += [table(slot, "v", None), table(slot, "v_row", 74)]
            if fmt == "p010":
                bad_tables += [table(slot, "y", 0x7000_0000_1001), table(slot, "u", 0x7000_0200_1001)]
        nbytes = L.pc_clip_tol_rate_workspace_size(T, 9)
        assert nbytes == 96 * 9
        ok = dict(x=Fp, sxt=3 * T * T, sxc=T * T, sxh=T, H=H, W=W, T=T, O=O, fmt=fid, range=0, kr=k.kr, kg=k.kg, kb=k.kb, ib=k.ib, ir=k.ir,
                  frames_host=table(), frames_dev=Tb, n_frames=3, tiles=Tl, offsets_host=offsets(0, 1, 3, 6, 7, 9), offsets_dev=Of, slots=Sl,
                  n_jobs=5, n_entries=9, ws=Wk, nbytes=nbytes, out=S, stream=None)
        bads = [dict(frames_host=t) for t in bad_tables] + [
            dict(H=0), dict(W=0), dict(H=-5), dict(T=0), dict(T=32), dict(T=96), dict(T=-64), dict(T=4096, O=0, sxt=3 * 4096 ** 2, sxc=4096 ** 2, sxh=4096),
            dict(O=2), dict(O=6), dict(O=36), dict(O=-4), dict(fmt=3), dict(fmt=-1), dict(range=2), dict(range=-1),
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
        if fmt == "p010":
            bads.append(dict(T=2048, O=0, sxt=3 * 2048 ** 2, sxc=2048 ** 2, sxh=2048, nbytes=L.pc_clip_tol_rate_workspace_size(2048, 9)))
        for bad in bads:
            assert L.pc_clip_tol_rate_sse_runs(*dict(ok, **bad).values()) == -1, (fmt, {k_: v for k_, v in bad.items() if k_ != "frames_host"})


# -- the contract --------------------------------------------------------------------------------------------------------------------

def test_frame_scale_is_the_lcm_of_the_denominators():
    from progressivecodec_amd import clip_tol_rate as ctr
    for fw, M, fwi in [((1, Fraction(1, 3), 0.5), 6, [6, 2, 3]), (None, 1, [1, 1, 1]), ((2, 4, 6), 1, [2, 4, 6]),
                       ((Fraction(3, 4), Fraction(5, 6), 7), 12, [9, 10, 84]), ((0.25, 0.125, 3), 8, [2, 1, 24]),
                       ((Fraction(2, 4), 1, 1), 2, [1, 2, 2])]:
        assert ctr.frame_scale(fw, 3) == (M, fwi) == TRC.frame_scale(fw, 3), fw
        assert all(isinstance(v, int) for v in ctr.frame_scale(fw, 3)[1])
    # a float is taken exactly: 0.1 is not 1/10
    M, fwi = ctr.frame_scale([0.1], 1)
    assert (M, fwi) == (2 ** 55, [Fraction(0.1).numerator]) == TRC.frame_scale([0.1], 1)
    for bad in ([1, 1], [1, 1, 1, 1], [1, 0, 1], [1, -1, 1], []):
        with pytest.raises(ValueError, match="frame_weights needs one positive number per frame, 3 in all"):
            ctr.frame_scale(bad, 3)
    items = [(0, 0), (0, 1), (0, 2), (2, 1)]
    assert ctr.item_importance(items, 3) == [1, 1, 1, 1] == TRC.weights(items)
    imp = [Fraction(1, 7), 10 ** 6, 0.1]
    got = ctr.item_importance(items, 3, imp)
    assert got == [Fraction(1, 7), 10 ** 6, Fraction(0.1), 10 ** 6] == TRC.weights(items, imp) and all(isinstance(v, Fraction) for v in got)
    for bad in ([1, 1], [1, 0, 1], [1, 1, -2]):
        with pytest.raises(ValueError, match="importance needs one positive number per tile, 3 in all"):
            ctr.item_importance(items, 3, bad)
    assert ctr.ClipTolRatePlan._fields == ("source", "items", "runs", "weights", "frame_scale", "levels", "rates", "dists", "plane_dists", "den",
                                           "container_bytes", "predicted", "sse", "n_coded", "n_reused", "stats", "worst")
    # decoding needs nothing new
    from progressivecodec_amd import clip_rate
    assert (ctr.decode_clip, ctr.frame_container, ctr.parse_clip) == (clip_rate.decode_clip, clip_rate.frame_container, clip_rate.parse_clip)
    assert ctr.Tolerance is __import__("progressivecodec_amd.clip_tol", fromlist=["Tolerance"]).Tolerance


def test_the_restatements_sums_on_a_hand_made_table():
    items, runs = RC2.items_of(SOURCE)
    assert runs == [[0], [0, 1, 2], [0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2], [0, 1, 2, 3], [1, 2, 3], [3], [3]]
    # plane_dists[i][l][j][p]: every (item, level, frame, plane) its own number
    pd = [[[[1000 * i + 100 * l + 10 * k + p for p in range(3)] for k in run] for l in range(2)] for i, run in enumerate(runs)]
    levels = [0, 1, 0, 1, 0, 1, 0, 1, 1]
    at = lambda i, k: pd[i][levels[i]][runs[i].index(k)]                              # noqa: E731
    sse = TRC.frame_sse(SOURCE, pd, levels)
    assert sse[0] == [sum(at(i, 0)[p] for i in range(6)) for p in range(3)]
    assert sse[2] == [sum(at(i, 2)[p] for i in (6, 1, 2, 3, 4, 5)) for p in range(3)]
    assert sse[3] == [sum(at(i, 3)[p] for i in (6, 7, 2, 3, 8, 5)) for p in range(3)]
    assert sse[1] != sse[2]                                                          # the same items, measured against another frame
    assert TRC.predicted(pd, levels) == sum(sum(row) for row in sse)
    assert TRC.predicted(pd, levels, (1, 0, 2)) == sum(row[0] + 2 * row[2] for row in sse)
    d = TRC.dists(pd, runs, (1, 2, 3), (1, Fraction(1, 3), 0.5, 2), 4)                # M = 6
    assert d[1][1] == sum(w * (v[0] + 2 * v[1] + 3 * v[2]) for w, v in zip((6, 2, 3), pd[1][1]))
    assert d[7][0] == 12 * (pd[7][0][0][0] + 2 * pd[7][0][0][1] + 3 * pd[7][0][0][2])
    assert TRC.dists(pd, runs)[2][0] == sum(sum(v) for v in pd[2][0])
    assert TRC.offsets_of(runs) == [0, 1, 4, 8, 12, 15, 19, 22, 23, 24]
    jobs, owner = TRC.expanded([t for _, t in items], runs)
    assert jobs[:5] == [(0, 0), (0, 1), (1, 1), (2, 1), (0, 2)] and owner[:5] == [0, 1, 1, 1, 2] and len(jobs) == 24
    assert TRC.container_bytes([[5, 9]] * 9, levels, 4, 6) == 42 + 16 * 24 + 4 * 5 + 5 * 9


def test_the_scaled_allocation_is_clip_rates():
    """Under the reuse identity every plane_dists[i][l][j] of a run is equal, so weights * dists of section 20 is M times section
    17's for every item; rate.allocate is invariant under that uniform scale: the levels are clip_rate's, on the restatement and on
    the module's allocator."""
    from progressivecodec_amd import rate
    g = np.random.default_rng(20)
    for trial in range(40):
        n, nl, F = int(g.integers(1, 9)), int(g.integers(1, 5)), int(g.integers(1, 6))
        runs = []
        for _ in range(n):
            first = int(g.integers(0, F))
            runs.append(list(range(first, int(g.integers(first, F)) + 1)))
        items = [(run[0], i) for i, run in enumerate(runs)]
        rates = [sorted(int(v) for v in g.integers(1, 2000, nl)) for _ in range(n)]
        base = [sorted((int(v) for v in g.integers(0, 10 ** 9, nl)), reverse=True) for _ in range(n)]      # D(f, t) per level
        if trial % 3 == 0:
            g.shuffle(base[0])                                                        # a level that is not on the hull
        fw = [Fraction(int(g.integers(1, 9)), int(g.integers(1, 9))) for _ in range(F)] if trial % 2 else None
        imp = [Fraction(int(g.integers(1, 50)), int(g.integers(1, 50))) for _ in range(n)] if trial % 4 < 2 else None
        # section 17: the item's weight is importance times the frame weights summed over its run, its distortion D(f, t)
        w17 = [(Fraction(1) if imp is None else imp[t]) * sum((Fraction(1) if fw is None else fw[k]) for k in run) for (_, t), run in zip(items, runs)]
        # section 20: the distortion is summed over the run with the integer frame weights, the weight is the importance alone
        pd = [[[[d, 0, 0] for _ in run] for d in base[i]] for i, run in enumerate(runs)]
        d20 = TRC.dists(pd, runs, (1, 1, 1), fw, F)
        w20 = TRC.weights(items, imp)
        M = TRC.frame_scale(fw, F)[0]
        for i in range(n):
            for l in range(nl):
                assert w20[i] * d20[i][l] == M * w17[i] * base[i][l]
        lo, hi = sum(min(r) for r in rates), sum(max(r) for r in rates)
        for budget in {lo, (lo + hi) // 2, lo + (hi - lo) // 3, hi, hi + 5}:
            want = RC.allocate(rates, base, budget, w17)
            assert RC.allocate(rates, d20, budget, w20) == want, (trial, budget)
            assert rate.allocate(rates, d20, budget, w20) == want == rate.allocate(rates, base, budget, w17), (trial, budget)


# -- the Python layer ----------------------------------------------------------------------------------------------------------------

def _no_device(monkeypatch):
    from progressivecodec_amd import clip_rate, clip_tol, clips
    from progressivecodec_amd import clip_tol_rate as ctr

    def touched(*a, **k):
        raise AssertionError("the device was reached")
    for name in ("device", "current_stream", "synchronize", "current_device", "_lazy_init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    for mod in (ctr, clip_rate, clip_tol, clips):
        monkeypatch.setattr(mod, "lib", touched)
    monkeypatch.setattr(ctr, "_scan", touched)
    return ctr


def test_python_rejects_before_any_device_call(monkeypatch):
    ctr = _no_device(monkeypatch)
    from progressivecodec_amd.tiles import grid_of
    y, uv, u = torch.zeros(100, 150, dtype=torch.uint8), torch.zeros(50, 75, 2, dtype=torch.uint8), torch.zeros(50, 75, dtype=torch.uint8)
    f = (y, uv)
    g = grid_of(100, 150, 64, 16)
    x = torch.zeros(2, 3, 64, 64)
    # CPU tensors
    with pytest.raises(ValueError, match="GPU"):
        ctr.tile_distortion_runs(x, g, [f, f], [0, 5], [[0], [1, 0]], "nv12")
    with pytest.raises(ValueError, match="GPU"):
        ctr.tile_distortion_runs(x, g, [(y, u, u)], [0, 5], [[0], [0]], "i420")
    with pytest.raises(ValueError, match="GPU"):
        ctr.tile_distortion_runs(x, g, (torch.stack([y, y]), torch.stack([uv, uv])), [0, 5], [[0, 1], [1]], "nv12")
    for kw in (dict(), dict(tolerance=ctr.Tolerance(1))):
        with pytest.raises(ValueError, match="GPU"):
            ctr.encode_clip_to_size(None, [f, f], [0, 1], 10 ** 6, "nv12", tile=64, **kw)
    # enums, the grid and the tile limit come before the frames
    with pytest.raises(ValueError, match="fmt"):
        ctr.tile_distortion_runs(x, g, [f], [0], [[0]], "nv21")
    with pytest.raises(ValueError, match="matrix"):
        ctr.tile_distortion_runs(x, g, [f], [0], [[0]], "nv12", matrix="bt470")
    with pytest.raises(ValueError, match="range"):
        ctr.tile_distortion_runs(x, g, [f], [0], [[0]], "nv12", range="tv")
    with pytest.raises(ValueError, match="the grid of a 100x150 frame is 2x3"):
        ctr.tile_distortion_runs(x, g._replace(nx=4), [f], [0], [[0]], "nv12")
    with pytest.raises(ValueError, match="at most 1024"):
        ctr.tile_distortion_runs(x, grid_of(100, 150, 2048, 0), [f], [0], [[0]], "p010")
    # clip_rate.encode_clip_to_size's checks, word for word
    for kw, msg in [(dict(fmt="nv21"), "fmt"), (dict(matrix="bt470"), "matrix"), (dict(range="tv"), "range"), (dict(upsample="cubic"), "upsample"),
                    (dict(max_tiles_per_call=0), "max_tiles_per_call must be at least 1"), (dict(qualities=[]), "at least one level"),
                    (dict(plane_weights=(1, 1)), "plane_weights"), (dict(plane_weights=(0, 0, 0)), "plane_weights"),
                    (dict(plane_weights=(1, 0.5, 1)), "plane_weights"), (dict(plane_weights=(1, -1, 1)), "plane_weights")]:
        a = dict(dict(qualities=[0, 1], target_bytes=10 ** 6, fmt="nv12"), **kw)
        with pytest.raises(ValueError, match=msg):
            ctr.encode_clip_to_size(None, [f], a.pop("qualities"), a.pop("target_bytes"), a.pop("fmt"), **a)
    for bad in ([], (), None, "clip"):
        with pytest.raises(ValueError, match="non-empty list"):
            ctr.encode_clip_to_size(None, bad, [0], 10 ** 6, "nv12")
    with pytest.raises(ValueError, match="got one frame"):
        ctr.encode_clip_to_size(None, f, [0], 10 ** 6, "nv12")


def test_python_checks_that_need_a_frame_that_passes(monkeypatch):
    """the checks behind the frame's own: with the frames' device test out of the way, nothing else may reach the device"""
    ctr = _no_device(monkeypatch)
    from progressivecodec_amd import clip_rate
    from progressivecodec_amd.tiles import grid_of
    y, uv = torch.zeros(100, 150, dtype=torch.uint8), torch.zeros(50, 75, 2, dtype=torch.uint8)
    f = (y, uv)
    passes = lambda fr, fmt, what="frames": ([[t.unsqueeze(0) for t in p] for p in fr], fr[0][0].shape[0], fr[0][0].shape[1])      # noqa: E731
    monkeypatch.setattr(ctr, "_clip_frames", passes)
    monkeypatch.setattr(clip_rate, "_clip_frames", passes)
    g = grid_of(100, 150, 64, 16)
    x = torch.zeros(2, 3, 64, 64)
    # tiles and runs are validated on the host before anything is uploaded
    for tiles, runs, msg in [([], [], "at least one tile"), ([0, 1], [[0]], "one list of frames per tile, 2 in all"), ([0], [[0], [1]], "one list of frames per tile"),
                             ([0, 6], [[0], [0]], "lies outside"), ([0, -1], [[0], [0]], "lies outside"), ([0, 1], [[0], [2]], "lies outside"),
                             ([0, 1], [[0], [0, -1]], "lies outside"), ([0, 1.0], [[0], [0]], "a tile is an int"), ([0, True], [[0], [0]], "a tile is an int"),
                             ([0, (1,)], [[0], [0]], "a tile is an int"), ([0, 1], [[0], []], "non-empty list"), ([0, 1], [[0], 1], "non-empty list"),
                             ([0, 1], [[0], [0.0]], "non-empty list"), ([0, 1], [[0], [True]], "non-empty list"), ([0, 1], [[0], None], "non-empty list"),
                             ([0, 1], [[0], ["1"]], "non-empty list"), (torch.tensor([0, 6]), [[0], [1]], "lies outside")]:
        with pytest.raises(ValueError, match=msg):
            ctr.tile_distortion_runs(x, g, [f, f], tiles, runs, "nv12")
    with pytest.raises(ValueError, match="one tile per entry of tiles"):
        ctr.tile_distortion_runs(x, g, [f, f], [0], [[0, 1]], "nv12")
    with pytest.raises(ValueError, match="one tile per entry of tiles"):
        ctr.tile_distortion_runs(x[0], g, [f, f], [0], [[0]], "nv12")
    small = (torch.zeros(64, 64, dtype=torch.uint8), torch.zeros(32, 32, 2, dtype=torch.uint8))
    with pytest.raises(ValueError, match="frames must be 100x150 frames"):
        ctr.tile_distortion_runs(x[:1], g, [small], [0], [[0]], "nv12")
    enc = lambda fmt="nv12", **kw: ctr.encode_clip_to_size(None, [f, f, f], [0, 1], 10 ** 6, fmt, **dict(dict(tile=64, overlap=16), **kw))     # noqa: E731
    with pytest.raises(ValueError, match="multiple of 64"):
        enc(tile=96)
    with pytest.raises(ValueError, match="overlap"):
        enc(overlap=6)
    with pytest.raises(ValueError, match="at most 2048"):
        enc(tile=4096, overlap=0)
    with pytest.raises(ValueError, match="at most 1024"):
        enc("p010", tile=2048, overlap=0)
    for imp in ([1] * 5, [[1, 1, 1], [1, 1]], [1] * 7):
        with pytest.raises(ValueError, match="importance needs one number per tile of the 2x3 grid"):
            enc(importance=imp)
    for fw in ([1, 1], [1] * 4, []):
        with pytest.raises(ValueError, match="frame_weights needs one number per frame"):
            enc(frame_weights=fw)
    # the tolerance, and the weights' signs: refused before the scan
    for tol in (None, 1, (1, 1, 1), "loose", dict(max_abs=1)):
        with pytest.raises(ValueError, match="tolerance must be a clip_tol.Tolerance"):
            enc(tolerance=tol)
    with pytest.raises(ValueError, match="max_abs must be at most 255"):
        enc(tolerance=ctr.Tolerance(256))
    with pytest.raises(ValueError, match="max_abs must be at most 255"):
        enc(tolerance=ctr.Tolerance((0, 0, 1023)))
    for fw in ([1, 0, 1], [1, 1, -1]):
        with pytest.raises(ValueError, match="frame_weights needs one positive number per frame, 3 in all"):
            enc(frame_weights=fw)
    for imp in ([1, 1, 1, 0, 1, 1], [[1, 1, 1], [1, -1, 1]]):
        with pytest.raises(ValueError, match="importance needs one positive number per tile, 6 in all"):
            enc(importance=imp)
    with pytest.raises(AssertionError, match="the device was reached"):             # nothing above is wrong with good arguments
        enc(tolerance=ctr.Tolerance(1), frame_weights=[1, Fraction(1, 3), 0.5], importance=[1] * 6)

"""Tolerant clips without a GPU: the restatement of DESIGN.md section 18 (tests/clip_tol_contract.py) on hand-made code arrays;
clip_tol.Tolerance's argument checks; libpc_clip_tol.so's C ABI up to the first device call; and progressivecodec_amd.clip_tol's
refusals.  Every comparison is exact equality of integers."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import clip_tol_contract as TOL
from tests import clips_contract as CC
from tests import frames_contract as FC
from tests import image_shared
from tests import tiles_contract as TC
from tests.test_frames_host import fake_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 64
NO = TOL.NO_MSE


def _lib():
    from progressivecodec_amd import clip_tol
    return clip_tol, clip_tol.lib()


def flat_codes(H, W, value):
    Hc, Wc = FC.chroma_size(H, W)
    return [np.full((1, H, W), value, np.int64), np.full((1, Hc, Wc), value, np.int64), np.full((1, Hc, Wc), value, np.int64)]


def random_codes(H, W, fmt, seed, lo=0, hi=None):
    g = np.random.default_rng(seed)
    Hc, Wc = FC.chroma_size(H, W)
    hi = (1 << FC.bits(fmt)) if hi is None else hi
    return [g.integers(lo, hi, s, dtype=np.int64) for s in ((1, H, W), (1, Hc, Wc), (1, Hc, Wc))]


# -- the restatement -------------------------------------------------------------------------------------------------------------------

def test_tolerance_zero_is_section_16s_source_table():
    from progressivecodec_amd import clips
    for fmt, (H, W), O, up in [("nv12", (100, 150), 16, "linear"), ("i420", (127, 129), 0, "nearest"), ("p010", (65, 63), 4, "linear")]:
        g = np.random.default_rng(H + O)
        base = random_codes(H, W, fmt, 1)
        clip = [FC.frame(*base, fmt)]
        for k in range(1, 6):
            nxt = [np.array(c) for c in FC.codes(clip[-1], fmt)]
            if k != 3:                                                               # frame 3 repeats frame 2
                p = k % 3
                y, x = g.integers(0, nxt[p].shape[1]), g.integers(0, nxt[p].shape[2])
                nxt[p][0, y, x] ^= 1
            clip.append(FC.frame(*nxt, fmt))
        n = int(np.prod(TC.grid(H, W, T, O)))
        changed = [[c != [0, 0, 0] for c in CC.tile_changes(clip[k], clip[k - 1], fmt, T, O, up)] for k in range(1, 6)]
        want = clips.source_table(changed)
        source, stats = TOL.scan(clip, fmt, T, O, up)
        assert source == want == CC.source_table(clip, fmt, T, O, up)
        assert any(s == k for k, row in enumerate(source[1:], 1) for s in row) and any(s != k for k, row in enumerate(source[1:], 1) for s in row)
        assert source[3] == source[2] and stats[0] == [[[0, 0, 0]] * 3] * n
        # a count is section 16's number wherever the anchor is the previous frame
        for k in range(1, 6):
            cnt = CC.tile_changes(clip[k], clip[k - 1], fmt, T, O, up)
            for t in range(n):
                if source[k - 1][t] == k - 1:
                    assert [s[0] for s in stats[k][t]] == cnt[t]


def test_ramp_is_judged_against_the_anchor_not_the_previous_frame():
    H, W = 100, 150
    for fmt, O, up in [("nv12", 16, "linear"), ("p010", 0, "nearest"), ("i420", 4, "linear")]:
        clip = [FC.frame(*flat_codes(H, W, 100 + k), fmt) for k in range(7)]         # away from 0 and from the top code
        n = int(np.prod(TC.grid(H, W, T, O)))
        source, stats = TOL.scan(clip, fmt, T, O, up, max_abs=(2, 2, 2))
        assert source == [[v] * n for v in [0, 0, 0, 3, 3, 3, 6]]
        for k, v in enumerate([0, 1, 2, 3, 1, 2, 3]):
            ns = TOL.nsamp(0, H, W, T, O, up)
            assert stats[k][0] == [[ns[p] if v else 0, v * v * ns[p], v] for p in range(3)]
        assert TOL.worst(source, stats) == [2, 2, 2]
        prev, _ = TOL.scan(clip, fmt, T, O, up, max_abs=(2, 2, 2), against_previous=True)
        assert prev == [[0] * n] * 7 and prev != source                              # the rule the contract rejects drifts for ever
        # one plane alone is enough to recode
        for p in range(3):
            ma = [6, 6, 6]
            ma[p] = 2
            assert TOL.scan(clip, fmt, T, O, up, max_abs=ma)[0] == source


def test_mse_boundary_is_exact_cross_multiplication():
    H = W = 64                                                                       # one tile, luma nsamp = 4096
    assert TOL.nsamp(0, H, W, T, 0, "linear") == [4096, 1024, 1024]
    base = flat_codes(H, W, 50)
    f0 = FC.frame(*base, "nv12")

    def off(n_luma, n_cb=0):
        c = [np.array(p) for p in base]
        c[0].reshape(-1)[[5, 77, 1000, 4095, 2048][:n_luma]] += 1
        c[1].reshape(-1)[:n_cb] -= 1
        return FC.frame(*c, "nv12")
    kw = dict(max_abs=(3, 3, 3), q10=(1, 1, 1))
    source, stats = TOL.scan([f0, off(4)], "nv12", T, 0, "linear", **kw)
    assert stats[1][0][0] == [4, 4, 1] and 1024 * 4 == 1 * 4096 and source[1] == [0]  # equality: reused
    source, stats = TOL.scan([f0, off(5)], "nv12", T, 0, "linear", **kw)
    assert stats[1][0][0] == [5, 5, 1] and source[1] == [1]                           # one more: recoded
    # chroma: nsamp = 1024, so one sample off by 1 is the boundary there
    assert TOL.scan([f0, off(0, 1)], "nv12", T, 0, "linear", **kw)[0][1] == [0]
    assert TOL.scan([f0, off(0, 2)], "nv12", T, 0, "linear", **kw)[0][1] == [1]
    # mse_q10 = 0 admits no difference; 2^30 never binds
    assert TOL.scan([f0, off(1)], "nv12", T, 0, "linear", max_abs=(3, 3, 3), q10=(0, 0, 0))[0][1] == [1]
    far = FC.frame(*flat_codes(H, W, 255), "nv12")
    zero = FC.frame(*flat_codes(H, W, 0), "nv12")
    assert TOL.scan([zero, far], "nv12", T, 0, "linear", max_abs=(255, 255, 255))[0][1] == [0]
    assert 1024 * 1023 ** 2 < NO and TOL.mse_q10(None) == NO == 2 ** 30


def test_max_abs_boundary_is_exact():
    H, W = 65, 63
    for fmt, a in [("nv12", 3), ("p010", 700), ("i420", 0)]:
        base = random_codes(H, W, fmt, 5, lo=0, hi=(1 << FC.bits(fmt)) - a - 1)
        f0 = FC.frame(*base, fmt)
        for p in range(3):
            for d, reused in [(a, True), (a + 1, False)]:
                c = [np.array(q) for q in base]
                c[p][0, 0, 0] += d
                source, stats = TOL.scan([f0, FC.frame(*c, fmt)], fmt, T, 0, "linear", max_abs=(a, a, a))
                if d == 0:
                    assert source[1] == [0, 0] and stats[1][0][p] == [0, 0, 0]
                    continue
                assert stats[1][0][p] == [1, d * d, d]
                assert source[1][0] == (0 if reused else 1) and source[1][1] == 0, (fmt, p, d)


def test_max_run_limits_the_frames_one_coded_tile_is_shown_in():
    f = FC.frame(*random_codes(100, 150, "nv12", 2), "nv12")
    clip = [f] * 7
    for run, col in [(0, [0] * 7), (1, list(range(7))), (2, [0, 0, 2, 2, 4, 4, 6]), (3, [0, 0, 0, 3, 3, 3, 6]), (7, [0] * 7), (6, [0] * 6 + [6])]:
        source, stats = TOL.scan(clip, "nv12", T, 16, "linear", max_run=run)
        assert source == [[v] * 6 for v in col], run
        assert stats == [[[[0, 0, 0]] * 3] * 6] * 7                                   # recoded by the run alone: the evidence is zero
    assert TOL.scan(clip, "nv12", T, 16, "linear", max_run=1)[0] == [[k] * 6 for k in range(7)]       # reuse=False


def test_p010_low_six_bits_are_ignored():
    base = random_codes(65, 63, "p010", 9)
    f0 = FC.frame(*base, "p010")
    g = np.random.default_rng(3)
    f1 = tuple(p | g.integers(0, 64, p.shape).astype(np.uint16) for p in f0)
    assert any((a != b).any() for a, b in zip(f0, f1))
    source, stats = TOL.scan([f0, f1, f0], "p010", T, 4, "linear")
    assert source == [[0, 0]] * 3 and stats == [[[[0, 0, 0]] * 3] * 2] * 3


def test_halo_belongs_to_the_footprint_under_linear_only():
    H, W, O = 100, 150, 16
    base = flat_codes(H, W, 90)
    f0 = FC.frame(*base, "nv12")
    c = [np.array(p) for p in base]
    c[1][0, 23, 40] += 9                                                             # the chroma row above tile (1, 1): S / 2 - 1 = 23
    f1 = FC.frame(*c, "nv12")
    assert TOL.scan([f0, f1], "nv12", T, O, "linear")[0][1] == [0, 1, 0, 0, 1, 0]
    assert TOL.scan([f0, f1], "nv12", T, O, "nearest")[0][1] == [0, 1, 0, 0, 0, 0]
    assert TOL.nsamp(4, H, W, T, O, "linear") == [52 * 64, 27 * 34, 27 * 34] and TOL.nsamp(4, H, W, T, O, "nearest") == [52 * 64, 26 * 32, 26 * 32]


# -- Tolerance -------------------------------------------------------------------------------------------------------------------------

def test_tolerance_arguments():
    ct, _ = _lib()
    Tl = ct.Tolerance
    assert Tl() == ((0, 0, 0), (NO, NO, NO), 0) and ct.NO_MSE == NO
    assert Tl(2) == ((2, 2, 2), (NO,) * 3, 0) and Tl((1, 2, 3), max_run=4) == ((1, 2, 3), (NO,) * 3, 4)
    assert Tl(max_mse=0.1).mse_q10 == (102, 102, 102) and Fraction(0.1) * 1024 > 102 and TOL.mse_q10(0.1) == 102
    assert Tl(max_mse=Fraction(1, 1024)).mse_q10 == (1, 1, 1) and Tl(max_mse=Fraction(1, 1025)).mse_q10 == (0, 0, 0)
    assert Tl(max_mse=(1, None, 2.5)).mse_q10 == (1024, NO, 2560) and Tl(max_mse=0).mse_q10 == (0, 0, 0)
    assert Tl(max_mse=2 ** 20).mse_q10 == (NO,) * 3 and Tl(1023).max_abs == (1023,) * 3 and Tl(max_run=1).max_run == 1
    assert Tl(1, 0.5, 3).max_abs == (1, 1, 1) and Tl(max_abs=[0, 1, 0]).max_abs == (0, 1, 0)
    for kw in [dict(max_abs=-1), dict(max_abs=1024), dict(max_abs=1.0), dict(max_abs=True), dict(max_abs=(1, 2)), dict(max_abs=(1, 2, -3)),
               dict(max_abs=None), dict(max_mse=-0.001), dict(max_mse=2 ** 20 + 1), dict(max_mse="x"), dict(max_mse=(1, 2)),
               dict(max_mse=float("nan")), dict(max_mse=float("inf")), dict(max_mse=True), dict(max_run=0), dict(max_run=-1),
               dict(max_run=1.5), dict(max_run=True), dict(max_run=2 ** 31)]:
        with pytest.raises(ValueError, match="max_abs|max_mse|max_run"):
            Tl(**kw)
    assert ct.ClipTolPlan._fields == ("source", "n_coded", "n_reused", "container_bytes", "stats", "worst")


# -- the library, no device ----------------------------------------------------------------------------------------------------------

def test_library_exports_every_declared_function():
    ct, L = _lib()
    hdr = open(os.path.join(ROOT, "progressivecodec_amd", "clip_tol_csrc", "pc_clip_tol.h")).read()
    declared = re.findall(r"PC_API\s+[\w\s\*]+?\b(pc_\w+)\s*\(", hdr)
    assert len(declared) == 5 and sorted(declared) == sorted(ct.EXPORTS)
    for name in declared:
        getattr(L, name)
    assert L.pc_clip_tol_strerror(-1).decode() and L.pc_clip_tol_strerror(-6).decode() and L.pc_clip_tol_last_hip_error() == 0
    # a library of its own: no other library of the project is linked, and the codec's source hash does not cover it
    import bench
    import inspect
    assert "clip_tol" not in inspect.getsource(bench.source_hash)
    mk = image_shared.build_rule("clip_tol")                                             # image_csrc/lib.mk, which the library's Makefile includes
    assert mk == image_shared.build_rule("clip_rate")                                # clip_rate_csrc's rule and flags: the same file
    assert "-ffp-contract=off" in mk and "--offload-arch=$(ARCH)" in mk and "-fvisibility=hidden" in mk
    assert not re.search(r"-lpc|libpc(odec|_pixels|_tiles|_rate|_metrics|_frames|_frame_tiles|_frame_rate|_clips|_clip_rate)\b", mk)
    top = open(os.path.join(ROOT, "progressivecodec_amd", "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\bclip_tol\b", top, re.M) and re.search(r"^\.PHONY:.*\bclip_tol\b", top, re.M)
    assert "$(MAKE) -C ../clip_tol_csrc clean" in top and re.search(r"^clip_tol:\n\t\$\(MAKE\) -C \.\./clip_tol_csrc$", top, re.M)
    # the frame is the one record of image_csrc/pc_yuv_frame.h, as pc_frames.h's is: frames.Frame serves this library, too
    image_shared.assert_frame_is_shared(hdr, "pc_ct_frame")
    # no atomics, no inline assembly in the kernels
    src = open(os.path.join(ROOT, "progressivecodec_amd", "clip_tol_csrc", "pc_clip_tol.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\batomic(Add|CAS|Exch|Max|Min|Or|And)\b|\basm\b|__asm", code)


def test_workspace_size_is_72_bytes_per_block_and_4_per_tile():
    _, L = _lib()
    for size, n in [(64, 1), (64, 6), (64, 7), (128, 9), (512, 40), (1024, 3), (2048, 2), (2048, 5)]:
        want = (72 * n * (size * size // 4096 + 1) + 4 * n + 7) // 8 * 8
        assert L.pc_clip_tol_workspace_size(size, n) == want == TOL.workspace_size(size, n) and want % 8 == 0, (size, n)
    assert L.pc_clip_tol_workspace_size(64, 1) == 152 and L.pc_clip_tol_workspace_size(64, 6) == 888
    for bad in [(0, 1), (32, 1), (96, 1), (-64, 1), (4096, 1), (64, 0), (64, -1), (2048, 2 ** 31 - 1)]:
        assert L.pc_clip_tol_workspace_size(*bad) == 0, bad


def table_of(frames, fs):
    return (frames.Frame * len(fs))(*fs)


def test_plan_is_host_only_and_each_precondition_is_broken_alone():
    """made-up pointer values: nothing may be dereferenced or launched (there is no GPU here).  Every frame of the table has to
    allow the wide path, wherever in the table it stands."""
    from progressivecodec_amd import frames
    _, L = _lib()
    H, W = 96, 160

    def plan(fmt, fs, O=0, n=None):
        wide = C.c_int(-1)
        tab = table_of(frames, fs) if fs else None
        rc = L.pc_clip_tol_plan(frames.FORMATS.get(fmt, fmt), tab, len(fs) if n is None else n, O, C.byref(wide))
        return rc, wide.value
    for fmt in FC.FORMATS:
        es = 2 if fmt == "p010" else 1
        good = lambda: [fake_frame(frames, fmt, H, W), fake_frame(frames, fmt, H, W, base=0x7100_0000_1000, pad=4),      # noqa: E731
                        fake_frame(frames, fmt, H, W, base=0x7200_0000_1000, pad=8)]
        assert plan(fmt, good()) == (0, 1) and plan(fmt, good()[:1]) == (0, 1)
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
        for O, wide in [(0, 1), (8, 1), (16, 1), (32, 1), (4, 0), (12, 0), (20, 0), (28, 0)]:
            assert plan(fmt, good(), O=O) == (0, wide), (fmt, O)
        assert plan(fmt, good(), O=-4)[0] == -1 and plan(fmt, [])[0] == -1 and plan(fmt, good(), n=0)[0] == -1 and plan(fmt, good(), n=-1)[0] == -1
        assert L.pc_clip_tol_plan(frames.FORMATS[fmt], table_of(frames, good()), 3, 0, None) == -1
    assert plan(3, [fake_frame(frames, "nv12", H, W)])[0] == -1 and plan(-1, [fake_frame(frames, "nv12", H, W)])[0] == -1
    assert plan("nv12", [fake_frame(frames, "nv12", H, W)]) == (0, 1) and plan("i420", [fake_frame(frames, "nv12", H, W)])[0] == -1


def test_every_argument_error_returns_before_the_device():
    """fake device pointers: every call below must return PC_ERR_ARG without touching them (no GPU here)"""
    from progressivecodec_amd import frames
    _, L = _lib()
    Wk, Sr, St, Tb = 0x7000_0200_0000, 0x7000_0300_0000, 0x7000_0400_0000, 0x7000_0500_0000
    H, W, O = 100, 150, 16                                                            # 2 x 3 tiles, S = 48
    i3 = lambda *v: (C.c_int * 3)(*v)                                                 # noqa: E731
    for fmt in FC.FORMATS:
        fid = frames.FORMATS[fmt]
        top = 1023 if fmt == "p010" else 255

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
        nbytes = L.pc_clip_tol_workspace_size(T, 6)
        ok = dict(frames_host=table(), frames_dev=Tb, n_frames=3, fmt=fid, up=1, H=H, W=W, T=T, O=O, max_abs=i3(1, top, 0), mse_q10=i3(0, NO, 5),
                  max_run=2, ws=Wk, nbytes=nbytes, source=Sr, stats=St, stream=None)
        bads = [dict(frames_host=t) for t in bad_tables] + [
            dict(H=0), dict(W=0), dict(H=-5), dict(T=0), dict(T=32), dict(T=96), dict(T=-64), dict(T=4096, O=0),
            dict(O=2), dict(O=6), dict(O=36), dict(O=-4), dict(fmt=3), dict(fmt=-1), dict(up=2), dict(up=-1),
            dict(frames_dev=None), dict(frames_dev=Tb + 4), dict(n_frames=0), dict(n_frames=-1),
            dict(max_abs=None), dict(mse_q10=None), dict(max_abs=i3(0, 0, -1)), dict(max_abs=i3(top + 1, 0, 0)), dict(max_abs=i3(0, top + 1, 0)),
            dict(mse_q10=i3(-1, 0, 0)), dict(mse_q10=i3(0, 0, NO + 1)), dict(mse_q10=i3(0, -2 ** 31, 0)), dict(max_run=-1),
            dict(ws=None), dict(ws=Wk + 4), dict(nbytes=nbytes - 1), dict(nbytes=0), dict(nbytes=L.pc_clip_tol_workspace_size(T, 5)),
            dict(source=None), dict(source=Sr + 2), dict(stats=None), dict(stats=St + 4)]
        for bad in bads:
            assert L.pc_clip_tol_scan(*dict(ok, **bad).values()) == -1, (fmt, {k_: v for k_, v in bad.items() if k_ != "frames_host"})


def test_python_rejects_before_any_device_call(monkeypatch):
    from progressivecodec_amd import clip_tol as ct
    from progressivecodec_amd import clips

    def touched(*a, **k):
        raise AssertionError("the device was reached")
    for name in ("device", "current_stream", "synchronize", "current_device", "_lazy_init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.setattr(ct, "lib", touched)
    monkeypatch.setattr(clips, "lib", touched)
    y, uv, u = torch.zeros(100, 150, dtype=torch.uint8), torch.zeros(50, 75, 2, dtype=torch.uint8), torch.zeros(50, 75, dtype=torch.uint8)
    f = (y, uv)
    tol = ct.Tolerance(1)
    # CPU tensors
    for frames, fmt in [([f, f], "nv12"), ([(y, u, u)], "i420"), ((torch.stack([y, y]), torch.stack([uv, uv])), "nv12")]:
        with pytest.raises(ValueError, match="GPU"):
            ct.scan_clip(frames, fmt, tol, tile=64)
        with pytest.raises(ValueError, match="GPU"):
            ct.encode_clip(None, frames, [0, 1], fmt, tile=64, tolerance=tol)
    # enums and the tolerance come before the frames
    for kw, msg in [(dict(fmt="nv21"), "fmt"), (dict(upsample="cubic"), "upsample"), (dict(tolerance=None), "Tolerance"), (dict(tolerance=1), "Tolerance"),
                    (dict(tolerance=(0, 0, 0)), "Tolerance"), (dict(tolerance=ct.Tolerance(256)), "at most 255")]:
        a = dict(dict(fmt="nv12", tolerance=tol), **kw)
        fmt_, tol_ = a.pop("fmt"), a.pop("tolerance")
        with pytest.raises(ValueError, match=msg):
            ct.scan_clip([f], fmt_, tol_, **a)
        with pytest.raises(ValueError, match=msg):
            ct.encode_clip(None, [f], [0], fmt_, tolerance=tol_, **a)
    for kw, msg in [(dict(matrix="bt470"), "matrix"), (dict(range="tv"), "range"), (dict(max_tiles_per_call=0), "max_tiles_per_call")]:
        with pytest.raises(ValueError, match=msg):
            ct.encode_clip(None, [f], [0], "nv12", tolerance=tol, **kw)
    for bad in ([], (), None, "clip"):
        with pytest.raises(ValueError, match="non-empty list"):
            ct.scan_clip(bad, "nv12", tol)
    with pytest.raises(ValueError, match="got one frame"):
        ct.scan_clip(f, "nv12", tol)
    # the grid, with the frames' device test out of the way
    monkeypatch.setattr(ct, "_clip_frames", lambda fr, fmt, what="frames": ([[t.unsqueeze(0) for t in p] for p in fr], fr[0][0].shape[0], fr[0][0].shape[1]))
    for kw, msg in [(dict(tile=96), "multiple of 64"), (dict(overlap=6), "overlap"), (dict(tile=4096), "at most 2048")]:
        with pytest.raises(ValueError, match=msg):
            ct.scan_clip([f, f], "nv12", tol, **kw)
        with pytest.raises(ValueError, match=msg):
            ct.encode_clip(None, [f, f], [0], "nv12", tolerance=tol, **kw)

"""Tolerant clips of YUV frames of any subsampling and siting without a GPU: the restatement of DESIGN.md section 29
(tests/chroma_clip_tol_contract.py) against section 18's and section 25's restatements and on hand-made code arrays;
libpc_chroma_clip_tol.so's C ABI up to the first device call; progressivecodec_amd.chroma_clip_tol's refusals; the structure of the
seventeenth image-side library; the ledger of kernel instantiations; and encode_clip against a fake model.  Every comparison is exact
equality of integers or bytes."""
import ctypes as C
import glob
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests import chroma_clip_tol_cases as CS
from tests import chroma_clip_tol_contract as TOL
from tests import chroma_clips_contract as CK
from tests import chroma_contract as CC
from tests import clip_tol_contract as TOL18
from tests import frames_contract as FC
from tests import image_shared
from tests import tiles_contract as TC
from tests.test_chroma_host import fake_frame
from tests.test_image_shared_host import DEFINITIONS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "progressivecodec_amd")
DIR = os.path.join(PKG, "chroma_clip_tol_gpu")
T = 64
NO = TOL.NO_MSE
SIZES = [(1, 1), (2, 2), (64, 64), (65, 63), (100, 150), (127, 129)]         # section 18's six sizes and four overlaps
OVERLAPS = [0, 4, 16, 32]


def _lib():
    """the module and its library; a library that is not built is an ImportError, as for every other one"""
    from progressivecodec_amd import chroma_clip_tol
    return chroma_clip_tol, chroma_clip_tol.lib()


def flat_codes(H, W, fmt, value):
    Hc, Wc = CC.chroma_size(H, W, fmt)
    return [np.full((1, H, W), value, np.int64), np.full((1, Hc, Wc), value, np.int64), np.full((1, Hc, Wc), value, np.int64)]


def random_codes(H, W, fmt, seed, lo=0, hi=None):
    g = np.random.default_rng(seed)
    Hc, Wc = CC.chroma_size(H, W, fmt)
    hi = (1 << CC.bits(fmt)) if hi is None else hi
    return [g.integers(lo, hi, s, dtype=np.int64) for s in ((1, H, W), (1, Hc, Wc), (1, Hc, Wc))]


def noisy_clip(H, W, fmt, seed, a=2, F=4):
    """frame 0 random, the later frames within a of it; frame 2 with one far sample per plane on top"""
    g = np.random.default_rng(seed)
    top = 1 << CC.bits(fmt)
    base = random_codes(H, W, fmt, seed, lo=a, hi=top - a - 40)
    clip = [base] + [[c + g.integers(-a, a + 1, c.shape) for c in base] for _ in range(F - 1)]
    for c in clip[2]:
        c[0, c.shape[1] // 2, c.shape[2] // 2] += 30
    return [CC.frame(*c, fmt) for c in clip]


# -- the restatement -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", SIZES)
def test_centre_sited_420_is_section_18(hw):
    H, W = hw
    for O, fmt, up in itertools.product(OVERLAPS, FC.FORMATS, FC.UPSAMPLES):
        clip = noisy_clip(H, W, fmt, 1000 * H + W + O)
        n = int(np.prod(TC.grid(H, W, T, O)))
        for t in range(n):
            assert TOL.nsamp(t, H, W, T, O, fmt, "centre", up) == TOL18.nsamp(t, H, W, T, O, up)
        for tol in [((2, 2, 2), (NO,) * 3, 0), ((1, 2, 2), (NO, TOL.mse_q10(1.5), NO), 0), ((40, 40, 40), (NO,) * 3, 2), ((0, 0, 0), (NO,) * 3, 0)]:
            assert TOL.scan(clip, fmt, "centre", T, O, up, *tol) == TOL18.scan(clip, fmt, T, O, up, *tol), (H, W, O, fmt, up, tol)
        assert TOL.scan(clip, fmt, "centre", T, O, up, (2, 2, 2))[0][2] != [0] * n     # the far samples recode


def test_tolerance_zero_is_section_25s_source_table_and_counts():
    for fmt, siting, (H, W), O, up in [("p210", "left", (100, 150), 16, "linear"), ("i444", "centre", (127, 129), 0, "nearest"),
                                       ("nv12", "topleft", (65, 63), 4, "linear"), ("i410", "left", (100, 150), 0, "linear")]:
        g = np.random.default_rng(H + O)
        clip = [CC.frame(*random_codes(H, W, fmt, 1), fmt)]
        for k in range(1, 6):
            nxt = [np.array(c) for c in CC.codes(clip[-1], fmt)]
            if k != 3:                                                               # frame 3 repeats frame 2
                p = k % 3
                y, x = g.integers(0, nxt[p].shape[1]), g.integers(0, nxt[p].shape[2])
                nxt[p][0, y, x] ^= 1
            clip.append(CC.frame(*nxt, fmt))
        n = int(np.prod(TC.grid(H, W, T, O)))
        source, stats = TOL.scan(clip, fmt, siting, T, O, up)
        assert source == CK.source_table(clip, fmt, siting, T, O, up)
        assert any(s == k for k, row in enumerate(source[1:], 1) for s in row) and any(s != k for k, row in enumerate(source[1:], 1) for s in row)
        assert source[3] == source[2] and stats[0] == [[[0, 0, 0]] * 3] * n
        # under the zero tolerance the anchor's footprint is the previous frame's: a count is section 25's number, everywhere
        for k in range(1, 6):
            cnt = CK.tile_changes(clip[k], clip[k - 1], fmt, siting, T, O, up)
            assert [[s[0] for s in stats[k][t]] for t in range(n)] == cnt, (fmt, k)
        # max_run = 1 codes everything, whatever the tolerance
        top = (1 << CC.bits(fmt)) - 1
        assert TOL.scan(clip, fmt, siting, T, O, up, max_run=1)[0] == [[k] * n for k in range(6)]
        assert TOL.scan(clip, fmt, siting, T, O, up, (top,) * 3, max_run=1)[0] == [[k] * n for k in range(6)]


def test_ramp_is_judged_against_the_anchor_not_the_previous_frame():
    H, W = 100, 150
    for fmt, siting, O, up in [("nv16", "left", 16, "linear"), ("p410", "centre", 0, "nearest"), ("i010", "topleft", 4, "linear")]:
        clip = [CC.frame(*flat_codes(H, W, fmt, 100 + k), fmt) for k in range(5)]    # away from 0 and from the top code
        n = int(np.prod(TC.grid(H, W, T, O)))
        source, stats = TOL.scan(clip, fmt, siting, T, O, up, max_abs=(2, 2, 2))
        assert source == [[v] * n for v in [0, 0, 0, 3, 3]]
        for k, v in enumerate([0, 1, 2, 3, 1]):
            ns = TOL.nsamp(0, H, W, T, O, fmt, siting, up)
            assert stats[k][0] == [[ns[p] if v else 0, v * v * ns[p], v] for p in range(3)]
        assert TOL.worst(source, stats) == [2, 2, 2]
        prev, _ = TOL.scan(clip, fmt, siting, T, O, up, max_abs=(2, 2, 2), against_previous=True)
        assert prev == [[0] * n] * 5 and prev != source                              # the rule the contract rejects drifts for ever


def test_nsamp_is_the_footprint_s_size_and_the_siting_moves_the_mse_decision():
    for fmt, siting, up, (H, W), O in itertools.product(("nv12", "p210", "i444", "i010"), CC.SITINGS, CC.UPSAMPLES, [(100, 150), (65, 63), (1, 1)], (0, 16)):
        sizes = CK.footprint_sizes(H, W, T, O, fmt, siting, up)
        assert [TOL.nsamp(t, H, W, T, O, fmt, siting, up) for t in range(len(sizes))] == sizes
    # tile (0, 1) of a 100 x 150 p210 frame, O = 0: chroma columns 31 .. 64 under centre siting, 32 .. 64 under left
    H, W = 100, 150
    assert TOL.nsamp(1, H, W, T, 0, "p210", "centre", "linear") == [64 * 64, 64 * 34, 64 * 34]
    assert TOL.nsamp(1, H, W, T, 0, "p210", "left", "linear") == [64 * 64, 64 * 33, 64 * 33]
    assert TOL.nsamp(1, H, W, T, 0, "p210", "left", "nearest") == [64 * 64, 64 * 32, 64 * 32]
    base = flat_codes(H, W, "p210", 500)
    c = [np.array(p) for p in base]
    c[1][0, :17, 40] += 8                                                            # 17 Cb samples off by 8 inside every footprint of tile 1
    clip = [CC.frame(*base, "p210"), CC.frame(*c, "p210")]
    q = (NO, 512, NO)                                                                # max_mse = 0.5: 1024 * 17 * 64 <= 512 * nsamp iff nsamp >= 2176
    assert 64 * 34 == 2176 and 64 * 33 < 2176
    assert TOL.scan(clip, "p210", "centre", T, 0, "linear", (8, 8, 8), q)[0][1][1] == 0
    assert TOL.scan(clip, "p210", "left", T, 0, "linear", (8, 8, 8), q)[0][1][1] == 1


#: (format, the changed Cb sample, [(siting, upsampling, the tiles recoded)]): T = 64, O = 0, 100 x 150 is 2 x 3 tiles; tile (0, 1)
#: starts at chroma column 32 of a 4:2:2 frame and tile (1, 0), number 3, at chroma row 32 of a 4:2:0 one
HALO = [
    ("p210", (10, 31), [("centre", "linear", [0, 1]), ("left", "linear", [0]), ("topleft", "linear", [0]), ("centre", "nearest", [0]),
                        ("left", "nearest", [0])]),
    ("p210", (10, 32), [("centre", "linear", [0, 1]), ("left", "linear", [0, 1]), ("topleft", "linear", [0, 1]), ("centre", "nearest", [1]),
                        ("left", "nearest", [1])]),
    ("nv12", (31, 10), [("centre", "linear", [0, 3]), ("left", "linear", [0, 3]), ("topleft", "linear", [0]), ("centre", "nearest", [0]),
                        ("topleft", "nearest", [0])]),
    ("nv12", (32, 10), [("centre", "linear", [0, 3]), ("left", "linear", [0, 3]), ("topleft", "linear", [0, 3]), ("centre", "nearest", [3]),
                        ("topleft", "nearest", [3])]),
]


def test_the_halo_rule_in_numbers():
    """one Cb sample changed, zero tolerance: the restatement's table is the authority, and says exactly what the text says"""
    H, W = 100, 150
    from tests import test_gpu_chroma_clip_tol as G
    assert G.HALO == HALO
    for fmt, where, rows in HALO:
        base = flat_codes(H, W, fmt, 90)
        c = [np.array(p) for p in base]
        c[1][0][where] += 9
        clip = [CC.frame(*base, fmt), CC.frame(*c, fmt)]
        for siting, up, recoded in rows:
            source, stats = TOL.scan(clip, fmt, siting, T, 0, up)
            assert [t for t, s in enumerate(source[1]) if s == 1] == recoded, (fmt, where, siting, up)
            assert all(stats[1][t] == ([[0, 0, 0], [1, 81, 9], [0, 0, 0]] if t in recoded else [[0, 0, 0]] * 3) for t in range(6))
            # a tolerance of nine codes takes the sample back in
            assert TOL.scan(clip, fmt, siting, T, 0, up, (0, 9, 0))[0] == [[0] * 6] * 2


def test_a_word_s_other_bits_change_no_code():
    g = np.random.default_rng(3)
    for fmt, keep in (("p210", 0xFFC0), ("i410", 0x03FF), ("p010", 0xFFC0)):
        f0 = CC.frame(*random_codes(65, 63, fmt, 9), fmt)
        f1 = tuple((p & np.uint16(keep)) | (g.integers(0, 2 ** 16, p.shape).astype(np.uint16) & np.uint16(~keep & 0xFFFF)) for p in f0)
        assert any((a != b).any() for a, b in zip(f0, f1))
        source, stats = TOL.scan([f0, f1, f0], fmt, "left", T, 4, "linear")
        assert source == [[0, 0]] * 3 and stats == [[[[0, 0, 0]] * 3] * 2] * 3


# -- the library, no device ----------------------------------------------------------------------------------------------------------

def test_workspace_size_is_72_bytes_per_block_and_4_per_tile():
    _, L = _lib()
    for size, n in [(64, 1), (64, 6), (64, 7), (128, 9), (512, 40), (1024, 3), (2048, 2), (2048, 5)]:
        for sy in (1, 2):
            want = (72 * n * (size * size // (2048 * sy) + 1) + 4 * n + 7) // 8 * 8
            assert L.pc_chroma_clip_tol_workspace_size(size, sy, n) == want == TOL.workspace_size(size, sy, n) and want % 8 == 0, (size, sy, n)
    assert L.pc_chroma_clip_tol_workspace_size(64, 2, 1) == 152 and L.pc_chroma_clip_tol_workspace_size(64, 2, 6) == 888
    assert L.pc_chroma_clip_tol_workspace_size(64, 1, 1) == 224
    from progressivecodec_amd import clip_tol
    assert L.pc_chroma_clip_tol_workspace_size(512, 2, 40) == clip_tol.lib().pc_clip_tol_workspace_size(512, 40)
    for bad in [(0, 1, 1), (32, 1, 1), (96, 2, 1), (-64, 1, 1), (4096, 1, 1), (64, 1, 0), (64, 2, -1), (64, 0, 1), (64, 3, 1),
                (2048, 1, 2 ** 31 - 1), (2048, 2, 2 ** 21)]:
        assert L.pc_chroma_clip_tol_workspace_size(*bad) == 0, bad


def table_of(fs):
    from progressivecodec_amd import frames
    return (frames.Frame * len(fs))(*fs)


def test_plan_is_host_only_and_each_precondition_is_broken_alone():
    """made-up pointer values: nothing may be dereferenced or launched (there is no GPU here).  Every frame of the table has to
    allow the wide path, wherever in the table it stands; what a frame needs is what pc_chroma_clips_plan(PC_CHC_CHANGES) needs."""
    from progressivecodec_amd import chroma, chroma_clips
    _, L = _lib()
    LC = chroma_clips.lib()
    H, W = 96, 160

    def plan(fmt, fs, O=0, n=None, sx=None):
        wide = C.c_int(-1)
        f = chroma.FORMATS[fmt]
        rc = L.pc_chroma_clip_tol_plan(f.layout, f.bits, f.sx if sx is None else sx, table_of(fs) if fs else None, len(fs) if n is None else n, O,
                                       C.byref(wide))
        return rc, wide.value

    def pair(fmt, a, b, O=0):
        wide = C.c_int(-1)
        f = chroma.FORMATS[fmt]
        assert LC.pc_chroma_clips_plan(chroma_clips.CHANGES, f.layout, f.bits, f.sx, C.byref(a), C.byref(b), None, O, C.byref(wide)) == 0
        return wide.value
    for fmt in sorted(chroma.FORMATS):
        f_ = chroma.FORMATS[fmt]
        es = 2 if f_.bits == 10 else 1
        planar = f_.layout == chroma.PLANAR
        good = lambda: [fake_frame(chroma, fmt, H, W), fake_frame(chroma, fmt, H, W, base=0x7100_0000_1000, pad=4),       # noqa: E731
                        fake_frame(chroma, fmt, H, W, base=0x7200_0000_1000, pad=8)]
        assert plan(fmt, good()) == (0, 1) and plan(fmt, good()[:1]) == (0, 1)
        for slot in range(3):
            for nm in ["y", "u"] + (["v"] if planar else []):
                for off in (1, 2, 3):
                    fs = good()
                    setattr(fs[slot], nm, getattr(fs[slot], nm) + off * es)           # each plane of each frame: aligned to four elements
                    assert plan(fmt, fs) == (0, 0), (fmt, slot, nm, off)
                    assert pair(fmt, fs[slot], fs[(slot + 1) % 3]) == 0
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
        for O in (0, 8, 16, 32, 4, 12, 20, 28):                                      # at sx == 1 every O qualifies
            fs = good()
            assert plan(fmt, fs, O=O) == (0, int(O % 8 == 0 or f_.sx == 1)) == (0, pair(fmt, fs[0], fs[1], O)), (fmt, O)
        assert plan(fmt, good(), O=-4)[0] == -1 and plan(fmt, [])[0] == -1 and plan(fmt, good(), n=0)[0] == -1 and plan(fmt, good(), n=-1)[0] == -1
        assert plan(fmt, good(), sx=3)[0] == -1 and plan(fmt, good(), sx=0)[0] == -1
        assert L.pc_chroma_clip_tol_plan(f_.layout, f_.bits, f_.sx, table_of(good()), 3, 0, None) == -1
    ok, wide = table_of([fake_frame(chroma, "nv12", H, W)]), C.c_int(-1)
    for layout, bits in [(2, 8), (-1, 8), (0, 9), (1, 12), (1, 16)]:
        assert L.pc_chroma_clip_tol_plan(layout, bits, 2, ok, 1, 0, C.byref(wide)) == -1
    assert plan("nv12", [fake_frame(chroma, "nv12", H, W)]) == (0, 1) and plan("i420", [fake_frame(chroma, "nv12", H, W)])[0] == -1


def test_every_argument_error_returns_before_the_device():
    """fake device pointers: every call below must return PC_ERR_ARG without touching them (no GPU here); each precondition is broken
    alone"""
    from progressivecodec_amd import chroma
    _, L = _lib()
    Wk, Sr, St, Tb = 0x7000_0200_0000, 0x7000_0300_0000, 0x7000_0400_0000, 0x7000_0500_0000
    H, W, O = 100, 150, 16                                                            # 2 x 3 tiles, S = 48
    i3 = lambda *v: (C.c_int * 3)(*v)                                                 # noqa: E731
    for fmt in sorted(chroma.FORMATS):
        f_ = chroma.FORMATS[fmt]
        planar = f_.layout == chroma.PLANAR
        top = (1 << f_.bits) - 1
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
        nbytes = L.pc_chroma_clip_tol_workspace_size(T, f_.sy, 6)
        assert nbytes == TOL.workspace_size(T, f_.sy, 6)
        ok = dict(frames_host=table(), frames_dev=Tb, n_frames=3, layout=f_.layout, bits=f_.bits, shift=f_.shift, sx=f_.sx, sy=f_.sy, hsite=1, vsite=0,
                  up=1, H=H, W=W, T=T, O=O, max_abs=i3(1, top, 0), mse_q10=i3(0, NO, 5), max_run=2, ws=Wk, nbytes=nbytes, source=Sr, stats=St,
                  stream=None)
        bads = [dict(frames_host=t) for t in bad_tables] + [
            dict(layout=2), dict(layout=-1), dict(bits=9), dict(bits=16), dict(shift=1), dict(shift=6 if f_.bits == 8 else 4), dict(sx=3), dict(sx=0),
            dict(sy=0), dict(sy=3), dict(sx=1, sy=2), dict(hsite=2), dict(hsite=-1), dict(vsite=2), dict(vsite=-1),
            dict(H=0), dict(W=0), dict(H=-5), dict(T=0), dict(T=32), dict(T=96), dict(T=-64), dict(T=4096, O=0),
            dict(O=2), dict(O=6), dict(O=36), dict(O=-4), dict(up=2), dict(up=-1),
            dict(frames_dev=None), dict(frames_dev=Tb + 4), dict(n_frames=0), dict(n_frames=-1),
            dict(max_abs=None), dict(mse_q10=None), dict(max_abs=i3(0, 0, -1)), dict(max_abs=i3(top + 1, 0, 0)), dict(max_abs=i3(0, top + 1, 0)),
            dict(mse_q10=i3(-1, 0, 0)), dict(mse_q10=i3(0, 0, NO + 1)), dict(mse_q10=i3(0, -2 ** 31, 0)), dict(max_run=-1),
            dict(ws=None), dict(ws=Wk + 4), dict(nbytes=nbytes - 1), dict(nbytes=0), dict(nbytes=L.pc_chroma_clip_tol_workspace_size(T, f_.sy, 5)),
            dict(source=None), dict(source=Sr + 2), dict(stats=None), dict(stats=St + 4)]
        for bad in bads:
            assert L.pc_chroma_clip_tol_scan(*dict(ok, **bad).values()) == -1, (fmt, {k_: v for k_, v in bad.items() if k_ != "frames_host"})
    # 2^31 blocks or more, and n * 9 above INT32_MAX: 64 x 64 tiles of a frame 2^15 * 64 on a side
    f = fake_frame(chroma, "i444", 1 << 21, 1 << 21)
    huge = dict(frames_host=table_of([f]), frames_dev=Tb, n_frames=1, layout=0, bits=8, shift=0, sx=1, sy=1, hsite=0, vsite=0, up=1, H=1 << 21,
                W=1 << 21, T=T, O=0, max_abs=i3(0, 0, 0), mse_q10=i3(0, 0, 0), max_run=0, ws=Wk, nbytes=1 << 62, source=Sr, stats=St, stream=None)
    assert L.pc_chroma_clip_tol_scan(*huge.values()) == -1                            # 2^30 tiles of 3 blocks
    f = fake_frame(chroma, "i420", 64 * 20000, 64 * 20000)
    many = dict(huge, frames_host=table_of([f]), sx=2, sy=2, H=64 * 20000, W=64 * 20000)
    assert 4 * 10 ** 8 * 2 < 2 ** 31 < 4 * 10 ** 8 * 9 and L.pc_chroma_clip_tol_scan(*many.values()) == -1
    assert L.pc_chroma_clip_tol_last_hip_error() == 0


def test_python_rejects_before_any_device_call(monkeypatch):
    from progressivecodec_amd import chroma_clip_tol as ct
    from progressivecodec_amd import chroma_clips, clip_tol, clips

    def touched(*a, **k):
        raise AssertionError("the device was reached")
    for name in ("device", "current_stream", "synchronize", "current_device", "_lazy_init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    for m in (ct, chroma_clips, clips, clip_tol):
        monkeypatch.setattr(m, "lib", touched)
    y, uv, u = torch.zeros(100, 150, dtype=torch.uint8), torch.zeros(100, 75, 2, dtype=torch.uint8), torch.zeros(100, 150, dtype=torch.uint8)
    f = (y, uv)
    p = (y.to(torch.uint16), uv.to(torch.uint16))
    tol = ct.Tolerance(1)
    assert ct.Tolerance is clip_tol.Tolerance and ct.ClipTolPlan is clip_tol.ClipTolPlan and ct.NO_MSE == NO
    # CPU tensors
    for frames, fmt in [([f, f], "nv16"), ([(y, u, u)], "i444"), ([p, p], "p210"), (tuple(torch.stack([t, t]) for t in f), "nv16")]:
        with pytest.raises(ValueError, match="GPU"):
            ct.scan_clip(frames, fmt, tol, "left", tile=64)
        with pytest.raises(ValueError, match="GPU"):
            ct.encode_clip(None, frames, [0, 1], fmt, siting="left", tile=64, tolerance=tol)
    # enums and the tolerance come before the frames
    for kw, msg in [(dict(fmt="nv21"), "fmt"), (dict(upsample="cubic"), "upsample"), (dict(siting="top"), "siting"), (dict(tolerance=None), "Tolerance"),
                    (dict(tolerance=1), "Tolerance"), (dict(tolerance=(0, 0, 0)), "Tolerance"), (dict(tolerance=ct.Tolerance(256)), "at most 255"),
                    (dict(tolerance=ct.Tolerance((0, 256, 0))), "at most 255")]:
        a = dict(dict(fmt="nv16", tolerance=tol), **kw)
        fmt_, tol_ = a.pop("fmt"), a.pop("tolerance")
        with pytest.raises(ValueError, match=msg):
            ct.scan_clip([f], fmt_, tol_, **a)
        with pytest.raises(ValueError, match=msg):
            ct.encode_clip(None, [f], [0], fmt_, tolerance=tol_, **a)
    with pytest.raises(ValueError, match="max_abs"):
        ct.Tolerance(1024)                                                            # above every format's top code
    for kw, msg in [(dict(matrix="bt470"), "matrix"), (dict(range="tv"), "range"), (dict(max_tiles_per_call=0), "max_tiles_per_call")]:
        with pytest.raises(ValueError, match=msg):
            ct.encode_clip(None, [f], [0], "nv16", tolerance=tol, **kw)
    with pytest.raises(TypeError, match="uint16"):
        ct.scan_clip([f], "p210", tol)
    for bad in ([], (), None, "clip"):
        with pytest.raises(ValueError, match="non-empty list"):
            ct.scan_clip(bad, "nv16", tol)
    with pytest.raises(ValueError, match="got one frame"):
        ct.scan_clip(f, "nv16", tol)
    with pytest.raises(ValueError, match=r"frames\[0\]: UV must be"):
        ct.scan_clip([(y, uv[:2]), f], "nv16", tol)
    # the grid, with the frames' device test out of the way
    monkeypatch.setattr(ct, "_clip_frames", lambda fr, fmt: ([[t.unsqueeze(0) for t in q] for q in fr], fr[0][0].shape[0], fr[0][0].shape[1]))
    for kw, msg in [(dict(tile=96), "multiple of 64"), (dict(overlap=6), "overlap"), (dict(tile=4096), "at most 2048")]:
        with pytest.raises(ValueError, match=msg):
            ct.scan_clip([f, f], "nv16", tol, **kw)
        with pytest.raises(ValueError, match=msg):
            ct.encode_clip(None, [f, f], [0], "nv16", tolerance=tol, **kw)
    assert issubclass(ct.ChromaClipTolError, ct._imagelib.ImageLibError) and ct.LIB_PATH == os.path.join(PKG, "libpc_chroma_clip_tol.so")
    sig = lambda fn: list(inspect.signature(fn).parameters)                                                           # noqa: E731
    assert sig(ct.scan_clip) == ["frames", "fmt", "tolerance", "siting", "tile", "overlap", "upsample"]
    assert sig(ct.plan) == ["frames", "fmt", "overlap"]
    assert sig(ct.encode_clip) == ["model", "frames", "qualities", "fmt", "matrix", "range", "upsample", "siting", "tile", "overlap", "mask_pol",
                                   "tolerance", "max_tiles_per_call"]
    d = {k: v.default for k, v in inspect.signature(ct.encode_clip).parameters.items()}
    assert (d["siting"], d["tile"], d["overlap"], d["upsample"], d["tolerance"], d["max_tiles_per_call"]) == ("centre", 512, 0, "linear", ct.Tolerance(), 32)
    assert inspect.signature(ct.scan_clip).parameters["siting"].default == "centre"


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


def test_the_seventeenth_library_keeps_the_rules_of_the_sixteen():
    ct, L = _lib()
    from progressivecodec_amd import chroma
    hdr = open(os.path.join(DIR, "pc_chroma_clip_tol.h")).read()
    declared = re.findall(r"PC_API\s+[\w\s\*]+?\b(pc_\w+)\s*\(", hdr)
    assert len(declared) == 5 and sorted(declared) == sorted(ct.EXPORTS)
    for name in declared:
        getattr(L, name)
    assert L.pc_chroma_clip_tol_strerror(-1).decode() and L.pc_chroma_clip_tol_strerror(-6).decode() and L.pc_chroma_clip_tol_last_hip_error() == 0
    # the directory holds the header and the source alone: no Makefile; csrc/Makefile drives it straight through the shared rule
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(DIR, "*")) if not p.endswith((".o", ".so")))
    assert names == ["pc_chroma_clip_tol.h", "pc_chroma_clip_tol.hip"]
    top = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\bchroma_clip_tol\b", top, re.M) and re.search(r"^\.PHONY:.*\bchroma_clip_tol\b", top, re.M)
    assert re.search(r"^chroma_clip_tol:\n\t\$\(MAKE\) -C \.\./chroma_clip_tol_gpu -f \.\./image_csrc/lib\.mk NAME=chroma_clip_tol$", top, re.M)
    assert "\t$(MAKE) -C ../chroma_clip_tol_gpu -f ../image_csrc/lib.mk NAME=chroma_clip_tol clean\n" in top
    bare = image_shared.uncommented(os.path.join(PKG, "csrc", "Makefile"))
    assert len(re.findall(r"\bchroma_clip_tol\b(?!_)", bare)) == 5 and len(re.findall(r"chroma_clip_tol_gpu", bare)) == 2
    rule = image_shared.uncommented(os.path.join(PKG, "image_csrc", "lib.mk"))
    assert "-ffp-contract=off" in rule and not re.search(r"-lpc|libpc(odec|_\w+)\b", rule)
    assert re.search(r"^OUT\s*:=\s*\.\./libpc_\$\(NAME\)\.so$", rule, re.M) and re.search(r"^SHARED\s*:=\s*\$\(wildcard \.\./image_csrc/\*\.h\)$", rule, re.M)
    # the pins of the earlier libraries' tests stay true
    assert len(glob.glob(os.path.join(PKG, "*_csrc", "*.hip"))) == len(image_shared.LIBS) == 10
    assert len(glob.glob(os.path.join(PKG, "*_hip", "*.hip"))) == 4 and len(glob.glob(os.path.join(PKG, "*_kernels", "*.hip"))) == 2
    assert len(glob.glob(os.path.join(PKG, "*", "Makefile"))) == 17
    src = open(os.path.join(DIR, "pc_chroma_clip_tol.hip")).read()
    code = _code(os.path.join(DIR, "pc_chroma_clip_tol.hip"))
    assert '#include "pc_image_host.h"' in src and '#include "pc_chroma_compare.h"' in src and '#include "pc_chroma_items.h"' in src
    for other in ("pc_chroma.h", "pc_chroma_clips.h", "pc_clip_tol.h", "pc_clips.h", "pc_yuv_items.h"):
        assert '"%s"' % other not in code, other
    # compare_chroma_tile and its item are defined once, under image_csrc/, and used here
    homes = [p for p in glob.glob(os.path.join(PKG, "*", "*.h")) + glob.glob(os.path.join(PKG, "*", "*.hip"))
             if re.search(r"\bvoid compare_chroma_tile\(", _code(p))]
    assert homes == [os.path.join(PKG, "image_csrc", "pc_chroma_compare.h")]
    shared_hdr = _code(homes[0])
    assert len(re.findall(r"\bvoid compare_chroma_tile\(", shared_hdr)) == 1 and len(re.findall(r"\bvoid compare_chroma_item\(", shared_hdr)) == 1
    assert re.search(r"template <class T, bool IL, int SX, int SY, bool WIDE, class Acc>\s*__device__ __forceinline__ void compare_chroma_tile\(", shared_hdr)
    assert "Acc::template take<T>" in shared_hdr and "Acc::N" in shared_hdr and shared_hdr.count("namespace {") == 1
    assert "compare_chroma_tile<T, IL, SX, SY, WIDE, Stats>(" in code and "compare_chroma_item" not in code
    # the shared names are used, not defined: neither here nor in the new header
    for name, pattern in DEFINITIONS.items():
        assert not re.search(pattern, code) and not re.search(pattern, shared_hdr), name
    for name in ("ingest_item", "Taps", "code_of", "format_of", "with_format", "picture_ok", "site_ok", "depth_levels"):
        assert not re.search(r"\b(struct|void|int|bool|unsigned|float|define|constexpr int)\s+%s\b\s*[({=]" % name, code + shared_hdr), name
    for name in ("HIPCHK", "g_last_hip", "planes_of", "block_reduce", "gather_partials", "wave_reduce", "plane_wide", "aligned", "upsample_ok", "cdiv",
                 "Grid", "geo_of", "NT", "COLS", "code_of", "Fmt", "format_of", "with_format", "picture_ok", "site_ok"):
        assert re.search(r"\b%s\b" % name, code), name
        assert not re.search(r"\b(struct|void|int|bool|unsigned|float|define|constexpr int)\s+%s\b\s*[({=]" % name, code), name
    assert "code_of<T>" in code and ">> SH" not in code and "load4" in shared_hdr
    image_shared.assert_frame_is_shared(hdr, "pc_cct_frame")
    found = dict(re.findall(r"\b(PC_CCT_(?:NEAREST|LINEAR)) = (\w+)", hdr))
    assert found == {"PC_CCT_NEAREST": "PC_YUV_NEAREST", "PC_CCT_LINEAR": "PC_YUV_LINEAR"}
    values = dict((k, int(v)) for k, v in re.findall(r"\b(PC_CCT_\w+) = (\d+)[,\s]", hdr) if k != "PC_CCT_NO_MSE")
    assert values == {"PC_CCT_PLANAR": chroma.PLANAR, "PC_CCT_SEMIPLANAR": chroma.SEMIPLANAR, "PC_CCT_CENTRE": chroma.CENTRE,
                      "PC_CCT_COSITED": chroma.COSITED}
    assert "PC_CCT_NO_MSE = 1 << 30" in hdr
    assert code.count("static_assert(PC_CCT_") == 2 and "LAYOUT_SEMIPLANAR" in code and "SITE_COSITED" in code
    # plain C++: no inline assembly, no builtins, no atomics, no LDS of its own -- in the source and in the new header
    for text in (code, shared_hdr):
        assert not re.search(r"\batomic(Add|CAS|Exch|Max|Min|Or|And)\b|\basm\b|__asm|__shared__|__syncthreads|__builtin_|__shfl", text)
    # 24 + 2 kernels; three launch sites in the scan: row 0 and the anchors before the loop, then a pair per step
    assert "24 diff kernels, the decide kernel and the init kernel" in src
    assert len(re.findall(r"__global__", code)) == 3
    scan = function_body(code, code.index('extern "C" int pc_chroma_clip_tol_scan('))
    loop = function_body(scan, scan.index("for (int k = 1; k < n_frames; ++k)"))
    before = scan[:scan.index("for (int k = 1; k < n_frames; ++k)")]
    assert before.count("hipLaunchKernelGGL(") == 1 and "hipLaunchKernelGGL(init_kernel" in before
    assert loop.count("hipLaunchKernelGGL(") == 3 and loop.count("hipLaunchKernelGGL((diff_kernel<") == 2 and loop.count("hipLaunchKernelGGL(decide_kernel") == 1
    assert scan.count("hipLaunchKernelGGL(") == 4 and not re.search(r"hipMalloc|hipFree|Synchronize|hipMemcpy|hipMemset", code)
    # every check comes before the first launch, and the scan decides the path through the exported plan
    assert scan.rindex("return PC_ERR_ARG") < scan.index("hipLaunchKernelGGL(") and "pc_chroma_clip_tol_plan(layout, bits, sx, frames_host" in before
    assert len(re.findall(r"\bpicture_wide\(", code)) == 2                             # its definition and the plan's use
    # the block-uniform guard ends before the reduction's barrier
    diff = function_body(code, code.index("void diff_kernel("))
    guard, reduce_ = diff.index("if (an >= 0 && an < k)"), diff.index("block_reduce<Stats>(")
    assert guard < diff.index("compare_chroma_tile<") < reduce_ and "{" not in diff[guard:reduce_] and diff[guard:reduce_].count(";") == 1
    assert "const int an = anchor[t];" in diff and "blockIdx.x" in diff and "threadIdx" not in diff
    import bench
    assert "chroma" not in inspect.getsource(bench.source_hash) and "_gpu" not in inspect.getsource(bench.source_hash)
    from progressivecodec_amd import _imagelib, chroma_clips, clip_tol
    assert "chroma_clip_tol" in _imagelib.__doc__ and "chroma_clip_tol" in chroma_clips.__doc__ and "chroma_clip_tol" in clip_tol.__doc__
    # own C calls, no copied body: the work loop is chroma_clips', shared by both encoders
    text = inspect.getsource(ct)
    assert "_encode_source(model, fs, g, source, qualities, fmt, matrix, range, upsample, siting, mask_pol, step)" in text
    assert "_encode_source(model, fs, g, source, qualities, fmt, matrix, range, upsample, siting, mask_pol, step)" in inspect.getsource(chroma_clips.encode_clip)
    assert "encode_items" not in text and "pack_clip" not in text and "class Tolerance" not in text and "namedtuple" not in text
    assert list(inspect.signature(chroma_clips._encode_source).parameters) == ["model", "fs", "g", "source", "qualities", "fmt", "matrix", "range",
                                                                               "upsample", "siting", "mask_pol", "step"]


# -- the ledger ----------------------------------------------------------------------------------------------------------------------

def test_every_instantiation_is_launched():
    """pc_chroma_clip_tol.hip: "24 diff kernels".  The tuples the table reaches are exactly those; a case taken away shows here by
    the name of the kernel nothing launches any more"""
    assert len(CS.ALL_KERNELS) == 24
    table = CS.table()
    assert len(table) == 12 * 12 + 4 * 6 and len(set(table)) == len(table)
    got = CS.reached(table)
    assert got == CS.ALL_KERNELS, "never launched: %s" % CS.names(CS.ALL_KERNELS - got)
    # the cases the issue names
    assert {(c.fmt, c.siting, c.upsample, c.O) for c in table if (c.H, c.W) == (100, 150) and c.n < 100} == \
        set(itertools.product(CC.FORMATS, CC.SITINGS, CC.UPSAMPLES, (0, 4)))
    assert {(c.fmt, c.H, c.W) for c in table if c.n >= 100} == set((f, H, W) for f in CS.OTHER_FORMATS for H, W in CS.OTHER_SIZES)
    assert CS.OTHER_FORMATS == ["nv16", "p210", "i444", "nv12"] and CS.OTHER_SIZES == [(1, 1), (2, 3), (3, 2), (37, 53), (65, 63), (127, 129)]
    assert {c.O for c in table if c.n >= 100} == {16, 32} and (CS.T, CS.F) == (64, 5)
    assert CS.ALIGNED == (True, False, False) and len(CS.TABLES) == 3
    for fmt in CC.FORMATS:                                          # O = 4 is narrow at sx == 2, whatever the table
        assert {CS.wide(c, 0) for c in table if c.fmt == fmt and c.n < 100 and c.O == 4} == {CC.sub(fmt)[0] == 1}
        assert {CS.wide(c, p) for c in table if c.fmt == fmt and c.n < 100 for p in range(3)} == {False, True}
    # the ledger notices a case that leaves
    less = [c for c in table if not (c.fmt == "i010" and c.O == 0)]
    assert CS.ALL_KERNELS - CS.reached(less) == {(2, False, 2, 2, True)} and CS.names([(2, False, 2, 2, True)]) == ["u16 planar 2:2 wide"]


# -- through a fake model ------------------------------------------------------------------------------------------------------------

SOURCE = [[0] * 6, [1, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [1, 3, 0, 0, 3, 0]]


def test_encode_clip_against_a_fake_model(monkeypatch):
    """one scan; the work list is chunked across frames, one cut per frame present in a chunk; the bytes do not depend on the
    chunking; the container is chroma_clips.pack_clip of the per-tile blobs selected by plan.source"""
    from progressivecodec_amd import chroma_clip_tol as ct
    from progressivecodec_amd import chroma_clips as kc
    from progressivecodec_amd import container
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    stats = torch.zeros(4, 6, 3, 3, dtype=torch.int64)
    stats[1, 0, 0] = torch.tensor([5, 500, 20])
    stats[1, 2, 1] = torch.tensor([7, 7, 1])                                         # reused with a difference of one code
    stats[2, 3, 2] = torch.tensor([9, 36, 2])                                        # and of two
    stats[3, 1, 1], stats[3, 4, 2] = torch.tensor([1, 81, 9]), torch.tensor([2, 8, 2])
    chunks, cuts, asked = [], [], []

    class Model:
        def compress_levels(self, x, qualities, mask_pol):
            chunks.append(list(x))
            return [{"strings": [[[bytes([t, s]) * (1 + s % 3) for t in x] for s in range(10 if q == 0 else 20)], [bytes([t]) for t in x]],
                     "shape": (1, 1)} for q in qualities]

    def scan(fs, fmt, siting, g, upsample, tol):
        asked.append((fmt, siting, upsample, tuple(g), tol))
        return torch.tensor(SOURCE, dtype=torch.int32), stats

    def cut_of(fs, g, work, *a):
        def cut(a_, b_):
            pieces = list(kc._tilecodec.frame_pieces(work[a_:a_ + b_]))
            cuts.append([(f, m1 - m0) for f, m0, m1 in pieces])
            return [16 * f + t for f, t in work[a_:a_ + b_]]
        return cut
    monkeypatch.setattr(ct, "_clip_frames", lambda frames, fmt: ([None] * 4, 100, 150))
    monkeypatch.setattr(ct, "_scan", scan)
    monkeypatch.setattr(kc, "_cut_of", cut_of)
    work = [16 * f + t for f, row in enumerate(SOURCE) for t, s in enumerate(row) if s == f]
    assert work == [0, 1, 2, 3, 4, 5, 16, 49, 52]
    outs = []
    tol = ct.Tolerance(2, max_run=3)
    kw = dict(matrix="bt2020", siting="left", tile=T, overlap=16, tolerance=tol)
    for per_call in (1, 4, 32):
        del chunks[:], cuts[:], asked[:]
        buf, plan = ct.encode_clip(Model(), None, [0, 0.5], "p210", max_tiles_per_call=per_call, **kw)
        assert chunks == [work[a:a + per_call] for a in range(0, 9, per_call)]                  # chunked across frames
        assert len(asked) == 1 and asked[0][:3] == ("p210", "left", "linear") and asked[0][3][:4] == (100, 150, T, 16) and asked[0][4] is tol
        assert plan == ct.ClipTolPlan(SOURCE, 9, 15, len(buf), stats.tolist(), [0, 1, 2])
        outs.append(buf)
    assert cuts == [[(0, 6), (1, 1), (3, 2)]]                                         # one call: one cut per frame present
    assert outs[0] == outs[1] == outs[2]
    hd = kc.parse_clip(outs[0])
    blobs = [[kc.clip_tile_bytes(outs[0], hd, f, t)[0] if s == f else None for t, s in enumerate(row)] for f, row in enumerate(SOURCE)]
    assert outs[0] == kc.pack_clip(blobs, plan.source, 100, 150, T, 16, "p210", "bt2020", "limited", "linear", "left")
    assert outs[0] == CK.pack_clip(blobs, SOURCE, 100, 150, T, 16, "p210", "bt2020", "limited", "linear", "left", 1)
    for f, t in [(0, 0), (1, 0), (3, 4)]:
        strings, shape, qs, _, pol = container.unpack(blobs[f][t], expect_contract=False)
        assert strings[1][1] == [bytes([16 * f + t])] and qs == [0, 0.5] and pol == "point-based-std" and tuple(shape) == (1, 1)
    # chroma_clips.encode_clip over the same source table gives the same bytes: one loop
    changed = torch.zeros(3, 6, 3, dtype=torch.int64)
    changed[0, 0, 0], changed[2, 1, 1], changed[2, 4, 2] = 5, 1, 2                   # SOURCE
    monkeypatch.setattr(kc, "_clip_frames", lambda frames, fmt: ([None] * 4, 100, 150))
    monkeypatch.setattr(kc, "_clip_changes", lambda *a: changed)
    buf, plan0 = kc.encode_clip(Model(), None, [0, 0.5], "p210", matrix="bt2020", siting="left", tile=T, overlap=16)
    assert buf == outs[0] and tuple(plan0) == tuple(plan[:4])

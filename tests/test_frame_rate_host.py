"""Rate-controlled tiled coding of YUV 4:2:0 frames without a GPU: the properties DESIGN.md section 15 promises, on the restatement
(tests/frame_rate_contract.py) alone; libpc_frame_rate.so's C ABI up to the first device call; and progressivecodec_amd.frame_rate's
argument checks."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import frame_rate_contract as QC
from tests import frame_tiles_contract as GC
from tests import frames_contract as FC
from tests import image_shared
from tests import rate_contract as RC
from tests import tiles_contract as TC
from tests.test_frames_host import fake_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 64
SIZES = [(65, 63), (100, 150), (127, 129)]
OVERLAPS = [0, 4, 16, 32]
MATS = list(FC.MATRICES)


def _lib():
    from progressivecodec_amd import frame_rate
    return frame_rate, frame_rate.lib()


@functools.lru_cache(maxsize=None)
def hostile(H, W, O):
    ny, nx = TC.grid(H, W, T, O)
    x = TC.hostile_tiles(ny * nx, T, seed=H * 1000 + W + O)
    x.setflags(write=False)
    return x


# -- the contract's properties -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("O", OVERLAPS + [8, 12, 28])
def test_the_weights_are_integers_and_partition_den_per_sample(O):
    """per axis, over the tiles that cover a sample, the luma numerators and the chroma weights both sum to den -- so den^2 per
    sample of the frame --, the last cell of an odd length included; and cy is the band weight at the cell's centre"""
    den = RC.den_of(O)
    lengths = sorted({v for hw in SIZES for v in hw} | {1, 2, 64, 66, 128, 191, 200})
    for L in lengths:
        n = TC.axis_tiles(L, T, O)
        assert QC.coverage(L, T, O, chroma=False) == [den] * L, (L, O)
        assert QC.coverage(L, T, O, chroma=True) == [den] * -(-L // 2), (L, O)
        for i in range(n):
            cy = QC.chroma_weights(i, n, T, O)                                        # raises if a half is left over
            assert all(isinstance(v, int) and 1 <= v <= den for v in cy)
            assert cy == [QC.chroma_weight_closed(i, k, n, T, O) for k in range(T // 2)], (L, O, i)
    for H, W in SIZES:                                                                # and per sample of the frames: den^2
        ty, tx = QC.coverage(H, T, O, False), QC.coverage(W, T, O, False)
        cy, cx = QC.coverage(H, T, O, True), QC.coverage(W, T, O, True)
        assert {a * b for a in ty for b in tx} == {den * den} == {a * b for a in cy for b in cx}
        assert (len(cy), len(cx)) == FC.chroma_size(H, W)


@pytest.mark.parametrize("hw", SIZES)
def test_without_overlap_the_table_adds_up_to_the_stitched_frames_sums(hw):
    H, W = hw
    x = hostile(H, W, 0)
    for k, fmt in enumerate(FC.FORMATS):
        for rng in FC.RANGES:
            matrix = MATS[(k + H) % 3]
            ref = FC.random_frame(1, H, W, fmt, seed=H + k)
            table = QC.tile_sse(x, H, W, T, 0, fmt, matrix, rng, ref)
            assert [sum(row[p] for row in table) for p in range(3)] == GC.sums(x, H, W, T, 0, fmt, matrix, rng, ref), (hw, fmt, rng)


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("O", OVERLAPS)
def test_a_tiles_sums_do_not_depend_on_the_range_it_is_part_of(hw, O):
    H, W = hw
    x = hostile(H, W, O)
    n = x.shape[0]
    for k, fmt in enumerate(FC.FORMATS):
        matrix, rng = MATS[(k + O // 4) % 3], FC.RANGES[(k + H) % 2]
        ref = FC.random_frame(1, H, W, fmt, seed=W + k)
        whole = QC.tile_sse(x, H, W, T, O, fmt, matrix, rng, ref)
        assert len(whole) == n and all(len(r) == 3 and all(isinstance(v, int) and v >= 0 for v in r) for r in whole)
        assert any(v > 0 for r in whole for v in r)
        for first, m in [(1, n - 1), (n // 2, 1), (n - 1, 1)]:
            assert QC.tile_sse(x[first:first + m], H, W, T, O, fmt, matrix, rng, ref, first_tile=first) == whole[first:first + m], (hw, O, fmt, first)
        with pytest.raises(ValueError):
            QC.tile_sse(x, H, W, T, O, fmt, matrix, rng, ref, first_tile=1)


def saturated(H, W, fmt):
    """the original of the largest error against all-zero tiles in full range: the maximum luma code, chroma code 0; and (e_Y, e_C)"""
    yo, ys, co, cs, mx = FC.levels(fmt, "full")
    Hc, Wc = FC.chroma_size(H, W)
    ref = FC.frame(np.full((1, H, W), mx, np.int64), np.zeros((1, Hc, Wc), np.int64), np.zeros((1, Hc, Wc), np.int64), fmt)
    return ref, mx - yo, co


@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_the_largest_error_meets_every_weight(fmt):
    """all-zero tiles render as (yo, co, co); the sums are then e^2 times the sum of the weights, den^2 per sample"""
    for (H, W), O in [((65, 63), 0), ((100, 150), 16), ((127, 129), 32), ((100, 150), 4)]:
        ny, nx = TC.grid(H, W, T, O)
        ref, eY, eC = saturated(H, W, fmt)
        assert (eY, eC) == ((255, 128) if fmt != "p010" else (1023, 512))
        table = QC.tile_sse(np.zeros((ny * nx, 3, T, T), np.float32), H, W, T, O, fmt, "bt709", "full", ref)
        den = RC.den_of(O)
        Hc, Wc = FC.chroma_size(H, W)
        assert sum(r[0] for r in table) == eY * eY * den * den * H * W, (fmt, H, W, O)
        assert sum(r[1] for r in table) == sum(r[2] for r in table) == eC * eC * den * den * Hc * Wc, (fmt, H, W, O)
    assert QC.max_tile("nv12") == QC.max_tile("i420") == 2048 and QC.max_tile("p010") == 1024
    assert 4096 ** 4 * 255 ** 2 >= 2 ** 60 and 2048 ** 4 * 1023 ** 2 >= 2 ** 60       # the next tile sizes do not fit


def test_edge_cells_clamp_inside_the_tile():
    """a tile whose in-frame part has odd sizes: its last chroma row and column are means over the rows and columns inside the frame
    alone, whatever the tile holds beyond them"""
    H, W, O = 65, 63, 0
    x = np.array(hostile(H, W, O))
    ref = FC.random_frame(1, H, W, "nv12", seed=9)
    want = QC.tile_sse(x, H, W, T, O, "nv12", "bt601", "limited", ref)
    y = x.copy()
    y[:, :, :, 63:] = 0.25                                                            # column 63 lies beyond W = 63
    y[1, :, 1:, :] = 0.75                                                             # tile 1 holds row 64 alone
    assert QC.tile_sse(y, H, W, T, O, "nv12", "bt601", "limited", ref) == want


# -- the library, no device ----------------------------------------------------------------------------------------------------------

def test_library_exports_every_declared_function():
    fr, L = _lib()
    hdr = open(os.path.join(ROOT, "progressivecodec_amd", "frame_rate_csrc", "pc_frame_rate.h")).read()
    declared = re.findall(r"PC_API\s+[\w\s\*]+?\b(pc_\w+)\s*\(", hdr)
    assert len(declared) == 5 and sorted(declared) == sorted(fr.EXPORTS)
    for name in declared:
        getattr(L, name)
    assert L.pc_frame_rate_strerror(-1).decode() and L.pc_frame_rate_strerror(-6).decode() and L.pc_frame_rate_last_hip_error() == 0
    # a library of its own: no other library of the project is linked, and the codec's source hash does not cover it
    import bench
    import inspect
    assert "frame_rate" not in inspect.getsource(bench.source_hash)
    mk = image_shared.build_rule("frame_rate")                                             # image_csrc/lib.mk, which the library's Makefile includes
    assert "-ffp-contract=off" in mk and not re.search(r"-lpc|libpc(odec|_pixels|_tiles|_rate|_metrics|_frames|_frame_tiles)\b", mk)
    top = open(os.path.join(ROOT, "progressivecodec_amd", "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\bframe_rate\b", top, re.M) and re.search(r"^\.PHONY:.*\bframe_rate\b", top, re.M)
    assert "$(MAKE) -C ../frame_rate_csrc clean" in top
    # the frame is the one record of image_csrc/pc_yuv_frame.h, as pc_frames.h's is: frames.Frame serves this library, too
    image_shared.assert_frame_is_shared(hdr, "pc_fr_frame")


def test_workspace_size_is_24_bytes_per_block():
    _, L = _lib()
    for size, n in [(64, 1), (64, 6), (128, 9), (512, 40), (1024, 3), (2048, 2)]:
        assert L.pc_frame_rate_workspace_size(size, n) == 24 * n * (size * size // 4096), (size, n)
    for bad in [(0, 1), (32, 1), (96, 1), (-64, 1), (4096, 1), (64, 0), (64, -1), (2048, 2 ** 31 - 1)]:
        assert L.pc_frame_rate_workspace_size(*bad) == 0, bad


def test_plan_is_host_only_and_each_precondition_is_broken_alone():
    """made-up pointer values: nothing may be dereferenced or launched (there is no GPU here)"""
    from progressivecodec_amd import frames
    _, L = _lib()
    Fp = 0x7000_0100_0000
    H, W = 96, 160
    FS = (3 * T * T, T * T, T)

    def plan(fmt, ref, f32=Fp, fs=FS, O=0):
        wide = C.c_int(-1)
        rc = L.pc_frame_rate_plan(f32, *fs, O, frames.FORMATS[fmt], C.byref(ref) if ref is not None else None, C.byref(wide))
        return rc, wide.value
    for fmt in FC.FORMATS:
        es = 2 if fmt == "p010" else 1
        ok = fake_frame(frames, fmt, H, W)
        assert plan(fmt, ok) == (0, 1)
        for off in (4, 8, 12):
            assert plan(fmt, ok, f32=Fp + off) == (0, 0)                                    # the floats: 16-byte aligned
        for k in range(3):
            fs = list(FS)
            fs[k] += 2
            assert plan(fmt, ok, fs=tuple(fs)) == (0, 0)                                    # their strides: multiples of 4
        for nm in ["y", "u"] + (["v"] if fmt == "i420" else []):
            for off in (1, 2, 3):
                bad = fake_frame(frames, fmt, H, W)
                setattr(bad, nm, getattr(bad, nm) + off * es)                               # each plane: aligned to four elements
                assert plan(fmt, bad) == (0, 0), (fmt, nm, off)
            bad = fake_frame(frames, fmt, H, W)
            setattr(bad, nm + "_row", getattr(bad, nm + "_row") + 2)                        # each row stride: a multiple of 4
            assert plan(fmt, bad) == (0, 0), (fmt, nm)
            free = fake_frame(frames, fmt, H, W)
            setattr(free, nm + "_batch", getattr(free, nm + "_batch") + 1)                  # one frame per call: no batch stride counts
            assert plan(fmt, free) == (0, 1), (fmt, nm)
        # O a multiple of 8: with O = 4 a tile's first chroma column is 2 mod 4 in the frame
        for O, wide in [(0, 1), (8, 1), (16, 1), (32, 1), (4, 0), (12, 0), (20, 0), (28, 0)]:
            assert plan(fmt, ok, O=O) == (0, wide), (fmt, O)
        assert plan(fmt, ok, O=-4)[0] == -1 and plan(fmt, ok, f32=None)[0] == -1 and plan(fmt, None)[0] == -1
        nul = fake_frame(frames, fmt, H, W)
        nul.u = None
        assert plan(fmt, nul)[0] == -1
        assert L.pc_frame_rate_plan(Fp, *FS, 0, frames.FORMATS[fmt], C.byref(ok), None) == -1
    wide = C.c_int(-1)
    f = fake_frame(frames, "nv12", H, W)
    assert L.pc_frame_rate_plan(Fp, *FS, 0, 3, C.byref(f), C.byref(wide)) == -1
    assert plan("nv12", f) == (0, 1) and plan("i420", f)[0] == -1                           # an I420 frame needs its V pointer


def test_every_argument_error_returns_before_the_device():
    """fake device pointers: every call below must return PC_ERR_ARG without touching them (no GPU here)"""
    from progressivecodec_amd import frames
    _, L = _lib()
    Fp, Wk, S = 0x7000_0100_0000, 0x7000_0200_0000, 0x7000_0300_0000
    H, W, O = 100, 150, 16                                                        # 2 x 3 tiles, S = 48
    k = frames.coefficients("bt709")
    for fmt in FC.FORMATS:
        fid = frames.FORMATS[fmt]

        def broken(field, value):
            f = fake_frame(frames, fmt, H, W)
            setattr(f, field, value)
            return f
        bad_frames = [broken("y", None), broken("u", None), broken("y_row", W - 1), broken("u_row", (2 * 75 if fmt != "i420" else 75) - 1)]
        if fmt == "i420":
            bad_frames += [broken("v", None), broken("v_row", 74)]
        if fmt == "p010":
            bad_frames += [broken("y", fake_frame(frames, fmt, H, W).y + 1), broken("u", fake_frame(frames, fmt, H, W).u + 1)]
        nbytes = L.pc_frame_rate_workspace_size(T, 6)
        ok = dict(x=Fp, sxt=3 * T * T, sxc=T * T, sxh=T, H=H, W=W, T=T, O=O, first=0, n=6, fmt=fid, range=0, kr=k.kr, kg=k.kg, kb=k.kb,
                  ib=k.ib, ir=k.ir, ref=fake_frame(frames, fmt, H, W), ws=Wk, nbytes=nbytes, out=S, stream=None)
        bads = [dict(ref=f) for f in bad_frames] + [
            dict(x=None), dict(x=Fp + 1), dict(sxh=T - 1), dict(sxc=0), dict(sxt=0), dict(fmt=3), dict(fmt=-1), dict(range=2), dict(range=-1),
            dict(H=0), dict(W=0), dict(H=-5), dict(T=0), dict(T=32), dict(T=96), dict(T=-64), dict(T=4096, O=0), dict(O=2), dict(O=6),
            dict(O=36), dict(O=-4), dict(first=-1), dict(first=1), dict(n=0), dict(n=7), dict(n=-1), dict(first=6, n=1),
            dict(first=2 ** 31 - 1, n=2 ** 31 - 1), dict(ws=None), dict(ws=Wk + 4), dict(out=None), dict(out=S + 4), dict(nbytes=nbytes - 1),
            dict(nbytes=0)]
        if fmt == "p010":
            bads.append(dict(T=2048, O=0, n=1, nbytes=1 << 30))                   # the sums of 10-bit codes fit up to T = 1024
        for bad in bads:
            a = dict(ok, **bad)
            args = [C.byref(v) if isinstance(v, frames.Frame) else v for v in a.values()]
            assert L.pc_frame_rate_tile_sse(*args) == -1, (fmt, bad)
        a = dict(ok, ref=None)
        assert L.pc_frame_rate_tile_sse(*a.values()) == -1


def test_python_rejects_before_any_device_call(monkeypatch):
    from progressivecodec_amd import frame_rate as fr

    def touched(*a, **k):
        raise AssertionError("the device was reached")
    for name in ("device", "current_stream", "synchronize", "current_device", "_lazy_init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.setattr(fr, "lib", touched)
    g = fr.grid_of(100, 150, 64, 16)
    x = torch.zeros(6, 3, 64, 64)
    yy, uu = torch.zeros(100, 150, dtype=torch.uint8), torch.zeros(50, 75, 2, dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU"):
        fr.frame_tile_distortion(x, g, (yy, uu), "nv12")
    with pytest.raises(ValueError, match="fmt"):
        fr.frame_tile_distortion(x, g, (yy, uu), "nv21")
    with pytest.raises(ValueError, match="matrix"):
        fr.frame_tile_distortion(x, g, (yy, uu), "nv12", matrix="bt470")
    with pytest.raises(ValueError, match="range"):
        fr.frame_tile_distortion(x, g, (yy, uu), "nv12", range="tv")
    with pytest.raises(TypeError, match="float32"):
        fr.frame_tile_distortion(x.double(), g, (yy, uu), "nv12")
    with pytest.raises(ValueError, match="outside"):
        fr.frame_tile_distortion(x, g, (yy, uu), "nv12", first_tile=1)
    with pytest.raises(ValueError, match="outside"):
        fr.frame_tile_distortion(x[:1], g, (yy, uu), "nv12", first_tile=-1)
    with pytest.raises(ValueError, match="n >= 1"):
        fr.frame_tile_distortion(x[:0], g, (yy, uu), "nv12")
    with pytest.raises(ValueError, match="x_hat_tiles must be"):
        fr.frame_tile_distortion(x[:, :2], g, (yy, uu), "nv12")
    with pytest.raises(ValueError, match="the grid of"):
        fr.frame_tile_distortion(x, g._replace(ny=3, nty=3), (yy, uu), "nv12")
    with pytest.raises(ValueError, match="ref: UV must be"):
        fr.frame_tile_distortion(x, g, (yy, uu[:2]), "nv12")
    with pytest.raises(TypeError, match="uint16"):
        fr.frame_tile_distortion(x, g, (yy, uu), "p010")
    big = fr.grid_of(5000, 5000, 2048, 0)
    with pytest.raises(ValueError, match="at most 1024"):
        fr.frame_tile_distortion(torch.zeros(1, 3, 1, 1).expand(1, 3, 2048, 2048), big, (yy.to(torch.uint16), uu.to(torch.uint16)), "p010")
    with pytest.raises(ValueError, match="at most 2048"):
        fr.frame_tile_distortion(torch.zeros(1, 3, 1, 1).expand(1, 3, 4096, 4096), fr.grid_of(5000, 5000, 4096, 0), (yy, uu), "nv12")
    enc = lambda **kw: fr.encode_frame_tiled_to_size(None, (yy, uu), [0, 1], 10 ** 6, "nv12", **dict(dict(tile=64), **kw))     # noqa: E731
    with pytest.raises(ValueError, match="GPU"):
        enc()
    with pytest.raises(ValueError, match="max_tiles_per_call"):
        enc(max_tiles_per_call=0)
    for bad in [(1, 1), (1, 1, -1), (0, 0, 0), (1.0, 1, 1), (True, 1, 1)]:
        with pytest.raises(ValueError, match="plane_weights"):
            enc(plane_weights=bad)
    with pytest.raises(ValueError, match="at least one level"):
        fr.encode_frame_tiled_to_size(None, (yy, uu), [], 10 ** 6, "nv12", tile=64)
    with pytest.raises(ValueError, match="upsample"):
        enc(upsample="cubic")
    assert fr.FrameRatePlan._fields == ("levels", "rates", "dists", "plane_dists", "den", "container_bytes", "predicted", "sse")

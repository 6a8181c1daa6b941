"""Rate-controlled tiled coding of YUV frames of any subsampling and siting without a GPU: the restatement
tests/chroma_rate_contract.py against section 15's, section 21's and section 23's; libpc_chroma_rate.so's C ABI up to the first device
call; progressivecodec_amd.chroma_rate's argument checks; the structure of the fourteenth library and the ledger of its kernels."""
import ctypes as C
import functools
import glob
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests import chroma_contract as CC
from tests import chroma_rate_cases as RS
from tests import chroma_rate_contract as XC
from tests import chroma_tiles_contract as KC
from tests import frame_rate_contract as QC
from tests import frames_contract as FC
from tests import image_shared
from tests import rate_contract as RC
from tests import tiles_contract as TC
from tests.test_chroma_host import fake_frame
from tests.test_image_shared_host import DEFINITIONS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "progressivecodec_amd")
DIR = os.path.join(PKG, "chroma_rate_hip")
T = 64
OVERLAPS = [0, 4, 16, 32]
MATS = list(FC.MATRICES)


def _lib():
    """the module and its library; a library that is not built is an ImportError, as for every other one"""
    from progressivecodec_amd import chroma_rate
    return chroma_rate, chroma_rate.lib()


@functools.lru_cache(maxsize=None)
def hostile(H, W, O):
    ny, nx = TC.grid(H, W, T, O)
    x = TC.hostile_tiles(ny * nx, T, seed=H * 1000 + W + O)
    x.setflags(write=False)
    return x


def totals(table):
    return [sum(row[p] for row in table) for p in range(3)]


# -- 1. identity with section 15, and the weights ------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", [(100, 150), (127, 129)])
@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_centre_sited_420_is_section_15_exactly(hw, fmt):
    H, W = hw
    for n, O in enumerate(OVERLAPS):
        matrix, rng = MATS[n % 3], FC.RANGES[(n + H) % 2]
        ref = FC.random_frame(1, H, W, fmt, seed=H + n)
        x = hostile(H, W, O)
        want = QC.tile_sse(x, H, W, T, O, fmt, matrix, rng, ref)
        assert XC.tile_sse(x, H, W, T, O, fmt, matrix, rng, "centre", ref) == want, (hw, fmt, O)
        assert XC.tile_sse(x[1:3], H, W, T, O, fmt, matrix, rng, "centre", ref, first_tile=1) == want[1:3]
    assert XC.max_tile(fmt) == QC.max_tile(fmt)


@pytest.mark.parametrize("O", OVERLAPS)
def test_the_weights_partition_den_squared_per_sample(O):
    """per axis, over the tiles that cover a sample, the luma numerators and the chroma weights of either subsampling sum to den -- so
    den^2 per luma and per chroma sample of the frame at (2, 2), (2, 1) and (1, 1) --, the last cell of an odd length included"""
    den = RC.den_of(O)
    for H, W in [(100, 150), (127, 129)]:
        for sx, sy in RS.SUBSAMPLINGS:
            ty, tx = XC.coverage(H, T, O, 1), XC.coverage(W, T, O, 1)
            cy, cx = XC.coverage(H, T, O, sy), XC.coverage(W, T, O, sx)
            assert (len(ty), len(tx), len(cy), len(cx)) == (H, W, -(-H // sy), -(-W // sx))
            assert {a * b for a in ty for b in tx} == {den * den} == {a * b for a in cy for b in cx}, (H, W, O, sx, sy)
        for L in (H, W):
            n = TC.axis_tiles(L, T, O)
            for i in range(n):
                half = XC.chroma_weights(i, n, T, O, 2)                               # raises if a half is left over
                assert half.tolist() == QC.chroma_weights(i, n, T, O) and XC.chroma_weights(i, n, T, O, 1).tolist() == RC.weights_int(i, n, T, O).tolist()
    # the weights do not look at the siting: the same tiles and original under the three sitings differ in the codes alone
    parts = [XC.tile_parts(hostile(100, 150, O), 100, 150, T, O, "nv12", "bt709", "limited", s) for s in CC.SITINGS]
    for a, b in zip(parts[0], parts[2]):
        assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])


# -- 2. relation to the stitch's sums at O = 0 ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", [(100, 150), (127, 129), (64, 150), (100, 64)])
def test_without_overlap_the_table_relates_to_the_stitchs_sums_as_the_contract_says(hw):
    H, W = hw
    ny, nx = TC.grid(H, W, T, 0)
    x = hostile(H, W, 0)
    differing = 0
    for k, (fmt, siting) in enumerate(itertools.product(sorted(CC.FORMATS), CC.SITINGS)):
        matrix, rng = MATS[k % 3], FC.RANGES[k % 2]
        sx, sy = CC.sub(fmt)
        hco, vco = CC.SITINGS[siting]
        ref = CC.random_frame(1, H, W, fmt, seed=H + k, garbage=True)
        got = totals(XC.tile_sse(x, H, W, T, 0, fmt, matrix, rng, siting, ref))
        want = KC.sums(x, H, W, T, 0, fmt, matrix, rng, siting, ref)
        assert got[0] == want[0], (hw, fmt, siting)
        exact = XC.sse_exact(H, W, T, 0, fmt, siting)
        assert exact is not ((sx == 2 and hco and nx > 1) or (sy == 2 and vco and ny > 1))
        if exact:
            assert got == want, (hw, fmt, siting)
            continue
        # sample by sample: the tile's own chroma codes against the stitch's, different in the named column and row alone
        whole = KC.stitch_codes(x, H, W, T, 0, fmt, matrix, rng, siting)
        for i, j, codes, _, _ in XC.tile_parts(x, H, W, T, 0, fmt, matrix, rng, siting):
            assert np.array_equal(codes[0], whole[0][0, i * T:i * T + codes[0].shape[0], j * T:j * T + codes[0].shape[1]])
            for p in (1, 2):
                hc, wc = codes[p].shape
                d = codes[p] != whole[p][0, i * T // sy:i * T // sy + hc, j * T // sx:j * T // sx + wc]
                may = np.zeros_like(d)
                if sx == 2 and hco and j > 0:
                    may[:, 0] = True
                if sy == 2 and vco and i > 0:
                    may[0, :] = True
                assert not (d & ~may).any(), (hw, fmt, siting, i, j, p)
                differing += int(d.sum())
    if nx > 1 or ny > 1:
        assert differing > 0                                                       # hostile tiles: the neighbour's pixel does differ


# -- 3. a single tile is section 21's emit -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", sorted(CC.FORMATS))
def test_a_single_tile_is_section_21s_sums(fmt):
    for k, (siting, (H, W)) in enumerate(itertools.product(CC.SITINGS, [(64, 64), (37, 53), (1, 1), (2, 3)])):
        matrix, rng = MATS[k % 3], FC.RANGES[k % 2]
        x = TC.hostile_tiles(1, T, seed=H + W + k)
        ref = CC.random_frame(1, H, W, fmt, seed=k, garbage=True)
        for O in (0, 16):
            assert XC.tile_sse(x, H, W, T, O, fmt, matrix, rng, siting, ref) == [[v * RC.den_of(O) ** 2 for v in CC.sums(x, 0, 0, H, W, fmt, matrix, rng, siting, ref)[0]]]
        assert XC.sse_exact(H, W, T, 0, fmt, siting) and not XC.sse_exact(H, W, T, 16, fmt, siting)


def test_edge_clamps_are_at_the_tiles_in_frame_part():
    """whatever a tile holds beyond the frame, and whatever its neighbours hold, its sums stay"""
    H, W, O = 65, 63, 0
    ref = CC.random_frame(1, H, W, "nv12", seed=9)
    x = np.array(hostile(H, W, O))
    for siting in CC.SITINGS:
        want = XC.tile_sse(x, H, W, T, O, "nv12", "bt601", "limited", siting, ref)
        y = x.copy()
        y[:, :, :, 63:] = 0.25                                                     # column 63 lies beyond W = 63
        y[1, :, 1:, :] = 0.75                                                      # tile 1 holds row 64 alone
        assert XC.tile_sse(y, H, W, T, O, "nv12", "bt601", "limited", siting, ref) == want
        y = x.copy()
        y[0] = 0.5                                                                 # tile 1 does not read tile 0
        assert XC.tile_sse(y, H, W, T, O, "nv12", "bt601", "limited", siting, ref)[1] == want[1]


# -- 4. the library, no device -------------------------------------------------------------------------------------------------------

def test_workspace_size_is_24_bytes_per_block():
    _, L = _lib()
    for size, n in [(64, 1), (64, 6), (128, 9), (512, 40), (1024, 3), (2048, 2)]:
        for sy in (1, 2):
            assert L.pc_chroma_rate_workspace_size(size, sy, n) == 24 * n * (size * size // (8 * sy * 256)), (size, sy, n)
            assert (size * size // (8 * sy)) % 256 == 0
    for bad in [(0, 2, 1), (32, 2, 1), (96, 1, 1), (-64, 2, 1), (4096, 2, 1), (64, 2, 0), (64, 1, -1), (64, 0, 1), (64, 3, 1), (64, -1, 1),
                (2048, 1, 2 ** 31 - 1)]:
        assert L.pc_chroma_rate_workspace_size(*bad) == 0, bad


def test_plan_is_host_only_and_each_precondition_is_broken_alone():
    """made-up pointer values: nothing may be dereferenced or launched (there is no GPU here)"""
    from progressivecodec_amd import chroma
    _, L = _lib()
    Fp = 0x7000_0100_0000
    H, W = 96, 160
    FS = (3 * T * T, T * T, T)

    def plan(fmt, ref, f32=Fp, fs=FS, O=0):
        f = chroma.FORMATS[fmt]
        wide = C.c_int(-1)
        rc = L.pc_chroma_rate_plan(f32, *fs, O, f.layout, f.bits, f.sx, C.byref(ref) if ref is not None else None, C.byref(wide))
        return rc, wide.value
    for fmt, f in chroma.FORMATS.items():
        es = 2 if f.bits == 10 else 1
        ok = fake_frame(chroma, fmt, H, W)
        assert plan(fmt, ok) == (0, 1)
        for off in (4, 8, 12):
            assert plan(fmt, ok, f32=Fp + off) == (0, 0)                                    # the floats: 16-byte aligned
        for k in range(3):
            fs = list(FS)
            fs[k] += 2
            assert plan(fmt, ok, fs=tuple(fs)) == (0, 0)                                    # their strides: multiples of 4
        for nm in ["y", "u"] + (["v"] if f.layout == chroma.PLANAR else []):
            for off in (1, 2, 3):
                bad = fake_frame(chroma, fmt, H, W)
                setattr(bad, nm, getattr(bad, nm) + off * es)                               # each plane: aligned to four elements
                assert plan(fmt, bad) == (0, 0), (fmt, nm, off)
            bad = fake_frame(chroma, fmt, H, W)
            setattr(bad, nm + "_row", getattr(bad, nm + "_row") + 2)                        # each row stride: a multiple of 4
            assert plan(fmt, bad) == (0, 0), (fmt, nm)
            free = fake_frame(chroma, fmt, H, W)
            setattr(free, nm + "_batch", getattr(free, nm + "_batch") + 1)                  # one frame per call: no batch stride counts
            assert plan(fmt, free) == (0, 1), (fmt, nm)
        # O a multiple of 8 at sx == 2; any O at 4:4:4
        for O in (0, 8, 16, 32, 4, 12, 20, 28):
            assert plan(fmt, ok, O=O) == (0, 1 if f.sx == 1 or O % 8 == 0 else 0), (fmt, O)
        assert plan(fmt, ok, O=-4)[0] == -1 and plan(fmt, ok, f32=None)[0] == -1 and plan(fmt, None)[0] == -1
        nul = fake_frame(chroma, fmt, H, W)
        nul.u = None
        assert plan(fmt, nul)[0] == -1
        assert L.pc_chroma_rate_plan(Fp, *FS, 0, f.layout, f.bits, f.sx, C.byref(ok), None) == -1
    wide = C.c_int(-1)
    f = fake_frame(chroma, "nv12", H, W)
    for lay, bits, sx in [(2, 8, 2), (-1, 8, 2), (1, 9, 2), (1, 16, 2), (1, 8, 3), (1, 8, 0)]:
        assert L.pc_chroma_rate_plan(Fp, *FS, 0, lay, bits, sx, C.byref(f), C.byref(wide)) == -1, (lay, bits, sx)
    assert plan("nv12", f) == (0, 1) and plan("i420", f)[0] == -1                           # a planar frame needs its V pointer


def test_every_argument_error_returns_before_the_device():
    """fake device pointers: every call below must return PC_ERR_ARG without touching them (no GPU here)"""
    from progressivecodec_amd import chroma, frames
    _, L = _lib()
    Fp, Wk, S = 0x7000_0100_0000, 0x7000_0200_0000, 0x7000_0300_0000
    H, W, O = 100, 150, 16                                                        # 2 x 3 tiles, S = 48
    k = frames.coefficients("bt709")
    for fmt, f in chroma.FORMATS.items():
        Hc, Wc = chroma.chroma_size(H, W, fmt)
        semi = f.layout == chroma.SEMIPLANAR

        def broken(field, value):
            fr = fake_frame(chroma, fmt, H, W)
            setattr(fr, field, value)
            return fr
        bad_frames = [broken("y", None), broken("u", None), broken("y_row", W - 1), broken("u_row", (2 * Wc if semi else Wc) - 1)]
        if not semi:
            bad_frames += [broken("v", None), broken("v_row", Wc - 1)]
        if f.bits == 10:
            bad_frames += [broken("y", fake_frame(chroma, fmt, H, W).y + 1), broken("u", fake_frame(chroma, fmt, H, W).u + 1)]
        nbytes = L.pc_chroma_rate_workspace_size(T, f.sy, 6)
        assert nbytes == 24 * 6 * (2 // f.sy)
        ok = dict(x=Fp, sxt=3 * T * T, sxc=T * T, sxh=T, H=H, W=W, T=T, O=O, first=0, n=6, layout=f.layout, bits=f.bits, shift=f.shift, sx=f.sx,
                  sy=f.sy, hsite=1, vsite=0, range=0, kr=k.kr, kg=k.kg, kb=k.kb, ib=k.ib, ir=k.ir, ref=fake_frame(chroma, fmt, H, W), ws=Wk,
                  nbytes=nbytes, out=S, stream=None)
        bads = [dict(ref=fr) for fr in bad_frames] + [
            dict(x=None), dict(x=Fp + 1), dict(sxh=T - 1), dict(sxc=0), dict(sxt=0),
            # the format tuple: unknown layout, depth, shift for the depth, subsampling
            dict(layout=2), dict(layout=-1), dict(bits=9), dict(bits=16), dict(shift=1), dict(shift=6 if f.bits == 8 else 4), dict(sx=1, sy=2),
            dict(sx=3), dict(sy=0), dict(sx=4, sy=1), dict(hsite=2), dict(hsite=-1), dict(vsite=2), dict(vsite=-1), dict(range=2), dict(range=-1),
            dict(H=0), dict(W=0), dict(H=-5), dict(T=0), dict(T=32), dict(T=96), dict(T=-64), dict(T=4096, O=0), dict(O=2), dict(O=6),
            dict(O=36), dict(O=-4), dict(first=-1), dict(first=1), dict(n=0), dict(n=7), dict(n=-1), dict(first=6, n=1),
            dict(first=2 ** 31 - 1, n=2 ** 31 - 1), dict(ws=None), dict(ws=Wk + 4), dict(out=None), dict(out=S + 4), dict(nbytes=nbytes - 1),
            dict(nbytes=0)]
        if f.bits == 10:
            bads.append(dict(T=2048, O=0, n=1, nbytes=1 << 30))                   # the sums of 10-bit codes fit up to T = 1024
        for bad in bads:
            a = dict(ok, **bad)
            args = [C.byref(v) if isinstance(v, frames.Frame) else v for v in a.values()]
            assert L.pc_chroma_rate_tile_sse(*args) == -1, (fmt, bad)
        a = dict(ok, ref=None)
        assert L.pc_chroma_rate_tile_sse(*a.values()) == -1


def test_python_rejects_before_any_device_call(monkeypatch):
    from progressivecodec_amd import chroma_rate as cr

    def touched(*a, **k):
        raise AssertionError("the device was reached")
    for name in ("device", "current_stream", "synchronize", "current_device", "_lazy_init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.setattr(cr, "lib", touched)
    g = cr.grid_of(100, 150, 64, 16)
    x = torch.zeros(6, 3, 64, 64)
    yy, uu = torch.zeros(100, 150, dtype=torch.uint8), torch.zeros(50, 75, 2, dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU"):
        cr.frame_tile_distortion(x, g, (yy, uu), "nv12")
    with pytest.raises(ValueError, match="fmt"):
        cr.frame_tile_distortion(x, g, (yy, uu), "nv21")
    with pytest.raises(ValueError, match="matrix"):
        cr.frame_tile_distortion(x, g, (yy, uu), "nv12", matrix="bt470")
    with pytest.raises(ValueError, match="range"):
        cr.frame_tile_distortion(x, g, (yy, uu), "nv12", range="tv")
    with pytest.raises(ValueError, match="siting"):
        cr.frame_tile_distortion(x, g, (yy, uu), "nv12", siting="top")
    with pytest.raises(TypeError, match="float32"):
        cr.frame_tile_distortion(x.double(), g, (yy, uu), "nv12")
    with pytest.raises(ValueError, match="outside"):
        cr.frame_tile_distortion(x, g, (yy, uu), "nv12", first_tile=1)
    with pytest.raises(ValueError, match="outside"):
        cr.frame_tile_distortion(x[:1], g, (yy, uu), "nv12", first_tile=-1)
    with pytest.raises(ValueError, match="n >= 1"):
        cr.frame_tile_distortion(x[:0], g, (yy, uu), "nv12")
    with pytest.raises(ValueError, match="x_hat_tiles must be"):
        cr.frame_tile_distortion(x[:, :2], g, (yy, uu), "nv12")
    with pytest.raises(ValueError, match="the grid of"):
        cr.frame_tile_distortion(x, g._replace(ny=3, nty=3), (yy, uu), "nv12")
    with pytest.raises(ValueError, match="ref: UV must be"):
        cr.frame_tile_distortion(x, g, (yy, uu[:2]), "nv12")
    with pytest.raises(ValueError, match="ref: UV must be"):
        cr.frame_tile_distortion(x, g, (yy, uu), "nv16")                           # 4:2:2 has a chroma row per luma row
    with pytest.raises(ValueError, match="tuple of 3 planes"):
        cr.frame_tile_distortion(x, g, (yy, uu), "i444")
    with pytest.raises(ValueError, match="one frame"):
        cr.frame_tile_distortion(x, g, (yy.expand(2, 100, 150), uu.expand(2, 50, 75, 2)), "nv12")
    with pytest.raises(TypeError, match="uint16"):
        cr.frame_tile_distortion(x, g, (yy, uu), "p010")
    big = cr.grid_of(5000, 5000, 2048, 0)
    y16 = yy.to(torch.uint16)
    for fmt10 in ("p010", "p210", "p410", "i010", "i210", "i410"):
        with pytest.raises(ValueError, match="at most 1024"):
            cr.frame_tile_distortion(torch.zeros(1, 3, 1, 1).expand(1, 3, 2048, 2048), big, (y16, y16), fmt10)
    with pytest.raises(ValueError, match="at most 2048"):
        cr.frame_tile_distortion(torch.zeros(1, 3, 1, 1).expand(1, 3, 4096, 4096), cr.grid_of(5000, 5000, 4096, 0), (yy, uu), "nv24")
    enc = lambda **kw: cr.encode_frame_tiled_to_size(None, (yy, uu), [0, 1], 10 ** 6, "nv12", **dict(dict(tile=64), **kw))     # noqa: E731
    with pytest.raises(ValueError, match="GPU"):
        enc()
    with pytest.raises(ValueError, match="max_tiles_per_call"):
        enc(max_tiles_per_call=0)
    for bad in [(1, 1), (1, 1, -1), (0, 0, 0), (1.0, 1, 1), (True, 1, 1)]:
        with pytest.raises(ValueError, match="plane_weights"):
            enc(plane_weights=bad)
    with pytest.raises(ValueError, match="at least one level"):
        cr.encode_frame_tiled_to_size(None, (yy, uu), [], 10 ** 6, "nv12", tile=64)
    with pytest.raises(ValueError, match="upsample"):
        enc(upsample="cubic")
    with pytest.raises(ValueError, match="siting"):
        enc(siting="right")
    assert cr.ChromaRatePlan._fields == ("levels", "rates", "dists", "plane_dists", "den", "container_bytes", "predicted", "sse", "sse_exact")
    from progressivecodec_amd import frame_rate
    assert cr.ChromaRatePlan._fields[:-1] == frame_rate.FrameRatePlan._fields
    # sse_exact is the contract's rule
    for fmt, siting, hw, O in itertools.product(sorted(CC.FORMATS), CC.SITINGS, [(100, 150), (64, 150), (100, 64), (37, 53)], (0, 16)):
        assert cr.sse_exact(cr.grid_of(*hw, T, O), fmt, siting) is XC.sse_exact(*hw, T, O, fmt, siting), (fmt, siting, hw, O)


def test_max_tile_for_all_twelve_formats():
    from progressivecodec_amd import _tilecodec, chroma, chroma_rate
    for fmt, f in chroma.FORMATS.items():
        want = 1024 if f.bits == 10 else 2048
        assert _tilecodec.max_tile(fmt) == chroma_rate.max_tile(fmt) == XC.max_tile(fmt) == want, fmt
        _tilecodec.tile_limit(want, fmt)
        with pytest.raises(ValueError, match=f"at most {want}"):
            _tilecodec.tile_limit(2 * want, fmt)
    assert sorted(f for f in chroma.FORMATS if _tilecodec.max_tile(f) == 1024) == ["i010", "i210", "i410", "p010", "p210", "p410"]


# -- 5. structure --------------------------------------------------------------------------------------------------------------------

def test_the_fourteenth_library_keeps_the_rules_of_the_thirteen():
    cr, L = _lib()
    from progressivecodec_amd import chroma
    hdr = open(os.path.join(DIR, "pc_chroma_rate.h")).read()
    declared = re.findall(r"PC_API\s+[\w\s\*]+?\b(pc_\w+)\s*\(", hdr)
    assert len(declared) == 5 and sorted(declared) == sorted(cr.EXPORTS)
    for name in declared:
        getattr(L, name)
    assert L.pc_chroma_rate_strerror(-1).decode() and L.pc_chroma_rate_strerror(-6).decode() and L.pc_chroma_rate_last_hip_error() == 0
    assert cr.LIB_PATH == os.path.join(PKG, "libpc_chroma_rate.so")
    assert issubclass(cr.ChromaRateError, cr._imagelib.ImageLibError)
    mk = image_shared.uncommented(os.path.join(DIR, "Makefile"))
    assert mk == "NAME := chroma_rate\ninclude ../image_csrc/lib.mk\n"
    rule = image_shared.uncommented(os.path.join(PKG, "image_csrc", "lib.mk"))
    assert "-ffp-contract=off" in rule and not re.search(r"-lpc|libpc(odec|_\w+)\b", rule.replace("libpc_$(NAME)", ""))
    top = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\bchroma_rate\b", top, re.M) and re.search(r"^\.PHONY:.*\bchroma_rate\b", top, re.M)
    assert "$(MAKE) -C ../chroma_rate_hip clean" in top and re.search(r"^chroma_rate:\n\t\$\(MAKE\) -C \.\./chroma_rate_hip$", top, re.M)
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(DIR, "*")) if not p.endswith((".o", ".so")))
    assert names == ["Makefile", "pc_chroma_rate.h", "pc_chroma_rate.hip"]
    assert len(glob.glob(os.path.join(PKG, "*_csrc", "*.hip"))) == len(image_shared.LIBS) == 10
    assert len(glob.glob(os.path.join(PKG, "*_hip", "*.hip"))) == 4
    src = open(os.path.join(DIR, "pc_chroma_rate.hip")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert '#include "pc_image_host.h"' in src
    for other in ("pc_chroma.h", "pc_chroma_tiles.h", "pc_frame_rate.h", "pc_yuv_items.h"):
        assert other not in code, other
    for name, pattern in DEFINITIONS.items():
        assert not re.search(pattern, code), name
    shared = ("HIPCHK", "g_last_hip", "Planes", "planes_of", "load4", "Levels", "EmitCoef", "emit_px", "clampi", "block_reduce",
              "row_final", "plane_wide", "f32_wide", "aligned", "F32", "Grid", "Geo", "geo_of", "axis_weight", "NT", "COLS", "Sum",
              "code_of", "Fmt", "format_of", "with_format", "picture_ok", "site_ok", "depth_levels")
    for name in shared:
        assert re.search(r"\b%s\b" % name, code), name
        assert not re.search(r"\b(struct|void|int|bool|unsigned|float|define|constexpr int)\s+%s\b\s*[({=]" % name, code), name
    image_shared.assert_frame_is_shared(hdr, "pc_chr_frame")
    found = dict(re.findall(r"\b(PC_CHR_(?:LIMITED|FULL)) = (\w+)", hdr))
    assert found == {"PC_CHR_" + k: "PC_YUV_" + k for k in ("LIMITED", "FULL")}
    assert "PC_YUV_" not in re.sub(r"PC_YUV_(LIMITED|FULL|NV12|P010)\b", "", hdr + code)
    values = dict((k, int(v)) for k, v in re.findall(r"\b(PC_CHR_\w+) = (\d+)", hdr))
    assert values == {"PC_CHR_PLANAR": chroma.PLANAR, "PC_CHR_SEMIPLANAR": chroma.SEMIPLANAR, "PC_CHR_CENTRE": chroma.CENTRE,
                      "PC_CHR_COSITED": chroma.COSITED}
    assert not re.search(r"\batomic\w*\b|\basm\b|__asm|__shared__|__syncthreads|__builtin_amdgcn", code.replace("std::atomic", ""))
    assert "atomic" not in code and "asm" not in re.findall(r"\b\w+\b", code)
    import bench
    text = inspect.getsource(bench.source_hash)
    assert "chroma" not in text and "_hip" not in text and "rate" not in text
    from progressivecodec_amd import _imagelib, frame_rate
    assert "thirteen" in _imagelib.__doc__ and "chroma_tiles" in _imagelib.__doc__ and "chroma_rate" in _imagelib.__doc__
    assert "chroma_rate" in frame_rate.__doc__
    assert "chroma_rate" in open(os.path.join(ROOT, "README.md")).read()


# -- 6. the ledger -------------------------------------------------------------------------------------------------------------------

def test_every_instantiation_is_launched():
    """pc_chroma_rate.hip: "32 sse kernels and the final".  The tuples the table reaches are exactly those; a case taken away shows
    here by the name of the kernel nothing launches any more"""
    src = open(os.path.join(DIR, "pc_chroma_rate.hip")).read()
    assert "32 sse kernels and the final" in src
    assert len(RS.ALL) == 32
    table = RS.table()
    assert len(table) == 12 * 6 + 4 * 5 and len(set(table)) == len(table)
    got = RS.reached(table)
    assert got == RS.ALL, "never launched: %s" % RS.names(RS.ALL - got)
    # the cases the issue names: all twelve formats x three sitings at 100 x 150 with O in {0, 4}; the other sizes with O in {16, 32}
    assert {(c.fmt, c.siting, c.O) for c in table if (c.H, c.W) == (100, 150)} == set(itertools.product(CC.FORMATS, CC.SITINGS, (0, 4)))
    assert {(c.fmt, c.H, c.W) for c in table if c.n >= 100} == set((f, H, W) for f in RS.OTHER_FORMATS for H, W in RS.OTHER_SIZES)
    assert set(RS.OTHER_SIZES) == {(1, 1), (2, 3), (3, 2), (65, 63), (127, 129)}
    assert {c.O for c in table if c.n >= 100} == {16, 32} and {(c.matrix, c.rng) for c in table if c.n >= 100} == set(RS.OTHER_SETTINGS)
    assert {c.siting for c in table if c.n >= 100} == set(CC.SITINGS)
    # both paths for every format, and an aligned O = 4 that is wide at 4:4:4 alone
    for fmt in CC.FORMATS:
        assert {RS.wide(c) for c in table if c.fmt == fmt and c.n < 100} == {False, True}
        assert {RS.wide(c) for c in table if c.fmt == fmt and c.n < 100 and c.aligned and c.O == 4} == {CC.sub(fmt)[0] == 1}
    # the ledger notices a case that leaves
    less = [c for c in table if not (c.fmt == "i010" and c.siting == "topleft" and c.aligned)]
    assert RS.ALL - RS.reached(less) == {(2, False, 2, 2, True, True)}
    assert RS.names([(2, False, 2, 2, True, True)]) == ["u16 planar 2:2 vco wide"]

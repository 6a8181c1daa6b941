"""Rate-controlled tiled coding of YUV frames of any subsampling and siting on the GPU (progressivecodec_amd/chroma_rate.py,
libpc_chroma_rate.so) against its restatement (tests/chroma_rate_contract.py): the per-tile, per-plane distortion sums exactly, on both
access paths, against frame_rate and against the stitch on the device, and encode_frame_tiled_to_size through the codec and a PCT2
container inside PCK1.  Every comparison is exact equality of integers or bytes.  T = 64 unless said otherwise.  The matrix is
tests/chroma_rate_cases.py's table; every case asserts the access path the table predicts."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import chroma_contract as CC
from tests import chroma_rate_cases as RS
from tests import chroma_rate_contract as XC
from tests import chroma_tiles_contract as KC
from tests import frames_contract as FC
from tests import image_limits as IL
from tests import rate_contract as RC
from tests import tiles_contract as TC
from tests.test_gpu_chroma_tiles import codec_frame, frame_views, on_device, struct_of
from tests.test_gpu_rate import POISON64, check_out, float_tiles
from tests.util import gpu_codec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POL = "point-based-std"
T = RS.T


def CR():
    from progressivecodec_amd import chroma_rate
    return chroma_rate


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def sse_raw(x, H, W, O, first, fmt, rng, matrix, siting, ref, size=T, nbytes=None, strides=None, **raw):
    """pc_chroma_rate_tile_sse on the tiles x holds -> (status, wide as pc_chroma_rate_plan reports it, the [n + 2, 3] buffer whose rows
    1 .. n are `out`, poisoned beforehand, whether every partial of the workspace and no word after it was written -- or, for a refused
    call, none at all).  ref: Views.  raw: format, siting and range integers that replace the named ones, for the calls that are to be
    refused."""
    from progressivecodec_amd import chroma, frames
    L = CR().lib()
    n = x.shape[0]
    f, (hs, vs) = chroma.FORMATS[fmt], chroma.SITINGS[siting]
    a = dict(f._asdict(), hsite=hs, vsite=vs, range=frames.RANGES[rng])
    a.update(raw)
    buf = torch.full((n + 2, 3), POISON64, dtype=torch.int64, device=DEV)
    need = L.pc_chroma_rate_workspace_size(size, f.sy, n)
    assert need == (24 * n * (size * size // (8 * f.sy * 256)) if size <= 2048 else 0)
    ws = torch.full((need // 8 + 1,), POISON64, dtype=torch.int64, device=DEV)
    k = frames.coefficients(matrix)
    rs = struct_of(ref)
    st = strides if strides is not None else (x.stride(0), x.stride(1), x.stride(2))
    wide = C.c_int(-1)
    assert L.pc_chroma_rate_plan(x.data_ptr(), *st, O, f.layout, f.bits, f.sx, C.byref(rs), C.byref(wide)) == 0
    rc = L.pc_chroma_rate_tile_sse(x.data_ptr(), *st, H, W, size, O, first, n, a["layout"], a["bits"], a["shift"], a["sx"], a["sy"], a["hsite"],
                                   a["vsite"], a["range"], k.kr, k.kg, k.kb, k.ib, k.ir, C.byref(rs), ws.data_ptr(),
                                   need if nbytes is None else nbytes, buf[1:].data_ptr(), stream())
    h = ws.cpu()
    return rc, wide.value, buf, bool(h[-1] == POISON64 and ((h[:-1] != POISON64).all() if rc == 0 else (h == POISON64).all()))


# -- 1. the matrix -------------------------------------------------------------------------------------------------------------------

def run_matrix(cases):
    """every case: hostile tiles (NaN, +-inf, values outside [0, 1]) against a reference with random bits outside its 10-bit codes;
    the whole grid, a sub-range, every tile alone; the Python call on a side stream and on views it has to copy"""
    cr = CR()
    for c in cases:
        H, W, O = c.H, c.W, c.O
        ny, nx = TC.grid(H, W, T, O)
        n = ny * nx
        f = CC.random_frame(1, H, W, c.fmt, seed=1000 * H + W + c.n, garbage=True)
        x_np = TC.hostile_tiles(n, T, seed=77 * H + W + c.n)
        want = XC.tile_sse(x_np, H, W, T, O, c.fmt, c.matrix, c.rng, c.siting, f)
        xv = float_tiles(x_np, c.variant)
        refv = frame_views(c.fmt, H, W, 0, c.aligned, f)
        for first, m in [(0, n)] + ([(1, n - 1)] if n > 1 else []) + [(t, 1) for t in range(n)]:
            rc, wide, buf, ws_ok = sse_raw(xv[first:first + m], H, W, O, first, c.fmt, c.rng, c.matrix, c.siting, refv)
            assert rc == 0 and ws_ok, (c, first, m)
            assert wide == int(RS.wide(c)), c
            check_out(buf, want[first:first + m], (c, first, m))
        g = cr.grid_of(H, W, T, O)
        planes = on_device(f)
        assert cr.plan(xv, [v.t for v in refv], c.fmt, overlap=O) is RS.wide(c)
        # the Python call: channels last in memory (copied), a luma plane whose innermost stride is not 1 (copied), a sub-range on a
        # second stream
        cl = torch.from_numpy(x_np).to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        wider = torch.from_numpy(np.repeat(f[0][0], 2, axis=1)).to(DEV)[:, ::2]
        got = cr.frame_tile_distortion(cl, g, (wider,) + planes[1:], c.fmt, c.matrix, c.rng, c.siting)
        assert got.dtype == torch.int64 and got.shape == (n, 3) and got.device.type == "cuda" and got.tolist() == want, c
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            got_s = cr.frame_tile_distortion(xv[n - 1:], g, tuple(v.t[0] for v in refv), c.fmt, c.matrix, c.rng, c.siting, first_tile=n - 1)
        side.synchronize()
        assert got_s.tolist() == want[n - 1:], c


@pytest.mark.parametrize("fmt", sorted(CC.FORMATS))
def test_every_format_and_siting_is_the_restatement_exactly(fmt):
    run_matrix(RS.main_cases(fmt))


@pytest.mark.parametrize("fmt", RS.OTHER_FORMATS)
def test_the_other_sizes_overlaps_matrices_and_full_range(fmt):
    run_matrix(RS.other_cases(fmt))


def band_cases():
    """O = 24 (S = 40, den = 48: wide where the views allow it) and O = 28 (S = 36, den = 56: narrow at sx = 2, wide at 4:4:4) on
    100 x 150: one format per kernel shape and element width, every siting, aligned and not.  Not part of tests/chroma_rate_cases.py's
    ledger: no instantiation depends on them."""
    shapes = [("nv12", "topleft"), ("p010", "centre"), ("nv16", "left"), ("i210", "centre"), ("i444", "left"), ("p410", "topleft")]
    out = []
    for n, ((fmt, siting), O) in enumerate((s, O) for s in shapes for O in (24, 28)):
        matrix, rng = RS.OTHER_SETTINGS[n % len(RS.OTHER_SETTINGS)]
        for aligned in (True, False):
            out.append(RS.Case(fmt, matrix, rng, siting, 100, 150, O, 200 + n, *RS.layout_of(n, aligned)))
    return out


def test_overlaps_whose_band_quotients_are_no_floats():
    """the sums weigh with the integer numerators 2u + 1, which are exact whatever 2 O is; what is new is the band geometry.  Every
    case asserts the access path chroma_rate_cases.wide predicts."""
    cases = band_cases()
    assert {RS.wide(c) for c in cases if c.O == 24} == {True, False}
    assert {(RS.wide(c), CC.sub(c.fmt)[0]) for c in cases if c.O == 28} == {(False, 2), (True, 1), (False, 1)}
    run_matrix(cases)


# -- 2. both paths on the same data --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,siting", [("nv16", "left"), ("p210", "topleft"), ("i444", "centre"), ("nv12", "topleft"), ("i010", "left")])
def test_wide_and_narrow_agree_on_the_same_data(fmt, siting):
    """one frame and one tile set under every alignment: aligned and pitched, offset planes; aligned, strided and misaligned tiles"""
    H, W = 65, 150
    sx, _ = CC.sub(fmt)
    f = CC.random_frame(1, H, W, fmt, seed=9, garbage=True)
    for O in (0, 4, 16):
        ny, nx = TC.grid(H, W, T, O)
        x = TC.hostile_tiles(ny * nx, T, seed=O)
        want = XC.tile_sse(x, H, W, T, O, fmt, "bt2020", "limited", siting, f)
        seen = set()
        for aligned in (True, False):
            refv = frame_views(fmt, H, W, 0, aligned, f)
            for variant in ("contiguous", "loose4", "odd"):
                rc, wide, buf, ws_ok = sse_raw(float_tiles(x, variant), H, W, O, 0, fmt, "limited", "bt2020", siting, refv)
                assert rc == 0 and ws_ok and wide == int(aligned and variant != "odd" and (sx == 1 or O % 8 == 0)), (fmt, O, aligned, variant)
                seen.add(wide)
                check_out(buf, want, (fmt, siting, O, aligned, variant))
        assert seen == ({0, 1} if sx == 1 or O % 8 == 0 else {0})


# -- 3. against frame_rate on the device ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_centre_sited_420_is_frame_rate_on_the_device(fmt):
    from progressivecodec_amd import frame_rate
    cr = CR()
    H, W = 100, 150
    planes = on_device(FC.random_frame(1, H, W, fmt, seed=3))
    for O in (0, 16):
        g = cr.grid_of(H, W, T, O)
        x = torch.from_numpy(TC.hostile_tiles(g.n, T, seed=O)).to(DEV)
        for matrix, rng in [("bt601", "full"), ("bt709", "limited")]:
            a = cr.frame_tile_distortion(x, g, planes, fmt, matrix, rng)
            b = frame_rate.frame_tile_distortion(x, g, planes, fmt, matrix, rng)
            assert torch.equal(a, b) and a.sum().item() > 0, (fmt, O, matrix, rng)
            assert torch.equal(cr.frame_tile_distortion(x[2:5], g, planes, fmt, matrix, rng, first_tile=2), b[2:5])


# -- 4. against the stitch -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,siting,hw", [("i444", "centre", (100, 150)), ("nv16", "centre", (100, 150)), ("nv12", "left", (100, 150)),
                                           ("nv12", "topleft", (37, 53))])
def test_without_overlap_the_tiles_sums_relate_to_the_stitchs_as_the_contract_says(fmt, siting, hw):
    from progressivecodec_amd import chroma_tiles
    cr = CR()
    H, W = hw
    g = cr.grid_of(H, W, T, 0)
    exact = cr.sse_exact(g, fmt, siting)
    assert exact is XC.sse_exact(H, W, T, 0, fmt, siting) and exact is ((fmt, siting) != ("nv12", "left"))
    x_np = TC.hostile_tiles(g.n, T, seed=H * W)
    x = torch.from_numpy(x_np).to(DEV)
    f = CC.random_frame(1, H, W, fmt, seed=3, garbage=True)
    planes = on_device(f)
    for k, rng in enumerate(FC.RANGES):
        matrix = list(FC.MATRICES)[k]
        per_tile = cr.frame_tile_distortion(x, g, planes, fmt, matrix, rng, siting).sum(0).tolist()
        whole = chroma_tiles.stitch_frame(x, g, fmt, matrix, rng, siting, ref=planes, image=False).sse[0].tolist()
        assert per_tile[0] == whole[0], (fmt, siting, rng)
        if exact:
            assert per_tile == whole, (fmt, siting, rng)
        else:
            # the first chroma column of the tiles with j > 0 reads its own first pixel: the restatements say by how much
            want = [sum(r[p] for r in XC.tile_sse(x_np, H, W, T, 0, fmt, matrix, rng, siting, f)) for p in range(3)]
            assert per_tile == want and whole == KC.sums(x_np, H, W, T, 0, fmt, matrix, rng, siting, f) and per_tile[1:] != whole[1:]


# -- 5. the halo ---------------------------------------------------------------------------------------------------------------------

def lit_case(fmt, siting, H, W, O, axis, p, tile, size=T):
    """gray tiles in which tile `tile` has its luma column (axis 1) or row (axis 0) p, in TILE coordinates, blue: both paths against
    the restatement -> the tile's chroma codes (Cb) with and without the light"""
    ny, nx = TC.grid(H, W, size, O)
    gray = np.full((ny * nx, 3, size, size), 0.5, np.float32)
    x = gray.copy()
    idx = [tile, slice(None), slice(None), slice(None)]
    idx[2 + axis] = p
    x[tuple(idx)] = np.array([0.0, 0.0, 1.0], np.float32)[:, None]
    f = CC.random_frame(1, H, W, fmt, seed=5, garbage=True)
    want = XC.tile_sse(x, H, W, size, O, fmt, "bt709", "limited", siting, f)
    assert want[tile] != XC.tile_sse(gray, H, W, size, O, fmt, "bt709", "limited", siting, f)[tile]
    for aligned, variant in [(True, "contiguous"), (False, "odd")]:
        rc, wide, buf, ws_ok = sse_raw(float_tiles(x, variant, size), H, W, O, 0, fmt, "limited", "bt709", siting,
                                       frame_views(fmt, H, W, 0, aligned, f), size)
        assert rc == 0 and ws_ok and wide == int(aligned and (CC.sub(fmt)[0] == 1 or O % 8 == 0)), (fmt, siting, O, axis, p, tile, variant)
        check_out(buf, want, (fmt, siting, H, W, O, axis, p, tile, variant))
    lit = XC.tile_parts(x[tile:tile + 1], H, W, size, O, fmt, "bt709", "limited", siting, tile)[0][2][1]
    dark = XC.tile_parts(gray[tile:tile + 1], H, W, size, O, fmt, "bt709", "limited", siting, tile)[0][2][1]
    return lit, dark


@pytest.mark.parametrize("fmt,siting", [("nv12", "left"), ("nv12", "topleft"), ("nv16", "left"), ("i010", "topleft"), ("p210", "topleft")])
def test_a_lit_column_reaches_the_chroma_samples_the_rule_names_inside_its_tile(fmt, siting):
    """tile columns 8k - 1 (the halo pixel of item k), 0 (the tile's left edge stands in for the column left of it) and ww - 1 (the
    odd last column of the ragged last tile of 127 x 129), in a tile with j > 0: the sample right of the column changes, too, and no
    sample of another column does"""
    H, W = 127, 129                                                            # 2 x 3 tiles at O = 0 and 4: the last is 1 column wide
    for O in (0, 4):
        ny, nx = TC.grid(H, W, T, O)
        ww = W - (nx - 1) * (T - O)
        for tile, p in [(1, 7), (1, 31), (1, 63), (nx + 1, 0), (nx - 1, ww - 1), (2 * nx - 1, 0)]:
            lit, dark = lit_case(fmt, siting, H, W, O, 1, p, tile)
            changed = {m for m in range(lit.shape[1]) if (lit[:, m] != dark[:, m]).any()}
            assert changed == {m for m in (p // 2, (p + 1) // 2) if m < lit.shape[1]}, (fmt, siting, O, tile, p)


@pytest.mark.parametrize("fmt,size", [("nv12", 64), ("i010", 64), ("p010", 64), ("nv12", 128)])
def test_a_lit_row_reaches_the_chroma_rows_the_rule_names_inside_its_tile(fmt, size):
    """the same along columns, under "topleft": tile rows 2i - 1 (the halo row of the item below), 0 and hh - 1 (the odd last row of
    the ragged last tile row); at T = 128 a tile has four blocks of 32 rows, and row 31 is the halo row of another block's items"""
    H, W = (127, 129) if size == 64 else (130, 200)
    for O in (0, 4) if size == 64 else (8,):
        ny, nx = TC.grid(H, W, size, O)
        hh = H - (ny - 1) * (size - O)
        for tile, p in [(0, 31), (1, 7), (nx, 0), ((ny - 1) * nx + 1, hh - 1)] + ([(0, 63), (1, 95)] if size == 128 else []):
            lit, dark = lit_case(fmt, "topleft", H, W, O, 0, p, tile, size)
            changed = {k for k in range(lit.shape[0]) if (lit[k] != dark[k]).any()}
            assert changed == {k for k in (p // 2, (p + 1) // 2) if k < lit.shape[0]}, (fmt, O, tile, p)


def test_sy_1_has_two_blocks_per_tile_and_a_lit_column_crosses_neither():
    """at 4:2:2 a 64-tile is two blocks of 32 rows: a lit column (item boundary 8k - 1) runs through both, a lit row 31 / 32 through
    one each; 4:4:4 has no filter at all"""
    for fmt, siting in [("nv16", "left"), ("p210", "topleft"), ("i444", "left")]:
        for axis, p in [(1, 39), (0, 31), (0, 32)]:
            lit, dark = lit_case(fmt, siting, 100, 150, 0, axis, p, 1)
            if axis == 0:
                assert {k for k in range(lit.shape[0]) if (lit[k] != dark[k]).any()} == {p}
            else:
                changed = {m for m in range(lit.shape[1]) if (lit[:, m] != dark[:, m]).any()}
                assert changed == ({p} if fmt == "i444" else {(p - 1) // 2, (p + 1) // 2})


# -- 6. limits -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,size", [("i444", 2048), ("p410", 1024)])
def test_the_largest_weights_meet_the_largest_error(fmt, size):
    """the largest tile and overlap of the depth, the reference at the top code in full range against all-zero tiles (which render
    as code 0 and the chroma offset): the centre tile of the 3 x 3 grid alone, against the closed form -- at 4:4:4 chroma weighs as
    luma does, and T^4 (2^n - 1)^2 < 2^60 holds for it just the same"""
    cr = CR()
    H = W = 2 * size
    O = size // 2
    g = cr.grid_of(H, W, size, O)
    assert (g.ny, g.nx) == (3, 3) and size == XC.max_tile(fmt)
    yo, ys, co, cs, mx = CC.levels(fmt, "full")
    dt = np.uint16 if CC.bits(fmt) == 10 else np.uint8
    top = mx << CC.FORMATS[fmt][2]
    planes = tuple(torch.from_numpy(np.full(s, top, dt)).to(DEV) for s in ([(H, W)] * 3 if fmt == "i444" else [(H, W), (H, W, 2)]))
    x = torch.zeros((1, 3, size, size), dtype=torch.float32, device=DEV)
    wsum = IL.axis_weight_sum(1, 3, size, O)
    assert wsum == O * O + 2 * O * (size - 2 * O) + O * O
    want = [(mx - yo) ** 2 * wsum * wsum, (mx - co) ** 2 * wsum * wsum, (mx - co) ** 2 * wsum * wsum]
    assert max(want) < 2 ** 60 and want[0] > 2 ** 55
    assert cr.plan(x, [p[None] for p in planes], fmt, overlap=O)
    assert cr.frame_tile_distortion(x, g, planes, fmt, "bt709", "full", "centre", first_tile=4).tolist() == [want]
    odd = torch.zeros(3 * size * size + 1, dtype=torch.float32, device=DEV)[1:].view(1, 3, size, size)
    assert not cr.plan(odd, [p[None] for p in planes], fmt, overlap=O)
    assert cr.frame_tile_distortion(odd, g, planes, fmt, "bt709", "full", "centre", first_tile=4).tolist() == [want]


def test_refused_calls_launch_nothing():
    cr = CR()
    L = cr.lib()
    H, W, O = 100, 150, 16
    x = torch.rand(6, 3, T, T, device=DEV)
    for fmt in ("nv12", "p210", "i444"):
        sy = CC.sub(fmt)[1]
        refv = frame_views(fmt, H, W, 0, True, CC.random_frame(1, H, W, fmt, seed=1))
        big = lambda size: dict(size=size, O=0, n=1, strides=(3 * size * size, size * size, size))                 # noqa: E731
        bads = [dict(first=1), dict(first=-1), dict(O=6), big(4096), dict(nbytes=L.pc_chroma_rate_workspace_size(T, sy, 6) - 1), dict(layout=2),
                dict(bits=9), dict(shift=3), dict(sx=1, sy=2), dict(hsite=2), dict(vsite=-1), dict(range=2), dict(range=-1)]
        bads += [big(2048)] if fmt == "p210" else []
        for kw in bads:
            a = dict(dict(H=H, W=W, O=O, first=0, fmt=fmt, rng="limited", matrix="bt709", siting="left", ref=refv), **kw)
            rc, _, buf, ws_ok = sse_raw(x[:a.pop("n", 6)], **a)
            torch.cuda.synchronize()
            assert rc == -1 and (buf == POISON64).all() and ws_ok, (fmt, kw)
        rc, _, buf, ws_ok = sse_raw(x, H, W, O, 0, fmt, "limited", "bt709", "left", refv)                          # unspoilt, it goes through
        assert rc == 0 and ws_ok and (buf[1:-1] != POISON64).all() and (buf[0] == POISON64).all() and (buf[-1] == POISON64).all()
    with pytest.raises(cr.ChromaRateError, match="PC_ERR_ARG"):
        raise cr.ChromaRateError(-1, "pc_chroma_rate_tile_sse")


def test_offsets_past_2_to_the_31():
    """two tiles at a tile stride past 2^31 bytes and a luma plane whose last rows lie past 2^31 bytes, inside one untouched
    allocation: every offset is 64-bit"""
    cr = CR()
    BIG = 2 ** 31 + 4096                                                   # tile stride in bytes
    ROW = 2 ** 26 + 64                                                     # luma row stride in bytes: row 32 starts past 2^31
    need = 2 * BIG + (16 << 20)
    free = torch.cuda.mem_get_info(DEV)[0]
    if free < need + (1 << 30):
        pytest.skip(f"{free >> 20} MiB of device memory free, the strided views need {need >> 20} MiB")
    buf = torch.empty(need, dtype=torch.uint8, device=DEV)
    H, W, O = 40, 100, 0                                                   # 1 x 2 tiles
    fmt, siting = "nv16", "left"
    f = CC.random_frame(1, H, W, fmt, seed=31)
    y = torch.as_strided(buf, (1, H, W), (H * ROW, ROW, 1), 8 << 20)
    y.copy_(torch.from_numpy(f[0]))
    uv = torch.from_numpy(f[1]).to(DEV)
    assert 39 * ROW > 2 ** 31
    x_np = TC.hostile_tiles(2, T, seed=32)
    want = XC.tile_sse(x_np, H, W, T, O, fmt, "bt709", "limited", siting, f)
    g = cr.grid_of(H, W, T, O)
    for off, wide in [((1 << 20) // 4, True), ((4 << 20) // 4 + 1, False)]:          # apart from each other and from y
        xv = torch.as_strided(buf.view(torch.float32), (2, 3, T, T), (BIG // 4, T * T, T, 1), off)
        xv.copy_(torch.from_numpy(x_np))
        assert cr.plan(xv, (y, uv), fmt) is wide
        assert cr.frame_tile_distortion(xv, g, (y[0], uv[0]), fmt, siting=siting).tolist() == want, wide
        assert cr.frame_tile_distortion(xv[1:], g, (y[0], uv[0]), fmt, siting=siting, first_tile=1).tolist() == want[1:]


# -- 7. through the codec ------------------------------------------------------------------------------------------------------------

QUALITIES = [0, 0.5, 10]
H0, W0 = 100, 150                                                          # 2 x 3 tiles of 64 x 64, with and without overlap
HEAD = 15 + 33                                                             # the PCK1 and the PCT2 header


@pytest.mark.parametrize("fmt,siting", [("p210", "left"), ("nv12", "topleft"), ("i444", "centre"), ("nv12", "centre")])
@pytest.mark.parametrize("O", [0, 16])
def test_encode_to_size_and_decode(O, fmt, siting):
    from progressivecodec_amd import chroma_tiles, container, frame_rate, tiles
    cr = CR()
    net = gpu_codec()
    f = codec_frame(H0, W0, fmt, siting)
    planes = on_device(f)
    g = cr.grid_of(H0, W0, T, O)
    assert HEAD == chroma_tiles.HEADER_BYTES + tiles.HEADER_BYTES
    enc = lambda target, **kw: cr.encode_frame_tiled_to_size(net, planes, QUALITIES, target, fmt, siting=siting, tile=T, overlap=O,   # noqa: E731
                                                             mask_pol=POL, **kw)
    free_buf, free = enc(10 ** 9)
    rates, dists, pd = free.rates, free.dists, free.plane_dists
    assert len(rates) == len(dists) == len(pd) == 6 and all(len(r) == 3 for r in rates + dists + pd) and free.den == (2 * O if O else 1)
    assert all(len(v) == 3 and dists[t][l] == sum(v) for t in range(6) for l, v in enumerate(pd[t]))         # the default plane weights
    assert free.sse_exact is (O == 0 and siting == "centre")
    lo, hi = HEAD + sum(min(r) for r in rates), HEAD + sum(max(r) for r in rates)
    assert lo < hi
    with pytest.raises(ValueError, match=rf"\b{lo - HEAD}\b"):
        enc(lo - 1)

    @functools.lru_cache(maxsize=None)
    def alone(t, l):
        """tile t cut and coded alone at level l, and the model's own output for it decoded alone"""
        x, _ = chroma_tiles.cut_frame(planes, fmt, siting=siting, tile=T, overlap=O, rect=(t // 3, t % 3, 1, 1))
        datas = net.compress_levels(x, [QUALITIES[l]], mask_pol=POL)
        b = container.pack([datas[0]["strings"]], datas[0]["shape"], [float(QUALITIES[l])], image_size=(T, T), mask_pol=POL)
        strings, shape, qs, _, pol = container.unpack(b, levels=[0])
        return b, net.decompress(strings[0], shape, qs[0], pol)["x_hat"][0]

    for target in (lo, lo + (hi - lo) // 3, lo + 2 * (hi - lo) // 3, hi):
        buf, plan = enc(target)
        assert isinstance(buf, bytes) and len(buf) == plan.container_bytes <= target, target
        assert plan.rates == rates and plan.dists == dists and plan.plane_dists == pd, target     # the tables do not depend on the budget
        assert len(buf) == HEAD + sum(rates[t][l] for t, l in enumerate(plan.levels))
        assert plan.predicted == sum(dists[t][l] for t, l in enumerate(plan.levels))
        assert plan.sse == [sum(pd[t][l][p] for t, l in enumerate(plan.levels)) for p in range(3)]
        assert plan.levels == RC.allocate(rates, dists, target - HEAD)
        hd = chroma_tiles.parse_frame_tiled(buf)
        assert buf[:4] == b"PCK1" and (hd["fmt"], hd["siting"], hd["matrix"], hd["range"], hd["upsample"], hd["H"], hd["W"]) == \
            (fmt, siting, "bt709", "limited", "linear", H0, W0)
        assert hd["inner"][:4] == b"PCT2" and hd["tiled"]["magic"] == b"PCT2" and hd["tiled"]["grid"] == g
        assert hd["tiled"]["contract"] == container.build_contract_id()
        for t, l in enumerate(plan.levels):
            tb, th = tiles.tile_bytes(hd["inner"], hd["tiled"], t)
            assert tb == alone(t, l)[0], (target, t, l)
            assert th["qualities"] == [float(QUALITIES[l])] and th["mask_pol"] == POL and rates[t][l] == 16 + len(tb)
        if target == hi:
            assert all(dists[t][l] == min(dists[t]) for t, l in enumerate(plan.levels))
            assert free.levels == plan.levels and free_buf == buf
        x = torch.stack([alone(t, l)[1] for t, l in enumerate(plan.levels)])
        # what was measured at encode time is what these tiles give
        assert cr.frame_tile_distortion(x, g, planes, fmt, siting=siting).tolist() == [pd[t][l] for t, l in enumerate(plan.levels)]
        x_np = x.cpu().numpy()
        want = KC.stitch(x_np, H0, W0, T, O, fmt, "bt709", "limited", siting)
        got = chroma_tiles.decode_frame_tiled(net, buf)
        assert len(got) == len(want) and all(np.array_equal(a.cpu().numpy(), b[0]) for a, b in zip(got, want)), target
        S = T - O
        region = (0, S, H0, W0 - S)
        part = chroma_tiles.decode_frame_tiled(net, buf, region=region, max_tiles_per_call=1)
        assert all(np.array_equal(a.cpu().numpy(), b[0]) for a, b in zip(part, KC.stitch(x_np, H0, W0, T, O, fmt, "bt709", "limited", siting, window=region)))
        sse = chroma_tiles.stitch_frame(x, g, fmt, siting=siting, ref=planes, image=False).sse[0].tolist()
        if O == 0:                                                         # luma always; chroma where the plan says so
            assert sse[0] == plan.sse[0] and (sse == plan.sse or not plan.sse_exact), target
        if target == lo + (hi - lo) // 3:
            if fmt == "p210":                                              # the 4:2:2 master straight to left-sited NV12
                nv = chroma_tiles.decode_frame_tiled(net, buf, fmt="nv12", siting="left")
                want_nv = KC.stitch(x_np, H0, W0, T, O, "nv12", "bt709", "limited", "left")
                assert nv[0].dtype == torch.uint8 and all(np.array_equal(a.cpu().numpy(), b[0]) for a, b in zip(nv, want_nv))
            for per_call in (1, 4, 32):
                assert enc(target, max_tiles_per_call=per_call) == (buf, plan), per_call
            if (fmt, siting) == ("nv12", "centre"):                        # section 15's plan and inner container, byte for byte
                fb, fp = frame_rate.encode_frame_tiled_to_size(net, planes, QUALITIES, target - chroma_tiles.HEADER_BYTES + 10, fmt, tile=T,
                                                               overlap=O, mask_pol=POL)
                from progressivecodec_amd import frame_tiles
                assert frame_tiles.HEADER_BYTES == 10 and frame_tiles.parse_frame_tiled(fb)["inner"] == hd["inner"]
                assert fp._replace(container_bytes=len(buf)) == plan[:-1]
    with pytest.raises(container.ContainerError, match="level must be -1 or 0"):
        chroma_tiles.decode_frame_tiled(net, free_buf, level=1)

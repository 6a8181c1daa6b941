"""Rate-controlled tiled coding on the GPU (progressivecodec_amd/rate.py, libpc_rate.so) against its restatement
(tests/rate_contract.py): the per-tile distortion sums exactly, on both access paths, and encode_tiled_to_size / decode_tiled through
the codec and the PCT2 container.  T = 64 throughout (one case at 128): the smallest tile, so that the images stay small while every
branch (one tile, several tiles, partial last tiles, bands of every allowed kind) is taken."""
import functools

import numpy as np
import pytest
import torch

from tests import pixels_contract as K
from tests import rate_contract as RC
from tests import tiles_contract as TC
from tests.util import gpu_codec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POL = "point-based-std"
T = 64
SIZES = [(1, 1), (64, 64), (65, 63), (100, 150), (127, 129)]
OVERLAPS = [0, 4, 16, 32]
BAND_OVERLAPS = [24, 28]                                                    # 2 O is no power of two (tests/band_cases.py)
POISON = 0xA5
POISON64 = -0x5A5A5A5A5A5A5A5B


def RT():
    from progressivecodec_amd import rate
    return rate


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def view_args(t, layout):
    """(pointer, layout, plane, row stride) of a 3-D uint8 tensor view"""
    return (t.data_ptr(), 0, 0, t.stride(0)) if layout == "hwc" else (t.data_ptr(), 1, t.stride(0), t.stride(1))


@functools.lru_cache(maxsize=None)
def image(H, W, seed=0):
    """uint8 [3,H,W]; every byte value occurs when there is room"""
    a = np.random.default_rng(1000 * H + W + seed).integers(0, 256, (3, H, W), dtype=np.uint8)
    flat = a.reshape(-1)
    n = min(256, flat.size)
    flat[:n] = np.arange(n, dtype=np.uint8)
    return a


def in_layout(chw, layout):
    return K.from_chw(chw[None], layout)[0]


def up4(v):
    return -(-v // 4) * 4


def u8_tensor(arr, layout, offset=0, loose=False, pad4=False):
    """`arr` (uint8 [H,W,3] or [3,H,W]) as a cuda view whose base is `offset` bytes past an allocation start; loose: a row stride larger
    than the row and no multiple of 4 and a plane stride that is no multiple of the row's; pad4: strides rounded up to multiples of 4"""
    if layout == "hwc":
        H, W, _ = arr.shape
        sr = 3 * W + 5 if loose else up4(3 * W) if pad4 else 3 * W
        sr += 1 if loose and sr % 4 == 0 else 0
        strides, span = (sr, 3, 1), H * sr
    else:
        _, H, W = arr.shape
        sr = W + 3 if loose else up4(W) if pad4 else W
        sr += 1 if loose and sr % 4 == 0 else 0
        sp = H * sr + 1 if loose else H * sr
        strides, span = (sp, sr, 1), 3 * sp
    buf = torch.full((offset + span + 16,), POISON, dtype=torch.uint8, device=DEV)
    v = torch.as_strided(buf, arr.shape, strides, storage_offset=offset)
    v.copy_(torch.from_numpy(np.ascontiguousarray(arr)))
    return v


def float_tiles(x_np, variant, size=T):
    """x_np [n,3,T,T] on the device: contiguous; "loose4": rows, planes and tiles apart inside a NaN-filled buffer, every 16-byte
    alignment kept; "odd": apart and one float past an allocation start, so that no row is 16-byte aligned"""
    t = torch.from_numpy(x_np).to(DEV)
    if variant == "contiguous":
        return t
    n = x_np.shape[0]
    sh, off = (size + 4, 0) if variant == "loose4" else (size + 1, 1)
    sc = size * sh + (8 if variant == "loose4" else 3)
    st = 3 * sc + (4 if variant == "loose4" else 2)
    buf = torch.full((off + n * st + 8,), float("nan"), dtype=torch.float32, device=DEV)
    v = torch.as_strided(buf, x_np.shape, (st, sc, sh, 1), storage_offset=off)
    v.copy_(t)
    return v


def sse_raw(L, x, H, W, O, first, rounding, ref, ref_layout, size=T, nbytes=None):
    """pc_rate_tile_sse_u8 on the tiles x holds -> (status, the [n + 2, 3] buffer whose rows 1 .. n are `out`, poisoned beforehand)"""
    n = x.shape[0]
    buf = torch.full((n + 2, 3), POISON64, dtype=torch.int64, device=DEV)
    need = L.pc_rate_workspace_size(size, n)
    ws = torch.full((max(1, need // 8),), POISON64, dtype=torch.int64, device=DEV)
    rc = L.pc_rate_tile_sse_u8(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), H, W, size, O, first, n, rounding, *view_args(ref, ref_layout),
                               ws.data_ptr(), need if nbytes is None else nbytes, buf[1:].data_ptr(), stream())
    return rc, buf


def check_out(buf, want, case):
    h = buf.cpu()
    assert h[0].tolist() == [POISON64] * 3 and h[-1].tolist() == [POISON64] * 3, case       # the guard words keep their bits
    assert h[1:-1].tolist() == want, case


REF_VIEWS = [(0, False, False), (0, False, True), (0, True, False), (1, False, True), (2, False, True), (3, False, True)]


def kernel_matrix(hw, overlaps):
    rate = RT()
    L = rate.lib()
    H, W = hw
    ref_chw = image(H, W, seed=7)
    seen = set()
    for O in overlaps:
        ny, nx = TC.grid(H, W, T, O)
        n = ny * nx
        x_np = TC.hostile_tiles(n, T, seed=H + W + O)
        xs = {v: float_tiles(x_np, v) for v in ("contiguous", "loose4", "odd")}
        refs = {(lay, rv): u8_tensor(in_layout(ref_chw, lay), lay, *rv) for lay in ("hwc", "chw") for rv in REF_VIEWS}
        ranges = [(0, n)] + ([(1, n - 1), (n // 2, 1)] if n > 1 else []) + ([(1, n - 2)] if n > 2 else [])
        for rounding in ("nearest", "trunc"):
            want = RC.tile_sse(x_np, H, W, T, O, rounding, ref_chw, "chw")
            for (lay, rv), ref in refs.items():
                offset, loose, pad4 = rv
                for variant, x in xs.items():
                    # by construction: the floats are wide unless "odd"; the bytes are wide at an allocation start with strides that
                    # are multiples of 4, which a contiguous image has when 4 | W
                    expect = variant != "odd" and offset == 0 and not loose and (pad4 or W % 4 == 0)
                    for first, m in ranges if (variant == "contiguous" or rv == REF_VIEWS[1]) else ranges[:1]:
                        part = x[first:first + m]
                        wide = rate.plan(part, ref, lay)
                        assert wide is expect, (lay, rv, variant, first)
                        seen.add(wide)
                        rc, buf = sse_raw(L, part, H, W, O, first, rate.ROUNDINGS[rounding], ref, lay)
                        case = (H, W, O, rounding, lay, rv, variant, first, m, wide)
                        assert rc == 0, case
                        check_out(buf, want[first:first + m], case)
            if rounding == "nearest":
                # every tile alone; the Python call, also on a second stream and on views it has to copy
                for t in range(n):
                    rc, buf = sse_raw(L, xs["odd"][t:t + 1], H, W, O, t, 0, refs[("chw", REF_VIEWS[2])], "chw")
                    assert rc == 0
                    check_out(buf, want[t:t + 1], (H, W, O, t))
                g = rate.grid_of(H, W, T, O)
                rt = torch.from_numpy(np.array(ref_chw)).to(DEV)
                got = rate.tile_distortion(xs["loose4"], g, rt, ref_layout="chw")
                assert got.dtype == torch.int64 and got.shape == (n, 3) and got.tolist() == want
                # channel stride H*W, not 1: copied; for one row, whatever row stride the copy reports
                assert rate.tile_distortion(xs["contiguous"], g, rt.permute(1, 2, 0), ref_layout="hwc").tolist() == want
                side = torch.cuda.Stream(DEV)
                side.wait_stream(torch.cuda.current_stream(DEV))
                with torch.cuda.stream(side):
                    got_s = rate.tile_distortion(xs["contiguous"][n - 1:], g, refs[("hwc", REF_VIEWS[0])], first_tile=n - 1)
                side.synchronize()
                assert got_s.tolist() == want[n - 1:]
            else:
                assert rate.tile_distortion(xs["odd"], rate.grid_of(H, W, T, O), refs[("hwc", REF_VIEWS[3])], rounding="trunc").tolist() == want
    assert seen == {True, False}


@pytest.mark.parametrize("hw", SIZES)
def test_kernel_matrix_exact_on_both_paths(hw):
    kernel_matrix(hw, OVERLAPS)


def test_kernel_matrix_at_overlaps_whose_band_quotients_are_no_floats():
    """O = 24 (S = 40, den = 48: the wide path where there is one) and O = 28 (S = 36, den = 56: narrow at 4:2:0) on one picture.  The
    sums weigh with the integer numerators 2u + 1, which are exact whatever 2 O is; what is new is the band geometry."""
    kernel_matrix((100, 150), BAND_OVERLAPS)


def test_the_largest_weights_meet_the_largest_error():
    rate = RT()
    L = rate.lib()
    H, W, size, O = 200, 250, 128, 64                                  # S = 64: 3 x 3 tiles, every interior pixel in a band
    assert TC.grid(H, W, size, O) == (3, 3)
    x_np = np.zeros((9, 3, size, size), np.float32)
    ref_chw = np.full((3, H, W), 255, np.uint8)
    want = RC.tile_sse(x_np, H, W, size, O, "nearest", ref_chw, "chw")
    den = RC.den_of(O)
    assert [sum(w[c] for w in want) for c in range(3)] == [65025 * den * den * H * W] * 3     # the weights partition den^2 per pixel
    assert want[4][0] == 65025 * int(RC.weights_int(1, 3, size, O).sum()) ** 2
    for variant, lay in [("contiguous", "chw"), ("odd", "hwc"), ("loose4", "hwc")]:
        x = float_tiles(x_np, variant, size)
        ref = u8_tensor(in_layout(ref_chw, lay), lay, pad4=True)
        rc, buf = sse_raw(L, x, H, W, O, 0, 0, ref, lay, size)
        assert rc == 0
        check_out(buf, want, (variant, lay))
        rc, buf = sse_raw(L, x[3:8], H, W, O, 3, 1, ref, lay, size)
        assert rc == 0
        check_out(buf, want[3:8], (variant, lay))


@pytest.mark.parametrize("hw", SIZES)
def test_without_overlap_the_tiles_sums_add_up_to_the_stitchs(hw):
    from progressivecodec_amd import tiles
    rate = RT()
    H, W = hw
    g = tiles.grid_of(H, W, T, 0)
    x = torch.from_numpy(TC.hostile_tiles(g.n, T, seed=H * W)).to(DEV)
    ref = u8_tensor(in_layout(np.array(image(H, W, seed=3)), "hwc"), "hwc")      # explicit strides: a 1 x 1 array's own may be anything
    for rounding in ("nearest", "trunc"):
        per_tile = rate.tile_distortion(x, g, ref, rounding=rounding)
        whole = tiles.stitch(x, g, rounding=rounding, ref=ref, image=False)
        assert per_tile.sum(0).tolist() == whole.sse_u8[0].tolist(), rounding


def test_refused_calls_launch_nothing():
    rate = RT()
    L = rate.lib()
    H, W, O = 100, 150, 16
    ref = u8_tensor(np.array(image(H, W)), "chw")
    x = torch.rand(6, 3, T, T, device=DEV)
    for kw in [dict(first=1), dict(first=-1), dict(O=6), dict(size=4096), dict(nbytes=L.pc_rate_workspace_size(T, 6) - 1), dict(rounding=2)]:
        a = dict(dict(H=H, W=W, O=O, first=0, rounding=0, ref=ref, ref_layout="chw"), **kw)
        rc, buf = sse_raw(L, x, **a)
        torch.cuda.synchronize()
        assert rc == -1 and (buf == POISON64).all(), kw
    with pytest.raises(rate.RateError, match="PC_ERR_ARG"):
        raise rate.RateError(-1, "pc_rate_tile_sse_u8")
    rc, buf = sse_raw(L, x, H, W, O, 0, 0, ref, "chw")                  # the same call, unspoilt, goes through
    assert rc == 0 and (buf[1:-1] != POISON64).all() and (buf[0] == POISON64).all()


def test_offsets_past_2_to_the_31():
    """two tiles and the planes of a small image at strides past 2^31 bytes, inside one untouched allocation: every offset is 64-bit"""
    rate = RT()
    L = rate.lib()
    BIG = 2 ** 31 + 4096                                                   # plane / tile stride in bytes
    need = 2 * BIG + (16 << 20)
    free = torch.cuda.mem_get_info(DEV)[0]
    if free < need + (1 << 30):
        pytest.skip(f"{free >> 20} MiB of device memory free, the strided views need {need >> 20} MiB")
    buf = torch.empty(need, dtype=torch.uint8, device=DEV)
    H, W, O = 40, 100, 0                                                   # 1 x 2 tiles
    chw = image(H, W, seed=31)
    ref = torch.as_strided(buf, (3, H, W), (BIG, W, 1), 0)
    ref.copy_(torch.from_numpy(chw))
    x_np = TC.hostile_tiles(2, T, seed=32)
    xv = torch.as_strided(buf.view(torch.float32), (2, 3, T, T), (BIG // 4, T * T, T, 1), (1 << 20) // 4)
    xv.copy_(torch.from_numpy(x_np))
    want = RC.tile_sse(x_np, H, W, T, O, "nearest", chw, "chw")
    assert rate.plan(xv, ref, "chw")
    rc, out = sse_raw(L, xv, H, W, O, 0, 0, ref, "chw")
    assert rc == 0
    check_out(out, want, "wide")
    odd = torch.as_strided(buf.view(torch.float32), (2, 3, T, T), (BIG // 4, T * T, T, 1), (4 << 20) // 4 + 1)      # apart from xv
    odd.copy_(torch.from_numpy(x_np))
    assert not rate.plan(odd, ref, "chw")
    rc, out = sse_raw(L, odd, H, W, O, 0, 0, ref, "chw")
    assert rc == 0
    check_out(out, want, "narrow")
    assert rate.tile_distortion(xv[1:], rate.grid_of(H, W, T, O), ref, first_tile=1, ref_layout="chw").tolist() == want[1:]


# -- through the codec ---------------------------------------------------------------------------------------------------------------

QUALITIES = [0, 0.5, 10]
H0, W0 = 100, 150                                                          # 2 x 3 tiles of 64 x 64, with and without overlap


def codec_image():
    return torch.from_numpy(in_layout(np.array(image(H0, W0, seed=21)), "hwc")).to(DEV)             # [100,150,3]


def crop(img, i, j, S):
    """the zero-extended 64 x 64 crop of tile (i, j)"""
    out = torch.zeros((T, T, 3), dtype=torch.uint8, device=DEV)
    part = img[i * S:i * S + T, j * S:j * S + T]
    out[:part.shape[0], :part.shape[1]] = part
    return out


@pytest.mark.parametrize("O", [0, 16])
def test_encode_to_size_and_decode(O):
    from progressivecodec_amd import container, pixels, tiles
    rate = RT()
    net = gpu_codec()
    img = codec_image()
    g = tiles.grid_of(H0, W0, T, O)
    enc = lambda target, **kw: rate.encode_tiled_to_size(net, img, QUALITIES, target, tile=T, overlap=O, mask_pol=POL, **kw)
    free_buf, free = enc(10 ** 9)
    rates, dists = free.rates, free.dists
    assert len(rates) == len(dists) == 6 and all(len(r) == 3 for r in rates + dists) and free.den == (2 * O if O else 1)
    lo, hi = 33 + sum(min(r) for r in rates), 33 + sum(max(r) for r in rates)
    assert lo < hi
    with pytest.raises(ValueError, match=rf"\b{lo - 33}\b"):
        enc(lo - 1)

    @functools.lru_cache(maxsize=None)
    def alone(t, l):
        """tile t coded alone at level l, and the model's own output for it decoded alone"""
        b = pixels.encode_image(net, crop(img, t // 3, t % 3, T - O), [QUALITIES[l]], mask_pol=POL)
        strings, shape, qs, _, pol = container.unpack(b, levels=[0])
        return b, net.decompress(strings[0], shape, qs[0], pol)["x_hat"][0]

    for target in (lo, lo + (hi - lo) // 3, lo + 2 * (hi - lo) // 3, hi):
        buf, plan = enc(target)
        assert isinstance(buf, bytes) and len(buf) == plan.container_bytes <= target, target
        assert plan.rates == rates and plan.dists == dists, target                   # the tables do not depend on the budget
        assert len(buf) == 33 + sum(rates[t][l] for t, l in enumerate(plan.levels))
        assert plan.predicted == sum(dists[t][l] for t, l in enumerate(plan.levels))
        assert plan.levels == RC.allocate(rates, dists, target - 33)
        hd = tiles.parse_tiled(buf)
        assert hd["magic"] == b"PCT2" and hd["grid"] == g and hd["contract"] == container.build_contract_id()
        for t, l in enumerate(plan.levels):
            tb, th = tiles.tile_bytes(buf, hd, t)
            assert tb == alone(t, l)[0], (target, t, l)
            assert th["qualities"] == [float(QUALITIES[l])] and th["mask_pol"] == POL and rates[t][l] == 16 + len(tb)
        for l in range(3):
            if 33 + sum(r[l] for r in rates) <= target:
                assert plan.predicted <= sum(d[l] for d in dists), (target, l)
        if target == hi:
            assert all(dists[t][l] == min(dists[t]) for t, l in enumerate(plan.levels))
            assert free.levels == plan.levels and free_buf == buf
        x = torch.stack([alone(t, l)[1] for t, l in enumerate(plan.levels)])
        # what was measured at encode time is what these tiles give
        assert rate.tile_distortion(x, g, img).sum(1).tolist() == [dists[t][l] for t, l in enumerate(plan.levels)]
        want = TC.stitch(x.cpu().numpy(), H0, W0, T, O, "nearest", "hwc")
        got = tiles.decode_tiled(net, buf)
        assert np.array_equal(got.cpu().numpy(), want), target
        assert torch.equal(tiles.decode_tiled(net, buf, level=0, max_tiles_per_call=4), got)
        assert torch.equal(tiles.decode_tiled(net, buf, region=(40, 90, 30, 30), max_tiles_per_call=1), got[40:70, 90:120])
        assert torch.equal(tiles.decode_tiled(net, buf, region=(5, 6, 20, 30), layout="chw"), got[5:25, 6:36].permute(2, 0, 1))
        if O == 0:
            assert int(tiles.stitch(x, g, ref=img, image=False).sse_u8.sum()) == plan.predicted, target
        if target == lo + (hi - lo) // 3:
            for per_call in (1, 4):
                assert enc(target, max_tiles_per_call=per_call) == (buf, plan), per_call
            # importance is passed on, nested or flat
            heavy = enc(target, importance=[[1, 1, 1], [1, 10 ** 6, 1]])[1]
            assert heavy.levels == RC.allocate(rates, dists, target - 33, [1, 1, 1, 1, 10 ** 6, 1])
            assert enc(target, importance=[1, 1, 1, 1, 10 ** 6, 1])[1] == heavy
    with pytest.raises(container.ContainerError, match="level must be -1 or 0"):
        tiles.decode_tiled(net, free_buf, level=1)

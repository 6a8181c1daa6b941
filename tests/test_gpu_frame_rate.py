"""Rate-controlled tiled coding of YUV 4:2:0 frames on the GPU (progressivecodec_amd/frame_rate.py, libpc_frame_rate.so) against its
restatement (tests/frame_rate_contract.py): the per-tile, per-plane distortion sums exactly, on both access paths, and
encode_frame_tiled_to_size / decode_frame_tiled through the codec and a PCT2 container inside PCG1.  Every comparison is exact
equality of integers or bytes.  T = 64 throughout (one case at 128): the smallest tile, so that the frames stay small while every
branch (one tile, several tiles, partial last tiles with odd edges, bands of every allowed kind) is taken."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import frame_rate_contract as QC
from tests import frame_tiles_contract as GC
from tests import frames_contract as FC
from tests import rate_contract as RC
from tests import tiles_contract as TC
from tests.test_gpu_frames import View
from tests.test_gpu_rate import POISON64, check_out, float_tiles
from tests.util import gpu_codec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POL = "point-based-std"
T = 64
SIZES = [(1, 1), (2, 2), (64, 64), (65, 63), (100, 150), (127, 129)]
OVERLAPS = [0, 4, 16, 32]
BAND_OVERLAPS = [24, 28]                                                    # 2 O is no power of two (tests/band_cases.py)
MATS = list(FC.MATRICES)
#: the reference planes: aligned with strides that are multiples of 4; pitched with a stride that is none; offset by one element
REF_VIEWS = [("pad4", 0), ("loose", 0), ("pad4", 1)]


def FQ():
    from progressivecodec_amd import frame_rate
    return frame_rate


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def ref_views(fmt, H, W, mode, offset, data):
    """the planes of the original frame as Views `offset` elements past an allocation start"""
    Hc, Wc = FC.chroma_size(H, W)
    dt = np.uint16 if fmt == "p010" else np.uint8
    shapes = [(1, H, W), (1, Hc, Wc), (1, Hc, Wc)] if fmt == "i420" else [(1, H, W), (1, Hc, Wc, 2)]
    return [View(s, dt, offset, mode, data[i]) for i, s in enumerate(shapes)]


def struct_of(tensors):
    from progressivecodec_amd import frames
    return frames._frame_struct(list(tensors))


def sse_raw(x, H, W, O, first, fmt, rng, matrix, ref, size=T, nbytes=None, strides=None):
    """pc_frame_rate_tile_sse on the tiles x holds -> (status, the [n + 2, 3] buffer whose rows 1 .. n are `out`, poisoned beforehand,
    whether every partial of the workspace and no word after it was written -- or, for a refused call, none at all).  fmt and rng:
    names, or raw ids for the calls that are to be refused."""
    from progressivecodec_amd import frames
    L = FQ().lib()
    n = x.shape[0]
    buf = torch.full((n + 2, 3), POISON64, dtype=torch.int64, device=DEV)
    need = L.pc_frame_rate_workspace_size(size, n)
    ws = torch.full((need // 8 + 1,), POISON64, dtype=torch.int64, device=DEV)
    k = frames.coefficients(matrix)
    rs = struct_of(ref)
    st = strides if strides is not None else (x.stride(0), x.stride(1), x.stride(2))
    rc = L.pc_frame_rate_tile_sse(x.data_ptr(), *st, H, W, size, O, first, n, frames.FORMATS.get(fmt, fmt), frames.RANGES.get(rng, rng),
                                  k.kr, k.kg, k.kb, k.ib, k.ir, C.byref(rs), ws.data_ptr(), need if nbytes is None else nbytes,
                                  buf[1:].data_ptr(), stream())
    h = ws.cpu()
    return rc, buf, bool(h[-1] == POISON64 and ((h[:-1] != POISON64).all() if rc == 0 else (h == POISON64).all()))


def kernel_matrix(hw, overlaps):
    """every overlap x format x range against the restatement; tiles contiguous and one float past an allocation start; reference
    planes aligned, pitched and offset by one element; sub-ranges and every tile alone; the Python call, on a side stream and on views
    it has to copy.  Wide exactly where pc_frame_rate_plan's preconditions hold."""
    fq = FQ()
    H, W = hw
    seen = set()
    for O in overlaps:
        ny, nx = TC.grid(H, W, T, O)
        n = ny * nx
        x_np = TC.hostile_tiles(n, T, seed=H + W + O)
        xs = {v: float_tiles(x_np, v) for v in ("contiguous", "odd")}
        ranges = [(0, n)] + ([(1, n - 1), (n // 2, 1)] if n > 1 else [])
        g = fq.grid_of(H, W, T, O)
        for k, fmt in enumerate(FC.FORMATS):
            f = FC.random_frame(1, H, W, fmt, seed=1000 * H + W + O + k)
            refs = {rv: ref_views(fmt, H, W, *rv, f) for rv in REF_VIEWS}
            planes = tuple(torch.from_numpy(p[0]).to(DEV) for p in f)
            for rng in FC.RANGES:
                matrix = MATS[(k + O // 4 + (rng == "full")) % 3]
                want = QC.tile_sse(x_np, H, W, T, O, fmt, matrix, rng, f)
                for rv, views in refs.items():
                    rt = [v.t for v in views]
                    for variant, x in xs.items():
                        # by construction: the floats are wide unless "odd"; the planes at an allocation start with strides that are
                        # multiples of 4; and a tile's first column is a multiple of 8 in the frame where O is one
                        expect = variant == "contiguous" and rv == REF_VIEWS[0] and O % 8 == 0
                        for first, m in ranges if (variant, rv) in (("contiguous", REF_VIEWS[0]), ("odd", REF_VIEWS[1])) else ranges[:1]:
                            part = x[first:first + m]
                            wide = fq.plan(part, rt, fmt, overlap=O)
                            case = (H, W, O, fmt, rng, rv, variant, first, m, wide)
                            assert wide is expect, case
                            seen.add(wide)
                            rc, buf, ws_ok = sse_raw(part, H, W, O, first, fmt, rng, matrix, rt)
                            assert rc == 0 and ws_ok, case
                            check_out(buf, want[first:first + m], case)
                if rng == "limited":
                    for t in range(n):                                     # every tile alone, on either path
                        for variant, rv in (("contiguous", REF_VIEWS[0]), ("odd", REF_VIEWS[2])):
                            rc, buf, ws_ok = sse_raw(xs[variant][t:t + 1], H, W, O, t, fmt, rng, matrix, [v.t for v in refs[rv]])
                            assert rc == 0 and ws_ok
                            check_out(buf, want[t:t + 1], (H, W, O, fmt, t, variant))
                else:
                    # the Python call: a pitched reference; channels last in memory (copied); a plane whose innermost stride is not
                    # 1 (copied); a sub-range on a second stream
                    got = fq.frame_tile_distortion(xs["odd"], g, tuple(v.t for v in refs[REF_VIEWS[1]]), fmt, matrix, rng)
                    assert got.dtype == torch.int64 and got.shape == (n, 3) and got.device.type == "cuda" and got.tolist() == want
                    cl = xs["contiguous"].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
                    wider = torch.from_numpy(np.repeat(f[0][0], 2, axis=1)).to(DEV)[:, ::2]
                    assert not wider.is_contiguous() or W == 1
                    assert fq.frame_tile_distortion(cl, g, (wider,) + planes[1:], fmt, matrix, rng).tolist() == want
                    side = torch.cuda.Stream(DEV)
                    side.wait_stream(torch.cuda.current_stream(DEV))
                    with torch.cuda.stream(side):
                        got_s = fq.frame_tile_distortion(xs["contiguous"][n - 1:], g, planes, fmt, matrix, rng, first_tile=n - 1)
                    side.synchronize()
                    assert got_s.tolist() == want[n - 1:]
    assert seen == {True, False}


@pytest.mark.parametrize("hw", SIZES)
def test_kernel_matrix_exact_on_both_paths(hw):
    kernel_matrix(hw, OVERLAPS)


def test_kernel_matrix_at_overlaps_whose_band_quotients_are_no_floats():
    """O = 24 (S = 40, den = 48: the wide path where there is one) and O = 28 (S = 36, den = 56: narrow at 4:2:0) on one picture.  The
    sums weigh with the integer numerators 2u + 1, which are exact whatever 2 O is; what is new is the band geometry."""
    kernel_matrix((100, 150), BAND_OVERLAPS)


def saturated(H, W, fmt):
    yo, ys, co, cs, mx = FC.levels(fmt, "full")
    Hc, Wc = FC.chroma_size(H, W)
    return FC.frame(np.full((1, H, W), mx, np.int64), np.zeros((1, Hc, Wc), np.int64), np.zeros((1, Hc, Wc), np.int64), fmt), mx - yo, co


@pytest.mark.parametrize("fmt", ["nv12", "p010"])
def test_the_largest_weights_meet_the_largest_error(fmt):
    H, W, size, O = 200, 250, 128, 64                                  # S = 64: 3 x 3 tiles, every interior pixel in a band
    assert TC.grid(H, W, size, O) == (3, 3)
    x_np = np.zeros((9, 3, size, size), np.float32)
    f, eY, eC = saturated(H, W, fmt)
    want = QC.tile_sse(x_np, H, W, size, O, fmt, "bt709", "full", f)
    den = RC.den_of(O)
    Hc, Wc = FC.chroma_size(H, W)
    assert sum(w[0] for w in want) == eY * eY * den * den * H * W                                  # the weights partition den^2 per sample
    assert sum(w[1] for w in want) == sum(w[2] for w in want) == eC * eC * den * den * Hc * Wc
    assert want[4][0] == eY * eY * int(RC.weights_int(1, 3, size, O).sum()) ** 2
    assert want[4][1] == eC * eC * sum(QC.chroma_weights(1, 3, size, O)) ** 2
    for variant, rv in [("contiguous", REF_VIEWS[0]), ("odd", REF_VIEWS[0]), ("contiguous", REF_VIEWS[1])]:
        x = float_tiles(x_np, variant, size)
        rt = [v.t for v in ref_views(fmt, H, W, *rv, f)]
        assert FQ().plan(x, rt, fmt, overlap=O) is (variant == "contiguous" and rv == REF_VIEWS[0])
        rc, buf, ws_ok = sse_raw(x, H, W, O, 0, fmt, "full", "bt709", rt, size)
        assert rc == 0 and ws_ok
        check_out(buf, want, (variant, rv))
        rc, buf, ws_ok = sse_raw(x[3:8], H, W, O, 3, fmt, "full", "bt709", rt, size)
        assert rc == 0 and ws_ok
        check_out(buf, want[3:8], (variant, rv))


@pytest.mark.parametrize("hw", SIZES)
def test_without_overlap_the_tiles_sums_add_up_to_the_stitchs(hw):
    from progressivecodec_amd import frame_tiles
    fq = FQ()
    H, W = hw
    g = fq.grid_of(H, W, T, 0)
    x = torch.from_numpy(TC.hostile_tiles(g.n, T, seed=H * W)).to(DEV)
    for k, fmt in enumerate(FC.FORMATS):
        planes = tuple(torch.from_numpy(p[0]).to(DEV) for p in FC.random_frame(1, H, W, fmt, seed=3 + k))
        for rng in FC.RANGES:
            per_tile = fq.frame_tile_distortion(x, g, planes, fmt, MATS[k], rng)
            whole = frame_tiles.stitch_frame(x, g, fmt, MATS[k], rng, ref=planes, image=False)
            assert per_tile.sum(0).tolist() == whole.sse[0].tolist(), (fmt, rng)


def test_refused_calls_launch_nothing():
    fq = FQ()
    L = fq.lib()
    H, W, O = 100, 150, 16
    x = torch.rand(6, 3, T, T, device=DEV)
    for fmt in ("nv12", "p010"):
        rt = [v.t for v in ref_views(fmt, H, W, "pad4", 0, FC.random_frame(1, H, W, fmt, seed=1))]
        big = lambda size: dict(size=size, O=0, n=1, strides=(3 * size * size, size * size, size))                 # noqa: E731
        bads = [dict(first=1), dict(first=-1), dict(O=6), big(4096), dict(nbytes=L.pc_frame_rate_workspace_size(T, 6) - 1), dict(fmt=3),
                dict(fmt=-1), dict(rng=2), dict(rng=-1)] + ([big(2048)] if fmt == "p010" else [])
        for kw in bads:
            a = dict(dict(H=H, W=W, O=O, first=0, fmt=fmt, rng="limited", matrix="bt709", ref=rt), **kw)
            rc, buf, ws_ok = sse_raw(x[:a.pop("n", 6)], **a)
            torch.cuda.synchronize()
            assert rc == -1 and (buf == POISON64).all() and ws_ok, (fmt, kw)
        rc, buf, ws_ok = sse_raw(x, H, W, O, 0, fmt, "limited", "bt709", rt)                                       # unspoilt, it goes through
        assert rc == 0 and ws_ok and (buf[1:-1] != POISON64).all() and (buf[0] == POISON64).all() and (buf[-1] == POISON64).all()
    with pytest.raises(fq.FrameRateError, match="PC_ERR_ARG"):
        raise fq.FrameRateError(-1, "pc_frame_rate_tile_sse")


def test_offsets_past_2_to_the_31():
    """two tiles at a tile stride past 2^31 bytes and a luma plane whose last rows lie past 2^31 bytes, inside one untouched
    allocation: every offset is 64-bit"""
    fq = FQ()
    BIG = 2 ** 31 + 4096                                                   # tile stride in bytes
    ROW = 2 ** 26 + 64                                                     # luma row stride in bytes: row 32 starts past 2^31
    need = 2 * BIG + (16 << 20)
    free = torch.cuda.mem_get_info(DEV)[0]
    if free < need + (1 << 30):
        pytest.skip(f"{free >> 20} MiB of device memory free, the strided views need {need >> 20} MiB")
    buf = torch.empty(need, dtype=torch.uint8, device=DEV)
    H, W, O = 40, 100, 0                                                   # 1 x 2 tiles
    f = FC.random_frame(1, H, W, "nv12", seed=31)
    y = torch.as_strided(buf, (1, H, W), (H * ROW, ROW, 1), 8 << 20)
    y.copy_(torch.from_numpy(f[0]))
    uv = torch.from_numpy(f[1]).to(DEV)
    assert 39 * ROW > 2 ** 31
    x_np = TC.hostile_tiles(2, T, seed=32)
    xv = torch.as_strided(buf.view(torch.float32), (2, 3, T, T), (BIG // 4, T * T, T, 1), (1 << 20) // 4)
    xv.copy_(torch.from_numpy(x_np))
    want = QC.tile_sse(x_np, H, W, T, O, "nv12", "bt709", "limited", f)
    assert fq.plan(xv, (y, uv), "nv12")
    rc, out, ws_ok = sse_raw(xv, H, W, O, 0, "nv12", "limited", "bt709", (y, uv))
    assert rc == 0 and ws_ok
    check_out(out, want, "wide")
    odd = torch.as_strided(buf.view(torch.float32), (2, 3, T, T), (BIG // 4, T * T, T, 1), (4 << 20) // 4 + 1)      # apart from xv and y
    odd.copy_(torch.from_numpy(x_np))
    assert not fq.plan(odd, (y, uv), "nv12")
    rc, out, ws_ok = sse_raw(odd, H, W, O, 0, "nv12", "limited", "bt709", (y, uv))
    assert rc == 0 and ws_ok
    check_out(out, want, "narrow")
    assert fq.frame_tile_distortion(xv[1:], fq.grid_of(H, W, T, O), (y, uv), "nv12", first_tile=1).tolist() == want[1:]


# -- through the codec ---------------------------------------------------------------------------------------------------------------

QUALITIES = [0, 0.5, 10]
H0, W0 = 100, 150                                                          # 2 x 3 tiles of 64 x 64, with and without overlap
HEAD = 10 + 33                                                             # the PCG1 and the PCT2 header


@functools.lru_cache(maxsize=None)
def codec_frame(fmt):
    """a smooth frame (the codec's synthetic weights are not meant for noise; any frame does)"""
    g = np.random.default_rng(H0 + W0)
    lo = torch.from_numpy(g.uniform(0.1, 0.9, (1, 3, 8, 8)).astype(np.float32))
    x = torch.nn.functional.interpolate(lo, size=(H0, W0), mode="bilinear", align_corners=False).numpy()
    return FC.emit(x, 0, 0, H0, W0, fmt, "bt709", "limited")


@pytest.mark.parametrize("fmt", ["nv12", "p010"])
@pytest.mark.parametrize("O", [0, 16])
def test_encode_to_size_and_decode(O, fmt):
    from progressivecodec_amd import container, frame_tiles, tiles
    fq = FQ()
    net = gpu_codec()
    f = codec_frame(fmt)
    planes = tuple(torch.from_numpy(p[0]).to(DEV) for p in f)
    g = fq.grid_of(H0, W0, T, O)
    enc = lambda target, **kw: fq.encode_frame_tiled_to_size(net, planes, QUALITIES, target, fmt, tile=T, overlap=O, mask_pol=POL, **kw)   # noqa: E731
    free_buf, free = enc(10 ** 9)
    rates, dists, pd = free.rates, free.dists, free.plane_dists
    assert len(rates) == len(dists) == len(pd) == 6 and all(len(r) == 3 for r in rates + dists + pd) and free.den == (2 * O if O else 1)
    assert all(len(v) == 3 and dists[t][l] == sum(v) for t in range(6) for l, v in enumerate(pd[t]))         # the default plane weights
    lo, hi = HEAD + sum(min(r) for r in rates), HEAD + sum(max(r) for r in rates)
    assert lo < hi
    with pytest.raises(ValueError, match=rf"\b{lo - HEAD}\b"):
        enc(lo - 1)

    @functools.lru_cache(maxsize=None)
    def alone(t, l):
        """tile t cut and coded alone at level l, and the model's own output for it decoded alone"""
        x, _ = frame_tiles.cut_frame(planes, fmt, tile=T, overlap=O, rect=(t // 3, t % 3, 1, 1))
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
        hd = frame_tiles.parse_frame_tiled(buf)
        assert (hd["fmt"], hd["matrix"], hd["range"], hd["upsample"], hd["H"], hd["W"]) == (fmt, "bt709", "limited", "linear", H0, W0)
        assert hd["tiled"]["magic"] == b"PCT2" and hd["tiled"]["grid"] == g and hd["tiled"]["contract"] == container.build_contract_id()
        for t, l in enumerate(plan.levels):
            tb, th = tiles.tile_bytes(hd["inner"], hd["tiled"], t)
            assert tb == alone(t, l)[0], (target, t, l)
            assert th["qualities"] == [float(QUALITIES[l])] and th["mask_pol"] == POL and rates[t][l] == 16 + len(tb)
        if target == hi:
            assert all(dists[t][l] == min(dists[t]) for t, l in enumerate(plan.levels))
            assert free.levels == plan.levels and free_buf == buf
        x = torch.stack([alone(t, l)[1] for t, l in enumerate(plan.levels)])
        # what was measured at encode time is what these tiles give
        assert fq.frame_tile_distortion(x, g, planes, fmt).tolist() == [pd[t][l] for t, l in enumerate(plan.levels)]
        want = GC.stitch(x.cpu().numpy(), H0, W0, T, O, fmt, "bt709", "limited")
        got = frame_tiles.decode_frame_tiled(net, buf)
        assert len(got) == len(want) == 2 and all(np.array_equal(a.cpu().numpy(), b[0]) for a, b in zip(got, want)), target
        assert all(torch.equal(a, b) for a, b in zip(frame_tiles.decode_frame_tiled(net, buf, level=0, max_tiles_per_call=4), got))
        part = frame_tiles.decode_frame_tiled(net, buf, region=(40, 90, 30, 30), max_tiles_per_call=1)
        assert torch.equal(part[0], got[0][40:70, 90:120]) and torch.equal(part[1], got[1][20:35, 45:60])
        if O == 0:                                                         # the table is the decoded frame's exact per-plane SSE
            assert frame_tiles.stitch_frame(x, g, fmt, ref=planes, image=False).sse[0].tolist() == plan.sse, target
        if target == lo + (hi - lo) // 3:
            for per_call in (1, 4, 32):
                assert enc(target, max_tiles_per_call=per_call) == (buf, plan), per_call
            luma = enc(target, plane_weights=(1, 0, 0))[1]
            assert luma.dists == [[v[0] for v in row] for row in pd] and luma.plane_dists == pd and luma.rates == rates
            assert luma.levels == RC.allocate(rates, luma.dists, target - HEAD)
            # importance is passed on, nested or flat
            heavy = enc(target, importance=[[1, 1, 1], [1, 10 ** 6, 1]])[1]
            assert heavy.levels == RC.allocate(rates, dists, target - HEAD, [1, 1, 1, 1, 10 ** 6, 1])
            assert enc(target, importance=[1, 1, 1, 1, 10 ** 6, 1])[1] == heavy
    with pytest.raises(container.ContainerError, match="level must be -1 or 0"):
        frame_tiles.decode_frame_tiled(net, free_buf, level=1)

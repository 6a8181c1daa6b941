"""The YUV 4:2:0 layer on the GPU (progressivecodec_amd/frames.py, libpc_frames.so) against its restatement (tests/frames_contract.py):
ingest and emit bit for bit for every format, matrix, range and upsampler on both access paths, the sums exactly, and encode_frame /
decode_frame through the codec and the PCF1 container.

Sizes: the smallest that take every branch -- odd dimensions, a single chroma sample, partial last items, both padding parities, left
odd, even and a multiple of 4 and 8.  Every plane is a view `offset` elements into a larger poisoned allocation with its own strides,
so that an element left unwritten, or one written outside the view, shows."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import frames_contract as FC
from tests.util import gpu_codec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POL = "point-based-std"
SIZES = [(1, 1), (2, 2), (3, 5), (64, 64), (65, 63), (100, 150), (127, 129)]
POISON64 = -0x5A5A5A5A5A5A5A5B


def FR():
    from progressivecodec_amd import frames
    return frames


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def geometry(H, W):
    from progressivecodec_amd.pixels import padding
    return padding(H, W)


def up4(v):
    return -(-v // 4) * 4


def poison_of(dtype):
    return 0xA5 if np.dtype(dtype).itemsize == 1 else 0xA5A5


class View:
    """One plane [B, rows, len] or [B, rows, len/2, 2] as a cuda view `offset` elements past an allocation start (allocations are at
    least 256-byte aligned).  mode "pad4": strides rounded up to multiples of 4 (the wide path's, at offset 0); "loose": a row stride
    larger than the row and no multiple of 4, and a batch stride that is no multiple of the row's; "tight": contiguous."""

    def __init__(self, shape, dtype, offset=0, mode="tight", data=None):
        B, rows = shape[:2]
        rowlen = int(np.prod(shape[2:]))
        sr = {"tight": rowlen, "pad4": up4(rowlen), "loose": rowlen + 3 + (1 if (rowlen + 3) % 4 == 0 else 0)}[mode]
        sb = {"tight": rows * sr, "pad4": up4(rows * sr) + 4, "loose": rows * sr + 1}[mode]
        self.shape, self.offset, self.dtype = tuple(shape), offset, np.dtype(dtype)
        self.strides = (sb, sr, 2, 1) if len(shape) == 4 else (sb, sr, 1)
        host = np.full(offset + B * sb + 16, poison_of(dtype), dtype)
        if data is not None:
            self.on(host)[...] = data
        self.buf = torch.from_numpy(host).to(DEV)
        self.t = torch.as_strided(self.buf, self.shape, self.strides, storage_offset=offset)

    def on(self, host):
        return np.lib.stride_tricks.as_strided(host[self.offset:], self.shape, [s * self.dtype.itemsize for s in self.strides])

    def read(self):
        """(the view's elements, whether every element outside the view still holds the poison)"""
        host = self.buf.cpu().numpy().copy()
        got = self.on(host).copy()
        self.on(host)[...] = poison_of(self.dtype)
        return got, bool((host == poison_of(self.dtype)).all())


def frame_views(fmt, B, H, W, offset=0, mode="tight", data=None):
    """the planes of a frame as Views; `data`: a frame of tests/frames_contract.py to hold, else poison (a destination)"""
    Hc, Wc = FC.chroma_size(H, W)
    dt = np.uint16 if fmt == "p010" else np.uint8
    shapes = [(B, H, W), (B, Hc, Wc), (B, Hc, Wc)] if fmt == "i420" else [(B, H, W), (B, Hc, Wc, 2)]
    return [View(s, dt, offset, mode, None if data is None else data[i]) for i, s in enumerate(shapes)]


def struct_of(views):
    return FR()._frame_struct([v.t for v in views])


def float_planes(x_np, variant):
    """x_np [B,3,Hp,Wp] on the device: contiguous; "loose4": rows, planes and pictures apart inside a NaN-filled buffer, every 16-byte
    alignment kept; "odd": apart and one float past an allocation start, so that no row is 16-byte aligned"""
    t = torch.from_numpy(x_np).to(DEV)
    if variant == "contiguous":
        return t
    B, _, Hp, Wp = x_np.shape
    sh, off = (Wp + 4, 0) if variant == "loose4" else (Wp + 1, 1)
    sc = Hp * sh + (8 if variant == "loose4" else 3)
    sb = 3 * sc + (4 if variant == "loose4" else 2)
    buf = torch.full((off + B * sb + 8,), float("nan"), dtype=torch.float32, device=DEV)
    v = torch.as_strided(buf, x_np.shape, (sb, sc, sh, 1), storage_offset=off)
    v.copy_(t)
    return v


def ingest_raw(views, fmt, matrix, rng, up, B, H, W, Hp, Wp, top, left, dst_offset=0):
    """pc_frames_ingest into a NaN-poisoned buffer with guard floats on both sides -> (status, wide as pc_frames_plan reports it,
    the [B,3,Hp,Wp] result, whether the guards kept their bits)"""
    frames = FR()
    L = frames.lib()
    k = frames.coefficients(matrix)
    n = B * 3 * Hp * Wp
    buf = torch.full((4 + dst_offset + n + 4,), float("nan"), dtype=torch.float32, device=DEV)
    dst = buf[4 + dst_offset:4 + dst_offset + n].view(B, 3, Hp, Wp)
    src = struct_of(views)
    wide = C.c_int(-1)
    assert L.pc_frames_plan(frames.INGEST, frames.FORMATS[fmt], C.byref(src), dst.data_ptr(), 3 * Hp * Wp, Hp * Wp, Wp, left, None, C.byref(wide)) == 0
    rc = L.pc_frames_ingest(C.byref(src), frames.FORMATS[fmt], frames.RANGES[rng], frames.UPSAMPLES[up], k.a, k.b, k.c, k.d, B, H, W,
                            dst.data_ptr(), Hp, Wp, top, left, stream())
    h = buf.cpu().numpy()
    guards = bool(np.isnan(h[:4 + dst_offset]).all() and np.isnan(h[4 + dst_offset + n:]).all())
    return rc, wide.value, h[4 + dst_offset:4 + dst_offset + n].reshape(B, 3, Hp, Wp), guards


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def emit_raw(xv, fmt, matrix, rng, H, W, Hp, Wp, top, left, dst_views, ref_views, nbytes=None):
    """pc_frames_emit -> (status, wide, the [B+2,3] sums buffer whose rows 1 .. B are `sse`, poisoned beforehand, the workspace)"""
    frames = FR()
    L = frames.lib()
    k = frames.coefficients(matrix)
    B = xv.shape[0]
    dst = struct_of(dst_views) if dst_views is not None else None
    ref = struct_of(ref_views) if ref_views is not None else None
    need = L.pc_frames_emit_workspace_size(B, H, W)
    ws = torch.full((max(1, need // 8) + 1,), POISON64, dtype=torch.int64, device=DEV)
    sse = torch.full((B + 2, 3), POISON64, dtype=torch.int64, device=DEV)
    wide = C.c_int(-1)
    pd, pr = (C.byref(dst) if dst is not None else None), (C.byref(ref) if ref is not None else None)
    assert L.pc_frames_plan(frames.EMIT, frames.FORMATS[fmt], pd, xv.data_ptr(), xv.stride(0), xv.stride(1), xv.stride(2), left, pr, C.byref(wide)) == 0
    rc = L.pc_frames_emit(xv.data_ptr(), xv.stride(0), xv.stride(1), xv.stride(2), Hp, Wp, top, left, B, H, W, frames.FORMATS[fmt],
                          frames.RANGES[rng], k.kr, k.kg, k.kb, k.ib, k.ir, pd, pr, ws.data_ptr() if ref is not None else None,
                          (need if nbytes is None else nbytes) if ref is not None else 0, sse[1:].data_ptr() if ref is not None else None, stream())
    return rc, wide.value, sse.cpu(), ws.cpu()


def check_sums(sse, ws, want, need):
    assert sse[0].tolist() == [POISON64] * 3 and sse[-1].tolist() == [POISON64] * 3          # the guard words keep their bits
    assert sse[1:-1].tolist() == want
    assert ws[-1].item() == POISON64 and (need == 0 or (ws[:need // 8] != POISON64).all())      # every partial written, none beyond


# -- ingest --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", SIZES)
def test_ingest_is_the_restatement_bit_for_bit(hw):
    """every fmt x matrix x range x upsample at B = 1 and 3.  The B = 3 call takes the standard geometry with loose, offset planes
    (narrow: left is odd or the planes are unaligned); the B = 1 call a left rounded down to a multiple of 8 and aligned planes (wide)."""
    H, W = hw
    g = geometry(H, W)
    seen = set()
    for n, (fmt, matrix, rng, up) in enumerate(itertools.product(FC.FORMATS, FC.MATRICES, FC.RANGES, FC.UPSAMPLES)):
        for B, left, offset, mode, dst_offset in [(3, g.left, 1 + n % 3, "loose", n % 2), (1, g.left // 8 * 8, 0, "pad4", 0)]:
            f = FC.random_frame(B, H, W, fmt, seed=1000 * H + W + n)
            views = frame_views(fmt, B, H, W, offset, mode, f)
            rc, wide, got, guards = ingest_raw(views, fmt, matrix, rng, up, B, H, W, g.Hp, g.Wp, g.top, left, dst_offset)
            case = (hw, fmt, matrix, rng, up, B, left, offset, mode)
            assert rc == 0 and guards, case
            assert wide == (1 if mode == "pad4" else 0), case
            seen.add(wide)
            assert same_bits(got, FC.ingest(f, fmt, matrix, rng, up, g.Hp, g.Wp, g.top, left)), case
    assert seen == {0, 1}


@pytest.mark.parametrize("fmt", FC.FORMATS)
@pytest.mark.parametrize("hw", [(3, 5), (65, 63), (100, 150), (127, 129)])
def test_ingest_paths_agree_on_the_same_data(hw, fmt):
    """one frame under every left in 0 .. 9 and 16 (odd, even, multiples of 4 and 8), both top parities, aligned and unaligned
    planes and destinations: wide exactly where pc_frames_plan's preconditions hold, and the same bits as the restatement everywhere"""
    H, W = hw
    Hp, Wp = -(-(H + 3) // 64) * 64, -(-(W + 16) // 64) * 64
    f = FC.random_frame(2, H, W, fmt, seed=H + W)
    seen = set()
    for left, top, (offset, mode), dst_offset in itertools.product([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 16], [0, 3], [(0, "pad4"), (0, "loose"), (2, "pad4")], [0, 1]):
        if (left + top + offset + dst_offset) % 2 and left not in (0, 8, 16):                   # half of the narrow cases are enough
            continue
        views = frame_views(fmt, 2, H, W, offset, mode, f)
        rc, wide, got, guards = ingest_raw(views, fmt, "bt601", "limited", "linear", 2, H, W, Hp, Wp, top, left, dst_offset)
        case = (hw, fmt, left, top, offset, mode, dst_offset)
        assert rc == 0 and guards, case
        assert wide == int(left % 8 == 0 and offset == 0 and mode == "pad4" and dst_offset == 0), case
        seen.add(wide)
        assert same_bits(got, FC.ingest(f, fmt, "bt601", "limited", "linear", Hp, Wp, top, left)), case
    assert seen == {0, 1}


def test_to_model_input_python_entry():
    frames = FR()
    for fmt, (H, W) in zip(FC.FORMATS, [(100, 150), (65, 63), (64, 64)]):
        f = FC.random_frame(2, H, W, fmt, seed=3)
        g = geometry(H, W)
        want = FC.ingest(f, fmt, "bt2020", "full", "nearest", g.Hp, g.Wp, g.top, g.left)
        planes = tuple(torch.from_numpy(p).to(DEV) for p in f)
        x, geom = frames.to_model_input(planes, fmt, "bt2020", "full", "nearest")
        assert geom == g and same_bits(x.cpu().numpy(), want)
        x1, _ = frames.to_model_input(tuple(p[1] for p in planes), fmt, "bt2020", "full", "nearest")         # one frame, no batch axis
        assert same_bits(x1.cpu().numpy(), want[1:])
        # planes whose innermost stride does not fit are copied, not refused: Y as every second column of a wider tensor
        wider = torch.from_numpy(np.repeat(f[0], 2, axis=2)).to(DEV)
        x2, _ = frames.to_model_input((wider[:, :, ::2],) + planes[1:], fmt, "bt2020", "full", "nearest")
        assert same_bits(x2.cpu().numpy(), want)
        assert frames.plan(frames.INGEST, planes, fmt, x, geom) == (geom.left % 8 == 0 and all(p.stride(1) % 4 == 0 and p.stride(0) % 4 == 0 for p in planes))


# -- emit ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", SIZES)
def test_emit_and_sums_are_the_restatement_exactly(hw):
    """every fmt x matrix x range at B = 1 and 3, x_hat with NaN, +-inf, values outside [0, 1] and -0.0 in it.  B = 3: the standard
    geometry, loose offset planes and float rows (narrow); B = 1: left rounded down to a multiple of 4, aligned planes (wide).  The
    sums also without an image, and the image also without sums."""
    H, W = hw
    g = geometry(H, W)
    L = FR().lib()
    seen = set()
    for n, (fmt, matrix, rng) in enumerate(itertools.product(FC.FORMATS, FC.MATRICES, FC.RANGES)):
        for B, left, offset, mode, variant in [(3, g.left, 1 + n % 3, "loose", ("odd", "contiguous")[n % 2]),
                                               (1, g.left // 4 * 4, 0, "pad4", ("contiguous", "loose4")[n % 2])]:
            ref = FC.random_frame(B, H, W, fmt, seed=77 * H + W + n)
            x = FC.hostile_planes(ref, fmt, matrix, rng, g.Hp, g.Wp, g.top, left, seed=n)
            assert H * W < 4096 or (np.isnan(x[:, :, g.top:g.top + H, left:left + W]).any() and np.isinf(x[:, :, g.top:g.top + H, left:left + W]).any())
            xv = float_planes(x, variant)
            want = FC.emit(x, g.top, left, H, W, fmt, matrix, rng)
            want_sums = FC.sums(x, g.top, left, H, W, fmt, matrix, rng, ref)
            need = L.pc_frames_emit_workspace_size(B, H, W)
            refv = frame_views(fmt, B, H, W, offset, mode, ref)
            case = (hw, fmt, matrix, rng, B, left, offset, mode, variant)
            for with_image, with_ref in [(True, True), (False, True), (True, False)]:
                dstv = frame_views(fmt, B, H, W, offset, mode) if with_image else None
                rc, wide, sse, ws = emit_raw(xv, fmt, matrix, rng, H, W, g.Hp, g.Wp, g.top, left, dstv, refv if with_ref else None)
                assert rc == 0, case
                assert wide == (1 if mode == "pad4" else 0), case
                seen.add(wide)
                if with_ref:
                    check_sums(sse, ws, want_sums, need)
                else:
                    assert (sse == POISON64).all() and (ws == POISON64).all(), case
                if with_image:
                    for v, w in zip(dstv, want):
                        got, clean = v.read()
                        assert clean and np.array_equal(got, w), case
    assert seen == {0, 1}


@pytest.mark.parametrize("fmt", FC.FORMATS)
@pytest.mark.parametrize("hw", [(3, 5), (65, 63), (100, 150)])
def test_emit_paths_agree_on_the_same_data(hw, fmt):
    H, W = hw
    Hp, Wp = -(-(H + 3) // 64) * 64, -(-(W + 8) // 64) * 64
    ref = FC.random_frame(2, H, W, fmt, seed=H * W)
    seen = set()
    for left, top in itertools.product([0, 1, 2, 4, 7, 8], [0, 3]):
        x = FC.hostile_planes(ref, fmt, "bt709", "limited", Hp, Wp, top, left, seed=left)
        want = FC.emit(x, top, left, H, W, fmt, "bt709", "limited")
        want_sums = FC.sums(x, top, left, H, W, fmt, "bt709", "limited", ref)
        for variant, (doff, dmode), (roff, rmode) in [("contiguous", (0, "pad4"), (0, "pad4")), ("loose4", (0, "pad4"), (0, "pad4")),
                                                      ("odd", (0, "pad4"), (0, "pad4")), ("contiguous", (1, "pad4"), (0, "pad4")),
                                                      ("contiguous", (0, "pad4"), (0, "loose")), ("contiguous", (0, "tight"), (3, "tight"))]:
            xv = float_planes(x, variant)
            dstv, refv = frame_views(fmt, 2, H, W, doff, dmode), frame_views(fmt, 2, H, W, roff, rmode, ref)
            rc, wide, sse, ws = emit_raw(xv, fmt, "bt709", "limited", H, W, Hp, Wp, top, left, dstv, refv)
            case = (hw, fmt, left, top, variant, doff, dmode, roff, rmode)
            aligned = lambda vs: all(v.offset == 0 and v.strides[0] % 4 == 0 and v.strides[1] % 4 == 0 for v in vs)      # noqa: E731
            assert rc == 0 and wide == int(left % 4 == 0 and variant != "odd" and aligned(dstv) and aligned(refv)), case
            seen.add(wide)
            check_sums(sse, ws, want_sums, FR().lib().pc_frames_emit_workspace_size(2, H, W))
            for v, w in zip(dstv, want):
                got, clean = v.read()
                assert clean and np.array_equal(got, w), case
    assert seen == {0, 1}


def test_nan_and_inf_behave_as_specified():
    """NaN -> 0 before the matrix, +inf -> 1, -inf -> 0: a frame of exactly known codes"""
    frames = FR()
    x = np.zeros((1, 3, 64, 64), np.float32)
    x[0, :, 0:2, 0:2] = np.nan                                    # black
    x[0, :, 0:2, 2:4] = np.inf                                    # white
    x[0, :, 2:4, 0:2] = -np.inf                                   # black
    x[0, 0, 2:4, 2:4], x[0, 1, 2:4, 2:4], x[0, 2, 2:4, 2:4] = np.inf, np.nan, -np.inf       # pure red
    geom = geometry(64, 64)
    for fmt, rng in itertools.product(FC.FORMATS, FC.RANGES):
        yo, ys, co, cs, mx = FC.levels(fmt, rng)
        out = frames.from_model_output(torch.from_numpy(x).to(DEV), geom, fmt, "bt709", rng)
        Y, Cb, Cr = FC.codes(tuple(p.cpu().numpy() for p in out), fmt)
        assert (Y[0, 0:2, 0:2] == yo).all() and (Y[0, 0:2, 2:4] == yo + ys).all() and (Y[0, 2:4, 0:2] == yo).all()
        assert (Cb[0, 0, 0:2] == co).all() and (Cr[0, 0, 0:2] == co).all() and Cb[0, 1, 0] == co and Cr[0, 1, 0] == co
        kr = np.float32(0.2126)
        assert (Y[0, 2:4, 2:4] == int(np.rint(kr * np.float32(ys) + np.float32(yo)))).all()
        assert abs(int(Cr[0, 1, 1]) - min(mx, co + cs / 2)) <= 1                               # Cr' of pure red is a half
        want = FC.emit(x, 0, 0, 64, 64, fmt, "bt709", rng)
        assert all(np.array_equal(p.cpu().numpy()[0], w[0]) for p, w in zip(out, want))


def test_from_model_output_python_entry_and_psnr():
    frames = FR()
    for fmt, (H, W) in zip(FC.FORMATS, [(100, 150), (65, 63), (3, 5)]):
        g = geometry(H, W)
        ref = FC.random_frame(2, H, W, fmt, seed=8)
        x = FC.hostile_planes(ref, fmt, "bt601", "full", g.Hp, g.Wp, g.top, g.left, seed=4)
        want = FC.emit(x, g.top, g.left, H, W, fmt, "bt601", "full")
        want_sums = FC.sums(x, g.top, g.left, H, W, fmt, "bt601", "full", ref)
        xt = torch.from_numpy(x).to(DEV)
        rt = tuple(torch.from_numpy(p).to(DEV) for p in ref)
        out, d = frames.from_model_output(xt, g, fmt, "bt601", "full", ref=rt)
        assert all(np.array_equal(p.cpu().numpy(), w) for p, w in zip(out, want)) and d.sse.tolist() == want_sums
        only = frames.from_model_output(xt, g, fmt, "bt601", "full", ref=rt, image=False)
        assert only.sse.tolist() == want_sums
        plain = frames.from_model_output(xt[0], g, fmt, "bt601", "full")
        assert all(np.array_equal(p.cpu().numpy(), w[0]) for p, w in zip(plain, want))
        Hc, Wc = FC.chroma_size(H, W)
        peak = 2 ** FC.bits(fmt) - 1
        assert d.psnr_y() == [FC.psnr(s[0], H * W, peak) for s in want_sums]
        assert d.psnr_cb() == [FC.psnr(s[1], Hc * Wc, peak) for s in want_sums] and d.psnr_cr() == [FC.psnr(s[2], Hc * Wc, peak) for s in want_sums]
        # a frame against itself: zero sums, infinite PSNR
        same = frames.from_model_output(xt, g, fmt, "bt601", "full", ref=out, image=False)
        assert same.sse.tolist() == [[0, 0, 0]] * 2 and same.psnr_y() == [float("inf")] * 2
        # a strided x_hat (channels last in memory) is copied, not refused
        cl = xt.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert all(torch.equal(a, b) for a, b in zip(frames.from_model_output(cl, g, fmt, "bt601", "full"), out))


# -- through the codec ---------------------------------------------------------------------------------------------------------------

QUALITIES = [0, 0.5]


@functools.lru_cache(maxsize=None)
def codec_frame(H, W):
    """a smooth NV12 frame (the codec's synthetic weights are not meant for noise; any frame does)"""
    g = np.random.default_rng(H + W)
    lo = torch.from_numpy(g.uniform(0.1, 0.9, (1, 3, 8, 8)).astype(np.float32))
    x = torch.nn.functional.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False).numpy()
    return FC.emit(x, 0, 0, H, W, "nv12", "bt709", "limited")


@pytest.mark.parametrize("hw", [(64, 64), (100, 150)])
def test_encode_frame_and_decode_frame_through_the_codec(hw):
    from progressivecodec_amd import container, pixels
    frames = FR()
    net = gpu_codec()
    H, W = hw
    f = codec_frame(H, W)
    planes = tuple(torch.from_numpy(p[0]).to(DEV) for p in f)
    buf = frames.encode_frame(net, planes, QUALITIES, "nv12", "bt709", "limited", "linear", mask_pol=POL)
    assert isinstance(buf, bytes)
    hd = frames.parse_frame(buf)
    assert (hd["fmt"], hd["matrix"], hd["range"], hd["upsample"], hd["bits"], hd["H"], hd["W"]) == ("nv12", "bt709", "limited", "linear", 8, H, W)
    # the PCB1 inside parses, and its strings are those of compress_levels on the ingested planes
    inner = container.parse_header(hd["blob"])
    g = geometry(H, W)
    assert inner["image_size"] == (H, W) and inner["shape"] == (g.Hp // 64, g.Wp // 64) and inner["qualities"] == [float(q) for q in QUALITIES]
    x, geom = frames.to_model_input(planes, "nv12", "bt709", "limited", "linear")
    assert geom == g and same_bits(x.cpu().numpy(), FC.ingest(f, "nv12", "bt709", "limited", "linear", g.Hp, g.Wp, g.top, g.left))
    datas = net.compress_levels(x, QUALITIES, mask_pol=POL)
    strings = container.unpack(hd["blob"])[0]
    for lv, d in enumerate(datas):
        ys, zs = d["strings"]
        assert strings[lv] == [[[bytes(s[0])] for s in ys], [bytes(zs[0])]]
    for lv, (q, d) in enumerate(zip(QUALITIES, datas)):
        x_hat = net.decompress(d["strings"], d["shape"], q, POL)["x_hat"]
        want = frames.from_model_output(x_hat, g, "nv12", "bt709", "limited")
        got = frames.decode_frame(net, buf, level=lv)
        assert len(got) == 2 and tuple(got[0].shape) == (H, W) and all(torch.equal(a, b[0]) for a, b in zip(got, want))
        assert all(np.array_equal(a.cpu().numpy(), b[0]) for a, b in zip(got, FC.emit(x_hat.cpu().numpy(), g.top, g.left, H, W, "nv12", "bt709", "limited")))
        # the same level in another layout: the NV12 codes re-laid out
        planar = frames.decode_frame(net, buf, level=lv, fmt="i420")
        relaid = FC.relayout(tuple(p.cpu().numpy()[None] for p in got), "nv12", "i420")
        assert len(planar) == 3 and all(np.array_equal(a.cpu().numpy(), b[0]) for a, b in zip(planar, relaid))
        # and the RGB rendering of the inner blob is pixels.decode_image's
        assert torch.equal(pixels.decode_image(net, hd["blob"], level=lv, layout="chw"), pixels.from_model_output(x_hat, g, "chw")[0])
    assert all(torch.equal(a, b) for a, b in zip(frames.decode_frame(net, buf), frames.decode_frame(net, buf, level=len(QUALITIES) - 1)))
    if hw == (64, 64):
        both = frames.encode_frame(net, tuple(torch.stack([p, p.flip(0)]) for p in planes), QUALITIES, "nv12", mask_pol=POL)
        assert isinstance(both, list) and len(both) == 2 and both[0] == buf and both[1] != buf


# -- refusals ------------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_return_their_codes_without_a_launch():
    """real device buffers, poisoned: a refused call leaves every one of them as it was"""
    frames = FR()
    L = frames.lib()
    H, W = 10, 12
    g = geometry(H, W)
    f = FC.random_frame(1, H, W, "nv12", seed=1)
    k = frames.coefficients("bt709")
    src = frame_views("nv12", 1, H, W, 0, "tight", f)
    for bad in [dict(fmt=3), dict(range=2), dict(up=2), dict(H=0), dict(W=0), dict(B=0), dict(top=60), dict(left=-1)]:
        a = dict(fmt=0, range=0, up=1, a=k.a, b=k.b, c=k.c, d=k.d, B=1, H=H, W=W)
        tail = dict(Hp=g.Hp, Wp=g.Wp, top=g.top, left=g.left)
        a.update({n: v for n, v in bad.items() if n in a})
        tail.update({n: v for n, v in bad.items() if n in tail})
        dst = torch.full((1, 3, g.Hp, g.Wp), float("nan"), device=DEV)
        s = struct_of(src)
        assert L.pc_frames_ingest(C.byref(s), *a.values(), dst.data_ptr(), *tail.values(), stream()) == -1, bad
        torch.cuda.synchronize()
        assert torch.isnan(dst).all(), bad
    short = struct_of(src)
    short.y_row = W - 1
    dst = torch.full((1, 3, g.Hp, g.Wp), float("nan"), device=DEV)
    assert L.pc_frames_ingest(C.byref(short), 0, 0, 1, k.a, k.b, k.c, k.d, 1, H, W, dst.data_ptr(), g.Hp, g.Wp, g.top, g.left, stream()) == -1
    assert L.pc_frames_ingest(C.byref(struct_of(src)), 0, 0, 1, k.a, k.b, k.c, k.d, 1, H, W, None, g.Hp, g.Wp, g.top, g.left, stream()) == -1
    torch.cuda.synchronize()
    assert torch.isnan(dst).all()
    # the emit: a workspace one byte short, a stride shorter than the row, no destination and no reference
    x = torch.zeros((1, 3, g.Hp, g.Wp), device=DEV)
    need = L.pc_frames_emit_workspace_size(1, H, W)
    dstv = frame_views("nv12", 1, H, W)
    rc, _, sse, ws = emit_raw(x, "nv12", "bt709", "limited", H, W, g.Hp, g.Wp, g.top, g.left, dstv, src, nbytes=need - 1)
    assert rc == -1 and (sse == POISON64).all() and (ws == POISON64).all()
    for v in dstv:
        got, clean = v.read()
        assert clean and (got == 0xA5).all()

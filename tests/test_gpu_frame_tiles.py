"""Tiled coding of YUV 4:2:0 frames on the GPU (progressivecodec_amd/frame_tiles.py, libpc_frame_tiles.so) against its restatement
(tests/frame_tiles_contract.py): the cut bit for bit and the stitch and its sums exactly, for every format, range and upsampler on
both access paths and with O = 4, and encode_frame_tiled / decode_frame_tiled through the codec and the PCG1 container.

T = 64 throughout.  Sizes: the smallest that take every branch -- a single chroma sample, odd dimensions, partial last items, one tile
and 2 x 3 tiles, bands that start in the middle of an eight-column item.  Every plane is a view some elements into a larger poisoned
allocation with its own strides (View of tests/test_gpu_frames.py), so that an element left unwritten, or one written outside the
view, shows."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import frame_tiles_contract as GC
from tests import frames_contract as FC
from tests import tiles_contract as TC
from tests.test_gpu_frames import POISON64, View, same_bits
from tests.test_gpu_tiles import float_tiles
from tests.util import gpu_codec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POL = "point-based-std"
T = 64
SIZES = [(1, 1), (2, 2), (3, 5), (64, 64), (65, 63), (100, 150), (127, 129)]
OVERLAPS = [0, 4, 16, 32]
MATS = list(FC.MATRICES)


def FT():
    from progressivecodec_amd import frame_tiles
    return frame_tiles


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def cases():
    """fmt x range x upsample, the matrix and the overlap cycled so that every format meets every overlap"""
    for n, (f, (rng, up)) in enumerate(itertools.product(range(3), itertools.product(FC.RANGES, FC.UPSAMPLES))):
        yield n, FC.FORMATS[f], MATS[n % 3], rng, up, OVERLAPS[(n + f) % 4]


def frame_views(fmt, H, W, back=0, mode="pad4", data=None):
    """The planes of one frame as Views.  back: the luma columns the frame's first sample lies past an aligned address (the window's
    x0 % 8, so that frame column 8 * floor(x0 / 8) is the aligned one: what the wide path of the stitch needs); the chroma planes lie
    back (interleaved) or back / 2 (planar) elements in.  mode "loose": odd offsets and row strides that are no multiples of 4."""
    Hc, Wc = FC.chroma_size(H, W)
    dt = np.uint16 if fmt == "p010" else np.uint8
    shapes = [(1, H, W), (1, Hc, Wc), (1, Hc, Wc)] if fmt == "i420" else [(1, H, W), (1, Hc, Wc, 2)]
    odd = 0 if mode == "pad4" else 1
    offs = [back + odd] + ([back // 2 + odd] * 2 if fmt == "i420" else [back + odd])
    return [View(s, dt, o, mode, None if data is None else data[i]) for i, (s, o) in enumerate(zip(shapes, offs))]


def struct_of(views):
    from progressivecodec_amd import frames
    return frames._frame_struct([v.t for v in views])


def cut_raw(views, fmt, matrix, rng, up, H, W, O, rect, dst_offset=0):
    """pc_frame_tiles_cut into a NaN-poisoned buffer with guard floats on both sides -> (status, wide as pc_frame_tiles_plan reports
    it, the [n,3,T,T] result, whether the guards kept their bits)"""
    from progressivecodec_amd import frames
    ft = FT()
    L = ft.lib()
    k = frames.coefficients(matrix)
    n = rect[2] * rect[3] * 3 * T * T
    buf = torch.full((4 + dst_offset + n + 4,), float("nan"), dtype=torch.float32, device=DEV)
    dst = buf[4 + dst_offset:4 + dst_offset + n]
    src = struct_of(views)
    wide = C.c_int(-1)
    assert L.pc_frame_tiles_plan(ft.CUT, frames.FORMATS[fmt], C.byref(src), dst.data_ptr(), 3 * T * T, T * T, T, O, 0, None, C.byref(wide)) == 0
    rc = L.pc_frame_tiles_cut(C.byref(src), frames.FORMATS[fmt], frames.RANGES[rng], frames.UPSAMPLES[up], k.a, k.b, k.c, k.d, H, W, T, O,
                              *rect, dst.data_ptr(), stream())
    h = buf.cpu().numpy()
    guards = bool(np.isnan(h[:4 + dst_offset]).all() and np.isnan(h[4 + dst_offset + n:]).all())
    return rc, wide.value, h[4 + dst_offset:4 + dst_offset + n].reshape(-1, 3, T, T), guards


# -- cut -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", SIZES)
def test_cut_is_the_restatement_bit_for_bit(hw):
    """every fmt x range x upsample; each case once from aligned planes (wide where O is a multiple of 8) and once from loose,
    offset planes into a misaligned destination (narrow).  Every element is written, NaN and guards show what is not."""
    H, W = hw
    seen = set()
    per_fmt = {f: set() for f in FC.FORMATS}
    for n, fmt, matrix, rng, up, O in cases():
        ny, nx = TC.grid(H, W, T, O)
        f = FC.random_frame(1, H, W, fmt, seed=1000 * H + W + n)
        want = GC.cut(f, fmt, matrix, rng, up, T, O)
        for mode, dst_offset in [("pad4", 0), ("loose", 1 + n % 3)]:
            views = frame_views(fmt, H, W, 0, mode, f)
            rc, wide, got, guards = cut_raw(views, fmt, matrix, rng, up, H, W, O, (0, 0, ny, nx), dst_offset)
            case = (hw, fmt, matrix, rng, up, O, mode)
            assert rc == 0 and guards, case
            assert wide == int(mode == "pad4" and O % 8 == 0), case
            seen.add(wide)
            per_fmt[fmt].add((wide, O))
            assert not np.isnan(got).any() and same_bits(got, want), case
        if ny * nx > 1:                                                             # a sub-grid is the corresponding tiles of the full cut
            for rect in [(ny - 1, 0, 1, nx), (0, nx - 1, ny, 1)]:
                rc, _, got, guards = cut_raw(frame_views(fmt, H, W, 0, "pad4", f), fmt, matrix, rng, up, H, W, O, rect)
                idx = [(rect[0] + a) * nx + rect[1] + b for a in range(rect[2]) for b in range(rect[3])]
                assert rc == 0 and guards and same_bits(got, want[idx]) and same_bits(got, GC.cut(f, fmt, matrix, rng, up, T, O, rect)), (hw, fmt, O, rect)
    assert seen == {0, 1}
    assert all({(1, 0), (0, 4), (1, 16), (1, 32), (0, 0)} <= s for s in per_fmt.values())


# -- stitch --------------------------------------------------------------------------------------------------------------------------

def windows(H, W, O):
    """(window, rectangle or None for the whole grid): the whole frame, the last odd (or last two) rows and columns, an interior
    2 x 2, one that straddles a band's first edge in the middle of an eight-column item, and that one from the sub-rectangle that
    just covers it"""
    from progressivecodec_amd import tiles
    S = T - O
    out = [((0, 0, H, W), None)]
    y1, x1 = H - 1 - (H - 1) % 2, W - 1 - (W - 1) % 2
    if (y1, x1) != (0, 0):
        out.append(((y1, x1, H - y1, W - x1), None))
    if H >= 8 and W >= 12:
        out.append(((2 * (H // 4), 2 * (W // 4) + 2, 2, 2), None))
    if H > T or W > T:
        y0, x0 = (S - 2 if H > T else 0), (S - 6 if W > T else 2)
        win = (y0, x0, min(O + 6, H - y0), min(O + 12, W - x0))                       # even sizes, or ending on the frame's edge
        out.append((win, None))
        out.append((win, tiles.grid_of(H, W, T, O).covering(win)))
    assert all(GC.admissible(H, W, w) for w, _ in out), (H, W, O, out)
    return out


def window_frame(f, fmt, win):
    """the window of a whole frame of tests/frames_contract.py, as a frame"""
    return FC.frame(*GC.crop_codes(FC.codes(f, fmt), win), fmt)


def stitch_raw(xv, fmt, matrix, rng, H, W, O, rect, win, dst_views, ref_views, nbytes=None, T=T):
    """pc_frame_tiles_stitch -> (status, wide, the [3,3] sums buffer whose middle row is `sse`, poisoned beforehand, the workspace
    with one more word than needed)"""
    from progressivecodec_amd import frames
    ft = FT()
    L = ft.lib()
    k = frames.coefficients(matrix)
    y0, x0, h, w = win
    dst = struct_of(dst_views) if dst_views is not None else None
    ref = struct_of(ref_views) if ref_views is not None else None
    need = L.pc_frame_tiles_stitch_workspace_size(x0, h, w)
    ws = torch.full((max(1, need // 8) + 1,), POISON64, dtype=torch.int64, device=DEV)
    sse = torch.full((3, 3), POISON64, dtype=torch.int64, device=DEV)
    wide = C.c_int(-1)
    pd, pr = (C.byref(dst) if dst is not None else None), (C.byref(ref) if ref is not None else None)
    prc = L.pc_frame_tiles_plan(ft.STITCH, frames.FORMATS[fmt], pd, xv.data_ptr(), xv.stride(0), xv.stride(1), xv.stride(2), O, x0, pr, C.byref(wide))
    assert prc == (-1 if x0 % 2 else 0)                                                         # an odd first column has no plan
    rc = L.pc_frame_tiles_stitch(xv.data_ptr(), xv.stride(0), xv.stride(1), xv.stride(2), H, W, T, O, *rect, y0, x0, h, w, frames.FORMATS[fmt],
                                 frames.RANGES[rng], k.kr, k.kg, k.kb, k.ib, k.ir, pd, pr, ws.data_ptr() if ref is not None else None,
                                 (need if nbytes is None else nbytes) if ref is not None else 0, sse[1].data_ptr() if ref is not None else None, stream())
    return rc, wide.value, sse.cpu(), ws.cpu(), need


def check_sums(sse, ws, want, need):
    assert sse[0].tolist() == [POISON64] * 3 and sse[2].tolist() == [POISON64] * 3              # the guard words keep their bits
    assert sse[1].tolist() == want
    assert ws[-1].item() == POISON64 and (ws[:need // 8] != POISON64).all()                     # every partial written, none beyond


def check_planes(views, want, case):
    for v, w in zip(views, want):
        got, clean = v.read()
        assert clean and np.array_equal(got, w), case


@pytest.mark.parametrize("hw", SIZES)
def test_stitch_and_sums_are_the_restatement_exactly(hw):
    """hostile tiles (NaN, +-inf, -0.0, denormals, values outside [0, 1]); the tile tensor contiguous, strided with every 16-byte
    alignment kept, and misaligned; destinations whose column 8 * floor(x0 / 8) is aligned (wide unless the tiles are misaligned)
    and loose ones (narrow).  The sums also without an image, and the image also without sums, for the whole frame."""
    H, W = hw
    L = FT().lib()
    seen = set()
    for n, fmt, matrix, rng, _, O in cases():
        ny, nx = TC.grid(H, W, T, O)
        x = TC.hostile_tiles(ny * nx, T, seed=77 * H + W + n)
        ref = FC.random_frame(1, H, W, fmt, seed=n)
        variant = ("contiguous", "loose4", "odd")[n % 3]
        mode = ("pad4", "loose")[(n // 3) % 2]
        for win, rect in windows(H, W, O):
            y0, x0, h, w = win
            full = rect is None
            rect = (0, 0, ny, nx) if full else rect
            idx = [(rect[0] + a) * nx + rect[1] + b for a in range(rect[2]) for b in range(rect[3])]
            xv = float_tiles(x[idx], variant)
            want = GC.stitch(x, H, W, T, O, fmt, matrix, rng, window=win)
            want_sums = GC.sums(x, H, W, T, O, fmt, matrix, rng, ref, window=win)
            refv = frame_views(fmt, h, w, x0 % 8, mode, window_frame(ref, fmt, win))
            case = (hw, fmt, matrix, rng, O, variant, mode, win, rect)
            for with_image, with_ref in [(True, True), (False, True), (True, False)] if win == (0, 0, H, W) and full else [(True, True)]:
                dstv = frame_views(fmt, h, w, x0 % 8, mode) if with_image else None
                rc, wide, sse, ws, need = stitch_raw(xv, fmt, matrix, rng, H, W, O, rect, win, dstv, refv if with_ref else None)
                assert rc == 0, case
                assert wide == int(mode == "pad4" and variant != "odd"), case
                seen.add(wide)
                assert need == L.pc_frame_tiles_stitch_workspace_size(x0, h, w) == 24 * -(-(-(-h // 2) * (-(-(x0 + w) // 8) - x0 // 8)) // 256)
                if with_ref:
                    check_sums(sse, ws, want_sums, need)
                else:
                    assert (sse == POISON64).all() and (ws == POISON64).all(), case
                if with_image:
                    check_planes(dstv, want, case)
    assert seen == {0, 1}


@pytest.mark.parametrize("fmt", FC.FORMATS)
@pytest.mark.parametrize("hw", [(3, 5), (65, 63), (100, 150)])
def test_wide_and_narrow_agree_on_the_same_data(hw, fmt):
    """one frame and one tile set under every alignment: the cut from aligned and from offset planes, with O = 0, 4 and 16; the
    stitch of windows whose first column is 0, 2, 4, 6 and 8 mod 8 into aligned and unaligned destinations, against aligned and loose
    references.  Wide exactly where pc_frame_tiles_plan's preconditions hold, and the same bits and sums everywhere."""
    H, W = hw
    f = FC.random_frame(1, H, W, fmt, seed=H + W)
    seen = set()
    for O in (0, 4, 16):
        ny, nx = TC.grid(H, W, T, O)
        want = GC.cut(f, fmt, "bt601", "limited", "linear", T, O)
        got = {}
        for mode, dst_offset in [("pad4", 0), ("pad4", 1), ("loose", 0), ("tight", 0)]:
            views = frame_views(fmt, H, W, 0, mode, f)
            rc, wide, out, guards = cut_raw(views, fmt, "bt601", "limited", "linear", H, W, O, (0, 0, ny, nx), dst_offset)
            aligned = all(v.offset == 0 and v.strides[1] % 4 == 0 for v in views)
            assert rc == 0 and guards and wide == int(O % 8 == 0 and aligned and dst_offset == 0), (hw, fmt, O, mode, dst_offset)
            got[wide] = out
            assert same_bits(out, want), (hw, fmt, O, mode, dst_offset)
        seen |= set(got)
        assert O == 4 or same_bits(got[0], got[1])
        x = TC.hostile_tiles(ny * nx, T, seed=O + H)
        for x0 in [v for v in (0, 2, 4, 6, 8) if v < W]:
            win = (0, x0, H, W - x0)
            want_f = GC.stitch(x, H, W, T, O, fmt, "bt709", "full", window=win)
            want_s = GC.sums(x, H, W, T, O, fmt, "bt709", "full", f, window=win)
            rf = window_frame(f, fmt, win)
            sums = {}
            for variant, (dback, dmode), (rback, rmode) in [("contiguous", (x0, "pad4"), (x0, "pad4")), ("loose4", (x0, "pad4"), (x0, "pad4")),
                                                            ("odd", (x0, "pad4"), (x0, "pad4")), ("contiguous", (x0 + 2, "pad4"), (x0, "pad4")),
                                                            ("contiguous", (x0, "pad4"), (x0, "loose")), ("contiguous", (x0, "tight"), (x0 + 1, "tight"))]:
                xv = float_tiles(x, variant)
                dstv, refv = frame_views(fmt, H, W - x0, dback % 8, dmode), frame_views(fmt, H, W - x0, rback % 8, rmode, rf)
                rc, wide, sse, ws, need = stitch_raw(xv, fmt, "bt709", "full", H, W, O, (0, 0, ny, nx), win, dstv, refv)
                case = (hw, fmt, O, x0, variant, dback, dmode, rback, rmode)

                def ok(vs, back):                                                     # column 8 * floor(x0 / 8) on four elements
                    halves = [1, 1] if fmt != "i420" else [1, 2, 2]
                    return all((v.offset - (x0 % 8) // d) % 4 == 0 and v.strides[1] % 4 == 0 for v, d in zip(vs, halves))
                assert rc == 0 and wide == int(variant != "odd" and ok(dstv, dback) and ok(refv, rback)), case
                sums[wide] = sse[1].tolist()
                check_sums(sse, ws, want_s, need)
                check_planes(dstv, want_f, case)
            seen |= set(sums)
            assert len(sums) == 2 and sums[0] == sums[1]
    assert seen == {0, 1}


def test_nan_inf_and_out_of_range_tiles_behave_as_specified():
    """NaN -> 0 before the blend, +inf -> 1, -inf -> 0, 7.5 -> 1, -3 -> 0: a frame of exactly known codes, with and without a band"""
    ft = FT()
    for O in (0, 16):
        H, W = 64, 100 if O else 64
        g = ft.grid_of(H, W, T, O)
        x = np.zeros((g.n, 3, T, T), np.float32)
        x[:, :, 0:2, 0:2] = np.nan                                    # black
        x[:, :, 0:2, 2:4] = np.inf                                    # white
        x[:, :, 2:4, 0:2] = -np.inf                                   # black
        x[:, 0, 2:4, 2:4], x[:, 1, 2:4, 2:4], x[:, 2, 2:4, 2:4] = np.inf, np.nan, -np.inf       # pure red
        x[:, :, 4:6, 0:2], x[:, :, 4:6, 2:4] = 7.5, -3.0              # white, black
        if O:                                                         # in the band (columns 48 .. 63): NaN in one tile, white in the other
            x[0, :, 8:10, 56:58], x[1, :, 8:10, 8:10] = np.nan, np.inf
        for fmt, rng in itertools.product(FC.FORMATS, FC.RANGES):
            yo, ys, co, cs, mx = FC.levels(fmt, rng)
            out = ft.stitch_frame(torch.from_numpy(x).to(DEV), g, fmt, "bt709", rng)
            Y, Cb, Cr = FC.codes(tuple(p.cpu().numpy()[None] for p in out), fmt)
            assert (Y[0, 0:2, 0:2] == yo).all() and (Y[0, 0:2, 2:4] == yo + ys).all() and (Y[0, 2:4, 0:2] == yo).all()
            assert (Y[0, 4:6, 0:2] == yo + ys).all() and (Y[0, 4:6, 2:4] == yo).all()
            assert (Cb[0, 0, 0:2] == co).all() and (Cr[0, 0, 0:2] == co).all() and Cb[0, 1, 0] == co and Cr[0, 1, 0] == co
            assert (Y[0, 2:4, 2:4] == int(np.rint(np.float32(0.2126) * np.float32(ys) + np.float32(yo)))).all()
            assert abs(int(Cr[0, 1, 1]) - min(mx, co + cs / 2)) <= 1                               # Cr' of pure red is a half
            if O:                                                     # m = w_later * 1: gray, at the band weights of columns 56, 57
                wl = TC.weights(1, 2, T, O)[8:10]
                assert (Y[0, 8:10, 56:58] == np.rint(wl * np.float32(ys) + np.float32(yo)).astype(np.int64)[None, :]).all()
            want = GC.stitch(x, H, W, T, O, fmt, "bt709", rng)
            assert all(np.array_equal(p.cpu().numpy(), w[0]) for p, w in zip(out, want))


def test_refused_calls_launch_nothing():
    """real device buffers, poisoned: a refused call leaves every one of them as it was"""
    from progressivecodec_amd import frames
    ft = FT()
    L = ft.lib()
    H, W, O = 100, 150, 16
    f = FC.random_frame(1, H, W, "nv12", seed=1)
    k = frames.coefficients("bt709")
    src = frame_views("nv12", H, W, 0, "tight", f)
    for bad in [dict(fmt=3), dict(range=2), dict(up=2), dict(H=0), dict(W=0), dict(T=96), dict(O=6), dict(nty=3), dict(tx0=-1)]:
        a = dict(fmt=0, range=0, up=1, a=k.a, b=k.b, c=k.c, d=k.d, H=H, W=W, T=T, O=O, ty0=0, tx0=0, nty=2, ntx=3)
        a.update(bad)
        dst = torch.full((6, 3, T, T), float("nan"), device=DEV)
        s = struct_of(src)
        assert L.pc_frame_tiles_cut(C.byref(s), *a.values(), dst.data_ptr(), stream()) == -1, bad
        torch.cuda.synchronize()
        assert torch.isnan(dst).all(), bad
    short = struct_of(src)
    short.y_row = W - 1
    dst = torch.full((6, 3, T, T), float("nan"), device=DEV)
    assert L.pc_frame_tiles_cut(C.byref(short), 0, 0, 1, k.a, k.b, k.c, k.d, H, W, T, O, 0, 0, 2, 3, dst.data_ptr(), stream()) == -1
    assert L.pc_frame_tiles_cut(C.byref(struct_of(src)), 0, 0, 1, k.a, k.b, k.c, k.d, H, W, T, O, 0, 0, 2, 3, None, stream()) == -1
    torch.cuda.synchronize()
    assert torch.isnan(dst).all()
    # the stitch: an inadmissible window, a rectangle that lacks a covering tile, a workspace one byte short
    x = torch.zeros((6, 3, T, T), device=DEV)
    for win, rect, short_by in [((41, 50, 30, 60), (0, 0, 2, 3), 0), ((40, 50, 31, 60), (0, 0, 2, 3), 0), ((40, 51, 30, 60), (0, 0, 2, 3), 0),
                                ((40, 50, 30, 61), (0, 0, 2, 3), 0), ((40, 50, 30, 60), (0, 0, 2, 2), 0), ((40, 50, 30, 60), (1, 0, 1, 3), 0),
                                ((40, 50, 30, 60), (0, 0, 2, 3), 1)]:
        h, w = win[2:]
        dstv = frame_views("nv12", h, w, win[1] % 8, "pad4")
        refv = frame_views("nv12", h, w, win[1] % 8, "pad4", window_frame(f, "nv12", (40, 50, h, w)))
        need = L.pc_frame_tiles_stitch_workspace_size(*win[1:])
        xs = x[:rect[2] * rect[3]]
        rc, _, sse, ws, _ = stitch_raw(xs, "nv12", "bt709", "limited", H, W, O, rect, win, dstv, refv, nbytes=need - short_by)
        assert rc == -1 and (sse == POISON64).all() and (ws == POISON64).all(), (win, rect, short_by)
        for v in dstv:
            got, clean = v.read()
            assert clean and (got == 0xA5).all(), (win, rect, short_by)


def test_python_entries():
    """cut_frame, stitch_frame (windows, ref as the whole frame, image=False, a strided tile tensor), Distortion and plan"""
    from progressivecodec_amd import frames
    ft = FT()
    for fmt, (H, W), O in zip(FC.FORMATS, [(100, 150), (65, 63), (127, 129)], [16, 4, 32]):
        f = FC.random_frame(1, H, W, fmt, seed=3)
        planes = tuple(torch.from_numpy(p[0]).to(DEV) for p in f)
        tiles, g = ft.cut_frame(planes, fmt, "bt2020", "full", "nearest", tile=T, overlap=O)
        ny, nx = TC.grid(H, W, T, O)
        assert g == ft.grid_of(H, W, T, O) and (g.ny, g.nx) == (ny, nx)
        assert same_bits(tiles.cpu().numpy(), GC.cut(f, fmt, "bt2020", "full", "nearest", T, O))
        batched = tuple(torch.from_numpy(p).to(DEV) for p in f)                          # [1,H,W] and so on are one frame, too
        assert torch.equal(ft.cut_frame(batched, fmt, "bt2020", "full", "nearest", tile=T, overlap=O)[0], tiles)
        sub, gs = ft.cut_frame(planes, fmt, "bt2020", "full", "nearest", tile=T, overlap=O, rect=(ny - 1, 0, 1, nx))
        assert gs.rect == (ny - 1, 0, 1, nx) and torch.equal(sub, tiles[(ny - 1) * nx:])
        assert ft.plan(ft.CUT, batched, fmt, tiles, overlap=O) == (O % 8 == 0 and all(p.stride(1) % 4 == 0 for p in batched))
        # planes whose innermost stride does not fit are copied, not refused
        wider = torch.from_numpy(np.repeat(f[0][0], 2, axis=1)).to(DEV)
        assert torch.equal(ft.cut_frame((wider[:, ::2],) + planes[1:], fmt, "bt2020", "full", "nearest", tile=T, overlap=O)[0], tiles)
        x = TC.hostile_tiles(ny * nx, T, seed=8)
        xt = torch.from_numpy(x).to(DEV)
        whole = GC.stitch(x, H, W, T, O, fmt, "bt601", "full")
        out, d = ft.stitch_frame(xt, g, fmt, "bt601", "full", ref=planes)
        want_sums = GC.sums(x, H, W, T, O, fmt, "bt601", "full", f)
        assert all(np.array_equal(p.cpu().numpy(), w[0]) for p, w in zip(out, whole)) and d.sse.tolist() == [want_sums]
        assert ft.stitch_frame(xt, g, fmt, "bt601", "full", ref=planes, image=False).sse.tolist() == [want_sums]
        Hc, Wc = FC.chroma_size(H, W)
        peak = 2 ** FC.bits(fmt) - 1
        assert d.psnr_y() == [FC.psnr(want_sums[0], H * W, peak)] and d.psnr_cb() == [FC.psnr(want_sums[1], Hc * Wc, peak)]
        same = ft.stitch_frame(xt, g, fmt, "bt601", "full", ref=out, image=False)          # a frame against itself: zero sums
        assert same.sse.tolist() == [[0, 0, 0]] and same.psnr_y() == [float("inf")]
        for win in [(H - 1 - (H - 1) % 2, 6, 1 + (H - 1) % 2, 20), (T - O - 2, T - O - 6, min(O + 6, H - T + O + 2), min(O + 12, W - T + O + 6)), (2, W - 1 - (W - 1) % 2, 8, 1 + (W - 1) % 2)]:
            y0, x0, h, w = win
            rect = g.covering(win)
            idx = [(rect[0] + a) * nx + rect[1] + b for a in range(rect[2]) for b in range(rect[3])]
            part, dw = ft.stitch_frame(xt[idx], g.with_rect(rect), fmt, "bt601", "full", window=win, ref=planes)
            want = window_frame(whole, fmt, win)
            assert all(np.array_equal(p.cpu().numpy(), w_[0]) for p, w_ in zip(part, want)), (fmt, win)
            assert dw.sse.tolist() == [GC.sums(x, H, W, T, O, fmt, "bt601", "full", f, window=win)] and (dw.H, dw.W) == (h, w)
        # a strided tile tensor (channels last in memory) is copied, not refused
        cl = xt.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert all(torch.equal(a, b) for a, b in zip(ft.stitch_frame(cl, g, fmt, "bt601", "full"), out))
        with pytest.raises(ValueError, match="admissible"):
            ft.stitch_frame(xt, g, fmt, window=(1, 0, 2, 2))


# -- through the codec ---------------------------------------------------------------------------------------------------------------

QUALITIES = [0, 0.5, 10]
H0, W0 = 100, 150                                                          # 2 x 3 tiles of 64 x 64, with and without overlap
PARAMS = ("nv12", "bt709", "limited", "linear")


@functools.lru_cache(maxsize=None)
def codec_frame(H, W):
    """a smooth NV12 frame (the codec's synthetic weights are not meant for noise; any frame does)"""
    g = np.random.default_rng(H + W)
    lo = torch.from_numpy(g.uniform(0.1, 0.9, (1, 3, 8, 8)).astype(np.float32))
    x = torch.nn.functional.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False).numpy()
    return FC.emit(x, 0, 0, H, W, "nv12", "bt709", "limited")


def codec_planes(H=H0, W=W0):
    return tuple(torch.from_numpy(p[0]).to(DEV) for p in codec_frame(H, W))


@functools.lru_cache(maxsize=None)
def encoded(O, per_call=32):
    return FT().encode_frame_tiled(gpu_codec(), codec_planes(), QUALITIES, *PARAMS, tile=T, overlap=O, mask_pol=POL, max_tiles_per_call=per_call)


@functools.lru_cache(maxsize=None)
def decoded_tiles(O, lv):
    """the model's own output for every tile, decoded one at a time: float32 [6,3,64,64] as numpy"""
    from progressivecodec_amd import container, tiles
    net = gpu_codec()
    inner = FT().parse_frame_tiled(encoded(O))["inner"]
    hd = tiles.parse_tiled(inner)
    outs = []
    for t in range(6):
        strings, shape, qs, _, pol = container.unpack(tiles.tile_bytes(inner, hd, t)[0], levels=[lv])
        outs.append(net.decompress(strings[0], shape, qs[0], pol)["x_hat"].cpu().numpy()[0])
    return np.stack(outs)


@pytest.mark.parametrize("O", [0, 16])
def test_the_inner_container_is_pack_tiled_of_every_tile_coded_as_if_alone(O):
    from progressivecodec_amd import container, tiles
    ft = FT()
    net = gpu_codec()
    buf = encoded(O)
    assert isinstance(buf, bytes)
    hd = ft.parse_frame_tiled(buf)
    g = hd["tiled"]["grid"]
    assert (hd["fmt"], hd["matrix"], hd["range"], hd["upsample"], hd["bits"], hd["H"], hd["W"]) == PARAMS + (8, H0, W0)
    assert (g.H, g.W, g.T, g.O, g.ny, g.nx) == (H0, W0, T, O, 2, 3) and hd["tiled"]["magic"] == b"PCT1" and buf[10:] == hd["inner"]
    x, gc = ft.cut_frame(codec_planes(), *PARAMS, tile=T, overlap=O)
    assert gc == g and same_bits(x.cpu().numpy(), GC.cut(codec_frame(H0, W0), *PARAMS, T, O))
    alone = []
    for t in range(6):
        datas = net.compress_levels(x[t:t + 1], QUALITIES, mask_pol=POL)
        alone.append(container.pack([d["strings"] for d in datas], datas[0]["shape"], [float(q) for q in QUALITIES], image_size=(T, T), mask_pol=POL))
        tb, th = tiles.tile_bytes(hd["inner"], hd["tiled"], t)
        assert tb == alone[t] and th["qualities"] == [float(q) for q in QUALITIES] and th["mask_pol"] == POL, t
    assert hd["inner"] == tiles.pack_tiled(alone, H0, W0, T, O)


@pytest.mark.parametrize("O", [0, 16])
def test_decode_frame_tiled_is_the_contracts_stitch_of_the_decoded_tiles(O):
    from progressivecodec_amd import tiles
    ft = FT()
    net = gpu_codec()
    buf = encoded(O)
    for lv in range(len(QUALITIES)):
        x = decoded_tiles(O, lv)
        got = ft.decode_frame_tiled(net, buf, level=lv)
        want = GC.stitch(x, H0, W0, T, O, "nv12", "bt709", "limited")
        assert len(got) == 2 and tuple(got[0].shape) == (H0, W0) and tuple(got[1].shape) == (50, 75, 2)
        assert all(np.array_equal(a.cpu().numpy(), b[0]) for a, b in zip(got, want)), lv
        # the same level in another layout: the NV12 codes re-laid out
        planar = ft.decode_frame_tiled(net, buf, level=lv, fmt="i420")
        relaid = FC.relayout(tuple(p.cpu().numpy()[None] for p in got), "nv12", "i420")
        assert len(planar) == 3 and all(np.array_equal(a.cpu().numpy(), b[0]) for a, b in zip(planar, relaid))
        # and the RGB rendering of the inner container is tiles.decode_tiled's: tiles.stitch of the same decoded tiles
        g = tiles.grid_of(H0, W0, T, O)
        inner = ft.parse_frame_tiled(buf)["inner"]
        assert torch.equal(tiles.decode_tiled(net, inner, level=lv), tiles.stitch(torch.from_numpy(x).to(DEV), g))
    assert all(torch.equal(a, b) for a, b in zip(ft.decode_frame_tiled(net, buf), ft.decode_frame_tiled(net, buf, level=len(QUALITIES) - 1)))
    ten = ft.decode_frame_tiled(net, buf, level=1, fmt="p010")                            # another bit depth: from the decoder's floats
    want = GC.stitch(decoded_tiles(O, 1), H0, W0, T, O, "p010", "bt709", "limited")
    assert ten[0].dtype == torch.uint16 and all(np.array_equal(a.cpu().numpy(), b[0]) for a, b in zip(ten, want))


def test_region_decode_equals_the_crop_and_decodes_the_covering_tiles_only(monkeypatch):
    from progressivecodec_amd import container
    ft = FT()
    net = gpu_codec()
    buf = encoded(16)                                                      # S = 48: bands at rows 48..63, columns 48..63 and 96..111
    whole = ft.decode_frame_tiled(net, buf, level=1)
    calls = []
    real = net.decompress

    def counting(strings, *a, **k):
        calls.append(len(strings[1]))
        return real(strings, *a, **k)
    monkeypatch.setattr(net, "decompress", counting)

    def crop(region):
        y0, x0, h, w = region
        return whole[0][y0:y0 + h, x0:x0 + w], whole[1][y0 // 2:y0 // 2 + -(-h // 2), x0 // 2:x0 // 2 + -(-w // 2)]
    for region, n_tiles in [((4, 6, 20, 30), 1),                           # inside tile (0, 0)
                            ((70, 64, 30, 32), 1),                         # inside tile (1, 1), between its bands
                            ((40, 10, 20, 30), 2),                         # across the horizontal band
                            ((60, 60, 8, 8), 4),                           # across a band corner
                            ((10, 100, 6, 6), 2),                          # inside the second vertical band
                            ((80, 120, 20, 30), 1),                        # touching the frame's corner
                            ((98, 148, 2, 2), 1),
                            ((0, 0, H0, W0), 6)]:
        del calls[:]
        got = ft.decode_frame_tiled(net, buf, level=1, region=region)
        assert all(torch.equal(a, b) for a, b in zip(got, crop(region))), region
        assert sum(calls) == n_tiles and len(calls) == 1, (region, calls)
    del calls[:]
    got = ft.decode_frame_tiled(net, buf, level=1, region=(60, 60, 8, 8), max_tiles_per_call=3, fmt="i420")
    assert calls == [3, 1] and torch.equal(got[0], whole[0][60:68, 60:68]) and torch.equal(got[1], whole[1][30:34, 30:34, 0])
    del calls[:]
    for region in [(5, 6, 20, 30), (4, 6, 21, 30), (4, 6, 20, 31)]:
        with pytest.raises(container.ContainerError, match="admissible"):
            ft.decode_frame_tiled(net, buf, level=1, region=region)
    assert calls == []


def test_max_tiles_per_call_changes_neither_the_bytes_nor_the_planes():
    ft = FT()
    net = gpu_codec()
    buf = encoded(16)
    whole = ft.decode_frame_tiled(net, buf)
    for per_call in (1, 4, 32):
        assert encoded(16, per_call) == buf, per_call
        assert all(torch.equal(a, b) for a, b in zip(ft.decode_frame_tiled(net, buf, max_tiles_per_call=per_call), whole)), per_call


def test_a_one_tile_frame_is_encode_frame_and_decode_frame():
    """a 64 x 64 frame at O = 0: the single tile's PCB1 is the PCB1 inside frames.encode_frame's PCF1, and the planes are decode_frame's"""
    from progressivecodec_amd import frames, tiles
    ft = FT()
    net = gpu_codec()
    planes = codec_planes(64, 64)
    buf = ft.encode_frame_tiled(net, planes, QUALITIES, *PARAMS, tile=T, overlap=0, mask_pol=POL)
    pcf = frames.encode_frame(net, planes, QUALITIES, *PARAMS, mask_pol=POL)
    hd = ft.parse_frame_tiled(buf)
    assert tiles.tile_bytes(hd["inner"], hd["tiled"], 0)[0] == frames.parse_frame(pcf)["blob"]
    for lv in range(len(QUALITIES)):
        assert all(torch.equal(a, b) for a, b in zip(ft.decode_frame_tiled(net, buf, level=lv), frames.decode_frame(net, pcf, level=lv))), lv


def test_a_truncated_container_decodes_the_regions_it_holds():
    from progressivecodec_amd import container
    ft = FT()
    net = gpu_codec()
    buf = encoded(16)
    hd = ft.parse_frame_tiled(buf)["tiled"]
    whole = ft.decode_frame_tiled(net, buf, level=1)
    k = 3
    cut = buf[:10 + hd["table"][k][0] + hd["table"][k][1]]                 # tiles 0 .. 3 are complete, 4 and 5 are gone
    for region in [(4, 6, 20, 30), (0, 0, 48, 150), (70, 10, 30, 30)]:     # tiles {0}, {0, 1, 2}, {3}
        y0, x0, h, w = region
        got = ft.decode_frame_tiled(net, cut, level=1, region=region)
        assert torch.equal(got[0], whole[0][y0:y0 + h, x0:x0 + w]) and torch.equal(got[1], whole[1][y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2]), region
    for region in [(70, 64, 30, 32), None, (60, 60, 8, 8)]:                # tile 4 is needed
        with pytest.raises(container.ContainerError, match="tile 4"):
            ft.decode_frame_tiled(net, cut, level=1, region=region)
    inside = cut[:-5]                                                      # tile 3 is incomplete: regions that need it are refused
    assert torch.equal(ft.decode_frame_tiled(net, inside, level=1, region=(4, 6, 20, 30))[0], whole[0][4:24, 6:36])
    with pytest.raises(container.ContainerError):
        ft.decode_frame_tiled(net, inside, level=1, region=(70, 10, 30, 30))
    with pytest.raises(container.ContainerError, match="no level"):
        ft.decode_frame_tiled(net, buf, level=3)

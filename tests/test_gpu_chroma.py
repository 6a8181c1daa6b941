"""The chroma layer on the GPU (progressivecodec_amd/chroma.py, libpc_chroma.so) against its restatement
(tests/chroma_contract.py): ingest and emit bit for bit and the sums exactly for all twelve formats, three sitings and both upsamplers
on both access paths, the cases read from tests/chroma_cases.py, whose ledger says which of the 24 + 64 kernels each launches;
against `frames` on the device where the two must agree; the halo pixels of the co-sited emit filter; sums past 2^32 in the chroma
planes; the 10-bit words Python does not name; whole 1026 x 1030 pictures of the subsampled formats under co-sited chroma; and
encode_frame / decode_frame through the codec and the PCH1 container.

Sizes: the smallest that take every branch -- a single sample, odd dimensions, partial last items, an odd last row, more than one
block.  Every plane is a view into a larger poisoned allocation (tests/test_gpu_frames.View), so that an element left unwritten, or
one written outside the view, shows."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests import chroma_cases as CS
from tests import chroma_contract as CC
from tests import frames_contract as FC
from tests import pixels_contract as K
from tests.test_gpu_frames import POISON64, View, check_sums, float_planes, same_bits
from tests.util import gpu_codec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POL = "point-based-std"


def CH():
    from progressivecodec_amd import chroma
    return chroma


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def geometry(H, W):
    from progressivecodec_amd.pixels import padding
    return padding(H, W)


def frame_views(fmt, B, H, W, offset=0, mode="tight", data=None):
    """the planes of a frame as Views; `data`: a frame of tests/chroma_contract.py to hold, else poison (a destination)"""
    Hc, Wc = CC.chroma_size(H, W, fmt)
    semi, n = CC.FORMATS[fmt][:2]
    dt = np.uint16 if n == 10 else np.uint8
    shapes = [(B, H, W), (B, Hc, Wc, 2)] if semi else [(B, H, W), (B, Hc, Wc), (B, Hc, Wc)]
    return [View(s, dt, offset, mode, None if data is None else data[i]) for i, s in enumerate(shapes)]


def struct_of(views):
    return CH()._frame_struct([v.t for v in views])


def ingest_raw(views, fmt, matrix, rng, up, siting, B, H, W, Hp, Wp, top, left, dst_offset=0, shift=None):
    """pc_chroma_ingest into a NaN-poisoned buffer with guard floats on both sides -> (status, wide as pc_chroma_plan reports it,
    the [B,3,Hp,Wp] result, whether the guards kept their bits).  shift: instead of the named format's"""
    ch = CH()
    L = ch.lib()
    k, f, (hs, vs) = ch.coefficients(matrix), ch.FORMATS[fmt], ch.SITINGS[siting]
    f = f if shift is None else f._replace(shift=shift)
    n = B * 3 * Hp * Wp
    buf = torch.full((4 + dst_offset + n + 4,), float("nan"), dtype=torch.float32, device=DEV)
    dst = buf[4 + dst_offset:4 + dst_offset + n].view(B, 3, Hp, Wp)
    src = struct_of(views)
    wide = C.c_int(-1)
    assert L.pc_chroma_plan(ch.INGEST, f.layout, f.bits, C.byref(src), dst.data_ptr(), 3 * Hp * Wp, Hp * Wp, Wp, left, None, C.byref(wide)) == 0
    rc = L.pc_chroma_ingest(C.byref(src), *f, hs, vs, ch.RANGES[rng], ch.UPSAMPLES[up], k.a, k.b, k.c, k.d, B, H, W, dst.data_ptr(), Hp, Wp,
                            top, left, stream())
    h = buf.cpu().numpy()
    guards = bool(np.isnan(h[:4 + dst_offset]).all() and np.isnan(h[4 + dst_offset + n:]).all())
    return rc, wide.value, h[4 + dst_offset:4 + dst_offset + n].reshape(B, 3, Hp, Wp), guards


def emit_raw(xv, fmt, matrix, rng, siting, H, W, Hp, Wp, top, left, dst_views, ref_views, shift=None):
    """pc_chroma_emit -> (status, wide, the [B+2,3] sums buffer whose rows 1 .. B are `sse`, poisoned beforehand, the workspace, the
    bytes of workspace the library asked for).  shift: instead of the named format's"""
    ch = CH()
    L = ch.lib()
    k, f, (hs, vs) = ch.coefficients(matrix), ch.FORMATS[fmt], ch.SITINGS[siting]
    f = f if shift is None else f._replace(shift=shift)
    B = xv.shape[0]
    dst = struct_of(dst_views) if dst_views is not None else None
    ref = struct_of(ref_views) if ref_views is not None else None
    need = L.pc_chroma_emit_workspace_size(B, H, W, f.sy)
    ws = torch.full((max(1, need // 8) + 1,), POISON64, dtype=torch.int64, device=DEV)
    sse = torch.full((B + 2, 3), POISON64, dtype=torch.int64, device=DEV)
    wide = C.c_int(-1)
    pd, pr = (C.byref(dst) if dst is not None else None), (C.byref(ref) if ref is not None else None)
    assert L.pc_chroma_plan(ch.EMIT, f.layout, f.bits, pd, xv.data_ptr(), xv.stride(0), xv.stride(1), xv.stride(2), left, pr, C.byref(wide)) == 0
    rc = L.pc_chroma_emit(xv.data_ptr(), xv.stride(0), xv.stride(1), xv.stride(2), Hp, Wp, top, left, B, H, W, *f, hs, vs, ch.RANGES[rng],
                          k.kr, k.kg, k.kb, k.ib, k.ir, pd, pr, ws.data_ptr() if ref is not None else None, need if ref is not None else 0,
                          sse[1:].data_ptr() if ref is not None else None, stream())
    return rc, wide.value, sse.cpu(), ws.cpu(), need


def on_halves(x, fmt, rng, top, left, H, W, seed):
    """x with gray pixels sprinkled over the window whose luma lands on a rounding half, (k + 1/2 - yo) / ys, as nearly as float32
    holds it: the code then turns on the last bit of Y' * ys + yo, so on the order of the operations"""
    g = np.random.default_rng(seed)
    yo, ys, _, _, mx = CC.levels(fmt, rng)
    n = max(1, H * W // 9)
    r, q = g.integers(0, H, n), g.integers(0, W, n)
    v = ((g.integers(yo, yo + ys, n) + 0.5 - yo) / ys).astype(np.float32)
    x[:, :, top + r, left + q] = v[None, None, :]
    return x


def hostile(ref, fmt, matrix, rng, siting, Hp, Wp, top, left, H, W, seed):
    return on_halves(CC.hostile_planes(ref, fmt, matrix, rng, siting, Hp, Wp, top, left, seed), fmt, rng, top, left, H, W, seed)


def check_planes(dstv, want, case):
    for v, w in zip(dstv, want):
        got, clean = v.read()
        assert clean and got.dtype == w.dtype and np.array_equal(got, w), case


# -- the full matrix -----------------------------------------------------------------------------------------------------------------

def run_matrix(cases):
    """the cases of tests/chroma_cases.py at batch 2: the ingest under the case's upsamplers, the emit calls it lists, from views
    that alternate between loose, offset planes with an odd left (narrow) and aligned planes with left a multiple of 8 (wide);
    pc_chroma_plan reports the path the table predicts for every call"""
    L = CH().lib()
    seen = set()
    for c in cases:
        fmt, matrix, rng, siting, H, W, n, left, offset, mode, variant = c[:11]
        g = geometry(H, W)
        assert (g.Hp, g.Wp, g.top, g.left) == K.geometry(H, W)
        narrow = n % 2 == 0
        f = CC.random_frame(2, H, W, fmt, seed=1000 * H + W + n, garbage=True)
        case = (fmt, matrix, rng, siting, H, W, left, mode)
        views = frame_views(fmt, 2, H, W, offset, mode, f)
        assert [v.strides[:2] for v in views] == [CS.view_strides(*rn, mode) for rn in CS.plane_rows(fmt, H, W)]
        for up in c.ups:
            rc, wide, got, guards = ingest_raw(views, fmt, matrix, rng, up, siting, 2, H, W, g.Hp, g.Wp, g.top, left, dst_offset=c.dst_offset)
            assert rc == 0 and guards and wide == int(not narrow) == int(CS.ingest_wide(c)), case
            assert same_bits(got, CC.ingest(f, fmt, matrix, rng, up, siting, g.Hp, g.Wp, g.top, left)), (case, up)
        x = hostile(f, fmt, matrix, rng, siting, g.Hp, g.Wp, g.top, left, H, W, seed=n)
        xv = float_planes(x, variant)
        assert (xv.stride(0), xv.stride(1), xv.stride(2)) == CS.float_strides(g.Hp, g.Wp, variant)[1]
        want = CC.emit(x, g.top, left, H, W, fmt, matrix, rng, siting)
        want_sums = CC.sums(x, g.top, left, H, W, fmt, matrix, rng, siting, f)
        for with_image, with_ref in c.emits:
            dstv = frame_views(fmt, 2, H, W, offset, mode) if with_image else None
            rc, wide, sse, ws, need = emit_raw(xv, fmt, matrix, rng, siting, H, W, g.Hp, g.Wp, g.top, left, dstv, views if with_ref else None)
            assert rc == 0 and wide == int(not narrow) == int(CS.emit_wide(c)), case
            seen.add(wide)
            if with_ref:
                assert need == L.pc_chroma_emit_workspace_size(2, H, W, CC.sub(fmt)[1]) > 0
                check_sums(sse, ws, want_sums, need)
            else:
                assert (sse == POISON64).all() and (ws == POISON64).all(), case
            if with_image:
                check_planes(dstv, want, case)
    assert seen == {0, 1}


@pytest.mark.parametrize("fmt", sorted(CC.FORMATS))
def test_every_format_siting_and_upsampler_is_the_restatement_exactly(fmt):
    run_matrix(CS.every_format_cases(fmt))


@pytest.mark.parametrize("fmt", CS.OTHER_FORMATS)
def test_the_other_matrices_and_full_range(fmt):
    run_matrix(CS.other_matrix_cases(fmt))


# -- agreement with frames on the device ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_centre_sited_420_is_frames_on_the_device(fmt):
    from progressivecodec_amd import frames
    ch = CH()
    for (H, W), (matrix, rng, up) in zip([(37, 53), (64, 64), (67, 130), (1, 1)], itertools.cycle(itertools.product(FC.MATRICES, FC.RANGES, FC.UPSAMPLES))):
        g = geometry(H, W)
        f = FC.random_frame(2, H, W, fmt, seed=H)
        planes = tuple(torch.from_numpy(p).to(DEV) for p in f)
        xa, ga = frames.to_model_input(planes, fmt, matrix, rng, up)
        xb, gb = ch.to_model_input(planes, fmt, matrix, rng, up)                                 # siting defaults to "centre"
        assert ga == gb == g and torch.equal(xa.view(torch.int32), xb.view(torch.int32))
        xt = torch.from_numpy(hostile(f, fmt, matrix, rng, "centre", g.Hp, g.Wp, g.top, g.left, H, W, seed=W)).to(DEV)
        (oa, da), (ob, db) = frames.from_model_output(xt, g, fmt, matrix, rng, ref=planes), ch.from_model_output(xt, g, fmt, matrix, rng, ref=planes)
        assert len(oa) == len(ob) and all(torch.equal(a, b) for a, b in zip(oa, ob)) and torch.equal(da.sse, db.sse)
        assert (da.psnr_y(), da.psnr_cb(), da.psnr_cr()) == (db.psnr_y(), db.psnr_cb(), db.psnr_cr())
        assert torch.equal(ch.from_model_output(xt, g, fmt, matrix, rng, "centre", ref=planes, image=False).sse, da.sse)


def smooth_rgb(H, W, seed):
    """smooth planes (the codec's synthetic weights are not meant for noise; any frame does)"""
    lo = torch.from_numpy(np.random.default_rng(seed).uniform(0.1, 0.9, (1, 3, 8, 8)).astype(np.float32))
    return torch.nn.functional.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False).numpy()


def test_pch1_holds_the_pcb1_blob_of_pcf1_at_centre_sited_nv12():
    from progressivecodec_amd import frames
    ch = CH()
    net = gpu_codec()
    f = FC.emit(smooth_rgb(64, 64, 1), 0, 0, 64, 64, "nv12", "bt709", "limited")
    planes = tuple(torch.from_numpy(p[0]).to(DEV) for p in f)
    a = frames.encode_frame(net, planes, [0, 0.5], "nv12", mask_pol=POL)
    b = ch.encode_frame(net, planes, [0, 0.5], "nv12", mask_pol=POL)
    assert a[:4] == b"PCF1" and b[:4] == b"PCH1" and a[frames.HEADER_BYTES:] == b[ch.HEADER_BYTES:]
    assert all(torch.equal(p, q) for p, q in zip(frames.decode_frame(net, a), ch.decode_frame(net, b)))


# -- wide and narrow -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["nv16", "p210", "i444", "nv24"])
def test_access_paths_agree_on_the_same_data(fmt):
    """one frame under every left in 0 .. 9 and 16, both parities of top, aligned, pitched and offset planes and floats, co-sited
    chroma: wide exactly where pc_chroma_plan's preconditions hold, the restatement's bits everywhere"""
    H, W = 35, 70
    Hp, Wp = 64, 128
    f = CC.random_frame(2, H, W, fmt, seed=H + W)
    seen_in, seen_out = set(), set()
    lefts = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 16]
    for n, (left, top) in enumerate(itertools.product(lefts, [0, 3])):
        siting = ("left", "topleft")[n % 2] if top else ("topleft", "left")[n % 2]
        offset, mode = [(0, "pad4"), (0, "loose"), (2, "pad4")][n % 3] if left % 8 else (0, "pad4")
        dst_offset = int(n % 5 == 4)
        views = frame_views(fmt, 2, H, W, offset, mode, f)
        rc, wide, got, guards = ingest_raw(views, fmt, "bt601", "limited", "linear", siting, 2, H, W, Hp, Wp, top, left, dst_offset)
        case = (fmt, siting, left, top, offset, mode, dst_offset)
        assert rc == 0 and guards, case
        assert wide == int(left % 8 == 0 and offset == 0 and mode == "pad4" and dst_offset == 0), case
        seen_in.add(wide)
        assert same_bits(got, CC.ingest(f, fmt, "bt601", "limited", "linear", siting, Hp, Wp, top, left)), case
        x = hostile(f, fmt, "bt709", "limited", siting, Hp, Wp, top, left, H, W, seed=left)
        want = CC.emit(x, top, left, H, W, fmt, "bt709", "limited", siting)
        want_sums = CC.sums(x, top, left, H, W, fmt, "bt709", "limited", siting, f)
        variant, (doff, dmode), (roff, rmode) = [("contiguous", (0, "pad4"), (0, "pad4")), ("loose4", (0, "pad4"), (0, "pad4")),
                                                 ("odd", (0, "pad4"), (0, "pad4")), ("contiguous", (1, "pad4"), (0, "pad4")),
                                                 ("contiguous", (0, "pad4"), (0, "loose")), ("contiguous", (0, "tight"), (3, "tight"))][n % 6]
        xv = float_planes(x, variant)
        dstv, refv = frame_views(fmt, 2, H, W, doff, dmode), frame_views(fmt, 2, H, W, roff, rmode, f)
        rc, wide, sse, ws, need = emit_raw(xv, fmt, "bt709", "limited", siting, H, W, Hp, Wp, top, left, dstv, refv)
        aligned = lambda vs: all(v.offset == 0 and v.strides[0] % 4 == 0 and v.strides[1] % 4 == 0 for v in vs)      # noqa: E731
        case = (fmt, siting, left, top, variant, doff, dmode, roff, rmode)
        assert rc == 0 and wide == int(left % 4 == 0 and variant != "odd" and aligned(dstv) and aligned(refv)), case
        seen_out.add(wide)
        check_sums(sse, ws, want_sums, need)
        check_planes(dstv, want, case)
    assert seen_in == {0, 1} and seen_out == {0, 1}                                             # pc_chroma_plan reported each path


# -- the halo of the co-sited filter -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["nv12", "i010", "nv16"])
def test_halo_pixels_reach_the_neighbouring_chroma_samples(fmt):
    """Gray planes (u = 0 everywhere) but for one red luma column 8k - 1, the last of an item, or one red luma row 2i - 1, the last of
    a row pair: under co-sited chroma the column is the only non-zero input of chroma column 4k from its left, the row the only one
    of chroma row i from above, and both belong to another item.  W = 70: G = 9 items to a row, the last a partial one of six columns
    whose halo is column 63; block 1 starts at item 256 = row pair 28, item 4.  A halo that is missing, taken from the wrong side or
    clamped where it should not be changes those samples and nothing else."""
    H, W, Hp, Wp, top, left = 64, 70, 64, 128, 0, 8
    sx, sy = CC.sub(fmt)
    cols, rows = [7, 15, 39, 63, 69], [1, 55, 57, 63]
    cases = [("col", c) for c in cols] + ([("row", r) for r in rows] if sy == 2 else []) + [("both", (39, 57))]
    x = np.full((len(cases), 3, Hp, Wp), 0.5, np.float32)
    for b, (kind, at) in enumerate(cases):
        c, r = (at, None) if kind == "col" else (None, at) if kind == "row" else at
        if c is not None:
            x[b, 0, top:top + H, left + c], x[b, 1:, top:top + H, left + c] = 1.0, 0.0
        if r is not None:
            x[b, 0, top + r, left:left + W], x[b, 1:, top + r, left:left + W] = 1.0, 0.0
    flat = CC.emit_codes(np.full((1, 3, Hp, Wp), 0.5, np.float32), top, left, H, W, fmt, "bt709", "limited", "centre")
    ref = CC.frame(*[np.repeat(p, len(cases), axis=0) for p in flat], fmt)
    for siting in ("left", "topleft"):
        want_codes = CC.emit_codes(x, top, left, H, W, fmt, "bt709", "limited", siting)
        for b, (kind, at) in enumerate(cases):                     # the restatement itself: the halo's sample moved, its far neighbour did not
            c, r = (at, None) if kind == "col" else (None, at) if kind == "row" else at
            if kind == "col" and c + 1 < W:
                j = (c + 1) // 2
                assert (want_codes[2][b, :, j] != flat[2][0, :, j]).all() and (want_codes[2][b, :, j + 1] == flat[2][0, :, j + 1]).all()
            if kind == "row" and r + 1 < H and siting == "topleft":
                i = (r + 1) // 2
                assert (want_codes[2][b, i, :] != flat[2][0, i, :]).all() and (want_codes[2][b, i + 1, :] == flat[2][0, i + 1, :]).all()
        want = CC.frame(*want_codes, fmt)
        want_sums = CC.sums(x, top, left, H, W, fmt, "bt709", "limited", siting, ref)
        for variant, mode, offset in [("contiguous", "pad4", 0), ("odd", "loose", 1)]:
            dstv, refv = frame_views(fmt, len(cases), H, W, offset, mode), frame_views(fmt, len(cases), H, W, offset, mode, ref)
            rc, wide, sse, ws, need = emit_raw(float_planes(x, variant), fmt, "bt709", "limited", siting, H, W, Hp, Wp, top, left, dstv, refv)
            assert rc == 0 and wide == int(mode == "pad4")
            check_sums(sse, ws, want_sums, need)
            check_planes(dstv, want, (fmt, siting, variant))


# -- sums past 2^32 in every plane ---------------------------------------------------------------------------------------------------

def test_large_sums_and_the_last_partials_at_444():
    """1026 x 1030 p410 pictures, 518 block partials each (thread t of the final takes t, t + 256, t + 512).  Saturated against a frame
    of zeros, in full range: white for luma, blue for Cb (Cb' = 1/2: 1023.5 rounds past the top code), red for Cr -- one picture
    cannot saturate two planes, since Cb' = 1/2 needs R = G = 0 and Cr' = 1/2 needs G = B = 0 -- so that each plane's sum reaches
    1023^2 * 1026 * 1030 = 1 105 950 916 620, past 2^32, which in a chroma plane no subsampled format comes near.  And a tail-only
    picture: equal to its reference but for the last row, so that only the last partial of the row is non-zero."""
    ch = CH()
    H, W = 1026, 1030
    g = geometry(H, W)
    big = 1023 * 1023 * H * W
    assert big == 1105950916620 > 2 ** 32 and ch.lib().pc_chroma_emit_workspace_size(1, H, W, 1) == 24 * 518
    colours = [(1.0, 1.0, 1.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)]
    x = torch.zeros((4, 3, g.Hp, g.Wp), dtype=torch.float32, device=DEV)
    want = []
    for b, rgb in enumerate(colours):
        for c in range(3):
            x[b, c] = rgb[c]
        codes = CC.emit_codes(np.broadcast_to(np.array(rgb, np.float32)[None, :, None, None], (1, 3, 2, 2)).copy(), 0, 0, 2, 2, "p410", "bt709", "full", "centre")
        want.append([int(p[0, 0, 0]) ** 2 * H * W for p in codes])
        assert want[b][b] == big
    x0 = np.random.default_rng(5).uniform(0.2, 0.8, (1, 3, g.Hp, g.Wp)).astype(np.float32)
    last = CC.emit(x0, g.top, g.left, H, W, "p410", "bt709", "full", "centre")
    eq = CC.ingest(last, "p410", "bt709", "full", "linear", "centre", g.Hp, g.Wp, g.top, g.left)        # 4:4:4: emit(eq) is `last` exactly
    tail = eq.copy()
    tail[:, :, g.top + H - 1, :] = np.where(tail[:, :, g.top + H - 1, :] > 0.5, np.float32(0), np.float32(1))
    x[3] = torch.from_numpy(tail[0]).to(DEV)
    tail_sums = CC.sums(tail[:, :, g.top + H - 2:], 0, g.left, 2, W, "p410", "bt709", "full", "centre", tuple(p[:, H - 2:] for p in last))[0]
    assert all(s > 0 for s in tail_sums)
    want.append(tail_sums)
    ref = tuple(torch.cat([torch.zeros((3,) + p.shape[1:], dtype=torch.uint16), torch.from_numpy(p)]).to(DEV) for p in last)
    out, d = ch.from_model_output(x, g, "p410", "bt709", "full", "topleft", ref=ref)
    assert d.sse.tolist() == want
    assert ch.from_model_output(x, g, "p410", "bt709", "full", ref=ref, image=False).sse.tolist() == want
    again = ch.from_model_output(torch.from_numpy(eq).to(DEV), g, "p410", "bt709", "full", ref=tuple(p[3:] for p in ref))
    assert again[1].sse.tolist() == [[0, 0, 0]] and all(torch.equal(a, r[3:]) for a, r in zip(again[0], ref))
    Y, Cb, Cr = (p.cpu().numpy() for p in (out[0], out[1][..., 0], out[1][..., 1]))
    assert (Y[0] == 1023 << 6).all() and (Cb[1] == 1023 << 6).all() and (Cr[2] == 1023 << 6).all()
    assert d.psnr_y()[0] == d.psnr_cb()[1] == d.psnr_cr()[2] == 0.0


# -- the 10-bit words Python does not name -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("named,shift", CS.UNNAMED)
def test_the_unnamed_10_bit_words_are_the_named_formats_shifted(named, shift):
    """pc_chroma.h admits bits = 10 with shift 0 or 6 in either layout; Python names semi-planar with 6 and planar with 0.  The other
    two through the C calls, both directions, both paths: the floats, the codes and the sums of the named format of the same
    layout; the bits of a word outside the code are ignored on input and zero on output"""
    H, W, siting = 37, 53, "left"
    g = geometry(H, W)
    assert {CC.FORMATS[named][2], shift} == {0, 6}
    f = CC.random_frame(2, H, W, named, seed=shift + 1)
    noise = np.random.default_rng(shift).integers(0, 2 ** 16, 10 ** 5).astype(np.uint16)
    words = CS.reshifted(f, named, shift, noise)
    assert all((w != CS.reshifted(f, named, shift)[i]).any() for i, w in enumerate(words))
    for n in (0, 1):
        left, offset, mode, variant, dst_offset = CS.layout_of(n, H, W)
        views = frame_views(named, 2, H, W, offset, mode, words)
        for up in CC.UPSAMPLES:
            rc, wide, got, guards = ingest_raw(views, named, "bt709", "limited", up, siting, 2, H, W, g.Hp, g.Wp, g.top, left, dst_offset, shift=shift)
            assert rc == 0 and guards and wide == n, (named, shift, n, up)
            assert same_bits(got, CC.ingest(f, named, "bt709", "limited", up, siting, g.Hp, g.Wp, g.top, left)), (named, shift, n, up)
        x = hostile(f, named, "bt709", "limited", siting, g.Hp, g.Wp, g.top, left, H, W, seed=n)
        want = CS.reshifted(CC.emit(x, g.top, left, H, W, named, "bt709", "limited", siting), named, shift)
        assert all((p & ~np.uint16(1023 << shift) == 0).all() for p in want)
        want_sums = CC.sums(x, g.top, left, H, W, named, "bt709", "limited", siting, f)
        dstv = frame_views(named, 2, H, W, offset, mode)
        rc, wide, sse, ws, need = emit_raw(float_planes(x, variant), named, "bt709", "limited", siting, H, W, g.Hp, g.Wp, g.top, left, dstv, views, shift=shift)
        assert rc == 0 and wide == n, (named, shift, n)
        check_sums(sse, ws, want_sums, need)
        check_planes(dstv, want, (named, shift, n))


# -- whole pictures: more than 256 block partials per picture in the subsampled and co-sited formats ----------------------------------------

WHOLE_IDS = [f"{fmt}-{siting}" for fmt, siting in CS.WHOLE_FORMATS]


@pytest.mark.parametrize("kind", ["hostile", "saturated", "tail"])
@pytest.mark.parametrize("fmt,siting", CS.WHOLE_FORMATS, ids=WHOLE_IDS)
def test_whole_pictures_planes_and_sums(fmt, siting, kind):
    """1026 x 1030: 259 block partials per picture at 4:2:0 and 518 at 4:2:2, so that thread t of emit_final takes t, t + 256 (and
    t + 512).  Hostile data with gray pixels on the rounding halves; white, blue and red pictures in full range against a frame of
    zeros, whose plane p of picture p is top^2 times the plane's samples, past 2^32 in chroma too; and a picture that differs from
    its reference in the last luma row alone, so that only the last partials are non-zero.  Image and sums on the wide path into
    poisoned views, then the sums alone on the narrow path"""
    H, W = CS.WHOLE["H"], CS.WHOLE["W"]
    g = geometry(H, W)
    left = g.left // 4 * 4
    assert (g.Hp, g.Wp) == (1088, 1088) and left % 4 == 0 and left + W <= g.Wp
    matrix, rng = ("bt709", "full") if kind == "saturated" else ("bt601", "limited")
    if kind == "hostile":
        ref = CC.random_frame(CS.WHOLE["B"], H, W, fmt, seed=21, garbage=True)
        x = hostile(ref, fmt, matrix, rng, siting, g.Hp, g.Wp, g.top, left, H, W, seed=22)
    elif kind == "saturated":
        x, ref, closed = CS.whole_saturated(fmt, g.Hp, g.Wp)
    else:
        x, ref = CS.whole_tail(fmt, siting, matrix, rng, g.Hp, g.Wp, g.top, left)
    B = x.shape[0]
    want = CC.emit(x, g.top, left, H, W, fmt, matrix, rng, siting)
    want_sums = CC.sums(x, g.top, left, H, W, fmt, matrix, rng, siting, ref)
    if kind == "saturated":
        assert [want_sums[p][p] for p in range(3)] == closed and min(closed) > 2 ** 32
    if kind == "tail":
        assert want_sums[0] == [0, 0, 0] and all(v > 0 for v in want_sums[1])
    sy = CC.sub(fmt)[1]
    nbytes = 24 * (259 if sy == 2 else 518) * B
    refv, dstv = frame_views(fmt, B, H, W, 0, "pad4", ref), frame_views(fmt, B, H, W, 0, "pad4")
    rc, wide, sse, ws, need = emit_raw(float_planes(x, "contiguous"), fmt, matrix, rng, siting, H, W, g.Hp, g.Wp, g.top, left, dstv, refv)
    assert rc == 0 and wide == 1 and need == nbytes == CH().lib().pc_chroma_emit_workspace_size(B, H, W, sy)
    check_sums(sse, ws, want_sums, need)
    check_planes(dstv, want, (fmt, siting, kind))
    del dstv
    loose = frame_views(fmt, B, H, W, 1, "loose", ref)
    rc, wide, sse, ws, need = emit_raw(float_planes(x, "odd"), fmt, matrix, rng, siting, H, W, g.Hp, g.Wp, g.top, left, None, loose)
    assert rc == 0 and wide == 0 and need == nbytes
    check_sums(sse, ws, want_sums, need)                                   # image=False: the same sums


@pytest.mark.parametrize("fmt,siting", CS.WHOLE_FORMATS, ids=WHOLE_IDS)
def test_whole_pictures_ingest(fmt, siting):
    """the ingest of the same frames: 578 blocks per picture at Hp = Wp = 1088; linear on the wide path, nearest on the narrow one"""
    H, W, B = CS.WHOLE["H"], CS.WHOLE["W"], CS.WHOLE["B"]
    g = geometry(H, W)
    assert g.Hp * (g.Wp // 8) == 578 * 256
    f = CC.random_frame(B, H, W, fmt, seed=21, garbage=True)
    for up, (left, offset, mode, dst_offset) in zip(("linear", "nearest"), [(g.left // 8 * 8, 0, "pad4", 0), (g.left, 1, "loose", 1)]):
        views = frame_views(fmt, B, H, W, offset, mode, f)
        rc, wide, got, guards = ingest_raw(views, fmt, "bt601", "limited", up, siting, B, H, W, g.Hp, g.Wp, g.top, left, dst_offset)
        assert rc == 0 and guards and wide == int(up == "linear"), (fmt, up)
        assert same_bits(got, CC.ingest(f, fmt, "bt601", "limited", up, siting, g.Hp, g.Wp, g.top, left)), (fmt, up)


# -- through the codec ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,siting,hw", [("p210", "left", (64, 96)), ("i444", "centre", (64, 64))])
def test_encode_frame_and_decode_frame_through_the_codec(fmt, siting, hw):
    from progressivecodec_amd import container
    ch = CH()
    net = gpu_codec()
    H, W = hw
    qualities = [0, 0.5]
    f = CC.emit(smooth_rgb(H, W, H + W), 0, 0, H, W, fmt, "bt709", "limited", siting)
    planes = tuple(torch.from_numpy(p[0]).to(DEV) for p in f)
    buf = ch.encode_frame(net, planes, qualities, fmt, "bt709", "limited", "linear", siting, mask_pol=POL)
    assert isinstance(buf, bytes)
    hd = ch.parse_frame(buf)
    assert (hd["fmt"], hd["siting"], hd["matrix"], hd["range"], hd["upsample"], hd["bits"], hd["H"], hd["W"]) == \
        (fmt, siting, "bt709", "limited", "linear", CC.bits(fmt), H, W)
    g = geometry(H, W)
    x, geom = ch.to_model_input(planes, fmt, "bt709", "limited", "linear", siting)
    assert geom == g and same_bits(x.cpu().numpy(), CC.ingest(f, fmt, "bt709", "limited", "linear", siting, g.Hp, g.Wp, g.top, g.left))
    datas = net.compress_levels(x, qualities, mask_pol=POL)
    strings = container.unpack(hd["blob"])[0]
    for lv, (q, d) in enumerate(zip(qualities, datas)):
        ys, zs = d["strings"]
        assert strings[lv] == [[[bytes(s[0])] for s in ys], [bytes(zs[0])]]
        x_hat = net.decompress(d["strings"], d["shape"], q, POL)["x_hat"]
        got = ch.decode_frame(net, buf, level=lv)
        want = CC.emit(x_hat.cpu().numpy(), g.top, g.left, H, W, fmt, "bt709", "limited", siting)
        assert len(got) == len(want) and all(tuple(a.shape) == b.shape[1:] and np.array_equal(a.cpu().numpy(), b[0]) for a, b in zip(got, want))
        if fmt == "p210":                                         # a 4:2:2 master straight to left-sited NV12, and to another siting
            nv12 = ch.decode_frame(net, buf, level=lv, fmt="nv12", siting="left")
            assert all(torch.equal(a, b[0]) for a, b in zip(nv12, ch.from_model_output(x_hat, g, "nv12", "bt709", "limited", "left")))
            assert all(np.array_equal(a.cpu().numpy(), b[0]) for a, b in
                       zip(nv12, CC.emit(x_hat.cpu().numpy(), g.top, g.left, H, W, "nv12", "bt709", "limited", "left")))
            other = ch.decode_frame(net, buf, level=lv, siting="centre")
            assert all(torch.equal(a, b[0]) for a, b in zip(other, ch.from_model_output(x_hat, g, "p210", "bt709", "limited", "centre")))
    assert all(torch.equal(a, b) for a, b in zip(ch.decode_frame(net, buf), ch.decode_frame(net, buf, level=len(qualities) - 1)))

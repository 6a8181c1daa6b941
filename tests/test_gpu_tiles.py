"""Tiled image coding on the GPU (progressivecodec_amd/tiles.py, libpc_tiles.so) against its numpy restatement
(tests/tiles_contract.py): cut and stitch bit for bit on both access paths, the distortion sums, and encode_tiled / decode_tiled
through the codec and the PCT1 container.  T = 64 throughout: the smallest tile, so that the images stay small while every branch
(one tile, several tiles, partial last tiles, bands of every allowed kind) is taken."""
import functools

import numpy as np
import pytest
import torch

from tests import pixels_contract as K
from tests import tiles_contract as TC
from tests.util import gpu_codec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POL = "point-based-std"
T = 64
SIZES = [(1, 1), (64, 64), (65, 63), (100, 150), (127, 129)]
OVERLAPS = [0, 4, 16, 32]
POISON = 0xA5


def TL():
    from progressivecodec_amd import tiles
    return tiles


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def view_args(t, layout):
    """(pointer, layout, plane, row stride) of a 3-D uint8 tensor view; None: no view"""
    if t is None:
        return (None, 0, 0, 0)
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


def bits_equal(t, want_np):
    w = torch.from_numpy(np.ascontiguousarray(want_np).view(np.int32)).to(t.device)
    return torch.equal(t.contiguous().view(torch.int32), w.view(t.shape))


# -- cut -----------------------------------------------------------------------------------------------------------------------------

def cut_raw(L, src, layout, H, W, O, rect, dst):
    return L.pc_tiles_cut_u8(*view_args(src, layout), H, W, T, O, *rect, dst.data_ptr(), stream())


@pytest.mark.parametrize("hw", SIZES)
def test_cut_matrix_bitwise_on_both_paths(hw):
    tiles = TL()
    L = tiles.lib()
    H, W = hw
    chw = image(H, W)
    seen = {"hwc": set(), "chw": set()}
    for O in OVERLAPS:
        ny, nx = TC.grid(H, W, T, O)
        g = tiles.grid_of(H, W, T, O)
        assert (g.ny, g.nx) == (ny, nx)
        want = TC.cut(chw, "chw", T, O)
        rects = [(0, 0, ny, nx)] + ([(ny - 1, 1, 1, nx - 1)] if nx > 1 else []) + ([(1, 0, ny - 1, 1)] if ny > 1 else [])
        for layout in ("hwc", "chw"):
            arr = in_layout(chw, layout)
            for offset, loose, pad4 in [(0, False, False), (0, False, True), (0, True, False), (1, False, True), (2, False, True), (3, False, True)]:
                src = u8_tensor(arr, layout, offset, loose, pad4)
                for rect in rects:
                    n = rect[2] * rect[3]
                    dst = torch.full((n, 3, T, T), float("nan"), dtype=torch.float32, device=DEV)       # poison: every element is written
                    wide = tiles.plan(tiles.CUT, src, layout, dst)
                    seen[layout].add(wide)
                    # by construction: strides that are multiples of 4 at an allocation start are wide, a 1..3-byte offset or a loose
                    # stride never is; a contiguous image is wide when 4 | W (then 4 | 3 W and 4 | H W)
                    expect = False if offset or loose else True if pad4 else W % 4 == 0
                    assert wide is expect, (layout, offset, loose, pad4)
                    assert cut_raw(L, src, layout, H, W, O, rect, dst) == 0
                    w_rect = want if rect == rects[0] else TC.cut(chw, "chw", T, O, rect)
                    case = (H, W, O, layout, offset, loose, pad4, rect, wide)
                    assert bits_equal(dst, w_rect), case
                if offset == 0 and not loose:                                                      # the Python call, same bits
                    x, gg = tiles.cut(src, T, O, layout)
                    assert gg == g and bits_equal(x, want)
                    if len(rects) > 1:
                        x, gg = tiles.cut(src, T, O, layout, rect=rects[1])
                        assert gg.rect == rects[1] and bits_equal(x, TC.cut(chw, "chw", T, O, rects[1]))
        beyond = torch.from_numpy(TC.cut(np.full((3, H, W), 255, np.uint8), "chw", T, O) == 0).to(DEV)
        x, _ = tiles.cut(torch.from_numpy(chw).to(DEV), T, O, "chw")
        assert (x.view(torch.int32)[beyond] == 0).all()                                             # +0.0 beyond the image, not -0.0
    assert seen == {"hwc": {True, False}, "chw": {True, False}}


def test_cut_copies_views_it_cannot_address():
    tiles = TL()
    chw = image(70, 90)
    t = torch.from_numpy(np.array(chw)).to(DEV)
    x, g = tiles.cut(t.permute(1, 2, 0), T, 16, "hwc")                                              # channel stride 70*90, not 1
    assert (g.ny, g.nx) == (2, 2) and bits_equal(x, TC.cut(chw, "chw", T, 16))
    x, _ = tiles.cut(t.flip(2), T, 0, "chw")
    assert bits_equal(x, TC.cut(chw[:, :, ::-1], "chw", T, 0))


# -- stitch --------------------------------------------------------------------------------------------------------------------------

def windows(H, W, O):
    S = T - O
    out = [(0, 0, H, W), (0, 0, 1, 1), (H - 1, W - 1, 1, 1)]
    if H >= 30 and W >= 20:
        out.append((5, 6, 20, 9))                                        # inside one tile, first column no multiple of 4
    if H > T and W <= T:
        out.append((H - 6, 1, 6, W - 2))
    if H > T and W > T:
        B = max(O, 4)
        out += [(S + 1, S + 2, 5, 7),                                    # starts inside the band (O >= 16) or just past it
                (S, S, B, B),                                            # the band exactly: on both of its edges
                (3, 5, S - 3, S - 5),                                    # ends on the pixel before the band
                (S - 2, S - 1, O + 4, O + 2),                            # starts before the band, ends after it
                (S + O, S + O, H - S - O, W - S - O),                    # starts on the pixel after the band
                (10, 3, H - 20, W - 7)]                                  # several tiles each way
    return out


def float_tiles(x_np, variant):
    """x_np [n,3,T,T] on the device: contiguous; "loose4": rows, planes and tiles apart, every 16-byte alignment kept; "odd": apart and
    one float past an allocation start, so that no row is 16-byte aligned"""
    t = torch.from_numpy(x_np).to(DEV)
    if variant == "contiguous":
        return t
    n, T = x_np.shape[0], x_np.shape[3]
    sh, off = (T + 4, 0) if variant == "loose4" else (T + 1, 1)
    sc = T * sh + (8 if variant == "loose4" else 3)
    st = 3 * sc + (4 if variant == "loose4" else 2)
    buf = torch.full((off + n * st + 8,), float("nan"), dtype=torch.float32, device=DEV)
    v = torch.as_strided(buf, x_np.shape, (st, sc, sh, 1), storage_offset=off)
    v.copy_(t)
    return v


def poisoned_destination(h, w, layout, x0, aligned):
    """(buffer, view): an h x w view inside a poisoned buffer, one row down; its first byte sits where the wide path wants image column
    4 * (x0 / 4) 4-byte aligned (aligned) or one pixel further (not)"""
    c0 = 4 + x0 % 4 + (0 if aligned else 1)
    wp = up4(w + 12)
    if layout == "hwc":
        buf = torch.full((h + 2, wp, 3), POISON, dtype=torch.uint8, device=DEV)                      # row stride 3 * wp, a multiple of 4
        return buf, buf[1:h + 1, c0:c0 + w, :]
    buf = torch.full((3, up4(h + 2), wp), POISON, dtype=torch.uint8, device=DEV)
    return buf, buf[:, 1:h + 1, c0:c0 + w]


def window_of(t, layout, win):
    y0, x0, h, w = win
    return t[y0:y0 + h, x0:x0 + w, :] if layout == "hwc" else t[:, y0:y0 + h, x0:x0 + w]


def stitch_raw(L, x, H, W, O, rect, win, rounding, dst, dst_layout, ref, ref_layout, T=T):
    y0, x0, h, w = win
    sums = torch.full((2, 3), -1, dtype=torch.int64, device=DEV)
    nbytes = L.pc_tiles_stitch_workspace_size(x0, h, w)
    ws = torch.empty(max(1, nbytes // 8), dtype=torch.int64, device=DEV)
    rc = L.pc_tiles_stitch_u8(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), H, W, T, O, *rect, y0, x0, h, w, rounding,
                              *view_args(dst, dst_layout), *view_args(ref, ref_layout), ws.data_ptr(), nbytes, sums[0].data_ptr(),
                              sums[1].data_ptr(), stream())
    return rc, sums


@pytest.mark.parametrize("hw", SIZES)
def test_stitch_matrix_bitwise_sums_and_untouched_surroundings(hw):
    tiles = TL()
    L = tiles.lib()
    H, W = hw
    ref_chw = image(H, W, seed=7)
    seen = set()
    for O in OVERLAPS:
        ny, nx = TC.grid(H, W, T, O)
        rect = (0, 0, ny, nx)
        x_np = TC.hostile_tiles(ny * nx, T, seed=H + W + O)
        xs = {v: float_tiles(x_np, v) for v in ("contiguous", "loose4", "odd")}
        refs = {(lay, al): u8_tensor(in_layout(ref_chw, lay), lay, 0 if al else 1, pad4=True) for lay in ("hwc", "chw") for al in (True, False)}
        for win in windows(H, W, O):
            y0, x0, h, w = win
            for rounding in ("nearest", "trunc"):
                want = TC.stitch(x_np, H, W, T, O, rounding, "chw", window=win)
                su, sf = TC.sums(x_np, H, W, T, O, rounding, ref_chw, "chw", window=win)
                sse_f_bits = None
                # (tiles, destination and reference aligned?) -> the path by construction
                for variant, aligned, ref_aligned, dst_layout, ref_layout in [("contiguous", True, True, "hwc", "chw"),
                                                                               ("loose4", True, True, "chw", "hwc"),
                                                                               ("odd", True, True, "hwc", "hwc"),
                                                                               ("contiguous", False, True, "chw", "chw"),
                                                                               ("contiguous", True, False, "hwc", "chw")]:
                    x = xs[variant]
                    ref = window_of(refs[(ref_layout, ref_aligned)], ref_layout, win)
                    buf, dst = poisoned_destination(h, w, dst_layout, x0, aligned)
                    wide = tiles.plan(tiles.STITCH, dst, dst_layout, x, x0, ref, ref_layout)
                    assert wide is (variant != "odd" and aligned and ref_aligned), (win, variant, aligned, ref_aligned)
                    seen.add(wide)
                    rc, sums = stitch_raw(L, x, H, W, O, rect, win, tiles.ROUNDINGS[rounding], dst, dst_layout, ref, ref_layout)
                    case = (H, W, O, win, rounding, variant, aligned, ref_aligned, dst_layout, ref_layout)
                    assert rc == 0, case
                    assert torch.equal(dst, torch.from_numpy(in_layout(want, dst_layout)).to(DEV)), case
                    dst.fill_(POISON)
                    assert (buf == POISON).all(), case                                  # nothing outside the window was written
                    hs = sums.cpu()
                    assert hs[0].tolist() == su, case
                    got_f = hs[1].view(torch.float64)
                    for c in range(3):
                        assert abs(got_f[c].item() - sf[c]) <= h * w * 2.0 ** -53 * sf[c], case
                    if sse_f_bits is None:
                        sse_f_bits = hs[1].clone()
                    assert torch.equal(hs[1], sse_f_bits), case                          # the same bits on both paths and in every layout
                if rounding == "nearest":
                    # the Python call; the sums alone; a second stream; the same window from the smallest rectangle that holds it
                    rt = torch.from_numpy(np.array(ref_chw)).to(DEV)
                    g = tiles.grid_of(H, W, T, O)
                    out, d = tiles.stitch(xs["contiguous"], g, win, "chw", ref=rt)
                    assert torch.equal(out.cpu(), torch.from_numpy(want)) and d.sse_u8.tolist() == [su]
                    assert torch.equal(d.sse_f.view(torch.int64).cpu()[0], sse_f_bits)
                    assert d.psnr() == [K.psnr(d.sse_f.tolist()[0], h, w)] and d.psnr_8bit() == [K.psnr_8bit(su, h, w)]
                    only = tiles.stitch(xs["odd"], g, win, ref=rt, ref_layout="chw", image=False)
                    assert torch.equal(only.sse_f.view(torch.int64).cpu()[0], sse_f_bits) and only.sse_u8.tolist() == [su]
                    side = torch.cuda.Stream(DEV)
                    side.wait_stream(torch.cuda.current_stream(DEV))
                    with torch.cuda.stream(side):
                        out_s, d_s = tiles.stitch(xs["contiguous"], g, win, "chw", ref=rt)
                    side.synchronize()
                    assert torch.equal(out_s, out) and torch.equal(d_s.sse_f.view(torch.int64).cpu()[0], sse_f_bits)
                    small = g.with_rect(g.covering(win))
                    if small.rect != g.rect:
                        idx = [(small.ty0 + a) * nx + small.tx0 + b for a in range(small.nty) for b in range(small.ntx)]
                        out_r, d_r = tiles.stitch(xs["contiguous"][idx], small, win, "chw", ref=rt)
                        assert torch.equal(out_r, out) and torch.equal(d_r.sse_f.view(torch.int64).cpu()[0], sse_f_bits)
                        assert d_r.sse_u8.tolist() == [su]
        full = tiles.stitch(xs["contiguous"], tiles.grid_of(H, W, T, O), layout="hwc", rounding="trunc")
        assert torch.equal(full.cpu(), torch.from_numpy(TC.stitch(x_np, H, W, T, O, "trunc", "hwc")))
    assert seen == {True, False}


def test_without_overlap_the_stitch_is_from_model_output_of_every_tile_pasted_together():
    from progressivecodec_amd import pixels
    tiles = TL()
    H, W = 100, 150
    x_np = TC.hostile_tiles(6, T, seed=77)
    x = torch.from_numpy(x_np).to(DEV)
    g = tiles.grid_of(H, W, T, 0)
    for rounding in ("nearest", "trunc"):
        per_tile = pixels.from_model_output(x, pixels.Geometry(T, T, T, T, 0, 0), "chw", rounding=rounding)     # [6,3,64,64]
        pasted = per_tile.view(2, 3, 3, T, T).permute(2, 0, 3, 1, 4).reshape(3, 2 * T, 3 * T)[:, :H, :W]
        assert torch.equal(tiles.stitch(x, g, layout="chw", rounding=rounding), pasted)
        assert torch.equal(tiles.stitch(x, g, (30, 61, 50, 70), layout="hwc", rounding=rounding), pasted[:, 30:80, 61:131].permute(1, 2, 0))


def test_a_cut_image_stitches_back_to_itself():
    tiles = TL()
    img = torch.from_numpy(in_layout(np.array(image(127, 129)), "hwc")).to(DEV)
    for O in OVERLAPS:
        x, g = tiles.cut(img, T, O)
        out, d = tiles.stitch(x, g, ref=img)
        assert torch.equal(out, img) and d.sse_u8.tolist() == [[0, 0, 0]]
        assert max(d.sse_f.tolist()[0]) <= 127 * 129 * 2.0 ** -42                          # |m - v| < 2^-21 (tests/test_tiles_host.py)
        down = tiles.stitch(x, g, rounding="trunc")
        diff = img.int() - down.int()
        assert diff.min() >= 0 and diff.max() <= (0 if O == 0 else 1)


def test_refused_calls_launch_nothing():
    tiles = TL()
    L = tiles.lib()
    H, W, O = 100, 150, 16
    src = u8_tensor(np.array(image(H, W)), "chw")
    dst = torch.full((6, 3, T, T), 7.0, dtype=torch.float32, device=DEV)
    for rect in [(0, 0, 3, 3), (0, 0, 2, 4), (1, 0, 2, 3), (0, 0, 0, 3)]:
        assert cut_raw(L, src, "chw", H, W, O, rect, dst) == -1
    assert L.pc_tiles_cut_u8(*view_args(src, "chw"), H, W, T, 6, 0, 0, 2, 3, dst.data_ptr(), stream()) == -1
    x = torch.rand(6, 3, T, T, device=DEV)
    out = torch.full((3, H, W), POISON, dtype=torch.uint8, device=DEV)
    for rect, win in [((0, 0, 1, 3), (0, 0, 49, 150)), ((0, 1, 2, 2), (0, 63, 100, 87)), ((0, 0, 2, 3), (0, 0, 101, 150)), ((0, 0, 2, 3), (0, 0, 100, 0))]:
        rc, sums = stitch_raw(L, x, H, W, O, rect, win, 0, window_of(out, "chw", (0, 0, max(1, min(win[2], H)), max(1, win[3]))), "chw", src, "chw")
        assert rc == -1 and (sums == -1).all()
    torch.cuda.synchronize()
    assert (dst == 7.0).all() and (out == POISON).all()
    with pytest.raises(tiles.TilesError, match="PC_ERR_ARG"):
        raise tiles.TilesError(-1, "pc_tiles_stitch_u8")
    rc, sums = stitch_raw(L, x, H, W, O, (0, 0, 2, 3), (0, 0, H, W), 0, out, "chw", src, "chw")     # the same call, unspoilt, goes through
    torch.cuda.synchronize()
    assert rc == 0 and (out != POISON).any() and (sums != -1).all()


def test_offsets_past_2_to_the_31():
    """a small image and its two tiles as views whose plane and tile strides pass 2^31 bytes, inside one untouched allocation: every
    offset is 64-bit"""
    tiles = TL()
    L = tiles.lib()
    BIG = 2 ** 31 + 4096                                                   # plane / tile stride in bytes
    need = 2 * BIG + (16 << 20)
    free = torch.cuda.mem_get_info(DEV)[0]
    if free < need + (1 << 30):
        pytest.skip(f"{free >> 20} MiB of device memory free, the strided views need {need >> 20} MiB")
    buf = torch.empty(need, dtype=torch.uint8, device=DEV)
    H, W, O = 40, 100, 0                                                   # 1 x 2 tiles
    chw = image(H, W, seed=31)
    src = torch.as_strided(buf, (3, H, W), (BIG, W, 1), 0)
    src.copy_(torch.from_numpy(chw))
    x, g = tiles.cut(src, T, O, "chw")
    assert bits_equal(x, TC.cut(chw, "chw", T, O))
    x_np = TC.hostile_tiles(2, T, seed=32)
    xv = torch.as_strided(buf.view(torch.float32), (2, 3, T, T), (BIG // 4, T * T, T, 1), (1 << 20) // 4)
    xv.copy_(torch.from_numpy(x_np))
    dst = torch.as_strided(buf, (3, H, W), (BIG, W, 1), 2 << 20)
    rc, sums = stitch_raw(L, xv, H, W, O, (0, 0, 1, 2), (0, 0, H, W), 0, dst, "chw", src, "chw")
    assert rc == 0
    assert torch.equal(dst.cpu(), torch.from_numpy(TC.stitch(x_np, H, W, T, O, "nearest", "chw")))
    su, sf = TC.sums(x_np, H, W, T, O, "nearest", chw, "chw")
    hs = sums.cpu()
    assert hs[0].tolist() == su
    for c in range(3):
        assert abs(hs[1].view(torch.float64)[c].item() - sf[c]) <= H * W * 2.0 ** -53 * sf[c]
    out, d = tiles.stitch(xv, g, layout="chw", ref=src)
    assert torch.equal(out, dst) and torch.equal(d.sse_f.view(torch.int64)[0], sums[1])


# -- through the codec ---------------------------------------------------------------------------------------------------------------

QUALITIES = [0, 0.5, 10]
H0, W0 = 100, 150                                                          # 2 x 3 tiles of 64 x 64, with and without overlap


def codec_image():
    return torch.from_numpy(in_layout(np.array(image(H0, W0, seed=21)), "hwc")).to(DEV)             # [100,150,3]


@functools.lru_cache(maxsize=None)
def encoded(O, per_call=32):
    return TL().encode_tiled(gpu_codec(), codec_image(), QUALITIES, tile=T, overlap=O, mask_pol=POL, max_tiles_per_call=per_call)


def crop(img, i, j, S):
    """the zero-extended 64 x 64 crop of tile (i, j)"""
    out = torch.zeros((T, T, 3), dtype=torch.uint8, device=DEV)
    part = img[i * S:i * S + T, j * S:j * S + T]
    out[:part.shape[0], :part.shape[1]] = part
    return out


@pytest.mark.parametrize("O", [0, 16])
def test_every_tile_is_coded_as_if_alone(O):
    from progressivecodec_amd import container, pixels
    tiles = TL()
    net = gpu_codec()
    buf = encoded(O)
    assert isinstance(buf, bytes)
    hd = tiles.parse_tiled(buf)
    g = hd["grid"]
    assert (g.H, g.W, g.T, g.O, g.ny, g.nx) == (H0, W0, T, O, 2, 3) and hd["contract"] == container.build_contract_id()
    img = codec_image()
    for i in range(2):
        for j in range(3):
            tb, th = tiles.tile_bytes(buf, hd, i * 3 + j)
            assert tb == pixels.encode_image(net, crop(img, i, j, T - O), QUALITIES, mask_pol=POL), (i, j)
            assert th["image_size"] == (T, T) and th["qualities"] == [float(q) for q in QUALITIES] and th["mask_pol"] == POL


def test_without_overlap_decode_tiled_is_decode_image_of_every_tile_pasted_together():
    from progressivecodec_amd import pixels
    tiles = TL()
    net = gpu_codec()
    buf = encoded(0)
    hd = tiles.parse_tiled(buf)
    for lv, rounding in [(0, "nearest"), (1, "trunc"), (-1, "nearest")]:
        want = torch.zeros((2 * T, 3 * T, 3), dtype=torch.uint8, device=DEV)
        for t in range(6):
            want[(t // 3) * T:(t // 3 + 1) * T, (t % 3) * T:(t % 3 + 1) * T] = pixels.decode_image(net, tiles.tile_bytes(buf, hd, t)[0], level=lv, rounding=rounding)
        assert torch.equal(tiles.decode_tiled(net, buf, level=lv, rounding=rounding), want[:H0, :W0])
    assert torch.equal(tiles.decode_tiled(net, buf, layout="chw"), want[:H0, :W0].permute(2, 0, 1))


def decoded_tiles(net, buf, lv):
    """the model's own output for every tile, decoded one at a time: float32 [6,3,64,64] as numpy"""
    from progressivecodec_amd import container
    tiles = TL()
    hd = tiles.parse_tiled(buf)
    outs = []
    for t in range(6):
        strings, shape, qs, _, pol = container.unpack(tiles.tile_bytes(buf, hd, t)[0], levels=[lv])
        outs.append(net.decompress(strings[0], shape, qs[0], pol)["x_hat"].cpu().numpy()[0])
    return np.stack(outs)


def test_with_overlap_decode_tiled_is_the_contracts_stitch_of_the_decoded_tiles():
    tiles = TL()
    net = gpu_codec()
    buf = encoded(16)
    for lv in (0, 2):
        x = decoded_tiles(net, buf, lv)
        for rounding in ("nearest", "trunc"):
            got = tiles.decode_tiled(net, buf, level=lv, rounding=rounding)
            assert np.array_equal(got.cpu().numpy(), TC.stitch(x, H0, W0, T, 16, rounding, "hwc")), (lv, rounding)


def test_region_decode_equals_the_crop_and_decodes_the_covering_tiles_only(monkeypatch):
    tiles = TL()
    net = gpu_codec()
    buf = encoded(16)                                                      # S = 48: bands at rows 48..63, columns 48..63 and 96..111
    whole = tiles.decode_tiled(net, buf, level=1)
    calls = []
    real = net.decompress

    def counting(strings, *a, **k):
        calls.append(len(strings[1]))
        return real(strings, *a, **k)
    monkeypatch.setattr(net, "decompress", counting)
    for region, n_tiles in [((5, 6, 20, 30), 1),                           # inside tile (0, 0)
                            ((70, 64, 30, 32), 1),                         # inside tile (1, 1), between its bands
                            ((40, 10, 20, 30), 2),                         # across the horizontal band
                            ((60, 60, 8, 8), 4),                           # across a band corner
                            ((10, 100, 5, 5), 2),                          # inside the second vertical band
                            ((80, 120, 20, 30), 1),                        # touching the image's corner
                            ((0, 0, H0, W0), 6)]:
        y0, x0, h, w = region
        del calls[:]
        got = tiles.decode_tiled(net, buf, level=1, region=region)
        assert torch.equal(got, whole[y0:y0 + h, x0:x0 + w]), region
        assert sum(calls) == n_tiles and len(calls) == 1, (region, calls)
    del calls[:]
    got = tiles.decode_tiled(net, buf, level=1, region=(60, 60, 8, 8), max_tiles_per_call=3, layout="chw")
    assert calls == [3, 1] and torch.equal(got, whole[60:68, 60:68].permute(2, 0, 1))


def test_max_tiles_per_call_changes_neither_the_bytes_nor_the_image():
    tiles = TL()
    net = gpu_codec()
    buf = encoded(16)
    whole = tiles.decode_tiled(net, buf)
    for per_call in (1, 4, 32):
        assert encoded(16, per_call) == buf, per_call
        assert torch.equal(tiles.decode_tiled(net, buf, max_tiles_per_call=per_call), whole), per_call


def test_a_truncated_container_decodes_the_regions_it_holds():
    from progressivecodec_amd import container
    tiles = TL()
    net = gpu_codec()
    buf = encoded(16)
    hd = tiles.parse_tiled(buf)
    whole = tiles.decode_tiled(net, buf, level=1)
    k = 3
    cut = buf[:hd["table"][k][0] + hd["table"][k][1]]                      # tiles 0 .. 3 are complete, 4 and 5 are gone
    for region in [(5, 6, 20, 30), (0, 0, 48, 150), (70, 10, 30, 30)]:     # tiles {0}, {0, 1, 2}, {3}
        y0, x0, h, w = region
        assert torch.equal(tiles.decode_tiled(net, cut, level=1, region=region), whole[y0:y0 + h, x0:x0 + w]), region
    for region in [(70, 64, 30, 32), (0, 0, H0, W0), (60, 60, 8, 8)]:      # tile 4 is needed
        with pytest.raises(container.ContainerError, match="tile 4"):
            tiles.decode_tiled(net, cut, level=1, region=region)
    inside = buf[:hd["table"][k][0] + hd["table"][k][1] - 5]               # tile 3 is incomplete: regions that need it are refused
    assert torch.equal(tiles.decode_tiled(net, inside, level=1, region=(5, 6, 20, 30)), whole[5:25, 6:36])
    with pytest.raises(container.ContainerError):
        tiles.decode_tiled(net, inside, level=1, region=(70, 10, 30, 30))
    with pytest.raises(container.ContainerError, match="no level"):
        tiles.decode_tiled(net, buf, level=3)


def test_post_filtered_decode_runs_per_tile():
    from tests.test_gpu_unet_post import net_of
    tiles = TL()
    net = net_of(1)
    buf = tiles.encode_tiled(net, codec_image(), [0, 0.5], tile=T, overlap=16, mask_pol=POL)
    x = decoded_tiles(net, buf, 1)
    assert np.array_equal(tiles.decode_tiled(net, buf).cpu().numpy(), TC.stitch(x, H0, W0, T, 16, "nearest", "hwc"))
    assert torch.equal(tiles.decode_tiled(net, buf, region=(40, 90, 30, 30)), tiles.decode_tiled(net, buf)[40:70, 90:120])

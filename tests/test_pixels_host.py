"""The image-domain layer without a GPU: the numpy restatement (tests/pixels_contract.py) against torch bit for bit, the geometry against
harness.compute_padding, and libpc_pixels.so's C ABI and progressivecodec_amd.pixels up to the first device call: exports, the plan,
every argument error.

The tests of the first section ("the restatement against torch") run tests/pixels_contract.py against torch only: they check the
reference the GPU tests compare with, not the feature, and pass without it.  The rest needs progressivecodec_amd.pixels."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import pixels_contract as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# -- the restatement against torch ---------------------------------------------------------------------------------------------------

def test_unit_is_torch_division_for_every_byte_and_not_the_reciprocal_multiply():
    v = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(v).float().div(255).numpy()
    assert np.array_equal(bits(K.unit(v)), bits(want))
    recip = v.astype(np.float32) * (np.float32(1) / np.float32(255))
    assert int((bits(recip) != bits(want)).sum()) == 126             # why a multiply by 1/255.f will not do


def test_geometry_and_padding_equal_compute_padding():
    from progressivecodec_amd.harness import compute_padding
    from progressivecodec_amd.pixels import padding
    for h in range(1, 201):
        for w in range(1, 201):
            (left, right, top, bottom), unpad = compute_padding(h, w, 64)
            g = padding(h, w)
            assert (g.H, g.W, g.Hp, g.Wp, g.top, g.left) == (h, w, h + top + bottom, w + left + right, top, left)
            assert g.pad == (left, right, top, bottom) and g.unpad == unpad
            assert K.geometry(h, w) == (g.Hp, g.Wp, g.top, g.left)
            assert g.Hp % 64 == 0 and g.Wp % 64 == 0 and 0 <= bottom - top <= 1 and 0 <= right - left <= 1
    assert tuple(padding(5, 7, multiple=8)) == (5, 7, 8, 8, 1, 0)
    with pytest.raises(ValueError):
        padding(0, 5)


@pytest.mark.parametrize("hw", [(1, 1), (63, 65), (5, 200), (64, 64), (65, 127)])
def test_ingest_is_totensor_then_pad(hw):
    from progressivecodec_amd.harness import compute_padding
    H, W = hw
    rng = np.random.default_rng(H * 1000 + W)
    chw = rng.integers(0, 256, (2, 3, H, W), dtype=np.uint8)
    pad, _ = compute_padding(H, W, 64)
    want = F.pad(torch.from_numpy(chw).float().div(255), pad, mode="constant", value=0).numpy()
    hp, wp, top, left = K.geometry(H, W)
    assert np.array_equal(bits(K.ingest(chw, "chw", hp, wp, top, left)), bits(want))
    assert np.array_equal(bits(K.ingest(K.from_chw(chw, "hwc"), "hwc", hp, wp, top, left)), bits(want))


def test_emit_is_unpad_clamp_and_the_two_roundings():
    from progressivecodec_amd.harness import compute_padding
    H, W = 63, 65
    hp, wp, top, left = K.geometry(H, W)
    ref = np.random.default_rng(5).integers(0, 256, (2, 3, H, W), dtype=np.uint8)
    x = K.hostile_planes(ref, hp, wp, top, left, 6)
    assert np.isnan(x).any() and np.isinf(x).any() and (x < 0).any() and (x > 1).any()
    _, unpad = compute_padding(H, W, 64)
    t = F.pad(torch.from_numpy(x), unpad)
    finite = torch.nan_to_num(t, nan=0.0, posinf=2.0, neginf=-2.0)          # torch.clamp propagates NaN; the definition maps it to 0
    cl = finite.clamp(0, 1)
    assert np.array_equal(K.emit(x, top, left, H, W, "trunc", "chw"), cl.mul(255).byte().numpy())
    assert np.array_equal(K.emit(x, top, left, H, W, "nearest", "chw"), np.rint(cl.mul(255).numpy()).astype(np.uint8))
    assert np.array_equal(K.emit(x, top, left, H, W, "nearest", "hwc"), K.emit(x, top, left, H, W, "nearest", "chw").transpose(0, 2, 3, 1))
    nan_at = np.isnan(x[:, :, top:top + H, left:left + W])
    assert nan_at.any() and (K.emit(x, top, left, H, W, "nearest", "chw")[nan_at] == 0).all()


def test_ties_go_to_even_and_trunc_goes_down():
    ties = K.exact_ties()
    assert len(ties) >= 32
    prod = (ties * K.F255).astype(np.float32)
    k = np.floor(prod)
    assert np.array_equal(prod - k, np.full(len(ties), 0.5, np.float32))
    near, down = K.quantise(ties, "nearest"), K.quantise(ties, "trunc")
    assert (near % 2 == 0).all() and np.array_equal(down, k.astype(np.uint8))
    assert (near == k + 1).any() and (near == k).any()                    # both directions occur: it is not "half up"
    half = np.float32(0.5)                                                # 127.5 exactly
    assert K.quantise(np.array([half]), "nearest")[0] == 128 and K.quantise(np.array([half]), "trunc")[0] == 127
    # the 0.5/255 * k pattern, in float32: whatever the product is, rint of it is what numpy and torch agree on
    pat = (np.arange(1, 511, 2, dtype=np.float32) * np.float32(0.5)) / K.F255
    assert np.array_equal(K.quantise(pat, "nearest"), torch.from_numpy(pat).mul(255).round().byte().numpy())


def test_the_ingest_of_every_byte_emits_that_byte_in_both_roundings():
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(K.quantise(K.unit(v), "nearest"), v)
    assert np.array_equal(K.quantise(K.unit(v), "trunc"), v)


def test_sums_on_a_hand_case():
    ref = np.zeros((1, 3, 1, 2), np.uint8)
    ref[0, :, 0, 1] = (255, 51, 0)
    x = np.zeros((1, 3, 1, 2), np.float32)
    x[0, :, 0, 1] = (0.5, 0.2, np.nan)
    su, sf = K.sums(x, 0, 0, 1, 2, "nearest", ref, "chw")
    assert su == [[(128 - 255) ** 2, 0, 0]]                               # 0.5 * 255 = 127.5 -> 128; 0.2f * 255 -> 51; NaN -> 0
    d1 = float(np.float32(np.float32(51) / np.float32(255)) - np.float32(0.2))
    assert sf == [[0.25, d1 * d1, 0.0]]
    assert K.psnr([0.0, 0.0, 0.0], 1, 2) == float("inf") and K.psnr_8bit([0, 0, 0], 1, 2) == float("inf")
    assert abs(K.psnr_8bit([65025, 65025, 65025], 1, 1)) < 1e-12 and abs(K.psnr([3.0, 0, 0], 1, 1)) < 1e-12


# -- the library, no device ----------------------------------------------------------------------------------------------------------

def _lib():
    from progressivecodec_amd import pixels
    return pixels, pixels.lib()


def test_library_exports_every_declared_function():
    pixels, L = _lib()
    hdr = open(os.path.join(ROOT, "progressivecodec_amd", "pixels_csrc", "pc_pixels.h")).read()
    declared = re.findall(r"PC_API\s+[\w\s\*]+?\b(pc_\w+)\s*\(", hdr)
    assert len(declared) == 6 and sorted(declared) == sorted(pixels.EXPORTS)
    for name in declared:
        getattr(L, name)
    assert L.pc_pixels_strerror(-1).decode() and L.pc_pixels_strerror(-6).decode() and L.pc_pixels_last_hip_error() == 0


def test_workspace_size():
    _, L = _lib()
    blocks = lambda h, w: -(-(h * -(-w // 4)) // 1024)
    for B, H, W in [(1, 1, 1), (32, 256, 256), (1, 2160, 3840), (3, 65, 127), (2, 5, 200), (1, 4097, 1)]:
        assert L.pc_pixels_emit_workspace_size(B, H, W) == 48 * B * blocks(H, W)
    for bad in [(0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, 2 ** 31 - 1, 2 ** 31 - 1)]:
        assert L.pc_pixels_emit_workspace_size(*bad) == 0


def _plan(L, op, u8, layout, sb, sp, sr, f32, fb, fc, fh, top, left, B, H, W, ref=None, ref_layout=0, rb=0, rp=0, rr=0):
    wide = C.c_int(-1)
    rc = L.pc_pixels_plan(op, u8, layout, sb, sp, sr, f32, fb, fc, fh, top, left, B, H, W, ref, ref_layout, rb, rp, rr, C.byref(wide))
    return rc, wide.value


def test_plan_is_host_only_and_reports_the_path():
    """made-up pointer values: nothing may be dereferenced or launched (there is no GPU here)"""
    _, L = _lib()
    HWC, CHW, ING, EMIT = 0, 1, 0, 1
    A, Fp = 0x7000_0000_1000, 0x7000_0100_0000
    H, W, Hp, Wp = 64, 64, 64, 64
    fs = (3 * Hp * Wp, Hp * Wp, Wp)
    ok = lambda *a, **k: _plan(L, *a, **k)
    # ingest, interleaved: aligned everything -> wide; base off by 1..3, odd row or batch stride, unaligned float base -> narrow
    assert ok(ING, A, HWC, 3 * H * W, 0, 3 * W, Fp, *fs, 0, 0, 2, H, W) == (0, 1)
    for off in (1, 2, 3):
        assert ok(ING, A + off, HWC, 3 * H * W, 0, 3 * W, Fp, *fs, 0, 0, 2, H, W) == (0, 0)
    assert ok(ING, A, HWC, 3 * H * W, 0, 3 * W + 1, Fp, *fs, 0, 0, 2, H, W) == (0, 0)
    assert ok(ING, A, HWC, 3 * H * W + 2, 0, 3 * W, Fp, *fs, 0, 0, 2, H, W) == (0, 0)
    assert ok(ING, A, HWC, 3 * H * W, 0, 3 * W, Fp + 4, *fs, 0, 0, 2, H, W) == (0, 0)
    assert ok(ING, A, HWC, 3 * H * W, 77, 3 * W, Fp, *fs, 0, 0, 2, H, W) == (0, 1)              # s_plane is ignored when interleaved
    # a 3*W row of 63 pixels is 189 bytes: never wide unless the row stride is padded
    assert ok(ING, A, HWC, 63 * 189, 0, 189, Fp, *fs, 0, 0, 1, 63, 63) == (0, 0)
    assert ok(ING, A, HWC, 63 * 192, 0, 192, Fp, *fs, 0, 0, 1, 63, 63) == (0, 1)
    # `left` moves the address of padded column 0: src - 3*left (interleaved), src - left (planar)
    assert ok(ING, A, HWC, 3 * 60 * 60, 0, 180, Fp, *fs, 2, 2, 1, 60, 60) == (0, 0)             # 3*2 = 6: off by 2
    assert ok(ING, A + 2, HWC, 3 * 60 * 60, 0, 180, Fp, *fs, 2, 2, 1, 60, 60) == (0, 1)
    assert ok(ING, A, HWC, 3 * 56 * 56, 0, 168, Fp, *fs, 4, 4, 1, 56, 56) == (0, 1)
    assert ok(ING, A, CHW, 3 * 60 * 60, 3600, 60, Fp, *fs, 2, 2, 1, 60, 60) == (0, 0)
    assert ok(ING, A + 2, CHW, 3 * 60 * 60, 3600, 60, Fp, *fs, 2, 2, 1, 60, 60) == (0, 1)
    assert ok(ING, A, CHW, 3 * H * W, H * W, W, Fp, *fs, 0, 0, 2, H, W) == (0, 1)
    assert ok(ING, A, CHW, 3 * H * W, H * W + 1, W, Fp, *fs, 0, 0, 2, H, W) == (0, 0)
    assert ok(ING, A, CHW, 3 * H * W, H * W, W, Fp, 3 * Hp * 66, Hp * 66, 66, 0, 0, 2, H, W) == (0, 0)     # Wp = 66
    # emit: the float side needs left % 4 == 0 and strides % 4 == 0; every u8 view its own alignment; ref counts when given
    assert ok(EMIT, A, HWC, 3 * H * W, 0, 3 * W, Fp, *fs, 0, 0, 2, H, W) == (0, 1)
    assert ok(EMIT, A, HWC, 3 * 56 * 56, 0, 168, Fp, *fs, 4, 4, 1, 56, 56) == (0, 1)
    assert ok(EMIT, A, HWC, 3 * 58 * 58, 0, 176, Fp, *fs, 3, 3, 1, 58, 58) == (0, 0)
    assert ok(EMIT, A + 1, HWC, 3 * H * W, 0, 3 * W, Fp, *fs, 0, 0, 2, H, W) == (0, 0)
    assert ok(EMIT, A, CHW, 3 * H * W, H * W, W, Fp, 3 * 70 * 70, 70 * 70, 70, 0, 0, 2, H, W) == (0, 0)
    assert ok(EMIT, A, CHW, 3 * H * W, H * W, W, Fp, 3 * 72 * 72, 72 * 72, 72, 0, 0, 2, H, W) == (0, 1)
    assert ok(EMIT, A, CHW, 3 * H * W, H * W, W, Fp, *fs, 0, 0, 2, H, W, A + 0x10000, HWC, 3 * H * W, 0, 3 * W) == (0, 1)
    assert ok(EMIT, A, CHW, 3 * H * W, H * W, W, Fp, *fs, 0, 0, 2, H, W, A + 0x10001, HWC, 3 * H * W, 0, 3 * W) == (0, 0)
    assert ok(ING, A, CHW, 3 * H * W, H * W, W, Fp, *fs, 0, 0, 2, H, W, A + 0x10001, HWC, 3 * H * W, 0, 3 * W) == (0, 1)   # ingest: no ref
    # refusals
    for bad in [dict(op=2), dict(u8=None), dict(f32=None), dict(layout=2), dict(B=0), dict(H=0), dict(W=0), dict(left=-1)]:
        a = dict(op=ING, u8=A, layout=HWC, sb=3 * H * W, sp=0, sr=3 * W, f32=Fp, fb=fs[0], fc=fs[1], fh=fs[2], top=0, left=0, B=2, H=H, W=W)
        a.update(bad)
        assert _plan(L, *a.values())[0] == -1, bad
    assert L.pc_pixels_plan(ING, A, HWC, 3 * H * W, 0, 3 * W, Fp, *fs, 0, 0, 2, H, W, None, 0, 0, 0, 0, None) == -1
    # sums only: an emit without a destination is planned from x and ref
    assert ok(EMIT, None, 0, 0, 0, 0, Fp, *fs, 0, 0, 2, H, W, A, CHW, 3 * H * W, H * W, W) == (0, 1)
    assert ok(EMIT, None, 0, 0, 0, 0, Fp, *fs, 0, 0, 2, H, W, A + 2, CHW, 3 * H * W, H * W, W) == (0, 0)
    assert ok(EMIT, None, 0, 0, 0, 0, Fp, *fs, 0, 0, 2, H, W)[0] == -1 and ok(ING, None, 0, 0, 0, 0, Fp, *fs, 0, 0, 2, H, W, A, CHW, 1, 1, W)[0] == -1


def test_every_argument_error_returns_before_the_device():
    """fake device pointers: every call below must return PC_ERR_ARG without touching them (no GPU here)"""
    _, L = _lib()
    A, Fp, Wk, S = 0x7000_0000_1000, 0x7000_0100_0000, 0x7000_0200_0000, 0x7000_0300_0000
    H, W, Hp, Wp = 60, 62, 64, 64
    ing = dict(src=A, layout=0, sb=3 * H * W, sp=0, sr=3 * W, B=2, H=H, W=W, dst=Fp, Hp=Hp, Wp=Wp, top=2, left=1, stream=None)
    for bad in [dict(src=None), dict(dst=None), dict(layout=2), dict(layout=-1), dict(B=0), dict(H=0), dict(W=0), dict(top=-1), dict(left=-1),
                dict(top=5), dict(left=3), dict(Hp=0), dict(sr=3 * W - 1), dict(sb=0), dict(dst=Fp + 2), dict(layout=1, sp=0),
                dict(layout=1, sr=W - 1)]:
        assert L.pc_pixels_ingest_u8(*dict(ing, **bad).values()) == -1, bad
    nbytes = L.pc_pixels_emit_workspace_size(2, H, W)
    em = dict(x=Fp, sxb=3 * Hp * Wp, sxc=Hp * Wp, sxh=Wp, Hp=Hp, Wp=Wp, top=2, left=1, B=2, H=H, W=W, rounding=0, dst=A, dl=0, db=3 * H * W,
              dp=0, dr=3 * W, ref=A + 0x100000, rl=1, rb=3 * H * W, rp=H * W, rr=W, ws=Wk, nbytes=nbytes, su=S, sf=S + 64, stream=None)
    for bad in [dict(x=None), dict(dl=2), dict(rl=7), dict(rounding=2), dict(rounding=-1), dict(B=0), dict(H=0), dict(W=0),
                dict(top=5), dict(left=3), dict(top=-1), dict(sxh=Wp - 1), dict(sxc=0), dict(x=Fp + 1), dict(dr=3 * W - 1),
                dict(db=3 * H * W - 1), dict(dl=1, dp=H * W - 1, dr=W), dict(ws=None), dict(su=None), dict(sf=None), dict(nbytes=nbytes - 1),
                dict(nbytes=0), dict(ws=Wk + 4), dict(rr=W - 1), dict(su=S + 4), dict(sf=S + 68), dict(dst=None, ref=None)]:
        assert L.pc_pixels_emit_u8(*dict(em, **bad).values()) == -1, bad
    # a destination must be nested rows-in-planes-in-images: [B,H,3,W] memory (plane stride < row stride) is refused though disjoint
    assert L.pc_pixels_emit_u8(*dict(em, dl=1, db=3 * H * W, dp=W, dr=3 * W).values()) == -1


def test_python_rejects_before_any_device_call(monkeypatch):
    from progressivecodec_amd import pixels

    def touched(*a, **k):
        raise AssertionError("the device was reached")
    for name in ("device", "current_stream", "synchronize", "current_device", "_lazy_init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.setattr(pixels, "lib", touched)
    hwc = torch.zeros(5, 7, 3, dtype=torch.uint8)
    g = pixels.padding(5, 7)
    with pytest.raises(ValueError, match="GPU"):
        pixels.to_model_input(hwc)
    with pytest.raises(ValueError, match="GPU"):
        pixels.to_model_input(hwc.permute(2, 0, 1), layout="chw")
    with pytest.raises(ValueError, match="layout"):
        pixels.to_model_input(hwc, layout="nhwc")
    with pytest.raises(TypeError, match="uint8"):
        pixels.to_model_input(hwc.float())
    with pytest.raises(TypeError, match="tensor"):
        pixels.to_model_input(hwc.numpy())
    with pytest.raises(ValueError, match="3 channels"):
        pixels.to_model_input(hwc, layout="chw")
    for bad in (torch.zeros(7, 3, dtype=torch.uint8), torch.zeros(1, 1, 5, 7, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="must be"):
            pixels.to_model_input(bad)
    with pytest.raises(ValueError, match="empty"):
        pixels.to_model_input(torch.zeros(0, 7, 3, dtype=torch.uint8))
    xh = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match="GPU"):
        pixels.from_model_output(xh, g)
    with pytest.raises(ValueError, match="GPU"):
        pixels.from_model_output(xh, g, ref=hwc)
    with pytest.raises(ValueError, match="rounding"):
        pixels.from_model_output(xh, g, rounding="floor")
    with pytest.raises(ValueError, match="layout"):
        pixels.from_model_output(xh, g, layout="cwh")
    with pytest.raises(TypeError, match="float32"):
        pixels.from_model_output(xh.double(), g)
    with pytest.raises(ValueError, match="x_hat must be"):
        pixels.from_model_output(xh[:, :, :63], g)
    with pytest.raises(ValueError, match="x_hat must be"):
        pixels.from_model_output(xh[0, 0], g)
    with pytest.raises(ValueError, match="outside"):
        pixels.from_model_output(xh, pixels.Geometry(5, 7, 64, 64, 60, 0))
    with pytest.raises(TypeError, match="uint8"):
        pixels.from_model_output(xh, g, ref=hwc.float())
    with pytest.raises(ValueError, match="image=False"):
        pixels.from_model_output(xh, g, image=False)
    with pytest.raises(ValueError, match="GPU"):
        pixels.from_model_output(xh, g, ref=hwc, image=False)
    with pytest.raises(ValueError, match="GPU"):
        pixels.encode_image(None, hwc, [0])
    with pytest.raises(ValueError, match="layout"):
        pixels.decode_image(None, b"", layout="x")
    with pytest.raises(ValueError, match="rounding"):
        pixels.decode_image(None, b"", rounding="x")


def test_decode_image_refuses_bad_headers_before_the_model():
    from progressivecodec_amd import container, pixels
    y = [[b"ab"] for _ in range(20)]
    ok = container.pack([[y[:10], [b"z"]], [y, [b"z"]]], (2, 2), [0, 0.5], image_size=(65, 127), contract=1)
    with pytest.raises(container.ContainerError, match="no level"):
        pixels.decode_image(None, ok, level=2)
    with pytest.raises(container.ContainerError, match="no level"):
        pixels.decode_image(None, ok, level=-3)
    wrong = container.pack([[y[:10], [b"z"]]], (2, 3), [0], image_size=(65, 127), contract=1)
    with pytest.raises(container.ContainerError, match="header shape"):
        pixels.decode_image(None, wrong)
    empty = container.pack([[y[:10], [b"z"]]], (0, 2), [0], image_size=(0, 127), contract=1)
    with pytest.raises(container.ContainerError, match="image size"):
        pixels.decode_image(None, empty)
    with pytest.raises(container.ContainerError):
        pixels.decode_image(None, b"nope")


def test_harness_pixel_io_is_refused_in_the_batched_paths():
    from progressivecodec_amd.harness import compress_with_ac
    img = torch.zeros(3, 64, 64, dtype=torch.uint8)
    with pytest.raises(NotImplementedError, match="pixel_io"):
        compress_with_ac(None, [img], [0], pixel_io=True, batch_same_size=True)
    with pytest.raises(NotImplementedError, match="pixel_io"):
        compress_with_ac(None, [img], [0], pixel_io=True, overlap=True)

"""MS-SSIM without a GPU: the float64 checker (tests/msssim_ref.py) against itself and hand-computed cases, and libpc_metrics.so's
C ABI up to the first HIP call (metrics_csrc/pc_metrics.h): exports, the workspace formula and every argument error."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import msssim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _smooth(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    lo = torch.rand(B, 3, (H + 7) // 8, (W + 7) // 8, generator=g)
    return F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False)


# -- the checker ---------------------------------------------------------------------------------------------------------------------

def test_ref_identity_and_symmetry():
    x = _smooth(2, 181, 203, 1)
    y = (x + 0.05 * torch.randn(x.shape, generator=torch.Generator().manual_seed(2))).clamp(0, 1)
    assert torch.allclose(R.ms_ssim_ref(x, x, data_range=1.0), torch.ones(2, dtype=torch.float64), rtol=0, atol=1e-12)
    a, b = R.ms_ssim_ref(x, y, data_range=1.0), R.ms_ssim_ref(y, x, data_range=1.0)
    assert torch.equal(a, b) or torch.allclose(a, b, rtol=0, atol=1e-14)
    assert (a < 1).all() and (a > 0).all()


def test_ref_separable_filter_equals_the_2d_window():
    x = torch.rand(1, 2, 23, 19, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    g = R.gauss_1d(11, 1.5).double()
    w2 = torch.outer(g, g).view(1, 1, 11, 11).repeat(2, 1, 1, 1)
    direct = F.conv2d(x, w2, groups=2)
    sep = R.gaussian_filter(x, g)
    assert sep.shape == (1, 2, 13, 9)
    assert torch.allclose(sep, direct, rtol=0, atol=1e-14)
    assert abs(float(R.gauss_1d(11, 1.5).sum()) - 1) < 1e-6


def test_ref_pool_of_an_odd_plane():
    x = torch.arange(1, 10, dtype=torch.float64).view(1, 1, 3, 3)       # 1 2 3 / 4 5 6 / 7 8 9
    # zero on both sides of both odd sides, divisor 4: windows [-1,0] x [-1,0], [-1,0] x [1,2], ...
    want = torch.tensor([[1 / 4, (2 + 3) / 4], [(4 + 7) / 4, (5 + 6 + 8 + 9) / 4]], dtype=torch.float64)
    assert torch.equal(R.pool2(x)[0, 0], want)


# -- the library, no device ----------------------------------------------------------------------------------------------------------

def _lib():
    from progressivecodec_amd import metrics
    return metrics, metrics.lib()


def test_library_exports_every_declared_function():
    metrics, L = _lib()
    hdr = open(os.path.join(ROOT, "progressivecodec_amd", "metrics_csrc", "pc_metrics.h")).read()
    declared = re.findall(r"PC_API\s+[\w\s\*]+?\b(pc_\w+)\s*\(", hdr)
    assert sorted(declared) == sorted(metrics.EXPORTS)
    for name in declared:
        getattr(L, name)
    assert L.pc_metrics_strerror(-1).decode() and L.pc_metrics_strerror(-3).decode()


def _workspace_formula(B, C, H, W, ws, levels):
    a256 = lambda n: (n + 255) // 256 * 256
    hs, wsz = [H], [W]
    for _ in range(1, levels):
        hs.append((hs[-1] + 1) // 2)
        wsz.append((wsz[-1] + 1) // 2)
    tiles = [-(-(h - ws + 1) // 32) * -(-(w - ws + 1) // 64) for h, w in zip(hs, wsz)]
    total = a256(16 * B * C * sum(tiles))
    for s in range(1, levels):
        total += 2 * a256(4 * B * C * hs[s] * wsz[s])
    return total


@pytest.mark.parametrize("shape", [(1, 3, 256, 256, 11, 5), (32, 3, 256, 256, 11, 5), (2, 1, 181, 203, 11, 5), (1, 3, 2161, 3841, 11, 5),
                                   (3, 3, 161, 161, 7, 3), (2, 3, 11, 40, 11, 1), (1, 1, 97, 97, 7, 5), (4, 2, 40, 35, 3, 2)])
def test_workspace_size_formula(shape):
    _, L = _lib()
    assert L.pc_msssim_workspace_size(*shape) == _workspace_formula(*shape)


def test_workspace_size_rejects_what_the_call_rejects():
    _, L = _lib()
    for bad in [(0, 3, 256, 256, 11, 5), (1, 0, 256, 256, 11, 5), (1, 3, 160, 256, 11, 5), (1, 3, 256, 160, 11, 5),
                (1, 3, 256, 256, 10, 5), (1, 3, 256, 256, 33, 5), (1, 3, 256, 256, 11, 0), (1, 3, 256, 256, 11, 6),
                (1, 3, 10, 256, 11, 1), (1, 3, 256, 256, -1, 1)]:
        assert L.pc_msssim_workspace_size(*bad) == 0, bad
    assert L.pc_msssim_workspace_size(1, 3, 161, 161, 11, 5) > 0


def test_every_argument_error_returns_before_the_device():
    """fake device pointers: every call below must return PC_ERR_ARG / PC_ERR_BUFFER without touching them (no GPU here)"""
    _, L = _lib()
    fake = 0x1000
    ok = dict(X=fake, sxb=3 * 256 * 256, sxc=256 * 256, sxh=256, Y=fake, syb=3 * 256 * 256, syc=256 * 256, syh=256, B=1, C=3, H=256, W=256,
              data_range=1.0, win_size=11, win_sigma=1.5, K1=0.01, K2=0.03, levels=5,
              weights=(C.c_float * 5)(0.0448, 0.2856, 0.3001, 0.2363, 0.1333), nonnegative=0, ws=fake,
              nbytes=L.pc_msssim_workspace_size(1, 3, 256, 256, 11, 5), out=fake, out_scales=None, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.pc_msssim(a["X"], a["sxb"], a["sxc"], a["sxh"], a["Y"], a["syb"], a["syc"], a["syh"], a["B"], a["C"], a["H"], a["W"],
                           a["data_range"], a["win_size"], a["win_sigma"], a["K1"], a["K2"], a["levels"], a["weights"], a["nonnegative"],
                           a["ws"], a["nbytes"], a["out"], a["out_scales"], a["stream"])
    ERR_ARG, ERR_BUFFER = -1, -3
    cases = [dict(X=None), dict(Y=None), dict(out=None), dict(ws=None), dict(weights=None), dict(B=0), dict(C=0), dict(H=160),
             dict(W=100), dict(win_size=10), dict(win_size=33), dict(win_size=0), dict(levels=0), dict(levels=6), dict(win_sigma=0.0),
             dict(win_sigma=float("nan")), dict(data_range=float("inf")), dict(K1=float("nan")), dict(sxh=0), dict(syc=-1),
             dict(levels=1, H=10), dict(weights=(C.c_float * 5)(0.0448, float("nan"), 0.3001, 0.2363, 0.1333))]
    for kw in cases:
        assert call(**kw) == ERR_ARG, kw
    assert call(nbytes=ok["nbytes"] - 1) == ERR_BUFFER


def test_python_rejects_before_any_device_call():
    from progressivecodec_amd import metrics
    x = torch.rand(1, 3, 192, 192)
    with pytest.raises(ValueError, match="GPU"):
        metrics.ms_ssim(x, x, data_range=1.0)
    with pytest.raises(ValueError, match="GPU"):
        metrics.ssim(x, x, data_range=1.0)
    with pytest.raises(TypeError, match="float32"):
        metrics.ms_ssim(x.double(), x.double(), data_range=1.0)
    with pytest.raises(ValueError, match="same dimensions"):
        metrics.ms_ssim(x, x[:, :, :191], data_range=1.0)
    with pytest.raises(NotImplementedError):
        metrics.ms_ssim(x, x, win=torch.ones(1, 1, 1, 11))
    with pytest.raises(ValueError, match="odd"):
        metrics.ssim(x, x, win_size=10)
    with pytest.raises(ValueError, match="weights"):
        metrics.ms_ssim(x, x, weights=[1.0])

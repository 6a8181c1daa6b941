"""MS-SSIM and SSIM on the GPU (libpc_metrics.so, metrics_csrc/pc_metrics.h): a drop-in for the `pytorch_msssim` functions the reference
calls (training/step.py:7,350; utils/functions.py:5,21,140; utils/eval_model/__main__.py:32,121).

The definition is the public behaviour of pytorch_msssim 1.0.  Differences: a custom `win` tensor, non-float32
inputs and 5-D inputs raise; `ssim()` requires H, W >= win_size (the library would skip filtering along a shorter axis with a warning);
`ms_ssim()` takes 2 to 5 weights.  There is no CPU fallback: CPU tensors raise before any device call.
"""
import ctypes as C

from . import _imagelib
from ._lib import PC_OK

LIB_PATH = _imagelib.lib_path("metrics")

#: every symbol metrics_csrc/pc_metrics.h declares
EXPORTS = ["pc_msssim_workspace_size", "pc_msssim", "pc_msssim_plan", "pc_metrics_strerror", "pc_metrics_last_hip_error"]

#: the library's default scale weights (Wang, Simoncelli, Bovik 2003)
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def _prototypes():
    i64, vp = C.c_int64, C.c_void_p
    return {
        "pc_msssim_workspace_size": (C.c_size_t, [C.c_int] * 6),
        "pc_msssim": (None, [vp, i64, i64, i64, vp, i64, i64, i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float,
                             C.c_float, C.c_float, C.c_int, C.POINTER(C.c_float), C.c_int, vp, C.c_size_t, vp, vp, vp]),
        "pc_msssim_plan": (None, [vp, i64, i64, i64, vp, i64, i64, i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp,
                                  C.POINTER(C.c_int)]),
        "pc_metrics_strerror": (C.c_char_p, [C.c_int]),
    }


def lib():
    return _imagelib.load(LIB_PATH, _prototypes)


class MetricsError(_imagelib.ImageLibError):
    _lib, _prefix = staticmethod(lib), "pc_metrics"


def _check_inputs(X, Y, win, win_size):
    import torch
    if win is not None:
        raise NotImplementedError("a custom `win` tensor is not supported: pass win_size / win_sigma")
    if not (torch.is_tensor(X) and torch.is_tensor(Y)):
        raise TypeError("X and Y must be tensors")
    if X.shape != Y.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {tuple(X.shape)} and {tuple(Y.shape)}.")
    if X.dim() != 4:
        raise ValueError(f"Input images should be 4-d tensors [B, C, H, W], but got {tuple(X.shape)}")
    if X.dtype != torch.float32 or Y.dtype != torch.float32:
        raise TypeError(f"Input images should be float32, but got {X.dtype} and {Y.dtype}")
    if not win_size % 2 == 1:
        raise ValueError("Window size should be odd.")
    if X.device.type != "cuda" or Y.device != X.device:
        raise ValueError(f"Input images should be on one GPU (there is no CPU fallback), but got {X.device} and {Y.device}")
    if X.stride(3) != 1 or Y.stride(3) != 1 or min(X.stride()[:3] + Y.stride()[:3]) < 1:
        raise ValueError("X and Y need a unit stride along W and positive strides elsewhere (call .contiguous())")


def _run(X, Y, data_range, win_size, win_sigma, K, weights, nonnegative, scales=False):
    """per-image values [B] (float32, X's device), and the per-scale means [levels][2][B][C] (float64) when `scales`"""
    import torch
    L = lib()
    B, Cc, H, W = X.shape
    levels = 1 if weights is None else len(weights)
    with torch.cuda.device(X.device):
        nbytes = L.pc_msssim_workspace_size(B, Cc, H, W, int(win_size), levels)
        if nbytes == 0:
            if levels > 1:
                raise ValueError(f"Image size should be larger than {(win_size - 1) * 2 ** 4} due to the 4 downsamplings in ms-ssim "
                                 f"(got {H}x{W}, win_size {win_size}, {levels} scales)")
            raise ValueError(f"Image size should be at least win_size = {win_size} (got {H}x{W})")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=X.device)
        out = torch.empty(B, dtype=torch.float32, device=X.device)
        per_scale = torch.empty(levels, 2, B, Cc, dtype=torch.float64, device=X.device) if scales else None
        w = (C.c_float * levels)(*[float(v) for v in weights]) if weights is not None else None
        st = torch.cuda.current_stream(X.device).cuda_stream
        rc = L.pc_msssim(X.data_ptr(), X.stride(0), X.stride(1), X.stride(2), Y.data_ptr(), Y.stride(0), Y.stride(1), Y.stride(2),
                         B, Cc, H, W, float(data_range), int(win_size), float(win_sigma), float(K[0]), float(K[1]), levels, w,
                         1 if nonnegative else 0, ws.data_ptr(), nbytes, out.data_ptr(),
                         per_scale.data_ptr() if scales else None, st)
        if rc != PC_OK:
            raise MetricsError(rc, "pc_msssim")
    return (out, per_scale) if scales else out


def ms_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, weights=None, K=(0.01, 0.03)):
    """pytorch_msssim.ms_ssim: X, Y float32 [B, C, H, W] on one GPU, min(H, W) > (win_size - 1) * 16.  Returns a float32 tensor on X's
    device: the mean over images (size_average=True) or one value per image [B].  Launched on the current stream."""
    weights = list(MS_WEIGHTS) if weights is None else [float(v) for v in weights]
    if not 2 <= len(weights) <= 5:
        raise ValueError(f"ms_ssim takes 2 to 5 scale weights, got {len(weights)}")
    _check_inputs(X, Y, win, win_size)
    out = _run(X, Y, data_range, win_size, win_sigma, K, weights, False)
    return out.mean() if size_average else out


def ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, K=(0.01, 0.03), nonnegative_ssim=False):
    """pytorch_msssim.ssim: X, Y float32 [B, C, H, W] on one GPU, H, W >= win_size.  Returns a float32 tensor on X's device: the mean
    over images (size_average=True) or one value per image [B].  nonnegative_ssim: relu on the per-channel value."""
    _check_inputs(X, Y, win, win_size)
    out = _run(X, Y, data_range, win_size, win_sigma, K, None, nonnegative_ssim)
    return out.mean() if size_average else out


def ms_ssim_scales(X, Y, data_range=255, win_size=11, win_sigma=1.5, weights=None, K=(0.01, 0.03)):
    """ms_ssim per image [B] and, per scale, the means of the SSIM and CS maps per (image, channel): float64 [levels][2][B][C] ([s][0]:
    SSIM, [s][1]: CS), before relu."""
    weights = list(MS_WEIGHTS) if weights is None else [float(v) for v in weights]
    if not 2 <= len(weights) <= 5:
        raise ValueError(f"ms_ssim takes 2 to 5 scale weights, got {len(weights)}")
    _check_inputs(X, Y, None, win_size)
    return _run(X, Y, data_range, win_size, win_sigma, K, weights, False, scales=True)


def compute_msssim(a, b):
    """utils/functions.py:140: ms_ssim(a, b, data_range=1.) as a Python float."""
    return ms_ssim(a, b, data_range=1.).item()

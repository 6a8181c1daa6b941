"""8-bit pixels in, 8-bit pixels out (libpc_pixels.so, pixels_csrc/pc_pixels.h): what stands between a decoded image
file and the codec's float32 [B,3,H,W] planes with H, W multiples of 64, and back.

  to_model_input      uint8 image -> centre-padded float planes (the reference's ToTensor + F.pad with compute_padding,
                      training/step.py:318-319), one kernel
  from_model_output   decoder output -> un-padded, clamped, rounded uint8 image and, given the original, the distortion sums behind
                      PSNR (training/step.py:13-15, 342-349), one kernel
  encode_image        uint8 image -> one PCB1 container (container.py) per image
  decode_image        PCB1 container -> uint8 image of the original size (the reference's save_images path, training/step.py:345-347)

Layouts: "hwc" is [H,W,3] / [B,H,W,3] (what PIL / numpy give), "chw" is [3,H,W] / [B,3,H,W].  There is no CPU fallback: CPU tensors
raise ValueError before any device call.  Everything runs on the current stream of the tensor's device.
"""
import collections
import ctypes as C
import math

from . import _imagelib
from ._lib import PC_OK
from .harness import compute_padding

LIB_PATH = _imagelib.lib_path("pixels")

#: every symbol pixels_csrc/pc_pixels.h declares
EXPORTS = ["pc_pixels_ingest_u8", "pc_pixels_emit_workspace_size", "pc_pixels_emit_u8", "pc_pixels_plan", "pc_pixels_strerror",
           "pc_pixels_last_hip_error"]

LAYOUTS = {"hwc": 0, "chw": 1}            # PC_PIXELS_HWC, PC_PIXELS_CHW
ROUNDINGS = {"nearest": 0, "trunc": 1}    # PC_PIXELS_NEAREST (rintf, half to even), PC_PIXELS_TRUNC (mul(255).byte())
INGEST, EMIT = 0, 1                       # pc_pixels_plan's `op`


def _prototypes():
    i64, vp, ci = C.c_int64, C.c_void_p, C.c_int
    u8v = [vp, ci, i64, i64, i64]                                   # a u8 view: pointer, layout, batch / plane / row stride in bytes
    return {
        "pc_pixels_ingest_u8": (None, u8v + [ci, ci, ci, vp, ci, ci, ci, ci, vp]),
        "pc_pixels_emit_workspace_size": (C.c_size_t, [ci, ci, ci]),
        "pc_pixels_emit_u8": (None, [vp, i64, i64, i64, ci, ci, ci, ci, ci, ci, ci, ci] + u8v + u8v + [vp, C.c_size_t, vp, vp, vp]),
        "pc_pixels_plan": (None, [ci] + u8v + [vp, i64, i64, i64, ci, ci, ci, ci, ci] + u8v + [C.POINTER(ci)]),
        "pc_pixels_strerror": (C.c_char_p, [ci]),
    }


def lib():
    return _imagelib.load(LIB_PATH, _prototypes)


class PixelsError(_imagelib.ImageLibError):
    _lib, _prefix = staticmethod(lib), "pc_pixels"


class Geometry(collections.namedtuple("Geometry", "H W Hp Wp top left")):
    """An H x W image inside its Hp x Wp padded planes, first pixel at (top, left)."""
    __slots__ = ()

    @property
    def pad(self):
        """(left, right, top, bottom) as F.pad takes it"""
        return (self.left, self.Wp - self.W - self.left, self.top, self.Hp - self.H - self.top)

    @property
    def unpad(self):
        return tuple(-v for v in self.pad)


def padding(h, w, multiple=64):
    """The geometry of harness.compute_padding (compressai.ops.compute_padding, training/step.py:318): padded up to the next multiple,
    centred, the extra row or column at the bottom / right."""
    h, w, multiple = int(h), int(w), int(multiple)
    if h < 1 or w < 1 or multiple < 1:
        raise ValueError(f"padding({h}, {w}, {multiple}): sizes must be positive")
    (left, right, top, bottom), _ = compute_padding(h, w, multiple)
    return Geometry(h, w, h + top + bottom, w + left + right, top, left)


def _u8_view(t, layout, what):
    """Checks a uint8 image tensor (no device call) and returns it as a 4-D tensor whose strides fit a u8 view, copying only when they
    do not (unit stride along the channel / column axis is needed), with (pointer, layout, batch, plane, row stride)."""
    import torch
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be 'hwc' or 'chw', got {layout!r}")
    if not torch.is_tensor(t):
        raise TypeError(f"{what} must be a tensor")
    if t.dtype != torch.uint8:
        raise TypeError(f"{what} must be uint8, got {t.dtype}")
    if t.dim() not in (3, 4):
        raise ValueError(f"{what} must be [H,W,3] / [B,H,W,3] ('hwc') or [3,H,W] / [B,3,H,W] ('chw'), got {tuple(t.shape)}")
    t4 = t if t.dim() == 4 else t.unsqueeze(0)
    if t4.shape[3 if layout == "hwc" else 1] != 3:
        raise ValueError(f"{what} must have 3 channels in layout {layout!r}, got {tuple(t.shape)}")
    if 0 in t4.shape:
        raise ValueError(f"{what} is empty: {tuple(t.shape)}")
    if t.device.type != "cuda":
        raise ValueError(f"{what} must be on a GPU (there is no CPU fallback), got {t.device}")
    sb, s1, s2, s3 = t4.stride()
    if layout == "hwc":
        W = t4.shape[2]
        if not (s3 == 1 and s2 == 3 and s1 >= 3 * W and sb >= 1):
            t4 = t4.contiguous()
        return t4, (t4.data_ptr(), 0, t4.stride(0), 0, t4.stride(1))
    W = t4.shape[3]
    if not (s3 == 1 and s2 >= W and s1 >= 1 and sb >= 1):
        t4 = t4.contiguous()
    return t4, (t4.data_ptr(), 1, t4.stride(0), t4.stride(1), t4.stride(2))


def _hw(t4, layout):
    return (t4.shape[1], t4.shape[2]) if layout == "hwc" else (t4.shape[2], t4.shape[3])


def to_model_input(img, layout="hwc", multiple=64):
    """uint8 cuda tensor [H,W,3] / [B,H,W,3] ("hwc") or [3,H,W] / [B,3,H,W] ("chw"), any strides -> (x_padded, geom): float32
    [B,3,Hp,Wp] = F.pad(img.float().div(255) as [B,3,H,W], geom.pad) bit for bit, and geom = padding(H, W, multiple)."""
    import torch
    t4, view = _u8_view(img, layout, "img")
    H, W = _hw(t4, layout)
    geom = padding(H, W, multiple)
    B = t4.shape[0]
    with torch.cuda.device(t4.device):
        x = torch.empty((B, 3, geom.Hp, geom.Wp), dtype=torch.float32, device=t4.device)
        rc = lib().pc_pixels_ingest_u8(*view, B, H, W, x.data_ptr(), geom.Hp, geom.Wp, geom.top, geom.left,
                                       torch.cuda.current_stream(t4.device).cuda_stream)
    if rc != PC_OK:
        raise PixelsError(rc, "pc_pixels_ingest_u8")
    return x, geom


def psnr_from_sse(sse, n):
    """-10 log10(sse / n) in Python doubles; inf at sse == 0"""
    return -10.0 * math.log10(sse / n) if sse > 0 else float("inf")


class Distortion:
    """The sums of one from_model_output(..., ref=...) call.  sse_u8 (int64 [B,3]): sum of (q - ref)^2 over the 8-bit values, exact.
    sse_f (float64 [B,3]): sum of (ref/255 - clamp(x_hat, 0, 1))^2, what the reference's compute_psnr(x, x_hat.clamp(0, 1)) averages.
    Both are device tensors; psnr() and psnr_8bit() read them back once (one copy for both) and compute in Python doubles."""

    def __init__(self, sums, H, W):
        import torch
        self._sums = sums                                   # int64 [2][B][3]: [0] the integer sums, [1] the bits of the float64 sums
        self.sse_u8 = sums[0]
        self.sse_f = sums[1].view(torch.float64)
        self.H, self.W = H, W
        self._host = None

    def _read(self):
        if self._host is None:
            h = self._sums.cpu()
            import torch
            self._host = (h[0].tolist(), h[1].view(torch.float64).tolist())
        return self._host

    def psnr(self):
        """per image: -10 log10(sum_c sse_f / (3 H W)), inf at 0 (training/step.py:13-18 on the clamped, un-padded x_hat)"""
        n = 3 * self.H * self.W
        return [psnr_from_sse(r[0] + r[1] + r[2], n) for r in self._read()[1]]

    def psnr_8bit(self):
        """per image: 10 log10(255^2 3 H W / sum_c sse_u8), the PSNR of the 8-bit images; inf at 0"""
        n = 3 * self.H * self.W
        return [10.0 * math.log10(65025.0 * n / (r[0] + r[1] + r[2])) if r[0] + r[1] + r[2] > 0 else float("inf") for r in self._read()[0]]


def from_model_output(x_hat, geom, layout="hwc", rounding="nearest", ref=None, ref_layout=None, image=True):
    """x_hat: float32 cuda [B,3,Hp,Wp] (or [3,Hp,Wp]; any batch / channel / row strides, unit stride along W) -> uint8 [B,H,W,3] ("hwc")
    or [B,3,H,W] ("chw") (without the batch axis for a 3-D x_hat): the window geom of x_hat, clamped to [0, 1], times 255, rounded
    half to even ("nearest") or towards zero ("trunc": the reference's ToPILImage, mul(255).byte()).  With ref (the original uint8
    image in ref_layout, default `layout`) returns (image, Distortion); with image=False (needs ref) no image is allocated or written
    and the Distortion alone is returned."""
    import torch
    if not image and ref is None:
        raise ValueError("image=False leaves nothing to compute without ref")
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be 'hwc' or 'chw', got {layout!r}")
    if rounding not in ROUNDINGS:
        raise ValueError(f"rounding must be 'nearest' or 'trunc', got {rounding!r}")
    if not torch.is_tensor(x_hat):
        raise TypeError("x_hat must be a tensor")
    if x_hat.dtype != torch.float32:
        raise TypeError(f"x_hat must be float32, got {x_hat.dtype}")
    if x_hat.dim() not in (3, 4):
        raise ValueError(f"x_hat must be [B,3,Hp,Wp] or [3,Hp,Wp], got {tuple(x_hat.shape)}")
    x4 = x_hat if x_hat.dim() == 4 else x_hat.unsqueeze(0)
    geom = Geometry(*geom)
    if x4.shape[1] != 3 or tuple(x4.shape[2:]) != (geom.Hp, geom.Wp) or x4.shape[0] < 1:
        raise ValueError(f"x_hat must be [B,3,{geom.Hp},{geom.Wp}] for {geom}, got {tuple(x_hat.shape)}")
    if geom.H < 1 or geom.W < 1 or geom.top < 0 or geom.left < 0 or geom.top + geom.H > geom.Hp or geom.left + geom.W > geom.Wp:
        raise ValueError(f"{geom}: the window lies outside the planes")
    B, H, W = x4.shape[0], geom.H, geom.W
    rview = (None, 0, 0, 0, 0)
    if ref is not None:
        ref_layout = layout if ref_layout is None else ref_layout
        r4, rview = _u8_view(ref, ref_layout, "ref")
        if r4.shape[0] != B or _hw(r4, ref_layout) != (H, W) or r4.device != x4.device:
            raise ValueError(f"ref must hold {B} image(s) of {H}x{W} on {x4.device}, got {tuple(ref.shape)} on {ref.device}")
    if x_hat.device.type != "cuda":
        raise ValueError(f"x_hat must be on a GPU (there is no CPU fallback), got {x_hat.device}")
    if x4.stride(3) != 1 or x4.stride(2) < geom.Wp or min(x4.stride()[:2]) < 1:
        x4 = x4.contiguous()
    L = lib()
    with torch.cuda.device(x4.device):
        out, oview = None, (None, 0, 0, 0, 0)
        if image:
            out = torch.empty((B, H, W, 3) if layout == "hwc" else (B, 3, H, W), dtype=torch.uint8, device=x4.device)
            oview = (out.data_ptr(), LAYOUTS[layout], out.stride(0), 0 if layout == "hwc" else out.stride(1),
                     out.stride(1 if layout == "hwc" else 2))
        ws = sums = None
        nbytes = 0
        if ref is not None:
            nbytes = L.pc_pixels_emit_workspace_size(B, H, W)
            ws = torch.empty(nbytes // 8, dtype=torch.int64, device=x4.device)
            sums = torch.empty((2, B, 3), dtype=torch.int64, device=x4.device)
        rc = L.pc_pixels_emit_u8(x4.data_ptr(), x4.stride(0), x4.stride(1), x4.stride(2), geom.Hp, geom.Wp, geom.top, geom.left, B, H, W,
                                 ROUNDINGS[rounding], *oview, *rview, ws.data_ptr() if ws is not None else None, nbytes,
                                 sums[0].data_ptr() if sums is not None else None, sums[1].data_ptr() if sums is not None else None,
                                 torch.cuda.current_stream(x4.device).cuda_stream)
    if rc != PC_OK:
        raise PixelsError(rc, "pc_pixels_emit_u8")
    if not image:
        return Distortion(sums, H, W)
    if x_hat.dim() == 3:
        out = out[0]
    return (out, Distortion(sums, H, W)) if ref is not None else out


def plan(op, u8, layout, f32, geom, ref=None, ref_layout=None):
    """pc_pixels_plan for tensors (host only, nothing is launched or copied): True where the ingest (op = INGEST: u8 the source, f32 the
    padded destination) or the emit (op = EMIT: u8 the destination, f32 x_hat) of exactly these tensors takes the wide-access path.
    u8 and ref are 4-D uint8 tensors whose strides already fit a view (unit stride along the channel / column axis)."""
    def view(t, lay):
        return ((t.data_ptr(), 0, t.stride(0), 0, t.stride(1)) if lay == "hwc" else (t.data_ptr(), 1, t.stride(0), t.stride(1), t.stride(2)))
    geom = Geometry(*geom)
    rl = layout if ref_layout is None else ref_layout
    wide = C.c_int(-1)
    rc = lib().pc_pixels_plan(op, *view(u8, layout), f32.data_ptr(), f32.stride(0), f32.stride(1), f32.stride(2), geom.top, geom.left,
                              f32.shape[0], geom.H, geom.W, *(view(ref, rl) if ref is not None else (None, 0, 0, 0, 0)), C.byref(wide))
    if rc != PC_OK:
        raise PixelsError(rc, "pc_pixels_plan")
    return bool(wide.value)


def encode_image(model, img, qualities, mask_pol="point-based-std", layout="hwc"):
    """uint8 cuda image(s) -> PCB1 container(s) holding every level of `qualities` (container.pack with the un-padded size in the
    header): `bytes` for one image ([H,W,3] / [3,H,W]), a list with one `bytes` per image for a batch ([B,H,W,3] / [B,3,H,W]; one size
    per batch, as the codec's batch is).  model: a loaded ChannelProgresssiveWACNN (any topology / post-filter setting)."""
    from . import container
    qualities = [float(q) for q in qualities]
    x, geom = to_model_input(img, layout)
    datas = model.compress_levels(x, qualities, mask_pol=mask_pol)
    strings = [d["strings"] for d in datas]
    bufs = [container.pack(strings, datas[0]["shape"], qualities, image_size=(geom.H, geom.W), mask_pol=mask_pol, image_index=b)
            for b in range(x.shape[0])]
    return bufs[0] if img.dim() == 3 else bufs


def decode_image(model, buf, level=-1, layout="hwc", rounding="nearest"):
    """One level (index into the container's quality list, negative from the end) of a PCB1 container -> uint8 [H,W,3] ("hwc") or
    [3,H,W] ("chw") on the model's device, at the size the header records.  Only the header, the base segment and that level's segment
    are read, so a truncated container still decodes the levels it holds completely (ContainerError for the others).  A header whose
    latent shape is not the one padding(H, W) gives is refused."""
    from . import container
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be 'hwc' or 'chw', got {layout!r}")
    if rounding not in ROUNDINGS:
        raise ValueError(f"rounding must be 'nearest' or 'trunc', got {rounding!r}")
    hd = container.parse_header(buf)
    n = len(hd["qualities"])
    lv = int(level) + n if int(level) < 0 else int(level)
    if not 0 <= lv < n:
        raise container.ContainerError(f"no level {level} among {n}")
    H, W = hd["image_size"]
    if H < 1 or W < 1:
        raise container.ContainerError(f"corrupt header: image size {H}x{W}")
    geom = padding(H, W)
    if tuple(hd["shape"]) != (geom.Hp // 64, geom.Wp // 64):
        raise container.ContainerError(f"header shape {tuple(hd['shape'])} is not that of a {H}x{W} image padded to {geom.Hp}x{geom.Wp}")
    strings, shape, qs, _, mask_pol = container.unpack(buf, levels=[lv])
    x_hat = model.decompress(strings[0], shape, qs[0], mask_pol)["x_hat"]
    return from_model_output(x_hat, geom, layout=layout, rounding=rounding)[0]

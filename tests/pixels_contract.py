"""The image-domain layer (progressivecodec_amd/pixels.py, pixels_csrc/pc_pixels.h) restated in numpy from its definition (DESIGN.md
section 10), not from the kernels: what tests/test_pixels_host.py checks against torch and tests/test_gpu_pixels.py checks the GPU against.

Images are uint8 arrays [B,H,W,3] ("hwc") or [B,3,H,W] ("chw"); planes are float32 [B,3,Hp,Wp].
"""
import math

import numpy as np

F255 = np.float32(255.0)


def geometry(h, w, multiple=64):
    """(Hp, Wp, top, left): each axis padded up to the next multiple, the image centred, the odd row / column at the bottom / right"""
    hp = -(-h // multiple) * multiple
    wp = -(-w // multiple) * multiple
    return hp, wp, (hp - h) // 2, (wp - w) // 2


def to_chw(img, layout):
    if layout not in ("hwc", "chw"):
        raise ValueError(layout)
    return np.ascontiguousarray(img.transpose(0, 3, 1, 2)) if layout == "hwc" else np.asarray(img)


def from_chw(img, layout):
    if layout not in ("hwc", "chw"):
        raise ValueError(layout)
    return np.ascontiguousarray(img.transpose(0, 2, 3, 1)) if layout == "hwc" else np.asarray(img)


def unit(u8):
    """the correctly rounded float32 quotient v / 255 (IEEE division of two float32 values)"""
    return np.asarray(u8).astype(np.float32) / F255


def ingest(img, layout, hp, wp, top, left):
    x = unit(to_chw(img, layout))
    B, _, H, W = x.shape
    out = np.zeros((B, 3, hp, wp), np.float32)
    out[:, :, top:top + H, left:left + W] = x
    return out


def clamp01(v):
    """fminf(fmaxf(v, 0), 1): NaN -> 0"""
    return np.fmin(np.fmax(np.asarray(v, np.float32), np.float32(0)), np.float32(1))


def quantise(c, rounding):
    s = (c * F255).astype(np.float32)
    if rounding == "nearest":
        q = np.rint(s)
    elif rounding == "trunc":
        q = np.trunc(s)
    else:
        raise ValueError(rounding)
    return q.astype(np.uint8)


def emit(x, top, left, H, W, rounding, layout):
    """x: float32 [B,3,Hp,Wp] -> uint8 image of the window in `layout`"""
    c = clamp01(x[:, :, top:top + H, left:left + W])
    return from_chw(quantise(c, rounding), layout)


def sums(x, top, left, H, W, rounding, ref, ref_layout):
    """(sse_u8 [B][3] of Python ints, sse_f [B][3] of floats): sum (q - ref)^2 in integers; sum (ref/255 - c)^2 with the difference in
    float32, the square in float64 (exact) and the sum exact, rounded once (math.fsum)"""
    c = clamp01(x[:, :, top:top + H, left:left + W])
    q = quantise(c, rounding).astype(np.int64)
    r = to_chw(ref, ref_layout)
    e = q - r.astype(np.int64)
    d = (unit(r) - c).astype(np.float32).astype(np.float64)
    B = c.shape[0]
    sse_u8 = [[int((e[b, ch] * e[b, ch]).sum()) for ch in range(3)] for b in range(B)]
    sse_f = [[math.fsum((d[b, ch] * d[b, ch]).ravel().tolist()) for ch in range(3)] for b in range(B)]
    return sse_u8, sse_f


def psnr(sse_f_row, H, W):
    s = sse_f_row[0] + sse_f_row[1] + sse_f_row[2]
    return -10.0 * math.log10(s / (3 * H * W)) if s > 0 else float("inf")


def psnr_8bit(sse_u8_row, H, W):
    s = sse_u8_row[0] + sse_u8_row[1] + sse_u8_row[2]
    return 10.0 * math.log10(255.0 ** 2 * 3 * H * W / s) if s > 0 else float("inf")


def exact_ties():
    """float32 values v in (0, 1) whose float32 product v * 255 is exactly k + 0.5"""
    out = []
    for k in range(255):
        v0 = np.float32((k + 0.5) / 255.0)
        for v in (np.nextafter(v0, np.float32(0)), v0, np.nextafter(v0, np.float32(1))):
            if np.float32(v * F255) == np.float32(k + 0.5):
                out.append(np.float32(v))
    return np.array(out, np.float32)


def hostile_planes(ref_chw, hp, wp, top, left, seed):
    """Decoder-like planes for an emit test: the ingest of `ref` plus noise, with values below 0, above 1, +-inf, NaN, -0.0 and exact
    ties sprinkled over it, padding included."""
    rng = np.random.default_rng(seed)
    B, _, H, W = ref_chw.shape
    x = ingest(ref_chw, "chw", hp, wp, top, left)
    x = (x + rng.normal(0, 0.05, x.shape).astype(np.float32)).astype(np.float32)
    flat = x.reshape(-1)
    ties = exact_ties()
    special = np.concatenate([np.array([-0.0, 0.0, 1.0, -1.5, 2.5, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 0.5, 1 - 2.0 ** -24],
                                       np.float32), ties])
    n = min(flat.size, max(len(special), flat.size // 7))
    idx = rng.choice(flat.size, n, replace=False)
    flat[idx] = special[np.arange(n) % len(special)]
    return x

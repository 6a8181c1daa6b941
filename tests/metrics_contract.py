"""The metrics kernels (progressivecodec_amd/metrics_csrc/pc_metrics.hip: msssim_scale_kernel<WS>, pool2x2_kernel, msssim_final_kernel)
restated on the CPU, for tests/test_gpu_metrics_matrix.py (GPU) and tests/test_metrics_contract_host.py (no GPU).  Never imported by
product code.

  restate(c, d)       the float32 contract of DESIGN.md section 9 (oracle/pc_oracle.c orc_msssim: fmaf chains with the taps in order, f64
                      sums in the stated order): per-tile (ssim, cs) pairs, pooled planes, per-(scale, image, channel) means, the value.
                      The GPU must return these bits (the value: within one float32 ulp, device pow is not correctly rounded).
  reference64(c, d)   the definition in float64, written from the formulae (not from the kernel), and a bound on a float32 evaluation.
  ws_layout(c)        the workspace layout restated independently of the library's geometry().
  matrix()            the cases, each with the staging path per scale (`vec`) it is written to reach; REQUIRED the coverage set.

How the bound is derived (never fitted).  U = 2^-24, fl(a op b) = (a op b)(1 + e), |e| <= U.  First-order terms; the factor 2 at the end
covers their products (as stage_contract does).
  window    t_k = expf(-d^2 / two_s2): the argument carries two roundings (two_s2, the quotient), 2 U |arg| relative on exp, expf itself
            within 1 ulp (2 U): rho_k = 2 U |arg_k| + 2 U.  S = fl(sum t_k) has the t-weighted mean of rho_k plus U; the quotient U:
            tau_k = rho_k + rho_bar + 2 U relative on g_k, plus 2^-149 absolute (a subnormal t_k).
  moments   v in (X, Y, X*X, Y*Y, X*Y): the product is one rounding (U |v|, none for X, Y); each pass is a chain of n = win_size fmaf,
            within n U sum |terms|: (c_m + 2 n) U G*|v|.  The tap errors add (g tau (x) g + g (x) g tau) * |v|.  An input error e_x of a
            pooled plane adds G * e_v with e_(x*x) = 2 |x| e_x, e_(x*y) = |x| e_y + |y| e_x.
  maps      mu^2 and mu1 mu2: the product rule plus U of the result.  s = G*(X.X) - mu^2: e(moment) + e(mu^2) + U |s|: the subtraction
            is paid for ABSOLUTELY, which is where mu^2 / (sigma^2 + C2) enters.  C = (K L)(K L): 3 U C.  Sums: the operands' errors plus
            U of the result.  A quotient n / d: e_n / d_lo + |n| e_d / (d_lo |d|) + U |n / d| with d_lo = |d| - e_d; where d_lo <= 0 the
            float32 quotient is not bounded by the operation (data_range = 0 on flat regions) and the bound is +inf.
  means     the mean of the pixel bounds (the f64 sums add at most 2^-50 relative to the mean of |values|).
  pool      three additions, the product with 0.25 exact: e' = pool(e) + 3 U pool(|x|).
  value     intervals: relu and m -> m^w are monotone, the product of non-negative intervals is the product of the ends, the channel mean is
            monotone; plus U |value| for the rounding to float32.  No derivative of m^w at 0 is needed.
Where the reference or the bound is not finite (a NaN or Inf in the image, 0 / 0 at data_range = 0) the float64 check says nothing and the
bit comparison with the restatement is the whole check; `check64` reports how many values that concerns.
"""
import ctypes as C
import os
import re
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import liboracle as lo

F32 = np.float32
U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP32, SENT32 = 0x7FE1A5A5, 0x7FE2B6B6       # quiet NaNs of a distinctive payload: input gaps / workspace and output sentinels
GUARD = 1024                                  # bytes on both sides of the workspace, `out` and `out_scales`
LEAD = 64                                     # floats of NaN before every input view (keeps a 256-byte aligned base aligned)
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
PC_ERR_ARG, PC_ERR_BUFFER = -1, -3
MISREADINGS = ("window_unnormalised", "pool_zero_one_side", "pool_divisor_valid", "relu_per_pixel", "cs_last_scale", "mean_over_HW",
               "c1_c2_swapped", "k2l")

REQUIRED = ({("win", w) for w in range(1, 32, 2)} | {("vec0", 0), ("vec0", 1), ("vecp", 0), ("vecp", 1), ("C", "le64"), ("C", "gt64")} |
            {("levels", n) for n in range(1, 6)})


def reached(c):
    """the REQUIRED entries a passing case accounts for"""
    r = {("win", c["ws"]), ("vec0", c["vec"][0]), ("C", "gt64" if c["C"] > 64 else "le64"), ("levels", c["levels"])}
    return r | {("vecp", v) for v in c["vec"][1:]}


# -- the cases -----------------------------------------------------------------------------------------------------------------------

def _up4(n):
    return (n + 3) // 4 * 4


def contiguous(c):
    H, W, Cc = c["H"], c["W"], c["C"]
    return dict(lead=0, sh=W, sc=H * W, sb=Cc * H * W)


def padded(c, lead=0, dh=0, dc=0, db=0):
    """rows, planes and images each a multiple of four floats apart, plus dh / dc / db"""
    sh = _up4(c["W"]) + 4 + dh
    sc = _up4(c["H"] * sh) + 8 + dc
    sb = _up4(c["C"] * sc) + 12 + db
    return dict(lead=lead, sh=sh, sc=sc, sb=sb)


def case(name, group, B, Cc, H, W, ws, levels, vec, sigma=1.5, weights=None, K=(0.01, 0.03), L=1.0, nonneg=False, data="noise", xl=None,
         yl=None, big=False, twin=None):
    if levels > 1 and weights is None:
        weights = MS_WEIGHTS[:levels]
    c = dict(name=name, group=group, B=B, C=Cc, H=H, W=W, ws=ws, levels=levels, vec=tuple(vec), sigma=sigma,
             weights=None if levels == 1 else tuple(weights), K=K, L=L, nonneg=nonneg, data=data, big=big, twin=twin)
    c["xl"] = xl(c) if callable(xl) else (xl or contiguous(c))
    c["yl"] = yl(c) if callable(yl) else (yl or contiguous(c))
    assert len(c["vec"]) == levels
    return c


def matrix():
    m = []
    # SSIM at every window instantiation: one output pixel (contiguous, W odd: the scalar path) and output extents on and around the
    # 32 x 64 tile edges (padded rows, 16-byte path: the float4 load that straddles W falls back per element)
    HO, WO = (31, 32, 33, 64, 65), (63, 64, 65, 128, 129)
    for i, ws in enumerate(range(1, 32, 2)):
        m.append(case(f"ssim_w{ws}_one_pixel", "ssim", 2, 3, ws, ws, ws, 1, (0,), nonneg=bool(i & 1), data=("anti", "noise")[i % 2],
                      sigma=(0.5, 1.5, 5.0)[i % 3]))
        m.append(case(f"ssim_w{ws}_edges", "ssim", 1, 2, HO[i % 5] + ws - 1, WO[(i + i // 5) % 5] + ws - 1, ws, 1, (1,), nonneg=not (i & 1),
                      data=("noise", "anti", "smooth_noise")[i % 3], sigma=(1.5, 5.0, 0.5)[i % 3], L=(1.0, 255.0)[i % 2], xl=padded,
                      yl=padded))
    # MS-SSIM: windows, level counts, sigmas, weights (a zero weight among them), the size rule's edge (min side = 16 (ws - 1) + 1)
    m += [case("ms_w3_l2_rule_edge", "ms", 2, 3, 33, 35, 3, 2, (0, 0), sigma=0.5, weights=(0.4, 0.6)),
          case("ms_w3_l5_odd_every_scale", "ms", 1, 3, 33, 65, 3, 5, (0, 0, 0, 0, 0), sigma=0.5),             # 33 17 9 5 3 x 65 33 17 9 5
          case("ms_w3_l3_vec_110", "ms", 2, 1, 40, 104, 3, 3, (1, 1, 0), weights=(0.3, 0.5, 0.2)),            # W 104 52 26
          case("ms_w3_l3_vec_010", "ms", 2, 1, 40, 103, 3, 3, (0, 1, 0), weights=(0.2, 0.2, 0.6)),            # W 103 52 26
          case("ms_w3_l4_vec_1100", "ms", 1, 2, 66, 200, 3, 4, (1, 1, 0, 0), sigma=5.0),                       # W 200 100 50 25, H 66 33 17 9
          case("ms_w7_l3", "ms", 2, 3, 97, 120, 7, 3, (1, 1, 0), weights=(0.3, 0.5, 0.2), data="smooth_noise"),   # 49 x 60, 25 x 30
          case("ms_w7_l4_zero_weight", "ms", 1, 3, 100, 113, 7, 4, (0, 0, 0, 0), weights=(0.2, 0.0, 0.5, 0.3)),
          case("ms_w11_l5_q8_255", "ms", 2, 3, 161, 176, 11, 5, (1, 1, 1, 0, 0), L=255.0, data="quant8"),      # 161x176 81x88 41x44 21x22 11x11
          case("ms_w11_l4_noise", "ms", 1, 1, 163, 161, 11, 4, (0, 0, 0, 0)),
          case("ms_w15_l2_sigma5", "ms", 1, 2, 225, 232, 15, 2, (1, 1), sigma=5.0, weights=(0.7, 0.3)),        # 113 x 116
          case("ms_w31_l5_sigma5", "ms", 1, 1, 481, 483, 31, 5, (0, 0, 0, 0, 0), sigma=5.0),
          case("ms_w31_l2_sigma05", "ms", 1, 1, 484, 481, 31, 2, (0, 0), sigma=0.5, weights=(0.5, 0.5), data="smooth_noise")]
    # channel passes of the final kernel (64 channels per pass) and batch sizes
    m += [case("ms_c64_b1", "channels", 1, 64, 40, 40, 3, 2, (1, 1), weights=(0.4, 0.6)),
          case("ms_c65_b2", "channels", 2, 65, 40, 40, 3, 2, (1, 1), weights=(0.4, 0.6)),
          case("ms_c130_b1_l3", "channels", 1, 130, 40, 35, 3, 3, (0, 0, 0), weights=(0.2, 0.3, 0.5)),
          case("ms_c1_b5", "channels", 5, 1, 35, 40, 3, 2, (1, 1), weights=(0.5, 0.5)),                        # 18 x 20
          case("ssim_c130_b2", "channels", 2, 130, 13, 70, 5, 1, (0,), nonneg=True, data="anti")]
    # tiles per plane: more than 64 (the lane-strided sum of the final kernel), and the pool's grid-stride loop (> 8192 * 256 outputs)
    m += [case("ms_72_tiles", "tiles", 1, 1, 290, 464, 3, 2, (1, 1), weights=(0.5, 0.5)),                      # 288 x 462 outputs: 9 x 8 tiles
          case("ssim_130_tiles", "tiles", 1, 1, 330, 650, 11, 1, (0,), xl=lambda c: padded(c, dh=1)),        # 320 x 640: 10 x 10
          case("ssim_100_tiles_wide_range", "tiles", 1, 1, 330, 650, 11, 1, (0,), L=0.0, data="wide"),      # f64 sums that round
          case("ms_big_frame", "tiles", 1, 1, 2201, 3901, 11, 5, (0, 0, 1, 1, 1), big=True)]          # 551 x 976, 276 x 488, 138 x 244
    # strides: 2 x 3 x 40 x 36, ws 3, two levels (pooled 20 x 18: scalar)
    s = dict(B=2, Cc=3, H=40, W=36, ws=3, levels=2, weights=(0.4, 0.6))
    m += [case("stride_x_padded_y_contig", "strides", vec=(1, 0), xl=padded, **s),
          case("stride_y_padded_x_contig", "strides", vec=(1, 0), yl=padded, **s),
          case("stride_both_different", "strides", vec=(0, 0), xl=lambda c: padded(c, lead=3, dh=1), yl=lambda c: padded(c, dc=2, db=5), **s),
          case("stride_batch_step", "strides", vec=(1, 0), xl=lambda c: dict(lead=0, sh=36, sc=1440, sb=2 * 3 * 1440), **s),      # t[::2]
          case("stride_channel_slice", "strides", vec=(1, 0), yl=lambda c: dict(lead=1440, sh=36, sc=1440, sb=5 * 1440), **s)]   # t[:, 1:4] of 5
    # each of the eight preconditions of the 16-byte path broken alone, against the aligned twin (same data, same bits)
    m.append(case("vec_twin", "vec", vec=(1, 0), xl=padded, yl=padded, data="noise@vec", **s))
    for who in ("x", "y"):
        for what, kw in (("base", dict(lead=1)), ("sh", dict(dh=1)), ("sc", dict(dc=1)), ("sb", dict(db=1))):
            lay = {who + "l": (lambda c, kw=kw: padded(c, **kw)), ("y" if who == "x" else "x") + "l": padded}
            m.append(case(f"vec_break_{who}_{what}", "vec", vec=(0, 0), data="noise@vec", twin="vec_twin", **lay, **s))
    # data
    d = dict(B=2, Cc=2, H=40, W=48, ws=3, levels=2, weights=(0.4, 0.6), vec=(1, 1))
    m += [case("data_range_0", "data", L=0.0, **d), case("data_range_0_const", "data", L=0.0, data="const", **d),
          case("data_identical", "data", data="identical", **d), case("data_anti", "data", data="anti", **d),
          case("data_const_255", "data", L=255.0, data="const", **d),
          case("data_flat_bright", "data", 1, 1, 181, 203, 11, 5, (0, 0, 0, 0, 0), L=255.0, data="flat_bright"),
          case("data_nan_image", "data", 3, 2, 40, 48, 3, 2, (1, 1), weights=(0.4, 0.6), data="nan_image"),
          case("data_inf_image", "data", 3, 2, 40, 48, 3, 2, (1, 1), weights=(0.4, 0.6), data="inf_image"),
          case("ssim_nan_image", "data", 3, 1, 20, 24, 5, 1, (1,), data="nan_image")]
    assert len({c["name"] for c in m}) == len(m)
    return m


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def make_data(c):
    """X, Y [B, C, H, W] float32 in [0, L] (L = 1 when data_range is 0)"""
    kind, _, key = c["data"].partition("@")
    g = _rng(key or c["name"])
    shape = (c["B"], c["C"], c["H"], c["W"])
    L = c["L"] or 1.0
    x = g.random(shape)
    if kind in ("smooth_noise", "quant8"):
        yy, xx = np.meshgrid(np.arange(c["H"]), np.arange(c["W"]), indexing="ij")
        f = g.random((c["B"], c["C"], 4, 1, 1))
        x = 0.5 + 0.22 * np.sin(0.02 * (1 + 5 * f[:, :, 0]) * yy + 6 * f[:, :, 1]) + 0.22 * np.cos(0.02 * (1 + 5 * f[:, :, 2]) * xx + 6 * f[:, :, 3])
    if kind == "noise":
        y = g.random(shape)
    elif kind == "smooth_noise":
        y = x + 0.05 * g.standard_normal(shape)
    elif kind == "quant8":
        x = x + 0.02 * g.standard_normal(shape)
        y = np.round(np.clip(x, 0, 1) * 255) / 255
    elif kind == "identical":
        y = x
    elif kind == "anti":
        y = 1 - x
    elif kind == "const":
        x = np.full(shape, 0.7)
        y = np.full(shape, 0.4)
    elif kind == "flat_bright":
        x = np.full(shape, 0.9)
        y = x + (0.3 / 255) * g.standard_normal(shape)
    elif kind in ("nan_image", "inf_image"):
        y = g.random(shape)
    elif kind == "wide":                                  # map values over 60 binades inside every tile: the f64 sums are inexact,
        y = g.random(shape) * 2.0 ** (-30 * (np.arange(c["W"]) % 64) / 63)         # so the order of the tile sum shows in the bits
    else:
        raise KeyError(kind)
    X, Y = (x * L).astype(F32), (y * L).astype(F32)
    if kind == "flat_bright":
        X[:] = F32(229.5)
    if kind in ("nan_image", "inf_image"):                # image 1, channel 0: one pixel in the middle of X
        X[1, 0, c["H"] // 2, c["W"] // 2] = np.nan if kind == "nan_image" else np.inf
    return dict(X=X, Y=Y)


def place(arr, lay):
    """(buffer of uint32 words, element offset of the view, index array [B, C, H, W]): the tensor at its strides, LEAD words of NaN
    before it, every gap and 64 words after it a quiet NaN"""
    B, Cc, H, W = arr.shape
    b, ch, h, w = np.ogrid[:B, :Cc, :H, :W]
    index = LEAD + lay["lead"] + b * lay["sb"] + ch * lay["sc"] + h * lay["sh"] + w
    assert np.unique(index).size == index.size, "overlapping view"
    buf = np.full(int(index.max()) + 1 + 64, GAP32, np.uint32)
    buf[index] = arr.view(np.uint32)
    return buf, LEAD + lay["lead"], index


# -- the restatement -------------------------------------------------------------------------------------------------------------------

def restate(c, d, variant=0):
    return lo.msssim(d["X"], d["Y"], c["L"], c["ws"], c["sigma"], c["K"], c["weights"], c["nonneg"], variant)


def sizes(c):
    hw = [(c["H"], c["W"])]
    for _ in range(1, c["levels"]):
        hw.append(((hw[-1][0] + 1) // 2, (hw[-1][1] + 1) // 2))
    return hw


def ws_layout(c):
    """the workspace as pc_metrics.h describes it: the slab [scale][plane][tile] of f64 pairs, then per scale >= 1 the pooled X and the
    pooled Y, every array on a 256-byte boundary.  Byte offsets; `pad` the byte ranges no kernel may write."""
    P, n = c["B"] * c["C"], c["ws"]
    up = lambda v: -(-v // 256) * 256
    hw = sizes(c)
    tiles = [-(-(h - n + 1) // 32) * -(-(w - n + 1) // 64) for h, w in hw]
    slab_off, off = [], 0
    for t in tiles:
        slab_off.append(off)
        off += 16 * P * t
    pad = [(off, up(off))]
    off = up(off)
    pool = [None]
    for h, w in hw[1:]:
        nb = 4 * P * h * w
        pool.append((off, off + up(nb)))
        pad += [(off + nb, off + up(nb)), (off + up(nb) + nb, off + 2 * up(nb))]
        off += 2 * up(nb)
    return dict(tiles=tiles, slab_off=slab_off, pool=pool, pad=pad, total=off, hw=hw)


def expected_workspace(c, r):
    """the workspace image (uint8) after a call: sentinel-filled, the restatement's slabs and pooled planes at their places; and a mask of
    the words that hold values (for NaN-aware comparison)"""
    lay = ws_layout(c)
    P = c["B"] * c["C"]
    img = np.full(lay["total"] // 4, SENT32, np.uint32).view(np.uint8)
    for s, t in enumerate(lay["tiles"]):
        a = np.ascontiguousarray(r["slab"][s]).view(np.uint8).reshape(-1)
        assert a.size == 16 * P * t
        img[lay["slab_off"][s]:lay["slab_off"][s] + a.size] = a
        if s:
            for off, pl in zip(lay["pool"][s], r["pooled"][s - 1]):
                a = np.ascontiguousarray(pl).view(np.uint8).reshape(-1)
                img[off:off + a.size] = a
    return img, lay


def same_bits(got, want, dtype):
    """elementwise: the same bits, or both NaN (a NaN's payload is not part of the contract)"""
    g, w = np.ascontiguousarray(got).reshape(-1).view(dtype), np.ascontiguousarray(want).reshape(-1).view(dtype)
    ui = np.uint32 if np.dtype(dtype).itemsize == 4 else np.uint64
    return (g.view(ui) == w.view(ui)) | (np.isnan(g) & np.isnan(w))


def compare_workspace(c, got_u8, r):
    """[] or the list of mismatches between a workspace read back and the restatement (regions NaN-aware, padding bit for bit)"""
    img, lay = expected_workspace(c, r)
    P, bad = c["B"] * c["C"], []
    for s, t in enumerate(lay["tiles"]):
        o, nb = lay["slab_off"][s], 16 * P * t
        ok = same_bits(got_u8[o:o + nb], img[o:o + nb], np.float64)
        if not ok.all():
            i = int(np.flatnonzero(~ok)[0])
            bad.append(f"slab scale {s}: {int((~ok).sum())} of {ok.size} f64 differ, first plane {i // (2 * t)} tile {i // 2 % t} "
                       f"{'cs' if i & 1 else 'ssim'}")
        if s:
            h, w = lay["hw"][s]
            for nm, o in zip("XY", lay["pool"][s]):
                ok = same_bits(got_u8[o:o + 4 * P * h * w], img[o:o + 4 * P * h * w], np.float32)
                if not ok.all():
                    i = int(np.flatnonzero(~ok)[0])
                    bad.append(f"pooled {nm} scale {s}: {int((~ok).sum())} of {ok.size} differ, first plane {i // (h * w)} row "
                               f"{i // w % h} column {i % w}")
    for a, b in lay["pad"]:
        if not np.array_equal(got_u8[a:b], img[a:b]):
            bad.append(f"padding bytes {a}..{b} were written")
    return bad


# -- the float64 reference -------------------------------------------------------------------------------------------------------------

def window64(n, sigma, misread=None):
    """(g, g*tau): the Gaussian of the definition in float64 and the bound on each float32 tap"""
    sigma = float(F32(sigma))
    d = np.arange(n, dtype=np.float64) - n // 2
    arg = d * d / (2 * sigma * sigma)
    t = np.exp(-arg)
    rho = 2 * U * arg + 2 * U
    tau = rho + float((t * rho).sum() / t.sum()) + 2 * U
    g = t if misread == "window_unnormalised" else t / t.sum()
    return torch.from_numpy(g), torch.from_numpy(g * tau + 2.0 ** -149)


def _filt(x, gh, gw):
    x = F.conv2d(x, gh.view(1, 1, -1, 1))
    return F.conv2d(x, gw.view(1, 1, 1, -1))


def _pool(x, misread=None):
    ph, pw = x.shape[2] % 2, x.shape[3] % 2
    if misread == "pool_zero_one_side":          # the zero after the plane only; the one before it is the one every window position uses
        return F.avg_pool2d(F.pad(x, (0, pw, 0, ph)), 2, 2)
    return F.avg_pool2d(x, 2, 2, padding=(ph, pw), count_include_pad=misread != "pool_divisor_valid")


def _quot(n, en, dn, ed):
    lo_ = dn.abs() - ed
    q = n / dn
    e = en / lo_ + n.abs() * ed / (lo_ * dn.abs()) + U * q.abs()
    return q, torch.where(lo_ > 0, e, torch.full_like(e, float("inf")))


def reference64(c, d, misread=None):
    """dict(means [levels, 2, B, C], means_bound, out [B], out_bound), float64 numpy"""
    B, Cc, n, levels = c["B"], c["C"], c["ws"], c["levels"]
    P = B * Cc
    x = torch.from_numpy(d["X"].astype(np.float64)).reshape(P, 1, c["H"], c["W"])
    y = torch.from_numpy(d["Y"].astype(np.float64)).reshape(P, 1, c["H"], c["W"])
    ex, ey = torch.zeros_like(x), torch.zeros_like(y)
    g, gt = window64(n, c["sigma"], misread)
    K1, K2, L = float(F32(c["K"][0])), float(F32(c["K"][1])), float(F32(c["L"]))
    C1, C2 = ((K1 * K1 * L, K2 * K2 * L) if misread == "k2l" else ((K1 * L) ** 2, (K2 * L) ** 2))
    if misread == "c1_c2_swapped":
        C1, C2 = C2, C1
    eC1, eC2 = 3 * U * C1, 3 * U * C2
    means, bounds = np.zeros((levels, 2, P)), np.zeros((levels, 2, P))
    for s in range(levels):
        ax, ay = x.abs(), y.abs()
        v = torch.cat([x, y, x * x, y * y, x * y])
        av = v.abs()
        w = torch.cat([2 * n * U * ax + ex, 2 * n * U * ay + ey, (1 + 2 * n) * U * av[2 * P:3 * P] + 2 * ax * ex,
                       (1 + 2 * n) * U * av[3 * P:4 * P] + 2 * ay * ey, (1 + 2 * n) * U * av[4 * P:] + ax * ey + ay * ex])
        M = _filt(v, g, g)
        E = _filt(w, g, g) + _filt(av, gt, g) + _filt(av, g, gt)
        m1, m2, m3, m4, m5 = M.split(P)
        e1, e2, e3, e4, e5 = E.split(P)
        mu1_sq, mu2_sq, mu12 = m1 * m1, m2 * m2, m1 * m2
        e11 = 2 * m1.abs() * e1 + U * mu1_sq
        e22 = 2 * m2.abs() * e2 + U * mu2_sq
        e12 = m1.abs() * e2 + m2.abs() * e1 + U * mu12.abs()
        s1, s2, s12 = m3 - mu1_sq, m4 - mu2_sq, m5 - mu12
        es1, es2, es12 = e3 + e11 + U * s1.abs(), e4 + e22 + U * s2.abs(), e5 + e12 + U * s12.abs()
        ncs, dcs = 2 * s12 + C2, s1 + s2 + C2
        encs = 2 * es12 + eC2 + U * ncs.abs()
        edcs = es1 + es2 + U * (s1 + s2).abs() + eC2 + U * dcs.abs()
        cs, ecs = _quot(ncs, encs, dcs, edcs)
        nl, dl = 2 * mu12 + C1, mu1_sq + mu2_sq + C1
        enl = 2 * e12 + eC1 + U * nl.abs()
        edl = e11 + e22 + U * (mu1_sq + mu2_sq) + eC1 + U * dl.abs()
        lum, el = _quot(nl, enl, dl, edl)
        ss = lum * cs
        ess = lum.abs() * ecs + cs.abs() * el + U * ss.abs()
        if misread == "relu_per_pixel":
            ss, cs = torch.relu(ss), torch.relu(cs)
        cnt = x.shape[2] * x.shape[3] if misread == "mean_over_HW" else ss.shape[2] * ss.shape[3]
        for k, (val, err) in enumerate(((ss, ess), (cs, ecs))):
            means[s, k] = (val.flatten(1).sum(1) / cnt).numpy()
            bounds[s, k] = (2 * err.flatten(1).sum(1) / cnt + 2.0 ** -50 * val.abs().flatten(1).sum(1) / cnt).numpy()
        if s + 1 < levels:
            ex, ey = _pool(ex) + 3 * U * _pool(ax), _pool(ey) + 3 * U * _pool(ay)
            x, y = _pool(x, misread), _pool(y, misread)
    means, bounds = means.reshape(levels, 2, B, Cc), bounds.reshape(levels, 2, B, Cc)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if levels == 1:
            relu = (lambda a: np.maximum(a, 0)) if c["nonneg"] else (lambda a: a)
            m, e = means[0, 0], bounds[0, 0]
            val, lo_, hi = relu(m), relu(m - e), relu(m + e)
        else:
            wts = np.asarray(c["weights"], F32).astype(np.float64)
            val, lo_, hi = np.ones((B, Cc)), np.ones((B, Cc)), np.ones((B, Cc))
            for s in range(levels):
                k = 1 if (s < levels - 1 or misread == "cs_last_scale") else 0
                m, e = means[s, k], bounds[s, k]
                a, b = np.maximum(m - e, 0) ** wts[s], np.maximum(m + e, 0) ** wts[s]
                val, lo_, hi = val * np.maximum(m, 0) ** wts[s], lo_ * np.minimum(a, b), hi * np.maximum(a, b)
        out = val.mean(1)
        ob = np.maximum(hi.mean(1) - out, out - lo_.mean(1)) * (1 + 2.0 ** -40) + U * np.abs(out)
    return dict(means=means, means_bound=bounds, out=out, out_bound=ob)


def check64(ref, means, out):
    """(ok, worst ratio over the bounded values, number of values the reference does not bound, text)"""
    worst, unbounded, bad = 0.0, 0, []
    for nm, got, want, bound in (("means", means, ref["means"], ref["means_bound"]), ("out", out, ref["out"], ref["out_bound"])):
        got = np.asarray(got, np.float64)
        with np.errstate(invalid="ignore"):
            fin = np.isfinite(want) & np.isfinite(bound)
            err = np.abs(got - want)
            miss = fin & ~(err <= bound)
            ratio = np.where(fin & (bound > 0), err / np.where(bound > 0, bound, 1), 0.0)
        unbounded += int((~fin).sum())
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
        if miss.any():
            i = np.unravel_index(int(np.argmax(np.where(miss, err / np.maximum(bound, 1e-300), 0))), got.shape)
            bad.append(f"{nm}{list(i)}: got {got[i]!r} want {want[i]!r} bound {bound[i]:.3g} ({int(miss.sum())} of {miss.size} outside)")
    return not bad, worst, unbounded, "; ".join(bad) or "inside"


# -- the plan's prototype ---------------------------------------------------------------------------------------------------------------

def header_prototype(name):
    """[ctype per parameter] of a PC_API function as metrics_csrc/pc_metrics.h declares it"""
    txt = open(os.path.join(ROOT, "progressivecodec_amd", "metrics_csrc", "pc_metrics.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    params = re.search(r"PC_API\s+int\s+" + name + r"\s*\((.*?)\)\s*;", txt, re.S).group(1)
    out = []
    for p in params.split(","):
        ty = re.fullmatch(r"(.*?)(\w+)", p.strip(), re.S).group(1).strip()
        out.append(C.c_void_p if ty.endswith("*") and ty != "int*" else
                   {"int": C.c_int, "float": C.c_float, "int64_t": C.c_int64, "size_t": C.c_size_t, "int*": C.POINTER(C.c_int)}[ty])
    return out

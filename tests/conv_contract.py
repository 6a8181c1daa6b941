"""The conv launcher (progressivecodec_amd/csrc/pc_conv.hip: pc_conv_launch) restated two ways, for the tests only -- product code never
imports this file.

A case is a plain dict (see `case()`): the input segments, the geometry (kind 0 conv k x k / 1 ConvTranspose2d(5, s2, p2, op1) / 2 the
192 -> 3 sub-pixel output layer), the epilogue and the output form.  `make_data` draws its operands; then

* `restate` is the numeric contract, bit-exact: the CPU oracle's fmaf chain (oracle.liboracle.conv_nhwc) over the
  concatenated channel axis, plus the bias, then the epilogue in numpy float32 one IEEE operation at a time with the contract's
  transcendental functions (oracle.liboracle.unary; the oracle is built with -ffp-contract=off), then the PixelShuffle / NCHW / slice
  placement;
* `reference64` is the operation itself in float64 (torch conv2d / conv_transpose2d / pixel_shuffle on CPU tensors; the sub-pixel layer
  as the real ConvTranspose2d on the original [Cin][3][5][5] weights) with a rigorous per-element error bound for a float32 evaluation:

      L_epi * K * 2^-24 * (|x| * |w| + |b|)  +  8 * 2^-24 * (magnitude of the epilogue's terms)  (+ 2^-140)

  K = taps * Cin + 1 (the chain plus the bias add), L_epi the epilogue's local slope.  A layout mistake (taps, channel order, phase,
  aux operand) moves an output by O(|x| |w|), orders of magnitude above the bound.

`mutate` names one deliberate mistake of the restatement; tests/test_conv_contract_host.py checks that each one leaves the bound.
tests/hostile_values.py is the table of the same shapes on operands outside the ordinary (subnormal, non-finite, overflowing chains).
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle.liboracle import conv_nhwc, unary

F32 = np.float32
U = 2.0 ** -24

EPI = dict(NONE=0, GELU=1, RES_GELU=2, RES=3, GATE=4, GDN=5, IGDN=6, CLAMP01=7, LRP=8, LRP_ADD=9, LEAKY=10, LEAKY_RES=11, RELU=12,
           SE_ADD=13)
EPI_NAME = {v: k for k, v in EPI.items()}
USES_AUX0 = {"RES_GELU", "RES", "GATE", "GDN", "IGDN", "LRP", "LRP_ADD", "LEAKY_RES", "SE_ADD"}
USES_AUX1 = {"GATE", "LRP_ADD", "SE_ADD"}
POSITIVE_PRE = {"GDN", "IGDN"}            # rsqrt / sqrt of the layer's output: operands drawn so that it stays >= 1

# include/pcodec.h PC_PLAN_* / PC_FORM_*
PLAN = dict(UNI_16_3=1, UNI_32_2=2, UNI_32_3=3, UNI_32_2_SQ=4, UNI_OTHER=5, L0_64x64=6, L0_64x64_SMALLC=7, L0_128x32=8,
            L0_128x32_SMALLC=9, L0_128x128=10, L0_128x128_SMALLC=11, IN_GDN=12)
FORM = dict(SLOW=1, DIRECT=2, TABLE=3, NCHW_PS=4, L0_DIRECT=5, L0_GENERIC=6, IN_GDN=7)
PLAN_NAME = {v: k for k, v in PLAN.items()}
FORM_NAME = {v: k for k, v in FORM.items()}

MUTATIONS = ("taps_flipped", "cin_cout_swapped", "ps_order", "se_per_pixel", "gate_aux_swapped", "subpixel_phase")


def case(name, B, H, W, segs=None, Cin=None, kind=0, k=3, stride=1, Cout=32, epi="NONE", out="nhwc", ldo=None, ooff=0,
         ps=False, relu=False, square=False, smallc=None, ngroup=1, fused_gdn=False, expect=None, seed=None):
    """segs: [(nch, ld, channel offset of the segment in its buffer)]; smallc: "nchw" / "nhwc" (Cin channels, element gather);
    out: "nhwc" (ldo >= Cout channels per pixel, this layer's channels start at ooff) or "nchw"; Cout: the layer's GEMM columns (kind 2:
    the 3 colours; the launch has 12); expect: (PLAN name, FORM name) the launcher must choose"""
    if smallc:
        segs = None
    else:
        Cin = sum(s[0] for s in segs)
    return dict(name=name, B=B, H=H, W=W, segs=segs, Cin=Cin, kind=kind, k=k if kind == 0 else 5, stride=stride if kind == 0 else 1,
                Cout=Cout, epi=epi, out=out, ldo=ldo, ooff=ooff, ps=ps, relu=relu, square=square, smallc=smallc, ngroup=ngroup,
                fused_gdn=fused_gdn, expect=expect, seed=seed if seed is not None else zlib.crc32(name.encode()))


# ---------------------------------------------------------------------------------------------------------------- geometry
def taps_of(c):
    """[(phase, oy, ox, [(dy, dx, weight tap (ky, kx))])] as the codec's tap tables order them"""
    if c["kind"] == 0:
        k = c["k"]
        return [(0, 0, 0, [(ky - k // 2, kx - k // 2, (ky, kx)) for ky in range(k) for kx in range(k)])]
    if c["kind"] == 1:
        out = []
        for py in range(2):
            for px in range(2):
                out.append((py * 2 + px, py, px, [((py + 2 - ky) // 2, (px + 2 - kx) // 2, (ky, kx))
                                                  for ky in range(py, 5, 2) for kx in range(px, 5, 2)]))
        return out
    return [(0, 0, 0, [(1 - t // 3, 1 - t % 3, t) for t in range(9)])]


def out_grid(c):
    """(Ho, Wo) of the GEMM, (outH, outW, channels) of the output tensor"""
    B, H, W = c["B"], c["H"], c["W"]
    if c["kind"] == 0:
        k, s = c["k"], c["stride"]
        Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
        oh, ow, oc = Ho, Wo, c["Cout"]
    elif c["kind"] == 1:
        Ho, Wo, oh, ow, oc = H, W, 2 * H, 2 * W, c["Cout"]
    else:
        Ho, Wo, oh, ow, oc = H, W, H, W, 12
    if c["ps"] or c["kind"] == 2:
        oh, ow, oc = 2 * oh, 2 * ow, oc // 4 if c["kind"] != 2 else 3
    return Ho, Wo, oh, ow, oc


def gemm_cout(c):
    return 12 if c["kind"] == 2 else c["Cout"]


def ktaps(c):
    return max(len(t[3]) for t in taps_of(c))


# ---------------------------------------------------------------------------------------------------------------- operands
def make_data(c):
    """seeded float32 operands of a case (host arrays): x [B,H,W,Cin] (the concatenated input), w (module layout), b, aux0, aux1, and
    the group-1 operands; GDN / IGDN cases draw x, w >= 0 and b >= 1"""
    rng = np.random.default_rng(c["seed"])
    B, H, W, Cin, Cout = c["B"], c["H"], c["W"], c["Cin"], c["Cout"]
    _, _, oh, ow, oc = out_grid(c)
    pos = c["epi"] in POSITIVE_PRE or c["square"] or c["fused_gdn"]
    K = ktaps(c) * Cin

    def draw_x():
        if c["fused_gdn"] or c["smallc"]:
            return rng.random((B, H, W, Cin)).astype(F32)
        return (rng.random((B, H, W, Cin)) if pos else rng.standard_normal((B, H, W, Cin))).astype(F32)

    def draw_w():
        shape = (Cout, Cin, c["k"], c["k"]) if c["kind"] == 0 else (Cin, Cout, 5, 5)
        if pos and not c["fused_gdn"]:
            return (rng.random(shape) / K).astype(F32)
        return (rng.standard_normal(shape) * (2.0 / K) ** 0.5).astype(F32)

    def draw_b():
        return (1.0 + rng.random(Cout)).astype(F32) if pos and not c["fused_gdn"] else (rng.standard_normal(Cout) * 0.1).astype(F32)

    d = dict(x=draw_x(), w=draw_w(), b=draw_b())
    if c["square"]:
        d["aux0"] = d["x"]                                  # GDN: the identity operand is the layer's own input (pc_codec.hip gdn())
    elif c["epi"] in USES_AUX0:
        d["aux0"] = rng.standard_normal((B, oh, ow, oc)).astype(F32)
    if c["epi"] in USES_AUX1:
        d["aux1"] = (rng.random((B, oc)) if c["epi"] == "SE_ADD" else rng.standard_normal((B, oh, ow, oc))).astype(F32)
    if c["fused_gdn"]:
        d["gamma"] = (rng.random((Cout, Cout)) * 0.01).astype(F32)   # re-parametrised GDN: gamma >= 0, beta >= 1
        d["beta"] = (1.0 + rng.random(Cout)).astype(F32)
    if c["ngroup"] == 2:
        d["x1"] = draw_x()
        d["w1"] = draw_w()
        d["b1"] = draw_b()
    return d


def pack_subpixel(w, mutate=None):
    """the weight transform of the sub-pixel layer, numpy: w [Cin][3][5][5] -> [9][12][Cin] (the GPU test packs with the library's
    pc_pack_conv_weight(kind = 2) and checks the two agree)"""
    Cin = w.shape[0]
    out = np.zeros((9, 12, Cin), F32)
    for t in range(9):
        dy, dx = 1 - t // 3, 1 - t % 3
        for n in range(12):
            ch, py, px = n >> 2, (n >> 1) & 1, n & 1
            if mutate == "subpixel_phase":
                py, px = px, py
            ky, kx = py + 2 - 2 * dy, px + 2 - 2 * dx
            if 0 <= ky < 5 and 0 <= kx < 5:
                out[t, n] = w[:, ch, ky, kx]
    return out


# ---------------------------------------------------------------------------------------------------------------- restatement
def _epilogue32(name, v, a0, a1, mutate=None):
    if name == "NONE":
        return v
    if name == "GELU":
        return unary(v, "gelu")
    if name == "RES_GELU":
        return unary((v + a0).astype(F32), "gelu")
    if name == "RES":
        return (a0 + v).astype(F32)
    if name == "GATE":
        if mutate == "gate_aux_swapped":
            a0, a1 = a1, a0
        return ((a0 * unary(v, "sigmoid")).astype(F32) + a1).astype(F32)
    if name == "GDN":
        return (a0 * unary(v, "rsqrt")).astype(F32)
    if name == "IGDN":
        return (a0 * unary(v, "sqrt")).astype(F32)
    if name == "CLAMP01":
        return np.where(v < 0, F32(0), np.where(v > 1, F32(1), v)).astype(F32)
    if name == "LRP":
        return (a0 + (F32(0.5) * unary(v, "tanh")).astype(F32)).astype(F32)
    if name == "LRP_ADD":
        return ((a0 + (F32(0.5) * unary(v, "tanh")).astype(F32)).astype(F32) + a1).astype(F32)
    if name == "LEAKY":
        return np.where(v > 0, v, (v * F32(0.01)).astype(F32)).astype(F32)
    if name == "LEAKY_RES":
        return (np.where(v > 0, v, (v * F32(0.01)).astype(F32)).astype(F32) + a0).astype(F32)
    if name == "RELU":
        return np.where(v > 0, v, F32(0)).astype(F32)
    if name == "SE_ADD":
        return (v + (a0 * a1).astype(F32)).astype(F32)
    raise ValueError(name)


def _se_scale(c, d, mutate=None):
    """aux1 of SE_ADD broadcast to [B, outH, outW, C]: the scale of (image, channel) -- or, mutated, of (pixel index mod B, channel)"""
    B = c["B"]
    _, _, oh, ow, oc = out_grid(c)
    s = d["aux1"]
    if mutate == "se_per_pixel":
        pix = np.arange(B * oh * ow) % B
        return s[pix].reshape(B, oh, ow, oc)
    return np.broadcast_to(s[:, None, None, :], (B, oh, ow, oc))


def _pixel_shuffle_nhwc(y, mutate=None):
    B, H, W, C4 = y.shape
    y = y.reshape(B, H, W, C4 // 4, 2, 2)                 # channel n = c*4 + py*2 + px
    if mutate == "ps_order":
        y = y.transpose(0, 1, 2, 3, 5, 4)
    y = y.transpose(0, 1, 4, 2, 5, 3)
    return np.ascontiguousarray(y.reshape(B, 2 * H, 2 * W, C4 // 4))


def _chains(c, x, w, b, mutate=None):
    """conv + bias in the GEMM's output space, float32 contract chains: [B, outH', outW', gemm Cout] before any PixelShuffle"""
    B, H, W = c["B"], c["H"], c["W"]
    Ho, Wo, _, _, _ = out_grid(c)
    Cin, Cout = c["Cin"], gemm_cout(c)
    if c["square"]:
        x = (x * x).astype(F32)
    sgn = -1 if mutate == "taps_flipped" else 1
    if c["kind"] == 0:
        k = c["k"]
        wt = np.ascontiguousarray(np.transpose(w, (2, 3, 1, 0)).reshape(k * k, Cin, Cout))
        if mutate == "cin_cout_swapped":
            wt = np.ascontiguousarray(np.transpose(w, (2, 3, 0, 1)).reshape(k * k, Cout, Cin))
        taps = [(sgn * dy, sgn * dx) for dy, dx, _ in taps_of(c)[0][3]]
        acc = conv_nhwc(x, wt, taps, c["stride"], Ho, Wo)
        return (acc + b).astype(F32)
    if c["kind"] == 1:
        acc = np.zeros((B, 2 * H, 2 * W, Cout), F32)
        for _, py, px, tl in taps_of(c):
            wt = np.ascontiguousarray(np.stack([w[:, :, ky, kx] for _, _, (ky, kx) in tl]))
            conv_nhwc(x, wt, [(sgn * dy, sgn * dx) for dy, dx, _ in tl], 1, H, W, out=acc, ostride=(2, 2), ooff=(py, px))
        return (acc + b).astype(F32)
    wp = pack_subpixel(w, mutate)                          # [9][12][Cin]
    wt = np.ascontiguousarray(wp.transpose(0, 2, 1))
    taps = [(sgn * dy, sgn * dx) for dy, dx, _ in taps_of(c)[0][3]]
    acc = conv_nhwc(x, wt, taps, 1, H, W)
    return (acc + np.repeat(b, 4)).astype(F32)


def restate(c, d, mutate=None, group=0):
    """the layer's output in the contract's float32, [B, outH, outW, C] NHWC (the output tensor's own values, before placement)"""
    x, w, b = (d["x1"], d["w1"], d["b1"]) if group == 1 else (d["x"], d["w"], d["b"])
    if group == 1:
        x = np.concatenate([d["x1"][..., :c["segs"][0][0]], d["x"][..., c["segs"][0][0]:]], axis=3)
    v = _chains(c, x, w, b, mutate)
    if c["fused_gdn"]:
        B, Ho, Wo, C = v.shape
        norm = conv_nhwc(v, np.ascontiguousarray(d["gamma"].T)[None], [(0, 0)], 1, Ho, Wo, square=True)
        norm = (norm + d["beta"]).astype(F32)
        return (v * unary(norm, "rsqrt")).astype(F32)
    if c["ps"] or c["kind"] == 2:
        v = _pixel_shuffle_nhwc(v, mutate)
    a0 = d.get("aux0")
    a1 = _se_scale(c, d, mutate) if c["epi"] == "SE_ADD" else d.get("aux1")
    return _epilogue32(c["epi"], v, a0, a1, mutate)


# ---------------------------------------------------------------------------------------------------------------- float64
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def _conv64(c, x, w):
    """the module's own operation in float64: NHWC x, module-layout w -> NHWC [B, outH, outW, C] after any PixelShuffle, no bias"""
    xt = _t(x).permute(0, 3, 1, 2)
    wt = _t(w)
    if c["kind"] == 0:
        y = F.conv2d(xt, wt, stride=c["stride"], padding=c["k"] // 2)
    else:
        y = F.conv_transpose2d(xt, wt, stride=2, padding=2, output_padding=1)
    if c["ps"]:
        y = F.pixel_shuffle(y, 2)
    return y.permute(0, 2, 3, 1).numpy()


def reference64(c, d, group=0):
    """(value, bound): the operation in float64 and the rigorous per-element bound on a float32 evaluation of it"""
    x, w, b = (d["x"], d["w"], d["b"])
    if group == 1:
        x = np.concatenate([d["x1"][..., :c["segs"][0][0]], d["x"][..., c["segs"][0][0]:]], axis=3)
        w, b = d["w1"], d["b1"]
    x64 = np.asarray(x, np.float64)
    if c["square"]:
        x64 = x64 * x64
    K = ktaps(c) * c["Cin"] + 1 + (1 if c["square"] else 0)
    pre = _conv64(c, x64, w)
    mag = _conv64(c, np.abs(x64), np.abs(np.asarray(w, np.float64)))
    if c["ps"]:
        # PixelShuffle of the bias: output channel c of sub-pixel (py, px) carries bias[c*4 + py*2 + px]
        B, oh, ow, oc = pre.shape
        bb = np.asarray(b, np.float64).reshape(oc, 2, 2)
        bmap = np.zeros((oh, ow, oc))
        for py in range(2):
            for px in range(2):
                bmap[py::2, px::2, :] = bb[:, py, px]
        pre = pre + bmap
        mag = mag + np.abs(bmap)
    else:
        pre = pre + np.asarray(b, np.float64)
        mag = mag + np.abs(np.asarray(b, np.float64))
    err = K * U * mag
    if c["fused_gdn"]:
        g, beta = np.asarray(d["gamma"], np.float64), np.asarray(d["beta"], np.float64)
        norm = beta + (pre * pre) @ g.T
        # the norm's chain (K2 = 192 + 1 terms, each x^2 rounded too) and the propagated error of x
        xa = np.abs(pre) + err
        err_norm = (g.shape[0] + 2) * U * (beta + (xa * xa) @ g.T) + (2 * xa * err) @ g.T
        val = pre / np.sqrt(norm)
        bound = err / np.sqrt(norm) + 0.5 * xa * err_norm / norm ** 1.5 + 8 * U * np.abs(val)
        return val, 2 * bound + 2.0 ** -140
    return _epilogue64(c, d, pre, err)


def _epilogue64(c, d, v, err):
    name = c["epi"]
    a0 = np.asarray(d["aux0"], np.float64) if "aux0" in d else None
    if name == "SE_ADD":
        B, oh, ow, oc = v.shape
        a1 = np.broadcast_to(np.asarray(d["aux1"], np.float64)[:, None, None, :], v.shape)
    else:
        a1 = np.asarray(d["aux1"], np.float64) if "aux1" in d else None
    av = np.abs(v)
    erf = torch.special.erf

    def gelu(t):
        return 0.5 * t * (1.0 + erf(torch.from_numpy(t / np.sqrt(2.0))).numpy())

    def sigmoid(t):
        return 1.0 / (1.0 + np.exp(-t))

    if name == "NONE":
        val, L, m = v, 1.0, av
    elif name == "GELU":
        val, L, m = gelu(v), 1.2, av
    elif name == "RES_GELU":
        val, L, m = gelu(v + a0), 1.2, av + np.abs(a0)
    elif name == "RES":
        val, L, m = a0 + v, 1.0, av + np.abs(a0)
    elif name == "GATE":
        val, L, m = a0 * sigmoid(v) + a1, 0.25 * np.abs(a0), np.abs(a0) + np.abs(a1)
    elif name == "GDN":
        val, L, m = a0 / np.sqrt(v), 0.5 * np.abs(a0) / np.maximum(v - err, 0.5) ** 1.5, np.abs(a0)
    elif name == "IGDN":
        val, L, m = a0 * np.sqrt(v), 0.5 * np.abs(a0) / np.sqrt(np.maximum(v - err, 0.5)), np.abs(a0) * np.sqrt(v + err)
    elif name == "CLAMP01":
        val, L, m = np.clip(v, 0.0, 1.0), 1.0, np.minimum(av, 1.0)
    elif name == "LRP":
        val, L, m = a0 + 0.5 * np.tanh(v), 0.5, np.abs(a0) + 0.5
    elif name == "LRP_ADD":
        val, L, m = (a0 + 0.5 * np.tanh(v)) + a1, 0.5, np.abs(a0) + np.abs(a1) + 0.5
    elif name == "LEAKY":
        val, L, m = np.where(v > 0, v, 0.01 * v), 1.0, av
    elif name == "LEAKY_RES":
        val, L, m = np.where(v > 0, v, 0.01 * v) + a0, 1.0, av + np.abs(a0)
    elif name == "RELU":
        val, L, m = np.maximum(v, 0.0), 1.0, av
    elif name == "SE_ADD":
        val, L, m = v + a0 * a1, 1.0, av + np.abs(a0 * a1)
    else:
        raise ValueError(name)
    bound = L * err + 8 * U * m
    return val, 2 * bound + 2.0 ** -140


def within(c, got, d, group=0):
    """(ok, worst ratio |got - ref| / bound, count of elements outside the bound)"""
    ref, bound = reference64(c, d, group)
    diff = np.abs(np.asarray(got, np.float64) - ref)
    bad = ~(diff <= bound)
    ratio = float(np.max(np.where(np.isfinite(diff), diff / bound, np.inf)))
    return not bad.any(), ratio, int(bad.sum())


FLT_MIN, FLT_MAX = 2.0 ** -126, float(np.finfo(np.float32).max)


def within_normal(c, got, d, group=0, exclude=None):
    """`within` for operands outside the ordinary (tests/hostile_values.py): the same reference and the same bound, asserted on the
    outputs whose float64 value is finite and of normal range and whose bound is finite and below FLT_MAX * 2^-24 (a chain whose
    |x| |w| sum passes FLT_MAX may overflow in float32 where float64 does not: the bound does not cover that), less the outputs of
    `exclude` (hostile_values.bound_exclusions).
    (ok, worst ratio, count outside the bound, count of outputs judged)"""
    with np.errstate(all="ignore"):
        ref, bound = reference64(c, d, group)
        judged = np.isfinite(ref) & (np.abs(ref) >= FLT_MIN) & (np.abs(ref) <= FLT_MAX) & np.isfinite(bound) & (bound < FLT_MAX * U)
        if exclude is not None:
            judged &= ~np.broadcast_to(exclude, judged.shape)
        diff = np.abs(np.asarray(got, np.float64) - ref)
        bad = judged & ~(diff <= bound)
        ratio = float(np.max(np.where(judged, np.where(np.isfinite(diff), diff / bound, np.inf), 0.0))) if judged.any() else 0.0
    return not bad.any(), ratio, int(bad.sum()), int(judged.sum())


# ---------------------------------------------------------------------------------------------------------------- the matrix
_COUTS = [36, 176, 224, 32, 96, 12, 36]


def matrix():
    """the launcher matrix of tests/test_gpu_conv_matrix.py: per case the (instantiation, epilogue form) it must reach"""
    cases = []
    for i, e in enumerate(EPI):
        # fast DIRECT (dense NHWC slice: ldo > Cout, offset channels; M tail 126 = 64 + 62, N tail); SE_ADD always takes the slow form
        co = _COUTS[i % len(_COUTS)]
        if i % 2 == 0:   # 3x3 over one 32-channel segment with ld 48: 9 chunks of 32 -> uni<32,3>
            cases.append(case(f"direct_{e}", 2, 7, 9, segs=[(32, 48, 8)], k=3, Cout=co, epi=e, ldo=co + 8, ooff=4,
                              expect=("UNI_32_3", "SLOW" if e == "SE_ADD" else "DIRECT")))
        else:            # 1x1 over 64 + 16 channels (a 16-channel tail segment): 3 chunks -> uni<32,2>
            cases.append(case(f"direct_{e}", 2, 7, 9, segs=[(64, 64, 0), (16, 20, 4)], k=1, Cout=co, epi=e, ldo=co + 4, ooff=4,
                              expect=("UNI_32_2", "SLOW" if e == "SE_ADD" else "DIRECT")))
        # the LDS row-table form with PERMUTED rows: stride 1, images <= 32 x 32, more than 256 64x64 blocks -> uni<16,3>
        cases.append(case(f"rowperm_{e}", 10, 30, 31, segs=[(16, 16, 0)], k=3, Cout=96, epi=e,
                          expect=("UNI_16_3", "SLOW" if e == "SE_ADD" else "TABLE")))
        # the slow form through an NCHW output (48 channels: a 32-chunk and a 16-channel tail)
        cases.append(case(f"nchw_{e}", 2, 6, 10, segs=[(48, 52, 0)], k=3, Cout=12, epi=e, out="nchw", expect=("UNI_32_3", "SLOW")))
    cases += [
        # h_s: 3x3 conv + GELU with PixelShuffle(2) into NHWC -- the row-table form on a strided output
        case("ps_nhwc_gelu", 2, 5, 6, segs=[(32, 32, 0)], k=3, Cout=64, epi="GELU", ps=True, expect=("UNI_32_3", "TABLE")),
        case("ps_nhwc_gelu_large", 4, 40, 40, segs=[(16, 16, 0)], k=3, Cout=192, epi="GELU", ps=True, expect=("UNI_16_3", "TABLE")),
        # the 192 -> 3 sub-pixel output layer into NCHW: Wo % 32 == 0 and M % 32 == 0 -> nchw_ps; otherwise the slow form
        case("subpixel_nchw_ps_none", 2, 4, 32, segs=[(32, 32, 0)], kind=2, Cout=3, epi="NONE", out="nchw",
             expect=("UNI_32_3", "NCHW_PS")),
        case("subpixel_nchw_ps_clamp", 1, 3, 64, segs=[(48, 48, 0)], kind=2, Cout=3, epi="CLAMP01", out="nchw",
             expect=("UNI_32_3", "NCHW_PS")),
        case("subpixel_nchw_ps_large", 1, 64, 288, segs=[(16, 16, 0)], kind=2, Cout=3, epi="CLAMP01", out="nchw",
             expect=("UNI_16_3", "NCHW_PS")),
        case("subpixel_slow_none", 2, 5, 20, segs=[(32, 32, 0)], kind=2, Cout=3, epi="NONE", out="nchw", expect=("UNI_32_3", "SLOW")),
        case("subpixel_slow_clamp", 1, 7, 33, segs=[(16, 32, 16)], kind=2, Cout=3, epi="CLAMP01", out="nchw",
             expect=("UNI_32_3", "SLOW")),
        # ConvTranspose2d(5, s2, p2, op1) as four output phases: strided output -> table form; with an aux epilogue -> slow form
        case("deconv_none", 2, 5, 7, segs=[(32, 32, 0)], kind=1, Cout=36, epi="NONE", expect=("UNI_32_3", "TABLE")),
        case("deconv_res", 1, 4, 6, segs=[(32, 32, 0), (16, 16, 0)], kind=1, Cout=32, epi="RES", expect=("UNI_32_3", "SLOW")),
        case("deconv_large", 2, 34, 34, segs=[(16, 16, 0)], kind=1, Cout=96, epi="GELU", expect=("UNI_16_3", "TABLE")),
        # large grids without permuted rows: stride 2 (direct), NCHW (slow)
        case("large_direct_s2", 2, 128, 130, segs=[(32, 32, 0)], k=3, stride=2, Cout=224, epi="GELU", ldo=232, ooff=8,
             expect=("UNI_16_3", "DIRECT")),
        case("large_nchw", 2, 100, 100, segs=[(16, 16, 0)], k=3, Cout=32, epi="CLAMP01", out="nchw", expect=("UNI_16_3", "SLOW")),
        case("large_5x5_s2_res", 2, 128, 128, segs=[(32, 32, 0)], k=5, stride=2, Cout=176, epi="RES", expect=("UNI_16_3", "DIRECT")),
        # GDN / IGDN: the contraction over x^2 (uni<32,2,square>), aux0 = the input itself
        case("gdn_square", 2, 9, 11, segs=[(64, 64, 0)], k=1, Cout=64, epi="GDN", square=True, expect=("UNI_32_2_SQ", "DIRECT")),
        case("igdn_square", 1, 8, 8, segs=[(192, 192, 0)], k=1, Cout=192, epi="IGDN", square=True, expect=("UNI_32_2_SQ", "DIRECT")),
        # weight layout 0 (conv_igemm_kernel)
        case("l0_64x64_se_add", 2, 6, 10, segs=[(32, 32, 0)], k=1, Cout=64, epi="SE_ADD", expect=("L0_64x64", "L0_GENERIC")),
        case("l0_64x64_leaky", 2, 6, 10, segs=[(32, 36, 0)], k=1, Cout=64, epi="LEAKY", expect=("L0_64x64", "L0_DIRECT")),
        case("l0_128x32_nchw", 2, 9, 13, segs=[(16, 16, 0)], k=3, Cout=3, epi="CLAMP01", out="nchw", expect=("L0_128x32", "L0_GENERIC")),
        case("l0_128x32_dense", 2, 9, 13, segs=[(16, 16, 0)], k=3, Cout=3, epi="NONE", expect=("L0_128x32", "L0_DIRECT")),
        case("l0_smallc_nchw_leaky", 2, 10, 14, Cin=3, smallc="nchw", k=3, Cout=32, epi="LEAKY",
             expect=("L0_64x64_SMALLC", "L0_DIRECT")),
        case("l0_smallc_nchw_se_add", 2, 10, 14, Cin=3, smallc="nchw", k=1, Cout=32, epi="SE_ADD",
             expect=("L0_64x64_SMALLC", "L0_GENERIC")),
        case("l0_smallc_nhwc_gelu", 2, 11, 9, Cin=3, smallc="nhwc", k=5, stride=2, Cout=96, epi="GELU",
             expect=("L0_64x64_SMALLC", "L0_DIRECT")),
        case("l0_smallc_128x32", 1, 12, 17, Cin=3, smallc="nchw", k=3, Cout=3, epi="NONE", expect=("L0_128x32_SMALLC", "L0_DIRECT")),
        # g_a.0 + g_a.1: 3 -> 192, 5x5 s2 from the NCHW image with the GDN fused (M = 99: a tail)
        case("in_gdn", 1, 18, 22, Cin=3, smallc="nchw", k=5, stride=2, Cout=192, fused_gdn=True, expect=("IN_GDN", "IN_GDN")),
        # input segments: 3, 4 and 8 segments, 16 / 48 / 80-channel tails, offset base pointers, ld > nch
        case("segs3", 2, 5, 6, segs=[(48, 52, 4), (80, 84, 0), (16, 16, 0)], k=3, Cout=96, epi="GELU", expect=("UNI_32_3", "DIRECT")),
        case("segs4_tail16", 1, 6, 7, segs=[(64, 68, 4), (32, 32, 0), (16, 24, 8), (16, 16, 0)], k=3, Cout=36, epi="LEAKY_RES",
             expect=("UNI_32_3", "DIRECT")),
        case("segs8_tail16", 1, 6, 7, segs=[(32, 36, 4), (16, 16, 0), (48, 48, 0), (16, 20, 4), (32, 32, 0), (80, 88, 8), (16, 16, 0),
                                             (16, 20, 4)], k=3, Cout=32, epi="RES_GELU", expect=("UNI_32_3", "DIRECT")),
        case("segs8_1x1", 2, 5, 5, segs=[(16, 16, 0)] * 7 + [(16, 20, 4)], k=1, Cout=224, epi="LRP_ADD", ldo=232, ooff=4,
             expect=("UNI_32_2", "DIRECT")),
        case("segs2_se_add_relu", 2, 8, 8, segs=[(64, 64, 0), (64, 64, 0)], k=1, Cout=32, epi="SE_ADD", relu=True,
             expect=("UNI_32_2", "SLOW")),
        # dual ReLU store (UNet): on a fast epilogue and on SE_ADD
        case("relu_store_res", 2, 8, 8, segs=[(128, 128, 0)], k=3, Cout=128, epi="RES", relu=True, expect=("UNI_32_3", "DIRECT")),
        case("relu_store_se_add", 2, 4, 4, segs=[(64, 64, 0)], k=1, Cout=128, epi="SE_ADD", relu=True, expect=("UNI_32_2", "SLOW")),
        case("relu_store_rowperm", 10, 30, 31, segs=[(16, 16, 0)], k=3, Cout=96, epi="RES", relu=True, expect=("UNI_16_3", "TABLE")),
        # grouped launch (cc_mean || cc_scale): both outputs
        case("group2_small", 2, 8, 8, segs=[(64, 68, 4), (32, 32, 0)], k=3, Cout=96, epi="GELU", ngroup=2, expect=("UNI_32_3", "DIRECT")),
        case("group2_large", 4, 32, 32, segs=[(32, 32, 0)], k=3, Cout=224, epi="NONE", ngroup=2, expect=("UNI_16_3", "TABLE")),
    ]
    return cases


# production (instantiation, epilogue form) pairs the matrix must reach
REQUIRED = {
    ("UNI_16_3", "DIRECT"), ("UNI_16_3", "TABLE"), ("UNI_16_3", "SLOW"), ("UNI_16_3", "NCHW_PS"),
    ("UNI_32_2", "DIRECT"), ("UNI_32_2", "SLOW"),
    ("UNI_32_3", "DIRECT"), ("UNI_32_3", "TABLE"), ("UNI_32_3", "SLOW"), ("UNI_32_3", "NCHW_PS"),
    ("UNI_32_2_SQ", "DIRECT"),
    ("L0_64x64", "L0_DIRECT"), ("L0_64x64", "L0_GENERIC"), ("L0_64x64_SMALLC", "L0_DIRECT"), ("L0_64x64_SMALLC", "L0_GENERIC"),
    ("L0_128x32", "L0_DIRECT"), ("L0_128x32", "L0_GENERIC"), ("L0_128x32_SMALLC", "L0_DIRECT"),
    ("IN_GDN", "IN_GDN"),
}

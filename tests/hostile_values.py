"""Values outside the ordinary through the conv, attention and stage kernels: the case table and its operand generators, for
tests/test_hostile_values_host.py (no GPU) and tests/test_gpu_hostile_values.py (GPU).  A pure host module: product code never imports
it.

The shapes are those of conv_contract.matrix() and stage_contract.matrix() -- one base case per REQUIRED pair of each matrix (plus one
small case per epilogue) -- and `expect` / the plan stay asserted; only the operands are replaced by a value class:

  conv      sub_in     x, x1, aux * 2^-128, biases * 2^-130 (GDN / IGDN / fused GDN keep beta): subnormal activations, normal weights
            sub_prod   x * 2^-70, w * 2^-62, b * 2^-135, aux * 2^-132: normal operands, subnormal products and sums
            sprinkle   one input element in 2000 (at least 4) replaced, cyclically, by NaN, +inf, -inf, 3e38, -3e38, 1e-40, -0.0
            sprinkle_nan  the same with NaN, 1e-40, -0.0, 3.0, -2.5 only: no inf - inf, so the NaN set EQUALS the geometric field
            overflow   terms of exactly +-2^126 whose signs follow one of three patterns over each aligned group of 8 k: a pattern that
                       passes 2^128 in the contract order 0,4,1,5,2,6,3,7 and not in ascending order, one the other way round, one in
                       neither -- the order decides between a number and an infinity (and, behind GELU, a NaN)
            cancel     +-2^60 u pairs (products exact) at k = 0, 1 of the even groups and k = 0, 4 of the odd ones in front of the
                       ordinary O(1) terms: where the pair is adjacent in the order the small terms survive, otherwise the first is lost
            (CLAMP01 and RELU cases of the subnormal classes take |x|, |w|, |b|: half of their outputs would be exact zeros otherwise)
  sweep     a 1 x 1 identity layer, zero bias, over the 2^24 floats of bit pattern 256 i + o (one odd o per epilogue): 16 channels x 2^20
            pixels (weight layout 0: K = 16 is below the 64 the unified kernel takes) and 64 channels x 2^18 pixels (the unified
            kernel, dense NHWC and NCHW output).  A pixel holds 16 (64) consecutive i: one exponent, so it is all finite -- the chain
            returns x bit for bit, subnormals included -- or all non-finite -- inf * 0 makes every channel NaN.  `branch_values()` is
            the list of pc_math.h's branch points with their +-4 ulp neighbours; non-finite pre-activations reach the epilogue through
            the bias (`bias_values()`: the chain of a zero input is +0).
  stages    attention (underflow / equal / nonfinite / sub_v), GDN (x * 2^64, x * 2^-128, sprinkle), SE (one inf, x * 2^-138), the NCHW
            copy (NaN payloads) and the quantisers at and beyond the int32 range (stage_contract.to_sym is the rule).

`MUTANTS` names deliberate mistakes of the restatements; the host test shows each one differs from the restatement on a named case.
"""
import zlib

import numpy as np

from oracle import liboracle as lo
from tests import conv_contract as cc
from tests import stage_contract as sc

F32 = np.float32
PERM8 = (0, 4, 1, 5, 2, 6, 3, 7)
SPECIALS = np.array([0x7FC00000, 0x7F800000, 0xFF800000, 0x7F61B1E6, 0xFF61B1E6, 0x000116C2, 0x80000000], np.uint32).view(F32)
#             NaN         +inf        -inf        3e38        -3e38       1e-40       -0.0
CAN_GIVE_INF = {"NONE", "GELU", "RES_GELU", "RES", "LEAKY", "LEAKY_RES", "RELU", "SE_ADD"}
DROPS_NAN = {"RELU"}                                   # v > 0 ? v : 0 -- the one epilogue a NaN pre-activation does not pass


def _u2f(u):
    return np.asarray(u, np.uint32).view(F32)


def same_bits_or_nan(got, want):
    """(mask of elements that differ, count of NaN pairs with different payloads): bits equal, except that where both are NaN only
    NaN-ness is compared -- the payload a NaN operation keeps is not part of the contract"""
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    both = np.isnan(g.view(F32)) & np.isnan(w.view(F32))
    ne = g != w
    return ne & ~both, int((ne & both).sum())


# ================================================================================================================ conv classes
CONV_CLASSES = ("sub_in", "sub_prod", "sprinkle", "sprinkle_nan", "overflow", "cancel")
NAN_ONLY = np.concatenate([np.array([0x7FC00000, 0x000116C2, 0x80000000], np.uint32).view(np.float32), np.array([3.0, -2.5], np.float32)])


def _work(c):
    Ho, Wo, _, _, _ = cc.out_grid(c)
    return c["B"] * Ho * Wo * cc.ktaps(c) * c["Cin"] * cc.gemm_cout(c) * (4 if c["kind"] == 1 else 1)


def conv_bases():
    """{(plan, form): the cheapest case of conv_contract.matrix() written for it}, every REQUIRED pair"""
    best = {}
    for c in cc.matrix():
        p = tuple(c["expect"])
        if p in cc.REQUIRED and (p not in best or _work(c) < _work(best[p])):
            best[p] = c
    assert set(best) == cc.REQUIRED
    return best


def _eligible(c, klass):
    plain = not (c["square"] or c["fused_gdn"] or c["epi"] in cc.POSITIVE_PRE)
    if klass == "sub_prod":
        return plain
    if klass in ("overflow", "cancel"):
        return plain and not c["smallc"] and c["Cin"] % 8 == 0
    return True


def conv_cases():
    """[dict(name, klass, c)]: every class on every base case it applies to; sprinkle also on one small case per epilogue"""
    bases = list(conv_bases().values())
    names = {c["name"] for c in bases}
    bases += [c for c in cc.matrix() if c["name"] == "group2_small"]     # the grouped launch: both groups, every class
    per_epi = [c for c in cc.matrix() if c["name"].startswith("direct_") and c["name"] not in names]
    out = []
    for klass in CONV_CLASSES:
        for c in bases + (per_epi if klass.startswith("sprinkle") else []):
            if _eligible(c, klass):
                out.append(dict(name=f"{klass}:{c['name']}", klass=klass, c=c))
    return out


def _groups(c):
    return ("",) if c["ngroup"] == 1 else ("", "1")


def conv_data(hc):
    """the operands of a hostile conv case (as conv_contract.make_data returns them)"""
    c, klass = hc["c"], hc["klass"]
    d = {k: np.array(v, F32, copy=True) for k, v in cc.make_data(c).items()}
    rng = np.random.default_rng(zlib.crc32(hc["name"].encode()))
    if klass in ("sub_in", "sub_prod"):
        if c["epi"] in ("CLAMP01", "RELU"):
            for k in ("x", "w", "b", "x1", "w1", "b1"):
                if k in d:
                    d[k] = np.abs(d[k])
        fx, fw, fb, fa = (2.0 ** -128, 1.0, 2.0 ** -130, 2.0 ** -128) if klass == "sub_in" else (2.0 ** -70, 2.0 ** -62, 2.0 ** -135, 2.0 ** -132)
        if klass == "sub_in" and c["epi"] in ("CLAMP01", "RELU"):
            fx, fb = fx * 2.0 ** -8, fb * 2.0 ** -8                  # a sum of K positive terms is O(sqrt K) larger than a signed one
        for g in _groups(c):
            d["x" + g] = (d["x" + g] * F32(fx)).astype(F32)
            d["w" + g] = (d["w" + g] * F32(fw)).astype(F32)
            if c["epi"] not in cc.POSITIVE_PRE:                        # there the bias is the GDN's beta: kept
                d["b" + g] = (d["b" + g] * F32(fb)).astype(F32)
        if "aux0" in d:
            d["aux0"] = (d["aux0"] * F32(fa)).astype(F32)
        if "aux1" in d and c["epi"] != "SE_ADD":                       # the SE scale stays in (0, 1): v + a0 * a1
            d["aux1"] = (d["aux1"] * F32(fa)).astype(F32)
    elif klass in ("sprinkle", "sprinkle_nan"):
        vals = SPECIALS if klass == "sprinkle" else NAN_ONLY
        for g in _groups(c):
            flat = d["x" + g].reshape(-1)
            n = max(4, flat.size // 2000)
            pos = rng.choice(flat.size, n, replace=False)
            flat[pos] = vals[np.arange(n) % len(vals)]
    elif klass == "overflow":
        pats = np.array([[1, -1, 1, -1, 1, -1, 1, -1],                  # passes 2^128 in neither order
                         [1, 1, 1, 1, -1, -1, -1, -1],                  # ascending: 4 * 2^126 = 2^128 -> inf; contract order: +-+-
                         [1, 1, -1, -1, 1, 1, -1, -1]], F32)            # contract order 0,4,1,5: ++++ -> inf; ascending: ++--
        B, H, W, Cin = d["x"].shape
        for g in _groups(c):
            which = rng.choice(3, (B, H, W), p=[0.84, 0.08, 0.08])
            sgn = rng.choice(np.array([-1, 1], F32), (B, H, W, 1))
            d["x" + g] = (np.tile(pats[which], Cin // 8) * sgn * F32(2.0 ** 63)).astype(F32)
            sn = rng.choice(np.array([-1, 1], F32), c["Cout"])
            shape = (-1, 1, 1, 1) if c["kind"] == 0 else (1, -1, 1, 1)
            d["w" + g] = np.broadcast_to(sn.reshape(shape) * F32(2.0 ** 63), d["w" + g].shape).astype(F32)
    elif klass == "cancel":
        B, H, W, Cin = d["x"].shape
        G = Cin // 8
        partner = np.where(np.arange(G) % 2 == 0, 1, 4)
        for g in _groups(c):
            big = (rng.choice(np.array([-1, 1], F32), (B, H, W, G)) * (1 + rng.integers(0, 2048, (B, H, W, G)) / 2048) * 2.0 ** 30).astype(F32)
            x = d["x" + g].reshape(B, H, W, G, 8)
            x[..., 0] = big
            for gi in range(G):
                x[..., gi, partner[gi]] = -big[..., gi]
            w = d["w" + g]
            if c["kind"] == 0:
                wv = w.reshape(w.shape[0], G, 8, *w.shape[2:])           # [Cout, G, 8, k, k]
                wb = (rng.choice(np.array([-1, 1], F32), wv[:, :, 0].shape) * (1 + rng.integers(0, 2048, wv[:, :, 0].shape) / 2048) * 2.0 ** 30).astype(F32)
                wv[:, :, 0] = wb
                for gi in range(G):
                    wv[:, gi, partner[gi]] = wb[:, gi]
            else:
                wv = w.reshape(G, 8, *w.shape[1:])                       # [G, 8, Cout, 5, 5]
                wb = (rng.choice(np.array([-1, 1], F32), wv[:, 0].shape) * (1 + rng.integers(0, 2048, wv[:, 0].shape) / 2048) * 2.0 ** 30).astype(F32)
                wv[:, 0] = wb
                for gi in range(G):
                    wv[gi, partner[gi]] = wb[gi]
    else:
        raise ValueError(klass)
    if c["square"]:
        d["aux0"] = d["x"]                                             # GDN: the identity operand is the layer's own input
    return d


def conv_case(name):
    """the case `klass:base` whether conv_cases() lists it or not"""
    klass, base = name.split(":")
    c = {x["name"]: x for x in cc.matrix()}[base]
    assert _eligible(c, klass), name
    return dict(name=name, klass=klass, c=c)


def conv_input(c, d, group=0):
    """the concatenated input a group's GEMM reads"""
    if group == 0:
        return d["x"]
    n0 = c["segs"][0][0]
    return np.concatenate([d["x1"][..., :n0], d["x"][..., n0:]], axis=3)


def field_of(c, mask_in):
    """per output PIXEL, whether its receptive field holds an input element of `mask_in` [B, H, W, Cin].  From the geometry alone:
    torch's float64 conv / conv_transpose of the indicator with all-ones weights (conv_contract._conv64), never the tap tables of the
    restatement"""
    ind = np.asarray(mask_in, np.float64)
    if c["kind"] == 2:
        # the sub-pixel form multiplies the whole 3 x 3 neighbourhood for each of the four phases, by an exact 0 where the 5 x 5 kernel
        # has no tap: NaN * 0 and inf * 0 are NaN, so the field of a non-finite input is wider than ConvTranspose2d's own
        g = dict(c, kind=0, k=3, stride=1, ps=False)
        f = cc._conv64(g, ind, np.ones((1, c["Cin"], 3, 3)))[..., 0]
        return np.repeat(np.repeat(f, 2, axis=1), 2, axis=2) > 0.5
    w1 = np.ones((c["Cout"], c["Cin"], c["k"], c["k"]) if c["kind"] == 0 else (c["Cin"], c["Cout"], 5, 5))
    return cc._conv64(c, ind, w1)[..., 0] > 0.5


def field_sets(c, d, group=0):
    """(holds a NaN, holds a non-finite or a |value| >= 1e38): the fields of the sprinkled inputs"""
    x = conv_input(c, d, group)
    with np.errstate(invalid="ignore"):
        return field_of(c, np.isnan(x)), field_of(c, ~np.isfinite(x) | (np.abs(x) >= 1e38))


def bound_exclusions(c, d, group=0):
    """outputs [B, outH, outW, 1] on which the float64 bound of the OPERATION says nothing about the float32 contract, or None:
    * the sub-pixel layer: the field of a non-finite input -- float64 is the real ConvTranspose2d, whose phases leave out the taps the
      packed form multiplies by 0 (a recorded difference);
    * GDN forms (x^2 operand, fused GDN): the field of an input of |x| >= 2^63 -- its square overflows in float32 and not in float64"""
    x = conv_input(c, d, group)
    with np.errstate(invalid="ignore"):
        if c["kind"] == 2:
            return field_of(c, ~np.isfinite(x))[..., None]
        if c["square"] or c["fused_gdn"]:
            return field_of(c, ~(np.abs(x) < 2.0 ** 63))[..., None]
    return None


# ---------------------------------------------------------------------------------------------------------------- conv mutants
def _flush(a):
    a = np.array(a, F32, copy=True)
    u = a.view(np.uint32)
    u[(u & 0x7F800000) == 0] &= np.uint32(0x80000000)
    return a


def ascending_k(c, d):
    """operands under which the oracle's in-group order 0,4,1,5,2,6,3,7 visits the ORIGINAL channels in ascending order: position
    PERM8[j] of every aligned group of 8 receives channel j (x's channel axis and w's Cin axis alike; needs Cin % 8 == 0, segments)"""
    assert c["Cin"] % 8 == 0 and not c["smallc"]
    idx = np.arange(c["Cin"]).reshape(-1, 8)
    src = np.empty_like(idx)
    src[:, PERM8] = idx                                    # new[PERM8[j]] = old[j]
    src = src.reshape(-1)
    out = dict(d)
    for g in _groups(c):
        out["x" + g] = np.ascontiguousarray(d["x" + g][..., src])
        out["w" + g] = np.ascontiguousarray(d["w" + g][:, src] if c["kind"] == 0 else d["w" + g][src])
    return out


def _epilogue_mutant(name, v, mutate):
    with np.errstate(invalid="ignore"):
        if mutate == "clamp_fminmax" and name == "CLAMP01":
            return np.fmin(np.fmax(v, F32(0)), F32(1)).astype(F32)            # fmin / fmax return the other operand for a NaN
        if mutate == "relu_nan" and name == "RELU":
            return np.where(np.isnan(v), v, np.where(v > 0, v, F32(0))).astype(F32)
    return None


def conv_restate(c, d, mutate=None, group=0):
    """conv_contract.restate, or one of this module's mutants of it"""
    with np.errstate(all="ignore"):
        if mutate is None:
            return cc.restate(c, d, group=group)
        if mutate == "flush_in":
            return cc.restate(c, {k: _flush(v) for k, v in d.items()}, group=group)
        if mutate == "flush_out":
            return _flush(cc.restate(c, d, group=group))
        if mutate == "ascending_k":
            return cc.restate(c, ascending_k(c, d), group=group)
        if mutate in ("clamp_fminmax", "relu_nan"):
            assert not (c["ps"] or c["kind"] == 2 or c["fused_gdn"])
            x = conv_input(c, d, group)
            v = cc._chains(c, x, d["w1"] if group else d["w"], d["b1"] if group else d["b"])
            return _epilogue_mutant(c["epi"], v, mutate)
    raise ValueError(mutate)


# ================================================================================================================ the epilogue sweep
# form: (channels, output layout) -- 16 channels: the layout-0 kernel (direct without aux0, generic with); 64: the unified kernel
SMALL_FORMS = {"l0": (16, "nhwc"), "uni_fast": (64, "nhwc"), "uni_slow": (64, "nchw")}


def sweep_offset(epi):
    """the odd low byte of the epilogue's 2^24 arguments"""
    return 2 * (17 * cc.EPI[epi] + 5) % 256 + 1


def sweep_values(epi):
    """the 2^24 arguments, float32 of bit pattern 256 i + o"""
    return _u2f(np.arange(2 ** 24, dtype=np.uint32) * np.uint32(256) + np.uint32(sweep_offset(epi)))


def _ulp_walk(v, k):
    u = np.array([v], F32).view(np.uint32)[0]
    return _u2f(np.array([u + k if k >= 0 else u - (-k)], np.uint32))[0]


def branch_values():
    """pc_math.h's branch points (|x| = 0.625, 1, 4, 9.5, 87, 88.7, 2^23, and the 0 / 1 of CLAMP01, LEAKY, RELU) with their +-4 ulp
    neighbours in both signs, FLT_MAX, the largest subnormal, the smallest normal, zeros of both signs; all finite.  Padded with 1.0 to
    a multiple of 64."""
    pts = [0.625, 1.0, 4.0, 9.5, 87.0, 88.7, 8388608.0, 0.5, 2.5, 0.70710678]
    vals = []
    for p in pts:
        for k in range(-4, 5):
            v = _ulp_walk(F32(p), k)
            vals += [v, -v]
    vals += [_u2f(0x7F7FFFFF), -_u2f(0x7F7FFFFF), _u2f(0x007FFFFF), -_u2f(0x007FFFFF), _u2f(0x00800000), -_u2f(0x00800000),
             _u2f(0x00000001), -_u2f(0x00000001), F32(0.0), F32(-0.0)]
    vals = np.array(vals, F32)
    pad = (-len(vals)) % 64
    return np.concatenate([vals, np.ones(pad, F32)])


def bias_values(n):
    """n pre-activations delivered through the bias: +-inf, NaN of both signs and a payload, +-FLT_MAX, -87, 88.7, ..."""
    base = np.concatenate([_u2f(np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7FA00123, 0x7F7FFFFF, 0xFF7FFFFF], np.uint32)),
                           np.array([-87.0, 88.7, -88.7, 89.0, -104.0, 9.5, -9.5, 4.0, -4.0], F32)])
    return np.resize(base, n).astype(F32)


def sweep_aux(epi, shape):
    """(aux0, aux1) that expose the epilogue's function: a0 = 0 where it is added, 1 where it multiplies"""
    a0 = a1 = None
    if epi in ("RES_GELU", "RES", "LRP", "LRP_ADD", "LEAKY_RES", "SE_ADD"):
        a0 = np.zeros(shape, F32)
    if epi in ("GATE", "GDN", "IGDN"):
        a0 = np.ones(shape, F32)
    if epi in ("GATE", "LRP_ADD"):
        a1 = np.zeros(shape, F32)
    if epi == "SE_ADD":
        a1 = np.ones((shape[0], shape[3]), F32)
    return a0, a1


def sweep_expect(epi, form, large):
    if form == "l0":
        return ("L0_64x64", "L0_GENERIC" if epi in cc.USES_AUX0 else "L0_DIRECT")
    plan = "UNI_16_3" if large else "UNI_32_2"
    return (plan, "SLOW" if (form == "uni_slow" or epi == "SE_ADD") else "DIRECT")


def sweep_case(epi, form, values, bias=None):
    """(case, data): the identity layer of `form` over `values` (a multiple of the channel count; every pixel all finite or all
    non-finite), or -- bias given -- over zeros with that bias"""
    Cc, out = SMALL_FORMS[form]
    P = values.size // Cc
    H = 1024 if P >= 2 ** 20 else (512 if P >= 2 ** 18 else 1)
    W = P // H
    c = cc.case(f"sweep_{epi}_{form}_{P}", 1, H, W, segs=[(Cc, Cc, 0)], k=1, Cout=Cc, epi=epi, out=out,
                expect=sweep_expect(epi, form, P >= 2 ** 18))
    d = dict(x=values.reshape(1, H, W, Cc), w=np.eye(Cc, dtype=F32).reshape(Cc, Cc, 1, 1), b=np.zeros(Cc, F32) if bias is None else bias)
    a0, a1 = sweep_aux(epi, (1, H, W, Cc))
    if a0 is not None:
        d["aux0"] = a0
    if a1 is not None:
        d["aux1"] = a1
    return c, d


def sweep_restate(c, d):
    """the identity layer's output by the shortcut the host test proves against conv_contract.restate: v = x on an all-finite pixel,
    NaN on every channel of a pixel that holds a non-finite value (inf * 0), then the bias add and the epilogue"""
    x = d["x"]
    with np.errstate(all="ignore"):
        fin = np.isfinite(x).all(axis=3, keepdims=True)
        v = np.where(fin, x + F32(0.0), F32(np.nan)).astype(F32)             # the chain starts at +0: -0 comes out as +0
        v = (v + d["b"]).astype(F32)
        a1 = cc._se_scale(c, d) if c["epi"] == "SE_ADD" else d.get("aux1")
        return cc._epilogue32(c["epi"], v, d.get("aux0"), a1)


# ================================================================================================================ stage classes
_STAGE = {c["name"]: c for c in sc.matrix()}
Q_VALUES = np.array([2.0 ** 23 - 0.5, 2.0 ** 23, 2.0 ** 23 + 1, 2.0 ** 24, 2147483520.0, 2.0 ** 31, 2.0 ** 31 + 256, 2.0 ** 40, 3e38, np.inf,
                     0.5, 1.5, 2.5, 1e-40, 0.0], np.float64)


def quant_values():
    """z - m (y - mu) of the quantiser cases: both signs of Q_VALUES, then NaNs of both signs"""
    v = np.concatenate([Q_VALUES, -Q_VALUES]).astype(F32)
    return np.concatenate([v, _u2f(np.array([0x7FC00000, 0xFFC00000, 0x7F800001], np.uint32))])


SYM_VALUES = np.array([-2 ** 31, 2 ** 31 - 1, 2 ** 24 + 1, -(2 ** 24 + 1), 2 ** 31 - 64, -(2 ** 31 - 65), 0, 1, -1], np.int64).astype(np.int32)
MU_VALUES = np.concatenate([_u2f(np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0x00000001, 0x80000000], np.uint32)), np.array([2.0 ** 31, -0.5, 3e38], F32)])
SCALE_VALUES = np.concatenate([_u2f(np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x00000001, 0x80000000, 0x7F7FFFFF], np.uint32)),
                               np.array([2.0 ** 31, -2.0 ** 31, 0.11], F32)])


def _derive(base, suffix, **kw):
    c = dict(_STAGE[base])
    c.update(kw)
    c["name"] = f"{base.split('@')[0]}@{suffix}" if c["kind"].startswith("PREP") or c["kind"] == "SE" else f"{base}@{suffix}"
    c["base"] = base
    return c


def stage_cases():
    """[dict(name, klass, c)] -- c a stage_contract case (its `expect` is the plan the base case was written for)"""
    out = []

    def add(c, klass):
        out.append(dict(name=f"{klass}:{c['name']}", klass=klass, c=c))

    for ws, D in ((8, 24), (4, 80), (4, 40)):
        for base in (f"att_{ws}_{D}_s0_ji0", f"att_{ws}_{D}_s{ws // 2}_ji1"):
            for klass in ("underflow", "equal", "nonfinite", "sub_v"):
                add(dict(_STAGE[base], base=base), klass)
    for base in ("gdn_c16_p65_f", "gdn_c192_p63_i", "gdn_c320_p64_f", "gdn_c16_p257_i"):
        for klass in ("x_2p64", "x_2m128", "sprinkle"):
            add(dict(_STAGE[base], base=base), klass)
    for base in ("se_c16_hw1@b3", "se_c32_hw4097@b3", "se_c128_hw4097@b3"):
        for klass in ("one_inf", "sub_x"):
            add(dict(_STAGE[base], base=base), klass)
    for base in ("nchw_c32_hw63", "nchw_c3_hw4096"):
        add(dict(_STAGE[base], base=base), "payloads")
    # the quantisers: mask mode 0, no ybase / yadd / likelihood, so that y - mu IS the planted value; HW 64 -> vec, 63 -> scalar
    plain = dict(mode=0, ybase=False, yadd=False, lik=False, edges=False, ties=False, mask=True, idx8=False)
    add(_derive("enc_hw64", "hostile", expect="PREP_VEC", **plain), "quant")
    add(_derive("enc_hw63", "hostile", expect="PREP_SCALAR", **plain), "quant")
    add(_derive("idx_hw64", "hostile", expect="PREP_VEC", mode=0, edges=False), "scale")
    add(_derive("idx_hw63", "hostile", expect="PREP_SCALAR", mode=1, edges=False), "scale")
    add(_derive("deq_hw64", "hostile"), "dequant")
    add(_derive("deq_hw63", "hostile"), "dequant")
    for base in ("eb_quant_c192_hw4", "eb_quant_c320_hw16"):
        add(dict(_STAGE[base], base=base), "quant")
    for base in ("eb_dequant_c192_hw4", "eb_dequant_c320_hw16"):
        add(dict(_STAGE[base], base=base), "dequant")
    return out


def _plant(flat, values, rng, avoid=()):
    """values written at distinct random positions of the flat view; returns the positions"""
    free = np.setdiff1d(np.arange(flat.size), np.asarray(avoid, np.int64))
    pos = rng.choice(free, len(values), replace=False)
    flat[pos] = values
    return pos


def stage_data(hc):
    c, klass = hc["c"], hc["klass"]
    d = sc.make_data(c)
    d = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    rng = np.random.default_rng(zlib.crc32(hc["name"].encode()))
    fam = sc.family(c)
    if fam == "attention":
        Cc = c["C"]
        if klass == "underflow":
            # most exp(s - max) lie below -87 and are exactly 0; one token per window carries v * 2^120, so that a key whose weight
            # should be that exact 0 would show in the output if the branch were missing (e^-87 * 2^120 is about 0.02)
            d["qkv"][..., :2 * Cc] *= F32(12.0)
            d["qkv"][:, ::c["ws"], ::c["ws"], 2 * Cc:] *= F32(2.0 ** 120)
        elif klass == "equal":
            d["qkv"][..., :Cc] = 0.0
            d["bias"][:] = 0.0
        elif klass == "nonfinite":
            ws = c["ws"]
            d["qkv"][0, 1, 1, 3] = np.inf                               # a q element of a token of the first window (unshifted frame)
            d["qkv"][0, ws + 1, 2 * ws + 1, 2 * Cc + 5] = np.nan        # a v element of a token in another window, shifted or not
        elif klass == "sub_v":
            d["qkv"][..., 2 * Cc:] *= F32(2.0 ** -128)
    elif fam == "gdn":
        if klass == "x_2p64":
            d["x"] = (d["x"] * F32(2.0 ** 64)).astype(F32)
        elif klass == "x_2m128":
            d["x"] = (d["x"] * F32(2.0 ** -128)).astype(F32)
        else:
            flat = d["x"].reshape(-1)
            n = max(4, flat.size // 2000)
            flat[rng.choice(flat.size, n, replace=False)] = SPECIALS[np.arange(n) % len(SPECIALS)]
    elif fam == "se":
        if klass == "one_inf":
            d["x"][c["B"] - 1, c["HW"] // 2, 3] = np.inf
        else:
            d["x"] = (d["x"] * F32(2.0 ** -138)).astype(F32)             # a chunk sums 4096 / G of them: still below 2^-126
    elif fam == "nchw_slice":
        flat = d["src"].reshape(-1)
        n = min(flat.size // 2, 96)
        pay = (np.arange(n, dtype=np.uint32) * np.uint32(0x9E3) + np.uint32(1)) & np.uint32(0x007FFFFF)
        sign = (np.arange(n, dtype=np.uint32) & np.uint32(1)) << np.uint32(31)
        vals = np.concatenate([_u2f(np.uint32(0x7F800000) | sign | pay), SPECIALS])        # signalling and quiet NaNs, distinct payloads
        _plant(flat, vals, rng)
    elif fam == "prep":
        if klass == "quant":
            v = quant_values()
            pos = _plant(d["y"].reshape(-1), v, rng)
            d["mu"].reshape(-1)[pos] = 0.0
            # and the same conversion reached through a subtraction: y - mu = 2^31 exactly, = -2^24 exactly
            pos2 = _plant(d["y"].reshape(-1), np.array([2.0 ** 31 + 256, -2.0 ** 24 + 1], F32), rng, avoid=pos)
            d["mu"].reshape(-1)[pos2] = np.array([256.0, 1.0], F32)
        elif klass == "scale":
            _plant(d["scale"].reshape(-1), SCALE_VALUES, rng)
        elif klass == "dequant":
            pos = _plant(d["sym_in"].reshape(-1), SYM_VALUES, rng)
            B, HW, Cc = c["B"], c["HW"], d["mu"].shape[2]
            b, ch, p = np.unravel_index(pos[:2], (B, Cc, HW))
            under = (b * HW + p) * Cc + ch                               # the means under the planted INT32 extremes: +1 and -1
            d["mu"].reshape(-1)[under] = np.array([1.0, -1.0], F32)
            _plant(d["mu"].reshape(-1), MU_VALUES, rng, avoid=under)
    elif fam == "eb":
        Cc, HW, B = c["C"], c["HW"], c["B"]
        if klass == "quant":
            v = quant_values()
            ch = rng.choice(Cc, 6, replace=False)
            d["med"][ch] = 0.0
            sub = d["z"][:, :, ch]                                        # [B, HW, 6]: planted where z - med is z
            flat = sub.reshape(-1)
            flat[rng.choice(flat.size, len(v), replace=False)] = v
            d["z"][:, :, ch] = flat.reshape(sub.shape)
        else:
            _plant(d["sym"].reshape(-1), SYM_VALUES, rng)
            d["med"][rng.choice(Cc, len(MU_VALUES), replace=False)] = MU_VALUES
    else:
        raise ValueError(fam)
    return d


def stage_restate(c, d, mutate=None):
    with np.errstate(all="ignore"):
        if mutate == "softmax_no_zero":
            o = lo.win_attention(d["qkv"], d["bias"], c["heads"], c["ws"], c["shift"], d["fscale"], variant=1)
            return dict(out=o.reshape(-1, c["C"]))
        if mutate == "copy_canonical_nan":
            out = sc.restate(c, d)
            o = out["out"].copy()
            o.view(np.uint32)[np.isnan(o)] = 0x7FC00000
            return dict(out=o)
        return sc.restate(c, d, mutate)


COPIES = {"NCHW_SLICE", "MAXPOOL"}               # copies and selections: all 32 bits compared, NaN payloads included

# mutant: (the restatement it is applied to, the case it must differ on).  LEAKY has no NaN mutant: `v > 0 ? v : 0.01 v` passes a NaN on
# whichever way the comparison is written, so there is nothing to get wrong; RELU is the epilogue where the choice shows.
MUTANTS = {
    "flush_in": ("conv", "sub_in:direct_NONE"),
    "flush_out": ("conv", "sub_in:direct_NONE"),
    "ascending_k@overflow": ("conv", "overflow:direct_NONE"),
    "ascending_k@cancel": ("conv", "cancel:direct_NONE"),
    "clamp_fminmax": ("conv", "sprinkle:direct_CLAMP01"),
    "relu_nan": ("conv", "sprinkle:direct_RELU"),
    "softmax_no_zero": ("stage", "underflow:att_8_24_s0_ji0"),
    "wrapping@prep": ("stage", "quant:enc_hw64@hostile"),
    "wrapping@eb": ("stage", "quant:eb_quant_c192_hw4"),
    "copy_canonical_nan": ("stage", "payloads:nchw_c32_hw63"),
}

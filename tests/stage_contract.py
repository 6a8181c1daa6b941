"""The non-conv device stages (progressivecodec_amd/csrc/pc_stages.hip, and GDN through the conv launcher) restated on the CPU, for
tests/test_gpu_stage_matrix.py (GPU) and tests/test_stage_contract_host.py (no GPU).  Per kernel family:

  restate(c, d)       the outputs in the contract's float32 and order (numpy float32, the oracle's chains, pc_math.h through the oracle).
                      Where the stage is specified bit-exact the GPU must return these bits.
  reference64(...)    the operation itself in float64, written from its definition (not from the kernel), and an elementwise bound on a
                      float32 evaluation of it.
  matrix()            the cases, each with the kernel variant (`expect`, a PC_SPLAN_* name) it is written to reach.

How the bounds are derived (never fitted): U = 2^-24 is the unit roundoff of one float32 operation, so fl(a op b) = (a op b)(1 + e),
|e| <= U, and an operation whose exact result is representable in float32 has e = 0 (`_rnd` tests exactly that: this is what lets an
exactly representable rounding tie be compared as a decision instead of being excluded).  A chain of n additions of terms t_i is within
n U sum|t_i| of the exact sum; a function with Lipschitz constant L passes an input error e on as L e; include/pc_math.h is pinned by
tests/test_pc_math.py to 1 ulp (exp, tanh, erf) and 2 ulp (sigmoid), i.e. 2 U and 4 U relative.  First-order products of these terms are
covered by the factor 2 every bound carries at the end (as conv_contract.reference64 does), flushed subnormals by an absolute 2^-140
(1e-40 where exp(-100) of the attention mask is involved).

  prep      v = (y - ybase) - mu: e1 = U|y - ybase| (0 if representable), e2 = U(|v| + e1) (0 if e1 = 0 and v representable); the product
            with the mask m in {0, 1} is exact.  sym is compared as a DECISION: an element is excluded iff its float64 v lies within
            e1 + e2 > 0 of k + 1/2.  idx and mask have no exclusions: s, s * m and thr are exact float32 inputs.  y_hat = (sym + mu) + yadd:
            one rounding per addition.  The likelihood follows the reference's eval path: values = |y_hat32 - mu| (mode 0, y_hat32 the
            float32 sum sym + mu: an exact input of the likelihood) or |sym|; t = (+-1/2 - a) / s has two roundings, the constant 2^-1/2 one
            and the product one: |d arg| <= 4 U |arg| + da / (s sqrt 2), da the rounding of the subtraction; erfc is evaluated in double and
            rounded once (U, plus 2^-50 for the double routine); d/darg (erfc / 2) = exp(-arg^2) / sqrt(pi).  The difference upper - lower is
            bounded ABSOLUTELY: U (upper + lower) + the two propagated terms + U |lik|, so the cancellation is paid for in full.
  attention score chain: q * scale (U), D fmaf steps, bias add, mask add: e_s = (D + 3) U (sum|q s k| + |bias| + 100 [masked]).  softmax:
            exp is 2 U relative and e^x turns an absolute argument error d into a relative one: numerator eta_j = 2 e_s + U|s_j - m| + 2 U,
            denominator max eta + T U, division U.  Output chain of T fmaf: T U sum p|v| + sum p_j rho_j |v_j|.
  GDN       norm = beta + gamma . x^2: (C + 2) U (beta + gamma . x^2); x * norm^(-+1/2) with the derivative of the root at norm - err and
            8 U of the result for rsqrt / sqrt / product (the conv contract's GDN epilogue bound).
  quantile  the interpolated order statistic is continuous and piecewise linear in the rank; rank = q (n - 1) in float32 is within
            2 U rank, so the value moves by at most that times the largest gap next to the two ranks, plus 4 U max|value| for the lerp.
  eb        quantise / dequantise as prep (median for mu).  Likelihood: the density network forward with a running error: a layer
            a = sum w l + b has e_a = sum|w| e_l + 4 U (sum|w l| + |b|); t = a + f tanh(a): e_t = e_a + |f|(e_a + 2 U) + 2 U (|a| + |f|);
            sigmoid: 4 U sigma + sigma'(max(|x| - e, 0)) e; the difference absolutely, U each for the sum and the product with the sign.
  rem       ret * att is exact (att in {-1, 0, 1}), one rounding of the sum; the two masks compare exact inputs.
  SE        the mean is a tree of depth CHUNK / G + G + nchunk + 1 over |x| / HW; fc chains (n + 1) U sum|m w| + sum|w| e; ReLU passes the
            error on; sigmoid as above.
  nchw, maxpool   copies and selections: the float64 value is the float32 value, bound 0 (NaN positions must agree).

NaN scales (and +inf under mask mode 3, where s * 0 is NaN) are not combined with `lik`: the reference's LowerBound passes a NaN scale on,
gc_likelihood takes `bound` for it; a NaN scale never reaches the likelihood in the codec (the hyper-synthesis output is finite) and the
case is left out of the matrix on purpose.  The other edge scales (table entries, below the bound, 0, +inf) reach both likelihood kernels.

Memory: every case is a few MB at most except `pool_grid_stride`: more than 8192 * 256 output quads need a 2898 x 2896 x 4 float input
(134 MB on the device); it is the one large case of the matrix.
"""
import ctypes as C
import os
import re
import zlib

import numpy as np

from oracle import liboracle as lo
from tests import unet_contract as uc

F32 = np.float32
U = 2.0 ** -24
TINY = 2.0 ** -140
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SE_CHUNK = 4096
QUANTILE_SMALL_N = 32768
QW_STRIDE = 8 + 32768            # PC_QW_STRIDE of pc_stages.hip: header + candidate list, uint32 per image
EB_NET = 58
PC_ERR_ARG = -1

KIND = dict(PREP_ENC=1, PREP_DEC_INDEX=2, PREP_DEQUANT=3, ATTENTION=4, GDN=5, QUANTILE=6, EB_QUANT=7, EB_DEQUANT=8, EB_LIK=9, REM=10,
            NCHW_SLICE=11, SE=12, MAXPOOL=13)
SPLAN = dict(SINGLE=1, PREP_SCALAR=2, PREP_VEC=3, PREP_VEC_LIK=4, ATT_8_24=5, ATT_4_80=6, ATT_4_40=7, Q_REG8=8, Q_REG32=9, Q_MULTI_VEC=10,
             Q_MULTI_SCALAR=11, GDN_SQ=16 + 4)
# every production variant: (kind, plan)
REQUIRED = {("PREP_ENC", "PREP_SCALAR"), ("PREP_ENC", "PREP_VEC"), ("PREP_ENC", "PREP_VEC_LIK"), ("PREP_DEC_INDEX", "PREP_SCALAR"),
            ("PREP_DEC_INDEX", "PREP_VEC"), ("PREP_DEQUANT", "PREP_SCALAR"), ("PREP_DEQUANT", "PREP_VEC"), ("ATTENTION", "ATT_8_24"),
            ("ATTENTION", "ATT_4_80"), ("ATTENTION", "ATT_4_40"), ("GDN", "GDN_SQ"), ("QUANTILE", "Q_REG8"), ("QUANTILE", "Q_REG32"),
            ("QUANTILE", "Q_MULTI_VEC"), ("QUANTILE", "Q_MULTI_SCALAR"), ("EB_QUANT", "SINGLE"), ("EB_DEQUANT", "SINGLE"),
            ("EB_LIK", "SINGLE"), ("REM", "SINGLE"), ("NCHW_SLICE", "SINGLE"), ("SE", "SINGLE"), ("MAXPOOL", "SINGLE")}

_P, _I, _F, _L = C.c_void_p, C.c_int, C.c_float, C.c_int64


class Desc(C.Structure):
    """mirror of pc_test_stage_desc (include/pcodec.h); test_stage_contract_host.py compares it with the header text"""
    _fields_ = [("size", _I), ("kind", _I), ("B", _I), ("HW", _I), ("C", _I), ("H", _I), ("W", _I),
                ("scale", _P), ("ld_scale", _I), ("mu", _P), ("ld_mu", _I), ("y", _P), ("ld_y", _I), ("ybase", _P), ("ld_ybase", _I),
                ("yadd", _P), ("ld_yadd", _I), ("thr", _P), ("mask_mode", _I), ("mask_src", _P), ("mask_sb", _L),
                ("table", _P), ("ntable", _I), ("bound", _F), ("sym", _P), ("idx", _P), ("idx8", _P), ("mask", _P),
                ("yhat", _P), ("ld_yhat", _I), ("lik", _P), ("lik_sb", _L), ("x", _P), ("ld_x", _I), ("aux0", _P), ("aux1", _P),
                ("out", _P), ("out2", _P), ("heads", _I), ("ws", _I), ("shift", _I), ("bias_ji", _I), ("fscale", _F), ("inverse", _I),
                ("q", _F), ("work", _P), ("sb", _L), ("thr_bar", _P), ("mode_star", _I), ("mode_bar", _I)]


def header_fields():
    """[(ctype, name)] of pc_test_stage_desc as include/pcodec.h declares it"""
    txt = open(os.path.join(ROOT, "include", "pcodec.h")).read()
    body = re.search(r"typedef struct pc_test_stage_desc \{(.*?)\} pc_test_stage_desc;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.fullmatch(r"(.*?)(\w+)", decl, re.S)
        ty, name = m.group(1).strip(), m.group(2)
        ct = _P if ty.endswith("*") else {"int": _I, "float": _F, "int64_t": _L}[ty]
        out.append((ct, name))
    return out


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _rnd(x64):
    """rounding error bound of one float32 operation with exact result x64: U|x|, 0 where x is representable"""
    x64 = np.asarray(x64, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        rep = x64.astype(F32).astype(np.float64) == x64
    return np.where(rep, 0.0, U * np.abs(x64))


def to_sym(v, mutate=None):
    """(int32_t)pc_roundevenf(v) as the contract fixes it outside the finite |v| < 2^31 ("values outside the
    ordinary"): round half to even in float32 (the identity from 2^23 on), clip to [-2^31, 2^31 - 1], then cast; NaN gives 0.  The
    mutation "wrapping" is the other conversion in use: the low 32 bits of the integer (INT32_MIN for what no int64 holds)."""
    v = np.asarray(v, F32)
    with np.errstate(invalid="ignore"):
        r = np.rint(v).astype(np.float64)
    if mutate == "wrapping":
        big = ~(np.abs(r) < 2.0 ** 63)                      # NaN included
        i = np.where(big, 0.0, r).astype(np.int64)
        return np.where(big, np.int64(-2 ** 31), ((i + 2 ** 31) % 2 ** 32) - 2 ** 31).astype(np.int32)
    r = np.where(np.isnan(r), 0.0, r)
    return np.clip(r, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64).astype(np.int32)


def _few_planted(n):
    """the N_PLANTED inexact ties count against the exclusion cap: planted only where the cap has room for them"""
    return n < 10 ** 4 or int(1e-4 * n) > 2 * N_PLANTED


def spec(field, arr=None, shape=None, dtype=None, ld=None, coff=0, lead=0, out=False):
    """one device buffer: rows of `shape[1]` elements at columns coff.. of rows ld wide, `lead` elements before the first row (a
    misaligned base); inputs carry `arr`, outputs (`out`) their shape and, when updated in place, their initial `arr`"""
    if arr is not None:
        arr = np.ascontiguousarray(arr)
        arr = arr.reshape(arr.shape[0], -1)
        shape, dtype = arr.shape, arr.dtype
    return dict(field=field, arr=arr, shape=tuple(shape), dtype=np.dtype(dtype), ld=ld or shape[1], coff=coff, lead=lead, out=out)


GAP32, SENT32, GUARD = 0x7FE1A5A5, 0x7FE2B6B6, 1024      # quiet NaNs of a distinctive payload: input gaps / around and between outputs


def layout(sp):
    """(buffer, ptr_offset, index): the spec's buffer as uint8 / uint32 words filled with the sentinel (GUARD elements on both sides), the
    element offset of the pointer handed to the launcher, and the flat positions [rows, n] of its elements"""
    rows, n = sp["shape"]
    ld, lead = sp["ld"], sp["lead"]
    wide = sp["dtype"].itemsize == 4
    r = np.arange(rows, dtype=np.int64)
    if "batch" in sp:                                  # rows are pixels, images `pad` elements further apart than HW * ld
        B, HW, pad = sp["batch"]
        start = (r // HW) * (HW * ld + pad) + (r % HW) * ld
        total = B * (HW * ld + pad)
    else:
        start, total = r * ld, rows * ld
    assert sp["coff"] + n <= ld
    fill = (SENT32 if sp["out"] else GAP32) if wide else (0xB6 if sp["out"] else 0xA5)
    buf = np.full(2 * GUARD + lead + total, fill, np.uint32 if wide else np.uint8)
    ptr = GUARD + lead + sp["coff"]
    index = ptr + start[:, None] + np.arange(n, dtype=np.int64)[None]
    return buf, ptr, index


def as_words(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint8 else a.view(np.uint32)


def case(name, kind, expect, **kw):
    c = dict(name=name, kind=kind, expect=expect)
    c.update(kw)
    return c


# ================================================================================================================ prep
PREP_DEFAULT = dict(B=2, HW=64, mode=0, ybase=False, yadd=False, lik=False, mask=True, idx8=False, mask_src=False, ld=32, coff=0,
                    ld_one=None, lead=None, lik_pad=0, idx8_lead=0, ntable=64, edges=True, mu_scale=1.0, ties=True)
N_PLANTED = 4


def _table(nt):
    from tests.util import tables_npz
    t = np.asarray(tables_npz()["scale_table"], F32)
    if nt == 64:
        return t
    return np.ascontiguousarray(t[np.linspace(0, 63, nt).round().astype(int)])


def prep_data(c):
    r = _rng(c["name"].split("@")[0])
    B, HW = c["B"], c["HW"]
    table = _table(c["ntable"])
    d = dict(table=table, bound=F32(0.11))
    scale = (0.6 + 0.7 * r.standard_normal((B, HW, 32))).astype(F32)
    mu = (r.standard_normal((B, HW, 32)) * c["mu_scale"]).astype(F32)
    ybase = (2 * r.standard_normal((B, HW, 32))).astype(F32)
    yadd = r.standard_normal((B, HW, 32)).astype(F32)
    dy = (2 * r.standard_normal((B, HW, 32))).astype(F32)
    if c["mu_scale"] > 1:                       # the likelihood's (sym + mu) - mu case: symbols of +-1, +-2 on large means
        dy = r.integers(-2, 3, (B, HW, 32)).astype(F32) + (0.3 * r.standard_normal((B, HW, 32))).astype(F32)
        scale = (0.3 + 0.2 * r.random((B, HW, 32))).astype(F32)
    y = (mu + dy + (ybase if c["ybase"] else 0)).astype(F32) if c["mu_scale"] > 1 else dy
    sf, mf, yf, bf = scale.reshape(-1), mu.reshape(-1), y.reshape(-1), ybase.reshape(-1)
    if c["edges"]:
        nt = len(table)
        sf[0:4] = table[[1 % nt, nt // 3, nt // 2, nt - 1]]                   # exactly on table entries
        sf[4:6] = [0.05, -1.0]                                                # below `bound`
        sf[9] = 0.0
        if not c["lik"]:
            sf[6:8] = np.array([0x7fc00000, 0xffc00001], np.uint32).view(F32) # NaN of both signs
        if not (c["lik"] and c["mode"] == 3):                                 # inf * 0 is a NaN scale: kept away from the likelihood too
            sf[8] = np.inf
    if c["ties"]:
        k = np.array([0, 1, 2, -3], F32)
        base = bf[12:16] if c["ybase"] else 0
        if _few_planted(B * HW * 32):
            yf[12:16] = ((mf[12:16] + k + F32(0.5)).astype(F32) + base).astype(F32)  # float32 ties, not exact in float64: excluded
        mf[16:20] = np.array([0.25, -0.75, 1.5, 0.0], F32)                            # exact ties: every operation representable
        bf[16:20] = np.array([0.5, -1.0, 0.0, 2.0], F32)
        yf[16:20] = mf[16:20] + np.array([0.5, 1.5, -2.5, -0.5], F32) + (bf[16:20] if c["ybase"] else 0)
    msrc = (0.6 + 0.7 * r.standard_normal((B, 32, HW))).astype(F32)
    src = msrc if c["mask_src"] else scale
    fin = np.where(np.isfinite(src), src, 0.6)
    thr = np.array([np.quantile(fin[b].astype(np.float64), 0.7) for b in range(B)]).astype(F32)
    if B > 1 and not c["mask_src"]:
        thr[1] = scale[1].reshape(-1)[min(40, HW * 32 - 1)]                    # a threshold that IS an element: the >= compare
    sym_in = r.integers(-40, 41, (B, 32, HW)).astype(np.int32)
    d.update(scale=scale, mu=mu, y=y, ybase=ybase, yadd=yadd, thr=thr, mask_src=msrc, sym_in=sym_in)
    return d


def _tr(a):
    """[B][HW][32] -> [B][32][HW]"""
    return np.ascontiguousarray(np.asarray(a).transpose(0, 2, 1))


def _index_np(s, table, bound, le=False):
    s = np.asarray(s, F32)
    nan = np.isnan(s)
    sb = np.where(s > bound, s, bound).astype(F32)
    t = table[: len(table) - 1]
    cnt = (t[None] <= sb.reshape(-1, 1)).sum(1) if le else (t[None] < sb.reshape(-1, 1)).sum(1)
    return np.where(nan.reshape(-1), len(table) - 1, cnt).astype(np.int32).reshape(s.shape)


def gc_likelihood32(values, s_eff):
    """gc_likelihood of pc_stages.hip: float32 arguments, erfc in double on the float32 argument, rounded once"""
    from scipy.special import erfc
    a = np.abs(values).astype(F32)
    cst = F32(-0.70710678118654752440)
    u = ((F32(0.5) - a) / s_eff).astype(F32)
    l = ((F32(-0.5) - a) / s_eff).astype(F32)
    up = F32(0.5) * erfc((cst * u).astype(F32).astype(np.float64)).astype(F32)
    low = F32(0.5) * erfc((cst * l).astype(F32).astype(np.float64)).astype(F32)
    lik = (up - low).astype(F32)
    return np.where(lik > F32(1e-9), lik, F32(1e-9)).astype(F32)


def prep_restate(c, d, mutate=None):
    B, HW, mode = c["B"], c["HW"], c["mode"]
    s, mu, table, bound = d["scale"], d["mu"], d["table"], d["bound"]
    out = {}
    if c["kind"] == "PREP_DEQUANT":
        sym = np.ascontiguousarray(d["sym_in"].transpose(0, 2, 1))
        out["yhat"] = (sym.astype(F32) + mu).astype(F32).reshape(B * HW, 32)
        return out
    mv = d["mask_src"].transpose(0, 2, 1) if c["mask_src"] else s
    thr = d["thr"].reshape(B, 1, 1)
    if mode == 1:
        m = ((mv > thr) if mutate == "mask_gt" else (mv >= thr)).astype(F32)
    elif mode == 3:
        m = np.zeros_like(s)
    else:
        m = np.ones_like(s)
    with np.errstate(invalid="ignore"):
        sm = s if mode == 0 else (s * m).astype(F32)
    src = s if mutate == "index_from_s" else sm
    idx = _index_np(src, table, bound, le=True) if mutate == "table_le" else lo.build_indexes(src, table, bound)
    out["idx"] = _tr(idx).reshape(B, -1)
    if c["idx8"]:
        out["idx8"] = out["idx"].astype(np.uint8)
    if c["mask"]:
        out["mask"] = _tr(m).reshape(B, -1)
    if c["kind"] == "PREP_DEC_INDEX":
        return out
    y = d["y"]
    if c["ybase"]:
        y = (y + d["ybase"]).astype(F32) if mutate == "ybase_added" else (y - d["ybase"]).astype(F32)
    v = (y - mu).astype(F32)
    if mode != 0:
        v = (v * m).astype(F32)
    if mutate == "round_away":
        sym = (np.sign(v) * np.floor(np.abs(v) + F32(0.5))).astype(np.int32)
    else:
        sym = to_sym(v, mutate)
    out["sym"] = _tr(sym).reshape(B, -1)
    yh = (sym.astype(F32) + mu).astype(F32)
    if c["yadd"] and mutate != "yadd_dropped":
        yh = (yh + d["yadd"]).astype(F32)
    out["yhat"] = yh.reshape(B * HW, 32)
    if c["lik"]:
        sf = sym.astype(F32)
        values = ((sf + mu).astype(F32) - mu).astype(F32) if (mode == 0 and mutate != "lik_from_sym") else sf
        out["lik"] = _tr(gc_likelihood32(values, np.where(sm > bound, sm, bound).astype(F32))).reshape(B, -1)
    return out


def _decision(v64, ebound):
    """(rint(v64), excluded): excluded iff v64 lies within a non-zero error bound of k + 1/2"""
    dist = np.abs(v64 - (np.floor(v64) + 0.5))
    return np.rint(v64), (ebound > 0) & (dist <= ebound)


def prep_check64(c, d, outs):
    """[(output, ok, worst ratio or mismatch count, excluded)]"""
    from scipy.special import erfc
    B, HW, mode = c["B"], c["HW"], c["mode"]
    mu64 = d["mu"].astype(np.float64)
    res = []
    if c["kind"] == "PREP_DEQUANT":
        ref = d["sym_in"].transpose(0, 2, 1).astype(np.float64) + mu64
        return [_bounded("yhat", outs["yhat"], ref.reshape(B * HW, 32), 2 * _rnd(ref).reshape(B * HW, 32) + TINY)]
    s64 = d["scale"].astype(np.float64)
    mv = (d["mask_src"].transpose(0, 2, 1) if c["mask_src"] else d["scale"]).astype(np.float64)
    thr = d["thr"].astype(np.float64).reshape(B, 1, 1)
    m = (mv >= thr).astype(np.float64) if mode == 1 else (np.zeros_like(s64) if mode == 3 else np.ones_like(s64))
    with np.errstate(invalid="ignore"):
        sm = s64 if mode == 0 else s64 * m
    # build_indexes (entropy_models.py:661-666): scales = max(sm, bound) with NaN propagated; idx = nt - 1 - #{k < nt - 1: scales <= table[k]}
    t64 = d["table"].astype(np.float64)
    sc = np.where(np.isnan(sm), np.nan, np.maximum(sm, float(d["bound"])))
    idx = np.full(sm.shape, len(t64) - 1, np.int64)
    with np.errstate(invalid="ignore"):
        for k in range(len(t64) - 1):
            idx -= (sc <= t64[k])
    res.append(_equal("idx", outs["idx"], _tr(idx).reshape(B, -1)))
    if c["idx8"]:
        res.append(_equal("idx8", outs["idx8"], _tr(idx).reshape(B, -1)))
    if c["mask"]:
        res.append(_equal("mask", outs["mask"], _tr(m).reshape(B, -1)))
    if c["kind"] == "PREP_DEC_INDEX":
        return res
    dd = d["y"].astype(np.float64) - (d["ybase"].astype(np.float64) if c["ybase"] else 0.0)
    e1 = _rnd(dd) if c["ybase"] else np.zeros_like(dd)
    v = dd - mu64
    e2 = np.where((e1 == 0) & (_rnd(v) == 0), 0.0, U * (np.abs(v) + e1))
    r, excl = _decision(v * m if mode != 0 else v, (e1 + e2) * (m if mode != 0 else 1.0))
    sym_got = outs["sym"].reshape(B, 32, HW).transpose(0, 2, 1)
    bad = (sym_got != r) & ~excl & _dec_mask(v * m if mode != 0 else v)
    res.append(("sym", not bad.any(), int(bad.sum()), int(excl.sum())))
    symf = sym_got.astype(np.float64)
    yh = symf + mu64
    eb = _rnd(yh)
    if c["yadd"]:
        yh2 = yh + d["yadd"].astype(np.float64)
        eb = eb + U * (np.abs(yh2) + eb)
        yh = yh2
    res.append(_bounded("yhat", outs["yhat"], yh.reshape(B * HW, 32), 2 * eb.reshape(B * HW, 32) + TINY))
    if c["lik"]:
        yhat32 = (sym_got.astype(F32) + d["mu"]).astype(F32).astype(np.float64)
        a = np.abs(yhat32 - mu64) if mode == 0 else np.abs(symf)
        da = _rnd(yhat32 - mu64) if mode == 0 else 0.0
        se = np.maximum(sm, float(d["bound"]))
        au, al = -(0.5 - a) / (se * np.sqrt(2.0)), -(-0.5 - a) / (se * np.sqrt(2.0))
        up, low = 0.5 * erfc(au), 0.5 * erfc(al)
        lik = np.maximum(up - low, 1e-9)
        dau, dal = 4 * U * np.abs(au) + da / (se * np.sqrt(2.0)), 4 * U * np.abs(al) + da / (se * np.sqrt(2.0))
        bnd = (U + 2.0 ** -50) * (up + low) + (np.exp(-au * au) * dau + np.exp(-al * al) * dal) / np.sqrt(np.pi) + U * lik + U * 1e-9
        res.append(_bounded("lik", outs["lik"], _tr(lik).reshape(B, -1), 2 * _tr(bnd).reshape(B, -1) + TINY))
    return res


_NORMAL_ONLY = [None]          # None: every element is judged (check64); a dict {output: mask to leave out}: check64_normal is running
FLT_MIN, FLT_MAX = 2.0 ** -126, float(np.finfo(np.float32).max)


def _dec_mask(v64):
    """decision outputs under check64_normal: judged where the float64 operand is finite and inside the int32 range"""
    if _NORMAL_ONLY[0] is None:
        return True
    with np.errstate(invalid="ignore"):
        return np.isfinite(v64) & (np.abs(v64) < 2.0 ** 31)


def _bounded(name, got, ref, bound):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        diff = np.abs(np.asarray(got, np.float64) - ref)
        if _NORMAL_ONLY[0] is not None:
            ref, bound = np.broadcast_to(ref, diff.shape), np.broadcast_to(bound, diff.shape)
            judged = np.isfinite(ref) & ((np.abs(ref) >= FLT_MIN) | (ref == 0)) & (np.abs(ref) <= FLT_MAX) & np.isfinite(bound)
            out = _NORMAL_ONLY[0].get(name)
            if out is not None:
                judged &= ~np.broadcast_to(out, diff.shape)
            bad = judged & ~(diff <= bound)
            ratio = float(np.max(np.where(judged, np.where(np.isfinite(diff), diff / bound, np.inf), 0.0))) if judged.any() else 0.0
            _NORMAL_ONLY.append((name, int(judged.sum()), int(judged.size)))
            return (name, not bad.any(), ratio, 0)
        bad = ~(diff <= bound)
        ratio = float(np.max(np.where(np.isfinite(diff), diff / bound, np.inf))) if diff.size else 0.0
    return (name, not bad.any(), ratio, 0)


def _equal(name, got, ref):
    """decision / selection outputs: equal values, NaN in the same places"""
    g, r = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bad = ~((g == r) | (np.isnan(g) & np.isnan(r)))
    return (name, not bad.any(), int(bad.sum()), 0)


def prep_specs(c, d):
    B, HW, ld, co = c["B"], c["HW"], c["ld"], c["coff"]
    lead = lambda f: 1 if c["lead"] == f else 0
    ldf = lambda f: 33 if c["ld_one"] == f else ld                    # ld_one: this tensor alone has rows of 33 floats
    rows = lambda f, a: spec(f, a.reshape(B * HW, 32), ld=ldf(f), coff=co, lead=lead(f))
    plane = lambda f, dt, **kw: spec(f, shape=(B, 32 * HW), dtype=dt, out=True, lead=lead(f), **kw)
    sp = [spec("table", d["table"].reshape(1, -1))]
    if c["kind"] == "PREP_DEQUANT":
        return sp[:0] + [spec("sym", d["sym_in"].reshape(B, -1), lead=lead("sym")), rows("mu", d["mu"]),
                         spec("yhat", shape=(B * HW, 32), dtype=F32, ld=ldf("yhat"), coff=co, lead=lead("yhat"), out=True)]
    sp += [rows("scale", d["scale"]), plane("idx", np.int32)]
    if c["mode"] == 1:
        sp.append(spec("thr", d["thr"].reshape(1, -1)))
    if c["mask_src"]:
        sp.append(spec("mask_src", d["mask_src"].reshape(B, -1), ld=32 * HW + 5))
    if c["idx8"]:
        sp.append(plane("idx8", np.uint8)); sp[-1]["lead"] = c["idx8_lead"]
    if c["mask"]:
        sp.append(plane("mask", F32))
    if c["kind"] == "PREP_DEC_INDEX":
        return sp
    sp += [rows("mu", d["mu"]), rows("y", d["y"]), plane("sym", np.int32),
           spec("yhat", shape=(B * HW, 32), dtype=F32, ld=ldf("yhat"), coff=co, lead=lead("yhat"), out=True)]
    if c["ybase"]:
        sp.append(rows("ybase", d["ybase"]))
    if c["yadd"]:
        sp.append(rows("yadd", d["yadd"]))
    if c["lik"]:
        sp.append(plane("lik", F32, ld=32 * HW + c["lik_pad"]))
    return sp


def prep_scalars(c, d):
    ld = c["ld"]
    ldf = lambda n: 33 if c["ld_one"] == n else ld
    f = dict(B=c["B"], HW=c["HW"], C=32, ld_scale=ldf("scale"), ld_mu=ldf("mu"), ld_y=ldf("y"), ld_ybase=ldf("ybase"), ld_yadd=ldf("yadd"),
             ld_yhat=ldf("yhat"), mask_mode=c["mode"],
             ntable=len(d["table"]), bound=float(d["bound"]), mask_sb=32 * c["HW"] + 5, lik_sb=32 * c["HW"] + c["lik_pad"])
    return f


def prep_cases():
    cs = []

    def add(name, kind, expect, **kw):
        p = dict(PREP_DEFAULT)
        p.update(kw)
        cs.append(case(name, kind, expect, **p))

    # every HW, the modes cycling, aligned (vec) and with the optional operands cycling
    for i, hw in enumerate([1, 3, 4, 60, 63, 64, 65, 100, 4132]):
        vec = hw % 4 == 0
        mode = i % 4
        opt = dict(ybase=bool(i & 1), yadd=bool(i & 2), lik=(i % 3 == 0), idx8=bool(i & 1), mask=(i % 4 != 3))
        e = "PREP_SCALAR" if not vec else ("PREP_VEC_LIK" if opt["lik"] else "PREP_VEC")
        add(f"enc_hw{hw}", "PREP_ENC", e, HW=hw, mode=mode, B=5 if hw == 60 else 2, **opt)
        add(f"idx_hw{hw}", "PREP_DEC_INDEX", "PREP_VEC" if vec else "PREP_SCALAR", HW=hw, mode=(i + 1) % 4, idx8=bool(i & 2), mask=bool(i & 1),
            B=1 if hw == 4 else 2)
        add(f"deq_hw{hw}", "PREP_DEQUANT", "PREP_VEC" if vec else "PREP_SCALAR", HW=hw, B=5 if hw == 64 else 1)
    # every mask mode with and without each optional operand (aligned: vec)
    for mode in range(4):
        add(f"enc_mode{mode}_all", "PREP_ENC", "PREP_VEC_LIK", mode=mode, ybase=True, yadd=True, lik=True, idx8=True, B=5)
        add(f"enc_mode{mode}_none", "PREP_ENC", "PREP_VEC", mode=mode, mask=False)
        add(f"enc_mode{mode}_edges", "PREP_ENC", "PREP_VEC", mode=mode, ybase=True, idx8=True, HW=4)
    add("enc_mask_src", "PREP_ENC", "PREP_SCALAR", mode=1, mask_src=True, ybase=True, lik=True)
    add("idx_mask_src", "PREP_DEC_INDEX", "PREP_SCALAR", mode=1, mask_src=True, idx8=True)
    # the vec preconditions broken one at a time: an aligned twin (`@` suffix shares the data) and the scalar plan
    full = dict(mode=1, ybase=True, yadd=True, lik=True, idx8=True, HW=64)
    add("twin@aligned", "PREP_ENC", "PREP_VEC_LIK", **full)
    add("twin@ld33", "PREP_ENC", "PREP_SCALAR", ld=33, **full)
    for f in ("scale", "mu", "y", "ybase", "yadd", "yhat", "sym", "idx", "mask", "lik"):
        add(f"twin@lead_{f}", "PREP_ENC", "PREP_SCALAR", lead=f, **full)
    for f in ("scale", "mu", "y", "ybase", "yadd", "yhat"):
        add(f"twin@ld_{f}", "PREP_ENC", "PREP_SCALAR", ld_one=f, **full)
    add("twin@lik_sb", "PREP_ENC", "PREP_SCALAR", lik_pad=3, **full)
    add("twin@idx8", "PREP_ENC", "PREP_SCALAR", idx8_lead=1, **full)
    add("twin@lik_sb_aligned", "PREP_ENC", "PREP_VEC_LIK", lik_pad=8, **full)
    add("idxtwin@aligned", "PREP_DEC_INDEX", "PREP_VEC", mode=1, idx8=True)
    add("idxtwin@ld33", "PREP_DEC_INDEX", "PREP_SCALAR", mode=1, idx8=True, ld=33)
    add("idxtwin@idx8", "PREP_DEC_INDEX", "PREP_SCALAR", mode=1, idx8=True, idx8_lead=1)
    for f in ("scale", "idx", "mask"):
        add(f"idxtwin@lead_{f}", "PREP_DEC_INDEX", "PREP_SCALAR", mode=1, idx8=True, lead=f)
    add("idxtwin@ld_scale", "PREP_DEC_INDEX", "PREP_SCALAR", mode=1, idx8=True, ld_one="scale")
    add("deqtwin@aligned", "PREP_DEQUANT", "PREP_VEC")
    add("deqtwin@ld33", "PREP_DEQUANT", "PREP_SCALAR", ld=33)
    add("deqtwin@lead_mu", "PREP_DEQUANT", "PREP_SCALAR", lead="mu")
    add("deqtwin@lead_sym", "PREP_DEQUANT", "PREP_SCALAR", lead="sym")
    add("deqtwin@lead_yhat", "PREP_DEQUANT", "PREP_SCALAR", lead="yhat")
    add("deqtwin@ld_mu", "PREP_DEQUANT", "PREP_SCALAR", ld_one="mu")
    add("deqtwin@ld_yhat", "PREP_DEQUANT", "PREP_SCALAR", ld_one="yhat")
    # slices at channel offset 32 k inside rows of 640 and 320 floats
    for ld, k in ((640, 0), (640, 7), (640, 19), (320, 3), (320, 9)):
        add(f"enc_slice_{ld}_{k}", "PREP_ENC", "PREP_VEC", ld=ld, coff=32 * k, mode=1, ybase=True, HW=100)
        add(f"deq_slice_{ld}_{k}", "PREP_DEQUANT", "PREP_VEC", ld=ld, coff=32 * k, HW=60)
    for nt in (2, 17):
        add(f"enc_ntable{nt}", "PREP_ENC", "PREP_VEC", ntable=nt, mode=1)
        add(f"enc_ntable{nt}_scalar", "PREP_ENC", "PREP_SCALAR", ntable=nt, mode=3, HW=63)
        add(f"idx_ntable{nt}", "PREP_DEC_INDEX", "PREP_VEC", ntable=nt, mode=0)
    # symbols on large means: (sym + mu) - mu is not the symbol (the likelihood's `values` of base slices)
    add("enc_lik_large_mu", "PREP_ENC", "PREP_VEC_LIK", lik=True, mu_scale=1000.0, edges=False, ties=False, HW=256)
    add("enc_lik_large_mu_scalar", "PREP_ENC", "PREP_SCALAR", lik=True, mu_scale=1000.0, edges=False, ties=False, HW=63, ybase=True)
    add("enc_cap_4m", "PREP_ENC", "PREP_VEC", HW=4132, B=5, ybase=True, mode=1)
    return cs


# ================================================================================================================ attention
def att_data(c):
    r = _rng(c["name"])
    B, H, W, Cc, heads, ws = c["B"], c["H"], c["W"], c["C"], c["heads"], c["ws"]
    T = ws * ws
    qkv = r.standard_normal((B, H, W, 3 * Cc)).astype(F32)
    bias = (r.standard_normal((heads, T, T)) * 0.8).astype(F32)          # [h][i][j], far from symmetric
    return dict(qkv=qkv, bias=bias, fscale=F32((Cc // heads) ** -0.5))


def att_restate(c, d, mutate=None):
    if mutate is not None:
        return dict(out=attention_np(c, d, F32, mutate).astype(F32).reshape(-1, c["C"]))
    o = lo.win_attention(d["qkv"], d["bias"], c["heads"], c["ws"], c["shift"], d["fscale"])
    return dict(out=o.reshape(-1, c["C"]))


def attention_np(c, d, dtype=np.float64, mutate=None, want_bound=False):
    """Shifted-window attention from its definition: roll by -shift, partition into windows, softmax(q k^T scale + bias + mask) v per head,
    merge, roll back (Swin; the mask of -100 between the three row / column regions (0, -ws), (-ws, -shift), (-shift, end))."""
    import torch
    B, H, W, Cc, heads, ws, shift = c["B"], c["H"], c["W"], c["C"], c["heads"], c["ws"], c["shift"]
    D, T = Cc // heads, ws * ws
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    x = torch.from_numpy(d["qkv"]).to(tdt)
    sgn = 1 if mutate == "roll_direction" else -1
    if shift:
        x = torch.roll(x, shifts=(sgn * shift, sgn * shift), dims=(1, 2))
    nwy, nwx = H // ws, W // ws
    xw = x.reshape(B, nwy, ws, nwx, ws, 3 * Cc).permute(0, 1, 3, 2, 4, 5).reshape(B * nwy * nwx, T, 3 * Cc)
    if mutate == "channel_major":
        qkv = xw.reshape(-1, T, 3, D, heads).permute(2, 0, 4, 1, 3)
    else:
        qkv = xw.reshape(-1, T, 3, heads, D).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]                                       # [nW B, heads, T, D]
    scale = float(d["fscale"])
    bias = torch.from_numpy(d["bias"]).to(tdt)
    if mutate == "bias_transposed":
        bias = bias.transpose(1, 2)
    attn = (q * scale) @ k.transpose(-2, -1) + bias.unsqueeze(0)
    mask = None
    if shift:
        img = torch.zeros(H, W)
        cut = ws // 2 if mutate == "region_boundary" else shift
        n = 0
        for hs in (slice(0, -ws), slice(-ws, -cut), slice(-cut, None)):
            for wsl in (slice(0, -ws), slice(-ws, -cut), slice(-cut, None)):
                img[hs, wsl] = n
                n += 1
        mw = img.reshape(nwy, ws, nwx, ws).permute(0, 2, 1, 3).reshape(nwy * nwx, T)
        mask = torch.where(mw[:, None, :] != mw[:, :, None], -100.0, 0.0).to(tdt)          # [nW, T, T]
        attn = (attn.reshape(B, nwy * nwx, heads, T, T) + mask[None, :, None]).reshape(-1, heads, T, T)
    p = torch.softmax(attn, dim=-1)
    o = p @ v                                                              # [nW B, heads, T, D]
    if mutate == "channel_major":
        o = o.permute(0, 2, 3, 1).reshape(-1, T, Cc)
    else:
        o = o.permute(0, 2, 1, 3).reshape(-1, T, Cc)
    o = o.reshape(B, nwy, nwx, ws, ws, Cc).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, Cc)
    if shift:
        o = torch.roll(o, shifts=(-sgn * shift, -sgn * shift), dims=(1, 2))
    if not want_bound:
        return o.numpy()
    # the bound, per (window, head, query) row
    mag = (q.abs() * abs(scale)) @ k.abs().transpose(-2, -1) + bias.abs().unsqueeze(0)
    if mask is not None:
        mag = (mag.reshape(B, nwy * nwx, heads, T, T) + mask.abs()[None, :, None]).reshape(-1, heads, T, T)
    e_s = ((D + 3) * U * mag).amax(dim=-1, keepdim=True)
    eta = 2 * e_s + U * (attn - attn.amax(dim=-1, keepdim=True)).abs() + 2 * U
    rho = eta + eta.amax(dim=-1, keepdim=True) + (T + 1) * U
    bnd = T * U * (p @ v.abs()) + (p * rho) @ v.abs()
    bnd = bnd.permute(0, 2, 1, 3).reshape(-1, T, Cc).reshape(B, nwy, nwx, ws, ws, Cc).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, Cc)
    if shift:
        bnd = torch.roll(bnd, shifts=(shift, shift), dims=(1, 2))
    return o.numpy(), 2 * bnd.numpy() + 1e-40


def att_check64(c, d, outs):
    ref, bnd = attention_np(c, d, np.float64, None, want_bound=True)
    return [_bounded("out", outs["out"], ref.reshape(-1, c["C"]), bnd.reshape(-1, c["C"]))]


def att_specs(c, d):
    bias = d["bias"].transpose(0, 2, 1) if c["bias_ji"] else d["bias"]
    return [spec("x", d["qkv"].reshape(-1, 3 * c["C"])), spec("aux0", np.ascontiguousarray(bias).reshape(1, -1)),
            spec("out", shape=(c["B"] * c["H"] * c["W"], c["C"]), dtype=F32, out=True)]


def att_scalars(c, d):
    return dict(B=c["B"], H=c["H"], W=c["W"], C=c["C"], heads=c["heads"], ws=c["ws"], shift=c["shift"], bias_ji=c["bias_ji"],
                fscale=float(d["fscale"]))


def att_cases():
    cs = []
    inst = (("ATT_8_24", 8, 24), ("ATT_4_80", 4, 80), ("ATT_4_40", 4, 40))
    for e, ws, D in inst:
        for shift in (0, 1, ws // 2, ws - 1):
            for ji in (0, 1):
                cs.append(case(f"att_{ws}_{D}_s{shift}_ji{ji}", "ATTENTION", e, B=1 + ji, H=2 * ws, W=3 * ws, C=8 * D, heads=8, ws=ws,
                               shift=shift, bias_ji=ji))
        # one window per side, one window in all; a pair count that leaves the last wave / block partly empty (3 heads, one window)
        cs.append(case(f"att_{ws}_{D}_h_eq_ws", "ATTENTION", e, B=1, H=ws, W=2 * ws, C=8 * D, heads=8, ws=ws, shift=ws // 2, bias_ji=1))
        cs.append(case(f"att_{ws}_{D}_w_eq_ws", "ATTENTION", e, B=1, H=3 * ws, W=ws, C=8 * D, heads=8, ws=ws, shift=1, bias_ji=0))
        cs.append(case(f"att_{ws}_{D}_one_window", "ATTENTION", e, B=1, H=ws, W=ws, C=8 * D, heads=8, ws=ws, shift=ws - 1, bias_ji=1))
        cs.append(case(f"att_{ws}_{D}_3pairs", "ATTENTION", e, B=1, H=ws, W=ws, C=3 * D, heads=3, ws=ws, shift=ws // 2, bias_ji=1))
        cs.append(case(f"att_{ws}_{D}_21pairs", "ATTENTION", e, B=1, H=ws, W=7 * ws, C=3 * D, heads=3, ws=ws, shift=1, bias_ji=0))
    return cs


# ================================================================================================================ GDN
def gdn_data(c):
    r = _rng(c["name"])
    Cc, P = c["C"], c["P"]
    x = r.standard_normal((1, 1, P, Cc)).astype(F32)
    beta = (1.0 + r.random(Cc)).astype(F32)                                 # norm >= 1 (as POSITIVE_PRE in the conv contract)
    gamma = (0.1 * np.eye(Cc) + 0.004 * np.abs(r.standard_normal((Cc, Cc)))).astype(F32)
    return dict(x=x, beta=beta, gamma=gamma)


def gdn_restate(c, d, mutate=None):
    Cc, P = c["C"], c["P"]
    norm = lo.conv_nhwc(d["x"], np.ascontiguousarray(d["gamma"].T).reshape(1, Cc, Cc), [(0, 0)], 1, 1, P, square=True) + d["beta"].reshape(1, 1, 1, -1)
    return dict(out=(d["x"] * lo.unary(norm.astype(F32), "sqrt" if c["inverse"] else "rsqrt")).astype(F32).reshape(P, Cc))


def gdn_check64(c, d, outs):
    x = d["x"].astype(np.float64).reshape(c["P"], c["C"])
    g, beta = d["gamma"].astype(np.float64), d["beta"].astype(np.float64)
    norm = beta + (x * x) @ g.T
    err = (c["C"] + 2) * U * norm
    lown = np.maximum(norm - err, 0.5)
    if c["inverse"]:
        val, L, m = x * np.sqrt(norm), 0.5 * np.abs(x) / np.sqrt(lown), np.abs(x) * np.sqrt(norm + err)
    else:
        val, L, m = x / np.sqrt(norm), 0.5 * np.abs(x) / lown ** 1.5, np.abs(x)
    return [_bounded("out", outs["out"], val, 2 * (L * err + 8 * U * m) + TINY)]


def gdn_cases():
    return [case(f"gdn_c{Cc}_p{P}_{'i' if inv else 'f'}", "GDN", "GDN_SQ", C=Cc, P=P, inverse=inv)
            for Cc in (16, 192, 320) for P in (1, 63, 64, 65, 257) for inv in (0, 1)]


# ================================================================================================================ quantile
def q_data(c):
    r = _rng(c["name"])
    s = (0.6 + 0.7 * r.standard_normal((c["B"], c["HW"], c["C"]))).astype(F32)
    if c.get("ties"):
        s[0] = np.round(s[0] * 4) / 4
    return dict(scale=s, q=F32(c["q"]))


def q_restate(c, d, mutate=None):
    return dict(out=np.array([lo.quantile(d["scale"][b], d["q"]) for b in range(c["B"])], F32).reshape(1, -1))


def q_check64(c, d, outs):
    n = c["HW"] * c["C"]
    ref, bnd = [], []
    for b in range(c["B"]):
        s = np.sort(d["scale"][b].reshape(-1).astype(np.float64))
        rank = float(d["q"]) * (n - 1)
        lo_, hi_ = int(np.floor(rank)), int(np.ceil(rank))
        ref.append(s[lo_] + (rank - lo_) * (s[hi_] - s[lo_]))
        a, z = max(lo_ - 1, 0), min(hi_ + 1, n - 1)
        gap = np.max(np.diff(s[a:z + 1])) if z > a else 0.0
        bnd.append(2 * (2 * U * rank * gap + 4 * U * max(abs(s[lo_]), abs(s[hi_]))) + TINY)
    return [_bounded("out", outs["out"], np.array(ref).reshape(1, -1), np.array(bnd).reshape(1, -1))]


def q_cases():
    mk = lambda name, e, HW, Cc, **kw: case(name, "QUANTILE", e, **{**dict(B=2, HW=HW, C=Cc, ld=Cc, sb_pad=0, q=0.95, lead=0, own_work=False), **kw})
    return [mk("q_8192", "Q_REG8", 256, 32), mk("q_8193", "Q_REG32", 2731, 3, q=0.5), mk("q_32768", "Q_REG32", 1024, 32, ties=True),
            mk("q_32769", "Q_MULTI_SCALAR", 10923, 3, q=0.3), mk("q_multi_vec", "Q_MULTI_VEC", 1025, 32),
            mk("q_multi_vec_sb", "Q_MULTI_VEC", 1100, 32, ld=40, sb_pad=64, B=3, q=0.7, own_work=True),
            mk("q_multi_ld33", "Q_MULTI_SCALAR", 1100, 32, ld=33, sb_pad=7, B=3, own_work=True),
            mk("q_multi_sb_only", "Q_MULTI_SCALAR", 1100, 32, sb_pad=2),          # `sb & 3` alone: ld, C and the base pointer stay aligned
            mk("q_multi_ld_only", "Q_MULTI_SCALAR", 1100, 32, ld=34, B=3),             # `ld & 3` alone: sb = 1100 * 34 is a multiple of 4
            mk("q_multi_lead", "Q_MULTI_SCALAR", 1100, 32, lead=1), mk("q_reg8_sb", "Q_REG8", 60, 32, ld=64, sb_pad=96, B=3, q=0.1),
            mk("q_reg32_sb", "Q_REG32", 700, 32, ld=36, sb_pad=4, q=0.999)]


# ================================================================================================================ EntropyBottleneck
def eb_data(c):
    r = _rng(c["name"])
    B, HW, Cc = c["B"], c["HW"], c["C"]
    med = (0.5 * r.standard_normal(Cc)).astype(F32)
    med[::8] = (np.arange(len(med[::8])) % 9 - 4).astype(F32) * F32(0.25)       # dyadic medians: exact ties possible
    med[0] = 0.0
    z = (3 * r.standard_normal((B, HW, Cc))).astype(F32)
    z[:, 0, 8::8] = (med[8::8] + F32(2.5)).astype(F32)                           # exact ties (k + 1/2 away, every operation exact)
    z[:, HW - 1, 16::16] = (med[16::16] - F32(1.5)).astype(F32)
    if _few_planted(B * HW * Cc):
        z[0, 0, 1:4] = (med[1:4] + np.array([0.5, 1.5, -2.5], F32)).astype(F32)  # float32 ties that float64 may see off the tie: excluded
    sym = np.rint(3 * r.standard_normal((B, Cc, HW))).astype(np.int32)
    sym.reshape(-1)[1::97] = 60
    sym.reshape(-1)[2::101] = -1000
    sym[:, 0, 0] = 0
    # density network per channel: [sp0 3][b0 3][tf0 3] 3 x {[sp 9][b 3][tf 3]} [sp4 3][b4 1], sp = softplus(matrix) > 0, tf = tanh(factor)
    net = np.zeros((Cc, EB_NET), F32)
    sp = lambda n: np.log1p(np.exp(r.standard_normal((Cc, n)))).astype(F32)
    net[:, 0:3], net[:, 3:6], net[:, 6:9] = sp(3), 0.5 * r.standard_normal((Cc, 3)), np.tanh(0.5 * r.standard_normal((Cc, 3)))
    for l in range(3):
        o = 9 + 15 * l
        net[:, o:o + 9], net[:, o + 9:o + 12], net[:, o + 12:o + 15] = 0.6 * sp(9), 0.5 * r.standard_normal((Cc, 3)), np.tanh(0.5 * r.standard_normal((Cc, 3)))
    net[:, 54:57], net[:, 57] = sp(3), 0.3 * r.standard_normal(Cc)
    for cz in (0, 5):                        # odd networks (no biases) on a zero median: lower + upper is exactly 0 at the symbol 0
        net[cz, 3:6] = 0
        net[cz, 57] = 0
        for l in range(3):
            net[cz, 9 + 15 * l + 9:9 + 15 * l + 12] = 0
        med[cz] = 0.0
        sym[:, cz, :] = np.where(r.random((B, HW)) < 0.5, 0, sym[:, cz, :])
    sym[:, 0, 0] = 0
    return dict(z=z, med=med, sym=sym, net=net)


def _eb_logits32(net, x):
    """eb_logits of pc_stages.hip; net [..., 58] broadcast against x"""
    n = lambda i: net[..., i]
    l = []
    for j in range(3):
        a = (n(j) * x).astype(F32) + n(3 + j)
        l.append((a + (n(6 + j) * lo.unary(a, "tanh")).astype(F32)).astype(F32))
    for layer in range(3):
        o = 9 + 15 * layer
        t = []
        for j in range(3):
            a = (n(o + 3 * j) * l[0]).astype(F32)
            a = (a + (n(o + 3 * j + 1) * l[1]).astype(F32)).astype(F32)
            a = (a + (n(o + 3 * j + 2) * l[2]).astype(F32)).astype(F32)
            a = (a + n(o + 9 + j)).astype(F32)
            t.append((a + (n(o + 12 + j) * lo.unary(a, "tanh")).astype(F32)).astype(F32))
        l = t
    a = (n(54) * l[0]).astype(F32)
    a = (a + (n(55) * l[1]).astype(F32)).astype(F32)
    a = (a + (n(56) * l[2]).astype(F32)).astype(F32)
    return (a + n(57)).astype(F32)


def _eb_logits64(net, x):
    """(value, error bound of the float32 evaluation)"""
    n = lambda i: net[..., i].astype(np.float64)
    l, e = [], []
    for j in range(3):
        a = n(j) * x + n(3 + j)
        ea = 4 * U * (np.abs(n(j) * x) + np.abs(n(3 + j)))
        l.append(a + n(6 + j) * np.tanh(a))
        e.append(ea + np.abs(n(6 + j)) * (ea + 2 * U) + 2 * U * (np.abs(a) + np.abs(n(6 + j))))
    for layer in range(3):
        o = 9 + 15 * layer
        t, et = [], []
        for j in range(3):
            w = [n(o + 3 * j + i) for i in range(3)]
            a = w[0] * l[0] + w[1] * l[1] + w[2] * l[2] + n(o + 9 + j)
            ea = sum(np.abs(w[i]) * e[i] for i in range(3)) + 4 * U * (sum(np.abs(w[i] * l[i]) for i in range(3)) + np.abs(n(o + 9 + j)))
            f = n(o + 12 + j)
            t.append(a + f * np.tanh(a))
            et.append(ea + np.abs(f) * (ea + 2 * U) + 2 * U * (np.abs(a) + np.abs(f)))
        l, e = t, et
    w = [n(54 + i) for i in range(3)]
    a = w[0] * l[0] + w[1] * l[1] + w[2] * l[2] + n(57)
    ea = sum(np.abs(w[i]) * e[i] for i in range(3)) + 4 * U * (sum(np.abs(w[i] * l[i]) for i in range(3)) + np.abs(n(57)))
    return a, ea


def eb_restate(c, d, mutate=None):
    B, HW, Cc = c["B"], c["HW"], c["C"]
    med = d["med"]
    if c["kind"] == "EB_QUANT":
        sym = to_sym((d["z"] - med).astype(F32), mutate)
        return dict(sym=_tr(sym).reshape(B, -1), out=(sym.astype(F32) + med).astype(F32).reshape(B * HW, Cc))
    if c["kind"] == "EB_DEQUANT":
        s = d["sym"].transpose(0, 2, 1).astype(F32)
        return dict(out=(s if mutate == "median_dropped" else (s + med).astype(F32)).reshape(B * HW, Cc))
    v = (d["sym"].astype(F32) + med.reshape(1, Cc, 1)).astype(F32)
    net = d["net"].reshape(1, Cc, 1, EB_NET)
    lower, upper = _eb_logits32(net, (v - F32(0.5)).astype(F32)), _eb_logits32(net, (v + F32(0.5)).astype(F32))
    sign = -np.sign((lower + upper).astype(F32)).astype(F32)
    l = np.abs((lo.unary((sign * upper).astype(F32), "sigmoid") - lo.unary((sign * lower).astype(F32), "sigmoid")).astype(F32))
    return dict(out=np.where(l > F32(1e-9), l, F32(1e-9)).astype(F32).reshape(B, -1))


def eb_check64(c, d, outs):
    B, HW, Cc = c["B"], c["HW"], c["C"]
    med = d["med"].astype(np.float64)
    if c["kind"] == "EB_QUANT":
        v = d["z"].astype(np.float64) - med
        r, excl = _decision(v, _rnd(v))
        got = outs["sym"].reshape(B, Cc, HW).transpose(0, 2, 1)
        bad = (got != r) & ~excl & _dec_mask(v)
        zh = got.astype(np.float64) + med
        return [("sym", not bad.any(), int(bad.sum()), int(excl.sum())),
                _bounded("out", outs["out"], zh.reshape(B * HW, Cc), 2 * _rnd(zh).reshape(B * HW, Cc) + TINY)]
    if c["kind"] == "EB_DEQUANT":
        zh = d["sym"].transpose(0, 2, 1).astype(np.float64) + med
        return [_bounded("out", outs["out"], zh.reshape(B * HW, Cc), 2 * _rnd(zh).reshape(B * HW, Cc) + TINY)]
    v = d["sym"].astype(np.float64) + med.reshape(1, Cc, 1)
    ev = _rnd(v)
    net = d["net"].reshape(1, Cc, 1, EB_NET)

    def logits(x):
        """value and error bound at the float32 argument fl(x): the network's own error plus the move of the (monotone) logits over
        the argument's error, taken on both sides"""
        ein = ev + U * np.abs(x)
        a, ea = _eb_logits64(net, x)
        hi, _ = _eb_logits64(net, x + ein)
        lw, _ = _eb_logits64(net, x - ein)
        return a, ea + 2 * np.maximum(np.abs(hi - a), np.abs(lw - a))

    lower, el = logits(v - 0.5)
    upper, eu = logits(v + 0.5)
    tot = lower + upper
    sign = -np.sign(tot)
    sig = lambda t: 0.5 * (1.0 + np.tanh(0.5 * t))
    dsig = lambda t, e: (lambda a: sig(a) * (1 - sig(a)))(np.maximum(np.abs(t) - e, 0.0))
    su, sl = sig(sign * upper), sig(sign * lower)
    lik = np.maximum(np.abs(su - sl), 1e-9)
    # a sign the float32 sum may see differently turns sigma(t) into 1 - sigma(t) on both terms: the same difference, rounded at the
    # complementary magnitudes
    flip = (np.abs(tot) <= el + eu + U * np.abs(tot)) & (tot != 0)
    mag = np.where(flip, np.maximum(su + sl, 2 - su - sl), su + sl)
    bnd = 4 * U * mag + dsig(upper, eu) * eu + dsig(lower, el) * el + U * lik + U * 1e-9
    return [_bounded("out", outs["out"], lik.reshape(B, -1), 2 * bnd.reshape(B, -1) + TINY)]


def eb_specs(c, d):
    B, HW, Cc = c["B"], c["HW"], c["C"]
    sp = [spec("aux0", d["med"].reshape(1, -1))]
    if c["kind"] == "EB_QUANT":
        return sp + [spec("x", d["z"].reshape(B * HW, Cc)), spec("sym", shape=(B, Cc * HW), dtype=np.int32, out=True),
                     spec("out", shape=(B * HW, Cc), dtype=F32, out=True)]
    sp.append(spec("sym", d["sym"].reshape(B, -1)))
    if c["kind"] == "EB_DEQUANT":
        return sp + [spec("out", shape=(B * HW, Cc), dtype=F32, out=True)]
    return sp + [spec("aux1", d["net"].reshape(1, -1)), spec("out", shape=(B, Cc * HW), dtype=F32, out=True)]


def eb_cases():
    cs = []
    for kind in ("EB_QUANT", "EB_DEQUANT", "EB_LIK"):
        for Cc in (192, 320):
            for HW in (1, 4, 16):
                cs.append(case(f"{kind.lower()}_c{Cc}_hw{HW}", kind, "SINGLE", B=2, HW=HW, C=Cc))
        cs.append(case(f"{kind.lower()}_grid_stride", kind, "SINGLE", B=1, HW=2731, C=192))         # n = 524352 > 2048 * 256
    return cs


# ================================================================================================================ REM combine, NCHW slice
def rem_data(c):
    r = _rng(c["name"])
    B, HW = c["B"], c["HW"]
    scale = (0.6 + 0.7 * r.standard_normal((B, HW, 32))).astype(F32)
    mu = r.standard_normal((B, HW, 32)).astype(F32)
    ret = r.standard_normal((B, HW, 64 if c["mu"] else 32)).astype(F32)
    ts = np.array([np.quantile(scale[b], 0.4) for b in range(B)]).astype(F32)
    tb = np.array([np.quantile(scale[b], 0.7) for b in range(B)]).astype(F32)
    ts[0] = scale[0].reshape(-1)[min(5, HW * 32 - 1)]
    return dict(scale=scale, mu=mu, ret=ret, thr_star=ts, thr_bar=tb)


def _rem(c, d, dt, mutate=None):
    """rem_combine_kernel in the kernel's own order (the float64 side is rem_check64, written apart from this)"""
    B = c["B"]
    s = d["scale"].astype(dt)
    ms, mb = (c["mode_bar"], c["mode_star"]) if mutate == "star_bar_swapped" else (c["mode_star"], c["mode_bar"])
    ts, tb = (d["thr_bar"], d["thr_star"]) if mutate == "star_bar_swapped" else (d["thr_star"], d["thr_bar"])
    f = lambda mode, thr: (s >= thr.astype(dt).reshape(B, 1, 1)).astype(dt) if mode == 1 else (np.ones_like(s) if mode == 2 else np.zeros_like(s))
    att = np.rint(f(ms, ts) - f(mb, tb)).astype(dt)
    ret = d["ret"].astype(dt)
    if not c["mu"]:
        return dict(out=((ret * att).astype(dt) + s).astype(dt))
    a, b = (ret[..., 32:], ret[..., :32]) if mutate == "halves_swapped" else (ret[..., :32], ret[..., 32:])
    return dict(out2=((a * att).astype(dt) + d["mu"].astype(dt)).astype(dt), out=((b * att).astype(dt) + s).astype(dt))


def rem_restate(c, d, mutate=None):
    return {k: v.reshape(-1, 32) for k, v in _rem(c, d, F32, mutate).items()}


def rem_check64(c, d, outs):
    """apply_latent_enhancement of the REM (CHProgREM.py:395-416) from its definition: both masks threshold the UNREFINED scale,
    attention = round(mask_star - mask_bar), scale <- ret_scale * attention + scale and, in the mu_std form where the net returns
    cat(mu part, scale part) along the channels, mu <- ret_mu * attention + mu"""
    import torch
    B, HW = c["B"], c["HW"]
    scale = torch.from_numpy(d["scale"]).double()
    ret = torch.from_numpy(d["ret"]).double()

    def channel_mask(mode, thr):
        if mode == 1:
            return (scale >= torch.from_numpy(thr).double().view(B, 1, 1)).double()
        return torch.ones_like(scale) if mode == 2 else torch.zeros_like(scale)

    attention = torch.round(channel_mask(c["mode_star"], d["thr_star"]) - channel_mask(c["mode_bar"], d["thr_bar"]))
    res = []
    if c["mu"]:
        ret_mu, ret_scale = torch.chunk(ret, 2, dim=-1)
        mu = (ret_mu * attention + torch.from_numpy(d["mu"]).double()).numpy().reshape(-1, 32)
        res.append(_bounded("out2", outs["out2"], mu, 2 * _rnd(mu) + TINY))
    else:
        ret_scale = ret
    new = (ret_scale * attention + scale).numpy().reshape(-1, 32)
    res.append(_bounded("out", outs["out"], new, 2 * _rnd(new) + TINY))
    return res


def rem_specs(c, d):
    P = c["B"] * c["HW"]
    sp = [spec("x", d["ret"].reshape(P, -1), ld=c["ld_ret"]), spec("out", d["scale"].reshape(P, 32), ld=c["ld"], coff=c["coff"], out=True)]
    if c["mode_star"] == 1:
        sp.append(spec("thr", d["thr_star"].reshape(1, -1)))
    if c["mode_bar"] == 1:
        sp.append(spec("thr_bar", d["thr_bar"].reshape(1, -1)))
    if c["mu"]:
        sp.append(spec("out2", d["mu"].reshape(P, 32), ld=c["ld"], coff=c["coff"], out=True))
    return sp


def rem_cases():
    cs = []
    i = 0
    for mu in (0, 1):
        for ms in (0, 1, 2):
            for mb in (0, 1, 2):
                ldr = (64, 96, 128)[i % 3] if mu else (32, 64, 96)[i % 3]
                wide = i % 2
                cs.append(case(f"rem_{'mu' if mu else 'sc'}_{ms}{mb}", "REM", "SINGLE", B=2, HW=(63, 64, 1)[i % 3], mu=mu, mode_star=ms, mode_bar=mb,
                               ld_ret=ldr, ld=320 if wide else 32, coff=64 if wide else 0))
                i += 1
    cs.append(case("rem_grid_stride", "REM", "SINGLE", B=1, HW=32769, mu=1, mode_star=1, mode_bar=1, ld_ret=64, ld=32, coff=0))   # n > 4096 * 256
    return cs


def nchw_data(c):
    return dict(src=_rng(c["name"]).standard_normal((c["B"], c["C"], c["HW"])).astype(F32))


def nchw_restate(c, d, mutate=None):
    return dict(out=np.ascontiguousarray(d["src"].transpose(0, 2, 1)).reshape(-1, c["C"]))


def nchw_check64(c, d, outs):
    return [_equal("out", outs["out"], d["src"].astype(np.float64).transpose(0, 2, 1).reshape(-1, c["C"]))]


def nchw_cases():
    return [case(f"nchw_c{Cc}_hw{HW}", "NCHW_SLICE", "SINGLE", B=2, C=Cc, HW=HW, pad=17) for Cc in (32, 3) for HW in (1, 63, 4096)]


# ================================================================================================================ SE squeeze, maxpool
def se_data(c):
    r = _rng(c["name"].split("@")[0])
    Cc, HW = c["C"], c["HW"]
    x = (r.standard_normal((3, HW, Cc)) + 0.5).astype(F32)[: c["B"]]
    fc1 = (r.standard_normal((Cc // 16, Cc)) * (2.0 / Cc) ** 0.5).astype(F32)          # z = O(1): the sigmoid is not saturated
    fc1[0] = np.abs(fc1[0])                                                             # the means are positive: this hidden unit is never clipped by the ReLU
    fc2 = (r.standard_normal((Cc, Cc // 16)) * 0.7).astype(F32)
    return dict(x=np.ascontiguousarray(x), fc1=fc1, fc2=fc2)


def se_chunk_sums(x):
    """se_partial_kernel: x [B, HW, C] -> part [B, nchunk, C]; per chunk G = 1024 / C pixel groups, group g adds pixels g, g + G, ... in
    ascending order from +0, then the groups are added in ascending g from +0"""
    B, HW, Cc = x.shape
    G = 1024 // Cc
    nchunk = (HW + SE_CHUNK - 1) // SE_CHUNK
    pad = np.zeros((B, nchunk * SE_CHUNK, Cc), F32)          # +0 tail: adding +0 to a chain that never holds -0 changes nothing
    pad[:, :HW] = x
    pad = pad.reshape(B, nchunk, SE_CHUNK // G, G, Cc)
    acc = np.zeros((B, nchunk, G, Cc), F32)
    for i in range(SE_CHUNK // G):
        acc = acc + pad[:, :, i]
    part = np.zeros((B, nchunk, Cc), F32)
    for g in range(G):
        part = part + acc[:, :, g]
    return part


def se_restate(c, d, mutate=None):
    B, HW, Cc = c["B"], c["HW"], c["C"]
    out = _se_scale(c, d, mutate)
    out["out2"] = se_chunk_sums(d["x"]).reshape(B, -1)
    return out


def _se_scale(c, d, mutate=None):
    B, HW, Cc = c["B"], c["HW"], c["C"]
    x = d["x"].reshape(B, 1, HW, Cc)
    if mutate == "mean_by_chunk":
        m = (uc.se_mean(x) * F32(HW) / F32(min(HW, SE_CHUNK))).astype(F32)
        h = uc.relu(uc.conv_nhwc(m.reshape(B, 1, 1, Cc), np.ascontiguousarray(d["fc1"].T)[None], [(0, 0)], 1, 1, 1))
        z = uc.conv_nhwc(h, np.ascontiguousarray(d["fc2"].T)[None], [(0, 0)], 1, 1, 1)
        return dict(out=uc.unary(z.reshape(B, Cc), "sigmoid"))
    return dict(out=uc.se_scale(x, d["fc1"], d["fc2"]).reshape(B, Cc))


def se_check64(c, d, outs):
    B, HW, Cc = c["B"], c["HW"], c["C"]
    x = d["x"].astype(np.float64)
    f1, f2 = d["fc1"].astype(np.float64), d["fc2"].astype(np.float64)
    mean = x.mean(axis=1)
    G = 1024 // Cc
    depth = SE_CHUNK // G + G + (HW + SE_CHUNK - 1) // SE_CHUNK + 1
    em = depth * U * np.abs(x).mean(axis=1)
    h = mean @ f1.T
    eh = em @ np.abs(f1.T) + (Cc + 1) * U * (np.abs(mean) @ np.abs(f1.T))
    hr = np.maximum(h, 0.0)
    z = hr @ f2.T
    ez = eh @ np.abs(f2.T) + (Cc // 16 + 1) * U * (hr + eh) @ np.abs(f2.T)
    s = 1.0 / (1.0 + np.exp(-z))
    a = np.maximum(np.abs(z) - ez, 0.0)
    sa = 1.0 / (1.0 + np.exp(-a))
    nchunk = (HW + SE_CHUNK - 1) // SE_CHUNK
    xp = np.zeros((B, nchunk * SE_CHUNK, Cc))
    xp[:, :HW] = x
    xp = xp.reshape(B, nchunk, SE_CHUNK, Cc)
    part = xp.sum(axis=2).reshape(B, -1)                                  # the scratch: the sum of each chunk of PC_SE_CHUNK pixels
    epart = (SE_CHUNK // G + G) * U * np.abs(xp).sum(axis=2).reshape(B, -1)
    return [_bounded("out", outs["out"], s, 2 * (4 * U * s + sa * (1 - sa) * ez) + TINY),
            _bounded("out2", outs["out2"], part, 2 * epart + TINY)]


def se_specs(c, d):
    B, HW, Cc = c["B"], c["HW"], c["C"]
    nchunk = (HW + SE_CHUNK - 1) // SE_CHUNK
    return [spec("x", d["x"].reshape(B * HW, Cc)), spec("aux0", d["fc1"].reshape(1, -1)), spec("aux1", d["fc2"].reshape(1, -1)),
            spec("out2", shape=(B, nchunk * Cc), dtype=F32, out=True, ld=nchunk * Cc), spec("out", shape=(B, Cc), dtype=F32, out=True)]


def se_cases():
    cs = []
    for Cc in (16, 32, 64, 128):
        for HW in (1, SE_CHUNK - 1, SE_CHUNK, SE_CHUNK + 1, 3 * SE_CHUNK + 5):
            cs.append(case(f"se_c{Cc}_hw{HW}@b1", "SE", "SINGLE", B=1, HW=HW, C=Cc))
            if HW in (1, SE_CHUNK + 1):
                cs.append(case(f"se_c{Cc}_hw{HW}@b3", "SE", "SINGLE", B=3, HW=HW, C=Cc))     # same first image: the same bits
    return cs


def pool_data(c):
    r = _rng(c["name"])
    x = r.standard_normal((c["B"], c["H"], c["W"], c["C"])).astype(F32)
    if c.get("special"):
        f = x.reshape(c["B"], c["H"] // 2, 2, c["W"] // 2, 2, c["C"])       # [b, oy, dy, ox, dx, ch] view
        for i, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            f[0, 0, dy, i % (c["W"] // 2), dx, i % c["C"]] = np.nan        # NaN in each of the four window positions
            f[-1, -1, dy, -1 - i % (c["W"] // 2), dx, (i + 1) % c["C"]] = np.uint32(0xffc00000 + i).view(F32)
        # zeros of both signs, the later one of the other sign, everything else in the window below them
        ch = 2 % c["C"]
        f[0, -1, :, 0, :, ch] = -5.0
        f[0, -1, 0, 0, 0, ch], f[0, -1, 1, 0, 1, ch] = -0.0, 0.0
        ch2 = 3 % c["C"]
        f[0, -1, :, 0, :, ch2] = -5.0
        f[0, -1, 0, 0, 1, ch2], f[0, -1, 1, 0, 0, ch2] = 0.0, -0.0
    return dict(x=x)


def pool_restate(c, d, mutate=None):
    x = d["x"]
    if mutate == "nan_dropped":
        v = [x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]]
        m = v[0]
        for a in v[1:]:
            m = np.where(a > m, a, m)
        return dict(out=m.astype(F32).reshape(-1, c["C"]))
    return dict(out=uc.maxpool2(x).reshape(-1, c["C"]))


def pool_check64(c, d, outs):
    x = d["x"].astype(np.float64)
    B, H, W, Cc = x.shape
    w = x.reshape(B, H // 2, 2, W // 2, 2, Cc)
    return [_equal("out", outs["out"], w.max(axis=(2, 4)).reshape(-1, Cc))]          # np.max propagates NaN, as MaxPool2d does


def pool_cases():
    cs = [case(f"pool_c{Cc}_{H}x{W}", "MAXPOOL", "SINGLE", B=2, H=H, W=W, C=Cc, special=True) for Cc in (4, 32, 64) for H, W in ((2, 2), (6, 10))]
    cs.append(case("pool_grid_stride", "MAXPOOL", "SINGLE", B=1, H=2 * 1449, W=2 * 1448, C=4, special=True))     # 2098152 quads > 8192 * 256
    return cs


# ================================================================================================================ dispatch
def family(c):
    k = c["kind"]
    return "prep" if k.startswith("PREP") else ("eb" if k.startswith("EB") else k.lower())


_DATA = dict(prep=prep_data, attention=att_data, gdn=gdn_data, quantile=q_data, eb=eb_data, rem=rem_data, nchw_slice=nchw_data, se=se_data,
             maxpool=pool_data)
_RESTATE = dict(prep=prep_restate, attention=att_restate, gdn=gdn_restate, quantile=q_restate, eb=eb_restate, rem=rem_restate,
                nchw_slice=nchw_restate, se=se_restate, maxpool=pool_restate)
_CHECK = dict(prep=prep_check64, attention=att_check64, gdn=gdn_check64, quantile=q_check64, eb=eb_check64, rem=rem_check64,
              nchw_slice=nchw_check64, se=se_check64, maxpool=pool_check64)


def make_data(c):
    return _DATA[family(c)](c)


def restate(c, d, mutate=None):
    """{output field: [rows, n] array} in the contract's float32 / integers"""
    return _RESTATE[family(c)](c, d, mutate)


def n_elements(c, outs):
    return max(v.size for v in outs.values())


def exclusion_cap(c, outs):
    """at most 1e-4 of a case's elements; below 10^4 elements the planted ties plus one"""
    n = n_elements(c, outs)
    return int(1e-4 * n) if n >= 10 ** 4 else N_PLANTED + 1


def check64(c, d, outs):
    """(ok, [(output, ok, ratio or mismatches, excluded)], worst ratio over the bounded outputs): check (b) of the matrix, the exclusion
    cap included"""
    res = _CHECK[family(c)](c, d, outs)
    cap = exclusion_cap(c, outs)
    ok = all(r[1] for r in res) and all(r[3] <= cap for r in res)
    ratios = [r[2] for r in res if isinstance(r[2], float)]
    return ok, res, (max(ratios) if ratios else 0.0)


def check64_normal(c, d, outs, exclude=None):
    """check64 for operands outside the ordinary (tests/hostile_values.py): the same references and the same bounds, asserted on the
    elements whose float64 value is finite and zero or of normal range and whose bound is finite -- less `exclude`, {output: mask}, where
    float64 says nothing about the float32 contract (a square that overflows in float32 only); symbols are judged where the float64
    operand is finite and inside the int32 range.  (ok, results, worst ratio, [(output, judged, of)])"""
    _NORMAL_ONLY[:] = [dict(exclude or {})]
    try:
        with np.errstate(all="ignore"):
            ok, res, ratio = check64(c, d, outs)
        return ok, res, ratio, list(_NORMAL_ONLY[1:])
    finally:
        _NORMAL_ONLY[:] = [None]


def specs(c, d):
    f = family(c)
    if f == "prep":
        return prep_specs(c, d)
    if f == "attention":
        return att_specs(c, d)
    if f == "gdn":
        P, Cc = c["P"], c["C"]
        return [spec("x", d["x"].reshape(P, Cc)), spec("aux0", d["beta"].reshape(1, -1)), spec("aux1", d["gamma"].reshape(1, -1)),
                spec("out", shape=(P, Cc), dtype=F32, out=True)]
    if f == "quantile":
        B, HW, Cc = c["B"], c["HW"], c["C"]
        # rows of C inside pixels ld wide, images sb apart: one spec row per pixel, the batch gap as extra rows of padding
        sp = [dict(spec("scale", d["scale"].reshape(B * HW, Cc), ld=c["ld"], lead=c["lead"]), batch=(B, HW, c["sb_pad"])),
              spec("out", shape=(1, B), dtype=F32, out=True)]
        if c["own_work"]:                              # the caller's scratch, as the codec hands it in: pc_quantile_work_bytes(B) / 4 words
            sp.append(spec("work", shape=(B, QW_STRIDE), dtype=np.uint32, out=True))
        return sp
    if f == "eb":
        return eb_specs(c, d)
    if f == "rem":
        return rem_specs(c, d)
    if f == "nchw_slice":
        return [spec("x", d["src"].reshape(c["B"], -1), ld=c["C"] * c["HW"] + c["pad"]), spec("out", shape=(c["B"] * c["HW"], c["C"]), dtype=F32, out=True)]
    if f == "se":
        return se_specs(c, d)
    return [spec("x", d["x"].reshape(-1, c["C"])), spec("out", shape=(c["B"] * (c["H"] // 2) * (c["W"] // 2), c["C"]), dtype=F32, out=True)]


def scalars(c, d):
    f = family(c)
    if f == "prep":
        return prep_scalars(c, d)
    if f == "attention":
        return att_scalars(c, d)
    if f == "gdn":
        return dict(B=1, H=1, W=c["P"], C=c["C"], inverse=c["inverse"])
    if f == "quantile":
        return dict(B=c["B"], HW=c["HW"], C=c["C"], ld_scale=c["ld"], q=float(d["q"]), sb=(c["HW"] * c["ld"] + c["sb_pad"]) if (c["sb_pad"] or c["name"].endswith("_sb")) else 0)
    if f == "eb":
        return dict(B=c["B"], HW=c["HW"], C=c["C"])
    if f == "rem":
        return dict(B=c["B"], HW=c["HW"], ld_x=c["ld_ret"], ld_scale=c["ld"], ld_mu=c["ld"], mode_star=c["mode_star"], mode_bar=c["mode_bar"])
    if f == "nchw_slice":
        return dict(B=c["B"], HW=c["HW"], C=c["C"], sb=c["C"] * c["HW"] + c["pad"])
    if f == "se":
        return dict(B=c["B"], HW=c["HW"], C=c["C"])
    return dict(B=c["B"], H=c["H"], W=c["W"], C=c["C"])


#: outputs whose contents are scratch (only what surrounds them is compared) or are compared by the float64 bound only (not specified bit-exact)
SCRATCH = {("QUANTILE", "work")}         # contents are the launcher's own; the guard bands around them are compared
BOUND_ONLY = {("PREP_ENC", "lik"), ("EB_LIK", "out")}


def matrix():
    return prep_cases() + att_cases() + gdn_cases() + q_cases() + eb_cases() + rem_cases() + nchw_cases() + se_cases() + pool_cases()


MUTATIONS = {
    # mutation: family
    "bias_transposed": "attention", "roll_direction": "attention", "region_boundary": "attention", "channel_major": "attention",
    "table_le": "prep", "mask_gt": "prep", "round_away": "prep", "ybase_added": "prep", "index_from_s": "prep", "yadd_dropped": "prep",
    "lik_from_sym": "prep", "star_bar_swapped": "rem", "halves_swapped": "rem", "median_dropped": "eb", "nan_dropped": "maxpool",
    "mean_by_chunk": "se",
}


def refusals():
    """(name, base case, desc overrides): launches the launchers must refuse on the host (PC_ERR_ARG, nothing launched).  An override
    value ("lead", field, bytes) moves a pointer, None clears it."""
    return [
        ("ntable_1", "enc_mode1_none", dict(ntable=1)), ("ntable_65", "enc_mode1_none", dict(ntable=65)),
        ("idx_ntable_1", "idxtwin@aligned", dict(ntable=1)), ("idx_ntable_65", "idxtwin@aligned", dict(ntable=65)),
        ("prep_c_16", "enc_mode1_none", dict(C=16)), ("deq_c_16", "deqtwin@aligned", dict(C=16)),
        ("att_c_mod_heads", "att_8_24_s4_ji0", dict(heads=7)), ("att_h_mod_ws", "att_8_24_s4_ji0", dict(H=17)),
        ("att_w_mod_ws", "att_4_40_s2_ji0", dict(W=10)), ("att_shift_ws", "att_4_80_s2_ji1", dict(shift=4)),
        ("att_shift_negative", "att_8_24_s4_ji0", dict(shift=-1)),
        # every earlier check passes (C % heads, H % ws, W % ws, 0 <= shift < ws): only the (ws, d) dispatch can refuse
        ("att_unsupported_4_24", "att_8_24_s1_ji0", dict(ws=4)), ("att_unsupported_8_48", "att_8_24_s0_ji0", dict(heads=4)),
        ("att_null_bias", "att_8_24_s4_ji0", dict(aux0=None)),
        ("eb_quant_null", "eb_quant_c192_hw4", dict(x=None)), ("eb_quant_b0", "eb_quant_c192_hw4", dict(B=0)),
        ("eb_dequant_null", "eb_dequant_c192_hw4", dict(aux0=None)), ("eb_dequant_hw0", "eb_dequant_c192_hw4", dict(HW=0)),
        ("eb_lik_null", "eb_lik_c192_hw4", dict(aux1=None)), ("eb_lik_c0", "eb_lik_c192_hw4", dict(C=0)),
        ("rem_null_thr", "rem_sc_11", dict(thr=None)), ("nchw_b0", "nchw_c3_hw63", dict(B=0)),
        ("se_c_48", "se_c32_hw1@b3", dict(C=48)), ("se_misaligned_x", "se_c32_hw1@b3", dict(x=("lead", 4))),
        ("se_b_65536", "se_c32_hw1@b3", dict(B=65536)),
        ("pool_odd_h", "pool_c32_6x10", dict(H=5)), ("pool_odd_w", "pool_c32_6x10", dict(W=9)), ("pool_c_6", "pool_c32_6x10", dict(C=6)),
        ("quantile_b0", "q_8192", dict(B=0)), ("unknown_kind", "q_8192", dict(kind=99)), ("size_mismatch", "q_8192", dict(size=8)),
    ]

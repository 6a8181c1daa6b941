"""CPU check of tests/hostile_values.py (no GPU): the table holds its own conditions under the restatements alone -- the subnormal
classes give subnormal outputs, the sprinkled NaN set is the one the geometry gives, the sweep's identity layer returns its argument --
and the cases can fail: every mutant of hostile_values.MUTANTS differs from the restatement on its named case, while the mutants of
flushing and of the k order are silent on the ordinary operands of conv_contract.make_data, which is the gap the table closes."""
import numpy as np
import pytest

from oracle import liboracle as lo
from tests import conv_contract as cc
from tests import hostile_values as hv
from tests import stage_contract as sc

F32 = np.float32
CONV = {hc["name"]: hc for hc in hv.conv_cases()}
STAGE = {hc["name"]: hc for hc in hv.stage_cases()}


def _by_class(klass):
    return sorted(n for n, hc in CONV.items() if hc["klass"] == klass)


def _subnormal(a):
    u = np.ascontiguousarray(a, F32).view(np.uint32)
    return ((u & 0x7F800000) == 0) & ((u & 0x007FFFFF) != 0)


def test_table_covers_both_matrices():
    assert len(CONV) == len(hv.conv_cases()) and len(STAGE) == len(hv.stage_cases())
    for klass in ("sub_in", "sprinkle"):
        assert {tuple(CONV[n]["c"]["expect"]) for n in _by_class(klass)} >= cc.REQUIRED, klass
    assert {CONV[n]["c"]["epi"] for n in _by_class("sprinkle")} == set(cc.EPI)
    for klass in ("sub_prod", "overflow", "cancel"):
        assert len(_by_class(klass)) >= 9, klass
    assert any(CONV[n]["c"]["ngroup"] == 2 for n in _by_class("overflow"))
    kinds = {hc["c"]["kind"] for hc in STAGE.values()}
    assert kinds == {"ATTENTION", "GDN", "SE", "NCHW_SLICE", "PREP_ENC", "PREP_DEC_INDEX", "PREP_DEQUANT", "EB_QUANT", "EB_DEQUANT"}
    for kind in ("PREP_ENC", "PREP_DEC_INDEX", "PREP_DEQUANT"):
        assert {hc["c"]["expect"] for hc in STAGE.values() if hc["c"]["kind"] == kind} == {"PREP_SCALAR", "PREP_VEC"}
    assert {hc["c"]["expect"] for hc in STAGE.values() if hc["c"]["kind"] == "ATTENTION"} == {"ATT_8_24", "ATT_4_80", "ATT_4_40"}


# ---------------------------------------------------------------------------------------------------------------- conv conditions
@pytest.mark.parametrize("name", _by_class("sub_in") + _by_class("sub_prod"))
def test_subnormal_classes_give_subnormal_outputs(name):
    hc = CONV[name]
    d = hv.conv_data(hc)
    for g in range(hc["c"]["ngroup"]):
        out = hv.conv_restate(hc["c"], d, group=g)
        frac = float(_subnormal(out).mean())
        print(f"{name} group {g}: {100 * frac:.2f} % of {out.size} outputs are non-zero subnormals")
        assert frac >= 0.9


@pytest.mark.parametrize("name", _by_class("sprinkle"))
def test_sprinkled_values_poison_their_receptive_fields(name):
    hc = CONV[name]
    c = hc["c"]
    d = hv.conv_data(hc)
    for g in range(c["ngroup"]):
        out = hv.conv_restate(c, d, group=g)
        nan, nonfinite = np.isnan(out), ~np.isfinite(out)
        r_nan, r_any = hv.field_sets(c, d, g)
        r_nan, r_any = r_nan[..., None], r_any[..., None]
        print(f"{name} group {g}: {100 * nonfinite.mean():.2f} % non-finite, {int(nan.sum())} NaN, {int(np.isinf(out).sum())} inf")
        assert nonfinite.mean() <= 0.5
        # the NaN set from the geometry alone: every output whose field holds a NaN input is NaN in every channel; nothing outside the
        # field of a non-finite or near-FLT_MAX input is non-finite (inside it, inf - inf and GELU(-inf) add value-dependent NaNs)
        assert not (nonfinite & ~r_any).any()
        if c["epi"] in hv.DROPS_NAN:
            assert not nan.any()
        else:
            assert nan.any()
            assert (nan | ~r_nan).all()
        if c["epi"] in hv.CAN_GIVE_INF and not c["fused_gdn"]:       # the fused GDN divides by the norm: inf * rsqrt(inf) is NaN
            assert np.isinf(out).any()
        # and the outputs outside every field are those of the ordinary operands, bit for bit
        if not (c["fused_gdn"] or c["square"]):
            plain = cc.restate(c, dict(d, **{k: np.where(_hostile(d[k]), F32(0.5), d[k]) for k in ("x", "x1") if k in d}), group=g)
            keep = np.broadcast_to(~r_any, out.shape)
            assert np.array_equal(out.view(np.uint32)[keep], plain.view(np.uint32)[keep])


@pytest.mark.parametrize("name", _by_class("sprinkle_nan"))
def test_nan_set_equals_the_receptive_field(name):
    """sprinkled with NaN and finite values only, nothing but the NaN inputs makes a NaN: the NaN set of the restatement EQUALS the set of
    outputs whose receptive field (from the geometry alone) holds a NaN input, in every channel; RELU alone has none; nothing is inf"""
    hc = CONV[name]
    c = hc["c"]
    d = hv.conv_data(hc)
    for g in range(c["ngroup"]):
        out = hv.conv_restate(c, d, group=g)
        r_nan, _ = hv.field_sets(c, d, g)
        assert r_nan.any() and not np.isinf(out).any()
        if c["epi"] in hv.DROPS_NAN:
            assert not np.isnan(out).any()
        else:
            assert np.array_equal(np.isnan(out), np.broadcast_to(r_nan[..., None], out.shape))


def _hostile(v):
    with np.errstate(invalid="ignore"):
        return ~np.isfinite(v) | (np.abs(v) >= 1e38)


@pytest.mark.parametrize("name", _by_class("overflow") + _by_class("cancel"))
def test_the_k_order_decides(name):
    hc = CONV[name]
    c = hc["c"]
    d = hv.conv_data(hc)
    for g in range(c["ngroup"]):
        out = hv.conv_restate(c, d, group=g)
        asc = hv.conv_restate(c, d, "ascending_k", group=g)
        bad, _ = hv.same_bits_or_nan(asc, out)
        pattern = (np.isnan(asc) != np.isnan(out)) | (np.isinf(asc) != np.isinf(out))
        print(f"{name} group {g}: ascending k changes {100 * bad.mean():.1f} % of the outputs, the inf / NaN pattern of {100 * pattern.mean():.1f} %")
        assert bad.mean() >= 0.1
        if hc["klass"] == "overflow" and c["epi"] in hv.CAN_GIVE_INF:
            assert pattern.mean() >= 0.05
            assert np.isfinite(out).any() and not np.isfinite(out).all()
        if hc["klass"] == "cancel":
            assert np.isfinite(out).all() and np.isfinite(asc).all()


# ---------------------------------------------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("epi", list(cc.EPI))
def test_sweep_shortcut_is_the_restatement(epi):
    """the identity layer over all 2^24 arguments of the epilogue, 16 channels: the full restatement (the oracle's chains) returns x bit
    for bit on every all-finite pixel and NaN on the others, and `sweep_restate` is that restatement"""
    x = hv.sweep_values(epi)
    c, d = hv.sweep_case(epi, "l0", x)
    with np.errstate(all="ignore"):
        v = cc._chains(c, d["x"], d["w"], d["b"])
        full = cc.restate(c, d)
    fin = np.isfinite(d["x"]).all(axis=3)
    assert int(fin.sum()) * 16 == 16711680
    assert np.array_equal(v[fin].view(np.uint32), d["x"][fin].view(np.uint32))
    assert np.isnan(v[~fin]).all() and not np.isfinite(d["x"][~fin]).any()
    bad, _ = hv.same_bits_or_nan(hv.sweep_restate(c, d), full)
    assert not bad.any()


@pytest.mark.parametrize("form", list(hv.SMALL_FORMS))
def test_sweep_small_cases_and_the_wide_form(form):
    """the branch-point list and the bias-delivered non-finite pre-activations, every epilogue, and (NONE) the 64-channel identity over
    all 2^24 arguments: the shortcut is the restatement"""
    for epi in cc.EPI:
        Cc = hv.SMALL_FORMS[form][0]
        for values, bias in ((hv.branch_values(), None), (np.zeros(4 * Cc, F32), hv.bias_values(Cc))):
            c, d = hv.sweep_case(epi, form, values, bias)
            with np.errstate(all="ignore"):
                full = cc.restate(c, d)
            bad, _ = hv.same_bits_or_nan(hv.sweep_restate(c, d), full)
            assert not bad.any(), (epi, form)
    if form == "uni_fast":
        c, d = hv.sweep_case("NONE", form, hv.sweep_values("NONE"))
        with np.errstate(all="ignore"):
            bad, _ = hv.same_bits_or_nan(hv.sweep_restate(c, d), cc.restate(c, d))
        assert not bad.any()


def test_branch_list_holds_the_branch_points():
    v = hv.branch_values()
    assert np.isfinite(v).all() and v.size % 64 == 0
    for p in (0.625, 1.0, 4.0, 9.5, 87.0, 88.7, 8388608.0):
        for s in (1, -1):
            u = np.array([s * p], F32).view(np.uint32)[0]
            got = set(v.view(np.uint32).tolist())
            assert {int(u) + k for k in range(-4, 5)} <= got, p
    b = hv.bias_values(16)
    assert np.isposinf(b).any() and np.isneginf(b).any() and np.isnan(b).any()


# ---------------------------------------------------------------------------------------------------------------- stages
def test_conversion_rule():
    """(int32_t)pc_roundevenf(v): stage_contract.to_sym (clip, then cast; NaN -> 0) is what the oracle's orc_quantize does, in range it is
    round-half-even, and the wrapping conversion differs only outside |v| < 2^31: at every v >= 2^31, at NaN, at -2^31 - 256, at -2^40"""
    v = hv.quant_values()
    want = sc.to_sym(v)
    assert np.array_equal(lo.quantize(v), want)
    assert want[np.isnan(v)].tolist() == [0, 0, 0]
    assert want[v >= 2.0 ** 31].tolist() == [2 ** 31 - 1] * int((v >= 2.0 ** 31).sum())
    assert want[v <= -2.0 ** 31].tolist() == [-2 ** 31] * int((v <= -2.0 ** 31).sum())
    assert want[v == F32(2147483520.0)].tolist() == [2147483520] and want[v == F32(-2147483520.0)].tolist() == [-2147483520]
    assert want[v == F32(8388607.5)].tolist() == [8388608] and want[v == F32(2.5)].tolist() == [2] and want[v == F32(-1.5)].tolist() == [-2]
    r = np.random.default_rng(3)
    w = np.concatenate([(r.standard_normal(100000) * 10 ** r.uniform(-2, 9, 100000)).astype(F32), (np.arange(-64, 64) / 2).astype(F32)])
    w = w[np.abs(w) < 2.0 ** 31]                                              # in range: plain round-half-even
    assert np.array_equal(sc.to_sym(w), np.rint(w.astype(np.float64)).astype(np.int64).astype(np.int32))
    assert np.array_equal(lo.quantize(w), sc.to_sym(w))
    wrap = sc.to_sym(v, "wrapping")
    differs = wrap != want
    with np.errstate(invalid="ignore"):
        assert not differs[np.abs(v) < 2.0 ** 31].any()
        assert differs[(v >= 2.0 ** 31) | np.isnan(v) | (v == F32(-2.0 ** 40)) | (v == F32(-2.0 ** 31 - 256))].all()


@pytest.mark.parametrize("name", sorted(STAGE))
def test_stage_case_conditions(name):
    hc = STAGE[name]
    c, klass = hc["c"], hc["klass"]
    d = hv.stage_data(hc)
    out = hv.stage_restate(c, d)
    assert sc.specs(c, d) and sc.scalars(c, d) is not None
    fam = sc.family(c)
    if fam == "attention":
        o = out["out"]
        D, T = c["C"] // c["heads"], c["ws"] ** 2
        if klass == "nonfinite":
            assert int(np.isnan(o).sum()) == D + T and not np.isinf(o).any()       # the q token's head, the v channel of its window
        else:
            assert np.isfinite(o).all()
        if klass == "underflow":
            assert _scores_below(c, d, -87.0) > 0.5                              # most exp(s - max) take the exact-zero branch
        if klass == "equal" and not c["shift"]:
            v = d["qkv"][..., 2 * c["C"]:]
            B, H, W, ws = c["B"], c["H"], c["W"], c["ws"]
            mean = v.reshape(B, H // ws, ws, W // ws, ws, -1).astype(np.float64).mean(axis=(2, 4), keepdims=True)
            assert np.abs(o.reshape(B, H // ws, ws, W // ws, ws, -1) - mean).max() < 1e-5
        if klass == "sub_v":
            assert _subnormal(o).mean() > 0.99
    elif fam == "gdn":
        o = out["out"]
        if klass == "x_2m128":
            assert _subnormal(o).mean() > 0.97
        elif klass == "x_2p64":
            assert (np.isinf(o).mean() > 0.9) if c["inverse"] else ((o == 0).mean() > 0.9)     # x sqrt(inf); x rsqrt(inf) = x * 0
        else:
            assert np.isnan(o).any() and np.isnan(o).mean() < 0.5
    elif fam == "se":
        if klass == "one_inf":
            assert int(np.isinf(out["out2"]).sum()) == 1
            assert np.isfinite(out["out"][: c["B"] - 1]).all()                     # the other images do not see it
        else:
            assert _subnormal(out["out2"]).mean() > 0.9 and np.isfinite(out["out"]).all()
    elif fam == "nchw_slice":
        src = np.sort(d["src"].view(np.uint32).reshape(-1))
        assert np.array_equal(np.sort(out["out"].view(np.uint32).reshape(-1)), src)
        nan = src[np.isnan(src.view(F32))]
        assert len(np.unique(nan)) == len(nan) >= 64
    elif klass == "quant":
        sym = out["sym"].reshape(-1)
        assert (sym == 2 ** 31 - 1).sum() >= 5 and (sym == -2 ** 31).sum() >= 5
        assert (sym == 2147483520).sum() == 1 and (sym == 8388608).sum() >= 2
        assert np.isfinite(out["yhat" if fam == "prep" else "out"]).all()


def _scores_below(c, d, t):
    """fraction of (window, head, query, key) scores that lie more than |t| below their row maximum, float64, unshifted windows"""
    B, H, W, Cc, heads, ws = c["B"], c["H"], c["W"], c["C"], c["heads"], c["ws"]
    D = Cc // heads
    x = d["qkv"].astype(np.float64).reshape(B, H // ws, ws, W // ws, ws, 3, heads, D).transpose(5, 0, 1, 3, 6, 2, 4, 7)
    q, k = x[0].reshape(-1, heads, ws * ws, D), x[1].reshape(-1, heads, ws * ws, D)
    s = (q * float(d["fscale"])) @ k.transpose(0, 1, 3, 2) + d["bias"].astype(np.float64)[None]
    return float(((s - s.max(axis=-1, keepdims=True)) < t).mean())


# ---------------------------------------------------------------------------------------------------------------- mutants
def _mutant_differs(mutant):
    where, name = hv.MUTANTS[mutant]
    m = mutant.split("@")[0]
    if where == "conv":
        hc = hv.conv_case(name)
        d = hv.conv_data(hc)
        want, got = hv.conv_restate(hc["c"], d), hv.conv_restate(hc["c"], d, m)
        bad, _ = hv.same_bits_or_nan(got, want)
        return float(bad.mean())
    hc = STAGE[name]
    d = hv.stage_data(hc)
    want, got = hv.stage_restate(hc["c"], d), hv.stage_restate(hc["c"], d, m)
    worst = 0.0
    for k in want:
        if hc["c"]["kind"] in hv.COPIES:
            bad = np.ascontiguousarray(got[k]).view(np.uint32) != np.ascontiguousarray(want[k]).view(np.uint32)
        elif want[k].dtype == F32:
            bad, _ = hv.same_bits_or_nan(got[k], want[k])
        else:
            bad = got[k] != want[k]
        worst = max(worst, float(bad.mean()))
    return worst


def test_no_mutant_survives():
    survivors = []
    for mutant in hv.MUTANTS:
        frac = _mutant_differs(mutant)
        print(f"{mutant} on {hv.MUTANTS[mutant][1]}: changes {100 * frac:.4f} % of the outputs")
        if frac == 0.0:
            survivors.append(mutant)
    assert survivors == []
    assert _mutant_differs("flush_in") >= 0.99 and _mutant_differs("flush_out") >= 0.99


@pytest.mark.parametrize("name", ["direct_NONE", "direct_GELU", "rowperm_RES", "deconv_none", "segs3", "group2_small"])
def test_flush_and_order_mutants_are_silent_on_ordinary_operands(name):
    """the evidence of the gap: on conv_contract.make_data's operands flushing changes no bit, and the ascending k order stays inside the
    float64 bound -- the host side of the existing matrix cannot tell either from the contract"""
    c = {x["name"]: x for x in cc.matrix()}[name]
    d = cc.make_data(c)
    for g in range(c["ngroup"]):
        want = cc.restate(c, d, group=g)
        for m in ("flush_in", "flush_out"):
            assert np.array_equal(hv.conv_restate(c, d, m, group=g).view(np.uint32), want.view(np.uint32)), m
        asc = hv.conv_restate(c, d, "ascending_k", group=g)
        assert not np.array_equal(asc.view(np.uint32), want.view(np.uint32))
        ok, ratio, nbad = cc.within(c, asc, d, group=g)
        assert ok, (ratio, nbad)


# ---------------------------------------------------------------------------------------------------------------- the arbiter
# where the restated epilogue function and ATen's CPU float32 op fall into different classes (NaN / +inf / -inf / finite): the record of
# DESIGN.md section 2.  Everything else agrees in class, and in value to the distances DESIGN.md section 2 already pins (erf, tanh, exp
# 1 ulp, sigmoid 2 ulp, GELU 1.2e-6 absolute; below FLT_MIN the sigmoid's exp underflows to an exact 0 in pc_math.h).
ATEN_CLASS_DIFFERENCES = {
    "RELU": "nan",            # v > 0 ? v : 0 gives +0; torch.relu passes NaN on
    "GELU": "top",            # +inf and FLT_MAX give themselves; ATen's vector GELU gives NaN at +inf and inf at FLT_MAX
    "RES_GELU": "top",
}
ATEN_TOLERANCE = {"GELU": (2, 1.2e-6), "RES_GELU": (2, 1.2e-6), "GATE": (2, 2.0 ** -126), "LRP": (2, 0.0), "LRP_ADD": (2, 0.0), "IGDN": (1, 0.0)}


def test_epilogues_against_the_aten_ops_at_special_values():
    """the epilogue functions of the restatement against the ATen CPU ops the reference calls, at +-inf, NaN, +-FLT_MAX, the exp range
    limits, zeros, negatives and pc_math.h's branch points: the same class everywhere but at the recorded differences"""
    import torch
    import torch.nn.functional as F
    v = np.concatenate([hv.bias_values(16), hv.branch_values(), np.array([0.0, -0.0, -2.0], F32)])
    t = torch.from_numpy(v.copy())
    leaky = lambda a: F.leaky_relu(a, 0.01)
    half_tanh = lambda a: 0.5 * torch.tanh(a)
    ident = lambda a: a
    aten = dict(NONE=ident, GELU=F.gelu, RES_GELU=F.gelu, RES=ident, GATE=torch.sigmoid, GDN=torch.rsqrt, IGDN=torch.sqrt,
                CLAMP01=lambda a: a.clamp(0, 1), LRP=half_tanh, LRP_ADD=half_tanh, LEAKY=leaky, LEAKY_RES=leaky, RELU=torch.relu, SE_ADD=ident)
    klass = lambda a: np.where(np.isnan(a), 0, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 3)))
    top = ~(np.abs(v) < np.finfo(F32).max) & (v > 0)                       # +inf and +FLT_MAX
    for epi in cc.EPI:
        a0, a1 = hv.sweep_aux(epi, (1, 1, v.size, 1))
        if epi == "SE_ADD":
            a1 = np.ones((1, 1, v.size, 1), F32)
        with np.errstate(all="ignore"):
            got = cc._epilogue32(epi, v.reshape(1, 1, -1, 1), a0, a1).reshape(-1)
        ref = aten[epi](t).numpy()
        differs = klass(got) != klass(ref)
        allowed = dict(nan=np.isnan(v), top=top).get(ATEN_CLASS_DIFFERENCES.get(epi), np.zeros(v.size, bool))
        assert not (differs & ~allowed).any(), (epi, v[differs & ~allowed])
        if epi in ATEN_CLASS_DIFFERENCES:
            assert (differs & allowed).any(), epi                         # the record stays true
        both = np.isfinite(got) & np.isfinite(ref)
        ulps, absolute = ATEN_TOLERANCE.get(epi, (0, 0.0))
        err = np.abs(got[both].astype(np.float64) - ref[both].astype(np.float64))
        with np.errstate(over="ignore"):
            ulp = np.minimum(np.spacing(np.abs(ref[both])).astype(np.float64), 2.0 ** 104)      # spacing(FLT_MAX) overflows float32
        assert (err <= ulps * ulp + absolute).all(), (epi, float(err.max()))

"""Values outside the ordinary through the conv, attention and stage kernels (tests/hostile_values.py is the table): subnormal operands
and products, NaN / inf / near-FLT_MAX activations, chains whose k order decides between a number and an infinity, every epilogue over
all 2^24 arguments of a sweep and at pc_math.h's branch points, the quantisers at and beyond the int32 range, NaN payloads through the
NCHW copy.  Every case is launched once through pc_test_conv / pc_test_stage with the helpers of the two launcher matrices and checked
as they check:

  (a) output bits equal the restatement's -- the one allowance: where both are NaN only NaN-ness is compared (payload differences are
      counted and printed per case; copies compare all 32 bits);
  (b) the float64 bound (conv_contract.within_normal) on the outputs whose float64 value is finite and of normal range, in the classes
      where the bound means something (not the subnormal classes: its absolute slack is vacuous there; not `overflow`: a float32 chain
      overflows where float64 does not; less hostile_values.bound_exclusions: the sub-pixel layer's zero taps, squares that overflow);
      the sweep carries it in every form (GDN on v >= 1, where its bound is derived); the stage cases carry
      stage_contract.check64_normal except the classes of STAGE_NO_BOUND, each with its reason there;
  (c) sentinels, guard bands and input gaps hold;
  (d) `plan` is the instantiation / variant the base case was written for;
  grouped cases: both groups, and each group against its own separate launch.

One codec-level case closes the file: an image of finite values in [-2, 3] codes to the oracle's strings, masks and x_hat bits.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import conv_contract as cc
from tests import hostile_values as hv
from tests import stage_contract as sc
from tests import test_gpu_conv_matrix as cm
from tests import test_gpu_stage_matrix as sm
from tests.util import gpu_codec, oracle_codec

pytestmark = pytest.mark.gpu

F32 = np.float32
CONV = {hc["name"]: hc for hc in hv.conv_cases()}
STAGE = {hc["name"]: hc for hc in hv.stage_cases()}
PAYLOADS = {}                      # case: NaN pairs whose payloads differ
REACHED = set()
BOUND_CLASSES = ("sprinkle", "sprinkle_nan", "cancel")
# stage classes without the float64 check: the subnormal ones (the bound's absolute slack is vacuous there); `underflow`, whose v * 2^120
# makes the contract's exact zero below -87 differ from the true softmax by up to 0.02 (measured on the restatement: 11 - 94 x the bound);
# `x_2p64`, where x^2 overflows in float32 and not in float64
STAGE_NO_BOUND = ("sub_v", "x_2m128", "sub_x", "underflow", "x_2p64")


def _run_conv(c, d, want_of, name, bound, exclude=None):
    """launch the case once; checks (a) - (d) on every output; returns the count of NaN payload differences.  `exclude`: outputs the
    float64 bound leaves out besides hostile_values.bound_exclusions"""
    desc, keep, out, relu, g1 = cm.build(c, d)
    rc, plan = cm.launch(desc)
    assert rc == 0, f"{name}: pc_test_conv returned {rc}"
    torch.cuda.synchronize()
    assert plan == tuple(c["expect"]), f"{name}: launcher chose {plan}, the case is meant for {tuple(c['expect'])}"
    REACHED.add(plan)
    cn = dict(c, name=name)
    want = want_of(0)
    pay = cm.check_out_nan(cn, d, out, want, "out")
    if bound:
        with np.errstate(all="ignore"):
            ok, ratio, nbad, judged = cc.within_normal(c, cm.values(out), d, exclude=hv.bound_exclusions(c, d) if exclude is None else exclude)
        assert judged > 0
        print(f"{name}: float64 bound on {judged} of {want.size} outputs, worst ratio {ratio:.3g}")
        assert ok, f"{name}: {nbad} outputs outside the float64 bound (worst ratio {ratio:.3g})"
    if relu is not None:
        with np.errstate(invalid="ignore"):
            pay += cm.check_out_nan(cn, d, relu, np.where(want > 0, want, F32(0)).astype(F32), "out_relu")
    if g1 is not None:
        pay += cm.check_out_nan(cn, d, g1, want_of(1), "group 1")
        if bound:
            with np.errstate(all="ignore"):
                ok, ratio, nbad, judged = cc.within_normal(c, cm.values(g1), d, group=1, exclude=hv.bound_exclusions(c, d, 1))
            assert ok, f"{name} group 1: {nbad} outputs outside the float64 bound (worst ratio {ratio:.3g})"
        for grp, o in ((0, out), (1, g1)):                                   # the two groups as separate launches: the same outputs
            desc1, keep1, out1, _, _ = cm.build(dict(c, ngroup=1), d, group=grp)
            rc1, _ = cm.launch(desc1)
            assert rc1 == 0
            torch.cuda.synchronize()
            bad, p1 = hv.same_bits_or_nan(out1.host(), o.host())
            assert not bad.any(), f"{name}: group {grp} differs from its separate launch in {int(bad.sum())} words"
            pay += p1
    del keep
    PAYLOADS[name] = pay
    print(f"{name}: plan {plan}, {pay} NaN payload differences")
    return pay


@pytest.mark.parametrize("name", list(CONV))
def test_conv_value_class(name):
    hc = CONV[name]
    c = hc["c"]
    d = hv.conv_data(hc)
    _run_conv(c, d, lambda g: hv.conv_restate(c, d, group=g), name, hc["klass"] in BOUND_CLASSES)


# ---------------------------------------------------------------------------------------------------------------- the epilogue sweep
@pytest.mark.parametrize("form", list(hv.SMALL_FORMS))
@pytest.mark.parametrize("epi", list(cc.EPI))
def test_epilogue_sweep(epi, form):
    """all 2^24 arguments 256 i + o of the epilogue through the identity layer: 16 channels x 2^20 pixels (layout-0 kernel, direct or
    generic form) or 64 channels x 2^18 pixels (unified kernel, fast and slow form)"""
    c, d = hv.sweep_case(epi, form, hv.sweep_values(epi))
    # the float64 bound on every argument whose float64 result is finite and of normal range; GDN's bound is derived for pre-activations
    # >= 1 (conv_contract.POSITIVE_PRE: its slope term is capped there), so GDN is judged on v >= 1 -- 2^22 of the arguments
    with np.errstate(invalid="ignore"):
        exclude = ~(d["x"] >= 1) if epi == "GDN" else None
    _run_conv(c, d, lambda g: hv.sweep_restate(c, d), c["name"], True, exclude)


@pytest.mark.parametrize("form", list(hv.SMALL_FORMS))
def test_epilogue_branch_points_and_nonfinite_preactivations(form):
    """every epilogue at pc_math.h's branch points +-4 ulp, FLT_MAX, the subnormal boundary and zeros, and -- through the bias -- at
    +-inf, NaN, +-FLT_MAX and the exp range limits"""
    Cc = hv.SMALL_FORMS[form][0]
    for epi in cc.EPI:
        for what, values, bias in (("branch", hv.branch_values(), None), ("bias", np.zeros(4 * Cc, F32), hv.bias_values(Cc))):
            c, d = hv.sweep_case(epi, form, values, bias)
            # the bound on the finite list; GDN / IGDN's is derived for pre-activations >= 1 (conv_contract.POSITIVE_PRE) only
            _run_conv(c, d, lambda g: hv.sweep_restate(c, d), f"{c['name']}_{what}", what == "branch" and epi not in cc.POSITIVE_PRE)


# ---------------------------------------------------------------------------------------------------------------- stages
@pytest.mark.parametrize("name", list(STAGE))
def test_stage_value_class(name):
    hc = STAGE[name]
    c = hc["c"]
    d = hv.stage_data(hc)
    want = hv.stage_restate(c, d)
    desc, bufs = sm.build(c, d)
    plan = (C.c_int * 1)(0)
    rc = sm._lib().pc_test_stage(C.byref(desc), plan, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert plan[0] == sc.SPLAN[c["expect"]], f"{name}: plan {plan[0]}, written for {c['expect']} ({sc.SPLAN[c['expect']]})"
    pay = 0
    for field, (sp, t, buf, index) in bufs.items():
        host = sm.read(t)
        if not sp["out"]:
            assert np.array_equal(host, buf), f"{name}: input {field} was written"
            continue
        assert (c["kind"], field) not in sc.SCRATCH and (c["kind"], field) not in sc.BOUND_ONLY
        exp = buf.copy()
        exp[index] = sc.as_words(want[field])
        differ = host != exp
        if sp["dtype"] == np.dtype(F32) and c["kind"] not in hv.COPIES:       # computed floats: NaN-ness where both are NaN
            inside = np.zeros(buf.shape, bool)
            inside[index] = True
            both = inside & np.isnan(host.view(F32)) & np.isnan(exp.view(F32)) & (host != np.uint32(sc.SENT32))
            pay += int((differ & both).sum())
            differ &= ~both
        bad = np.flatnonzero(differ)
        nin = int(np.isin(bad, index.reshape(-1)).sum()) if bad.size else 0
        assert bad.size == 0, f"{name}: {field}: {bad.size} words differ ({nin} inside the tensor, {bad.size - nin} sentinels), first at " \
                              f"{bad[:4]}: got {host[bad[:4]]}, restatement {exp[bad[:4]]}"
    if hc["klass"] not in STAGE_NO_BOUND:
        got = {f: sm.read(t)[index].view(sp["dtype"]) if sp["dtype"].itemsize == 4 else sm.read(t)[index]
               for f, (sp, t, buf, index) in bufs.items() if sp["out"]}
        exclude = None
        if c["kind"] == "GDN":                  # sprinkle: a pixel that holds |x| >= 2^63 has a norm that overflows in float32 only
            with np.errstate(invalid="ignore"):
                huge = ~(np.abs(d["x"]) < 2.0 ** 63).reshape(c["P"], c["C"])
            exclude = dict(out=np.broadcast_to(huge.any(axis=1, keepdims=True), huge.shape))
        ok, res, ratio, judged = sc.check64_normal(c, d, got, exclude)
        print(f"{name}: float64 check {res} worst ratio {ratio:.3g}, judged {judged}")
        assert ok, f"{name}: {res}"
        assert all(n > 0 for _, n, _ in judged)
    PAYLOADS[name] = pay
    print(f"{name}: plan {plan[0]}, {pay} NaN payload differences")


def test_conversion_rule_on_the_device():
    """(int32_t)pc_roundevenf(v) as the shipped encoder and decoder share it: saturating, NaN -> 0 -- read directly
    from the EntropyBottleneck quantiser, without the restatement in between"""
    hc = STAGE["quant:eb_quant_c192_hw4"]
    c = hc["c"]
    d = hv.stage_data(hc)
    desc, bufs = sm.build(c, d)
    assert sm._lib().pc_test_stage(C.byref(desc), None, None) == 0
    torch.cuda.synchronize()
    sp, t, buf, index = bufs["sym"]
    sym = sm.read(t)[index].view(np.int32).reshape(c["B"], c["C"], c["HW"]).transpose(0, 2, 1)
    with np.errstate(invalid="ignore"):
        v = (d["z"] - d["med"]).astype(F32)
        r = np.rint(v.astype(np.float64))
    assert np.array_equal(sym[np.isnan(v)], np.zeros(int(np.isnan(v).sum()), np.int32)) and np.isnan(v).sum() == 3
    assert (sym[r >= 2.0 ** 31] == 2 ** 31 - 1).all() and (r >= 2.0 ** 31).sum() >= 5
    assert (sym[r <= -2.0 ** 31] == -2 ** 31).all() and (r <= -2.0 ** 31).sum() >= 5
    ordinary = np.abs(r) < 2.0 ** 31
    assert np.array_equal(sym[ordinary], r[ordinary].astype(np.int64).astype(np.int32))


def test_table_reaches_every_production_pair():
    """every case asserts the plan it was written for, so the coverage is a property of the table (no state of other tests needed)"""
    for klass in ("sub_in", "sprinkle"):
        assert {tuple(hc["c"]["expect"]) for hc in CONV.values() if hc["klass"] == klass} >= cc.REQUIRED


def test_counts():
    """the printed record of DESIGN.md section 2 (asserts nothing): launches checked so far in this process and their NaN payload
    differences"""
    total = sum(PAYLOADS.values())
    worst = sorted(PAYLOADS.items(), key=lambda kv: -kv[1])[:8]
    whole = len(CONV) + len(STAGE) + 3 * len(cc.EPI) + 6 * len(cc.EPI)
    print(f"{len(PAYLOADS)} of {whole} launches ran in this process{'' if len(PAYLOADS) == whole else ' (INCOMPLETE record)'}, "
          f"{total} NaN payload differences; most: {worst}")
    print(f"conv (instantiation, form) pairs reached: {sorted(REACHED)}")


# ---------------------------------------------------------------------------------------------------------------- codec level
@pytest.mark.parametrize("quality", [0.0, 0.5])
def test_codec_on_out_of_range_pixels(quality):
    """a 1 x 3 x 64 x 64 image of finite values in [-2, 3] (compress() takes what it is given; non-finite pixels are out of scope): the GPU
    strings, masks and x_hat bits are the oracle's"""
    g = torch.Generator().manual_seed(2024)
    x = torch.rand(1, 3, 64, 64, generator=g) * 5.0 - 2.0
    assert torch.isfinite(x).all() and x.min() < -1.9 and x.max() > 2.9
    net = gpu_codec()
    out = net.compress(x.cuda(), quality, "point-based-std")
    x_hat = net.decompress(out["strings"], out["shape"], quality, "point-based-std")["x_hat"].cpu()
    orc = oracle_codec("cdet")
    ref = orc.compress(x, quality)
    assert tuple(out["shape"]) == tuple(ref["shape"])
    assert out["strings"][1] == ref["strings"][1], "z strings differ"
    assert len(out["strings"][0]) == len(ref["strings"][0])
    for s, (a, b) in enumerate(zip(out["strings"][0], ref["strings"][0])):
        assert a == b, f"y strings of slice {s} differ"
    assert len(out["masks"]) == len(ref["masks"])
    for m, rm in zip(out["masks"], ref["masks"]):
        assert np.array_equal(m.cpu().numpy(), rm.numpy())
    r_x_hat = orc.decompress(ref["strings"], ref["shape"], quality)["x_hat"]
    assert np.array_equal(x_hat.numpy().view(np.uint32), r_x_hat.numpy().view(np.uint32)), \
        f"x_hat max abs diff {(x_hat - r_x_hat).abs().max().item()}"

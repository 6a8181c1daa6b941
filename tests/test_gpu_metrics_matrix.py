"""The metrics kernels, path by path (progressivecodec_amd/metrics_csrc/pc_metrics.hip): every case of tests/metrics_contract.py launched
once through pc_msssim with a workspace the test provides, and checked four ways:

  (a) every (ssim, cs) pair of the per-tile slab, every pooled plane and every entry of out_scales is bit-equal to the restatement
      (a NaN for a NaN); out[b] is within one float32 ulp of the float32 rounding of the restated f64 value;
  (b) every per-scale mean and the value lie within the derived float64 bound of the definition, no exclusions;
  (c) sentinels hold: the padding between the workspace's regions, a guard band on both sides of the workspace, of out and of out_scales;
      the inputs are views inside buffers whose gaps hold a NaN, so a read outside a plane that reaches an unmasked output poisons it;
  (d) pc_msssim_plan names, per scale, the staging path the case was written to reach.

It closes with the coverage assertion over metrics_contract.REQUIRED; the refusals must come back from the host with every buffer
untouched.  Worst |got - ref| / bound per group is printed (a record, not a threshold).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import metrics_contract as mc

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in mc.matrix()}
REACHED = set()
WORST = {}
OUTS = {}


def _lib():
    from progressivecodec_amd import metrics
    return metrics.lib()


def _guarded(nbytes):
    """(device uint8 tensor of GUARD + nbytes + GUARD sentinel bytes, pointer to the middle)"""
    words = np.full((2 * mc.GUARD + nbytes + 3) // 4, mc.SENT32, np.uint32)
    t = torch.from_numpy(words.view(np.int32)).cuda()
    assert t.data_ptr() % 256 == 0
    return t, t.data_ptr() + mc.GUARD


def _bytes(t):
    return t.cpu().numpy().view(np.uint8)


def _guards_hold(name, what, host, nbytes):
    sent = np.full(mc.GUARD // 4, mc.SENT32, np.uint32).view(np.uint8)
    assert np.array_equal(host[:mc.GUARD], sent), f"{name}: the guard band before {what} was written"
    tail = host[mc.GUARD + nbytes:]
    assert np.array_equal(tail, np.full(tail.size // 4 + 1, mc.SENT32, np.uint32).view(np.uint8)[(nbytes % 4):][:tail.size]), \
        f"{name}: the guard band after {what} was written"


def launch(c, d, over=None):
    """one call of pc_msssim_plan and pc_msssim; returns rc and everything read back"""
    L = _lib()
    lay = mc.ws_layout(c)
    bufs = {}
    args = {}
    for k, nm in (("X", "xl"), ("Y", "yl")):
        buf, off, index = mc.place(d[k], c[nm])
        t = torch.from_numpy(buf.view(np.int32)).cuda()
        assert t.data_ptr() % 256 == 0
        bufs[k] = (t, buf)
        args[k] = t.data_ptr() + 4 * off
    B, Cc, levels = c["B"], c["C"], c["levels"]
    n_out, n_sc = 4 * B, 8 * levels * 2 * B * Cc
    ws_t, ws_p = _guarded(lay["total"])
    out_t, out_p = _guarded(n_out)
    sc_t, sc_p = _guarded(n_sc)
    w = (C.c_float * levels)(*c["weights"]) if c["weights"] else None
    xl, yl = c["xl"], c["yl"]
    a = dict(X=args["X"], sxb=xl["sb"], sxc=xl["sc"], sxh=xl["sh"], Y=args["Y"], syb=yl["sb"], syc=yl["sc"], syh=yl["sh"], B=B, C=Cc,
             H=c["H"], W=c["W"], L=c["L"], ws=c["ws"], sigma=c["sigma"], K1=c["K"][0], K2=c["K"][1], levels=levels, weights=w,
             nonneg=int(c["nonneg"]), work=ws_p, nbytes=lay["total"], out=out_p, scales=sc_p)
    a.update(over or {})
    vec = (C.c_int * 5)(7, 7, 7, 7, 7)
    prc = L.pc_msssim_plan(a["X"], a["sxb"], a["sxc"], a["sxh"], a["Y"], a["syb"], a["syc"], a["syh"], a["B"], a["C"], a["H"], a["W"],
                           a["ws"], a["levels"], a["work"], vec)
    rc = L.pc_msssim(a["X"], a["sxb"], a["sxc"], a["sxh"], a["Y"], a["syb"], a["syc"], a["syh"], a["B"], a["C"], a["H"], a["W"], a["L"],
                     a["ws"], a["sigma"], a["K1"], a["K2"], a["levels"], a["weights"], a["nonneg"], a["work"], a["nbytes"], a["out"],
                     a["scales"], None)
    torch.cuda.synchronize()
    return dict(rc=rc, prc=prc, vec=tuple(vec)[:levels], ws=_bytes(ws_t), out=_bytes(out_t), scales=_bytes(sc_t), lay=lay, n_out=n_out,
                n_sc=n_sc, inputs={k: (_bytes(t), buf.view(np.uint8)) for k, (t, buf) in bufs.items()})


def _untouched(name, g):
    for what, host, n in (("the workspace", g["ws"], 0), ("out", g["out"], 0), ("out_scales", g["scales"], 0)):
        assert np.array_equal(host, np.full(host.size // 4, mc.SENT32, np.uint32).view(np.uint8)), f"{name}: {what} was written"
    for k, (host, buf) in g["inputs"].items():
        assert np.array_equal(host, buf), f"{name}: input {k} was written"


@pytest.mark.parametrize("name", list(CASES))
def test_metrics_case(name):
    c = CASES[name]
    d = mc.make_data(c)
    want = mc.restate(c, d)
    g = launch(c, d)
    assert g["rc"] == 0 and g["prc"] == 0, (g["rc"], g["prc"])
    lay, G = g["lay"], mc.GUARD
    for k, (host, buf) in g["inputs"].items():
        assert np.array_equal(host, buf), f"{name}: input {k} was written"
    # (a) bits of the slab and the pooled planes, (c) the padding between them
    bad = mc.compare_workspace(c, g["ws"][G:G + lay["total"]], want)
    assert not bad, f"{name}: " + "; ".join(bad)
    means = g["scales"][G:G + g["n_sc"]].view(np.float64).reshape(want["means"].shape)
    ok = mc.same_bits(means, want["means"], np.float64).reshape(means.shape)
    assert ok.all(), f"{name}: out_scales differs from the restatement at [scale, ssim/cs, image, channel] {np.argwhere(~ok)[:4].tolist()}"
    out = g["out"][G:G + g["n_out"]].view(np.float32)
    # device pow in f64 is not correctly rounded: the runtime documents it to 1 ulp, the host's is within 1 ulp too, so each of the at
    # most 5 factors differs by 2^-51 relative; the product's 4 and the channel sum's roundings are the same operations on both sides and
    # every term is non-negative (relu), so nothing cancels: the two f64 values differ by at most about 10 * 2^-52 relative, 2^-25 of a
    # float32 ulp.  Two reals that close round to the same float32 or, across a rounding boundary, to neighbours: one float32 ulp.
    # levels == 1 has no pow: the value is the same f64 operations, so the same bits.
    w32 = want["out"].astype(np.float32)
    with np.errstate(invalid="ignore"):
        near = (out == w32) | (np.isnan(out) & np.isnan(w32)) | (np.abs(out.astype(np.float64) - w32.astype(np.float64)) <= np.spacing(np.abs(w32)))
    assert near.all(), f"{name}: out {out} restated {w32}"
    if c["levels"] == 1:
        assert mc.same_bits(out, w32, np.float32).all(), f"{name}: out {out} restated {w32}"
    # (c) guard bands
    _guards_hold(name, "the workspace", g["ws"], lay["total"])
    _guards_hold(name, "out", g["out"], g["n_out"])
    _guards_hold(name, "out_scales", g["scales"], g["n_sc"])
    # (b) the float64 bound of the definition
    ok64, ratio, unbounded, txt = mc.check64(mc.reference64(c, d), means, out.astype(np.float64))
    print(f"{name}: plan {g['vec']} float64 check {txt}, worst ratio {ratio:.3g}, {unbounded} values not bounded")
    assert ok64, f"{name}: {txt}"
    grp = WORST.get(c["group"], (0, 0.0))
    WORST[c["group"]] = (grp[0] + 1, max(grp[1], ratio))
    # (d) the staging path per scale
    assert g["vec"] == c["vec"], f"{name}: plan {g['vec']}, written for {c['vec']}"
    OUTS[name] = (g["ws"][G:G + lay["total"]].copy(), means.copy(), out.copy())
    if c["twin"]:                                               # one precondition broken alone: the other path, the same bits
        assert c["twin"] in OUTS, "the aligned twin runs first"
        tw = OUTS[c["twin"]]
        assert CASES[c["twin"]]["vec"][0] == 1 and g["vec"][0] == 0
        assert np.array_equal(tw[0], OUTS[name][0]) and np.array_equal(tw[1], means) and np.array_equal(tw[2], out)
    REACHED.update(mc.reached(c))


def _refusals():
    inf, nan = float("inf"), float("nan")
    r = [(f"{k}_{v}", "vec_twin", {k: v}, mc.PC_ERR_ARG) for k in ("sxb", "sxc", "sxh", "syb", "syc", "syh") for v in (0, -4)]
    r += [(f"{k}_{v}", "vec_twin", {k: v}, mc.PC_ERR_ARG) for k in ("L", "K1", "K2", "sigma") for v in (inf, nan)]
    r += [("sigma_0", "vec_twin", dict(sigma=0.0), mc.PC_ERR_ARG), ("sigma_negative", "vec_twin", dict(sigma=-1.5), mc.PC_ERR_ARG)]
    r += [(f"weight_{v}", "vec_twin", dict(weights=(C.c_float * 2)(0.4, v)), mc.PC_ERR_ARG) for v in (inf, nan)]
    r += [(f"null_{k}", "vec_twin", {k: None}, mc.PC_ERR_ARG) for k in ("X", "Y", "out", "work", "weights")]
    r += [("workspace_one_byte_short", "vec_twin", dict(nbytes=mc.ws_layout(CASES["vec_twin"])["total"] - 1), mc.PC_ERR_BUFFER),
          ("workspace_zero", "vec_twin", dict(nbytes=0), mc.PC_ERR_BUFFER)]
    # the size rule: levels >= 2 needs min(H, W) > 16 (ws - 1) (ms_w3_l2_rule_edge runs at 33 x 35), levels == 1 needs H, W >= ws
    r += [("rule_h_32", "ms_w3_l2_rule_edge", dict(H=32), mc.PC_ERR_ARG), ("rule_w_32", "ms_w3_l2_rule_edge", dict(W=32), mc.PC_ERR_ARG),
          ("ssim_h_below_ws", "ssim_w7_one_pixel", dict(H=6), mc.PC_ERR_ARG), ("ssim_w_below_ws", "ssim_w7_one_pixel", dict(W=6), mc.PC_ERR_ARG),
          ("win_even", "vec_twin", dict(ws=4), mc.PC_ERR_ARG), ("win_33", "vec_twin", dict(ws=33), mc.PC_ERR_ARG),
          ("levels_0", "vec_twin", dict(levels=0), mc.PC_ERR_ARG), ("levels_6", "vec_twin", dict(levels=6), mc.PC_ERR_ARG)]
    return r


@pytest.mark.parametrize("name,base,over,code", _refusals(), ids=[r[0] for r in _refusals()])
def test_metrics_refusal(name, base, over, code):
    c = CASES[base]
    g = launch(c, mc.make_data(c), over)
    assert g["rc"] == code, g["rc"]
    _untouched(name, g)
    if any(k in over for k in ("sxb", "sxc", "sxh", "syb", "syc", "syh", "X", "Y", "work", "H", "W", "ws", "levels")):
        assert g["prc"] == mc.PC_ERR_ARG and g["vec"] == (7,) * len(g["vec"])           # the plan refuses what it takes, and writes nothing


def test_metrics_matrix_coverage():
    for grp, (n, ratio) in sorted(WORST.items()):
        print(f"{grp}: {n} cases, worst |got - ref| / bound = {ratio:.3g}")
    missing = mc.REQUIRED - REACHED
    assert not missing, f"paths no case reached: {sorted(missing)}"
    assert sum(n for n, _ in WORST.values()) == len(CASES)

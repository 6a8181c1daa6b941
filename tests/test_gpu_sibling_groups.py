"""Sibling convolutions in one launch (pc_codec.hip: hyper(), wam()).

Launcher level, through pc_test_conv / pc_test_conv_g1aux and the helpers of tests/conv_contract.py: the grouped launch in the forms the
codec newly uses -- with the PixelShuffle epilogue (h_s layers 2 and 4), as a 1x1 layer with N and K tails (ResidualUnit), with
PC_EPI_RES_GELU and one residual tensor per group (the unit's tail) -- and the layer of n * 192 outputs against n layers of 192.  Both
groups' outputs equal the restatement bit for bit, lie within the float64 bound, and leave every sentinel word alone.

Codec level: the same seeded model with the option "group_siblings" 0 and 1 gives the same strings, x_hat and latent_means /
latent_scales, reports the same FLOPs to the launch ledger and exactly the expected number of launches fewer.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from tests import conv_contract as cc
from tests import test_gpu_conv_matrix as cm
from tests.util import gpu_codec, inputs

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- launcher level
def _run_grouped(c, d, aux0_g1=None):
    """launch the grouped case; returns (plan, out of group 0, out of group 1)"""
    desc, keep, out, relu, g1 = cm.build(c, d)
    assert g1 is not None
    plan = (C.c_int * 2)()
    if aux0_g1 is None:
        rc = cm._lib().pc_test_conv(C.byref(desc), plan, None)
    else:
        _, _, oh, ow, oc = cc.out_grid(c)
        t = cm.strided(aux0_g1.reshape(-1, oc), desc.ld0, 0)          # the pixel stride of the descriptor's aux0, gaps poisoned
        keep.append(t)
        rc = cm._lib().pc_test_conv_g1aux(C.byref(desc), C.c_void_p(cm.addr(t)), plan, None)
    assert rc == 0, f"{c['name']}: launcher returned {rc}"
    torch.cuda.synchronize()
    return (cc.PLAN_NAME.get(plan[0], plan[0]), cc.FORM_NAME.get(plan[1], plan[1])), out, g1, keep


def _check_both(c, d, out, g1, d1=None):
    d1 = d if d1 is None else d1
    for grp, o, dd in ((0, out, d), (1, g1, d1)):
        cm.check_out(c, dd, o, cc.restate(c, dd, group=grp), f"group {grp}")
        ok, ratio, nbad = cc.within(c, cm.values(o), dd, group=grp)
        assert ok, f"{c['name']} group {grp}: {nbad} outputs outside the float64 bound (worst ratio {ratio:.3g})"


PS_CASES = [cc.case(f"g2_ps_gelu_cin{cin}_{B}x{H}x{W}", B, H, W, segs=[(cin, cin, 0)], k=3, Cout=64, epi="GELU", ps=True, ngroup=2)
            for cin in (32, 48) for (B, H, W) in ((1, 1, 1), (1, 2, 3), (1, 9, 7), (2, 9, 7))]


@pytest.mark.parametrize("c", PS_CASES, ids=[c["name"] for c in PS_CASES])
def test_grouped_pixel_shuffle_gelu(c):
    """h_s layers 2 and 4 as scale || mean: the N = 4 * Cout sub-pixel form of one phase, stored through the PixelShuffle epilogue"""
    d = cc.make_data(c)
    plan, out, g1, keep = _run_grouped(c, d)
    assert plan == ("UNI_32_3", "TABLE"), plan
    _check_both(c, d, out, g1)


ONE_CASES = [cc.case(f"g2_1x1_gelu_m{B * H * W}", B, H, W, segs=[(160, 160, 0)], k=1, Cout=160, epi="GELU", ngroup=2)
             for (B, H, W) in ((1, 4, 4), (5, 8, 8))]


@pytest.mark.parametrize("c", ONE_CASES, ids=[c["name"] for c in ONE_CASES])
def test_grouped_1x1(c):
    """N and K tails (160 = 2 * 64 + 32 = 5 * 32); M = 16: one M tile, fewer than the XCD halves; M = 320: five M tiles, no multiple of 4"""
    d = cc.make_data(c)
    plan, out, g1, keep = _run_grouped(c, d)
    assert plan == ("UNI_32_2", "DIRECT"), plan
    _check_both(c, d, out, g1)


RES_CASES = [cc.case(f"g2_res_gelu_m{B * H * W}", B, H, W, segs=[(80, 80, 0)], k=1, Cout=160, epi="RES_GELU", ngroup=2)
             for (B, H, W) in ((1, 4, 4), (2, 5, 7))]


@pytest.mark.parametrize("c", RES_CASES, ids=[c["name"] for c in RES_CASES])
def test_grouped_res_gelu_two_residuals(c):
    """the ResidualUnit tail a[k] || b[k]: each group adds its own identity tensor (pc_conv_params::g1_aux0)"""
    d = cc.make_data(c)
    rng = np.random.default_rng(c["seed"] + 1)
    d1 = dict(d, aux0=rng.standard_normal(d["aux0"].shape).astype(np.float32))
    plan, out, g1, keep = _run_grouped(c, d, aux0_g1=d1["aux0"])
    assert plan == ("UNI_32_2", "DIRECT"), plan
    _check_both(c, d, out, g1, d1)
    # and with no tensor of its own, group 1 reads the launch's aux0
    plan, out, g1, keep = _run_grouped(c, d)
    _check_both(c, d, out, g1)


@pytest.mark.parametrize("bhw", [(1, 1, 1), (1, 2, 3), (1, 7, 10)], ids=["m1", "m6", "m70"])
def test_n_concatenation(bhw):
    """h_s layer 1 of four nets: one launch of Cout = 4 * 192 against four launches of Cout = 192 on the same input"""
    B, H, W = bhw
    cw = cc.case(f"cat4_m{B * H * W}", B, H, W, segs=[(192, 192, 0)], k=3, Cout=4 * 192, epi="GELU")
    dw = cc.make_data(cw)
    desc, keep, out, _, _ = cm.build(cw, dw)
    rc, _ = cm.launch(desc)
    assert rc == 0
    torch.cuda.synchronize()
    cm.check_out(cw, dw, out, cc.restate(cw, dw), "wide")
    ok, ratio, nbad = cc.within(cw, cm.values(out), dw)
    assert ok, f"{cw['name']}: {nbad} outputs outside the float64 bound (worst ratio {ratio:.3g})"
    wide = cm.values(out)
    for j in range(4):
        cj = dict(cw, Cout=192, name=f"{cw['name']}_net{j}")
        dj = dict(x=dw["x"], w=dw["w"][192 * j:192 * (j + 1)], b=dw["b"][192 * j:192 * (j + 1)])
        descj, keepj, outj, _, _ = cm.build(cj, dj)
        rcj, _ = cm.launch(descj)
        assert rcj == 0
        torch.cuda.synchronize()
        assert (outj.host()[:cm.GUARD] == cm.SENT).all() and (outj.host()[-cm.GUARD:] == cm.SENT).all()
        a, b = np.ascontiguousarray(wide[..., 192 * j:192 * (j + 1)]), np.ascontiguousarray(cm.values(outj))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"net {j}: the slice of the wide launch differs from its own launch"


# ---------------------------------------------------------------------------------------------------------------- codec level
POL = "point-based-std"


@functools.lru_cache(maxsize=None)
def _variant_net(kw):
    from progressivecodec_amd import ChannelProgresssiveWACNN
    from progressivecodec_amd.arch import CodecConfig
    from progressivecodec_amd.synth import synthetic_state_dict
    from tests.util import tables_npz
    kw = dict(kw)
    sd = synthetic_state_dict(CodecConfig(**kw))
    t = tables_npz()
    for k, f in (("gaussian_conditional._quantized_cdf", "gc_cdf"), ("gaussian_conditional._cdf_length", "gc_len"),
                 ("gaussian_conditional._offset", "gc_off"), ("entropy_bottleneck._quantized_cdf", "eb_cdf"),
                 ("entropy_bottleneck._cdf_length", "eb_len"), ("entropy_bottleneck._offset", "eb_off")):
        sd[k] = torch.from_numpy(t[f])
    net = ChannelProgresssiveWACNN(device="cuda:0", **kw)
    net.load_state_dict(sd)
    return net


def _profiled(net, fn):
    from progressivecodec_amd._lib import check, lib
    n, ms, fl = C.c_int64(), C.c_double(), C.c_double()
    check(lib().pc_codec_profile_begin(net._h), "pc_codec_profile_begin")
    r = fn()
    torch.cuda.synchronize()
    check(lib().pc_codec_profile_end(net._h, C.byref(n), C.byref(ms), C.byref(fl)), "pc_codec_profile_end")
    return r, n.value, fl.value


def _taps(net, M, nch):
    return [net.read_tap(k)[:M * 640].reshape(M, 640)[:, :nch].copy().view(np.uint32) for k in ("latent_means", "latent_scales")]


def _code(net, x, q, on):
    B, _, H, W = x.shape
    M = B * (H // 16) * (W // 16)
    net.set_option("group_siblings", on)
    o, n_enc, fl_enc = _profiled(net, lambda: net.compress(x, q, POL))
    nch = 320 if q == 0 else 640                                       # a base-only call computes the base half of the 640 channels
    taps_enc = _taps(net, M, nch)
    d, n_dec, fl_dec = _profiled(net, lambda: net.decompress(o["strings"], o["shape"], q, POL))
    return dict(strings=o["strings"], x_hat=d["x_hat"].cpu(), taps_enc=taps_enc, taps_dec=_taps(net, M, nch),
                n_enc=n_enc, n_dec=n_dec, fl_enc=fl_enc, fl_dec=fl_dec)


def _wam_pairs(M, C_):
    """wam() runs a[k] || b[k] as grouped launches when one launch of the module's 3x3 layer (N = C / 2) has fewer than 4 rounds of
    32x32 accumulator chains on the 1024 SIMDs"""
    return math.ceil(M / 32) * math.ceil((C_ // 2) / 32) < 4096


def _expected_drop(B, H, W, q, single_hyperprior, multiple_encoder):
    """launches saved per call (encoder, decoder), from the layer counts: a window-attention module has 2 x 3 ResidualUnits of 3 convs,
    18 launches, 9 when paired; a hyper-synthesis net has 5 layers: 4 nets 20 -> 1 + 2 * 4 = 9 launches, 2 nets 10 -> 1 + 4 = 5"""
    m4, m16 = B * (H // 4) * (W // 4), B * (H // 16) * (W // 16)
    cy = 320 if multiple_encoder else 640
    enc_wams = [(m4, 192), (m16, cy)] * (2 if multiple_encoder else 1)        # g_a: the H/4 module and the latent module, per encoder
    dec_wams = [(m16, 320), (m4, 192)]                                        # g_s: the latent module and the H/4 module
    assert all(_wam_pairs(M, C_) for M, C_ in enc_wams + dec_wams)            # (every module of these small shapes is under the threshold)
    hyper = 11 if (q != 0 and not single_hyperprior) else 5
    return 9 * len(enc_wams) + hyper, 9 * len(dec_wams) + hyper


CODEC_CASES = [
    ("canonical_q0_b2_64x64", (), 2, 64, 64, 0.0), ("canonical_q05_b2_64x64", (), 2, 64, 64, 0.5),
    ("canonical_q0_b1_128x192", (), 1, 128, 192, 0.0), ("canonical_q05_b1_128x192", (), 1, 128, 192, 0.5),
    ("single_hyperprior_q05_b2_64x64", (("multiple_hyperprior", False),), 2, 64, 64, 0.5),
    ("multiple_encoder_q05_b2_64x64", (("multiple_encoder", True),), 2, 64, 64, 0.5),
]


@pytest.mark.parametrize("name,kw,B,H,W,q", CODEC_CASES, ids=[c[0] for c in CODEC_CASES])
def test_codec_group_siblings_on_off(name, kw, B, H, W, q):
    net = _variant_net(kw) if kw else gpu_codec()
    x = inputs(B, H, W, 900 + B + H + W, "smooth").cuda()
    try:
        off = _code(net, x, q, 0)
        on = _code(net, x, q, 1)
    finally:
        net.set_option("group_siblings", 1)                            # the default (the canonical object is shared with other tests)
    assert on["strings"] == off["strings"]
    assert torch.equal(on["x_hat"].view(torch.int32), off["x_hat"].view(torch.int32))
    for k in ("taps_enc", "taps_dec"):
        for a, b, tap in zip(on[k], off[k], ("latent_means", "latent_scales")):
            assert np.array_equal(a, b), (k, tap)
    # the launch ledger: the same algorithmic FLOPs in fewer launches
    assert on["fl_enc"] == off["fl_enc"] and on["fl_dec"] == off["fl_dec"]
    d_enc, d_dec = _expected_drop(B, H, W, q, dict(kw).get("multiple_hyperprior") is False, bool(dict(kw).get("multiple_encoder")))
    assert off["n_enc"] - on["n_enc"] == d_enc, (off["n_enc"], on["n_enc"], d_enc)
    assert off["n_dec"] - on["n_dec"] == d_dec, (off["n_dec"], on["n_dec"], d_dec)

"""The conv launcher, path by path: every epilogue in every epilogue form, every production kernel instantiation, the operand and output
forms of the codec's layers, the grouped launch, the dual ReLU store and the documented refusals -- each case launched alone through
pc_test_conv (include/pcodec.h) and checked four ways:

  (a) bit-equal to the contract restatement (tests/conv_contract.py: the CPU oracle's chains + float32 epilogue);
  (b) within the rigorous float64 bound of the operation itself;
  (c) sentinels hold: the gaps of strided input segments and aux tensors hold a NaN of a distinctive payload (a read there poisons the
      result), and the gap columns of an output slice plus a guard band before and after every output tensor keep their sentinel bits;
  (d) `plan` names the instantiation and epilogue form the case is meant to reach.

The matrix closes with a coverage assertion over the production (instantiation, form) pairs (conv_contract.REQUIRED).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import conv_contract as cc

pytestmark = pytest.mark.gpu

GAP = np.uint32(0x7FE1A5A5)       # quiet NaN in the gaps of input segments and aux tensors
SENT = np.uint32(0x7FE2B6B6)      # quiet NaN around / between outputs
GUARD = 1024                      # floats of guard band on both sides of every output tensor
MAX_SEG = 8


class Desc(C.Structure):
    _fields_ = [("nseg", C.c_int), ("seg_ptr", C.c_void_p * MAX_SEG), ("seg_ld", C.c_int * MAX_SEG), ("seg_nch", C.c_int * MAX_SEG),
                ("smallc", C.c_int), ("in_sb", C.c_int64), ("in_sy", C.c_int64), ("in_sx", C.c_int64), ("in_sc", C.c_int64),
                ("Cin", C.c_int), ("B", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("kind", C.c_int), ("k", C.c_int), ("stride", C.c_int), ("square", C.c_int),
                ("w", C.c_void_p), ("bias", C.c_void_p), ("Cout", C.c_int), ("epi", C.c_int),
                ("aux0", C.c_void_p), ("ld0", C.c_int), ("aux1", C.c_void_p), ("ld1", C.c_int),
                ("fg_gamma", C.c_void_p), ("fg_beta", C.c_void_p),
                ("out", C.c_void_p), ("out_sb", C.c_int64), ("out_sy", C.c_int64), ("out_sx", C.c_int64), ("out_sc", C.c_int64),
                ("pixel_shuffle", C.c_int), ("out_relu", C.c_void_p),
                ("ngroup", C.c_int), ("g1_seg0", C.c_void_p), ("g1_w", C.c_void_p), ("g1_bias", C.c_void_p), ("g1_out", C.c_void_p),
                ("tile_cfg", C.c_int)]


def _lib():
    from progressivecodec_amd._lib import lib
    return lib()


def _f2u(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()


def addr(t, off_floats=0):
    return t.data_ptr() + 4 * off_floats


def pack(w, kind, Cout, Cin, k):
    n = 9 * 12 * Cin if kind == 2 else k * k * Cin * Cout
    out = np.empty(n, np.float32)
    rc = _lib().pc_pack_conv_weight(np.ascontiguousarray(w, np.float32).ctypes.data_as(C.c_void_p), kind, Cout, Cin, k,
                                    out.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return out


def strided(a2d, ld, off):
    """rows of a2d [P, n] at columns off .. off+n of a [P, ld] buffer whose other columns hold the GAP NaN"""
    P, n = a2d.shape
    assert off + n <= ld
    buf = np.full((P, ld), GAP, np.uint32)
    buf[:, off:off + n] = _f2u(a2d)
    return dev_u32(buf)


class Out:
    """an output tensor inside a sentinel-filled buffer with GUARD floats on both sides"""

    def __init__(self, c):
        B = c["B"]
        _, _, oh, ow, oc = cc.out_grid(c)
        self.c, self.shape = c, (B, oh, ow, oc)
        if c["out"] == "nchw":
            self.n = B * oc * oh * ow
            self.strides = (oc * oh * ow, ow, 1, oh * ow)
            self.off = 0
        else:
            ldo = c["ldo"] or oc
            assert c["ooff"] + oc <= ldo
            self.ldo = ldo
            self.n = B * oh * ow * ldo
            self.strides = (oh * ow * ldo, ow * ldo, ldo, 1)
            self.off = c["ooff"]
        self.t = torch.full((self.n + 2 * GUARD,), int(SENT), dtype=torch.int32, device="cuda")

    def ptr(self):
        return addr(self.t, GUARD + self.off)

    def expected(self, val):
        """the whole buffer as it must read: `val` [B, outH, outW, C] placed, sentinel everywhere else"""
        full = np.full(self.n + 2 * GUARD, SENT, np.uint32)
        body = full[GUARD:GUARD + self.n]
        B, oh, ow, oc = self.shape
        if self.c["out"] == "nchw":
            body.reshape(B, oc, oh, ow)[:] = _f2u(val).reshape(B, oh, ow, oc).transpose(0, 3, 1, 2)
        else:
            body.reshape(B * oh * ow, self.ldo)[:, self.off:self.off + oc] = _f2u(val).reshape(-1, oc)
        return full

    def host(self):
        return self.t.cpu().numpy().view(np.uint32)


def build(c, d, group=0):
    """device operands and the descriptor of one case (group 1 alone: the second GEMM of a grouped case as a launch of its own)"""
    keep = []
    desc = Desc()
    B, H, W, Cin = c["B"], c["H"], c["W"], c["Cin"]
    x = d["x1"] if group == 1 else d["x"]
    if c["smallc"]:
        if c["smallc"] == "nchw":
            t = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))).cuda()
            desc.in_sb, desc.in_sy, desc.in_sx, desc.in_sc = Cin * H * W, W, 1, H * W
        else:
            t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
            desc.in_sb, desc.in_sy, desc.in_sx, desc.in_sc = H * W * Cin, W * Cin, Cin, 1
        keep.append(t)
        desc.nseg, desc.smallc = 1, 1
        desc.seg_ptr[0], desc.seg_ld[0], desc.seg_nch[0] = addr(t), 0, Cin
    else:
        desc.nseg = len(c["segs"])
        c0 = 0
        for s, (nch, ld, off) in enumerate(c["segs"]):
            src = x if s == 0 else d["x"]
            t = strided(src[..., c0:c0 + nch].reshape(-1, nch), ld, off)
            keep.append(t)
            desc.seg_ptr[s], desc.seg_ld[s], desc.seg_nch[s] = addr(t, off), ld, nch
            c0 += nch
    desc.Cin, desc.B, desc.H, desc.W = Cin, B, H, W
    desc.kind, desc.k, desc.stride, desc.square = c["kind"], c["k"], c["stride"], int(c["square"])
    w, b = (d["w1"], d["b1"]) if group == 1 else (d["w"], d["b"])
    wp = pack(w, c["kind"], c["Cout"], Cin, c["k"])
    if c["kind"] == 2:
        assert np.array_equal(wp.reshape(9, 12, Cin), cc.pack_subpixel(w)), "pc_pack_conv_weight(kind 2) != the sub-pixel transform"
        b = np.repeat(b, 4)
    wt, bt = torch.from_numpy(wp).cuda(), torch.from_numpy(np.ascontiguousarray(b)).cuda()
    keep += [wt, bt]
    desc.w, desc.bias, desc.Cout = addr(wt), addr(bt), cc.gemm_cout(c)
    desc.epi = cc.EPI[c["epi"]]
    _, _, oh, ow, oc = cc.out_grid(c)
    if c["square"]:
        desc.aux0, desc.ld0 = desc.seg_ptr[0], desc.seg_ld[0]
    elif "aux0" in d:
        t = strided(d["aux0"].reshape(-1, oc), oc + 4, 0)
        keep.append(t)
        desc.aux0, desc.ld0 = addr(t), oc + 4
    if "aux1" in d:
        t = strided(d["aux1"].reshape(-1, oc), oc + 8, 4)
        keep.append(t)
        desc.aux1, desc.ld1 = addr(t, 4), oc + 8
    if c["fused_gdn"]:
        g, be = torch.from_numpy(d["gamma"]).cuda(), torch.from_numpy(d["beta"]).cuda()
        keep += [g, be]
        desc.fg_gamma, desc.fg_beta = addr(g), addr(be)
    out = Out(c)
    desc.out = out.ptr()
    desc.out_sb, desc.out_sy, desc.out_sx, desc.out_sc = out.strides
    desc.pixel_shuffle = int(c["ps"])
    relu = None
    if c["relu"]:
        relu = Out(c)
        desc.out_relu = relu.ptr()
    g1 = None
    if c["ngroup"] == 2 and group == 0:
        nch, ld, off = c["segs"][0]
        t = strided(d["x1"][..., :nch].reshape(-1, nch), ld, off)
        w1 = torch.from_numpy(pack(d["w1"], c["kind"], c["Cout"], Cin, c["k"])).cuda()
        b1 = torch.from_numpy(d["b1"]).cuda()
        keep += [t, w1, b1]
        g1 = Out(c)
        desc.ngroup, desc.g1_seg0, desc.g1_w, desc.g1_bias, desc.g1_out = 2, addr(t, off), addr(w1), addr(b1), g1.ptr()
    return desc, keep, out, relu, g1


def launch(desc):
    plan = (C.c_int * 2)()
    rc = _lib().pc_test_conv(C.byref(desc), plan, None)
    return rc, (cc.PLAN_NAME.get(plan[0], plan[0]), cc.FORM_NAME.get(plan[1], plan[1]))


def check_out(c, d, o, val, what):
    got = o.host()
    want = o.expected(val)
    exp_sent = want == SENT
    bad_sent = exp_sent & (got != SENT)
    assert not bad_sent.any(), f"{c['name']} {what}: {int(bad_sent.sum())} sentinel words overwritten " \
                               f"(first at buffer word {int(np.argmax(bad_sent))}, guard {GUARD})"
    bad = ~exp_sent & (got != want)
    assert not bad.any(), f"{c['name']} {what}: {int(bad.sum())} of {int((~exp_sent).sum())} outputs differ from the restatement"


def check_out_nan(c, d, o, val, what):
    """check_out for operands outside the ordinary (tests/test_gpu_hostile_values.py): every sentinel word holds, every output equals
    the restatement bit for bit -- except that where both are NaN only NaN-ness is compared (the payload a NaN operation keeps is not
    part of the contract).  Returns the count of such NaN pairs whose payloads differ."""
    got = o.host()
    want = o.expected(val)
    exp_sent = want == SENT
    bad_sent = exp_sent & (got != SENT)
    assert not bad_sent.any(), f"{c['name']} {what}: {int(bad_sent.sum())} sentinel words overwritten " \
                               f"(first at buffer word {int(np.argmax(bad_sent))}, guard {GUARD})"
    both_nan = ~exp_sent & np.isnan(got.view(np.float32)) & np.isnan(want.view(np.float32))
    bad = ~exp_sent & (((got != want) & ~both_nan) | (got == SENT))       # an output that still reads as the sentinel was never stored
    if bad.any():
        i = int(np.argmax(bad))
        raise AssertionError(f"{c['name']} {what}: {int(bad.sum())} of {int((~exp_sent).sum())} outputs differ from the restatement, "
                             f"first at buffer word {i}: got {got[i]:#010x}, restatement {want[i]:#010x}")
    return int((both_nan & (got != want)).sum())


def values(o):
    """the output tensor's values [B, outH, outW, C] read back from its buffer"""
    B, oh, ow, oc = o.shape
    body = o.host()[GUARD:GUARD + o.n].view(np.float32)
    if o.c["out"] == "nchw":
        return body.reshape(B, oc, oh, ow).transpose(0, 2, 3, 1)
    return body.reshape(B * oh * ow, o.ldo)[:, o.off:o.off + oc].reshape(B, oh, ow, oc)


REACHED = set()
CASES = cc.matrix()


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_conv_matrix_case(c):
    d = cc.make_data(c)
    desc, keep, out, relu, g1 = build(c, d)
    rc, plan = launch(desc)
    assert rc == 0, f"{c['name']}: pc_test_conv returned {rc}"
    torch.cuda.synchronize()
    REACHED.add(plan)
    assert plan == tuple(c["expect"]), f"{c['name']}: launcher chose {plan}, the case is meant for {tuple(c['expect'])}"
    want = cc.restate(c, d)
    check_out(c, d, out, want, "out")                                         # (a) bits + (c) sentinels
    ok, ratio, nbad = cc.within(c, values(out), d)                             # (b)
    assert ok, f"{c['name']}: {nbad} outputs outside the float64 bound (worst ratio {ratio:.3g})"
    if relu is not None:
        check_out(c, d, relu, np.where(want > 0, want, np.float32(0)).astype(np.float32), "out_relu")
    if g1 is not None:
        want1 = cc.restate(c, d, group=1)
        check_out(c, d, g1, want1, "group 1")
        ok, ratio, nbad = cc.within(c, values(g1), d, group=1)
        assert ok, f"{c['name']} group 1: {nbad} outputs outside the float64 bound (worst ratio {ratio:.3g})"
        # the two groups as separate launches give the same bits
        for grp, o in ((0, out), (1, g1)):
            c1 = dict(c, ngroup=1)
            desc1, keep1, out1, _, _ = build(c1, d, group=grp)
            rc1, _ = launch(desc1)
            assert rc1 == 0
            torch.cuda.synchronize()
            assert np.array_equal(out1.host(), o.host()), f"{c['name']}: group {grp} differs from its separate launch"
    del keep


def test_conv_matrix_coverage():
    """every production (instantiation, epilogue form) pair was reached -- if a selection threshold moves, this fails instead of the
    matrix quietly testing one path twice"""
    if len(REACHED) == 0:
        for c in CASES:
            d = cc.make_data(c)
            desc, keep, *_ = build(c, d)
            rc, plan = launch(desc)
            assert rc == 0
            REACHED.add(plan)
        torch.cuda.synchronize()
    missing = cc.REQUIRED - REACHED
    assert not missing, f"production pairs not reached: {sorted(missing)}; reached {sorted(REACHED)}"


# ---------------------------------------------------------------------------------------------------------------- refusals
def _refusal(name, edit):
    c = dict({x["name"]: x for x in CASES}[name])
    edit(c)
    return c, cc.make_data(c)


def _se_on_deconv(c):
    c.update(epi="SE_ADD")


def _bad_align(desc):
    desc.seg_ptr[0] += 4


REFUSALS = {
    "out_relu_non_dense": ("nchw_NONE", lambda c: c.update(relu=True), None),
    "se_add_four_phases": ("deconv_none", _se_on_deconv, None),
    "fused_gdn_cout_96": ("in_gdn", lambda c: c.update(Cout=96), None),
    "misaligned_segment": ("direct_NONE", None, _bad_align),
    "nch_not_multiple_of_16": ("direct_NONE", lambda c: c.update(segs=[(24, 24, 0)], Cin=24), None),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_conv_refusal(what):
    name, edit, poke = REFUSALS[what]
    c, d = _refusal(name, edit or (lambda c: None))
    desc, keep, out, relu, g1 = build(c, d)
    if poke:
        poke(desc)
    rc, _ = launch(desc)
    torch.cuda.synchronize()
    assert rc == -1, f"{what}: pc_test_conv returned {rc}, PC_ERR_ARG (-1) expected"
    for o in (out, relu, g1):
        if o is not None:
            assert (o.host() == SENT).all(), f"{what}: a refused launch wrote its output"


# ---------------------------------------------------------------------------------------------------------------- > 2^32 bytes
def test_conv_operand_beyond_4gb():
    """a 3x3 32 -> 32 layer whose input and output each pass 2^32 bytes (one full-resolution 32-channel UNet tensor of a 4096 x 4224
    frame, two images): output pixels sampled at tile boundaries, around the 2^32-byte mark and in the last rows, checked against the
    restatement (bits) and float64 (bound) computed for those pixels only; the guard bands around the output stay intact"""
    B, H, W, Cin, Cout = 2, 4096, 4224, 32, 32
    M = B * H * W
    assert M * Cin * 4 > 2 ** 32
    rng = np.random.default_rng(77)
    w = (rng.standard_normal((Cout, Cin, 3, 3)) * (2.0 / (9 * Cin)) ** 0.5).astype(np.float32)
    b = (rng.standard_normal(Cout) * 0.1).astype(np.float32)
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(M * Cin, device="cuda", generator=gen, dtype=torch.float32)
    out = torch.full((M * Cout + 2 * GUARD,), int(SENT), dtype=torch.int32, device="cuda")
    wt, bt = torch.from_numpy(pack(w, 0, Cout, Cin, 3)).cuda(), torch.from_numpy(b).cuda()
    desc = Desc()
    desc.nseg, desc.seg_ptr[0], desc.seg_ld[0], desc.seg_nch[0] = 1, addr(x), Cin, Cin
    desc.Cin, desc.B, desc.H, desc.W, desc.kind, desc.k, desc.stride = Cin, B, H, W, 0, 3, 1
    desc.w, desc.bias, desc.Cout, desc.epi = addr(wt), addr(bt), Cout, cc.EPI["NONE"]
    desc.out = addr(out, GUARD)
    desc.out_sb, desc.out_sy, desc.out_sx, desc.out_sc = H * W * Cout, W * Cout, Cout, 1
    rc, plan = launch(desc)
    assert rc == 0
    torch.cuda.synchronize()
    assert plan == ("UNI_16_3", "DIRECT"), plan
    assert (out[:GUARD] == int(SENT)).all().item() and (out[-GUARD:] == int(SENT)).all().item()
    mark = 2 ** 32 // (4 * Cout)                                   # first output pixel at or beyond byte 2^32
    ms = {0, 63, 64, 65, mark - 65, mark - 64, mark - 1, mark, mark + 1, mark + 63, H * W - 1, H * W, M - W, M - 65, M - 64, M - 1}
    ms |= set(int(v) for v in rng.integers(0, M, 200))
    ms = np.array(sorted(ms), np.int64)
    bb, rr = ms // (H * W), ms % (H * W)
    yy, xx = rr // W, rr % W
    # 3x3 neighbourhoods of the sampled pixels (zero outside the image), gathered on the device
    xv = x.view(B, H, W, Cin)
    patch = torch.zeros(len(ms), 3, 3, Cin)
    for dy in range(3):
        for dx in range(3):
            iy, ix = torch.from_numpy(yy + dy - 1), torch.from_numpy(xx + dx - 1)
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            vals = xv[torch.from_numpy(bb).cuda(), iy.clamp(0, H - 1).cuda(), ix.clamp(0, W - 1).cuda()].cpu()
            patch[:, dy, dx] = torch.where(ok[:, None], vals, torch.zeros(()))
    got = out[GUARD:GUARD + M * Cout].view(M, Cout)[torch.from_numpy(ms).cuda()].cpu().numpy().view(np.float32)
    pc = cc.case("beyond_4gb_sample", len(ms), 3, 3, segs=[(Cin, Cin, 0)], k=3, Cout=Cout)
    pd = dict(x=patch.numpy(), w=w, b=b)
    want = cc.restate(pc, pd)[:, 1, 1, :]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{int((got != want).sum())} sampled outputs differ"
    ref, bound = cc.reference64(pc, pd)
    assert (np.abs(got - ref[:, 1, 1, :]) <= bound[:, 1, 1, :]).all()

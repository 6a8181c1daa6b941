"""The non-conv stage launchers, path by path (progressivecodec_amd/csrc/pc_stages.hip; GDN through the conv launcher): every case of
tests/stage_contract.py launched alone, once, through pc_test_stage (include/pcodec.h) and checked four ways:

  (a) bit-equal to the contract restatement wherever the stage is specified bit-exact (the two likelihoods are held to (b) only);
  (b) within the derived float64 bound of the operation itself, integer and mask outputs as decisions under the exclusion cap;
  (c) sentinels hold: every input gap (the columns beside a slice, the bytes before an offset base pointer, the space between batch strides)
      holds a quiet NaN of a distinctive payload, and every output buffer -- guard bands, gap columns, batch gaps -- must read back as the
      restatement placed in a sentinel-filled buffer, bit for bit;
  (d) `plan` is the kernel variant the case was written to reach.

It closes with the coverage assertion over stage_contract.REQUIRED; the refusals must come back PC_ERR_ARG from the host with every output
untouched.  Worst |got - ref| / bound per family is printed (a record, not a threshold).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import stage_contract as sc

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in sc.matrix()}
REACHED = set()
WORST = {}


def _lib():
    from progressivecodec_amd._lib import lib
    return lib()


def build(c, d):
    """(descriptor, {field: (spec, device tensor, expected-if-untouched words, index)})"""
    desc = sc.Desc()
    desc.size, desc.kind = C.sizeof(sc.Desc), sc.KIND[c["kind"]]
    for k, v in sc.scalars(c, d).items():
        setattr(desc, k, v)
    bufs = {}
    for sp in sc.specs(c, d):
        buf, ptr, index = sc.layout(sp)
        if sp["arr"] is not None:
            buf[index] = sc.as_words(sp["arr"])
        t = torch.from_numpy(buf.view(np.int32) if buf.dtype == np.uint32 else buf).cuda()
        setattr(desc, sp["field"], t.data_ptr() + ptr * sp["dtype"].itemsize)
        bufs[sp["field"]] = (sp, t, buf, index)
    return desc, bufs


def read(t):
    a = t.cpu().numpy()
    return a if a.dtype == np.uint8 else a.view(np.uint32)


def test_descriptor_size_is_checked_first():
    plan = (C.c_int * 1)(7)
    c = CASES["q_8192"]                                       # a descriptor that is valid in everything but its size
    desc, bufs = build(c, sc.make_data(c))
    for size in (0, C.sizeof(sc.Desc) - 4, C.sizeof(sc.Desc) + 8):
        desc.size = size
        assert _lib().pc_test_stage(C.byref(desc), plan, None) == sc.PC_ERR_ARG
        assert plan[0] == 0
    torch.cuda.synchronize()
    for field, (sp, t, buf, index) in bufs.items():
        assert np.array_equal(read(t), buf), f"{field} was written although the size was wrong"
    desc.size = C.sizeof(sc.Desc)                             # and the mirror's own size is the one the library accepts
    assert _lib().pc_test_stage(C.byref(desc), plan, None) == 0
    torch.cuda.synchronize()
    assert plan[0] == sc.SPLAN["Q_REG8"]


@pytest.mark.parametrize("name", list(CASES))
def test_stage_case(name):
    c = CASES[name]
    d = sc.make_data(c)
    want = sc.restate(c, d)
    desc, bufs = build(c, d)
    plan = (C.c_int * 1)(0)
    rc = _lib().pc_test_stage(C.byref(desc), plan, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = {}
    for field, (sp, t, buf, index) in bufs.items():
        host = read(t)
        if not sp["out"]:
            assert np.array_equal(host, buf), f"{name}: input {field} was written"
            continue
        scratch = (c["kind"], field) in sc.SCRATCH
        if not scratch:
            got[field] = host[index].view(sp["dtype"]) if sp["dtype"].itemsize == 4 else host[index]
        exp = buf.copy()
        if scratch:                                                             # (c) alone: the launcher's own scratch keeps inside its bounds
            exp[index] = host[index]
        elif (c["kind"], field) in sc.BOUND_ONLY:                                 # (c) alone: everything outside the tensor
            exp[index] = host[index]
            nbits = int((sc.as_words(want[field]) != host[index]).sum())
            print(f"{name}: {field} differs from the restatement in {nbits} of {index.size} elements (held to the float64 bound)")
        else:
            exp[index] = sc.as_words(want[field])                               # (a) and (c) at once
        diff = np.flatnonzero(host != exp)
        inside = np.isin(diff, index.reshape(-1)).sum() if diff.size else 0
        assert diff.size == 0, f"{name}: {field}: {diff.size} words differ ({inside} inside the tensor, {diff.size - inside} sentinels), first at {diff[:4]}"
    ok, res, ratio = sc.check64(c, d, got)                                       # (b)
    print(f"{name}: plan {plan[0]} float64 check {res} worst ratio {ratio:.3g}")
    assert ok, f"{name}: {res} (exclusion cap {sc.exclusion_cap(c, got)})"
    fam = sc.family(c)
    WORST[fam] = (WORST.get(fam, (0, 0.0))[0] + 1, max(WORST.get(fam, (0, 0.0))[1], ratio))
    assert plan[0] == sc.SPLAN[c["expect"]], f"{name}: plan {plan[0]}, written for {c['expect']} ({sc.SPLAN[c['expect']]})"     # (d)
    REACHED.add((c["kind"], c["expect"]))


@pytest.mark.parametrize("name,base,over", sc.refusals(), ids=[r[0] for r in sc.refusals()])
def test_stage_refusal(name, base, over):
    c = CASES[base]
    desc, bufs = build(c, sc.make_data(c))
    for k, v in over.items():
        if isinstance(v, tuple):
            setattr(desc, k, getattr(desc, k) + v[1])
        else:
            setattr(desc, k, v)
    plan = (C.c_int * 1)(7)
    assert _lib().pc_test_stage(C.byref(desc), plan, None) == sc.PC_ERR_ARG
    assert plan[0] == 0
    torch.cuda.synchronize()
    for field, (sp, t, buf, index) in bufs.items():
        assert np.array_equal(read(t), buf), f"{name}: {field} was written by a refused launch"


def test_stage_matrix_coverage():
    for fam, (n, ratio) in sorted(WORST.items()):
        print(f"{fam}: {n} cases, worst |got - ref| / bound = {ratio:.3g}")
    missing = sc.REQUIRED - REACHED
    assert not missing, f"production variants no case reached: {sorted(missing)}"

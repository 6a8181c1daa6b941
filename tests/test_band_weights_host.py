"""The witness tile sets of tests/band_cases.py can see the errors they are built for (no GPU): mutants of tests/tiles_contract.py
-- every inexact weight one ulp up, one ulp down, the product wy * wx left unrounded inside the fused multiply-add, a rounded
multiply and a rounded add in place of the fmaf -- run through the three restatements that blend through it, and what they change
is counted.  These are conditions, not measurements: tests/test_gpu_band_weights.py puts the same sets through the kernels and
asserts exact equality with the unbroken restatement, so a kernel that is one of these mutants fails there on every sample counted
here.

Counts measured with this table: the fewest DISTINCT witness values the search finds for an inexact weight and a direction, over
the four quantisers, are O = 12: 8, O = 20: 5, O = 24: 4, O = 28: 5, O = 40: 3, O = 48: 2, O = 96: 1 -- no coordinate is left out,
at O = 96 either (the search tries 8 floats either side of every tie).  A band row repeats its witnesses over its columns, so every
inexact coordinate has at least 64 witnessing SAMPLES per axis, side and direction (96 at O = 96).  Corner sets: "unrounded" changes
31 .. 4097 samples of the "zero" set, "unfused" 55 .. 5246 of the "lit" set and none of the "zero" set (acc = 0 there, and
fl(fl(w v) + 0) is the fmaf).
"""
from fractions import Fraction

import numpy as np
import pytest

from tests import band_cases as BC
from tests import tiles_contract as TC


def test_the_table_is_the_gap():
    """at every overlap of the table a weight is no float32; at the overlaps every GPU test used before, none is"""
    for T, O in BC.OVERLAPS:
        TC.check(T, O)
        assert BC.inexact_coordinates(O), (T, O)
        w = TC.weights(1, 2, T, O)[:O].astype(np.float64) * (2 * O)
        assert [u for u in range(O) if w[u] != 2 * u + 1] == BC.inexact_coordinates(O)
    for T, O in BC.DYADIC:
        assert BC.inexact_coordinates(O) == [], (T, O)
        w = TC.weights(1, 2, T, O)[:O]
        assert (w.astype(np.float64) * (2 * O) == 2 * np.arange(O) + 1).all()
        assert (TC.product(w, w).astype(np.float64) == np.outer(w.astype(np.float64), w.astype(np.float64))).all()      # the products too
    assert BC.COMPLETE == [(T, O) for T, O in BC.OVERLAPS if O <= 48] and (192, 96) in BC.OVERLAPS


def test_a_mutant_leaves_nothing_behind():
    before = TC.weights, TC.product, TC.fmaf
    for name in BC.MUTANTS:
        with BC.mutant(name):
            assert (TC.weights, TC.product, TC.fmaf) != before
        assert (TC.weights, TC.product, TC.fmaf) == before
    with BC.mutant("up"):
        w = TC.weights(1, 2, 64, 12)
        assert w[1] == np.float32(0.125) and w[0] == np.nextafter(np.float32(1) / np.float32(24), np.float32(1)) and w[12] == 1
    with BC.mutant("down"):
        assert TC.weights(0, 2, 64, 12)[63] == np.nextafter(np.float32(1) / np.float32(24), np.float32(0))
    with BC.mutant("up"):
        assert (TC.weights(1, 2, 64, 16) == before[0](1, 2, 64, 16)).all()                   # dyadic: nothing to move


def test_the_integer_fma_is_the_contracts_on_float32_weights():
    g = np.random.default_rng(0)
    a, b, c = (g.uniform(0, 1, 600).astype(np.float32) for _ in range(3))
    b[::7] = 0
    a64 = a.astype(np.float64) * (1 + 2.0 ** -30)                                            # no float32: the integer path
    got = BC.fmaf_unrounded(a64, b, c)
    assert got.dtype == np.float32
    for x, y, z, r in zip(a64, b, c, got):                                                   # no float32 lies nearer to the exact value
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        err = abs(Fraction(float(r)) - exact)
        assert all(err <= abs(Fraction(float(np.nextafter(r, np.float32(t)))) - exact) for t in (-1, 2))
    assert (BC.fmaf_unrounded(a.astype(np.float64), b, c) == TC.fmaf(a, b, c)).all()
    # one case by hand: (1 + 2^-30) * (1 + 2^-23) + 2^-24 = 1 + 2^-23 + 2^-24 + 2^-30 + ..: just above the tie, rounds up
    one = BC.fmaf_unrounded(np.float64(1 + 2.0 ** -30), np.float32(1 + 2.0 ** -23), np.float32(2.0 ** -24))
    assert one == np.float32(1 + 2.0 ** -22)
    assert TC.fmaf(np.float32(1), np.float32(1 + 2.0 ** -23), np.float32(2.0 ** -24)) == np.float32(1 + 2.0 ** -22)       # the tie: to even


def witnessed(lib, param, q, T, O, name):
    """{(axis, side): per band coordinate the number of samples of the band sets whose code the mutant changes}"""
    out = {}
    S = T - O
    for axis, side, _, x, H, W in BC.band_sets(T, O, q):
        win = (S, 0, O, W) if axis == 0 else (0, S, H, O)
        ref = BC.render(lib, param, x, H, W, T, O, win)
        with BC.mutant(name):
            mut = BC.render(lib, param, x, H, W, T, O, win)
        out[(axis, side)] = out.get((axis, side), 0) + (ref != mut).sum(axis=1 - axis)
    return out


#: O = 96: the numerators whose weight no sample of the sets witnesses, per direction.  Recorded, and asserted exactly.
UNWITNESSED_96 = {"up": [], "down": []}


@pytest.mark.parametrize("TO", BC.OVERLAPS)
def test_every_inexact_band_coordinate_has_a_witness_for_either_direction(TO):
    """per library, axis and tile of the band: a weight one ulp up and one ulp down each change a code in every row (column) whose
    weight is no float32, and in no row whose weight is one"""
    T, O = TO
    lowest = None
    for lib, param, q in BC.LIBRARIES:
        for name in ("up", "down"):
            for (axis, side), count in witnessed(lib, param, q, T, O, name).items():
                nums = [2 * u + 1 if side else 2 * (O - 1 - u) + 1 for u in range(O)]
                need = [u for u in range(O) if BC.inexact(nums[u], O)]
                assert all(count[u] == 0 for u in range(O) if u not in need)
                missing = sorted(nums[u] for u in need if count[u] == 0)
                case = (T, O, lib, param, name, axis, side)
                if TO in BC.COMPLETE:
                    assert missing == [], case
                else:
                    assert missing == UNWITNESSED_96[name], case
                seen = min(count[u] for u in need if nums[u] not in missing)
                lowest = seen if lowest is None else min(lowest, seen)
    print(f"T = {T}, O = {O}: at least {lowest} witnessing samples per inexact coordinate, axis, side and direction")
    assert lowest >= 1


@pytest.mark.parametrize("TO", BC.OVERLAPS)
def test_the_corner_sets_see_an_unrounded_product_and_an_unfused_add(TO):
    T, O = TO
    win = BC.corner_window(T, O)
    for lib, param, q in BC.LIBRARIES:
        changed = {}
        for kind, names in [("zero", ("unrounded", "unfused")), ("lit", ("unfused",))]:
            x, H, W = BC.corner_set(T, O, q, kind)
            assert not x[:3].any() if kind == "zero" else x[:3].any()
            ref = BC.render(lib, param, x, H, W, T, O, win)
            for name in names:
                with BC.mutant(name):
                    changed[(kind, name)] = int((BC.render(lib, param, x, H, W, T, O, win) != ref).sum())
        print(f"T = {T}, O = {O}, {lib} {param}: {changed}")
        assert changed[("zero", "unrounded")] >= 1 and changed[("lit", "unfused")] >= 1, (TO, lib, param, changed)
        assert changed[("zero", "unfused")] == 0                       # why there is a "lit" set: three zero tiles cannot see it


@pytest.mark.parametrize("TO", BC.OVERLAPS)
def test_a_one_row_windows_float_sum_carries_its_weight(TO):
    """what tests/test_gpu_band_weights.py's one-row windows rest on: against an all-zero reference sse_f = sum m^2 over the row, and
    with the row's weight one ulp off in either direction it moves by more than a thousand times the GPU test's bound
    w * 2^-53 * sse_f -- for every inexact coordinate of either tile of the band, those of O = 96 included"""
    T, O = TO
    S = T - O
    least = None
    for side in (0, 1):
        x, H, W = BC.band_set(T, O, "nearest", 0, side, 0)
        zero = np.zeros((3, H, W), np.uint8)
        for u in range(O):
            if not BC.inexact(2 * u + 1 if side else 2 * (O - 1 - u) + 1, O):
                continue
            win = (S + u, 0, 1, W)
            ref = TC.sums(x, H, W, T, O, "nearest", zero, "chw", window=win)[1][0]
            for name in ("up", "down"):
                with BC.mutant(name):
                    moved = TC.sums(x, H, W, T, O, "nearest", zero, "chw", window=win)[1][0]
                ratio = abs(moved - ref) / (W * 2.0 ** -53 * ref)
                least = ratio if least is None else min(least, ratio)
    print(f"T = {T}, O = {O}: a one-ulp weight moves a one-row sum by at least {least:.3g} times the bound")
    assert least > 1000


def test_the_sets_are_deterministic_and_inside_the_unit_interval():
    for T, O in BC.OVERLAPS[:2]:
        for q in BC.QUANTISERS:
            a = BC.band_set(T, O, q, 0, 1, 0)[0]
            BC.band_set.cache_clear()
            BC.witnesses.cache_clear()
            b = BC.band_set(T, O, q, 0, 1, 0)[0]
            assert a is not b and np.array_equal(a.view(np.int32), b.view(np.int32))
            assert (a >= 0).all() and (a <= 1).all() and not a[0].any() and a[1, :, :O].all() and not a[1, :, O:].any()
            t = BC.band_set(T, O, q, 1, 1, 0)[0]
            assert np.array_equal(t, a.transpose(0, 1, 3, 2))

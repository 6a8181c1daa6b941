"""CPU check of tests/conv_contract.py: for every case of the conv launcher matrix the float32 contract restatement lies within the
rigorous float64 bound of the operation itself, and each deliberate layout mistake of the restatement leaves it (no GPU needed)."""
import numpy as np
import pytest

from tests import conv_contract as cc

CASES = {c["name"]: c for c in cc.matrix()}


def test_matrix_names_are_unique_and_cover_the_required_pairs():
    cases = cc.matrix()
    assert len(CASES) == len(cases)
    assert {tuple(c["expect"]) for c in cases} >= cc.REQUIRED
    assert {c["epi"] for c in cases} == set(cc.EPI)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_within_float64_bound(name):
    c = CASES[name]
    d = cc.make_data(c)
    for g in range(c["ngroup"]):
        got = cc.restate(c, d, group=g)
        ok, ratio, nbad = cc.within(c, got, d, group=g)
        assert ok, f"{name} group {g}: {nbad} elements outside the bound (worst |err| / bound = {ratio:.3g})"
        assert np.isfinite(got).all()


MUTANTS = [
    ("taps_flipped", "direct_NONE"),
    ("taps_flipped", "deconv_none"),
    ("cin_cout_swapped", "relu_store_res"),
    ("ps_order", "ps_nhwc_gelu"),
    ("se_per_pixel", "nchw_SE_ADD"),
    ("gate_aux_swapped", "direct_GATE"),
    ("subpixel_phase", "subpixel_nchw_ps_none"),
]


def test_every_mutation_has_a_case():
    assert {m for m, _ in MUTANTS} == set(cc.MUTATIONS)


@pytest.mark.parametrize("mutation,name", MUTANTS)
def test_mutation_leaves_the_bound(mutation, name):
    c = CASES[name]
    d = cc.make_data(c)
    ok, ratio, nbad = cc.within(c, cc.restate(c, d, mutate=mutation), d)
    assert not ok, f"the bound does not see {mutation} on {name} (worst ratio {ratio:.3g})"
    assert ratio > 100, f"{mutation} on {name} only {ratio:.3g} x the bound"

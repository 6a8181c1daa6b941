"""CPU check of tests/stage_contract.py (no GPU needed): for every case of the stage matrix the float32 restatement lies within the derived
float64 bound of the operation itself with its exclusions under the cap, each listed misreading of a kernel leaves the bound on at least
one case, and the ctypes mirror of pc_test_stage_desc agrees with include/pcodec.h."""
import ctypes as C

import numpy as np
import pytest

from tests import stage_contract as sc

CASES = {c["name"]: c for c in sc.matrix()}


def test_matrix_names_are_unique_and_cover_the_required_variants():
    cases = sc.matrix()
    assert len(CASES) == len(cases)
    assert {(c["kind"], c["expect"]) for c in cases} >= sc.REQUIRED
    assert all(c["expect"] in sc.SPLAN and c["kind"] in sc.KIND for c in cases)
    assert all(base in CASES for _, base, _ in sc.refusals())


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_within_float64_bound(name):
    c = CASES[name]
    d = sc.make_data(c)
    outs = sc.restate(c, d)
    ok, res, ratio = sc.check64(c, d, outs)
    print(name, res, "exclusion cap", sc.exclusion_cap(c, outs))
    assert ok, f"{name}: {res} (cap {sc.exclusion_cap(c, outs)})"
    for sp in sc.specs(c, d):                      # every output has a layout, and the layout holds it
        if sp["out"] and (c["kind"], sp["field"]) not in sc.SCRATCH:
            assert outs[sp["field"]].shape == sp["shape"], (sp["field"], outs[sp["field"]].shape, sp["shape"])
            buf, ptr, index = sc.layout(sp)
            assert index.max() < buf.size - sc.GUARD and index.min() >= sc.GUARD


def test_twins_share_their_data():
    """the cases that break one vec precondition compute exactly what their aligned twin computes"""
    groups = {}
    for c in CASES.values():
        if "@" in c["name"]:
            groups.setdefault(c["name"].split("@")[0], []).append(c)
    assert len(groups) >= 4
    for g in groups.values():
        outs = [sc.restate(c, sc.make_data(c)) for c in g]
        for o in outs[1:]:
            for k in o:
                n = min(len(o[k]), len(outs[0][k]))
                assert np.array_equal(sc.as_words(o[k][:n]), sc.as_words(outs[0][k][:n])), (g[0]["name"], k)


MUTANTS = [
    ("bias_transposed", "att_8_24_s0_ji0"), ("bias_transposed", "att_4_40_s2_ji1"), ("roll_direction", "att_8_24_s1_ji0"),
    ("roll_direction", "att_4_80_s3_ji1"), ("region_boundary", "att_8_24_s1_ji1"), ("region_boundary", "att_4_40_s3_ji0"),
    ("channel_major", "att_4_80_s0_ji0"), ("channel_major", "att_8_24_s4_ji1"),
    ("table_le", "enc_mode0_edges"), ("mask_gt", "enc_mode1_none"), ("round_away", "enc_mode0_none"), ("ybase_added", "enc_mode2_all"),
    ("index_from_s", "enc_mode3_none"), ("index_from_s", "enc_mode1_none"), ("yadd_dropped", "enc_mode1_all"),
    ("lik_from_sym", "enc_lik_large_mu"), ("star_bar_swapped", "rem_sc_12"), ("star_bar_swapped", "rem_mu_21"),
    ("halves_swapped", "rem_mu_20"), ("median_dropped", "eb_dequant_c192_hw4"), ("nan_dropped", "pool_c4_2x2"),
    ("mean_by_chunk", "se_c32_hw4097@b1"), ("mean_by_chunk", "se_c16_hw12293@b1"),
]


def test_every_mutation_has_a_case():
    assert {m for m, _ in MUTANTS} == set(sc.MUTATIONS)


@pytest.mark.parametrize("mutation,name", MUTANTS)
def test_mutation_leaves_the_bound(mutation, name):
    c = CASES[name]
    assert sc.family(c) == sc.MUTATIONS[mutation]
    d = sc.make_data(c)
    ok, res, ratio = sc.check64(c, d, sc.restate(c, d, mutate=mutation))
    assert not ok, f"check (b) does not see {mutation} on {name}: {res}"


def test_ctypes_mirror_agrees_with_the_header():
    hdr = sc.header_fields()
    assert [n for _, n in hdr] == [n for n, _ in sc.Desc._fields_]
    assert [t for t, _ in hdr] == [t for _, t in sc.Desc._fields_]
    # natural alignment of the same member sequence: the C compiler's sizeof on LP64
    off = 0
    for t, _ in hdr:
        a = C.alignment(t)
        off = (off + a - 1) // a * a + C.sizeof(t)
    assert C.sizeof(sc.Desc) == (off + 7) // 8 * 8

"""tests/chroma_clips_limits.py without a GPU: the table does what it claims.  The closed forms are the restatement's values at a small
T and the listed numbers at the table's T; the rows of partials are as long as the cases say (from the library's own workspace-size
function) and take the stated trips; the witness samples land where the cases say, by the table's layout model, which is held to the
restatement first; and every mutant of the model -- a subtly wrong kernel -- differs from the restatement on a named case, so that
tests/test_gpu_chroma_clips_limits.py would fail on it."""
import itertools

import pytest

from tests import chroma_clips_contract as CK
from tests import chroma_clips_limits as XL
from tests import chroma_contract as CC
from tests import image_limits as IL
from tests import tiles_contract as TC

RULES = list(itertools.product(CC.SITINGS, CC.UPSAMPLES))
SMALL_SIDES = dict(T=64, O=0, H=140, W=140, tile=4)                        # the grid shape of XL.RING_SIDES at a small T


def geo(c):
    return tuple(c[k] for k in ("H", "W", "T", "O"))


# -- the table against the restatement -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["nv12", "p210", "i420", "nv16"])
def test_the_side_pairs_closed_form_is_the_restatement_at_a_small_tile(fmt):
    c = SMALL_SIDES
    H, W, T, O = geo(c)
    assert TC.grid(H, W, T, O) == (3, 3)
    for side in XL.SIDES:
        cur, prev = XL.ring_side_pair(fmt, side, c)
        for siting, up in RULES:
            assert CK.tile_changes(cur, prev, fmt, siting, T, O, up, 4, 1) == [XL.ring_side_expect(fmt, siting, up, side, c)], (side, siting, up)


@pytest.mark.parametrize("fmt,loop,trips", XL.RING_SIDES_FORMATS)
def test_the_side_pairs_at_the_tables_tile(fmt, loop, trips):
    """the restatement gives side length or 0 per lo / hi; the loop covers 1156 and 1732 indices, five and seven trips; Cb and Cr
    differ in different numbers of samples"""
    c = XL.RING_SIDES
    H, W, T, O = geo(c)
    assert TC.grid(H, W, T, O) == (3, 3)
    row, _, _ = XL.ring(H, W, T, O, fmt, XL.rule(fmt, "centre", "linear"), 4)
    assert len(row) == loop and -(-loop // XL.NT) == trips
    seen = set()
    for side in XL.SIDES:
        cur, prev = XL.ring_side_pair(fmt, side)
        for siting, up in RULES:
            want = XL.ring_side_expect(fmt, siting, up, side)
            assert CK.tile_changes(cur, prev, fmt, siting, T, O, up, 4, 1) == [want], (side, siting, up)
            assert want[1] == 0 or want[1] != want[2]
            seen.add((side, want[1] > 0))
    sy = CC.sub(fmt)[1]
    assert seen == {(s, on) for s in XL.SIDES for on in (False, True) if on is False or sy == 2 or s in ("left", "right")}
    assert XL.ring_side_expect("nv12", "centre", "linear", "above") == [0, 290, 283]
    assert XL.ring_side_expect("nv12", "centre", "linear", "corners") == [0, 4, 1]
    assert XL.ring_side_expect("nv12", "topleft", "linear", "corners") == [0, 1, 0]
    assert XL.ring_side_expect("p210", "left", "linear", "right") == [0, 576, 571] and XL.ring_side_expect("p210", "left", "linear", "left") == [0, 0, 0]


@pytest.mark.parametrize("fmt", XL.RING_SMALL_FORMATS)
def test_the_small_rings_witness_samples_are_the_loops_second_trip(fmt):
    """T = 128, tile 4 of 300 x 300: under centre / linear nv12's loop covers 2 * 66 + 2 * 64 = 260 indices and the four changed Cb
    samples are indices 256 .. 259; nv16's covers 2 * 66 + 2 * 128 = 388, its top and bottom are off, and the changed samples are
    indices 256 .. 259 (Cr, left column) and 384 .. 387 (Cb, right column)"""
    c = XL.RING_SMALL
    H, W, T, O = geo(c)
    assert TC.grid(H, W, T, O) == (3, 3)
    sy = CC.sub(fmt)[1]
    row, col, on = XL.ring(H, W, T, O, fmt, XL.rule(fmt, "centre", "linear"), 4)
    assert len(row) == (260 if sy == 2 else 388) and bool(on[:132].all()) is (sy == 2) and bool(on[132:].all())
    where = {(p, XL.ring_index(H, W, T, O, fmt, "centre", "linear", 4, r, q)) for p, r, q in XL.ring_small_witness(fmt)}
    assert where == ({(1, k) for k in range(256, 260)} if sy == 2 else {(1, k) for k in range(384, 388)} | {(2, k) for k in range(256, 260)})
    if fmt == "nv12":
        assert XL.ring_small_witness(fmt) == [(1, r, 128) for r in range(124, 128)]
    for kind in ("smooth", "random"):
        cur, prev = XL.ring_small_pair(fmt, kind)
        for siting, up in RULES:
            want = XL.ring_small_expect(fmt, siting, up)
            assert want[4][:2] == ([0, 4] if up == "linear" else [0, 0]) and want[5] == [0, 4, 0]
            table = CK.tile_changes(cur, prev, fmt, siting, T, O, up)
            assert table == [want.get(t, [0, 0, 0]) for t in range(9)], (kind, siting, up)


@pytest.mark.parametrize("fmt,siting", XL.TAIL_FORMATS + [("nv12", "centre"), ("i422", "centre")])
def test_the_tail_pairs_closed_form_is_the_restatement(fmt, siting):
    """at T = 64 on 100 x 150 and at the table's T; the tile's own samples are its last item block's, the halo sample the ring's"""
    for T, H, W in [(64, 100, 150), tuple(XL.SECOND_TRIP[k] for k in ("T", "H", "W"))]:
        sx, sy = CC.sub(fmt)
        bpt = XL.partials_per_tile(T, fmt) - 1
        for halo, up in itertools.product((True, False), CC.UPSAMPLES):
            cur, prev = XL.tail_pair(fmt, T, H, W, halo)
            want = XL.tail_expect(fmt, siting, up, T, halo)
            assert CK.tile_changes(cur, prev, fmt, siting, T, 0, up, 0, 1) == [want], (T, halo, up)
            d = [a[0] != b[0] for a, b in zip(CC.codes(cur, fmt), CC.codes(prev, fmt))]
            part, active = XL.tile_partials(d, H, W, T, 0, fmt, XL.rule(fmt, siting, up), 0)
            assert active.all() and not part[:bpt - 1].any() and part[bpt - 1].tolist() == [sy * T, T // sx, T // sx]
            assert part[bpt].tolist() == [0, want[1] - T // sx, 0]
        s = XL.tail_halo_sample(fmt, T)
        assert (s is None) == (sx == 1)
        if s is not None and T == 576:
            assert XL.tail_expect(fmt, siting, "linear", T, True)[1] == T // sx + 1
            assert XL.ring_index(H, W, T, 0, fmt, siting, "linear", 0, *s) is not None
        assert {XL.item_block(T, fmt, y, x) for y in range(T - sy, T) for x in (0, T - 1)} == {bpt - 1}


def test_the_largest_tiles_closed_form_is_the_restatement():
    for fmt, siting, linear, nearest in XL.LIMIT_FORMATS:
        for T in (64, 2048):
            H = W = 2 * T + 2
            assert TC.grid(H, W, T, 0) == (3, 3)
            for up in CC.UPSAMPLES:
                assert CK.footprint_sizes(H, W, T, 0, fmt, siting, up)[4] == XL.limit_expect(fmt, siting, up, T)
        assert XL.limit_expect(fmt, siting, "linear") == [XL.LIMIT_LUMA, linear, linear]
        assert XL.limit_expect(fmt, siting, "nearest") == [XL.LIMIT_LUMA, nearest, nearest]
    assert [v[2:] for v in XL.LIMIT_FORMATS] == [(1052676, 1048576), (1050625, 1048576), (2099200, 2097152)]
    # frames that differ in every sample count the footprint: the restatement on data, at a small T
    for fmt, siting, _, _ in XL.LIMIT_FORMATS:
        top = XL.top_of(fmt) - 1
        f0, f1 = XL.CL.const_frame(fmt, 130, 130, 0, 0, 0), XL.CL.const_frame(fmt, 130, 130, top, top, top)
        for up in CC.UPSAMPLES:
            assert CK.tile_changes(f1, f0, fmt, siting, 64, 0, up) == CK.footprint_sizes(130, 130, 64, 0, fmt, siting, up)
        if CC.bits(fmt) == 10:
            f2 = XL.below_the_code(f1, fmt, 10)
            assert any((a != b).any() for a, b in zip(f1, f2)) and CK.tile_changes(f2, f1, fmt, siting, 64, 0, "linear") == [[0, 0, 0]] * 9
    c = XL.CLIP_LIMIT
    assert (c["H"], c["W"], c["T"], c["O"], c["tile"]) == (4098, 4098, 2048, 0, 4)


# -- partial counts and trips --------------------------------------------------------------------------------------------------------

def test_the_rows_of_partials_are_as_long_as_the_cases_say():
    from progressivecodec_amd import chroma_clips
    size = chroma_clips.lib().pc_chroma_clips_changes_workspace_size
    cases = XL.workspace_cases()
    assert {T for T, _, _ in cases} == {128, 576, 1024, 2048} and {sy for _, sy, _ in cases} == {1, 2}
    for T, sy, n in cases:
        assert size(T, sy, n) == 24 * n * (T * T // (2048 * sy) + 1), (T, sy, n)
    for T, p2, p1, t2, t1 in XL.TRIPS:
        assert (XL.partials_per_tile(T, "nv12"), XL.partials_per_tile(T, "p210"), XL.partials_per_tile(T, "i444")) == (p2, p1, p1)
        assert (XL.trips(p2), XL.trips(p1)) == (t2, t1)
        assert size(T, 2, 1) == 24 * p2 and size(T, 1, 1) == 24 * p1
    assert XL.TRIPS == [(576, 82, 163, 2, 3), (1024, 257, 513, 5, 9), (2048, 1025, 2049, 17, 33)]
    assert size(2048, 2, 9) == 24 * 9 * 1025 and size(2048, 1, 9) == 24 * 9 * 2049 and size(2112, 2, 9) == 0 == size(2112, 1, 1)
    for fmt, _, partials, trips in XL.FINAL_1024:
        assert XL.partials_per_tile(1024, fmt) == partials and XL.trips(partials) == trips and (partials - 1) % 64 == 0
    H, W, T = (XL.SECOND_TRIP[k] for k in ("H", "W", "T"))
    assert [TC.grid(H, W, T, O) for O in XL.OVERLAPS] == [(2, 2), (2, 3), (2, 2), (2, 3)]
    assert TC.grid(*geo(XL.FOUR_TRIPS)) == (2, 2)
    # T = 64, where the other tests of the library run: the final's walk and the ring's loop never make a second trip
    assert XL.partials_per_tile(64, "nv12") == 2 and XL.partials_per_tile(64, "p210") == 3
    assert max(len(XL.ring(100, 150, 64, 0, f, (1, 1, 1, 1), 0)[0]) for f in ("nv12", "nv16")) <= 196 < XL.NT


def test_one_ring_sample_at_1024_is_the_only_entry_of_the_finals_last_trip():
    """tile 3 is clipped to 6 x 476: most blocks of its row have no active item; the pair that differs in one ring sample of tile 0
    leaves tile 0's row zero but for its last partial, entry 256 or 512: the only one of the fifth or ninth trip"""
    H, W, T, O = geo(XL.FOUR_TRIPS)
    for fmt, siting, partials, trips in XL.FINAL_1024:
        cur, prev = XL.ring_sample_pair(fmt)
        d = [a[0] != b[0] for a, b in zip(CC.codes(cur, fmt), CC.codes(prev, fmt))]
        assert [int(x.sum()) for x in d] == [0, 1, 0] and any((a != b).sum() > 1 for a, b in zip(cur, prev))
        flags = XL.rule(fmt, siting, "linear")
        part, active = XL.tile_partials(d, H, W, T, O, fmt, flags, 0)
        assert len(part) == partials and active.all() and not part[:-1].any() and part[-1].tolist() == [0, 1, 0]
        assert (partials - 1) // 64 == trips - 1 and (partials - 1) % 64 == 0
        assert XL.ring_index(H, W, T, O, fmt, siting, "linear", 0, *XL.ring_sample_1024(fmt)) is not None
        assert CK.tile_changes(cur, prev, fmt, siting, T, O, "linear")[0] == [0, 1, 0]
        assert CK.tile_changes(cur, prev, fmt, siting, T, O, "nearest")[0] == [0, 0, 0]
        (_, _, hh, ww), _ = XL.tile_geo(H, W, T, O, fmt, 3)
        _, active3 = XL.tile_partials(d, H, W, T, O, fmt, flags, 3)
        assert (hh, ww) == (6, 476) and active3.sum() == -(-(6 // CC.sub(fmt)[1] * 128) // 256) <= 3 and len(active3) == partials - 1 >= 256


# -- the model and its mutants -------------------------------------------------------------------------------------------------------

def host_cases():
    """name -> (cur, prev, fmt, T, O, tiles or None, [(siting, upsample)]): the cases of the table the mutants are run on"""
    out = {}
    for fmt in XL.RING_SMALL_FORMATS:
        out["ring_small %s" % fmt] = XL.ring_small_pair(fmt, "random") + (fmt, 128, 0, None, RULES)
    for (fmt, _, _), side in itertools.product(XL.RING_SIDES_FORMATS, XL.SIDES):
        out["ring_sides %s %s" % (fmt, side)] = XL.ring_side_pair(fmt, side) + (fmt, 576, 0, [4], RULES)
    T, H, W = (XL.SECOND_TRIP[k] for k in ("T", "H", "W"))
    for fmt, siting in XL.TAIL_FORMATS:
        out["tail %s %s" % (fmt, siting)] = XL.tail_pair(fmt, T, H, W, True) + (fmt, T, 0, None, [(siting, "linear"), (siting, "nearest")])
    for fmt, siting, _, _ in XL.FINAL_1024:
        out["ring_sample_1024 %s" % fmt] = XL.ring_sample_pair(fmt) + (fmt, 1024, 0, None, [(siting, "linear")])
    return out


#: mutant -> a case of host_cases() that it is asserted to differ on
KILLED_BY = {
    "final_first_64": "tail nv12 topleft",
    "ring_first_256": "ring_small nv12",
    "swap_lo_hi_y": "ring_sides nv12 above",
    "swap_lo_hi_x": "ring_sides p210 left",
    "swap_sitings": "ring_sides nv12 left",
    "ring_without_corners": "ring_sides nv12 corners",
    "right_column_at_c1c": "ring_small nv16",
    "ring_cb_cr_swapped": "ring_sides p210 right",
    "inactive_block_unwritten": "ring_sample_1024 p010",
}


@pytest.fixture(scope="module")
def verdicts():
    """{case: {mutant or None: whether the model differs from the restatement there}}"""
    out = {}
    for name, (cur, prev, fmt, T, O, tiles, rules) in host_cases().items():
        out[name] = dict.fromkeys([None] + list(XL.MUTANTS), False)
        d, H, W = XL.diff_maps(cur, prev, fmt)
        for siting, up in rules:
            table = CK.tile_changes(cur, prev, fmt, siting, T, O, up)
            want = table if tiles is None else [table[t] for t in tiles]
            for mutant in out[name]:
                out[name][mutant] |= XL.model_counts(d, H, W, fmt, siting, T, O, up, tiles, mutant) != want
    return out


def test_the_layout_model_is_the_restatement_on_every_case(verdicts):
    assert [name for name, v in verdicts.items() if v[None]] == []


def test_no_mutant_survives_the_table(verdicts):
    assert set(KILLED_BY) == set(XL.MUTANTS) and len(XL.MUTANTS) == 9
    survivors = [m for m in XL.MUTANTS if not any(v[m] for v in verdicts.values())]
    assert survivors == []
    assert [m for m, case in KILLED_BY.items() if not verdicts[case][m]] == []


def test_the_mutants_are_silent_at_64():
    """what the issue of this table rests on: at T = 64 the first three of them count as the restatement does"""
    cur, prev = XL.tail_pair("nv12", 64, 100, 150, True)
    for m in ("final_first_64", "ring_first_256"):
        for siting, up in RULES:
            assert XL.model_changes(cur, prev, "nv12", siting, 64, 0, up, None, m) == CK.tile_changes(cur, prev, "nv12", siting, 64, 0, up)


# -- the size cap --------------------------------------------------------------------------------------------------------------------

def test_the_size_cap():
    assert XL.MAX_FRAME == (4098, 4098) and XL.MAX_LIST_AT_2048 == 4
    assert all(H <= XL.MAX_FRAME[0] and W <= XL.MAX_FRAME[1] for H, W in XL.frames_of_the_table())
    c = XL.CUT_LIST_LARGE
    assert c["T"] == 2048 and max(len(c["tiles"]), len(c["raw"])) <= XL.MAX_LIST_AT_2048
    assert (c["H"], c["W"], c["fmt"], c["siting"]) == (4098, 4098, "nv12", "left") and TC.grid(*geo(c)) == (3, 3)
    assert XL.tile_geo(c["H"], c["W"], c["T"], c["O"], c["fmt"], 8)[0][2:] == (2, 2)           # the corner of 2 x 2 pixels
    assert [t for t in c["raw"] if not 0 <= t < 9] == [9, -1]
    assert IL.CLIP_LIMIT["T"] == max(T for T, _, _ in XL.workspace_cases())

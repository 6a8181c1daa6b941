"""tests/image_limits.py without a GPU: the table does what it claims.  Every limit case sits at the largest tile its library admits;
the rows of block partials are as long as the cases need them (derived from the libraries' own workspace-size functions); the
closed forms of the saturated cases are the restatements' values; the sums have the widths the cases are there for; and the
tail-only cases are non-zero through their last two rows alone."""
import numpy as np
import pytest

from tests import clip_tol_contract as TOL
from tests import clip_tol_rate_contract as TRC
from tests import clips_contract as CC
from tests import frame_rate_contract as QC
from tests import frame_tiles_contract as GC
from tests import frames_contract as FC
from tests import image_limits as IL
from tests import pixels_contract as K
from tests import rate_contract as RC
from tests import tiles_contract as TC


def libs():
    from progressivecodec_amd import clip_rate, clip_tol, clip_tol_rate, clips, frame_rate, rate
    return {"rate": rate.lib().pc_rate_workspace_size, "frame_rate": frame_rate.lib().pc_frame_rate_workspace_size,
            "clip_rate": clip_rate.lib().pc_clip_rate_workspace_size, "clips": clips.lib().pc_clips_changes_workspace_size,
            "clip_tol": clip_tol.lib().pc_clip_tol_workspace_size, "clip_tol_rate": clip_tol_rate.lib().pc_clip_tol_rate_workspace_size}


def partials_per_tile(name, T):
    """the block partials of one tile's row, the halo block of the clip libraries included: the workspace of one tile over the bytes
    of one partial (clip_tol's also holds the tile's 4-byte anchor, rounded up to 8).  clip_tol_rate writes a partial per wave, four
    to a block, and its row is an entry's: the figure here is the blocks, as for the others"""
    nbytes = libs()[name](T, 1)
    assert nbytes > 0
    if name == "clip_tol":
        assert (nbytes - 8) % 72 == 0 and nbytes == TOL.workspace_size(T, 1)
        return (nbytes - 8) // 72
    if name == "clip_tol_rate":
        assert nbytes % 96 == 0
        return nbytes // 96
    assert nbytes % 24 == 0
    return nbytes // 24


def test_each_limit_case_sits_at_the_largest_tile_its_library_admits():
    from progressivecodec_amd import clip_rate, clips, frame_rate
    size = libs()
    for name, by_bits in IL.T_MAX.items():
        top = max(by_bits.values())
        assert size[name](top, 1) > 0 and size[name](top + 64, 1) == 0, name                # the function takes no format: the 8-bit limit
    assert IL.RATE_LIMIT["T"] == IL.T_MAX["rate"][8]
    for fmt, c in IL.FRAME_LIMITS.items():
        # per format the limit is the call's own (pc_frame_rate_tile_sse, pc_clip_rate_sse_jobs refuse T + 64: the GPU test makes the
        # call); here what the modules and the restatement say it is
        assert c["T"] == IL.T_MAX["frame_rate"][FC.bits(fmt)] == IL.T_MAX["clip_rate"][FC.bits(fmt)]
        assert c["T"] == QC.max_tile(fmt) == frame_rate.max_tile(fmt) == clip_rate.max_tile(fmt)
        assert c["T"] ** 4 * IL.top_code(fmt) ** 2 < 2 ** 60 <= (2 * c["T"]) ** 4 * IL.top_code(fmt) ** 2
        assert TC.grid(c["H"], c["W"], c["T"], c["O"]) == (3, 3) and c["O"] == c["T"] // 2
    assert IL.CLIP_LIMIT["T"] == IL.T_MAX["clips"][8] == IL.T_MAX["clips"][10] == IL.T_MAX["clip_tol"][10] == clips.MAX_TILE
    assert TC.grid(*(IL.CLIP_LIMIT[k] for k in "HWTO")) == (3, 3) and TC.grid(*(IL.RATE_LIMIT[k] for k in "HWTO")) == (3, 3)
    assert TC.grid(*(IL.RATE_CLIPPED[k] for k in "HWTO")) == (2, 3) and IL.RATE_CLIPPED["H"] % 8 and IL.RATE_CLIPPED["W"] % 8
    # the limit cases' rows of partials are the longest there are: 1024 (and the halo block)
    assert partials_per_tile("rate", 2048) == partials_per_tile("frame_rate", 2048) == 1024
    assert partials_per_tile("clips", 2048) == partials_per_tile("clip_tol", 2048) == 1025 and partials_per_tile("clip_rate", 1024) == 256


def test_the_rows_of_partials_are_as_long_as_the_cases_need():
    """B: more than 64 per tile in every case (a second trip of the wave that gathers them), 256 or 257 in the four-trip case; C: more
    than 256 per picture (a second trip of the block that gathers them)"""
    from progressivecodec_amd import frame_tiles, frames, pixels, tiles
    for name in IL.T_MAX:
        extra = 1 if name in ("clips", "clip_tol") else 0
        assert partials_per_tile(name, IL.SECOND_TRIP["T"]) == 81 + extra
        assert partials_per_tile(name, IL.FOUR_TRIPS["T"]) == 256 + extra > 3 * 64
        assert partials_per_tile(name, 512) == 64 + extra                                   # the tile size before: one trip (and a lane)
    H, W, B = IL.WHOLE["H"], IL.WHOLE["W"], IL.WHOLE["B"]
    per_picture = {"pixels": pixels.lib().pc_pixels_emit_workspace_size(B, H, W) // 48 // B,
                   "frames": frames.lib().pc_frames_emit_workspace_size(B, H, W) // 24 // B,
                   "tiles": tiles.lib().pc_tiles_stitch_workspace_size(0, H, W) // 48,
                   "frame_tiles": frame_tiles.lib().pc_frame_tiles_stitch_workspace_size(0, H, W) // 24}
    assert all(256 < v <= 512 for v in per_picture.values()), per_picture
    assert H * W > 2 ** 20 and TC.grid(H, W, IL.WHOLE["T"], IL.WHOLE["O"]) == (2, 2)
    for O, _ in IL.SECOND_TRIP_OVERLAPS:
        ny, nx = TC.grid(IL.SECOND_TRIP["H"], IL.SECOND_TRIP["W"], IL.SECOND_TRIP["T"], O)
        assert ny == 2 and nx in (2, 3)
    assert TC.grid(*(IL.FOUR_TRIPS[k] for k in "HWTO")) == (2, 2)


@pytest.mark.parametrize("mirror", [False, True])
def test_rate_closed_form_is_the_restatement(mirror):
    c = IL.RATE_LIMIT
    x, ref, e = IL.rate_saturated(mirror)
    closed = IL.rate_closed(c, e)
    assert closed == 285982974384537600 == 65025 * (2 ** 21) ** 2 and 2 ** 54 <= closed < 2 ** 60
    rounding = "trunc" if mirror else "nearest"
    assert RC.tile_sse(x, c["H"], c["W"], c["T"], c["O"], rounding, ref, "chw", first_tile=c["tile"]) == [[closed] * 3]
    assert IL.axis_weight_sum(1, 3, c["T"], c["O"]) == int(RC.weights_int(1, 3, c["T"], c["O"]).sum()) == 2 ** 21
    assert IL.axis_weight_sum(0, 3, c["T"], c["O"]) == int(RC.weights_int(0, 3, c["T"], c["O"]).sum())


@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_frame_rate_closed_forms_are_the_restatement(fmt):
    c = IL.FRAME_LIMITS[fmt]
    table = {"nv12": [285982974384537600, 2 ** 54, 2 ** 54], "i420": [285982974384537600, 2 ** 54, 2 ** 54],
             "p010": [287667701076197376, 2 ** 54, 2 ** 54]}
    for mirror in (False, True):
        v, frame, eY, eC = IL.frame_saturated(fmt, mirror)
        closed = IL.frame_rate_closed(c, eY, eC)
        x = IL.const_tile(c["T"], v)
        assert QC.tile_sse(x, c["H"], c["W"], c["T"], c["O"], fmt, "bt709", "full", frame, first_tile=c["tile"]) == [closed], (fmt, mirror)
        if not mirror:
            assert closed == table[fmt] and all(2 ** 54 <= s < 2 ** 60 for s in closed)
        else:
            # the luma sum is the table's; the chroma error is top - co = 2^(n-1) - 1, so those sums end just below 2^54
            assert closed[0] == table[fmt][0] and all(2 ** 53 <= s < 2 ** 54 for s in closed[1:])
    # the corner tile of the clip_rate jobs
    corner = dict(c, tile=0)
    v, frame, eY, eC = IL.frame_saturated(fmt, False)
    assert QC.tile_sse(IL.const_tile(c["T"], v), c["H"], c["W"], c["T"], c["O"], fmt, "bt709", "full", frame) == [IL.frame_rate_closed(corner, eY, eC)]
    assert {t for _, t in IL.LIMIT_JOBS} == {0, 4} and {f for f, _ in IL.LIMIT_JOBS} == {0, 1} and len(set(IL.LIMIT_JOBS)) < len(IL.LIMIT_JOBS)


@pytest.mark.parametrize("fmt", IL.CLIP_FORMATS)
def test_clip_limit_closed_forms_are_the_restatements(fmt):
    c = IL.CLIP_LIMIT
    H, W, T, O, t = (c[k] for k in ("H", "W", "T", "O", "tile"))
    f0, f1, f2 = IL.clip_limit_frames(fmt)
    top = IL.top_code(fmt)
    for up in FC.UPSAMPLES:
        counts = CC.tile_changes(f1, f0, fmt, T, O, up)
        assert counts[t] == IL.footprint_sizes(c, up) == TOL.nsamp(t, H, W, T, O, up)
        assert all(row == TOL.nsamp(k, H, W, T, O, up) for k, row in enumerate(counts))
        assert CC.tile_changes(f2, f1, fmt, T, O, up) == [[0, 0, 0]] * 9 == CC.tile_changes(f0, f0, fmt, T, O, up)
    assert IL.footprint_sizes(c, "linear") == [4194304, 1052676, 1052676]
    assert any((a != b).any() for a, b in zip(f1, f2)) == (fmt == "p010")
    ns = [TOL.nsamp(k, H, W, T, O, "linear") for k in range(9)]
    stats1 = [[[n, n * top * top, top] for n in row] for row in ns]
    zeros = [[[0, 0, 0]] * 3] * 9
    if fmt == "p010":
        assert stats1[t][0][1] == 4389460770816
    for max_abs, q10, max_run, reused in IL.boundary_tolerances(fmt):
        source, stats = TOL.scan([f0, f1, f2], fmt, T, O, "linear", max_abs, q10, max_run)
        if reused:
            assert source == [[0] * 9] * 3 and stats == [zeros, stats1, stats1]
        else:                                                              # step 2 compares against the anchor step 1 moved
            assert source == [[0] * 9, [1] * 9, [1] * 9] and stats == [zeros, stats1, zeros]


def test_whole_picture_saturated_sums_do_not_fit_32_bits():
    for peak in (255, 1023):
        s = IL.whole_saturated_sum(peak)
        assert s > 2 ** 32 and s % 2 ** 32 != s and s < 2 ** 63
    H, W = IL.WHOLE["H"], IL.WHOLE["W"]
    Hc, Wc = FC.chroma_size(H, W)
    assert IL.whole_saturated_sum(255) == 65025 * 1026 * 1030
    assert 128 * 128 * Hc * Wc > 2 ** 32 and 512 * 512 * Hc * Wc > 2 ** 32                  # the chroma sums of the same pair, too
    # closed form against the restatements on the saturated pair: zero planes against the top code
    hp, wp, top, left = K.geometry(H, W)
    x = np.zeros((1, 3, hp, wp), np.float32)
    su, sf = K.sums(x, top, left, H, W, "nearest", np.full((1, 3, H, W), 255, np.uint8), "chw")
    assert su == [[IL.whole_saturated_sum(255)] * 3] and sf == [[float(H * W)] * 3]
    for fmt in ("nv12", "p010"):
        _, _, co, _, mx = FC.levels(fmt, "full")
        ref = IL.const_frame(fmt, H, W, mx, 0, 0)
        assert FC.sums(x, top, left, H, W, fmt, "bt709", "full", ref) == [[IL.whole_saturated_sum(mx), co * co * Hc * Wc, co * co * Hc * Wc]]


def test_tail_only_cases_are_non_zero_through_their_last_two_rows_alone():
    T, H, W = (IL.SECOND_TRIP[k] for k in ("T", "H", "W"))
    tail, eq, ref = IL.rate_tail(T, H, W)
    assert np.array_equal(tail[:, :, :T - 2].view(np.uint32), eq[:, :, :T - 2].view(np.uint32))
    got = RC.tile_sse(tail, H, W, T, 0, "nearest", ref, "chw")
    assert all(v > 0 for v in got[0]) and RC.tile_sse(eq, H, W, T, 0, "nearest", ref, "chw") == [[0, 0, 0]]
    for fmt in FC.FORMATS:
        tail, eq, frame = IL.frame_tail(fmt, T, H, W)
        assert np.array_equal(tail[:, :, :T - 2].view(np.uint32), eq[:, :, :T - 2].view(np.uint32))
        got = QC.tile_sse(tail, H, W, T, 0, fmt, "bt709", "limited", frame)
        assert all(v > 0 for v in got[0]) and QC.tile_sse(eq, H, W, T, 0, fmt, "bt709", "limited", frame) == [[0, 0, 0]], fmt
        cur, prev = IL.clip_tail(fmt, T, H, W)
        inner, _ = IL.clip_tail(fmt, T, H, W, halo=False)
        want = CC.tile_changes(cur, prev, fmt, T, 0, "linear", 0, 1)
        assert want == [[2 * T, T // 2 + 1, T // 2]]                                        # the last row pair, the last chroma row, the halo's Cb
        assert CC.tile_changes(inner, prev, fmt, T, 0, "linear", 0, 1) == CC.tile_changes(cur, prev, fmt, T, 0, "nearest", 0, 1) == [[2 * T, T // 2, T // 2]]
        assert CC.tile_changes(prev, prev, fmt, T, 0, "linear", 0, 1) == [[0, 0, 0]]
        # before the last two rows and outside the halo nothing changed
        a, b = FC.codes(cur, fmt), FC.codes(prev, fmt)
        assert not (a[0][0, :T - 2] != b[0][0, :T - 2]).any() and not (a[1][0, :T // 2 - 1] != b[1][0, :T // 2 - 1]).any()
        stats = TOL.scan([prev, cur], fmt, T, 0, "linear")[1][1][0]
        assert [s[0] for s in stats] == want[0] and all(s[1] > 0 and s[2] > 0 for s in stats)


def test_whole_picture_tail_pairs_are_non_zero_through_the_last_two_rows_alone():
    H, W, B, T, O = (IL.WHOLE[k] for k in ("H", "W", "B", "T", "O"))
    hp, wp, top, left = K.geometry(H, W)
    eq = K.hostile_planes(IL.byte_image(H, W, 1)[None].repeat(B, 0), hp, wp, top, left, seed=2)
    tail = np.array(eq)
    tail[B - 1, :, top + H - 2:top + H] = IL.flip(eq[B - 1, :, top + H - 2:top + H])
    ref = K.emit(eq, top, left, H, W, "nearest", "chw")
    su, sf = K.sums(tail, top, left, H, W, "nearest", ref, "chw")
    assert su[0] == [0, 0, 0] and all(v > 0 for v in su[1]) and K.sums(eq, top, left, H, W, "nearest", ref, "chw")[0] == [[0, 0, 0]] * B
    fref = FC.emit(eq, top, left, H, W, "nv12", "bt709", "limited")
    fs = FC.sums(tail, top, left, H, W, "nv12", "bt709", "limited", fref)
    assert fs[0] == [0, 0, 0] and all(v > 0 for v in fs[1]) and FC.sums(eq, top, left, H, W, "nv12", "bt709", "limited", fref) == [[0, 0, 0]] * B
    ny, nx = TC.grid(H, W, T, O)
    xe = TC.hostile_tiles(ny * nx, T, seed=3)
    xt = IL.stitch_tail(xe, T, O, H, W)
    assert IL.rows_kept(T, O, H) == {0: [], 1: [H - 2 - (T - O), H - 1 - (T - O)]}
    assert np.array_equal(xt[:nx].view(np.uint32), xe[:nx].view(np.uint32)) and not np.array_equal(xt[nx:].view(np.uint32), xe[nx:].view(np.uint32))
    img = TC.stitch(xe, H, W, T, O, "nearest", "chw")
    assert all(v > 0 for v in TC.sums(xt, H, W, T, O, "nearest", img, "chw")[0]) and TC.sums(xe, H, W, T, O, "nearest", img, "chw")[0] == [0, 0, 0]
    assert not (TC.stitch(xt, H, W, T, O, "nearest", "chw")[:, :H - 2] != img[:, :H - 2]).any()
    fr = GC.stitch(xe, H, W, T, O, "p010", "bt709", "limited")
    assert all(v > 0 for v in GC.sums(xt, H, W, T, O, "p010", "bt709", "limited", fr)) and GC.sums(xe, H, W, T, O, "p010", "bt709", "limited", fr) == [0, 0, 0]


# -- clip_tol_rate ---------------------------------------------------------------------------------------------------------------------

def test_clip_tol_rate_limits_and_the_trips_of_its_final():
    """the per-format limit is the module's and the restatement's; an entry's row of WAVE partials is 4096 long at T = 2048 (64 trips
    of the final's 64 lanes), 1024 at T = 1024 (16), 324 at T = 576 (six, the last partial); and the workspace of every case of the
    table is 96 (T^2 / 4096) n_entries"""
    from progressivecodec_amd import clip_tol_rate
    size = libs()["clip_tol_rate"]
    for fmt, c in IL.FRAME_LIMITS.items():
        assert c["T"] == IL.T_MAX["clip_tol_rate"][FC.bits(fmt)] == QC.max_tile(fmt) == clip_tol_rate.max_tile(fmt)
    waves = lambda T: size(T, 1) // 24                                                     # noqa: E731
    assert (waves(2048), waves(1024), waves(576), waves(64)) == (4096, 1024, 324, 4)
    assert (-(-waves(2048) // 64), -(-waves(1024) // 64), -(-waves(576) // 64)) == (64, 16, 6) and waves(576) % 64 == 4
    cases = IL.run_workspace_cases()
    assert len(cases) == 3 + 10 + 2 and (64, 300) in cases
    for T, ne in cases:
        assert size(T, ne) == 96 * (T * T // 4096) * ne == TRC.workspace_size(T, ne), (T, ne)
    assert max(size(T, ne) for T, ne in cases) < 1 << 20


@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_clip_tol_rate_closed_forms_are_the_restatement(fmt):
    """A: every row of the three jobs is frame_rate_closed of its (tile value, frame) pair and run_sse's row; the jobs reach both
    frames from both tile values, a frame twice in one run and the corner tile"""
    c = IL.FRAME_LIMITS[fmt]
    frames, vals, tile_ids, runs, want = IL.run_limit_case(fmt)
    x = np.concatenate([IL.const_tile(c["T"], v) for v in vals])
    assert TRC.run_sse(x, frames, tile_ids, runs, c["H"], c["W"], c["T"], c["O"], fmt, "bt709", "full") == want
    assert len(want) == 6 and want[0] == want[2] != want[1] and want[5] != want[0]
    for (v, mirror), closed in {(0.0, False): want[0], (1.0, True): want[3]}.items():            # the pairs frame_rate's case has
        _, _, eY, eC = IL.frame_saturated(fmt, mirror)
        assert IL.saturated_errors(fmt, v, mirror) == (eY, eC) and closed == IL.frame_rate_closed(c, eY, eC)
    # the other two pairs leave luma equal: the whole sum is chroma's
    assert want[1][0] == want[4][0] == 0 and min(want[1][1:] + want[4][1:]) >= 2 ** 53
    assert all(s < 2 ** 60 for row in want for s in row) and max(want[0]) >= 2 ** 54
    assert all((a == b).all() for a, b in zip(frames[0], frames[2])) and any((a != b).any() for a, b in zip(frames[0], frames[1]))


def test_clip_tol_rate_run_lists_are_what_the_cases_need():
    for n in (4, 6):
        tile_ids, runs = IL.run_list(n)
        assert {s for r in runs for s in r} == {0, 1} and any(len(set(r)) < len(r) for r in runs) and runs[0][0] > runs[0][1]
        assert tile_ids[1] == tile_ids[3] and runs[1] != runs[3] and {0, n - 1} <= set(tile_ids)
    cases = IL.run_trip_cases()
    assert len(cases) == 10 and {(c[3], c[5]) for c in cases[:9]} == {(O, f) for O, _ in IL.SECOND_TRIP_OVERLAPS for f in FC.FORMATS}
    assert cases[-1] == (1024, 1030, 1500, 0, True, "p010") and 3 in IL.run_list(4)[0]          # tile 3, clipped to 6 x 476
    c = IL.LONG_RUNS
    tile_ids, runs = IL.long_runs()
    assert TC.grid(c["H"], c["W"], c["T"], c["O"]) == (2, 3) and c["O"] % 8 == 0 and all(0 <= t < 6 for t in tile_ids)
    assert [len(r) for r in runs] == [70, 1, 2, 33, 64, 130] and TRC.offsets_of(runs)[-1] == 300 and len(tile_ids) == 6
    for r in runs:
        assert set(r) <= {0, 1, 2} and (len(r) < 3 or set(r) == {0, 1, 2})
        assert len(r) < 5 or any(a == b for a, b in zip(r, r[1:]))                              # a frame twice in a row
    # past the 64th entry a run names other frames than at its start: a loop that ran out of entries of its own would show
    assert all(any(r[j] != r[0] for j in range(64, len(r))) for r in runs if len(r) > 64) and sum(len(r) > 64 for r in runs) == 2


@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_clip_tol_rate_tail_only_comes_from_the_last_row_pair_alone(fmt):
    T, H, W = (IL.SECOND_TRIP[k] for k in ("T", "H", "W"))
    tail, eq, frame = IL.frame_tail(fmt, T, H, W)
    assert np.array_equal(tail[:, :, :T - 2].view(np.uint32), eq[:, :, :T - 2].view(np.uint32))
    x = np.concatenate([tail, eq])
    got = TRC.run_sse(x, [frame], [0, 0], [[0, 0], [0, 0]], H, W, T, 0, fmt, "bt709", "limited")
    want = QC.tile_sse(tail, H, W, T, 0, fmt, "bt709", "limited", frame)[0]
    assert got == [want, want, [0, 0, 0], [0, 0, 0]] and all(v > 0 for v in want)
    # the same value from the last row pair on its own: the tile of T rows whose first T - 2 are the equal tile's, so that every
    # item above the last row pair adds nothing -- of an entry's 324 wave partials only the last block's are non-zero
    y, cb, cr = QC.tile_codes(tail[0], T, T, fmt, "bt709", "limited")
    ey, ecb, ecr = QC.tile_codes(eq[0], T, T, fmt, "bt709", "limited")
    assert (y[:T - 2] == ey[:T - 2]).all() and (cb[:T // 2 - 1] == ecb[:T // 2 - 1]).all() and (cr[:T // 2 - 1] == ecr[:T // 2 - 1]).all()
    assert want == [int(((y[T - 2:] - ey[T - 2:]) ** 2).sum()), int(((cb[-1] - ecb[-1]) ** 2).sum()), int(((cr[-1] - ecr[-1]) ** 2).sum())]

"""chroma_clips (libpc_chroma_clips.so) on the GPU past T = 64 (tests/chroma_clips_limits.py holds the table; DESIGN.md section 19.1 the
limits): the halo ring's loop making its second to seventh trip, every side of the ring alone; final_kernel's later trips over rows
of 82 and 163 (T = 576), 257 and 513 (T = 1024), 1025 and 2049 (T = 2048) block partials, on frames that differ everywhere, sparsely,
in a tile's last rows alone and in one ring sample alone; blocks without an active item; and cut_list_kernel at T = 576 and T = 2048.
Every comparison is exact equality of integers or float bits against the restatements (tests/chroma_clips_contract.py,
tests/chroma_tiles_contract.cut); the closed forms are the table's, which tests/test_chroma_clips_limits_host.py holds to the
restatement, and which it shows to tell nine subtly wrong kernels from the right one.  Every raw call asserts its status, that every
partial of its workspace and no word after them was written, and the access path pc_chroma_clips_plan reports."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import chroma_clips_cases as CS
from tests import chroma_clips_contract as CK
from tests import chroma_clips_limits as XL
from tests import chroma_contract as CC
from tests import chroma_tiles_contract as KT
from tests import image_limits as IL
from tests import tiles_contract as TC
from tests.test_gpu_chroma_clips import KC, PAIR, bits, changes_raw, float_buffer, frame_pair, guards_kept, stream, views
from tests.test_gpu_chroma_tiles import on_device
from tests.test_gpu_frames import POISON64
from tests.test_gpu_image_limits import need_memory
from tests.test_gpu_rate import check_out

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RULES = list(itertools.product(CC.SITINGS, CC.UPSAMPLES))
#: frame_pair's seed per tile size: every tile's three "few" counts differ from every other tile's, at every overlap and upsampling
FEW_SEED = {576: 576, 1024: 1024}


def ids(v):
    return "-".join(str(a) for a in v) if isinstance(v, tuple) else str(v)


def geo(c):
    return tuple(c[k] for k in ("H", "W", "T", "O"))


def device_pair(fmt, H, W, cur, prev, aligned):
    """the two frames as views: both aligned but pitched differently, or cur one element past an allocation start with loose rows"""
    (cm, co), (pm, po) = PAIR[aligned]
    return views(fmt, H, W, cm, co, cur), views(fmt, H, W, pm, po, prev)


def check_changes(cv, pv, fmt, siting, up, H, W, T, O, aligned, ranges, want, note):
    """raw calls over the (first, count) ranges against want, the table of the whole grid -> the access path"""
    kc = KC()
    wide = kc.plan(kc.CHANGES, cv, fmt, other=pv, overlap=O)
    assert wide is CS.wide(CS.Case(fmt, siting, up, H, W, O, 0, None, None), aligned), (note, aligned)
    for first, m in ranges:
        rc, buf, ws_ok = changes_raw(cv, pv, fmt, siting, up, H, W, O, first, m, size=T)
        assert rc == 0 and ws_ok, (note, siting, up, aligned, first, m)
        check_out(buf, want[first:first + m], (note, siting, up, aligned, first, m))
    return wide


# -- the halo ring -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["smooth", "random"])
@pytest.mark.parametrize("fmt", XL.RING_SMALL_FORMATS)
def test_ring_second_trip_at_its_smallest_size(fmt, kind):
    """T = 128, tile 4 of 300 x 300: the frames differ in the samples the ring's loop reaches from index 256 on (nv12: four Cb samples
    of the right column, the loop's last four; nv16: the last four of the left column in Cr and of the right column in Cb).  Tile 4
    counts them under the rules that have that side, tile 5 (and 3) as its own samples"""
    H, W, T, O = geo(XL.RING_SMALL)
    cur, prev = XL.ring_small_pair(fmt, kind)
    for aligned in CS.ALIGNMENTS:
        cv, pv = device_pair(fmt, H, W, cur, prev, aligned)
        for siting, up in RULES:
            want = CK.tile_changes(cur, prev, fmt, siting, T, O, up)
            expect = XL.ring_small_expect(fmt, siting, up)
            assert want == [expect.get(t, [0, 0, 0]) for t in range(9)] and want[4][1] == (4 if up == "linear" else 0)
            check_changes(cv, pv, fmt, siting, up, H, W, T, O, aligned, [(0, 9), (4, 1), (5, 1)], want, (fmt, kind))


@pytest.mark.parametrize("side", XL.SIDES)
@pytest.mark.parametrize("fmt", [f for f, _, _ in XL.RING_SIDES_FORMATS])
def test_each_ring_side_alone(fmt, side):
    """T = 576, tile 4 of 1300 x 1300: the frames differ in one side of tile 4's ring alone -- the complete chroma row above or below
    its rectangle, the column left or right of it, corners included, or the four corners -- in Cb everywhere and in Cr in fewer
    samples; the loop covers up to 1156 (nv12) and 1732 (p210) indices.  Side length or 0 per lo / hi, under every rule"""
    H, W, T, O = geo(XL.RING_SIDES)
    cur, prev = XL.ring_side_pair(fmt, side)
    for aligned in CS.ALIGNMENTS:
        cv, pv = device_pair(fmt, H, W, cur, prev, aligned)
        for siting, up in RULES:
            want = CK.tile_changes(cur, prev, fmt, siting, T, O, up)
            assert want[4] == XL.ring_side_expect(fmt, siting, up, side), (side, siting, up)
            check_changes(cv, pv, fmt, siting, up, H, W, T, O, aligned, [(0, 9), (4, 1)], want, (fmt, side))


# -- the final's later trips ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("O", XL.OVERLAPS)
@pytest.mark.parametrize("fs", XL.FORMATS, ids=ids)
def test_final_later_trips_at_576(fs, O):
    """601 x 1101 in 576-tiles: 82 block partials per tile at 4:2:0, 163 at 4:2:2 and 4:4:4, a second and a third trip of the final's
    64 lanes; frames that differ in a few hundred samples (every tile's counts differ from every other's) and in every sample (the
    counts are the footprint's sizes); the whole grid, a sub-range and every tile alone, both upsamplers, and the Python call"""
    kc = KC()
    fmt, siting = fs
    T, H, W = (XL.SECOND_TRIP[k] for k in ("T", "H", "W"))
    n = int(np.prod(TC.grid(H, W, T, O)))
    ranges = [(0, n), IL.sub_range(n)] + [(t, 1) for t in range(n)]
    seen = set()
    for kind in ("few", "all"):
        cur, prev = frame_pair(fmt, H, W, kind, FEW_SEED[T])
        want = {up: CK.tile_changes(cur, prev, fmt, siting, T, O, up) for up in CC.UPSAMPLES}
        for up in CC.UPSAMPLES:
            if kind == "few":
                assert XL.all_differ(want[up]), (fs, O, up)
            else:
                assert want[up] == CK.footprint_sizes(H, W, T, O, fmt, siting, up)
        for aligned in CS.ALIGNMENTS:
            cv, pv = device_pair(fmt, H, W, cur, prev, aligned)
            for up in CC.UPSAMPLES:
                seen.add(check_changes(cv, pv, fmt, siting, up, H, W, T, O, aligned, ranges, want[up], (fs, O, kind)))
        for up in CC.UPSAMPLES:
            got = kc.tile_changes(on_device(cur), on_device(prev), fmt, siting, T, O, up)
            assert got.dtype == torch.int64 and got.shape == (n, 3) and got.tolist() == want[up], (fs, O, kind, up)
    assert seen == ({False, True} if CC.sub(fmt)[0] == 1 or O % 8 == 0 else {False})


@pytest.mark.parametrize("fsp", XL.FINAL_1024, ids=ids)
def test_final_five_and_nine_trips_at_1024(fsp):
    """T = 1024, O = 0 on 1030 x 1500: 257 partials per tile in p010, 513 in p210; tile 3 is clipped to 6 x 476, so that most blocks
    of its row hold no active item and still write their zeros.  In the third pair one Cb sample of tile 0's ring differs and nothing
    else: the only non-zero partial of tile 0's row is the single entry of the final's fifth, or ninth, trip"""
    need_memory(300 << 20)
    fmt, siting, partials, trips = fsp
    H, W, T, O = geo(XL.FOUR_TRIPS)
    assert XL.partials_per_tile(T, fmt) == partials and XL.trips(partials) == trips
    pairs = [("few", frame_pair(fmt, H, W, "few", FEW_SEED[T])), ("all", frame_pair(fmt, H, W, "all", FEW_SEED[T])), ("ring", XL.ring_sample_pair(fmt))]
    for kind, (cur, prev) in pairs:
        want = {up: CK.tile_changes(cur, prev, fmt, siting, T, O, up) for up in CC.UPSAMPLES}
        if kind == "ring":
            assert want["linear"][0] == [0, 1, 0] and want["nearest"][0] == [0, 0, 0]
        elif kind == "few":
            assert XL.all_differ(want["linear"]) and XL.all_differ(want["nearest"])
        else:
            assert all(want[up] == CK.footprint_sizes(H, W, T, O, fmt, siting, up) for up in CC.UPSAMPLES)
        for aligned in CS.ALIGNMENTS:
            cv, pv = device_pair(fmt, H, W, cur, prev, aligned)
            for up in CC.UPSAMPLES:
                wide = check_changes(cv, pv, fmt, siting, up, H, W, T, O, aligned, [(0, 4), (3, 1), (1, 2), (0, 1)], want[up], (fsp, kind))
                assert wide is aligned


@pytest.mark.parametrize("fs", XL.TAIL_FORMATS, ids=ids)
def test_tail_only(fs):
    """T = 576, tile 0 of 601 x 1101: the frames differ in the tile's last sy luma rows and last chroma row and, with the halo, in one
    Cb sample of the ring where the rule has that side (the row below at 4:2:0, the column right at 4:2:2): of the row of 82 or 163
    partials only the last item block's and the ring's are non-zero.  The counts in closed form; equal frames, and at 10 bits frames
    that differ outside the code alone, count nothing"""
    fmt, siting = fs
    T, H, W = (XL.SECOND_TRIP[k] for k in ("T", "H", "W"))
    halo, prev = XL.tail_pair(fmt, T, H, W, True)
    inner, _ = XL.tail_pair(fmt, T, H, W, False)
    outside = XL.below_the_code(prev, fmt, 5) if CC.bits(fmt) == 10 else None
    for aligned in CS.ALIGNMENTS:
        pv = device_pair(fmt, H, W, prev, prev, aligned)[1]
        for name, cur in (("halo", halo), ("inner", inner), ("equal", prev), ("outside", outside)):
            if cur is None:
                continue
            cv = device_pair(fmt, H, W, cur, prev, aligned)[0]
            for up in CC.UPSAMPLES:
                want = CK.tile_changes(cur, prev, fmt, siting, T, 0, up)
                if name in ("halo", "inner"):
                    assert want[0] == XL.tail_expect(fmt, siting, up, T, name == "halo"), (fs, name, up)
                else:
                    assert want == [[0, 0, 0]] * 4 and (name == "equal" or any((a != b).any() for a, b in zip(cur, prev)))
                check_changes(cv, pv, fmt, siting, up, H, W, T, 0, aligned, [(0, 4), (0, 1)], want, (fs, name))


@pytest.mark.parametrize("aligned", CS.ALIGNMENTS)
@pytest.mark.parametrize("fsc", XL.LIMIT_FORMATS, ids=ids)
def test_largest_tile_counts_its_whole_footprint(fsc, aligned):
    """T = 2048, O = 0 on 4098 x 4098, rows of 1025 and 2049 partials: all codes 0 against all codes at the top count every tile's
    footprint -- tile 4's is 4 194 304 luma samples and 1026^2, 1025^2 or 2048 * 1025 chroma samples under linear, 1024^2 or
    2048 * 1024 under nearest upsampling; equal frames and, for p210, frames that differ below the code count nothing.  The grid of
    nine and tile 4 alone; the Python call returns the numbers as int64; T = 2112 is refused, having launched nothing"""
    need_memory(500 << 20)
    kc = KC()
    fmt, siting, linear, nearest = fsc
    H, W, T, O = geo(XL.CLIP_LIMIT)
    t = XL.CLIP_LIMIT["tile"]
    f0, f1, f2 = XL.limit_frames(fmt)
    v1, v0 = device_pair(fmt, H, W, f1, f0, aligned)
    v2 = device_pair(fmt, H, W, f2, f0, aligned)[0] if f2 is not None else None
    for up, chroma in (("linear", linear), ("nearest", nearest)):
        want = CK.footprint_sizes(H, W, T, O, fmt, siting, up)
        assert want[t] == XL.limit_expect(fmt, siting, up) == [XL.LIMIT_LUMA, chroma, chroma]
        assert check_changes(v1, v0, fmt, siting, up, H, W, T, O, aligned, [(0, 9), (t, 1)], want, (fsc, "all")) is aligned
        check_changes(v0, v0, fmt, siting, up, H, W, T, O, True, [(0, 9)], [[0, 0, 0]] * 9, (fsc, "equal"))
        if v2 is not None:
            check_changes(v2, v1, fmt, siting, up, H, W, T, O, aligned, [(0, 9), (t, 1)], [[0, 0, 0]] * 9, (fsc, "below the code"))
    if aligned:
        got = kc.tile_changes(tuple(p[0] for p in v1), tuple(p[0] for p in v0), fmt, siting, T, O, "linear", first_tile=t, n_tiles=1)
        assert got.dtype == torch.int64 and got.tolist() == [[XL.LIMIT_LUMA, linear, linear]]
        sy = CC.sub(fmt)[1]
        L = kc.lib()
        assert L.pc_chroma_clips_changes_workspace_size(T, sy, 9) == 24 * 9 * (1025 if sy == 2 else 2049)
        assert L.pc_chroma_clips_changes_workspace_size(T + 64, sy, 9) == 0
        rc, buf, ws_ok = changes_raw(v1, v0, fmt, siting, "linear", H, W, O, 0, 9, size=T + 64)
        assert rc == -1 and ws_ok and (buf == POISON64).all()


# -- the cut of a list ---------------------------------------------------------------------------------------------------------------

def device_cuts(planes, fmt, matrix, rng, up, siting, T, O, nx, tiles):
    """chroma_tiles.cut_frame of each tile's rectangle"""
    from progressivecodec_amd import chroma_tiles
    return {t: chroma_tiles.cut_frame(planes, fmt, matrix, rng, up, siting, T, O, rect=(t // nx, t % nx, 1, 1))[0][0] for t in tiles}


def same(t, want_np):
    return torch.equal(bits(t), torch.from_numpy(np.ascontiguousarray(want_np).view(np.int32)).to(DEV))


@pytest.mark.parametrize("O", XL.OVERLAPS)
@pytest.mark.parametrize("fs", XL.FORMATS, ids=ids)
def test_cut_list_at_576(fs, O):
    """601 x 1101 in 576-tiles, tile_items = 41472: a scattered list with repeats and the reversed list, from aligned planes into a
    16-byte-aligned destination (wide where O is a multiple of 8, or at 4:4:4) and from offset, loose planes into a destination one
    float past alignment (narrow), guards kept; bit for bit the restatement's cut and chroma_tiles.cut_frame of each rectangle"""
    kc = KC()
    fmt, siting = fs
    T, H, W = (XL.SECOND_TRIP[k] for k in ("T", "H", "W"))
    ny, nx = TC.grid(H, W, T, O)
    n = ny * nx
    matrix, rng = XL.CL.settings(O // 4 + len(fmt))
    f = CC.random_frame(1, H, W, fmt, seed=O + 2, garbage=True)
    planes = on_device(f)
    seen = set()
    for up in CC.UPSAMPLES:
        want_np = KT.cut(f, fmt, matrix, rng, up, siting, T, O)
        each = device_cuts(planes, fmt, matrix, rng, up, siting, T, O, nx, range(n))
        want = torch.stack([each[t] for t in range(n)])
        assert same(want, want_np), (fs, O, up)
        for aligned in CS.ALIGNMENTS:
            (mode, off), _ = PAIR[aligned]
            src = views(fmt, H, W, mode, off, f)
            foff = 4 if aligned else 5
            for idx in XL.cut_lists(n, H + O):
                store, dst = float_buffer(len(idx) * 3 * T * T, foff)
                dst = dst.view(len(idx), 3, T, T)
                wide = kc.plan(kc.CUT, src, fmt, f32=dst, overlap=O)
                assert wide is CS.wide(CS.Case(fmt, siting, up, H, W, O, 0, matrix, rng), aligned), (fs, O, aligned)
                seen.add(wide)
                got = kc.cut_tiles(tuple(v[0] for v in src), fmt, idx, matrix, rng, up, siting, T, O, out=dst)
                assert got is dst and torch.equal(bits(dst), bits(want[idx])), (fs, O, up, aligned, len(idx))
                assert guards_kept(store, foff, dst.numel()), (fs, O, up, aligned)
    assert seen == ({False, True} if CC.sub(fmt)[0] == 1 or O % 8 == 0 else {False})


@functools.lru_cache(maxsize=None)
def large_cut_frame():
    """the 4098 x 4098 frame and the restatement's cut of its tile 4, computed once"""
    c = XL.CUT_LIST_LARGE
    g = np.random.default_rng(13)
    Hc, Wc = CC.chroma_size(c["H"], c["W"], c["fmt"])
    f = CC.frame(*[g.integers(0, 256, s, dtype=np.int64) for s in ((1, c["H"], c["W"]), (1, Hc, Wc), (1, Hc, Wc))], c["fmt"])
    return f, KT.cut(f, c["fmt"], "bt709", "limited", "linear", c["siting"], c["T"], c["O"], c["rect"])[0]


@pytest.mark.parametrize("aligned", CS.ALIGNMENTS)
def test_cut_list_at_2048(aligned):
    """T = 2048, tile_items = 2^19, on the 4098 x 4098 left-sited nv12 frame: the list [4, 0, 8, 4] through cut_tiles (tile 8 is a
    corner of 2 x 2 pixels) and [4, 9, -1, 0] through the C call, whose entries outside the grid are whole tiles of +0.0f with
    nothing past the destination touched.  Tile 4 against the restatement's cut, every tile against chroma_tiles.cut_frame of its
    rectangle on the device"""
    need_memory(900 << 20)
    from progressivecodec_amd import chroma, frames
    kc = KC()
    c = XL.CUT_LIST_LARGE
    H, W, T, O = geo(c)
    fmt, siting = c["fmt"], c["siting"]
    f, want4 = large_cut_frame()
    (mode, off), _ = PAIR[aligned]
    src = views(fmt, H, W, mode, off, f)
    each = device_cuts(on_device(f), fmt, "bt709", "limited", "linear", siting, T, O, 3, (4, 0, 8))
    assert same(each[4], want4) and (bits(each[8])[:, 2:] == 0).all() and (bits(each[8])[:, :, 2:] == 0).all()
    foff = 4 if aligned else 5
    m = len(c["tiles"])
    store, dst = float_buffer(m * 3 * T * T, foff)
    dst = dst.view(m, 3, T, T)
    assert kc.plan(kc.CUT, src, fmt, f32=dst, overlap=O) is aligned
    got = kc.cut_tiles(tuple(v[0] for v in src), fmt, c["tiles"], "bt709", "limited", "linear", siting, T, O, out=dst)
    assert got is dst and all(torch.equal(bits(dst[k]), bits(each[t])) for k, t in enumerate(c["tiles"])), aligned
    assert guards_kept(store, foff, dst.numel())
    # the raw call into the same buffer, patterned again: the entries outside the grid are +0.0f
    store.view(torch.int32)[:] = store.view(torch.int32)[0]
    didx = torch.tensor(c["raw"], dtype=torch.int32, device=DEV)
    coef = frames.coefficients("bt709")
    s = frames._frame_struct(src)
    rc = kc.lib().pc_chroma_clips_cut_list(C.byref(s), *chroma.FORMATS[fmt], *chroma.SITINGS[siting], frames.RANGES["limited"],
                                           frames.UPSAMPLES["linear"], coef.a, coef.b, coef.c, coef.d, H, W, T, O, didx.data_ptr(), m,
                                           dst.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(bits(dst[0]), bits(each[4])) and torch.equal(bits(dst[3]), bits(each[0])) and (bits(dst[1:3]) == 0).all(), aligned
    assert guards_kept(store, foff, dst.numel())

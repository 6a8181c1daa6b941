"""Clips of YUV 4:2:0 frames without a GPU: the footprint DESIGN.md section 16 defines, on the restatements alone
(tests/clips_contract.py against tests/frame_tiles_contract.cut); the PCS1 container up to the model; libpc_clips.so's C ABI up to the
first device call; and progressivecodec_amd.clips' argument checks."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest
import torch

from tests import clips_contract as CC
from tests import frame_tiles_contract as GC
from tests import frames_contract as FC
from tests import image_shared
from tests import tiles_contract as TC
from tests.test_frames_host import fake_frame
from tests.test_tiles_host import blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 64
SIZES = [(1, 1), (2, 2), (64, 64), (65, 63), (100, 150), (127, 129)]
OVERLAPS = [0, 4, 16, 32]
MATS = list(FC.MATRICES)


def _lib():
    from progressivecodec_amd import clips
    return clips, clips.lib()


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def with_footprint_of(other, base, lu, ch):
    """the frame `other` with the samples of the footprint (lu, ch) taken from `base`"""
    out = [np.array(p) for p in other]
    out[0][:, lu[0]:lu[1], lu[2]:lu[3]] = base[0][:, lu[0]:lu[1], lu[2]:lu[3]]
    for p in range(1, len(out)):                                                     # the interleaved pair, or U and V
        out[p][:, ch[0]:ch[1], ch[2]:ch[3]] = base[p][:, ch[0]:ch[1], ch[2]:ch[3]]
    return tuple(out)


# -- the footprint -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("O", OVERLAPS)
def test_a_tile_whose_counts_are_zero_is_cut_to_the_same_bits(hw, O):
    """every sample outside one tile's footprint randomised: that tile's counts are zero and its cut is bit-identical; and whichever
    other tile has zero counts, too, is cut to the same bits as well"""
    H, W = hw
    ny, nx = TC.grid(H, W, T, O)
    for k, fmt in enumerate(FC.FORMATS):
        prev = FC.random_frame(1, H, W, fmt, seed=H * W + O + k)
        other = FC.random_frame(1, H, W, fmt, seed=H * W + O + k + 77)
        for up in FC.UPSAMPLES:
            matrix, rng = MATS[(k + O // 4) % 3], FC.RANGES[(k + (up == "linear")) % 2]
            for t in range(ny * nx):
                lu, ch = CC.footprint(t // nx, t % nx, H, W, T, O, up)
                cur = with_footprint_of(other, prev, lu, ch)
                counts = CC.tile_changes(cur, prev, fmt, T, O, up)
                assert counts[t] == [0, 0, 0], (hw, O, fmt, up, t)
                for s in range(ny * nx):
                    if counts[s] == [0, 0, 0]:
                        rect = (s // nx, s % nx, 1, 1)
                        a, b = (GC.cut(f, fmt, matrix, rng, up, T, O, rect) for f in (cur, prev))
                        assert same_bits(a, b), (hw, O, fmt, up, t, s)
                assert ny * nx == 1 or any(c != [0, 0, 0] for c in counts)
                # a sub-range counts the same
                assert CC.tile_changes(cur, prev, fmt, T, O, up, first_tile=t, n_tiles=1) == [counts[t]]


def test_the_footprint_in_numbers():
    # 100 x 150, O = 16: S = 48, 2 x 3 tiles; tile (1, 1) holds luma rows 48 .. 99, columns 48 .. 111
    assert CC.footprint(1, 1, 100, 150, T, 16, "linear") == ((48, 100, 48, 112), (23, 50, 23, 57))
    assert CC.footprint(1, 1, 100, 150, T, 16, "nearest") == ((48, 100, 48, 112), (24, 50, 24, 56))
    assert CC.footprint(0, 0, 100, 150, T, 16, "linear") == ((0, 64, 0, 64), (0, 33, 0, 33))
    assert CC.footprint(0, 2, 100, 150, T, 16, "linear") == ((0, 64, 96, 150), (0, 33, 47, 75))
    # an odd last luma row takes the chroma row after it where the frame has one: 127 x 129, O = 0, tile (0, 0) ends at row 63
    assert CC.footprint(0, 0, 127, 129, T, 0, "linear") == ((0, 64, 0, 64), (0, 33, 0, 33))
    assert CC.footprint(1, 2, 127, 129, T, 0, "linear") == ((64, 127, 128, 129), (31, 64, 63, 65))
    assert CC.footprint(0, 0, 1, 1, T, 0, "linear") == ((0, 1, 0, 1), (0, 1, 0, 1))


@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_the_halo_matters_under_linear_and_not_under_nearest(fmt):
    """a flat mid-grey frame with one chroma sample of the halo of tile (1, 1) changed: in the row above its chroma rows 24 .. 49, in
    the column left of its chroma columns 24 .. 55, and in the column right of them (luma column 111, the tile's last, is odd)"""
    H, W, O = 100, 150, 16
    mid = 1 << (FC.bits(fmt) - 1)
    Hc, Wc = FC.chroma_size(H, W)
    grey = lambda: [np.full((1, H, W), mid, np.int64), np.full((1, Hc, Wc), mid, np.int64), np.full((1, Hc, Wc), mid, np.int64)]   # noqa: E731
    prev = FC.frame(*grey(), fmt)
    inner = CC.footprint(1, 1, H, W, T, O, "nearest")[1]
    assert inner == (24, 50, 24, 56)
    for plane, where in [(1, (23, 40)), (2, (23, 40)), (1, (30, 23)), (2, (49, 56))]:
        c = grey()
        c[plane][0][where] = mid + 40
        cur = FC.frame(*c, fmt)
        # a footprint without the halo would call the tile static
        assert not (FC.codes(cur, fmt)[plane][0][inner[0]:inner[1], inner[2]:inner[3]] != mid).any()
        for up, differs in (("linear", True), ("nearest", False)):
            counts = CC.tile_changes(cur, prev, fmt, T, O, up)
            a, b = (GC.cut(f, fmt, "bt709", "limited", up, T, O, (1, 1, 1, 1)) for f in (cur, prev))
            assert (counts[4] != [0, 0, 0]) is differs, (fmt, plane, where, up, counts)
            assert same_bits(a, b) is not differs, (fmt, plane, where, up)
            assert counts[4] == ([0, int(plane == 1), int(plane == 2)] if differs else [0, 0, 0])


def test_p010_ignores_the_low_six_bits():
    H, W, O = 100, 150, 16
    prev = FC.random_frame(1, H, W, "p010", seed=5)
    g = np.random.default_rng(6)
    cur = tuple((p | g.integers(0, 64, p.shape).astype(np.uint16)) for p in prev)
    assert any((a != b).any() for a, b in zip(cur, prev))
    for up in FC.UPSAMPLES:
        assert CC.tile_changes(cur, prev, "p010", T, O, up) == [[0, 0, 0]] * 6
        assert same_bits(GC.cut(cur, "p010", "bt2020", "full", up, T, O), GC.cut(prev, "p010", "bt2020", "full", up, T, O))
    assert CC.source_table([prev, cur, prev], "p010", T, O, "linear") == [[0] * 6] * 3
    one = tuple(np.array(p) for p in cur)
    one[0][0, 99, 149] ^= 64                                                         # the lowest bit of a code
    assert CC.tile_changes(one, prev, "p010", T, O, "linear") == [[0, 0, 0]] * 5 + [[1, 0, 0]]
    assert CC.source_table([prev, cur, one, one, prev], "p010", T, O, "linear") == [[0] * 6, [0] * 6, [0] * 5 + [2], [0] * 5 + [2], [0] * 5 + [4]]


# -- PCS1 ----------------------------------------------------------------------------------------------------------------------------

SOURCE = [[0] * 6, [1, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [1, 3, 0, 0, 3, 0]]            # the codec test's clip under "linear"


def clip_blobs(source=SOURCE, contract=1, T_=T):
    return [[blob(T_, 16 * f + t, contract) if s == f else None for t, s in enumerate(row)] for f, row in enumerate(source)]


def pcs1(source=SOURCE, H=100, W=150, O=16, fmt="nv12", matrix="bt709", rng="limited", up="linear", contract=1):
    from progressivecodec_amd import clips
    blobs = clip_blobs(source, contract)
    return clips.pack_clip(blobs, source, H, W, T, O, fmt, matrix, rng, up, contract=contract), blobs


def test_pcs1_round_trip_aliasing_and_frame_container():
    from progressivecodec_amd import clips, container, frame_tiles, tiles
    assert clips.HEADER_BYTES == CC.HEADER_BYTES == 42 and clips.MAGIC == CC.MAGIC
    for k, (fmt, matrix, rng, up) in enumerate([("nv12", "bt709", "limited", "linear"), ("i420", "bt601", "full", "nearest"),
                                                ("p010", "bt2020", "limited", "linear")]):
        buf, blobs = pcs1(fmt=fmt, matrix=matrix, rng=rng, up=up, contract=7 + k)
        assert buf == CC.pack_clip(blobs, SOURCE, 100, 150, T, 16, fmt, matrix, rng, up, 7 + k)
        assert len(buf) == CC.container_bytes(blobs, SOURCE) == 42 + 16 * 24 + sum(len(b) for row in blobs for b in row if b is not None)
        hd = clips.parse_clip(buf)
        g = hd["grid"]
        assert (hd["fmt"], hd["matrix"], hd["range"], hd["upsample"], hd["bits"], hd["contract"], hd["F"]) == (fmt, matrix, rng, up, FC.bits(fmt), 7 + k, 4)
        assert (g.H, g.W, g.T, g.O, g.ny, g.nx) == (100, 150, T, 16, 2, 3) and hd["payload_start"] == 42 + 16 * 24
        assert clips.parse_clip(bytearray(buf))["table"] == hd["table"] == clips.parse_clip(memoryview(buf))["table"]
        # a reused tile repeats the entry of the frame it was last coded in; coded tiles follow each other in (frame, tile) order
        off = hd["payload_start"]
        for f in range(4):
            for t in range(6):
                assert hd["table"][f][t] == hd["table"][SOURCE[f][t]][t]
                if SOURCE[f][t] == f:
                    assert hd["table"][f][t] == (off, len(blobs[f][t]))
                    off += len(blobs[f][t])
                tb, th = clips.clip_tile_bytes(buf, hd, f, t)
                assert tb == blobs[SOURCE[f][t]][t] and th["image_size"] == (T, T)
        assert off == len(buf)
        for f in range(4):
            want = frame_tiles.pack_frame_tiled(tiles.pack_tiled([blobs[SOURCE[f][t]][t] for t in range(6)], 100, 150, T, 16, contract=7 + k),
                                                fmt, matrix, rng, up)
            assert clips.frame_container(buf, f) == want
            assert frame_tiles.parse_frame_tiled(want)["tiled"]["contract"] == 7 + k
    # one frame, one tile
    one, b1 = pcs1([[0]], 1, 1, 0)
    assert len(one) == 42 + 16 + len(b1[0][0]) and clips.parse_clip(one)["F"] == 1 and clips.frame_container(one, 0)[10 + 33 + 16:] == b1[0][0]
    assert clips.source_table([[True, False], [False, False], [False, True]]) == [[0, 0], [1, 0], [1, 0], [1, 3]]
    assert clips.source_table([]) == [[]]
    for bad in [[[1] * 6], [[0] * 6, [2] * 6], [[0] * 6, [1] * 6, [0] * 6], [[0] * 5], []]:
        with pytest.raises(container.ContainerError):
            clips.pack_clip([[blob(T, 1)] * len(r) for r in bad], bad, 100, 150, T, 16, "nv12", "bt709", "limited", "linear", contract=1)
    with pytest.raises(ValueError, match="fmt"):
        clips.pack_clip(clip_blobs(), SOURCE, 100, 150, T, 16, "nv21", "bt709", "limited", "linear", contract=1)


def test_pcs1_every_malformed_container_raises_before_the_model(monkeypatch):
    from progressivecodec_amd import clips, container
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    buf, blobs = pcs1(fmt="p010", matrix="bt2020")
    hd = clips.parse_clip(buf)

    def patched(off, fmt, *vals):
        b = bytearray(buf)
        struct.pack_into(fmt, b, off, *vals)
        return bytes(b)
    entry = lambda f, t: 42 + 16 * (6 * f + t)                                      # noqa: E731
    o00, l00 = hd["table"][0][0]
    cases = [(b"PCS2" + buf[4:], "not a PCS1"), (b"PCG1" + buf[4:], "not a PCS1"), (b"", "not a PCS1"), (b"PCS", "not a PCS1"),
             (patched(4, "B", 2), "version"), (patched(4, "B", 0), "version"),
             (patched(5, "B", 3), "corrupt"), (patched(6, "B", 3), "corrupt"), (patched(7, "B", 2), "corrupt"), (patched(8, "B", 2), "corrupt"),
             (patched(9, "B", 8), "bits"), (patched(5, "B", 0), "bits"),
             (patched(14, "<I", 200), "grid"), (patched(18, "<I", 64), "grid"),      # H, W: another grid than the header's ny x nx
             (patched(22, "<I", 96), "corrupt"), (patched(26, "<I", 6), "corrupt"), (patched(26, "<I", 36), "corrupt"),       # T, O
             (patched(30, "<I", 3), "grid"), (patched(34, "<I", 2), "grid"), (patched(14, "<I", 0), "corrupt"),
             (patched(14, "<I", 2 ** 31), "corrupt"),
             (patched(38, "<I", 0), "no frames"), (patched(38, "<I", 2 ** 32 - 1), "truncated PCS1 table"),
             (buf[:42], "truncated PCS1 table"), (buf[:hd["payload_start"] - 1], "truncated PCS1 table"),
             # two entries are either equal or disjoint
             (patched(entry(1, 1), "<QQ", o00 + 1, l00), "overlaps"), (patched(entry(1, 1), "<QQ", o00, l00 - 1), "overlaps"),
             (patched(entry(1, 1), "<QQ", o00, l00 + 1), "overlaps"), (patched(entry(3, 5), "<QQ", o00 + l00 - 1, 2), "overlaps"),
             (patched(entry(2, 2), "<QQ", 0, len(buf)), "overlaps")]
    for n in range(4, 42):
        cases.append((buf[:n], "truncated PCS1 header"))
    for bad, msg in cases:
        with pytest.raises(container.ContainerError, match=msg):
            clips.parse_clip(bad)
        with pytest.raises(container.ContainerError, match=msg):
            clips.decode_clip(None, bad)
        with pytest.raises(container.ContainerError, match=msg):
            clips.frame_container(bad, 0)
    # an entry equal to another is aliasing, whoever wrote it
    assert clips.parse_clip(patched(entry(3, 5), "<QQ", o00, l00))["table"][3][5] == (o00, l00)
    # refusals that need the frames, the region, the tiles or the level
    for frames in ([4], [-1], [0, 4], 3, [0.5], ["0"], [None]):
        with pytest.raises(container.ContainerError, match="frame"):
            clips.decode_clip(None, buf, frames=frames)
    for k in (4, -1, 1.5, None):
        with pytest.raises(container.ContainerError, match="frame"):
            clips.frame_container(buf, k)
    for region in [(1, 0, 2, 2), (0, 1, 2, 2), (0, 0, 3, 2), (0, 0, 2, 3), (0, 0, 101, 150), (-2, 0, 4, 4), (0, 0, 0, 2), "all"]:
        with pytest.raises(container.ContainerError, match="admissible|outside|region"):
            clips.decode_clip(None, buf, region=region)
    for level in (2, -3):
        with pytest.raises(container.ContainerError, match="no level"):
            clips.decode_clip(None, buf, level=level)
    with pytest.raises(ValueError, match="fmt"):
        clips.decode_clip(None, buf, fmt="nv21")
    with pytest.raises(ValueError, match="max_tiles_per_call"):
        clips.decode_clip(None, buf, max_tiles_per_call=0)
    # a tile whose container is for another tile size, coded otherwise than its neighbours, or under another contract
    for bad_blob, msg in [(blob(128, 5), "frame 3, tile 4.*128x128"), (blob(T, 5, qualities=(0, 0.75)), "was coded as"),
                          (blob(T, 5, contract=2), "frame 3, tile 4: numeric contract")]:
        bl = clip_blobs()
        bl[3][4] = bad_blob
        bad = clips.pack_clip(bl, SOURCE, 100, 150, T, 16, "nv12", "bt709", "limited", "linear", contract=1)
        with pytest.raises(container.ContainerError, match=msg):
            clips.decode_clip(None, bad, frames=[3])
        with pytest.raises(AttributeError):                                          # the frames before it are not touched by it
            clips.decode_clip(None, bad, frames=[0, 1, 2])
    with pytest.raises(container.ContainerError, match="contract"):
        monkeypatch.setattr(container, "build_contract_id", lambda: 2)
        clips.decode_clip(None, buf)
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    # a clip cut off inside its payload still gives every frame whose tiles it holds completely, and refuses the others before the model
    end2 = hd["table"][1][0][0] + hd["table"][1][0][1]                               # frames 0 .. 2 are complete here
    cut = buf[:end2]
    for k in range(3):
        assert clips.frame_container(cut, k) == clips.frame_container(buf, k)
    with pytest.raises(container.ContainerError, match="frame 3, tile 1"):
        clips.frame_container(cut, 3)
    with pytest.raises(container.ContainerError, match="frame 3, tile 1"):
        clips.decode_clip(None, cut)
    with pytest.raises(container.ContainerError, match="frame 1, tile 0"):
        clips.decode_clip(None, buf[:end2 - 1], frames=[1])
    with pytest.raises(AttributeError):                                              # tile (0, 0) of frame 3 is frame 1's
        clips.decode_clip(None, cut, frames=[3], region=(4, 6, 20, 30))
    # nothing above is wrong with a good container: with a model (here: none) the decode goes on to use it
    with pytest.raises(AttributeError):
        clips.decode_clip(None, buf)
    with pytest.raises(AttributeError):
        clips.decode_clip(None, cut, frames=range(3), level=0, fmt="nv12")


def test_decode_asks_the_model_for_each_byte_range_once(monkeypatch):
    """what reaches the model: frame 0 whole, then only the tiles whose entries differ from the frame handled just before"""
    from progressivecodec_amd import clips, container
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    buf, _ = pcs1()
    seen = []

    class Model:
        def decompress(self, strings, shape, q, mask_pol):
            seen.append((len(strings[1]), tuple(shape), q, mask_pol))
            raise KeyError("far enough")
    for kw, n in [(dict(), 6), (dict(max_tiles_per_call=4), 4), (dict(region=(60, 60, 8, 8)), 4), (dict(frames=[3], region=(4, 6, 20, 30)), 1)]:
        del seen[:]
        with pytest.raises(KeyError):
            clips.decode_clip(Model(), buf, level=1, **kw)
        assert seen == [(n, (1, 1), 0.5, "point-based-std")], (kw, seen)

    class Quiet:
        calls = []

        def decompress(self, strings, shape, q, mask_pol):
            Quiet.calls.append(len(strings[1]))
            return {"x_hat": torch.zeros(len(strings[1]), 3, T, T)}
    monkeypatch.setattr(clips, "stitch_frame", lambda x, g, *a, **k: x.shape[0])
    assert clips.decode_clip(Quiet(), buf) == [6] * 4 and Quiet.calls == [6, 1, 2]
    del Quiet.calls[:]
    assert clips.decode_clip(Quiet(), buf, frames=[3, 3, 0, 1], max_tiles_per_call=2) == [6] * 4 and Quiet.calls == [2, 2, 2, 2, 1, 1]


# -- the library, no device ----------------------------------------------------------------------------------------------------------

def test_library_exports_every_declared_function():
    cl, L = _lib()
    hdr = open(os.path.join(ROOT, "progressivecodec_amd", "clips_csrc", "pc_clips.h")).read()
    declared = re.findall(r"PC_API\s+[\w\s\*]+?\b(pc_\w+)\s*\(", hdr)
    assert len(declared) == 6 and sorted(declared) == sorted(cl.EXPORTS)
    for name in declared:
        getattr(L, name)
    assert L.pc_clips_strerror(-1).decode() and L.pc_clips_strerror(-6).decode() and L.pc_clips_last_hip_error() == 0
    # a library of its own: no other library of the project is linked, and the codec's source hash does not cover it
    import bench
    import inspect
    assert "clips" not in inspect.getsource(bench.source_hash)
    mk = image_shared.build_rule("clips")                                             # image_csrc/lib.mk, which the library's Makefile includes
    assert "-ffp-contract=off" in mk and not re.search(r"-lpc|libpc(odec|_pixels|_tiles|_rate|_metrics|_frames|_frame_tiles|_frame_rate)\b", mk)
    top = open(os.path.join(ROOT, "progressivecodec_amd", "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\bclips\b", top, re.M) and re.search(r"^\.PHONY:.*\bclips\b", top, re.M)
    assert "$(MAKE) -C ../clips_csrc clean" in top and re.search(r"^clips:\n\t\$\(MAKE\) -C \.\./clips_csrc$", top, re.M)
    # the frame is the one record of image_csrc/pc_yuv_frame.h, as pc_frames.h's is: frames.Frame serves this library, too
    image_shared.assert_frame_is_shared(hdr, "pc_cl_frame")


def test_workspace_size_is_24_bytes_per_block():
    _, L = _lib()
    for size, n in [(64, 1), (64, 6), (128, 9), (512, 40), (1024, 3), (2048, 2)]:
        assert L.pc_clips_changes_workspace_size(size, n) == 24 * n * (size * size // 4096 + 1), (size, n)
    for bad in [(0, 1), (32, 1), (96, 1), (-64, 1), (4096, 1), (64, 0), (64, -1), (2048, 2 ** 31 - 1)]:
        assert L.pc_clips_changes_workspace_size(*bad) == 0, bad


def test_plan_is_host_only_and_each_precondition_is_broken_alone():
    """made-up pointer values: nothing may be dereferenced or launched (there is no GPU here)"""
    from progressivecodec_amd import frames
    cl, L = _lib()
    Fp = 0x7000_0100_0000
    H, W = 96, 160

    def plan(op, fmt, frame, other=None, f32=Fp, O=0):
        wide = C.c_int(-1)
        rc = L.pc_clips_plan(op, frames.FORMATS[fmt], C.byref(frame) if frame is not None else None,
                             C.byref(other) if other is not None else None, f32, O, C.byref(wide))
        return rc, wide.value
    for fmt in FC.FORMATS:
        es = 2 if fmt == "p010" else 1
        ok = fake_frame(frames, fmt, H, W)
        ok2 = fake_frame(frames, fmt, H, W, base=0x7100_0000_1000, pad=4)            # pitched differently
        assert plan(cl.CHANGES, fmt, ok, ok2) == (0, 1) and plan(cl.CUT, fmt, ok) == (0, 1)
        assert plan(cl.CHANGES, fmt, ok, ok2, f32=None) == (0, 1)                     # the changes have no floats
        assert plan(cl.CUT, fmt, ok, None, f32=None)[0] == -1 and plan(cl.CHANGES, fmt, ok, None)[0] == -1
        for off in (4, 8, 12):
            assert plan(cl.CUT, fmt, ok, f32=Fp + off) == (0, 0)                      # the floats: 16-byte aligned
        for nm in ["y", "u"] + (["v"] if fmt == "i420" else []):
            for off in (1, 2, 3):
                bad = fake_frame(frames, fmt, H, W)
                setattr(bad, nm, getattr(bad, nm) + off * es)                         # each plane: aligned to four elements
                assert plan(cl.CUT, fmt, bad) == (0, 0) and plan(cl.CHANGES, fmt, bad, ok2) == (0, 0), (fmt, nm, off)
                assert plan(cl.CHANGES, fmt, ok2, bad) == (0, 0), (fmt, nm, off)      # in either frame
                assert plan(cl.CUT, fmt, ok, bad) == (0, 1)                           # the cut has no second frame
            bad = fake_frame(frames, fmt, H, W)
            setattr(bad, nm + "_row", getattr(bad, nm + "_row") + 2)                  # each row stride: a multiple of 4
            assert plan(cl.CUT, fmt, bad) == (0, 0) and plan(cl.CHANGES, fmt, bad, ok2) == (0, 0) and plan(cl.CHANGES, fmt, ok, bad) == (0, 0)
            free = fake_frame(frames, fmt, H, W)
            setattr(free, nm + "_batch", getattr(free, nm + "_batch") + 1)            # one frame per call: no batch stride counts
            assert plan(cl.CUT, fmt, free) == (0, 1) and plan(cl.CHANGES, fmt, free, free) == (0, 1)
        for O, wide in [(0, 1), (8, 1), (16, 1), (32, 1), (4, 0), (12, 0), (20, 0), (28, 0)]:
            assert plan(cl.CUT, fmt, ok, O=O) == (0, wide) and plan(cl.CHANGES, fmt, ok, ok2, O=O) == (0, wide), (fmt, O)
        assert plan(cl.CUT, fmt, ok, O=-4)[0] == -1 and plan(cl.CUT, fmt, None)[0] == -1 and plan(2, fmt, ok, ok2)[0] == -1
        nul = fake_frame(frames, fmt, H, W)
        nul.u = None
        assert plan(cl.CUT, fmt, nul)[0] == -1 and plan(cl.CHANGES, fmt, ok, nul)[0] == -1
        assert L.pc_clips_plan(cl.CUT, frames.FORMATS[fmt], C.byref(ok), None, Fp, 0, None) == -1
    f = fake_frame(frames, "nv12", H, W)
    wide = C.c_int(-1)
    assert L.pc_clips_plan(cl.CUT, 3, C.byref(f), None, Fp, 0, C.byref(wide)) == -1
    assert plan(cl.CUT, "nv12", f) == (0, 1) and plan(cl.CUT, "i420", f)[0] == -1     # an I420 frame needs its V pointer


def test_every_argument_error_returns_before_the_device():
    """fake device pointers: every call below must return PC_ERR_ARG without touching them (no GPU here)"""
    from progressivecodec_amd import frames
    _, L = _lib()
    Fp, Wk, S, Ix = 0x7000_0100_0000, 0x7000_0200_0000, 0x7000_0300_0000, 0x7000_0400_0000
    H, W, O = 100, 150, 16                                                            # 2 x 3 tiles, S = 48
    k = frames.coefficients("bt709")
    for fmt in FC.FORMATS:
        fid = frames.FORMATS[fmt]

        def broken(field, value):
            f = fake_frame(frames, fmt, H, W)
            setattr(f, field, value)
            return f
        bad_frames = [None, broken("y", None), broken("u", None), broken("y_row", W - 1), broken("u_row", (2 * 75 if fmt != "i420" else 75) - 1)]
        if fmt == "i420":
            bad_frames += [broken("v", None), broken("v_row", 74)]
        if fmt == "p010":
            bad_frames += [broken("y", fake_frame(frames, fmt, H, W).y + 1), broken("u", fake_frame(frames, fmt, H, W).u + 1)]
        geo = [dict(H=0), dict(W=0), dict(H=-5), dict(T=0), dict(T=32), dict(T=96), dict(T=-64), dict(T=4096, O=0), dict(O=2), dict(O=6),
               dict(O=36), dict(O=-4), dict(fmt=3), dict(fmt=-1), dict(up=2), dict(up=-1)]
        call = lambda fn, a: fn(*[C.byref(v) if isinstance(v, frames.Frame) else v for v in a.values()])     # noqa: E731

        nbytes = L.pc_clips_changes_workspace_size(T, 6)
        ok = dict(cur=fake_frame(frames, fmt, H, W), prev=fake_frame(frames, fmt, H, W, base=0x7100_0000_1000), fmt=fid, up=1, H=H, W=W, T=T,
                  O=O, first=0, n=6, ws=Wk, nbytes=nbytes, out=S, stream=None)
        bads = [dict(cur=f) for f in bad_frames] + [dict(prev=f) for f in bad_frames] + geo + [
            dict(first=-1), dict(first=1), dict(n=0), dict(n=7), dict(n=-1), dict(first=6, n=1), dict(first=2 ** 31 - 1, n=2 ** 31 - 1),
            dict(ws=None), dict(ws=Wk + 4), dict(out=None), dict(out=S + 4), dict(nbytes=nbytes - 1), dict(nbytes=0)]
        for bad in bads:
            assert call(L.pc_clips_tile_changes, dict(ok, **bad)) == -1, (fmt, bad)

        ok = dict(src=fake_frame(frames, fmt, H, W), fmt=fid, range=0, up=1, a=k.a, b=k.b, c=k.c, d=k.d, H=H, W=W, T=T, O=O, tiles=Ix, n=4,
                  dst=Fp, stream=None)
        bads = [dict(src=f) for f in bad_frames] + geo + [dict(range=2), dict(range=-1), dict(tiles=None), dict(tiles=Ix + 2), dict(n=0),
                                                          dict(n=-1), dict(n=2 ** 31 - 1), dict(dst=None), dict(dst=Fp + 2)]
        for bad in bads:
            assert call(L.pc_clips_cut_list, dict(ok, **bad)) == -1, (fmt, bad)


def test_python_rejects_before_any_device_call(monkeypatch):
    from progressivecodec_amd import clips as cl

    def touched(*a, **k):
        raise AssertionError("the device was reached")
    for name in ("device", "current_stream", "synchronize", "current_device", "_lazy_init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.setattr(cl, "lib", touched)
    y, uv, u = torch.zeros(100, 150, dtype=torch.uint8), torch.zeros(50, 75, 2, dtype=torch.uint8), torch.zeros(50, 75, dtype=torch.uint8)
    f = (y, uv)
    with pytest.raises(ValueError, match="GPU"):
        cl.tile_changes(f, f, "nv12", tile=64)
    with pytest.raises(ValueError, match="GPU"):
        cl.tile_changes((y, u, u), (y, u, u), "i420", tile=64)
    with pytest.raises(ValueError, match="GPU"):
        cl.clip_changes([f, f], "nv12", tile=64)
    with pytest.raises(ValueError, match="GPU"):
        cl.clip_changes((torch.stack([y, y]), torch.stack([uv, uv])), "nv12", tile=64)
    with pytest.raises(ValueError, match="GPU"):
        cl.cut_tiles(f, "nv12", [0], tile=64)
    with pytest.raises(ValueError, match="GPU"):
        cl.encode_clip(None, [f, f], [0, 1], "nv12", tile=64)
    with pytest.raises(ValueError, match="GPU"):
        cl.encode_clip(None, [f, f], [0, 1], "nv12", tile=64, reuse=False)
    for fn in (lambda **kw: cl.tile_changes(f, f, **dict(dict(fmt="nv12"), **kw)), lambda **kw: cl.clip_changes([f], **dict(dict(fmt="nv12"), **kw))):
        with pytest.raises(ValueError, match="fmt"):
            fn(fmt="nv21")
        with pytest.raises(ValueError, match="upsample"):
            fn(upsample="cubic")
    with pytest.raises(ValueError, match="matrix"):
        cl.cut_tiles(f, "nv12", [0], matrix="bt470")
    with pytest.raises(ValueError, match="range"):
        cl.cut_tiles(f, "nv12", [0], range="tv")
    with pytest.raises(ValueError, match="range"):
        cl.encode_clip(None, [f], [0], "nv12", range="tv")
    with pytest.raises(ValueError, match="max_tiles_per_call"):
        cl.encode_clip(None, [f], [0], "nv12", max_tiles_per_call=0)
    with pytest.raises(TypeError, match="uint16"):
        cl.tile_changes(f, f, "p010")
    with pytest.raises(ValueError, match="UV must be"):
        cl.tile_changes((y, uv[:2]), f, "nv12")
    with pytest.raises(ValueError, match="one frame"):
        cl.tile_changes((torch.stack([y, y]), torch.stack([uv, uv])), f, "nv12")
    for bad in ([], (), None, "clip"):
        with pytest.raises(ValueError, match="non-empty list"):
            cl.clip_changes(bad, "nv12")
    with pytest.raises(ValueError, match="got one frame"):
        cl.clip_changes(f, "nv12")
    with pytest.raises(ValueError, match=r"frames\[0\]: UV must be"):
        cl.clip_changes([(y, uv[:2]), f], "nv12")
    assert cl.ClipPlan._fields == ("source", "n_coded", "n_reused", "container_bytes")
    assert (cl.CHANGES, cl.CUT) == (0, 1)


def test_python_checks_that_need_a_frame_that_passes(monkeypatch):
    """the checks behind the frame's own: with frames._frame_view's device test out of the way, nothing else may reach the device"""
    from progressivecodec_amd import clips as cl

    def touched(*a, **k):
        raise AssertionError("the device was reached")
    for name in ("device", "current_stream", "synchronize", "current_device", "_lazy_init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.setattr(cl, "lib", touched)
    y, uv = torch.zeros(100, 150, dtype=torch.uint8), torch.zeros(50, 75, 2, dtype=torch.uint8)
    small = (torch.zeros(64, 64, dtype=torch.uint8), torch.zeros(32, 32, 2, dtype=torch.uint8))
    monkeypatch.setattr(cl, "_one_frame", lambda p, fmt, what: ([t.unsqueeze(0) for t in p], p[0].shape[0], p[0].shape[1]))
    f = (y, uv)
    with pytest.raises(ValueError, match="prev must be a 100x150 frame"):
        cl.tile_changes(f, small, "nv12", tile=64)
    with pytest.raises(ValueError, match=r"frames\[1\] is 64x64"):
        cl.clip_changes([f, small], "nv12", tile=64)
    for kw in (dict(first_tile=-1), dict(first_tile=6), dict(n_tiles=0), dict(n_tiles=7), dict(first_tile=3, n_tiles=4)):
        with pytest.raises(ValueError, match="outside the 2x3 grid"):
            cl.tile_changes(f, f, "nv12", tile=64, overlap=16, **kw)
        with pytest.raises(ValueError, match="outside the 2x3 grid"):
            cl.clip_changes([f, f], "nv12", tile=64, overlap=16, **kw)
    with pytest.raises(ValueError, match="multiple of 64"):
        cl.tile_changes(f, f, "nv12", tile=96)
    with pytest.raises(ValueError, match="overlap"):
        cl.tile_changes(f, f, "nv12", tile=64, overlap=6)
    with pytest.raises(ValueError, match="at most 2048"):
        cl.tile_changes(f, f, "nv12", tile=4096)
    # indices are validated on the host before they are uploaded
    for bad in ([6], [-1], [0, 1, 6], [0.0], [True], ["1"], [None], [], torch.tensor([2, 7])):
        with pytest.raises(ValueError, match="tile.ind"):
            cl.cut_tiles(f, "nv12", bad, tile=64, overlap=16)
    for out, exc in [(torch.zeros(2, 3, 64, 64, dtype=torch.float64), TypeError), (torch.zeros(3, 3, 64, 64), ValueError),
                     (torch.zeros(2, 3, 64, 65)[..., :64], ValueError), (torch.zeros(4, 3, 64, 64)[::2], ValueError), ("x", TypeError)]:
        with pytest.raises(exc, match="out must be"):
            cl.cut_tiles(f, "nv12", [0, 5], tile=64, overlap=16, out=out)

"""Rate-controlled clips without a GPU: the restatement of DESIGN.md section 17 (tests/clip_rate_contract.py) on hand-made source
tables; the PCS2 container up to the model; decode_clip's byte work and what reaches a recording model; libpc_clip_rate.so's C ABI up
to the first device call; and progressivecodec_amd.clip_rate's argument checks."""
import ctypes as C
import os
import re
import struct
from fractions import Fraction

import pytest
import torch

from tests import clip_rate_contract as RC2
from tests import clips_contract as CC
from tests import frames_contract as FC
from tests import image_shared
from tests.test_clips_host import SOURCE
from tests.test_frames_host import fake_frame
from tests.test_tiles_host import blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 64
#: the quality of the one level a coded tile of SOURCE holds, by (frame, tile): three qualities, mixed within every frame
Q_OF = {(0, 0): 0.5, (0, 1): 0, (0, 2): 10, (0, 3): 0.5, (0, 4): 0, (0, 5): 0.5, (1, 0): 10, (3, 1): 0.5, (3, 4): 10}


def _lib():
    from progressivecodec_amd import clip_rate
    return clip_rate, clip_rate.lib()


def clip_blobs(source=SOURCE, contract=1, q_of=Q_OF):
    return [[blob(T, 16 * f + t, contract, qualities=(q_of.get((f, t), 0.5),)) if s == f else None for t, s in enumerate(row)]
            for f, row in enumerate(source)]


def pcs2(source=SOURCE, H=100, W=150, O=16, fmt="nv12", matrix="bt709", rng="limited", up="linear", contract=1):
    from progressivecodec_amd import clip_rate
    blobs = clip_blobs(source, contract)
    return clip_rate.pack_clip(blobs, source, H, W, T, O, fmt, matrix, rng, up, contract=contract), blobs


# -- the items, the weights, the budget ------------------------------------------------------------------------------------------------

def test_items_runs_and_weights_on_hand_made_tables():
    from progressivecodec_amd import clip_rate as cr
    items, runs = cr.items_of(SOURCE)
    assert items == [(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (1, 0), (3, 1), (3, 4)]
    assert runs == [[0], [0, 1, 2], [0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2], [0, 1, 2, 3], [1, 2, 3], [3], [3]]
    assert (items, runs) == RC2.items_of(SOURCE)
    assert sum(len(r) for r in runs) == 4 * 6                                        # every (frame, tile) is shown by exactly one item
    # the default weight is the run length
    assert cr.item_weights(items, runs, 6, 4) == [1, 3, 4, 4, 3, 4, 3, 1, 1] == RC2.weights(SOURCE)
    assert all(isinstance(w, Fraction) for w in cr.item_weights(items, runs, 6, 4))
    fw = [Fraction(1, 3), 2, Fraction(5, 2), 1]
    imp = [1, Fraction(1, 7), 3, 1, 10 ** 6, Fraction(9, 4)]
    got = cr.item_weights(items, runs, 6, 4, imp, fw)
    s012, s0123, s123 = Fraction(1, 3) + 2 + Fraction(5, 2), Fraction(1, 3) + 2 + Fraction(5, 2) + 1, 2 + Fraction(5, 2) + 1
    assert got == [Fraction(1, 3), s012 / 7, 3 * s0123, s0123, 10 ** 6 * s012, Fraction(9, 4) * s0123, s123, Fraction(1, 7), 10 ** 6]
    assert got == RC2.weights(SOURCE, imp, fw)
    assert cr.item_weights(items, runs, 6, 4, None, fw) == RC2.weights(SOURCE, None, fw)
    # floats are taken exactly
    assert cr.item_weights(items, runs, 6, 4, [0.1] * 6)[0] == Fraction(0.1) != Fraction(1, 10)
    # without reuse every tile is its own item of weight 1; a static clip has n items of weight F
    every = [[f] * 3 for f in range(5)]
    items, runs = cr.items_of(every)
    assert items == [(f, t) for f in range(5) for t in range(3)] and runs == [[f] for f, _ in items]
    assert cr.item_weights(items, runs, 3, 5) == [1] * 15
    items, runs = cr.items_of([[0] * 3] * 5)
    assert items == [(0, 0), (0, 1), (0, 2)] and runs == [[0, 1, 2, 3, 4]] * 3 and cr.item_weights(items, runs, 3, 5) == [5] * 3
    assert cr.items_of([[0]]) == ([(0, 0)], [[0]])
    with pytest.raises(ValueError, match="was not coded in"):
        cr.items_of([[0, 0], [0, 2]])
    for bad in (dict(importance=[1] * 5), dict(importance=[1, 1, 0]), dict(importance=[1, -1, 1]), dict(frame_weights=[1] * 4),
                dict(frame_weights=[1, 1, 1, 1, 0])):
        with pytest.raises(ValueError, match="importance|frame_weights"):
            cr.item_weights(items, runs, 3, 5, **bad)
    assert RC2.budget(10 ** 6, 4, 6) == 10 ** 6 - 42 - 16 * 24
    assert cr.ClipRatePlan._fields == ("source", "items", "weights", "levels", "rates", "dists", "plane_dists", "den", "container_bytes",
                                       "predicted", "sse", "n_coded", "n_reused")


def test_the_restatements_per_frame_sums():
    pd = [[[100 * i + 10 * l + p for p in range(3)] for l in range(2)] for i in range(9)]
    levels = [0, 1, 0, 1, 0, 1, 0, 1, 1]
    sse = RC2.frame_sse(SOURCE, pd, levels)
    at = lambda i: pd[i][levels[i]]                                                  # noqa: E731
    assert sse[0] == [sum(at(i)[p] for i in range(6)) for p in range(3)]
    assert sse[1] == sse[2] == [sum(at(i)[p] for i in (6, 1, 2, 3, 4, 5)) for p in range(3)]
    assert sse[3] == [sum(at(i)[p] for i in (6, 7, 2, 3, 8, 5)) for p in range(3)]
    dists = [[sum(v) for v in row] for row in pd]
    assert RC2.predicted(SOURCE, dists, levels) == sum(sum(row) for row in sse)


# -- PCS2 ----------------------------------------------------------------------------------------------------------------------------

def test_pcs2_round_trip_aliasing_and_frame_container():
    from progressivecodec_amd import clip_rate as cr
    from progressivecodec_amd import clips, container, frame_tiles, tiles
    assert cr.HEADER_BYTES == RC2.HEADER_BYTES == 42 and cr.MAGIC == RC2.MAGIC == b"PCS2" != clips.MAGIC
    for k, (fmt, matrix, rng, up) in enumerate([("nv12", "bt709", "limited", "linear"), ("i420", "bt601", "full", "nearest"),
                                                ("p010", "bt2020", "limited", "linear")]):
        buf, blobs = pcs2(fmt=fmt, matrix=matrix, rng=rng, up=up, contract=7 + k)
        assert buf == RC2.pack_clip(blobs, SOURCE, 100, 150, T, 16, fmt, matrix, rng, up, 7 + k)
        assert buf[:4] == b"PCS2" and buf[4:] == clips.pack_clip(blobs, SOURCE, 100, 150, T, 16, fmt, matrix, rng, up, contract=7 + k)[4:]
        assert len(buf) == CC.container_bytes(blobs, SOURCE) == 42 + 16 * 24 + sum(len(b) for row in blobs for b in row if b is not None)
        hd = cr.parse_clip(buf)
        g = hd["grid"]
        assert (hd["fmt"], hd["matrix"], hd["range"], hd["upsample"], hd["bits"], hd["contract"], hd["F"]) == (fmt, matrix, rng, up, FC.bits(fmt), 7 + k, 4)
        assert (g.H, g.W, g.T, g.O, g.ny, g.nx) == (100, 150, T, 16, 2, 3) and hd["payload_start"] == 42 + 16 * 24
        assert cr.parse_clip(bytearray(buf))["table"] == hd["table"] == cr.parse_clip(memoryview(buf))["table"]
        assert hd == clips.parse_clip(b"PCS1" + buf[4:])                             # PCS1's header, table and payload rules
        off = hd["payload_start"]
        for f in range(4):
            for t in range(6):
                assert hd["table"][f][t] == hd["table"][SOURCE[f][t]][t]
                if SOURCE[f][t] == f:
                    assert hd["table"][f][t] == (off, len(blobs[f][t]))
                    off += len(blobs[f][t])
                tb, th = cr.tile_blob(buf, hd, f, t)
                assert tb == blobs[SOURCE[f][t]][t] and th["image_size"] == (T, T) and th["qualities"] == [Q_OF[(SOURCE[f][t], t)]]
        assert off == len(buf)
        for f in range(4):
            inner = tiles.pack_tiled([blobs[SOURCE[f][t]][t] for t in range(6)], 100, 150, T, 16, contract=7 + k, per_tile_levels=True)
            want = frame_tiles.pack_frame_tiled(inner, fmt, matrix, rng, up)
            assert cr.frame_container(buf, f) == want
            hf = frame_tiles.parse_frame_tiled(want)
            assert hf["tiled"]["magic"] == b"PCT2" and hf["tiled"]["contract"] == 7 + k
        # each module reads its own magic only
        with pytest.raises(container.ContainerError, match="not a PCS1"):
            clips.parse_clip(buf)
        with pytest.raises(container.ContainerError, match="not a PCS1"):
            clips.frame_container(buf, 0)
        pcs1 = clips.pack_clip(blobs, SOURCE, 100, 150, T, 16, fmt, matrix, rng, up, contract=7 + k)
        with pytest.raises(container.ContainerError, match="not a PCS2"):
            cr.parse_clip(pcs1)
        with pytest.raises(container.ContainerError, match="not a PCS2"):
            cr.frame_container(pcs1, 0)
    one, b1 = pcs2([[0]], 1, 1, 0)
    assert len(one) == 42 + 16 + len(b1[0][0]) and cr.parse_clip(one)["F"] == 1 and cr.frame_container(one, 0)[10 + 33 + 16:] == b1[0][0]
    for bad in [[[1] * 6], [[0] * 6, [2] * 6], [[0] * 6, [1] * 6, [0] * 6], [[0] * 5], []]:
        with pytest.raises(container.ContainerError):
            cr.pack_clip([[blob(T, 1, qualities=(0.5,))] * len(r) for r in bad], bad, 100, 150, T, 16, "nv12", "bt709", "limited", "linear", contract=1)
    with pytest.raises(ValueError, match="fmt"):
        cr.pack_clip(clip_blobs(), SOURCE, 100, 150, T, 16, "nv21", "bt709", "limited", "linear", contract=1)


def test_pcs2_every_malformed_container_raises_before_the_model(monkeypatch):
    from progressivecodec_amd import clip_rate as cr
    from progressivecodec_amd import container
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    buf, blobs = pcs2(fmt="p010", matrix="bt2020")
    hd = cr.parse_clip(buf)

    def patched(off, fmt, *vals):
        b = bytearray(buf)
        struct.pack_into(fmt, b, off, *vals)
        return bytes(b)
    entry = lambda f, t: 42 + 16 * (6 * f + t)                                      # noqa: E731
    o00, l00 = hd["table"][0][0]
    cases = [(b"PCS3" + buf[4:], "not a PCS2"), (b"PCG1" + buf[4:], "not a PCS2"), (b"", "not a PCS2"), (b"PCS", "not a PCS2"),
             (patched(4, "B", 2), "version"), (patched(4, "B", 0), "version"),
             (patched(5, "B", 3), "corrupt"), (patched(6, "B", 3), "corrupt"), (patched(7, "B", 2), "corrupt"), (patched(8, "B", 2), "corrupt"),
             (patched(9, "B", 8), "bits"), (patched(5, "B", 0), "bits"),
             (patched(14, "<I", 200), "grid"), (patched(18, "<I", 64), "grid"),
             (patched(22, "<I", 96), "corrupt"), (patched(26, "<I", 6), "corrupt"), (patched(26, "<I", 36), "corrupt"),
             (patched(30, "<I", 3), "grid"), (patched(34, "<I", 2), "grid"), (patched(14, "<I", 0), "corrupt"),
             (patched(14, "<I", 2 ** 31), "corrupt"),
             (patched(38, "<I", 0), "no frames"), (patched(38, "<I", 2 ** 32 - 1), "truncated PCS2 table"),
             (buf[:42], "truncated PCS2 table"), (buf[:hd["payload_start"] - 1], "truncated PCS2 table"),
             (patched(entry(1, 1), "<QQ", o00 + 1, l00), "overlaps"), (patched(entry(1, 1), "<QQ", o00, l00 - 1), "overlaps"),
             (patched(entry(1, 1), "<QQ", o00, l00 + 1), "overlaps"), (patched(entry(3, 5), "<QQ", o00 + l00 - 1, 2), "overlaps"),
             (patched(entry(2, 2), "<QQ", 0, len(buf)), "overlaps")]
    for n in range(4, 42):
        cases.append((buf[:n], "truncated PCS2 header"))
    for bad, msg in cases:
        with pytest.raises(container.ContainerError, match=msg):
            cr.parse_clip(bad)
        with pytest.raises(container.ContainerError, match=msg):
            cr.decode_clip(None, bad)
        with pytest.raises(container.ContainerError, match=msg):
            cr.frame_container(bad, 0)
    assert cr.parse_clip(patched(entry(3, 5), "<QQ", o00, l00))["table"][3][5] == (o00, l00)
    for frames in ([4], [-1], [0, 4], 3, [0.5], ["0"], [None]):
        with pytest.raises(container.ContainerError, match="frame"):
            cr.decode_clip(None, buf, frames=frames)
    for k in (4, -1, 1.5, None):
        with pytest.raises(container.ContainerError, match="frame"):
            cr.frame_container(buf, k)
    for region in [(1, 0, 2, 2), (0, 1, 2, 2), (0, 0, 3, 2), (0, 0, 2, 3), (0, 0, 101, 150), (-2, 0, 4, 4), (0, 0, 0, 2), "all"]:
        with pytest.raises(container.ContainerError, match="admissible|outside|region"):
            cr.decode_clip(None, buf, region=region)
    for level in (1, 2, -2, -3, None, "top"):
        with pytest.raises(container.ContainerError, match="level must be -1 or 0"):
            cr.decode_clip(None, buf, level=level)
    with pytest.raises(ValueError, match="fmt"):
        cr.decode_clip(None, buf, fmt="nv21")
    with pytest.raises(ValueError, match="max_tiles_per_call"):
        cr.decode_clip(None, buf, max_tiles_per_call=0)
    # a tile whose container is for another tile size, holds another number of levels than one, or was coded under another contract
    for bad_blob, msg in [(blob(128, 5, qualities=(0.5,)), "frame 3, tile 4.*128x128"), (blob(T, 5, qualities=(0, 0.75)), "frame 3, tile 4 holds 2 levels"),
                          (blob(T, 5, qualities=(0, 0.5, 10)), "holds 3 levels"), (blob(T, 5, contract=2, qualities=(0.5,)), "frame 3, tile 4: numeric contract")]:
        bl = clip_blobs()
        bl[3][4] = bad_blob
        bad = cr.pack_clip(bl, SOURCE, 100, 150, T, 16, "nv12", "bt709", "limited", "linear", contract=1)
        with pytest.raises(container.ContainerError, match=msg):
            cr.decode_clip(None, bad, frames=[3])
        with pytest.raises(container.ContainerError, match=msg):
            cr.frame_container(bad, 3)
        with pytest.raises(AttributeError):                                          # the frames before it are not touched by it
            cr.decode_clip(None, bad, frames=[0, 1, 2])
    with pytest.raises(container.ContainerError, match="contract"):
        monkeypatch.setattr(container, "build_contract_id", lambda: 2)
        cr.decode_clip(None, buf)
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    # a clip cut off inside its payload still gives every frame whose tiles it holds completely, and refuses the others before the model
    end2 = hd["table"][1][0][0] + hd["table"][1][0][1]                               # frames 0 .. 2 are complete here
    cut = buf[:end2]
    for k in range(3):
        assert cr.frame_container(cut, k) == cr.frame_container(buf, k)
    with pytest.raises(container.ContainerError, match="frame 3, tile 1"):
        cr.frame_container(cut, 3)
    with pytest.raises(container.ContainerError, match="frame 3, tile 1"):
        cr.decode_clip(None, cut)
    with pytest.raises(container.ContainerError, match="frame 1, tile 0"):
        cr.decode_clip(None, buf[:end2 - 1], frames=[1])
    with pytest.raises(AttributeError):                                              # tile (0, 0) of frame 3 is frame 1's
        cr.decode_clip(None, cut, frames=[3], region=(4, 6, 20, 30))
    # nothing above is wrong with a good container: with a model (here: none) the decode goes on to use it
    with pytest.raises(AttributeError):
        cr.decode_clip(None, buf)
    with pytest.raises(AttributeError):
        cr.decode_clip(None, cut, frames=range(3), level=0, fmt="nv12")


def test_decode_groups_by_quality_reuses_and_chunks(monkeypatch):
    """what reaches the model: per frame only the tiles whose entries differ from the frame handled just before, grouped by quality
    (ascending, tile order within a group), max_tiles_per_call at a time; the z strings say which tiles (blob's tag is 16 f + t)"""
    from progressivecodec_amd import clip_rate as cr
    from progressivecodec_amd import clips, container
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    buf, _ = pcs2()
    calls, stitched = [], []

    class Quiet:
        def decompress(self, strings, shape, q, mask_pol):
            tags = [z[0] for z in strings[1]]
            assert all(len(col) == len(tags) for col in strings[0]) and len(strings[0]) == (10 if q == 0 else 20)
            assert all(strings[0][s][i][:1] == bytes([tag]) for s in range(len(strings[0])) for i, tag in enumerate(tags))
            assert tuple(shape) == (1, 1) and mask_pol == "point-based-std"
            calls.append((q, tags))
            return {"x_hat": torch.tensor(tags, dtype=torch.float32).reshape(-1, 1, 1, 1).expand(-1, 3, T, T).contiguous()}

    def stitch(x, g, *a, **k):
        stitched.append(x[:, 0, 0, 0].tolist())
        return x.shape[0]
    monkeypatch.setattr(cr, "stitch_frame", stitch)
    assert cr.decode_clip(Quiet(), buf) == [6] * 4
    # frame 0: q = 0 {1, 4}, q = 0.5 {0, 3, 5}, q = 10 {2}; frame 1: tile 0 (tag 16); frame 2: nothing; frame 3: tiles 1 (49) and 4 (52)
    assert calls == [(0, [1, 4]), (0.5, [0, 3, 5]), (10, [2]), (10, [16]), (0.5, [49]), (10, [52])]
    assert stitched == [[0, 1, 2, 3, 4, 5], [16, 1, 2, 3, 4, 5], [16, 1, 2, 3, 4, 5], [16, 49, 2, 3, 52, 5]]
    del calls[:], stitched[:]
    assert cr.decode_clip(Quiet(), buf, frames=[3, 3, 0, 1], max_tiles_per_call=2, level=0) == [6] * 4
    # frame 3 whole: q 0.5 {1, 3, 5}, q 10 {0, 2, 4}; again: nothing; frame 0: tiles 0, 1, 4; frame 1: tile 0
    assert calls == [(0.5, [49, 3]), (0.5, [5]), (10, [16, 2]), (10, [52]), (0, [1, 4]), (0.5, [0]), (10, [16])]
    assert stitched == [[16, 49, 2, 3, 52, 5]] * 2 + [[0, 1, 2, 3, 4, 5], [16, 1, 2, 3, 4, 5]]
    # a region: only the tiles that cover it -- (60, 60, 8, 8) lies in the bands of tiles 0, 1, 3, 4
    del calls[:], stitched[:]
    assert cr.decode_clip(Quiet(), buf, frames=[0, 3], region=(60, 60, 8, 8), max_tiles_per_call=1) == [4, 4]
    assert calls == [(0, [1]), (0, [4]), (0.5, [0]), (0.5, [3]), (0.5, [49]), (10, [16]), (10, [52])]
    assert stitched == [[0, 1, 3, 4], [16, 49, 3, 52]]
    # PCS1 goes through clips.decode_clip, with every argument
    seen = []
    monkeypatch.setattr(clips, "decode_clip", lambda *a, **k: seen.append((a, k)) or "pcs1")
    old = b"PCS1" + buf[4:]
    assert cr.decode_clip("model", old, frames=[1], level=1, region=(0, 0, 2, 2), fmt="p010", max_tiles_per_call=3) == "pcs1"
    assert seen == [(("model", old), dict(frames=[1], level=1, region=(0, 0, 2, 2), fmt="p010", max_tiles_per_call=3))]
    # tiles of one frame that differ in latent shape or mask policy are refused, a reused tile included
    bl = clip_blobs()
    from progressivecodec_amd import container as ct
    y = [[bytes([52, s])] for s in range(20)]
    bl[3][4] = ct.pack([[y, [bytes([52])]]], (1, 1), [10.0], image_size=(T, T), mask_pol="two-levels", contract=1)
    bad = cr.pack_clip(bl, SOURCE, 100, 150, T, 16, "nv12", "bt709", "limited", "linear", contract=1)
    with pytest.raises(container.ContainerError, match="frame 3, tile 4 was coded as"):
        cr.decode_clip(None, bad, frames=[2, 3])


# -- the library, no device ----------------------------------------------------------------------------------------------------------

def test_library_exports_every_declared_function():
    cr, L = _lib()
    hdr = open(os.path.join(ROOT, "progressivecodec_amd", "clip_rate_csrc", "pc_clip_rate.h")).read()
    declared = re.findall(r"PC_API\s+[\w\s\*]+?\b(pc_\w+)\s*\(", hdr)
    assert len(declared) == 5 and sorted(declared) == sorted(cr.EXPORTS)
    for name in declared:
        getattr(L, name)
    assert L.pc_clip_rate_strerror(-1).decode() and L.pc_clip_rate_strerror(-6).decode() and L.pc_clip_rate_last_hip_error() == 0
    # a library of its own: no other library of the project is linked, and the codec's source hash does not cover it
    import bench
    import inspect
    assert "clip_rate" not in inspect.getsource(bench.source_hash)
    mk = image_shared.build_rule("clip_rate")                                             # image_csrc/lib.mk, which the library's Makefile includes
    assert "-ffp-contract=off" in mk
    assert not re.search(r"-lpc|libpc(odec|_pixels|_tiles|_rate|_metrics|_frames|_frame_tiles|_frame_rate|_clips)\b", mk)
    top = open(os.path.join(ROOT, "progressivecodec_amd", "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\bclip_rate\b", top, re.M) and re.search(r"^\.PHONY:.*\bclip_rate\b", top, re.M)
    assert "$(MAKE) -C ../clip_rate_csrc clean" in top and re.search(r"^clip_rate:\n\t\$\(MAKE\) -C \.\./clip_rate_csrc$", top, re.M)
    # the frame is the one record of image_csrc/pc_yuv_frame.h, as pc_frame_rate.h's and pc_frames.h's are: frames.Frame serves this
    # library, too
    image_shared.assert_frame_is_shared(hdr, "pc_cr_frame")
    image_shared.assert_frame_is_shared(open(os.path.join(ROOT, "progressivecodec_amd", "frame_rate_csrc", "pc_frame_rate.h")).read(), "pc_fr_frame")
    # no atomics, no inline assembly in the kernels
    src = open(os.path.join(ROOT, "progressivecodec_amd", "clip_rate_csrc", "pc_clip_rate.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\batomic(Add|CAS|Exch|Max|Min|Or|And)\b|\basm\b|__asm", code)


def test_workspace_size_is_24_bytes_per_block():
    from progressivecodec_amd import frame_rate
    _, L = _lib()
    for size, n in [(64, 1), (64, 6), (128, 9), (512, 40), (1024, 3), (2048, 2)]:
        assert L.pc_clip_rate_workspace_size(size, n) == 24 * n * (size * size // 4096) == frame_rate.lib().pc_frame_rate_workspace_size(size, n)
    for bad in [(0, 1), (32, 1), (96, 1), (-64, 1), (4096, 1), (64, 0), (64, -1), (2048, 2 ** 31 - 1)]:
        assert L.pc_clip_rate_workspace_size(*bad) == 0, bad


def table_of(frames, fs):
    return (frames.Frame * len(fs))(*fs)


def test_plan_is_host_only_and_each_precondition_is_broken_alone():
    """made-up pointer values: nothing may be dereferenced or launched (there is no GPU here).  Every frame of the table has to
    allow the wide path, wherever in the table it stands."""
    from progressivecodec_amd import frames
    _, L = _lib()
    Fp = 0x7000_0100_0000
    H, W, st = 96, 160, (3 * T * T, T * T, T)

    def plan(fmt, fs, x=Fp, strides=st, O=0, n=None):
        wide = C.c_int(-1)
        tab = table_of(frames, fs) if fs else None
        rc = L.pc_clip_rate_plan(x, *strides, O, frames.FORMATS.get(fmt, fmt), tab, len(fs) if n is None else n, C.byref(wide))
        return rc, wide.value
    for fmt in FC.FORMATS:
        es = 2 if fmt == "p010" else 1
        good = lambda: [fake_frame(frames, fmt, H, W), fake_frame(frames, fmt, H, W, base=0x7100_0000_1000, pad=4),      # noqa: E731
                        fake_frame(frames, fmt, H, W, base=0x7200_0000_1000, pad=8)]
        assert plan(fmt, good()) == (0, 1) and plan(fmt, good()[:1]) == (0, 1)
        for off in (4, 8, 12):
            assert plan(fmt, good(), x=Fp + off) == (0, 0)                            # the floats: 16-byte aligned
        for i in range(3):
            bad_st = list(st)
            bad_st[i] += 2
            assert plan(fmt, good(), strides=bad_st) == (0, 0)                        # and their strides multiples of 4
        for slot in range(3):
            for nm in ["y", "u"] + (["v"] if fmt == "i420" else []):
                for off in (1, 2, 3):
                    fs = good()
                    setattr(fs[slot], nm, getattr(fs[slot], nm) + off * es)           # each plane of each frame: aligned to four elements
                    assert plan(fmt, fs) == (0, 0), (fmt, slot, nm, off)
                    assert plan(fmt, fs[:slot] + fs[slot + 1:]) == (0, 1)             # without that frame the table is wide
                fs = good()
                setattr(fs[slot], nm + "_row", getattr(fs[slot], nm + "_row") + 2)    # each row stride: a multiple of 4
                assert plan(fmt, fs) == (0, 0), (fmt, slot, nm)
                fs = good()
                setattr(fs[slot], nm + "_batch", getattr(fs[slot], nm + "_batch") + 1)                # no batch stride counts
                assert plan(fmt, fs) == (0, 1)
                fs = good()
                setattr(fs[slot], nm, None)
                assert plan(fmt, fs)[0] == -1, (fmt, slot, nm)
        for O, wide in [(0, 1), (8, 1), (16, 1), (32, 1), (4, 0), (12, 0), (20, 0), (28, 0)]:
            assert plan(fmt, good(), O=O) == (0, wide), (fmt, O)
        assert plan(fmt, good(), O=-4)[0] == -1 and plan(fmt, [])[0] == -1 and plan(fmt, good(), n=0)[0] == -1 and plan(fmt, good(), n=-1)[0] == -1
        assert plan(fmt, good(), x=None)[0] == -1
        assert L.pc_clip_rate_plan(Fp, *st, 0, frames.FORMATS[fmt], table_of(frames, good()), 3, None) == -1
    assert plan(3, [fake_frame(frames, "nv12", H, W)])[0] == -1 and plan(-1, [fake_frame(frames, "nv12", H, W)])[0] == -1
    assert plan("nv12", [fake_frame(frames, "nv12", H, W)]) == (0, 1) and plan("i420", [fake_frame(frames, "nv12", H, W)])[0] == -1


def test_every_argument_error_returns_before_the_device():
    """fake device pointers: every call below must return PC_ERR_ARG without touching them (no GPU here)"""
    from progressivecodec_amd import frames
    _, L = _lib()
    Fp, Wk, S, Jb, Tb = 0x7000_0100_0000, 0x7000_0200_0000, 0x7000_0300_0000, 0x7000_0400_0000, 0x7000_0500_0000
    H, W, O = 100, 150, 16                                                            # 2 x 3 tiles, S = 48
    k = frames.coefficients("bt709")
    for fmt in FC.FORMATS:
        fid = frames.FORMATS[fmt]

        def table(slot=None, field=None, value=None):
            fs = [fake_frame(frames, fmt, H, W), fake_frame(frames, fmt, H, W, base=0x7100_0000_1000, pad=3),
                  fake_frame(frames, fmt, H, W, base=0x7200_0000_1000)]
            if slot is not None:
                setattr(fs[slot], field, value)
            return table_of(frames, fs)
        bad_tables = [None]
        for slot in range(3):                                                         # a bad frame anywhere in the table
            bad_tables += [table(slot, "y", None), table(slot, "u", None), table(slot, "y_row", W - 1),
                           table(slot, "u_row", (2 * 75 if fmt != "i420" else 75) - 1)]
            if fmt == "i420":
                bad_tables += [table(slot, "v", None), table(slot, "v_row", 74)]
            if fmt == "p010":
                bad_tables += [table(slot, "y", 0x7000_0000_1001), table(slot, "u", 0x7000_0200_1001)]
        nbytes = L.pc_clip_rate_workspace_size(T, 5)
        ok = dict(x=Fp, sxt=3 * T * T, sxc=T * T, sxh=T, H=H, W=W, T=T, O=O, fmt=fid, range=0, kr=k.kr, kg=k.kg, kb=k.kb, ib=k.ib, ir=k.ir,
                  frames_host=table(), frames_dev=Tb, n_frames=3, jobs=Jb, n_jobs=5, ws=Wk, nbytes=nbytes, out=S, stream=None)
        bads = [dict(frames_host=t) for t in bad_tables] + [
            dict(H=0), dict(W=0), dict(H=-5), dict(T=0), dict(T=32), dict(T=96), dict(T=-64), dict(T=4096, O=0, sxt=3 * 4096 ** 2, sxc=4096 ** 2, sxh=4096),
            dict(O=2), dict(O=6), dict(O=36), dict(O=-4), dict(fmt=3), dict(fmt=-1), dict(range=2), dict(range=-1),
            dict(x=None), dict(x=Fp + 2), dict(sxh=T - 1), dict(sxc=0), dict(sxt=0),
            dict(frames_dev=None), dict(frames_dev=Tb + 4), dict(n_frames=0), dict(n_frames=-1),
            dict(jobs=None), dict(jobs=Jb + 2), dict(n_jobs=0), dict(n_jobs=-1), dict(n_jobs=2 ** 31 - 1),
            dict(ws=None), dict(ws=Wk + 4), dict(out=None), dict(out=S + 4), dict(nbytes=nbytes - 1), dict(nbytes=0)]
        if fmt == "p010":
            bads.append(dict(T=2048, O=0, sxt=3 * 2048 ** 2, sxc=2048 ** 2, sxh=2048, nbytes=L.pc_clip_rate_workspace_size(2048, 5)))
        for bad in bads:
            assert L.pc_clip_rate_sse_jobs(*dict(ok, **bad).values()) == -1, (fmt, {k_: v for k_, v in bad.items() if k_ != "frames_host"})


def test_python_rejects_before_any_device_call(monkeypatch):
    from progressivecodec_amd import clip_rate as cr
    from progressivecodec_amd import clips

    def touched(*a, **k):
        raise AssertionError("the device was reached")
    for name in ("device", "current_stream", "synchronize", "current_device", "_lazy_init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.setattr(cr, "lib", touched)
    monkeypatch.setattr(clips, "lib", touched)
    y, uv, u = torch.zeros(100, 150, dtype=torch.uint8), torch.zeros(50, 75, 2, dtype=torch.uint8), torch.zeros(50, 75, dtype=torch.uint8)
    f = (y, uv)
    g = cr.grid_of(100, 150, 64, 16)
    x = torch.zeros(2, 3, 64, 64)
    # CPU tensors
    with pytest.raises(ValueError, match="GPU"):
        cr.tile_distortion_jobs(x, g, [f, f], [(0, 0), (1, 5)], "nv12")
    with pytest.raises(ValueError, match="GPU"):
        cr.tile_distortion_jobs(x, g, [(y, u, u)], [(0, 0), (0, 5)], "i420")
    with pytest.raises(ValueError, match="GPU"):
        cr.tile_distortion_jobs(x, g, (torch.stack([y, y]), torch.stack([uv, uv])), [(0, 0), (1, 5)], "nv12")
    for kw in (dict(), dict(reuse=False)):
        with pytest.raises(ValueError, match="GPU"):
            cr.encode_clip_to_size(None, [f, f], [0, 1], 10 ** 6, "nv12", tile=64, **kw)
    # enums, the grid and the tile limit come before the frames
    with pytest.raises(ValueError, match="fmt"):
        cr.tile_distortion_jobs(x, g, [f], [(0, 0)], "nv21")
    with pytest.raises(ValueError, match="matrix"):
        cr.tile_distortion_jobs(x, g, [f], [(0, 0)], "nv12", matrix="bt470")
    with pytest.raises(ValueError, match="range"):
        cr.tile_distortion_jobs(x, g, [f], [(0, 0)], "nv12", range="tv")
    with pytest.raises(ValueError, match="the grid of a 100x150 frame is 2x3"):
        cr.tile_distortion_jobs(x, g._replace(nx=4), [f], [(0, 0)], "nv12")
    with pytest.raises(ValueError, match="at most 1024"):
        cr.tile_distortion_jobs(x, cr.grid_of(100, 150, 2048, 0), [f], [(0, 0)], "p010")
    for kw, msg in [(dict(fmt="nv21"), "fmt"), (dict(matrix="bt470"), "matrix"), (dict(range="tv"), "range"), (dict(upsample="cubic"), "upsample"),
                    (dict(max_tiles_per_call=0), "max_tiles_per_call"), (dict(qualities=[]), "at least one level"),
                    (dict(plane_weights=(1, 1)), "plane_weights"), (dict(plane_weights=(0, 0, 0)), "plane_weights"),
                    (dict(plane_weights=(1, 0.5, 1)), "plane_weights"), (dict(plane_weights=(1, -1, 1)), "plane_weights")]:
        a = dict(dict(qualities=[0, 1], target_bytes=10 ** 6, fmt="nv12"), **kw)
        with pytest.raises(ValueError, match=msg):
            cr.encode_clip_to_size(None, [f], a.pop("qualities"), a.pop("target_bytes"), a.pop("fmt"), **a)
    for bad in ([], (), None, "clip"):
        with pytest.raises(ValueError, match="non-empty list"):
            cr.encode_clip_to_size(None, bad, [0], 10 ** 6, "nv12")
    with pytest.raises(ValueError, match="got one frame"):
        cr.encode_clip_to_size(None, f, [0], 10 ** 6, "nv12")


def test_python_checks_that_need_a_frame_that_passes(monkeypatch):
    """the checks behind the frame's own: with the frames' device test out of the way, nothing else may reach the device"""
    from progressivecodec_amd import clip_rate as cr
    from progressivecodec_amd import clips

    def touched(*a, **k):
        raise AssertionError("the device was reached")
    for name in ("device", "current_stream", "synchronize", "current_device", "_lazy_init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.setattr(cr, "lib", touched)
    monkeypatch.setattr(clips, "lib", touched)
    y, uv = torch.zeros(100, 150, dtype=torch.uint8), torch.zeros(50, 75, 2, dtype=torch.uint8)
    f = (y, uv)
    monkeypatch.setattr(cr, "_clip_frames", lambda fr, fmt, what="frames": ([[t.unsqueeze(0) for t in p] for p in fr], fr[0][0].shape[0], fr[0][0].shape[1]))
    g = cr.grid_of(100, 150, 64, 16)
    x = torch.zeros(2, 3, 64, 64)
    # jobs are validated on the host before anything is uploaded
    for bad in ([], [(0, 6), (0, 0)], [(2, 0), (0, 0)], [(-1, 0), (0, 0)], [(0, -1), (0, 0)], [(0, 0), (0.0, 1)], [(0, 0), (True, 1)], [(0, 0), (0,)],
                [(0, 0), 3], [(0, 0), (0, 1, 2)], [(0, 0), ("0", 1)], [(0, 0), None], torch.tensor([[0, 0], [1, 6]])):
        with pytest.raises(ValueError, match="job"):
            cr.tile_distortion_jobs(x, g, [f, f], bad, "nv12")
    with pytest.raises(ValueError, match="one tile per job"):
        cr.tile_distortion_jobs(x, g, [f, f], [(0, 0)], "nv12")
    with pytest.raises(ValueError, match="one tile per job"):
        cr.tile_distortion_jobs(x[0], g, [f, f], [(0, 0)], "nv12")
    small = (torch.zeros(64, 64, dtype=torch.uint8), torch.zeros(32, 32, 2, dtype=torch.uint8))
    with pytest.raises(ValueError, match="frames must be 100x150 frames"):
        cr.tile_distortion_jobs(x[:1], g, [small], [(0, 0)], "nv12")
    enc = lambda **kw: cr.encode_clip_to_size(None, [f, f, f], [0, 1], 10 ** 6, "nv12", **dict(dict(tile=64, overlap=16), **kw))     # noqa: E731
    with pytest.raises(ValueError, match="multiple of 64"):
        enc(tile=96)
    with pytest.raises(ValueError, match="overlap"):
        enc(overlap=6)
    with pytest.raises(ValueError, match="at most 2048"):
        enc(tile=4096, overlap=0)
    with pytest.raises(ValueError, match="at most 1024"):
        cr.encode_clip_to_size(None, [f], [0], 10 ** 6, "p010", tile=2048)
    for imp in ([1] * 5, [[1, 1, 1], [1, 1]], [1] * 7):
        with pytest.raises(ValueError, match="importance needs one number per tile of the 2x3 grid"):
            enc(importance=imp)
    for fw in ([1, 1], [1] * 4, []):
        with pytest.raises(ValueError, match="frame_weights needs one number per frame"):
            enc(frame_weights=fw)

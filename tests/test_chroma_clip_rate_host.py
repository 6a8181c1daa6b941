"""Rate-controlled clips of YUV frames of any subsampling and siting (progressivecodec_amd/chroma_clip_rate.py,
chroma_clip_rate_kernels/pc_chroma_clip_rate.h) without a GPU: the reuse identity per axis, the PCL2 container up
to the model, encode and decode against fake models, every refusal of the module and of the C ABI up to the first device call, the
structure of the sixteenth library and the ledger of its kernels."""
import contextlib
import ctypes as C
import glob
import inspect
import itertools
import os
import re
import struct
import types

import pytest
import torch

from tests import chroma_clip_rate_cases as JS
from tests import chroma_clip_rate_contract as JC
from tests import chroma_clips_contract as CK
from tests import chroma_contract as CC
from tests import image_shared
from tests import rate_contract as RC
from tests import tiles_contract as TC
from tests.test_chroma_clips_host import SOURCE, function_body
from tests.test_chroma_host import fake_frame
from tests.test_clip_rate_host import Q_OF, clip_blobs
from tests.test_image_shared_host import DEFINITIONS
from tests.test_tiles_host import blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "progressivecodec_amd")
DIR = os.path.join(PKG, "chroma_clip_rate_kernels")
T = 64


def _lib():
    """the module and its library; a library that is not built is an ImportError, as for every other one"""
    from progressivecodec_amd import chroma_clip_rate
    return chroma_clip_rate, chroma_clip_rate.lib()


def pcl2(source=SOURCE, H=100, W=150, O=16, fmt="p210", matrix="bt2020", rng="limited", up="linear", siting="left", contract=1):
    cr, _ = _lib()
    blobs = clip_blobs(source, contract)
    return cr.pack_clip(blobs, source, H, W, T, O, fmt, matrix, rng, up, siting, contract=contract), blobs


# -- 1. the reuse identity -------------------------------------------------------------------------------------------------------------

def test_the_footprint_holds_what_the_measure_reads():
    """per axis, over test_chroma_clips_host's axis cases: the samples of the original a job reads (the tile's luma positions and its
    chroma cells, no halo under any siting) lie inside section 25's footprint, for every siting and upsampling"""
    cases = 0
    modes = [(False, False, False), (True, False, False), (True, False, True), (True, True, False), (True, True, True)]
    for TT in (64, 128):
        for O in range(0, TT // 2 + 1, 4):
            S = TT - O
            for L in sorted(set(range(1, 264, 9)) | {2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257}):
                for i in range(TC.axis_tiles(L, TT, O)):
                    for subsampled, linear, cosited in modes:
                        (l0, l1), (c0, c1) = CK.axis_footprint(i, L, TT, O, subsampled, linear, cosited)
                        (m0, m1), (k0, k1) = JC.measured(i, L, TT, O, subsampled)
                        hh = min(TT, L - i * S)
                        assert (m0, m1) == (l0, l1) == (i * S, i * S + hh)
                        # pc_chroma_rate.h: chroma sample k of the tile is the frame's i*S/s + k, k < ceil(hh / s)
                        s = 2 if subsampled else 1
                        assert (k0, k1) == (i * S // s, i * S // s + -(-hh // s) - 1)
                        assert c0 <= k0 <= k1 <= c1, (TT, O, L, i, subsampled, linear, cosited)
                        cases += 1
    assert cases > 10000


# -- 2. PCL2 ---------------------------------------------------------------------------------------------------------------------------

def test_pcl2_is_pcl1_under_its_magic_with_one_level_per_tile():
    from progressivecodec_amd import chroma, chroma_clips, chroma_tiles, clip_rate, container, tiles
    cr, _ = _lib()
    assert cr.MAGIC == JC.MAGIC == b"PCL2" and cr.HEADER_BYTES == JC.HEADER_BYTES == 47 and cr.ENTRY_BYTES == 16
    assert cr.ChromaClipRatePlan._fields == clip_rate.ClipRatePlan._fields + ("sse_exact",)
    for k, (fmt, siting) in enumerate(itertools.product(sorted(chroma.FORMATS), chroma.SITINGS)):
        matrix, rng, up = list(CC.MATRICES)[k % 3], list(CC.RANGES)[k % 2], list(CC.UPSAMPLES)[(k // 2) % 2]
        O = (0, 16)[k % 2]
        blobs = clip_blobs(SOURCE, 7 + k)
        buf = cr.pack_clip(blobs, SOURCE, 100, 150, T, O, fmt, matrix, rng, up, siting, contract=7 + k)
        assert buf == JC.pack_clip(blobs, SOURCE, 100, 150, T, O, fmt, matrix, rng, up, siting, 7 + k)
        assert buf[4:] == chroma_clips.pack_clip(blobs, SOURCE, 100, 150, T, O, fmt, matrix, rng, up, siting, contract=7 + k)[4:]
        hd = cr.parse_clip(buf)
        assert (hd["fmt"], hd["siting"], hd["matrix"], hd["range"], hd["upsample"], hd["contract"], hd["F"]) == (fmt, siting, matrix, rng, up, 7 + k, 4)
        assert hd["grid"] == tiles.grid_of(100, 150, T, O) and hd["payload_start"] == 47 + 16 * 24
        for f, row in enumerate(SOURCE):
            for t, s in enumerate(row):
                tb, th = cr.tile_blob(buf, hd, f, t)
                assert tb == blobs[s][t] and th["qualities"] == [float(Q_OF.get((s, t), 0.5))]
            fc = cr.frame_container(buf, f)
            shown = [blobs[s][t] for t, s in enumerate(row)]
            assert fc == JC.frame_container(shown, 100, 150, T, O, fmt, matrix, rng, up, siting, 7 + k)
            hf = chroma_tiles.parse_frame_tiled(fc)
            assert hf["tiled"]["magic"] == b"PCT2" and hf["tiled"]["contract"] == 7 + k and (hf["fmt"], hf["siting"]) == (fmt, siting)
        with pytest.raises(container.ContainerError, match="not a PCL1"):
            chroma_clips.parse_clip(buf)
        with pytest.raises(container.ContainerError, match="not a PCL2"):
            cr.parse_clip(b"PCL1" + buf[4:])


def test_pcl2_every_malformed_container_raises_before_the_model(monkeypatch):
    from progressivecodec_amd import container
    cr, _ = _lib()
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    buf, blobs = pcl2()
    hd = cr.parse_clip(buf)

    def patched(off, fmt, *vals):
        b = bytearray(buf)
        struct.pack_into(fmt, b, off, *vals)
        return bytes(b)
    entry = lambda f, t: 47 + 16 * (6 * f + t)                                      # noqa: E731
    o00, l00 = hd["table"][0][0]
    # header: magic 0, version 4, layout 5, shift 6, sx 7, sy 8, hsite 9, vsite 10, matrix 11, range 12, upsample 13, bits 14,
    # contract 15, H 19, W 23, T 27, O 31, ny 35, nx 39, F 43
    cases = [(b"PCL3" + buf[4:], "not a PCL2"), (b"PCS2" + buf[4:], "not a PCL2"), (b"", "not a PCL2"), (b"PCL", "not a PCL2"),
             (patched(4, "B", 2), "version"), (patched(4, "B", 0), "version"),
             (patched(5, "B", 2), "corrupt"), (patched(6, "B", 3), "corrupt"), (patched(7, "B", 3), "corrupt"), (patched(8, "B", 3), "corrupt"),
             (patched(9, "B", 2), "corrupt"), (patched(10, "B", 2), "corrupt"), (patched(11, "B", 3), "corrupt"), (patched(12, "B", 2), "corrupt"),
             (patched(13, "B", 2), "corrupt"), (patched(14, "B", 9), "bits"), (patched(14, "B", 8), "corrupt"),
             (patched(19, "<I", 200), "grid"), (patched(23, "<I", 64), "grid"),
             (patched(27, "<I", 96), "corrupt"), (patched(31, "<I", 6), "corrupt"), (patched(31, "<I", 36), "corrupt"),
             (patched(35, "<I", 3), "grid"), (patched(39, "<I", 2), "grid"), (patched(19, "<I", 0), "corrupt"),
             (patched(19, "<I", 2 ** 31), "corrupt"),
             (patched(43, "<I", 0), "no frames"), (patched(43, "<I", 2 ** 32 - 1), "truncated PCL2 table"),
             (buf[:47], "truncated PCL2 table"), (buf[:hd["payload_start"] - 1], "truncated PCL2 table"),
             (patched(entry(1, 1), "<QQ", o00 + 1, l00), "overlaps"), (patched(entry(1, 1), "<QQ", o00, l00 - 1), "overlaps"),
             (patched(entry(3, 5), "<QQ", o00 + l00 - 1, 2), "overlaps"), (patched(entry(2, 2), "<QQ", 0, len(buf)), "overlaps")]
    for n in range(4, 47):
        cases.append((buf[:n], "truncated PCL2 header"))
    for bad, msg in cases:
        with pytest.raises(container.ContainerError, match=msg):
            cr.parse_clip(bad)
        with pytest.raises(container.ContainerError, match=msg):
            cr.decode_clip(None, bad)
        with pytest.raises(container.ContainerError, match=msg):
            cr.frame_container(bad, 0)
    for frames in ([4], [-1], [0, 4], 3, [0.5], ["0"], [None]):
        with pytest.raises(container.ContainerError, match="frame"):
            cr.decode_clip(None, buf, frames=frames)
    for k in (4, -1, 1.5, None):
        with pytest.raises(container.ContainerError, match="frame"):
            cr.frame_container(buf, k)
    for region in [(0, 1, 2, 2), (0, 0, 2, 3), (0, 0, 101, 150), (-2, 0, 4, 4), (0, 0, 0, 2), "all"]:
        with pytest.raises(container.ContainerError, match="admissible|outside|region"):
            cr.decode_clip(None, buf, region=region)
    for level in (1, 2, -2, -3, None, "top"):
        with pytest.raises(container.ContainerError, match="a PCL2 container holds one level per tile: level must be -1 or 0"):
            cr.decode_clip(None, buf, level=level)
    with pytest.raises(ValueError, match="fmt"):
        cr.decode_clip(None, buf, fmt="nv21")
    with pytest.raises(ValueError, match="siting"):
        cr.decode_clip(None, buf, siting="top")
    with pytest.raises(ValueError, match="max_tiles_per_call"):
        cr.decode_clip(None, buf, max_tiles_per_call=0)
    # a tile whose container is for another tile size, holds two levels, or was coded under another contract
    for bad_blob, msg in [(blob(128, 5, qualities=(0.5,)), "frame 3, tile 4.*128x128"), (blob(T, 5, qualities=(0, 0.75)), "frame 3, tile 4 holds 2 levels"),
                          (blob(T, 5, contract=2, qualities=(0.5,)), "frame 3, tile 4: numeric contract")]:
        bl = clip_blobs()
        bl[3][4] = bad_blob
        bad = cr.pack_clip(bl, SOURCE, 100, 150, T, 16, "p210", "bt2020", "limited", "linear", "left", contract=1)
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
    with pytest.raises(AttributeError):                                              # nothing is wrong with a good container
        cr.decode_clip(None, buf)


# -- 3. decode and encode against fake models ------------------------------------------------------------------------------------------

def test_decode_reads_the_halo_s_tiles_groups_by_quality_and_hands_pcl1_down(monkeypatch):
    """what reaches the model: the tiles of covering(halo_window(region)) under the OUTPUT format and siting, per frame only those
    whose entries differ from the frame handled just before, grouped by quality; each byte range once"""
    from progressivecodec_amd import chroma_clips, container
    cr, _ = _lib()
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    buf, _ = pcl2()
    calls, stitched = [], []

    class Quiet:
        def decompress(self, strings, shape, q, mask_pol):
            tags = [z[0] for z in strings[1]]
            assert tuple(shape) == (1, 1) and mask_pol == "point-based-std"
            calls.append((q, tags))
            return {"x_hat": torch.tensor(tags, dtype=torch.float32).reshape(-1, 1, 1, 1).expand(-1, 3, T, T).contiguous()}

    def stitch(x, g, fmt, matrix, rng, siting, window):
        stitched.append((x[:, 0, 0, 0].tolist(), fmt, matrix, rng, siting, window))
        return x.shape[0]
    monkeypatch.setattr(cr, "stitch_frame", stitch)
    assert cr.decode_clip(Quiet(), buf) == [6] * 4
    # frame 0: q = 0 {1, 4}, q = 0.5 {0, 3, 5}, q = 10 {2}; frame 1: tile 0 (tag 16); frame 2: nothing; frame 3: tiles 1 (49) and 4 (52)
    assert calls == [(0, [1, 4]), (0.5, [0, 3, 5]), (10, [2]), (10, [16]), (0.5, [49]), (10, [52])]
    assert [s[0] for s in stitched] == [[0, 1, 2, 3, 4, 5], [16, 1, 2, 3, 4, 5], [16, 1, 2, 3, 4, 5], [16, 49, 2, 3, 52, 5]]
    assert all(s[1:] == ("p210", "bt2020", "limited", "left", (0, 0, 100, 150)) for s in stitched)
    del calls[:], stitched[:]
    assert cr.decode_clip(Quiet(), buf, frames=[3, 3, 0, 1], max_tiles_per_call=2, level=0, fmt="nv12", siting="topleft", region=(2, 2, 96, 146)) == [6] * 4
    assert calls == [(0.5, [49, 3]), (0.5, [5]), (10, [16, 2]), (10, [52]), (0, [1, 4]), (0.5, [0]), (10, [16])]
    assert all(s[1:] == ("nv12", "bt2020", "limited", "topleft", (2, 2, 96, 146)) for s in stitched)
    # the halo of the OUTPUT format and siting chooses the tiles: 2 x 3 tiles at O = 0, S = 64
    buf0, _ = pcl2(O=0, fmt="nv12", siting="left")

    def tiles_of(**kw):
        del calls[:]
        cr.decode_clip(Quiet(), buf0, frames=[0], **kw)
        return sorted(t for _, tags in calls for t in tags)
    assert tiles_of(region=(0, 64, 64, 64)) == [0, 1]                                # the halo column 63 is tile 0's
    assert tiles_of(region=(0, 64, 64, 64), siting="centre") == [1] and tiles_of(region=(0, 64, 64, 64), fmt="i444") == [1]
    assert tiles_of(region=(64, 64, 36, 64)) == [3, 4] and tiles_of(region=(64, 64, 36, 64), siting="topleft") == [0, 1, 3, 4]
    assert tiles_of(region=(64, 0, 36, 64), fmt="nv16", siting="topleft") == [3]
    # PCL1 goes through chroma_clips.decode_clip, with every argument
    seen = []
    monkeypatch.setattr(chroma_clips, "decode_clip", lambda *a, **k: seen.append((a, k)) or "pcl1")
    old = b"PCL1" + buf[4:]
    assert cr.decode_clip("model", old, frames=[1], level=1, region=(0, 0, 2, 2), fmt="p010", siting="left", max_tiles_per_call=3) == "pcl1"
    assert seen == [(("model", old), dict(frames=[1], level=1, region=(0, 0, 2, 2), fmt="p010", siting="left", max_tiles_per_call=3))]


def test_encode_against_a_fake_model(monkeypatch):
    """the items are chunked across frames, one sse_jobs call per level and chunk over the job list uploaded once, the bytes and the
    plan do not depend on the chunking, the budget is target - 47 - 16 F n, and a target below the minimum names it"""
    from progressivecodec_amd import container
    cr, _ = _lib()
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    chunks, measured, asked = [], [], []
    items = [(f, t) for f, row in enumerate(SOURCE) for t, s in enumerate(row) if s == f]
    tags = [16 * f + t for f, t in items]
    assert tags == [0, 1, 2, 3, 4, 5, 16, 49, 52]

    class Model:
        def compress_levels(self, x, qualities, mask_pol):
            chunks.append(list(x))
            return [{"strings": [[[bytes([t, s]) * (1 + (s + t) % 3 + 2 * l) for t in x] for s in range(10 if q == 0 else 20)], [bytes([t]) for t in x]],
                     "shape": (1, 1)} for l, q in enumerate(qualities)]

        def decompress_levels(self, strings, shape, qualities, mask_pol):
            return [{"x_hat": torch.full((len(s[1]), 3, T, T), float(l))} for l, s in enumerate(strings)]

    def source(fs, fmt, siting, g, upsample, reuse):
        asked.append((fmt, siting, upsample, reuse))
        return [list(r) for r in SOURCE] if reuse else [[f] * 6 for f in range(4)]

    def cut_of(fs, g, work, *a):
        assert a == ("p210", "bt2020", "limited", "linear", "left")
        return lambda a_, b_: [16 * f + t for f, t in work[a_:a_ + b_]]

    def sse_jobs_into(L, x, g, fmt, siting, rng, k, host, table, F, jobs_ptr, n, ws, nbytes, out, stream):
        level = int(x[0, 0, 0, 0].item())
        first = (jobs_ptr - djobs_ptr[0]) // 8                                        # the job list of the whole clip, uploaded once
        measured.append((first, n, level, F, nbytes))
        for m in range(n):
            tag = 16 * uploads[-1][first + m][0] + uploads[-1][first + m][1]
            out[m] = torch.tensor([1000 * (3 - level) + tag, 10 * (3 - level), 3 - level])
    djobs_ptr, uploads = [], []
    real_tensor = torch.tensor

    def tensor(data, *a, **k):
        t = real_tensor(data, *a, **k)
        if k.get("dtype") == torch.int32 and t.dim() == 2:
            djobs_ptr[:] = [t.data_ptr()]
            uploads.append(t.tolist())
        return t
    fake_lib = types.SimpleNamespace(pc_chroma_clip_rate_workspace_size=lambda T_, sy, n: 24 * n * (T_ * T_ // (2048 * sy)))
    monkeypatch.setattr(cr, "_clip_frames", lambda frames, fmt: ([[torch.zeros(1)]] * 4, 100, 150))
    monkeypatch.setattr(cr, "_source", source)
    monkeypatch.setattr(cr, "_cut_of", cut_of)
    monkeypatch.setattr(cr, "_frame_table", lambda fs, dev: ("host", torch.zeros(1)))
    monkeypatch.setattr(cr, "_sse_jobs_into", sse_jobs_into)
    monkeypatch.setattr(cr, "lib", lambda: fake_lib)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev: types.SimpleNamespace(cuda_stream=0))
    monkeypatch.setattr(torch, "tensor", tensor)
    kw = dict(matrix="bt2020", siting="left", tile=T, overlap=16)
    outs = []
    for per_call in (1, 4, 32):
        del chunks[:], measured[:], asked[:], uploads[:]
        buf, plan = cr.encode_clip_to_size(Model(), None, [0, 0.5, 10], 10 ** 6, "p210", max_tiles_per_call=per_call, **kw)
        assert chunks == [tags[a:a + per_call] for a in range(0, 9, per_call)] and asked == [("p210", "left", "linear", True)]
        assert measured == [(a, min(per_call, 9 - a), l, 4, 24 * min(per_call, 9) * 2) for a in range(0, 9, per_call) for l in range(3)]
        assert uploads == [[list(it) for it in items]]
        outs.append((buf, plan))
    assert outs[0] == outs[1] == outs[2]
    buf, plan = outs[0]
    assert plan.source == SOURCE and plan.items == items and plan.weights == [1, 3, 4, 4, 3, 4, 3, 1, 1] and plan.den == 32
    assert plan.plane_dists == [[[1000 * (3 - l) + tag, 10 * (3 - l), 3 - l] for l in range(3)] for tag in tags]
    assert plan.dists == [[sum(v) for v in row] for row in plan.plane_dists] and plan.sse_exact is False
    assert (plan.n_coded, plan.n_reused, plan.container_bytes) == (9, 15, len(buf)) and plan.levels == [2] * 9
    hd = cr.parse_clip(buf)
    blobs = [[cr.tile_blob(buf, hd, f, t)[0] if s == f else None for t, s in enumerate(row)] for f, row in enumerate(SOURCE)]
    assert buf == JC.pack_clip(blobs, SOURCE, 100, 150, T, 16, "p210", "bt2020", "limited", "linear", "left", 1)
    assert [len(blobs[f][t]) for f, t in items] == [r[2] for r in plan.rates]
    # the budget arithmetic: 47 bytes of header, 16 per frame and tile
    fixed = 47 + 16 * 4 * 6
    lo, hi = fixed + sum(min(r) for r in plan.rates), fixed + sum(max(r) for r in plan.rates)
    assert hi == len(buf) and lo < hi
    for target in (lo, (lo + hi) // 2, hi - 1, hi):
        b, p = cr.encode_clip_to_size(Model(), None, [0, 0.5, 10], target, "p210", **kw)
        assert p.levels == RC.allocate(plan.rates, plan.dists, target - fixed, plan.weights) and p.levels == RC.allocate(
            plan.rates, plan.dists, JC.budget(target, 4, 6), plan.weights)
        assert len(b) == JC.container_bytes(plan.rates, p.levels, 4, 6) <= target
        assert p.sse == JC.frame_sse(SOURCE, plan.plane_dists, p.levels) and p.predicted == JC.predicted(SOURCE, plan.dists, p.levels)
    with pytest.raises(ValueError, match=rf"target_bytes = {lo - 1} is below the minimum of {lo} bytes: {fixed} bytes of header and table"):
        cr.encode_clip_to_size(Model(), None, [0, 0.5, 10], lo - 1, "p210", **kw)
    # importance and frame weights reach the allocator as exact fractions; without reuse every tile is an item of weight 1
    seen = []
    monkeypatch.setattr(cr.clip_rate, "allocate", lambda rates, dists, budget, weights: seen.append((budget, weights)) or [0] * len(rates))
    cr.encode_clip_to_size(Model(), None, [0, 0.5, 10], hi, "p210", importance=[[1, 2, 3], [4, 5, 6]], frame_weights=[1, 1, 1, 3], **kw)
    assert seen == [(hi - fixed, [1, 2 * 3, 3 * 6, 4 * 6, 5 * 3, 6 * 6, 1 * 5, 2 * 3, 5 * 3])]
    del seen[:]
    _, p = cr.encode_clip_to_size(Model(), None, [0, 0.5, 10], 10 ** 6, "p210", reuse=False, **kw)
    assert seen == [(10 ** 6 - fixed, [1] * 24)] and (p.n_coded, p.n_reused) == (24, 0)


# -- 4. the module's refusals ----------------------------------------------------------------------------------------------------------

def test_python_rejects_before_any_device_call(monkeypatch):
    cr, _ = _lib()

    def touched(*a, **k):
        raise AssertionError("the device was reached")
    for name in ("device", "current_stream", "synchronize", "current_device", "_lazy_init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.setattr(cr, "lib", touched)
    y, uv, u = torch.zeros(100, 150, dtype=torch.uint8), torch.zeros(100, 75, 2, dtype=torch.uint8), torch.zeros(100, 150, dtype=torch.uint8)
    f = (y, uv)
    p = (y.to(torch.uint16), uv.to(torch.uint16))
    x = torch.zeros(2, 3, 64, 64)
    g = cr.grid_of(100, 150, 64, 16)
    for planes, fmt in [(f, "nv16"), ((y, u, u), "i444"), (p, "p210")]:
        with pytest.raises(ValueError, match="GPU"):
            cr.tile_distortion_jobs(x, g, [planes, planes], [(0, 0), (1, 5)], fmt, siting="left")
        with pytest.raises(ValueError, match="GPU"):
            cr.encode_clip_to_size(None, [planes, planes], [0, 1], 10 ** 6, fmt, siting="left", tile=64)
        with pytest.raises(ValueError, match="GPU"):
            cr.encode_clip_to_size(None, tuple(torch.stack([t, t]) for t in planes), [0, 1], 10 ** 6, fmt, tile=64, reuse=False)
    dist = lambda **kw: cr.tile_distortion_jobs(x, g, [f, f], [(0, 0), (1, 5)], **dict(dict(fmt="nv16"), **kw))     # noqa: E731
    enc = lambda **kw: cr.encode_clip_to_size(None, [f], [0], 10 ** 6, **dict(dict(fmt="nv16"), **kw))             # noqa: E731
    for fn in (dist, enc):
        with pytest.raises(ValueError, match="fmt"):
            fn(fmt="nv21")
        with pytest.raises(ValueError, match="matrix"):
            fn(matrix="bt470")
        with pytest.raises(ValueError, match="range"):
            fn(range="tv")
        with pytest.raises(ValueError, match="siting"):
            fn(siting="top")
    with pytest.raises(ValueError, match="upsample"):
        enc(upsample="cubic")
    with pytest.raises(ValueError, match="max_tiles_per_call"):
        enc(max_tiles_per_call=0)
    with pytest.raises(ValueError, match="at least one level"):
        cr.encode_clip_to_size(None, [f], [], 10 ** 6, "nv16")
    with pytest.raises(ValueError, match="plane_weights"):
        enc(plane_weights=(1, 1))
    with pytest.raises(ValueError, match="the grid of a 100x150 frame"):
        cr.tile_distortion_jobs(x, g._replace(ny=3), [f, f], [(0, 0), (1, 5)], "nv16")
    with pytest.raises(ValueError, match="at most 1024"):
        cr.tile_distortion_jobs(x, cr.grid_of(3000, 3000, 2048, 0), [p], [(0, 0)], "p210")
    with pytest.raises(TypeError, match="uint16"):
        dist(fmt="p210")
    for bad in ([], (), None, "clip"):
        with pytest.raises(ValueError, match="non-empty list"):
            cr.tile_distortion_jobs(x, g, bad, [(0, 0)], "nv16")
    with pytest.raises(ValueError, match="got one frame"):
        cr.tile_distortion_jobs(x, g, f, [(0, 0)], "nv16")
    with pytest.raises(ValueError, match="plan|fmt"):
        cr.plan(x, [], "nv21")
    assert issubclass(cr.ChromaClipRateError, cr._imagelib.ImageLibError) and cr.LIB_PATH == os.path.join(PKG, "libpc_chroma_clip_rate.so")
    sig = lambda fn: list(inspect.signature(fn).parameters)                                                           # noqa: E731
    assert sig(cr.tile_distortion_jobs) == ["x_hat_tiles", "grid", "frames", "jobs", "fmt", "matrix", "range", "siting"]
    assert sig(cr.plan) == ["x_hat_tiles", "frames", "fmt", "overlap"]
    assert sig(cr.encode_clip_to_size) == ["model", "frames", "qualities", "target_bytes", "fmt", "matrix", "range", "upsample", "siting", "tile",
                                           "overlap", "mask_pol", "plane_weights", "importance", "frame_weights", "reuse", "max_tiles_per_call"]
    assert sig(cr.decode_clip) == ["model", "buf", "frames", "level", "region", "fmt", "siting", "max_tiles_per_call"]
    d = inspect.signature(cr.encode_clip_to_size).parameters
    assert (d["siting"].default, d["tile"].default, d["overlap"].default, d["reuse"].default, d["max_tiles_per_call"].default) == ("centre", 512, 0, True, 32)


def test_python_checks_that_need_a_frame_that_passes(monkeypatch):
    """the checks behind the frames' own, the jobs' among them with clip_rate's texts: nothing may reach the device"""
    from progressivecodec_amd import clip_rate
    cr, _ = _lib()

    def touched(*a, **k):
        raise AssertionError("the device was reached")
    for name in ("device", "current_stream", "synchronize", "current_device", "_lazy_init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.setattr(cr, "lib", touched)
    y, uv = torch.zeros(100, 150, dtype=torch.uint8), torch.zeros(100, 75, 2, dtype=torch.uint8)
    f = (y, uv)
    monkeypatch.setattr(cr, "_clip_frames", lambda frames, fmt: ([[t.unsqueeze(0) for t in p] for p in frames], 100, 150))
    g = cr.grid_of(100, 150, 64, 16)
    x = torch.zeros(2, 3, 64, 64)
    assert cr.clip_rate._jobs is clip_rate._jobs
    for jobs, msg in [([], "at least one"), ([(0, 0), (2, 0)], r"job \(2, 0\) lies outside the 2 frames or the 2x3 grid"),
                      ([(0, 0), (0, 6)], r"job \(0, 6\) lies outside"), ([(0, 0), (-1, 0)], "lies outside"), ([(0, 0), (0, -1)], "lies outside"),
                      ([(0, 0), (0.0, 1)], "pair of ints"), ([(0, 0), (True, 1)], "pair of ints"), ([(0, 0), (0, 1, 2)], "pair of ints"),
                      ([(0, 0), 3], "pair of ints"), (torch.tensor([[0, 0], [0, 6]]), "lies outside")]:
        with pytest.raises(ValueError, match=msg):
            cr.tile_distortion_jobs(x, g, [f, f], jobs, "nv16")
    with pytest.raises(ValueError, match=r"x_hat_tiles must be a \[3,3,64,64\] tensor, one tile per job"):
        cr.tile_distortion_jobs(x, g, [f, f], [(0, 0), (1, 1), (0, 2)], "nv16")
    with pytest.raises(ValueError, match="x_hat_tiles"):
        cr.tile_distortion_jobs(None, g, [f, f], [(0, 0), (1, 1)], "nv16")
    with pytest.raises((ValueError, TypeError)):
        cr.tile_distortion_jobs(x.double(), g, [f, f], [(0, 0), (1, 1)], "nv16")
    monkeypatch.setattr(cr, "_clip_frames", lambda frames, fmt: ([[t.unsqueeze(0) for t in p] for p in frames], 64, 64))
    with pytest.raises(ValueError, match="frames must be 100x150 frames"):
        cr.tile_distortion_jobs(x, g, [f, f], [(0, 0), (1, 1)], "nv16")
    monkeypatch.setattr(cr, "_clip_frames", lambda frames, fmt: ([[t.unsqueeze(0) for t in p] for p in frames], 100, 150))
    enc = lambda **kw: cr.encode_clip_to_size(None, [f, f], [0], 10 ** 6, "nv16", **dict(dict(tile=64, overlap=16), **kw))     # noqa: E731
    with pytest.raises(ValueError, match="multiple of 64"):
        enc(tile=96)
    with pytest.raises(ValueError, match="overlap"):
        enc(overlap=6)
    with pytest.raises(ValueError, match="at most 2048"):
        enc(tile=4096, overlap=0)
    with pytest.raises(ValueError, match="importance needs one number per tile of the 2x3 grid"):
        enc(importance=[1, 2, 3])
    with pytest.raises(ValueError, match="frame_weights needs one number per frame of the clip, 2 in all"):
        enc(frame_weights=[1])


# -- 5. the library, no device ---------------------------------------------------------------------------------------------------------

def test_workspace_size_is_24_bytes_per_block():
    from progressivecodec_amd import chroma_rate
    _, L = _lib()
    for size, n in [(64, 1), (64, 6), (128, 9), (512, 40), (576, 2), (1024, 3), (2048, 2)]:
        for sy in (1, 2):
            assert L.pc_chroma_clip_rate_workspace_size(size, sy, n) == 24 * n * (size * size // (2048 * sy)) == \
                chroma_rate.lib().pc_chroma_rate_workspace_size(size, sy, n), (size, sy, n)
    for bad in [(0, 1, 1), (32, 1, 1), (96, 2, 1), (-64, 1, 1), (4096, 1, 1), (64, 1, 0), (64, 2, -1), (64, 0, 1), (64, 3, 1), (2048, 1, 2 ** 31 - 1)]:
        assert L.pc_chroma_clip_rate_workspace_size(*bad) == 0, bad


def table_of(fs):
    from progressivecodec_amd import frames
    return (frames.Frame * len(fs))(*fs)


def test_plan_is_host_only_and_each_precondition_is_broken_alone():
    """made-up pointer values: nothing may be dereferenced or launched (there is no GPU here).  Every frame of the table has to
    allow the wide path, wherever in the table it stands: one misaligned frame among aligned ones makes the call narrow."""
    from progressivecodec_amd import chroma
    _, L = _lib()
    Fp = 0x7000_0100_0000
    H, W, st = 96, 160, (3 * T * T, T * T, T)

    def plan(fmt, fs, x=Fp, strides=st, O=0, n=None, **raw):
        wide = C.c_int(-1)
        f = dict(chroma.FORMATS[fmt]._asdict(), **raw)
        tab = table_of(fs) if fs else None
        rc = L.pc_chroma_clip_rate_plan(x, *strides, O, f["layout"], f["bits"], f["sx"], tab, len(fs) if n is None else n, C.byref(wide))
        return rc, wide.value
    for fmt in sorted(chroma.FORMATS):
        f_ = chroma.FORMATS[fmt]
        es = 2 if f_.bits == 10 else 1
        planar = f_.layout == chroma.PLANAR
        good = lambda: [fake_frame(chroma, fmt, H, W), fake_frame(chroma, fmt, H, W, base=0x7100_0000_1000, pad=4),      # noqa: E731
                        fake_frame(chroma, fmt, H, W, base=0x7200_0000_1000, pad=8)]
        assert plan(fmt, good()) == (0, 1) and plan(fmt, good()[:1]) == (0, 1)
        for off in (4, 8, 12):
            assert plan(fmt, good(), x=Fp + off) == (0, 0)                            # the floats: 16-byte aligned
        for i in range(3):
            bad_st = list(st)
            bad_st[i] += 2
            assert plan(fmt, good(), strides=bad_st) == (0, 0)                        # and their strides multiples of 4
        for slot in range(3):
            for nm in ["y", "u"] + (["v"] if planar else []):
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
            if not planar:
                fs = good()
                fs[slot].v = 0x7300_0000_0001                                         # a semi-planar format ignores v
                assert plan(fmt, fs) == (0, 1)
        for O in (0, 8, 16, 32):
            assert plan(fmt, good(), O=O) == (0, 1), (fmt, O)
        for O in (4, 12, 20, 28):                                                    # at sx == 1 every O qualifies
            assert plan(fmt, good(), O=O) == (0, int(f_.sx == 1)), (fmt, O)
        assert plan(fmt, good(), O=-4)[0] == -1 and plan(fmt, [])[0] == -1 and plan(fmt, good(), n=0)[0] == -1 and plan(fmt, good(), n=-1)[0] == -1
        assert plan(fmt, good(), x=None)[0] == -1 and plan(fmt, good(), sx=3)[0] == -1 and plan(fmt, good(), sx=0)[0] == -1
        assert plan(fmt, good(), layout=2)[0] == -1 and plan(fmt, good(), bits=9)[0] == -1 and plan(fmt, good(), bits=16)[0] == -1
        assert L.pc_chroma_clip_rate_plan(Fp, *st, 0, f_.layout, f_.bits, f_.sx, table_of(good()), 3, None) == -1
    assert plan("nv12", [fake_frame(chroma, "nv12", H, W)]) == (0, 1) and plan("i420", [fake_frame(chroma, "nv12", H, W)])[0] == -1


def test_every_argument_error_returns_before_the_device():
    """fake device pointers: every call below must return PC_ERR_ARG without touching them (no GPU here); every argument broken alone"""
    from progressivecodec_amd import chroma
    _, L = _lib()
    Fp, Wk, S, Jb, Tb = 0x7000_0100_0000, 0x7000_0200_0000, 0x7000_0300_0000, 0x7000_0400_0000, 0x7000_0500_0000
    H, W, O = 100, 150, 16                                                            # 2 x 3 tiles, S = 48
    k = chroma.coefficients("bt709")
    for fmt in sorted(chroma.FORMATS):
        f_ = chroma.FORMATS[fmt]
        planar = f_.layout == chroma.PLANAR
        Wc = chroma.chroma_size(H, W, fmt)[1]

        def table(slot=None, field=None, value=None):
            fs = [fake_frame(chroma, fmt, H, W), fake_frame(chroma, fmt, H, W, base=0x7100_0000_1000, pad=3),
                  fake_frame(chroma, fmt, H, W, base=0x7200_0000_1000)]
            if slot is not None:
                setattr(fs[slot], field, value)
            return table_of(fs)
        bad_tables = [None]
        for slot in range(3):                                                         # a bad frame anywhere in the table
            bad_tables += [table(slot, "y", None), table(slot, "u", None), table(slot, "y_row", W - 1),
                           table(slot, "u_row", (Wc if planar else 2 * Wc) - 1)]
            if planar:
                bad_tables += [table(slot, "v", None), table(slot, "v_row", Wc - 1)]
            if f_.bits == 10:
                bad_tables += [table(slot, "y", 0x7000_0000_1001), table(slot, "u", 0x7000_0200_1001)]
        nbytes = L.pc_chroma_clip_rate_workspace_size(T, f_.sy, 5)
        assert nbytes == 24 * 5 * (2 if f_.sy == 1 else 1)
        ok = dict(x=Fp, sxt=3 * T * T, sxc=T * T, sxh=T, H=H, W=W, T=T, O=O, layout=f_.layout, bits=f_.bits, shift=f_.shift, sx=f_.sx, sy=f_.sy,
                  hsite=1, vsite=0, range=0, kr=k.kr, kg=k.kg, kb=k.kb, ib=k.ib, ir=k.ir, frames_host=table(), frames_dev=Tb, n_frames=3, jobs=Jb,
                  n_jobs=5, ws=Wk, nbytes=nbytes, out=S, stream=None)
        big = lambda size: dict(T=size, O=0, sxt=3 * size ** 2, sxc=size ** 2, sxh=size, nbytes=2 ** 40)               # noqa: E731
        bads = [dict(frames_host=t) for t in bad_tables] + [
            dict(H=0), dict(W=0), dict(H=-5), dict(T=0), dict(T=32), dict(T=96), dict(T=-64), big(4096),
            dict(O=2), dict(O=6), dict(O=36), dict(O=-4),
            dict(layout=2), dict(layout=-1), dict(bits=9), dict(bits=16), dict(shift=1), dict(shift=6 if f_.bits == 8 else 4), dict(sx=3),
            dict(sx=0), dict(sy=0), dict(sy=3), dict(sx=1, sy=2), dict(hsite=2), dict(hsite=-1), dict(vsite=2), dict(vsite=-1),
            dict(range=2), dict(range=-1),
            dict(x=None), dict(x=Fp + 2), dict(sxh=T - 1), dict(sxc=0), dict(sxt=0),
            dict(frames_dev=None), dict(frames_dev=Tb + 4), dict(n_frames=0), dict(n_frames=-1),
            dict(jobs=None), dict(jobs=Jb + 2), dict(n_jobs=0), dict(n_jobs=-1), dict(n_jobs=2 ** 31 - 1),
            dict(ws=None), dict(ws=Wk + 4), dict(out=None), dict(out=S + 4), dict(nbytes=nbytes - 1), dict(nbytes=0)]
        if f_.bits == 10:
            bads.append(big(2048))
        for bad in bads:
            assert L.pc_chroma_clip_rate_sse_jobs(*dict(ok, **bad).values()) == -1, (fmt, {k_: v for k_, v in bad.items() if k_ != "frames_host"})
    assert L.pc_chroma_clip_rate_last_hip_error() == 0


# -- 6. structure ----------------------------------------------------------------------------------------------------------------------

def test_the_sixteenth_library_keeps_the_rules_of_the_fifteen():
    cr, L = _lib()
    from progressivecodec_amd import chroma
    hdr = open(os.path.join(DIR, "pc_chroma_clip_rate.h")).read()
    declared = re.findall(r"PC_API\s+[\w\s\*]+?\b(pc_\w+)\s*\(", hdr)
    assert len(declared) == 5 and sorted(declared) == sorted(cr.EXPORTS)
    for name in declared:
        getattr(L, name)
    assert L.pc_chroma_clip_rate_strerror(-1).decode() and L.pc_chroma_clip_rate_strerror(-6).decode() and L.pc_chroma_clip_rate_last_hip_error() == 0
    mk = image_shared.uncommented(os.path.join(DIR, "Makefile"))
    assert mk == "NAME := chroma_clip_rate\ninclude ../image_csrc/lib.mk\n"
    rule = image_shared.uncommented(os.path.join(PKG, "image_csrc", "lib.mk"))
    assert "-ffp-contract=off" in rule and not re.search(r"-lpc|libpc(odec|_\w+)\b", rule)
    top = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\bchroma_clip_rate\b", top, re.M) and re.search(r"^\.PHONY:.*\bchroma_clip_rate\b", top, re.M)
    assert "$(MAKE) -C ../chroma_clip_rate_kernels clean" in top
    assert re.search(r"^chroma_clip_rate:\n\t\$\(MAKE\) -C \.\./chroma_clip_rate_kernels$", top, re.M)
    code_top = image_shared.uncommented(os.path.join(PKG, "csrc", "Makefile"))
    assert len(re.findall(r"\bchroma_clip_rate\b(?!_)", code_top)) == 3 and len(re.findall(r"chroma_clip_rate_kernels", code_top)) == 2
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(DIR, "*")) if not p.endswith((".o", ".so")))
    assert names == ["Makefile", "pc_chroma_clip_rate.h", "pc_chroma_clip_rate.hip"]
    # the pins of the earlier libraries' tests stay true: the directory is neither a *_csrc nor a *_hip, nor chroma_clips_kernels
    assert len(glob.glob(os.path.join(PKG, "*_csrc", "*.hip"))) == len(image_shared.LIBS) == 10
    assert len(glob.glob(os.path.join(PKG, "*_hip", "*.hip"))) == 4 and len(glob.glob(os.path.join(PKG, "*_kernels", "*.hip"))) == 2
    assert len(glob.glob(os.path.join(PKG, "*", "Makefile"))) == 16 + 1                # sixteen image-side libraries and libpcodec
    src = open(os.path.join(DIR, "pc_chroma_clip_rate.hip")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert '#include "pc_image_host.h"' in src and '#include "pc_chroma_sse_item.h"' in src
    for other in ("pc_chroma.h", "pc_chroma_tiles.h", "pc_chroma_rate.h", "pc_chroma_clips.h", "pc_clip_rate.h", "pc_frame_rate.h"):
        assert other not in code, other
    for name, pattern in DEFINITIONS.items():
        assert not re.search(pattern, code), name
    shared = ("HIPCHK", "g_last_hip", "Planes", "planes_of", "Levels", "EmitCoef", "block_reduce", "row_final", "plane_wide", "f32_wide", "aligned",
              "Grid", "geo_of", "axis_weight", "NT", "COLS", "Sum", "Fmt", "format_of", "with_format", "picture_ok", "site_ok", "depth_levels",
              "Measure", "sse_item")
    for name in shared:
        assert re.search(r"\b%s\b" % name, code), name
        assert not re.search(r"\b(struct|void|int|bool|unsigned|float|define|constexpr int)\s+%s\b\s*[({=]" % name, code), name
    for name in ("weighted_row", "emit_px", "load4", "clampi", "code_of"):          # only the item uses them
        assert not re.search(r"\b%s\b" % name, code), name
    image_shared.assert_frame_is_shared(hdr, "pc_ccr_frame")
    found = dict(re.findall(r"\b(PC_CCR_(?:LIMITED|FULL)) = (\w+)", hdr))
    assert found == {"PC_CCR_LIMITED": "PC_YUV_LIMITED", "PC_CCR_FULL": "PC_YUV_FULL"}
    values = dict((k, int(v)) for k, v in re.findall(r"\b(PC_CCR_\w+) = (\d+)", hdr))
    assert values == {"PC_CCR_PLANAR": chroma.PLANAR, "PC_CCR_SEMIPLANAR": chroma.SEMIPLANAR, "PC_CCR_CENTRE": chroma.CENTRE,
                      "PC_CCR_COSITED": chroma.COSITED}
    assert len(re.findall(r"static_assert\(PC_CCR_", code)) == 2
    # plain C++: no inline assembly, no builtins, no atomics, no LDS of its own; 64-bit offsets; two launches
    assert not re.search(r"\batomic(Add|CAS|Exch|Max|Min|Or|And)\b|\basm\b|__asm|__shared__|__syncthreads|__builtin_|__shfl", code)
    assert len(re.findall(r"hipLaunchKernelGGL\(", function_body_of_call(code))) == 2
    # the kernel: the job pair and the frame record through blockIdx alone, the guard outside the reduction's barrier
    body = function_body(src, "sse_jobs_kernel")
    assert "jobs[2 * (int64_t)m]" in body and "planes_of<const T>(frames + slot)" in body
    assert "slot >= 0 && slot < n_frames && tile >= 0 && tile < gr.ny * gr.nx" in body
    assert body.rstrip().endswith("block_reduce<Sum>(su, partials + (int64_t)blockIdx.x * 3);") and "threadIdx" not in body.split("if (slot")[0]
    assert "row_final<Sum, 3>(p, bpt, out);" in function_body(src, "final_kernel")
    import bench
    assert "chroma" not in inspect.getsource(bench.source_hash) and "_kernels" not in inspect.getsource(bench.source_hash)
    from progressivecodec_amd import _imagelib, chroma_clips, chroma_rate, clip_rate
    for word in ("thirteen", "chroma_tiles", "chroma_rate", "chroma_clips", "chroma_clip_rate"):
        assert word in _imagelib.__doc__, word
    assert all("chroma_clip_rate" in m.__doc__ for m in (chroma_clips, chroma_rate, clip_rate))
    # no body is copied: the loops, the items, the checks and the allocation are the earlier modules'
    text = inspect.getsource(cr)
    for call in ("clips._decode(", "_tilecodec.encode_items(", "clip_rate._to_size_arguments(", "clip_rate._allocate_and_pack(", "clip_rate._jobs(",
                 "chroma_clips._parse(buf, MAGIC)", "clips.clip_tile_bytes(buf, hd, k, t, one_level=True)", "chroma_rate.sse_exact("):
        assert call in text, call
    assert "decode_positions" not in text and "import struct" not in text and "allocate(" not in text.replace("_allocate_and_pack(", "")


def function_body_of_call(code):
    """the text of pc_chroma_clip_rate_sse_jobs' definition"""
    start = code.index('extern "C" int pc_chroma_clip_rate_sse_jobs(')
    return code[start:code.index('extern "C" const char*', start)]


def test_the_item_has_one_text_in_two_places():
    """image_csrc/pc_chroma_sse_item.h holds Measure, weighted_row and sse_item word for word as pc_chroma_rate.hip does, until the
    refactoring that deletes the copy there"""
    ours = open(os.path.join(PKG, "image_csrc", "pc_chroma_sse_item.h")).read()
    theirs = open(os.path.join(PKG, "chroma_rate_hip", "pc_chroma_rate.hip")).read()
    for name in ("weighted_row", "sse_item"):
        a, b = function_body(ours, name), function_body(theirs, name)
        assert a == b and len(a) > 1500, name
        head = re.compile(r"template <[^>]*>\n__device__ __forceinline__ void %s\([^{]*\)\n\{" % name)
        assert head.search(ours).group(0) == head.search(theirs).group(0), name
    measure = re.compile(r"struct Measure \{[^}]*\};")
    assert measure.search(ours).group(0) == measure.search(theirs).group(0)
    assert "namespace {" in ours and "__global__" not in re.sub(r"//[^\n]*", "", ours) and "#ifndef PC_CHROMA_SSE_ITEM_H" in ours
    for name in ("emit_px", "load4", "clampi", "code_of"):                          # pc_chroma_rate.hip still uses them, through its copy
        assert re.search(r"\b%s\b" % name, theirs) and re.search(r"\b%s\b" % name, ours), name


def test_the_two_helpers_of_clip_rate_are_unchanged_at_their_defaults(monkeypatch):
    from progressivecodec_amd import clip_rate, clips
    p = inspect.signature(clip_rate._allocate_and_pack).parameters
    assert list(p)[:11] == ["bufs", "dists", "weights", "items", "source", "target_bytes", "g", "fmt", "matrix", "range", "upsample"]
    assert list(p)[11:] == ["header_bytes", "pack"] and p["header_bytes"].default is None and p["pack"].default is None
    q = inspect.signature(clip_rate._to_size_arguments).parameters
    assert list(q)[13:] == ["check_enums", "clip_frames", "grid"] and all(q[n].default is None for n in list(q)[13:])
    # at the defaults: PCS2's 42 bytes, pack_clip, the 4:2:0 checks, clips._clip_frames and clips._grid
    g = clips.grid_of(100, 150, 64, 16)
    items = [(f, t) for f, row in enumerate(SOURCE) for t, s in enumerate(row) if s == f]
    bufs = [[blob(T, 16 * f + t, qualities=(q_,)) for q_ in (0, 0.5)] for f, t in items]
    dists = [[100 + i, 10 + i] for i in range(len(items))]
    fixed = 42 + 16 * 4 * 6
    hi = fixed + sum(len(r[1]) for r in bufs)
    buf, levels, rates = clip_rate._allocate_and_pack(bufs, dists, [1] * 9, items, SOURCE, hi, g, "nv12", "bt709", "limited", "linear")
    assert buf[:4] == b"PCS2" and len(buf) == hi and levels == [1] * 9 and rates == [[len(b) for b in r] for r in bufs]
    blobs = [[bufs[items.index((f, t))][1] if s == f else None for t, s in enumerate(row)] for f, row in enumerate(SOURCE)]
    assert buf == clip_rate.pack_clip(blobs, SOURCE, 100, 150, 64, 16, "nv12", "bt709", "limited", "linear")
    lo = fixed + sum(min(r) for r in rates)
    with pytest.raises(ValueError, match=rf"target_bytes = {lo - 1} is below the minimum of {lo} bytes: {fixed} bytes of header and table"):
        clip_rate._allocate_and_pack(bufs, dists, [1] * 9, items, SOURCE, lo - 1, g, "nv12", "bt709", "limited", "linear")
    seen = []
    out = clip_rate._allocate_and_pack(bufs, dists, [1] * 9, items, SOURCE, hi + 5, g, "p210", "bt709", "limited", "linear", header_bytes=47,
                                       pack=lambda *a: seen.append(a[1:]) or b"packed")
    assert out[0] == b"packed" and seen == [(SOURCE, 100, 150, 64, 16, "p210", "bt709", "limited", "linear")] and out[1] == [1] * 9
    monkeypatch.setattr(clip_rate, "_clip_frames", lambda frames, fmt: (["f0", "f1"], 100, 150))
    a = clip_rate._to_size_arguments("clip", [0, 1], "5000", "nv12", "bt709", "limited", "linear", 64, 16, (1, 2, 3), None, [1, 2], 8)
    assert a == ([0.0, 1.0], 8, [1, 2, 3], 5000, ["f0", "f1"], g, None, [1, 2])
    with pytest.raises(ValueError, match="fmt must be one of"):
        clip_rate._to_size_arguments("clip", [0], 1, "p210", "bt709", "limited", "linear", 64, 16, (1, 1, 1), None, None, 8)
    calls = []
    b = clip_rate._to_size_arguments("clip", [0], 1, "p210", "bt709", "limited", "linear", 64, 16, (1, 1, 1), None, None, 8,
                                     check_enums=lambda *a_: calls.append(a_), clip_frames=lambda fr, fmt: (["g0"], 100, 150),
                                     grid=lambda H, W, t, o: calls.append((H, W, t, o)) or g)
    assert calls == [("p210", "bt709", "limited", "linear"), (100, 150, 64, 16)] and b[4:6] == (["g0"], g)


# -- 7. the ledger ---------------------------------------------------------------------------------------------------------------------

def test_every_instantiation_is_launched():
    """pc_chroma_clip_rate.hip: "32 sse_jobs kernels and the final".  The tuples the table reaches are exactly those; a case taken
    away shows here by the names of the kernels nothing launches any more"""
    src = open(os.path.join(DIR, "pc_chroma_clip_rate.hip")).read()
    assert "32 sse_jobs kernels and the final" in src
    assert len(JS.ALL) == 32
    table = JS.table()
    assert len(table) == 12 * 6 + 4 * 5 and len(set(table)) == len(table)
    got = JS.reached(table)
    assert got == JS.ALL, "never launched: %s" % JS.names(JS.ALL - got)
    assert {(c.fmt, c.siting, c.O) for c in table if (c.H, c.W) == (100, 150) and c.n < 100} == set(itertools.product(CC.FORMATS, CC.SITINGS, (0, 4)))
    assert {(c.fmt, c.H, c.W) for c in table if c.n >= 100} == set((f, H, W) for f in JS.OTHER_FORMATS for H, W in JS.OTHER_SIZES)
    assert {c.O for c in table if c.n >= 100} == {16, 32}
    # the wide rule is over every frame of the table
    assert JS.frames_wide(JS.ALIGNED) and not JS.frames_wide(JS.MIXED) and sum(m == "loose" or o % 4 for m, o in JS.MIXED) == 1
    assert all(not JS.wide(c) for c in table if not c.aligned)
    for fmt in CC.FORMATS:
        assert {JS.wide(c) for c in table if c.fmt == fmt and c.n < 100} == {False, True}
    # the ledger notices a case that leaves
    less = [c for c in table if not (c.fmt == "i010" and c.siting == "topleft" and c.O == 0)]
    gone = JS.ALL - JS.reached(less)
    assert len(gone) == 1 and JS.names(gone) == ["u16 planar 2:2 vco wide"]

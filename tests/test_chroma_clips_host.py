"""Clips of YUV frames of any subsampling and siting without a GPU: the footprint on the restatements alone
(tests/chroma_clips_contract.py against tests/chroma_tiles_contract.cut and tests/chroma_contract.taps, and against
tests/clips_contract.py for centre-sited 4:2:0); the PCL1 container up to the model; encode and decode against fake models;
libpc_chroma_clips.so's C ABI up to the first device call; progressivecodec_amd.chroma_clips' argument checks; the structure of the
fifteenth library and the ledger of its kernels."""
import ctypes as C
import glob
import inspect
import itertools
import os
import re
import struct

import numpy as np
import pytest
import torch

from tests import chroma_clips_cases as CS
from tests import chroma_clips_contract as CK
from tests import chroma_contract as CC
from tests import chroma_tiles_contract as KC
from tests import clips_contract as SC
from tests import frames_contract as FC
from tests import image_shared
from tests import tiles_contract as TC
from tests.test_chroma_host import fake_frame
from tests.test_image_shared_host import DEFINITIONS
from tests.test_tiles_host import blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "progressivecodec_amd")
DIR = os.path.join(PKG, "chroma_clips_kernels")
T = 64


def _lib():
    """the module and its library; a library that is not built is an ImportError, as for every other one"""
    from progressivecodec_amd import chroma_clips
    return chroma_clips, chroma_clips.lib()


def function_body(text, name):
    """the text between the braces of the definition of `name` (the first `name(` that is followed by a body)"""
    m = re.search(r"\bvoid %s\(" % name, text)
    assert m, name
    start = text.index("{", text.index(")\n{", m.end()))
    depth = 0
    for i in range(start, len(text)):
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        if depth == 0:
            return text[start + 1:i]
    raise AssertionError("unbalanced braces")


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def grey(fmt, H, W):
    """the (Y, Cb, Cr) codes of a flat mid-grey frame"""
    mid = 1 << (CC.bits(fmt) - 1)
    Hc, Wc = CC.chroma_size(H, W, fmt)
    return [np.full((1, H, W), mid, np.int64), np.full((1, Hc, Wc), mid, np.int64), np.full((1, Hc, Wc), mid, np.int64)]


# -- 1. the footprint ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["i420", "p210", "nv24"])
@pytest.mark.parametrize("siting", list(CC.SITINGS))
def test_the_footprint_is_sound_and_tight(fmt, siting):
    """one sample of a mid-grey frame changed at a time (no clamp hides a change there), every sample of every plane, against
    chroma_tiles_contract.cut of every tile: outside a tile's footprint the tile keeps its bits, inside it they change.  Two tiles
    along one axis at a time, in frames four samples thin along the other: 66 x 4 at O = 0 and 4 x 66 at O = 32."""
    step = 40 << (CC.bits(fmt) - 8)
    for up in CC.UPSAMPLES:
        for H, W, O in [(66, 4, 0), (4, 66, 32)]:
            ny, nx = TC.grid(H, W, T, O)
            assert ny * nx == 2
            base = grey(fmt, H, W)
            before = KC.cut(CC.frame(*base, fmt), fmt, "bt709", "limited", up, siting, T, O)
            fps = [CK.footprint(t // nx, t % nx, H, W, T, O, fmt, siting, up) for t in range(ny * nx)]
            inside = outside = 0
            for p in range(3):
                for r, q in itertools.product(range(base[p].shape[1]), range(base[p].shape[2])):
                    codes = [np.array(c) for c in base]
                    codes[p][0, r, q] += step
                    after = KC.cut(CC.frame(*codes, fmt), fmt, "bt709", "limited", up, siting, T, O)
                    for t, (lu, ch) in enumerate(fps):
                        box = lu if p == 0 else ch
                        within = box[0] <= r < box[1] and box[2] <= q < box[3]
                        assert same_bits(before[t], after[t]) is not within, (fmt, siting, up, (H, W, O), p, (r, q), t)
                        inside += within
                        outside += not within
            assert inside and outside, (fmt, siting, up, H, W)


def test_the_closed_form_is_the_set_of_non_zero_taps():
    """per axis: the chroma range of pc_chroma_clips.h is exactly the set of chroma samples chroma_contract.taps gives a non-zero
    weight for some luma position of the tile"""
    cases = 0
    modes = [(False, False, False), (True, False, False), (True, False, True), (True, True, False), (True, True, True)]
    for TT in (64, 128):
        for O in range(0, TT // 2 + 1, 4):
            S = TT - O
            for L in sorted(set(range(1, 264, 9)) | {2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257}):
                for i in range(TC.axis_tiles(L, TT, O)):
                    for subsampled, linear, cosited in modes:
                        n = -(-L // 2) if subsampled else L
                        (l0, l1), (c0, c1) = CK.axis_footprint(i, L, TT, O, subsampled, linear, cosited)
                        assert (l0, l1) == (i * S, min(i * S + TT, L)) and l0 < l1
                        read = {j for r in range(l0, l1) for j, w in CC.taps(r, n, subsampled, linear, cosited) if w}
                        assert read == set(range(c0, c1 + 1)), (TT, O, L, i, subsampled, linear, cosited)
                        cases += 1
    assert cases > 10000


def test_the_footprint_in_numbers():
    # 100 x 150, O = 16: S = 48, 2 x 3 tiles; tile (1, 1) holds luma rows 48 .. 99, columns 48 .. 111
    fp = lambda fmt, siting, up: CK.footprint(1, 1, 100, 150, T, 16, fmt, siting, up)                                  # noqa: E731
    assert fp("nv12", "centre", "linear") == ((48, 100, 48, 112), (23, 50, 23, 57))
    assert fp("nv12", "left", "linear") == ((48, 100, 48, 112), (23, 50, 24, 57))          # no chroma column left of the first one
    assert fp("nv12", "topleft", "linear") == ((48, 100, 48, 112), (24, 50, 24, 57))
    assert fp("nv12", "topleft", "nearest") == fp("nv12", "centre", "nearest") == ((48, 100, 48, 112), (24, 50, 24, 56))
    assert fp("p210", "centre", "linear") == ((48, 100, 48, 112), (48, 100, 23, 57))
    assert fp("p210", "left", "linear") == fp("p210", "topleft", "linear") == ((48, 100, 48, 112), (48, 100, 24, 57))
    for siting, up in itertools.product(CC.SITINGS, CC.UPSAMPLES):
        assert fp("i444", siting, up) == ((48, 100, 48, 112), (48, 100, 48, 112))
    # an odd last luma column takes no chroma column after it: the frame has none
    assert CK.footprint(0, 2, 100, 150, T, 16, "nv16", "left", "linear") == ((0, 64, 96, 150), (0, 64, 48, 75))
    assert CK.footprint(0, 0, 1, 1, T, 0, "i010", "topleft", "linear") == ((0, 1, 0, 1), (0, 1, 0, 1))


@pytest.mark.parametrize("fmt", FC.FORMATS)
def test_centre_sited_420_is_section_16(fmt):
    for (H, W), O in itertools.product([(1, 1), (2, 2), (64, 64), (65, 63), (100, 150), (127, 129)], (0, 4, 16, 32)):
        ny, nx = TC.grid(H, W, T, O)
        frames = [FC.random_frame(1, H, W, fmt, seed=H + W + O)]
        g = np.random.default_rng(H * W + O)
        for _ in range(3):
            nxt = tuple(np.array(p) for p in frames[-1])
            for p in nxt:
                flat = p.reshape(-1)
                idx = g.choice(flat.size, min(flat.size, 5), replace=False)
                flat[idx] ^= 0x80 if fmt != "p010" else (0x80 << 6) | 1
            frames.append(nxt)
        frames.append(frames[-1])
        for up in FC.UPSAMPLES:
            for t in range(ny * nx):
                assert CK.footprint(t // nx, t % nx, H, W, T, O, fmt, "centre", up) == SC.footprint(t // nx, t % nx, H, W, T, O, up)
            assert CK.tile_changes(frames[1], frames[0], fmt, "centre", T, O, up) == SC.tile_changes(frames[1], frames[0], fmt, T, O, up)
            assert CK.source_table(frames, fmt, "centre", T, O, up) == SC.source_table(frames, fmt, T, O, up)


def test_a_word_s_other_bits_change_no_code():
    H, W, O = 100, 150, 16
    for fmt in ("p210", "i010"):
        prev = CC.random_frame(1, H, W, fmt, seed=5)
        cur = CC.random_frame(1, H, W, fmt, seed=5, garbage=True)
        assert any((a != b).any() for a, b in zip(cur, prev))
        for siting, up in itertools.product(CC.SITINGS, CC.UPSAMPLES):
            assert CK.tile_changes(cur, prev, fmt, siting, T, O, up) == [[0, 0, 0]] * 6
            assert same_bits(KC.cut(cur, fmt, "bt2020", "full", up, siting, T, O), KC.cut(prev, fmt, "bt2020", "full", up, siting, T, O))


# -- 2. PCL1 -------------------------------------------------------------------------------------------------------------------------

SOURCE = [[0] * 6, [1, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [1, 3, 0, 0, 3, 0]]


def clip_blobs(source=SOURCE, contract=1, T_=T):
    return [[blob(T_, 16 * f + t, contract) if s == f else None for t, s in enumerate(row)] for f, row in enumerate(source)]


def pcl1(source=SOURCE, H=100, W=150, O=16, fmt="p210", matrix="bt2020", rng="limited", up="linear", siting="left", contract=1):
    from progressivecodec_amd import chroma_clips as kc
    blobs = clip_blobs(source, contract)
    return kc.pack_clip(blobs, source, H, W, T, O, fmt, matrix, rng, up, siting, contract=contract), blobs


def test_pcl1_round_trip_aliasing_and_frame_container():
    from progressivecodec_amd import chroma, chroma_tiles, clips, container, tiles
    from progressivecodec_amd import chroma_clips as kc
    assert kc.HEADER_BYTES == CK.HEADER_BYTES == 47 and kc.MAGIC == CK.MAGIC == b"PCL1" and kc.ClipPlan is clips.ClipPlan
    params = itertools.product(sorted(chroma.FORMATS), chroma.SITINGS, CC.MATRICES, CC.RANGES, CC.UPSAMPLES)
    for k, (fmt, siting, matrix, rng, up) in enumerate(params):
        if k % 5:
            continue
        buf, blobs = pcl1(fmt=fmt, matrix=matrix, rng=rng, up=up, siting=siting, contract=7 + k)
        assert buf == CK.pack_clip(blobs, SOURCE, 100, 150, T, 16, fmt, matrix, rng, up, siting, 7 + k)
        assert len(buf) == 47 + 16 * 24 + sum(len(b) for row in blobs for b in row if b is not None)
        f_, (hs, vs) = chroma.FORMATS[fmt], chroma.SITINGS[siting]
        assert tuple(buf[4:15]) == (1, f_.layout, f_.shift, f_.sx, f_.sy, hs, vs, chroma._MATRIX_ID[matrix], chroma.RANGES[rng], chroma.UPSAMPLES[up],
                                    f_.bits) and buf[5:15] == chroma_tiles.pack_frame_tiled(tiles.pack_tiled([blob(T, 0)] * 6, 100, 150, T, 16, contract=1),
                                                                                          fmt, matrix, rng, up, siting)[5:15]
        hd = kc.parse_clip(buf)
        g = hd["grid"]
        assert (hd["fmt"], hd["siting"], hd["matrix"], hd["range"], hd["upsample"], hd["bits"], hd["contract"], hd["F"]) == \
            (fmt, siting, matrix, rng, up, f_.bits, 7 + k, 4)
        assert (g.H, g.W, g.T, g.O, g.ny, g.nx) == (100, 150, T, 16, 2, 3) and hd["payload_start"] == 47 + 16 * 24
        assert kc.parse_clip(bytearray(buf))["table"] == hd["table"] == kc.parse_clip(memoryview(buf))["table"]
        off = hd["payload_start"]
        for f in range(4):
            for t in range(6):
                assert hd["table"][f][t] == hd["table"][SOURCE[f][t]][t]
                if SOURCE[f][t] == f:
                    assert hd["table"][f][t] == (off, len(blobs[f][t]))
                    off += len(blobs[f][t])
                tb, th = kc.clip_tile_bytes(buf, hd, f, t)
                assert tb == blobs[SOURCE[f][t]][t] and th["image_size"] == (T, T)
        assert off == len(buf)
        for f in range(4):
            of_frame = [blobs[SOURCE[f][t]][t] for t in range(6)]
            want = CK.frame_container(of_frame, 100, 150, T, 16, fmt, matrix, rng, up, siting, 7 + k)
            assert kc.frame_container(buf, f) == want
            assert want == chroma_tiles.pack_frame_tiled(tiles.pack_tiled(of_frame, 100, 150, T, 16, contract=7 + k), fmt, matrix, rng, up, siting)
            assert chroma_tiles.parse_frame_tiled(want)["siting"] == siting
    one, b1 = pcl1([[0]], 1, 1, 0)
    assert len(one) == 47 + 16 + len(b1[0][0]) and kc.parse_clip(one)["F"] == 1 and kc.frame_container(one, 0)[15 + 33 + 16:] == b1[0][0]
    for bad in [[[1] * 6], [[0] * 6, [2] * 6], [[0] * 6, [1] * 6, [0] * 6], [[0] * 5], []]:
        with pytest.raises(container.ContainerError):
            kc.pack_clip([[blob(T, 1)] * len(r) for r in bad], bad, 100, 150, T, 16, "nv16", "bt709", "limited", "linear", "left", contract=1)
    with pytest.raises(ValueError, match="fmt"):
        kc.pack_clip(clip_blobs(), SOURCE, 100, 150, T, 16, "nv21", "bt709", "limited", "linear", "left", contract=1)
    with pytest.raises(ValueError, match="siting"):
        kc.pack_clip(clip_blobs(), SOURCE, 100, 150, T, 16, "nv16", "bt709", "limited", "linear", "top", contract=1)
    # PCL1 and PCS1 do not read each other
    pcs = clips.pack_clip(clip_blobs(), SOURCE, 100, 150, T, 16, "nv12", "bt709", "limited", "linear", contract=1)
    with pytest.raises(container.ContainerError, match="not a PCL1"):
        kc.parse_clip(pcs)
    with pytest.raises(container.ContainerError, match="not a PCS1"):
        clips.parse_clip(pcl1()[0])
    # the parser takes the magic: a container that differs in it alone costs nothing
    assert kc._parse(b"PCL2" + pcl1()[0][4:], b"PCL2") == kc.parse_clip(pcl1()[0])


def test_pcl1_every_malformed_container_raises_before_the_model(monkeypatch):
    from progressivecodec_amd import chroma_clips as kc
    from progressivecodec_amd import container
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    buf, blobs = pcl1()
    hd = kc.parse_clip(buf)
    # offsets: 4 version, 5 layout, 6 shift, 7 sx, 8 sy, 9 hsite, 10 vsite, 11 matrix, 12 range, 13 upsample, 14 bits, 15 contract,
    # 19 H, 23 W, 27 T, 31 O, 35 ny, 39 nx, 43 F, 47 the table
    assert tuple(buf[4:15]) == (1, 1, 6, 2, 1, 1, 0, 2, 0, 1, 10) and struct.unpack_from("<8I", buf, 15) == (1, 100, 150, T, 16, 2, 3, 4)

    def patched(off, fmt, *vals):
        b = bytearray(buf)
        struct.pack_into(fmt, b, off, *vals)
        return bytes(b)
    entry = lambda f, t: 47 + 16 * (6 * f + t)                                      # noqa: E731
    o00, l00 = hd["table"][0][0]
    cases = [(b"PCL2" + buf[4:], "not a PCL1"), (b"PCS1" + buf[4:], "not a PCL1"), (b"PCK1" + buf[4:], "not a PCL1"), (b"", "not a PCL1"),
             (b"PCL", "not a PCL1"), (patched(4, "B", 2), "version"), (patched(4, "B", 0), "version"),
             (patched(5, "B", 2), "corrupt"), (patched(5, "B", 0), "corrupt"),                   # planar with shift 6 is none of the twelve
             (patched(6, "B", 0), "corrupt"), (patched(6, "B", 4), "corrupt"), (patched(7, "B", 0), "corrupt"), (patched(7, "B", 4), "corrupt"),
             (patched(8, "B", 0), "corrupt"), (patched(8, "B", 3), "corrupt"), (patched(9, "B", 2), "corrupt"),
             (patched(9, "BB", 0, 1), "corrupt"),                                               # (centre, co-sited) is no siting
             (patched(10, "B", 7), "corrupt"), (patched(11, "B", 3), "corrupt"), (patched(12, "B", 2), "corrupt"), (patched(13, "B", 2), "corrupt"),
             (patched(14, "B", 8), "corrupt"), (patched(14, "B", 12), "bits"), (patched(14, "B", 0), "bits"),
             (patched(19, "<I", 200), "grid"), (patched(23, "<I", 64), "grid"),      # H, W: another grid than the header's ny x nx
             (patched(27, "<I", 96), "corrupt"), (patched(31, "<I", 6), "corrupt"), (patched(31, "<I", 36), "corrupt"),       # T, O
             (patched(35, "<I", 3), "grid"), (patched(39, "<I", 2), "grid"), (patched(19, "<I", 0), "corrupt"),
             (patched(19, "<I", 2 ** 31), "corrupt"),
             (patched(43, "<I", 0), "no frames"), (patched(43, "<I", 2 ** 32 - 1), "truncated PCL1 table"),
             (buf[:47], "truncated PCL1 table"), (buf[:hd["payload_start"] - 1], "truncated PCL1 table"),
             # two entries are either equal or disjoint
             (patched(entry(1, 1), "<QQ", o00 + 1, l00), "overlaps"), (patched(entry(1, 1), "<QQ", o00, l00 - 1), "overlaps"),
             (patched(entry(1, 1), "<QQ", o00, l00 + 1), "overlaps"), (patched(entry(3, 5), "<QQ", o00 + l00 - 1, 2), "overlaps"),
             (patched(entry(2, 2), "<QQ", 0, len(buf)), "overlaps")]
    for n in range(4, 47):
        cases.append((buf[:n], "truncated PCL1 header"))
    for bad, msg in cases:
        with pytest.raises(container.ContainerError, match=msg):
            kc.parse_clip(bad)
        with pytest.raises(container.ContainerError, match=msg):
            kc.decode_clip(None, bad)
        with pytest.raises(container.ContainerError, match=msg):
            kc.frame_container(bad, 0)
    assert kc.parse_clip(patched(entry(3, 5), "<QQ", o00, l00))["table"][3][5] == (o00, l00)
    # refusals that need the frames, the region, the tiles or the level
    for frames in ([4], [-1], [0, 4], 3, [0.5], ["0"], [None]):
        with pytest.raises(container.ContainerError, match="frame"):
            kc.decode_clip(None, buf, frames=frames)
    for k in (4, -1, 1.5, None):
        with pytest.raises(container.ContainerError, match="frame"):
            kc.frame_container(buf, k)
    # 4:2:2 takes every y0 and h, and no odd x0 or w ...
    for region in [(0, 1, 2, 2), (0, 0, 2, 3), (0, 0, 101, 150), (-2, 0, 4, 4), (0, 0, 0, 2), "all"]:
        with pytest.raises(container.ContainerError, match="admissible|outside|region"):
            kc.decode_clip(None, buf, region=region)
    for region in [(1, 0, 2, 2), (0, 0, 3, 2)]:                   # ... which the stored format takes and NV12 does not
        with pytest.raises(container.ContainerError, match="admissible"):
            kc.decode_clip(None, buf, region=region, fmt="nv12")
        with pytest.raises(AttributeError):
            kc.decode_clip(None, buf, region=region)
    for level in (2, -3):
        with pytest.raises(container.ContainerError, match="no level"):
            kc.decode_clip(None, buf, level=level)
    with pytest.raises(ValueError, match="fmt"):
        kc.decode_clip(None, buf, fmt="nv21")
    with pytest.raises(ValueError, match="siting"):
        kc.decode_clip(None, buf, siting="middle")
    with pytest.raises(ValueError, match="max_tiles_per_call"):
        kc.decode_clip(None, buf, max_tiles_per_call=0)
    for bad_blob, msg in [(blob(128, 5), "frame 3, tile 4.*128x128"), (blob(T, 5, qualities=(0, 0.75)), "was coded as"),
                          (blob(T, 5, contract=2), "frame 3, tile 4: numeric contract")]:
        bl = clip_blobs()
        bl[3][4] = bad_blob
        bad = kc.pack_clip(bl, SOURCE, 100, 150, T, 16, "p210", "bt2020", "limited", "linear", "left", contract=1)
        with pytest.raises(container.ContainerError, match=msg):
            kc.decode_clip(None, bad, frames=[3])
        with pytest.raises(AttributeError):                                          # the frames before it are not touched by it
            kc.decode_clip(None, bad, frames=[0, 1, 2])
    with pytest.raises(container.ContainerError, match="contract"):
        monkeypatch.setattr(container, "build_contract_id", lambda: 2)
        kc.decode_clip(None, buf)
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    # a clip cut off inside its payload still gives every frame whose tiles it holds completely, and refuses the others before the model
    end2 = hd["table"][1][0][0] + hd["table"][1][0][1]                               # frames 0 .. 2 are complete here
    cut = buf[:end2]
    for k in range(3):
        assert kc.frame_container(cut, k) == kc.frame_container(buf, k)
    with pytest.raises(container.ContainerError, match="frame 3, tile 1"):
        kc.frame_container(cut, 3)
    with pytest.raises(container.ContainerError, match="frame 3, tile 1"):
        kc.decode_clip(None, cut)
    with pytest.raises(container.ContainerError, match="frame 1, tile 0"):
        kc.decode_clip(None, buf[:end2 - 1], frames=[1])
    with pytest.raises(AttributeError):                                              # tile (0, 0) of frame 3 is frame 1's
        kc.decode_clip(None, cut, frames=[3], region=(4, 6, 20, 30))
    with pytest.raises(AttributeError):                                              # a good container goes on to the model
        kc.decode_clip(None, buf)
    with pytest.raises(AttributeError):
        kc.decode_clip(None, cut, frames=range(3), level=0, fmt="nv12", siting="topleft")


# -- 3. encode and decode against fake models ----------------------------------------------------------------------------------------

def test_decode_reads_the_halo_s_tiles_and_each_byte_range_once(monkeypatch):
    """what reaches the model: the tiles of covering(halo_window(region)) under the OUTPUT format and siting; frame 0 whole, then only
    the tiles whose entries differ from the frame handled just before"""
    from progressivecodec_amd import chroma_clips as kc
    from progressivecodec_amd import container
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    buf, _ = pcl1()
    seen = []

    class Model:
        def decompress(self, strings, shape, q, mask_pol):
            seen.append(([z[0] for z in strings[1]], tuple(shape), q, mask_pol))   # a tile's z string is its tag: 16 * frame + tile
            raise KeyError("far enough")

    def tiles_of(b, **kw):
        del seen[:]
        with pytest.raises(KeyError):
            kc.decode_clip(Model(), b, level=1, **kw)
        assert len(seen) == 1 and seen[0][1:] == ((1, 1), 0.5, "point-based-std")
        return seen[0][0]
    assert tiles_of(buf) == [0, 1, 2, 3, 4, 5] and tiles_of(buf, max_tiles_per_call=4) == [0, 1, 2, 3]
    assert tiles_of(buf, region=(60, 60, 8, 8)) == [0, 1, 3, 4] and tiles_of(buf, frames=[3], region=(4, 6, 20, 30)) == [16]
    assert tiles_of(buf, frames=[3]) == [16, 49, 2, 3, 52, 5]
    buf0, _ = pcl1(O=0, fmt="nv12", siting="left")                                   # 2 x 3 tiles, S = 64
    assert tiles_of(buf0, region=(0, 64, 64, 64)) == [0, 1]                          # the halo column 63 is tile 0's
    assert tiles_of(buf0, region=(0, 64, 64, 64), siting="centre") == [1] and tiles_of(buf0, region=(0, 64, 64, 64), fmt="i444") == [1]
    assert tiles_of(buf0, region=(64, 64, 36, 64)) == [3, 4] and tiles_of(buf0, region=(64, 64, 36, 64), siting="topleft") == [0, 1, 3, 4]
    assert tiles_of(buf0, region=(64, 0, 36, 64), siting="topleft") == [0, 3]
    assert tiles_of(buf0, region=(64, 0, 36, 64), fmt="nv16", siting="topleft") == [3]

    class Quiet:
        calls = []

        def decompress(self, strings, shape, q, mask_pol):
            Quiet.calls.append(len(strings[1]))
            return {"x_hat": torch.zeros(len(strings[1]), 3, T, T)}
    stitched = []
    monkeypatch.setattr(kc, "stitch_frame", lambda x, g, fmt, matrix, rng, siting, window: stitched.append((fmt, matrix, rng, siting, window)) or x.shape[0])
    assert kc.decode_clip(Quiet(), buf) == [6] * 4 and Quiet.calls == [6, 1, 2]
    assert stitched == [("p210", "bt2020", "limited", "left", (0, 0, 100, 150))] * 4
    del Quiet.calls[:], stitched[:]
    assert kc.decode_clip(Quiet(), buf, frames=[3, 3, 0, 1], max_tiles_per_call=2, fmt="nv12", siting="topleft", region=(2, 2, 96, 146)) == [6] * 4
    assert Quiet.calls == [2, 2, 2, 2, 1, 1] and stitched == [("nv12", "bt2020", "limited", "topleft", (2, 2, 96, 146))] * 4


def test_encode_clip_against_a_fake_model(monkeypatch):
    """the work list is chunked across frames, one cut per frame present in a chunk, and the bytes do not depend on the chunking"""
    from progressivecodec_amd import chroma_clips as kc
    from progressivecodec_amd import container
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)
    changed = torch.zeros(3, 6, 3, dtype=torch.int64)
    changed[0, 0, 0], changed[2, 1, 1], changed[2, 4, 2] = 5, 1, 2                   # SOURCE
    chunks, cuts, asked = [], [], []

    class Model:
        def compress_levels(self, x, qualities, mask_pol):
            chunks.append(list(x))
            return [{"strings": [[[bytes([t, s]) * (1 + s % 3) for t in x] for s in range(10 if q == 0 else 20)], [bytes([t]) for t in x]],
                     "shape": (1, 1)} for q in qualities]

    def clip_changes(fs, fmt, siting, g, upsample, first, n):
        asked.append((fmt, siting, upsample, first, n))
        return changed

    def cut_of(fs, g, work, *a):
        def cut(a_, b_):
            pieces = list(kc._tilecodec.frame_pieces(work[a_:a_ + b_]))
            cuts.append([(f, m1 - m0) for f, m0, m1 in pieces])
            return [16 * f + t for f, t in work[a_:a_ + b_]]
        return cut
    monkeypatch.setattr(kc, "_clip_frames", lambda frames, fmt: ([None] * 4, 100, 150))
    monkeypatch.setattr(kc, "_clip_changes", clip_changes)
    monkeypatch.setattr(kc, "_cut_of", cut_of)
    work = [16 * f + t for f, row in enumerate(SOURCE) for t, s in enumerate(row) if s == f]
    assert work == [0, 1, 2, 3, 4, 5, 16, 49, 52]
    outs = []
    kw = dict(matrix="bt2020", siting="left", tile=T, overlap=16)
    for per_call in (1, 4, 32):
        del chunks[:], cuts[:], asked[:]
        buf, plan = kc.encode_clip(Model(), None, [0, 0.5], "p210", max_tiles_per_call=per_call, **kw)
        assert chunks == [work[a:a + per_call] for a in range(0, 9, per_call)] and asked == [("p210", "left", "linear", 0, 6)]
        assert plan == kc.ClipPlan(SOURCE, 9, 15, len(buf))
        outs.append(buf)
    assert cuts == [[(0, 6), (1, 1), (3, 2)]]                                         # one call: one cut per frame present
    assert outs[0] == outs[1] == outs[2]
    hd = kc.parse_clip(outs[0])
    blobs = [[kc.clip_tile_bytes(outs[0], hd, f, t)[0] if s == f else None for t, s in enumerate(row)] for f, row in enumerate(SOURCE)]
    assert outs[0] == CK.pack_clip(blobs, SOURCE, 100, 150, T, 16, "p210", "bt2020", "limited", "linear", "left", 1)
    for f, t in [(0, 0), (1, 0), (3, 4)]:
        strings, shape, qs, _, pol = container.unpack(blobs[f][t], expect_contract=False)
        assert strings[1][1] == [bytes([16 * f + t])] and qs == [0, 0.5] and pol == "point-based-std" and tuple(shape) == (1, 1)
    del asked[:]
    buf, plan = kc.encode_clip(Model(), None, [0, 0.5], "p210", reuse=False, **kw)
    assert not asked and plan.source == [[f] * 6 for f in range(4)] and (plan.n_coded, plan.n_reused) == (24, 0)
    assert all(kc.frame_container(buf, k) == kc.frame_container(outs[0], k) for k in (0,))


# -- 4. the library, no device -------------------------------------------------------------------------------------------------------

def test_workspace_size_is_24_bytes_per_block():
    _, L = _lib()
    for size, n in [(64, 1), (64, 6), (128, 9), (512, 40), (1024, 3), (2048, 2)]:
        for sy in (1, 2):
            assert L.pc_chroma_clips_changes_workspace_size(size, sy, n) == 24 * n * (size * size // (2048 * sy) + 1), (size, sy, n)
    for bad in [(0, 1, 1), (32, 1, 1), (96, 2, 1), (-64, 1, 1), (4096, 1, 1), (64, 1, 0), (64, 2, -1), (64, 0, 1), (64, 3, 1),
                (2048, 1, 2 ** 31 - 1), (2048, 2, 2 ** 21)]:
        assert L.pc_chroma_clips_changes_workspace_size(*bad) == 0, bad


def test_plan_is_host_only_and_each_precondition_is_broken_alone():
    """made-up pointer values: nothing may be dereferenced or launched (there is no GPU here)"""
    kc, L = _lib()
    from progressivecodec_amd import chroma
    Fp = 0x7000_0100_0000
    H, W = 96, 160

    def plan(op, fmt, frame, other=None, f32=Fp, O=0, sx=None):
        wide = C.c_int(-1)
        f = chroma.FORMATS[fmt]
        rc = L.pc_chroma_clips_plan(op, f.layout, f.bits, f.sx if sx is None else sx, C.byref(frame) if frame is not None else None,
                                    C.byref(other) if other is not None else None, f32, O, C.byref(wide))
        return rc, wide.value
    for fmt in sorted(chroma.FORMATS):
        f_ = chroma.FORMATS[fmt]
        es = 2 if f_.bits == 10 else 1
        planar = f_.layout == chroma.PLANAR
        ok = fake_frame(chroma, fmt, H, W)
        ok2 = fake_frame(chroma, fmt, H, W, base=0x7100_0000_1000, pad=4)            # pitched differently
        assert plan(kc.CHANGES, fmt, ok, ok2) == (0, 1) and plan(kc.CUT, fmt, ok) == (0, 1)
        assert plan(kc.CHANGES, fmt, ok, ok2, f32=None) == (0, 1)                     # the changes have no floats
        assert plan(kc.CUT, fmt, ok, None, f32=None)[0] == -1 and plan(kc.CHANGES, fmt, ok, None)[0] == -1
        for off in (4, 8, 12):
            assert plan(kc.CUT, fmt, ok, f32=Fp + off) == (0, 0) and plan(kc.CHANGES, fmt, ok, ok2, f32=Fp + off) == (0, 1)
        for nm in ["y", "u"] + (["v"] if planar else []):
            for off in (1, 2, 3):
                bad = fake_frame(chroma, fmt, H, W)
                setattr(bad, nm, getattr(bad, nm) + off * es)                         # each plane: aligned to four elements
                assert plan(kc.CUT, fmt, bad) == (0, 0) and plan(kc.CHANGES, fmt, bad, ok2) == (0, 0), (fmt, nm, off)
                assert plan(kc.CHANGES, fmt, ok2, bad) == (0, 0), (fmt, nm, off)      # in either frame
                assert plan(kc.CUT, fmt, ok, bad) == (0, 1)                           # the cut has no second frame
            bad = fake_frame(chroma, fmt, H, W)
            setattr(bad, nm + "_row", getattr(bad, nm + "_row") + 2)                  # each row stride: a multiple of 4
            assert plan(kc.CUT, fmt, bad) == (0, 0) and plan(kc.CHANGES, fmt, bad, ok2) == (0, 0) and plan(kc.CHANGES, fmt, ok, bad) == (0, 0)
            free = fake_frame(chroma, fmt, H, W)
            setattr(free, nm + "_batch", getattr(free, nm + "_batch") + 1)            # one frame per call: no batch stride counts
            assert plan(kc.CUT, fmt, free) == (0, 1) and plan(kc.CHANGES, fmt, free, free) == (0, 1)
        for O in (0, 8, 16, 32):
            assert plan(kc.CUT, fmt, ok, O=O) == (0, 1) and plan(kc.CHANGES, fmt, ok, ok2, O=O) == (0, 1), (fmt, O)
        for O in (4, 12, 20, 28):                                                    # at sx == 1 every O qualifies
            assert plan(kc.CUT, fmt, ok, O=O) == (0, int(f_.sx == 1)) and plan(kc.CHANGES, fmt, ok, ok2, O=O) == (0, int(f_.sx == 1)), (fmt, O)
        assert plan(kc.CUT, fmt, ok, O=-4)[0] == -1 and plan(kc.CUT, fmt, None)[0] == -1 and plan(2, fmt, ok, ok2)[0] == -1
        assert plan(-1, fmt, ok, ok2)[0] == -1 and plan(kc.CUT, fmt, ok, sx=3)[0] == -1 and plan(kc.CUT, fmt, ok, sx=0)[0] == -1
        nul = fake_frame(chroma, fmt, H, W)
        nul.u = None
        assert plan(kc.CUT, fmt, nul)[0] == -1 and plan(kc.CHANGES, fmt, ok, nul)[0] == -1
        assert L.pc_chroma_clips_plan(kc.CUT, f_.layout, f_.bits, f_.sx, C.byref(ok), None, Fp, 0, None) == -1
    ok, wide = fake_frame(chroma, "nv12", H, W), C.c_int(-1)
    for layout, bits in [(2, 8), (-1, 8), (0, 9), (1, 12), (1, 16)]:
        assert L.pc_chroma_clips_plan(1, layout, bits, 2, C.byref(ok), None, Fp, 0, C.byref(wide)) == -1
    assert plan(kc.CUT, "nv12", ok) == (0, 1) and plan(kc.CUT, "i420", ok)[0] == -1  # a planar frame needs its V plane


def test_every_argument_error_returns_before_the_device():
    """fake device pointers: every call below must return PC_ERR_ARG without touching them (no GPU here)"""
    kc, L = _lib()
    from progressivecodec_amd import chroma, frames
    Fp, Wk, S, Ix = 0x7000_0100_0000, 0x7000_0200_0000, 0x7000_0300_0000, 0x7000_0400_0000
    H, W, O = 100, 150, 16                                                            # 2 x 3 tiles, S = 48
    k = chroma.coefficients("bt709")
    call = lambda fn, a: fn(*[C.byref(v) if isinstance(v, frames.Frame) else v for v in a.values()])     # noqa: E731
    for fmt in sorted(chroma.FORMATS):
        f_ = chroma.FORMATS[fmt]
        planar = f_.layout == chroma.PLANAR
        Wc = chroma.chroma_size(H, W, fmt)[1]

        def broken(field, value):
            f = fake_frame(chroma, fmt, H, W)
            setattr(f, field, value)
            return f
        bad_frames = [None, broken("y", None), broken("u", None), broken("y_row", W - 1), broken("u_row", (Wc if planar else 2 * Wc) - 1)]
        if planar:
            bad_frames += [broken("v", None), broken("v_row", Wc - 1)]
        if f_.bits == 10:
            bad_frames += [broken("y", fake_frame(chroma, fmt, H, W).y + 1), broken("u", fake_frame(chroma, fmt, H, W).u + 1)]
        fbads = [dict(layout=2), dict(layout=-1), dict(bits=9), dict(bits=16), dict(shift=1), dict(shift=6 if f_.bits == 8 else 4), dict(sx=3),
                 dict(sx=0), dict(sy=0), dict(sy=3), dict(sx=1, sy=2), dict(hsite=2), dict(hsite=-1), dict(vsite=2), dict(vsite=-1)]
        geo = [dict(H=0), dict(W=0), dict(H=-5), dict(T=0), dict(T=32), dict(T=96), dict(T=-64), dict(T=4096, O=0), dict(O=2), dict(O=6),
               dict(O=36), dict(O=-4), dict(up=2), dict(up=-1)]
        fm = dict(layout=f_.layout, bits=f_.bits, shift=f_.shift, sx=f_.sx, sy=f_.sy, hsite=1, vsite=0)

        nbytes = L.pc_chroma_clips_changes_workspace_size(T, f_.sy, 6)
        assert nbytes == 24 * 6 * (3 if f_.sy == 1 else 2)
        ok = dict(cur=fake_frame(chroma, fmt, H, W), prev=fake_frame(chroma, fmt, H, W, base=0x7100_0000_1000), **fm, up=1, H=H, W=W, T=T, O=O,
                  first=0, n=6, ws=Wk, nbytes=nbytes, out=S, stream=None)
        bads = [dict(cur=f) for f in bad_frames] + [dict(prev=f) for f in bad_frames] + fbads + geo + [
            dict(first=-1), dict(first=1), dict(n=0), dict(n=7), dict(n=-1), dict(first=6, n=1), dict(first=2 ** 31 - 1, n=2 ** 31 - 1),
            dict(ws=None), dict(ws=Wk + 4), dict(out=None), dict(out=S + 4), dict(nbytes=nbytes - 1), dict(nbytes=0)]
        for bad in bads:
            assert call(L.pc_chroma_clips_tile_changes, dict(ok, **bad)) == -1, (fmt, bad)

        ok = dict(src=fake_frame(chroma, fmt, H, W), **fm, range=0, up=1, a=k.a, b=k.b, c=k.c, d=k.d, H=H, W=W, T=T, O=O, tiles=Ix, n=4, dst=Fp,
                  stream=None)
        bads = [dict(src=f) for f in bad_frames] + fbads + geo + [dict(range=2), dict(range=-1), dict(tiles=None), dict(tiles=Ix + 2), dict(n=0),
                                                                  dict(n=-1), dict(n=2 ** 31 - 1), dict(dst=None), dict(dst=Fp + 2)]
        for bad in bads:
            assert call(L.pc_chroma_clips_cut_list, dict(ok, **bad)) == -1, (fmt, bad)
    assert L.pc_chroma_clips_last_hip_error() == 0


def test_python_rejects_before_any_device_call(monkeypatch):
    from progressivecodec_amd import chroma_clips as kc

    def touched(*a, **k):
        raise AssertionError("the device was reached")
    for name in ("device", "current_stream", "synchronize", "current_device", "_lazy_init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.setattr(kc, "lib", touched)
    y, uv, u = torch.zeros(100, 150, dtype=torch.uint8), torch.zeros(100, 75, 2, dtype=torch.uint8), torch.zeros(100, 150, dtype=torch.uint8)
    f = (y, uv)
    p = (y.to(torch.uint16), uv.to(torch.uint16))
    for planes, fmt in [(f, "nv16"), ((y, u, u), "i444"), (p, "p210")]:
        with pytest.raises(ValueError, match="GPU"):
            kc.tile_changes(planes, planes, fmt, "left", tile=64)
        with pytest.raises(ValueError, match="GPU"):
            kc.clip_changes([planes, planes], fmt, "left", tile=64)
        with pytest.raises(ValueError, match="GPU"):
            kc.clip_changes(tuple(torch.stack([t, t]) for t in planes), fmt, tile=64)
        with pytest.raises(ValueError, match="GPU"):
            kc.cut_tiles(planes, fmt, [0], siting="topleft", tile=64)
        with pytest.raises(ValueError, match="GPU"):
            kc.encode_clip(None, [planes, planes], [0, 1], fmt, siting="left", tile=64)
        with pytest.raises(ValueError, match="GPU"):
            kc.encode_clip(None, [planes, planes], [0, 1], fmt, tile=64, reuse=False)
    for fn in (lambda **kw: kc.tile_changes(f, f, **dict(dict(fmt="nv16"), **kw)), lambda **kw: kc.clip_changes([f], **dict(dict(fmt="nv16"), **kw))):
        with pytest.raises(ValueError, match="fmt"):
            fn(fmt="nv21")
        with pytest.raises(ValueError, match="upsample"):
            fn(upsample="cubic")
        with pytest.raises(ValueError, match="siting"):
            fn(siting="top")
    with pytest.raises(ValueError, match="matrix"):
        kc.cut_tiles(f, "nv16", [0], matrix="bt470")
    with pytest.raises(ValueError, match="range"):
        kc.cut_tiles(f, "nv16", [0], range="tv")
    with pytest.raises(ValueError, match="siting"):
        kc.cut_tiles(f, "nv16", [0], siting="bottom")
    with pytest.raises(ValueError, match="range"):
        kc.encode_clip(None, [f], [0], "nv16", range="tv")
    with pytest.raises(ValueError, match="siting"):
        kc.encode_clip(None, [f], [0], "nv16", siting="right")
    with pytest.raises(ValueError, match="max_tiles_per_call"):
        kc.encode_clip(None, [f], [0], "nv16", max_tiles_per_call=0)
    with pytest.raises(TypeError, match="uint16"):
        kc.tile_changes(f, f, "p210")
    with pytest.raises(ValueError, match="UV must be"):
        kc.tile_changes((y, uv[:2]), f, "nv16")
    with pytest.raises(ValueError, match="one frame"):
        kc.tile_changes((torch.stack([y, y]), torch.stack([uv, uv])), f, "nv16")
    for bad in ([], (), None, "clip"):
        with pytest.raises(ValueError, match="non-empty list"):
            kc.clip_changes(bad, "nv16")
    with pytest.raises(ValueError, match="got one frame"):
        kc.clip_changes(f, "nv16")
    with pytest.raises(ValueError, match=r"frames\[0\]: UV must be"):
        kc.clip_changes([(y, uv[:2]), f], "nv16")
    assert (kc.CHANGES, kc.CUT) == (0, 1) and issubclass(kc.ChromaClipsError, kc._imagelib.ImageLibError)
    assert kc.LIB_PATH == os.path.join(PKG, "libpc_chroma_clips.so")
    sig = lambda fn: list(inspect.signature(fn).parameters)                                                           # noqa: E731
    assert sig(kc.tile_changes) == ["cur", "prev", "fmt", "siting", "tile", "overlap", "upsample", "first_tile", "n_tiles"]
    assert sig(kc.clip_changes) == ["frames", "fmt", "siting", "tile", "overlap", "upsample", "first_tile", "n_tiles"]
    assert sig(kc.cut_tiles) == ["planes", "fmt", "tile_indices", "matrix", "range", "upsample", "siting", "tile", "overlap", "out"]
    assert sig(kc.encode_clip) == ["model", "frames", "qualities", "fmt", "matrix", "range", "upsample", "siting", "tile", "overlap", "mask_pol",
                                   "reuse", "max_tiles_per_call"]
    assert sig(kc.decode_clip) == ["model", "buf", "frames", "level", "region", "fmt", "siting", "max_tiles_per_call"]
    assert inspect.signature(kc.tile_changes).parameters["siting"].default == "centre"


def test_python_checks_that_need_a_frame_that_passes(monkeypatch):
    """the checks behind the frame's own: with the device test of chroma._frame_view out of the way, nothing else may reach the device"""
    from progressivecodec_amd import chroma_clips as kc

    def touched(*a, **k):
        raise AssertionError("the device was reached")
    for name in ("device", "current_stream", "synchronize", "current_device", "_lazy_init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.setattr(kc, "lib", touched)
    y, uv = torch.zeros(100, 150, dtype=torch.uint8), torch.zeros(100, 75, 2, dtype=torch.uint8)
    small = (torch.zeros(64, 64, dtype=torch.uint8), torch.zeros(64, 32, 2, dtype=torch.uint8))
    monkeypatch.setattr(kc, "_one_frame", lambda p, fmt, what: ([t.unsqueeze(0) for t in p], p[0].shape[0], p[0].shape[1]))
    f = (y, uv)
    with pytest.raises(ValueError, match="prev must be a 100x150 frame"):
        kc.tile_changes(f, small, "nv16", tile=64)
    with pytest.raises(ValueError, match=r"frames\[1\] is 64x64"):
        kc.clip_changes([f, small], "nv16", tile=64)
    for kw in (dict(first_tile=-1), dict(first_tile=6), dict(n_tiles=0), dict(n_tiles=7), dict(first_tile=3, n_tiles=4)):
        with pytest.raises(ValueError, match="outside the 2x3 grid"):
            kc.tile_changes(f, f, "nv16", tile=64, overlap=16, **kw)
        with pytest.raises(ValueError, match="outside the 2x3 grid"):
            kc.clip_changes([f, f], "nv16", tile=64, overlap=16, **kw)
    with pytest.raises(ValueError, match="multiple of 64"):
        kc.tile_changes(f, f, "nv16", tile=96)
    with pytest.raises(ValueError, match="overlap"):
        kc.tile_changes(f, f, "nv16", tile=64, overlap=6)
    with pytest.raises(ValueError, match="at most 2048"):
        kc.tile_changes(f, f, "nv16", tile=4096)
    for bad in ([6], [-1], [0, 1, 6], [0.0], [True], ["1"], [None], [], torch.tensor([2, 7])):
        with pytest.raises(ValueError, match="tile.ind"):
            kc.cut_tiles(f, "nv16", bad, tile=64, overlap=16)
    for out, exc in [(torch.zeros(2, 3, 64, 64, dtype=torch.float64), TypeError), (torch.zeros(3, 3, 64, 64), ValueError),
                     (torch.zeros(2, 3, 64, 65)[..., :64], ValueError), (torch.zeros(4, 3, 64, 64)[::2], ValueError), ("x", TypeError)]:
        with pytest.raises(exc, match="out must be"):
            kc.cut_tiles(f, "nv16", [0, 5], tile=64, overlap=16, out=out)


# -- 5. structure --------------------------------------------------------------------------------------------------------------------

def test_the_fifteenth_library_keeps_the_rules_of_the_fourteen():
    kc, L = _lib()
    from progressivecodec_amd import chroma
    hdr = open(os.path.join(DIR, "pc_chroma_clips.h")).read()
    declared = re.findall(r"PC_API\s+[\w\s\*]+?\b(pc_\w+)\s*\(", hdr)
    assert len(declared) == 6 and sorted(declared) == sorted(kc.EXPORTS)
    for name in declared:
        getattr(L, name)
    assert L.pc_chroma_clips_strerror(-1).decode() and L.pc_chroma_clips_strerror(-6).decode() and L.pc_chroma_clips_last_hip_error() == 0
    mk = image_shared.uncommented(os.path.join(DIR, "Makefile"))
    assert mk == "NAME := chroma_clips\ninclude ../image_csrc/lib.mk\n"
    rule = image_shared.uncommented(os.path.join(PKG, "image_csrc", "lib.mk"))
    assert "-ffp-contract=off" in rule and not re.search(r"-lpc|libpc(odec|_\w+)\b", rule)
    top = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\bchroma_clips\b", top, re.M) and re.search(r"^\.PHONY:.*\bchroma_clips\b", top, re.M)
    assert "$(MAKE) -C ../chroma_clips_kernels clean" in top and re.search(r"^chroma_clips:\n\t\$\(MAKE\) -C \.\./chroma_clips_kernels$", top, re.M)
    assert len(re.findall(r"\bchroma_clips\b(?!_)", image_shared.uncommented(os.path.join(PKG, "csrc", "Makefile")))) == 3
    assert len(re.findall(r"chroma_clips_kernels", image_shared.uncommented(os.path.join(PKG, "csrc", "Makefile")))) == 2
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(DIR, "*")) if not p.endswith((".o", ".so")))
    assert names == ["Makefile", "pc_chroma_clips.h", "pc_chroma_clips.hip"]
    # the pins of the earlier libraries' tests stay true: the directory is neither a *_csrc nor a *_hip
    assert len(glob.glob(os.path.join(PKG, "*_csrc", "*.hip"))) == len(image_shared.LIBS) == 10
    assert len(glob.glob(os.path.join(PKG, "*_hip", "*.hip"))) == 4
    src = open(os.path.join(DIR, "pc_chroma_clips.hip")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert '#include "pc_image_host.h"' in src
    for other in ("pc_chroma.h", "pc_chroma_tiles.h", "pc_clips.h", "pc_frame_tiles.h"):
        assert other not in code, other
    for name, pattern in DEFINITIONS.items():
        assert not re.search(pattern, code), name
    shared = ("HIPCHK", "g_last_hip", "Planes", "planes_of", "load4", "store8", "Levels", "IngestCoef",
              "block_reduce", "row_final", "plane_wide", "aligned", "upsample_ok", "cdiv", "Grid", "geo_of", "NT", "COLS", "Sum",
              "ingest_item", "Taps", "taps_of", "code_of", "Fmt", "format_of", "with_format", "picture_ok", "site_ok", "depth_levels")
    for name in shared:
        assert re.search(r"\b%s\b" % name, code), name
        assert not re.search(r"\b(struct|void|int|bool|unsigned|float|define|constexpr int)\s+%s\b\s*[({=]" % name, code), name
    image_shared.assert_frame_is_shared(hdr, "pc_chc_frame")
    found = dict(re.findall(r"\b(PC_CHC_(?:LIMITED|FULL|NEAREST|LINEAR)) = (\w+)", hdr))
    assert found == {"PC_CHC_" + k: "PC_YUV_" + k for k in ("LIMITED", "FULL", "NEAREST", "LINEAR")}
    assert "PC_YUV_" not in re.sub(r"PC_YUV_(LIMITED|FULL|NEAREST|LINEAR|NV12|P010)\b", "", hdr + code)
    values = dict((k, int(v)) for k, v in re.findall(r"\b(PC_CHC_\w+) = (\d+)", hdr))
    assert values == {"PC_CHC_PLANAR": chroma.PLANAR, "PC_CHC_SEMIPLANAR": chroma.SEMIPLANAR, "PC_CHC_CENTRE": chroma.CENTRE,
                      "PC_CHC_COSITED": chroma.COSITED, "PC_CHC_CHANGES": kc.CHANGES, "PC_CHC_CUT": kc.CUT}
    # the cut kernel differs from pc_chroma_tiles.hip's cut_kernel in where the tile comes from alone: the same item (the shared header's),
    # the same guard, the same stores
    theirs = open(os.path.join(PKG, "chroma_tiles_hip", "pc_chroma_tiles.hip")).read()
    for line in ("if (item >= items) return;", "ingest_item<T, IL, SX, SY, WIDE>(s, W, Hc, Wc, (int)Y64, (int)X64, t, lv, k, o);", "store8<WIDE>(dst + ("):
        assert line in function_body(src, "cut_list_kernel") and line in function_body(theirs, "cut_kernel")
    # plain C++: no inline assembly, no builtins, no atomics, no LDS of its own
    assert not re.search(r"\batomic(Add|CAS|Exch|Max|Min|Or|And)\b|\basm\b|__asm|__shared__|__syncthreads|__builtin_|__shfl", code)
    import bench
    assert "chroma" not in inspect.getsource(bench.source_hash) and "_kernels" not in inspect.getsource(bench.source_hash)
    from progressivecodec_amd import _imagelib, chroma_tiles, clips
    for word in ("thirteen", "chroma_tiles", "chroma_rate", "chroma_clips"):
        assert word in _imagelib.__doc__, word
    assert "chroma_clips" in clips.__doc__ and "chroma_clips" in chroma_tiles.__doc__
    # one decode loop: this module's decode is clips._decode with the two hooks, not a copy
    text = inspect.getsource(kc.decode_clip)
    assert "clips._decode(" in text and "window_of=" in text and "covering_of=" in text and "decode_positions" not in inspect.getsource(kc)
    params = inspect.signature(clips._decode).parameters
    assert params["window_of"].default is None and params["covering_of"].default is None


# -- 6. the ledger -------------------------------------------------------------------------------------------------------------------

def test_every_instantiation_is_launched():
    """pc_chroma_clips.hip: "24 changes kernels, 24 cut kernels".  The tuples the table reaches are exactly those; a case taken away
    shows here by the names of the kernels nothing launches any more"""
    src = open(os.path.join(DIR, "pc_chroma_clips.hip")).read()
    assert "24 changes kernels, 24 cut kernels and the final" in src
    assert len(CS.ALL_KERNELS) == 24
    table = CS.table()
    assert len(table) == 12 * 12 + 4 * 6 and len(set(table)) == len(table)
    got = CS.reached(table)
    assert got == CS.ALL_KERNELS, "never launched: %s" % CS.names(CS.ALL_KERNELS - got)
    # the cases the issue names
    assert {(c.fmt, c.siting, c.upsample, c.O) for c in table if (c.H, c.W) == (100, 150) and c.n < 100} == \
        set(itertools.product(CC.FORMATS, CC.SITINGS, CC.UPSAMPLES, (0, 4)))
    assert {(c.fmt, c.H, c.W) for c in table if c.n >= 100} == set((f, H, W) for f in CS.OTHER_FORMATS for H, W in CS.OTHER_SIZES)
    assert {c.O for c in table if c.n >= 100} == {16, 32}
    for fmt in CC.FORMATS:                                          # O = 4 is narrow at sx == 2, whatever the views
        assert {CS.wide(c, True) for c in table if c.fmt == fmt and c.n < 100 and c.O == 4} == {CC.sub(fmt)[0] == 1}
        assert {CS.wide(c, a) for c in table if c.fmt == fmt and c.n < 100 for a in CS.ALIGNMENTS} == {False, True}
    # the ledger notices a case that leaves
    less = [c for c in table if not (c.fmt == "i010" and c.O == 0)]
    assert CS.ALL_KERNELS - CS.reached(less) == {(2, False, 2, 2, True)} and CS.names([(2, False, 2, 2, True)]) == ["u16 planar 2:2 wide"]

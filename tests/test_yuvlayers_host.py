"""progressivecodec_amd._yuvlayers without a GPU: the two Family descriptors against each other where they
describe the same formats, the ten-byte sited header of PCH1 / PCK1 / PCL1 through its one packer and its one parser, and the
covering of a window with and without a halo."""
import itertools
import re

import pytest
import torch

YUV420 = ["nv12", "i420", "p010"]
NAMES = ["PCH1", "PCK1", "PCL1"]


def windows(H, W):
    """every window inside an H x W frame"""
    return [(y0, x0, h, w) for y0 in range(H) for h in range(1, H - y0 + 1) for x0 in range(W) for w in range(1, W - x0 + 1)]


# -- (a) the format table ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", YUV420)
def test_the_two_families_describe_the_420_formats_alike(fmt):
    from progressivecodec_amd import _yuvlayers as yl
    from progressivecodec_amd import chroma, chroma_tiles, frame_tiles, frames
    a, b = frames.FAMILY, chroma.FAMILY
    assert a.formats[fmt] == b.formats[fmt] == chroma.FORMATS[fmt]
    assert set(a.formats) == set(frames.FORMATS) == set(YUV420)
    assert frames.bits_of(fmt) == chroma.bits_of(fmt) == a.formats[fmt].bits
    n = 3 if fmt == "i420" else 2
    for fam, view in ((a, frames._frame_view), (b, chroma._frame_view)):
        with pytest.raises(ValueError, match=rf"^planes must be a tuple of {n} planes for '{fmt}': "):
            view((torch.zeros(4, 4),) * (5 - n), fmt, "planes")
        planes = yl.empty_frame(fam, fmt, 1, 5, 7, "cpu")
        assert len(planes) == n and {t.dtype for t in planes} == {torch.uint16 if fmt == "p010" else torch.uint8}
    for h, w in itertools.product(range(1, 9), range(1, 9)):
        assert frames.chroma_size(h, w) == chroma.chroma_size(h, w, fmt) == ((h + 1) // 2, (w + 1) // 2)
        for fam in (a, b):
            assert tuple(yl.empty_frame(fam, fmt, 1, h, w, "cpu")[1].shape[1:3]) == ((h + 1) // 2, (w + 1) // 2)
    seen = 0
    for H, W in ((5, 7), (6, 8)):
        for win in windows(H, W):
            y0, x0, h, w = win
            want = y0 % 2 == 0 and x0 % 2 == 0 and (h % 2 == 0 or y0 + h == H) and (w % 2 == 0 or x0 + w == W)
            assert frame_tiles.admissible(win, H, W) == chroma_tiles.admissible(win, H, W, fmt) == want, (win, H, W)
            for refused, ask in ((frame_tiles._admissible_window, (win, H, W)), (chroma_tiles._admissible_window, (win, H, W, fmt))):
                if want:
                    assert refused(*ask) == win
                else:
                    with pytest.raises(ValueError, match="is not admissible: "):
                        refused(*ask)
            seen += 1
    assert seen == 15 * 28 + 21 * 36


def test_a_family_is_plain_data_of_at_most_a_dozen_fields():
    from progressivecodec_amd import _yuvlayers as yl
    from progressivecodec_amd import chroma, frames
    assert len(yl.Family._fields) <= 12
    for fam, stack in ((frames.FAMILY, ("frames", "frame_tiles", "frame_rate")), (chroma.FAMILY, ("chroma", "chroma_tiles", "chroma_rate"))):
        assert tuple(name for name, _ in fam.owners) == stack
        for layer in (yl.FRAME, yl.TILED, yl.RATE):
            mod, err, symbols = yl._layer(fam, layer)
            assert all(name == f"pc_{stack[layer]}_{verb}" for verb, name in symbols.items()) and set(mod.EXPORTS) - set(symbols.values()) \
                == {f"pc_{stack[layer]}_strerror", f"pc_{stack[layer]}_last_hip_error"}
            assert mod.__name__ == f"progressivecodec_amd.{stack[layer]}" and err._prefix == f"pc_{stack[layer]}" and err._lib is mod.lib


def test_a_replaced_lib_is_the_one_a_shared_body_calls(monkeypatch):
    from progressivecodec_amd import _yuvlayers as yl
    from progressivecodec_amd import chroma, chroma_tiles, frame_tiles, frames

    class Touched(Exception):
        pass

    def touched():
        raise Touched
    for fam, mod in ((frames.FAMILY, frame_tiles), (chroma.FAMILY, chroma_tiles)):
        monkeypatch.setattr(mod, "lib", touched)
        with pytest.raises(Touched):
            yl.tiled_plan(fam, mod.CUT, None, "nv12", torch.zeros(1, 3, 64, 64), 0, 0, None)


# -- (b), (c) the sited header -----------------------------------------------------------------------------------------------------------

def test_sited_params_round_trips_sited_head():
    from progressivecodec_amd import _tilecodec as tc
    from progressivecodec_amd import chroma, frames
    n = 0
    for fmt, siting, matrix, rng, up in itertools.product(chroma.FORMATS, chroma.SITINGS, frames.MATRICES, frames.RANGES, frames.UPSAMPLES):
        head = tc.sited_head(fmt, matrix, rng, up, siting)
        assert len(head) == 10 and all(isinstance(v, int) and 0 <= v < 256 for v in head)
        f, (hs, vs) = chroma.FORMATS[fmt], chroma.SITINGS[siting]
        assert head[:6] == (f.layout, f.shift, f.sx, f.sy, hs, vs) and head[9] == f.bits
        assert tc.sited_params(*head, "PCK1") == {"fmt": fmt, "siting": siting, "matrix": matrix, "range": rng, "upsample": up, "bits": f.bits}
        n += 1
    assert n == 12 * 3 * 3 * 2 * 2


@pytest.mark.parametrize("name", NAMES)
def test_sited_params_refuses_every_corrupted_byte(name):
    from progressivecodec_amd import _tilecodec as tc
    from progressivecodec_amd.container import ContainerError
    good = tc.sited_head("p210", "bt709", "limited", "linear", "left")
    assert tc.sited_params(*good, name)["fmt"] == "p210"
    for at, bad in itertools.product(range(10), (77, 255)):
        v = list(good)
        v[at] = bad
        lay, sh, sx, sy, hs, vs, m, r, u, bits = v
        text = f"corrupt {name} header: {bits} bits" if at == 9 else \
            f"corrupt {name} header: layout {lay}, shift {sh} at {bits} bits, subsampling {sx}x{sy}, siting {hs}, {vs}, matrix {m}, range {r}, upsample {u}"
        with pytest.raises(ContainerError, match="^" + re.escape(text) + "$"):
            tc.sited_params(*v, name)
    lay, sh, sx, sy, hs, vs, m, r, u, _ = good                                   # a depth that exists, for a format that has another
    with pytest.raises(ContainerError, match="^" + re.escape(f"corrupt {name} header: layout {lay}, shift {sh} at 8 bits, subsampling {sx}x{sy}, ")):
        tc.sited_params(lay, sh, sx, sy, hs, vs, m, r, u, 8, name)


def test_the_three_sited_containers_refuse_through_sited_params(monkeypatch):
    """PCH1, PCK1 and PCL1 hand their ten bytes to the one parser: a corrupted byte in a real container gives its text"""
    from progressivecodec_amd import chroma, chroma_clips, chroma_tiles
    from progressivecodec_amd.container import ContainerError
    from tests.test_frames_host import pcb1
    pch = bytearray(chroma.pack_frame(pcb1(6, 10), "nv16", "bt709", "limited", "linear", "left", 6, 10))
    pch[4 + 1 + 9] = 9
    with pytest.raises(ContainerError, match="^corrupt PCH1 header: 9 bits$"):
        chroma.parse_frame(bytes(pch))
    for mod, parse, magic in ((chroma_tiles, chroma_tiles.parse_frame_tiled, b"PCK1"), (chroma_clips, chroma_clips.parse_clip, b"PCL1")):
        head = magic + bytes([1, 0, 0, 2, 3, 0, 0, 1, 0, 1, 8]) + bytes(mod.HEADER_BYTES)
        with pytest.raises(ContainerError, match=f"^corrupt {magic.decode()} header: layout 0, shift 0 at 8 bits, subsampling 2x3, siting 0, 0, matrix 1, "):
            parse(head)


# -- (d) the halo ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("O", [0, 16])
def test_covering_without_a_halo_is_the_grids(O):
    """100 x 150, T = 64, admissible windows whose origin lies on the 2-pixel lattice: 1275 row intervals times 2850 column
    intervals, 3.6 million windows and minutes of calls, so the product is not walked whole.  What is asserted instead:

      1. no halo at "centre": halo_window(chroma.FAMILY, win, fmt, "centre") is win -- the one thing in which the chroma family's
         covering could differ from the grid's -- for every row interval with every column ORIGIN (the halo depends on a window's
         origin and never on how far it reaches), and the 4:2:0 family has no halo function at all;
      2. the covering is separable: the tile rows of covering(win) depend on (y0, h) alone and its tile columns on (x0, w) alone,
         checked on 20 000 windows drawn from the whole product against the two one-axis answers;
      3. so the cross -- every row interval with four column intervals and every column interval with four row intervals -- carries
         the equality of the three coverings to the product."""
    import random
    from progressivecodec_amd import _yuvlayers as yl
    from progressivecodec_amd import chroma, frames, tiles
    H, W, T = 100, 150, 64
    g = tiles.grid_of(H, W, T, O)
    rows = [(y0, h) for y0 in range(0, H, 2) for h in range(2, H - y0 + 1, 2)]
    cols = [(x0, w) for x0 in range(0, W, 2) for w in range(2, W - x0 + 1, 2)]
    assert (len(rows), len(cols)) == (1275, 2850)
    assert frames.FAMILY.halo is None
    for (y0, h), x0, fmt in itertools.product(rows, range(0, W, 2), YUV420):                                     # 1.
        assert chroma.FAMILY.halo((y0, x0, h, 2), fmt, "centre") == (y0, x0, h, 2)
    by_row = {r: g.covering((r[0], 0, r[1], W)) for r in rows}
    by_col = {c: g.covering((0, c[0], H, c[1])) for c in cols}
    rnd = random.Random(O)
    for _ in range(20000):                                                                                     # 2.
        (y0, h), (x0, w) = rnd.choice(rows), rnd.choice(cols)
        want = (by_row[y0, h][0], by_col[x0, w][1], by_row[y0, h][2], by_col[x0, w][3])
        assert g.covering((y0, x0, h, w)) == want == yl.covering(chroma.FAMILY, g, (y0, x0, h, w), "nv12", "centre")
    some_rows, some_cols = [(0, H), (T - O, 36), (62, 4), (H - 2, 2)], [(0, W), (T - O, 52), (62, 4), (W - 2, 2)]
    cross = {(y0, x0, h, w) for (y0, h), (x0, w) in itertools.chain(itertools.product(rows, some_cols), itertools.product(some_rows, cols))}
    for win in cross:                                                                                          # 3.
        want = g.covering(win)
        assert yl.covering(frames.FAMILY, g, win, "nv12", None) == want, win
        for fmt in YUV420:
            assert yl.covering(chroma.FAMILY, g, win, fmt, "centre") == want, (win, fmt)
    assert yl.halo_window(frames.FAMILY, (32, 64, 40, 52), "p010", None) == (32, 64, 40, 52)
    assert yl.halo_window(chroma.FAMILY, (32, 64, 40, 52), "nv12", "topleft") == (31, 63, 41, 53)     # and a halo where there is one

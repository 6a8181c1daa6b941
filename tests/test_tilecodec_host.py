"""progressivecodec_amd._tilecodec without a GPU: the encode loop, the two cut walks and the decode loop against
a fake model and a fake cut, and the tile table as the PCT and the PCS parsers read it."""
import pytest
import torch

from tests.test_clip_rate_host import clip_blobs
from tests.test_clips_host import SOURCE
from tests.test_tiles_host import blob

T = 64
QUALITIES = [0.05, 0.5, 2.0]


class Model:
    """strings that depend on a tile's content alone: a tile is filled with its tag, slice s of level l is bytes([tag, s, l]) (the ten
    base slices are shared by the levels, as container.pack wants them)"""

    def __init__(self):
        self.calls = []

    def compress_levels(self, x, qualities, mask_pol):
        tags = [int(v) for v in x[:, 0, 0, 0].tolist()]
        self.calls.append(("compress_levels", tags, list(qualities), mask_pol))
        return [{"strings": [[[bytes([t, s, l if s >= 10 else 0]) for t in tags] for s in range(20)], [bytes([t]) for t in tags]], "shape": (1, 1)}
                for l in range(len(qualities))]

    def decompress_levels(self, strings, shape, qualities, mask_pol):
        tags = [z[0] for z in strings[0][1]]
        self.calls.append(("decompress_levels", tags, list(qualities), mask_pol))
        return [{"x_hat": torch.tensor(tags, dtype=torch.float32).reshape(-1, 1, 1, 1).expand(-1, 3, T, T) + l / 8} for l in range(len(qualities))]

    def decompress(self, strings, shape, q, mask_pol):
        tags = [z[0] for z in strings[1]]
        assert all(len(col) == len(tags) and all(s[:1] == bytes([t]) for s, t in zip(col, tags)) for col in strings[0])
        self.calls.append(("decompress", tags, q, tuple(shape), mask_pol))
        return {"x_hat": torch.tensor(tags, dtype=torch.float32).reshape(-1, 1, 1, 1).expand(-1, 3, T, T).contiguous()}


def fake_cut(seen):
    def cut(a, b):
        seen.append((a, b))
        return torch.arange(a, a + b, dtype=torch.float32).reshape(-1, 1, 1, 1).expand(-1, 3, T, T)
    return cut


@pytest.fixture
def contract_one(monkeypatch):
    from progressivecodec_amd import container
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)


# -- the encode loop -------------------------------------------------------------------------------------------------------------------

def test_encode_loop_chunks_cuts_and_packs(contract_one):
    from progressivecodec_amd import _tilecodec as tc
    from progressivecodec_amd import container
    by_step = {}
    for step in (1, 3, 7, 32):
        model, seen = Model(), []
        by_step[step] = tc.encode_items(model, 7, step, QUALITIES, "two-levels", T, fake_cut(seen))
        chunks = [(a, min(step, 7 - a)) for a in range(0, 7, step)]
        assert seen == chunks
        assert model.calls == [("compress_levels", list(range(a, a + b)), QUALITIES, "two-levels") for a, b in chunks]
        for a, b in chunks:                                                              # each blob is its chunk's strings at its position
            datas = Model().compress_levels(fake_cut([])(a, b), QUALITIES, "two-levels")
            for m in range(b):
                assert by_step[step][a + m] == container.pack([d["strings"] for d in datas], (1, 1), QUALITIES, image_size=(T, T),
                                                              mask_pol="two-levels", image_index=m)
    model, seen = Model(), []
    tc.encode_items(model, 7, 3, QUALITIES, "point-based-std", T, fake_cut(seen))
    assert seen == [(0, 3), (3, 3), (6, 1)] and [c[1] for c in model.calls] == [[0, 1, 2], [3, 4, 5], [6]]
    assert len(by_step[1]) == 7 and all(by_step[s] == by_step[1] for s in by_step)       # the bytes do not depend on the chunking
    assert [container.parse_header(b)["qualities"] for b in by_step[1]] == [QUALITIES] * 7
    assert tc.encode_items(Model(), 0, 3, QUALITIES, "two-levels", T, fake_cut([])) == []


def test_encode_loop_with_a_measurement(contract_one):
    from progressivecodec_amd import _tilecodec as tc
    from progressivecodec_amd import container
    results = {}
    for step in (1, 3, 7, 32):
        model, seen, measured = Model(), [], []

        def measure(a, b, decoded):
            assert len(decoded) == len(QUALITIES) and all(tuple(d["x_hat"].shape) == (b, 3, T, T) for d in decoded)
            measured.append((a, b))
            return [[float(d["x_hat"][m, 0, 0, 0]) for d in decoded] for m in range(b)]
        bufs, got = tc.encode_items(model, 7, step, QUALITIES, "two-levels", T, fake_cut(seen), measure)
        chunks = [(a, min(step, 7 - a)) for a in range(0, 7, step)]
        assert seen == measured == chunks                                                # once per chunk, with (a, b, decoded)
        assert [c[0] for c in model.calls] == ["compress_levels", "decompress_levels"] * len(chunks)
        assert [c[1] for c in model.calls] == [list(range(a, a + b)) for a, b in chunks for _ in range(2)]
        assert got == [[i + l / 8 for l in range(3)] for i in range(7)]                   # concatenated in item order
        assert len(bufs) == 7 and all(len(row) == 3 for row in bufs)                     # one single-level blob per item and level
        for i, row in enumerate(bufs):
            for l, b in enumerate(row):
                hd = container.parse_header(b)
                assert hd["qualities"] == [QUALITIES[l]] and hd["image_size"] == (T, T) and hd["mask_pol"] == "two-levels"
                strings = container.unpack(b, expect_contract=False)[0]
                assert strings[0][1] == [bytes([i])] and strings[0][0][19] == [bytes([i, 19, l])]
        results[step] = bufs
    assert all(results[s] == results[1] for s in results)


# -- the two cut walks -----------------------------------------------------------------------------------------------------------------

def test_one_piece_per_grid_row():
    from progressivecodec_amd import _tilecodec as tc
    assert list(tc.row_pieces(1, 4, 3)) == [(0, 1, 2), (1, 0, 2)]                        # a 2 x 3 grid, the tiles 1 .. 4
    assert list(tc.row_pieces(0, 6, 3)) == [(0, 0, 3), (1, 0, 3)]
    assert list(tc.row_pieces(5, 1, 3)) == [(1, 2, 1)] and list(tc.row_pieces(2, 5, 1)) == [(k, 0, 1) for k in range(2, 7)]
    assert list(tc.row_pieces(3, 0, 3)) == []
    for nx in (1, 2, 3, 5):                                                              # the pieces are the range, in order, within a row each
        for a in range(7):
            for b in range(1, 9):
                tiles = [i * nx + j + k for i, j, m in tc.row_pieces(a, b, nx) for k in range(m)]
                assert tiles == list(range(a, a + b)) and all(j + m <= nx and m >= 1 for _, j, m in tc.row_pieces(a, b, nx))


def test_one_piece_per_frame_present():
    from progressivecodec_amd import _tilecodec as tc
    chunk = [(0, 4), (0, 5), (2, 0), (2, 3), (3, 1)]
    pieces = list(tc.frame_pieces(chunk))
    assert pieces == [(0, 0, 2), (2, 2, 4), (3, 4, 5)]                                   # three launches of 2, 2 and 1 tiles
    x = torch.zeros(5, 1)
    for f, m0, m1 in pieces:                                                             # into x[0:2], x[2:4], x[4:5]
        x[m0:m1] += 1 + f
    assert x[:, 0].tolist() == [1, 1, 3, 3, 4]
    assert list(tc.frame_pieces([])) == [] and list(tc.frame_pieces([(7, 1)])) == [(7, 0, 1)]
    assert list(tc.frame_pieces([(1, t) for t in range(4)])) == [(1, 0, 4)]


# -- the decode loop -------------------------------------------------------------------------------------------------------------------

def strings_of(tags):
    return {p: [[[bytes([t, s])] for s in range(20)], [bytes([t])]] for p, t in tags.items()}


def test_decode_loop_groups_chunks_and_places():
    from progressivecodec_amd import _tilecodec as tc
    model = Model()
    tags = {p: 10 + p for p in range(6)}
    groups = sorted({2.0: [1, 2, 5], 0.5: [0, 3, 4]}.items())
    x = tc.decode_positions(model, strings_of(tags), groups, (1, 1), "two-levels", 2, 6)
    # ascending quality, tile order within a group, two at a time
    assert model.calls == [("decompress", t, q, (1, 1), "two-levels") for q, t in [(0.5, [10, 13]), (0.5, [14]), (2.0, [11, 12]), (2.0, [15])]]
    assert tuple(x.shape) == (6, 3, T, T) and x[:, 0, 0, 0].tolist() == [10, 11, 12, 13, 14, 15]
    # a list of strings serves as well as a dict, and a call that covers every position gives the model's tensor itself
    held = []

    class Keeps(Model):
        def decompress(self, *a):
            held.append(super().decompress(*a)["x_hat"])
            return {"x_hat": held[-1]}
    per_tile = [strings_of(tags)[p] for p in range(6)]
    assert tc.decode_positions(Keeps(), per_tile, [(0.5, list(range(6)))], (1, 1), "two-levels", 32, 6) is held[0] and len(held) == 1
    assert tc.decode_positions(Keeps(), per_tile, [(0.5, list(range(6)))], (1, 1), "two-levels", 6, 6) is held[1]
    y = tc.decode_positions(Keeps(), per_tile, [(0.5, list(range(6)))], (1, 1), "two-levels", 5, 6)
    assert len(held) == 4 and y is not held[2] and y[:, 0, 0, 0].tolist() == [10, 11, 12, 13, 14, 15]


def test_decode_loop_over_a_previous_frame():
    from progressivecodec_amd import _tilecodec as tc
    model = Model()
    prev = torch.arange(6, dtype=torch.float32).reshape(-1, 1, 1, 1).expand(-1, 3, T, T).contiguous()
    before = prev.clone()
    x = tc.decode_positions(model, strings_of({1: 41, 4: 44}), [(0.5, [1, 4])], (1, 1), "point-based-std", 32, 6, prev)
    assert model.calls == [("decompress", [41, 44], 0.5, (1, 1), "point-based-std")]
    assert x is not prev and x.data_ptr() != prev.data_ptr() and torch.equal(prev, before)           # a clone: prev is as it was
    assert x[:, 0, 0, 0].tolist() == [0, 41, 2, 3, 44, 5] and torch.equal(x[[0, 2, 3, 5]], prev[[0, 2, 3, 5]])
    assert torch.equal(x[1], torch.full((3, T, T), 41.0)) and torch.equal(x[4], torch.full((3, T, T), 44.0))
    # nothing fresh: the previous tensor itself, and the model is not asked
    assert tc.decode_positions(None, {}, [], None, None, 32, 6, prev) is prev
    # every position fresh: the previous tensor is not needed
    x = tc.decode_positions(model, strings_of({p: 50 + p for p in range(6)}), [(0.5, [0, 1, 2]), (2.0, [3, 4, 5])], (1, 1), "point-based-std", 32, 6, prev)
    assert x[:, 0, 0, 0].tolist() == [50, 51, 52, 53, 54, 55] and torch.equal(prev, before)


def test_tiles_that_disagree_are_refused_before_the_model(contract_one):
    from progressivecodec_amd import _tilecodec as tc
    from progressivecodec_amd import clip_rate, clips, container, tiles
    with pytest.raises(container.ContainerError, match=r"^tile 5 of the region was coded as \(\(2, 2\), 'two-levels'\), its first tile as \(\(1, 1\), 'two-levels'\)$"):
        tc.same_coding(((2, 2), "two-levels"), ((1, 1), "two-levels"), "tile 5 of the region", "its first tile")
    tc.same_coding(((1, 1), "two-levels"), ((1, 1), "two-levels"), "tile 5", "tile 0")
    y = [[bytes([5, s])] for s in range(20)]
    odd = container.pack([[y[:10], [bytes([5])]], [y, [bytes([5])]]], (1, 1), [0, 0.5], image_size=(T, T), mask_pol="two-levels", contract=1)
    # PCT1: the first tile and the offending one, by their place in the region
    pct1 = tiles.pack_tiled([blob(T, t) for t in range(5)] + [odd], 100, 150, T, 16, contract=1)
    with pytest.raises(container.ContainerError, match=r"tile 5 of the region was coded as \(\(1, 1\), 0\.5, 'two-levels', 20\), its first tile as "
                                                       r"\(\(1, 1\), 0\.5, 'point-based-std', 20\)"):
        tiles.decode_tiled(None, pct1)
    with pytest.raises(container.ContainerError, match="tile 1 of the region was coded as .*, its first tile as"):
        tiles.decode_tiled(None, pct1, region=(64, 64, 36, 86))                          # tiles 4 and 5 alone
    # PCT2: shape and mask policy, whatever the qualities
    one = container.pack([[y, [bytes([5])]]], (1, 1), [2.0], image_size=(T, T), mask_pol="two-levels", contract=1)
    pct2 = tiles.pack_tiled([blob(T, t, qualities=(0.5,)) for t in range(5)] + [one], 100, 150, T, 16, contract=1, per_tile_levels=True)
    with pytest.raises(container.ContainerError, match=r"tile 5 of the region was coded as \(\(1, 1\), 'two-levels'\), its first tile as \(\(1, 1\), 'point-based-std'\)"):
        tiles.decode_tiled(None, pct2)
    # PCS1 and PCS2: the frame and tile, against the first tile the frame was held to
    bl = [[blob(T, 16 * f + t) if s == f else None for t, s in enumerate(row)] for f, row in enumerate(SOURCE)]
    bl[3][4] = odd
    pcs1 = clips.pack_clip(bl, SOURCE, 100, 150, T, 16, "nv12", "bt709", "limited", "linear", contract=1)
    with pytest.raises(container.ContainerError, match=r"frame 3, tile 4 was coded as \(\(1, 1\), 0\.5, 'two-levels', 20\), tile 1 as "):
        clips.decode_clip(None, pcs1, frames=[2, 3])
    bl = clip_blobs()
    bl[3][4] = one
    pcs2 = clip_rate.pack_clip(bl, SOURCE, 100, 150, T, 16, "nv12", "bt709", "limited", "linear", contract=1)
    with pytest.raises(container.ContainerError, match=r"frame 3, tile 4 was coded as \(\(1, 1\), 'two-levels'\), tile 0 as \(\(1, 1\), 'point-based-std'\)"):
        clip_rate.decode_clip(None, pcs2, frames=[2, 3])


def test_level_index_refusals(contract_one):
    from progressivecodec_amd import _tilecodec as tc
    from progressivecodec_amd import container
    b = blob(T, 3)                                                                       # two levels: 0 and 0.5
    th = container.parse_header(b)
    assert tc.level_strings(b, th, -1)[:3] == ((1, 1), 0.5, "point-based-std") and tc.level_strings(b, th, 0)[1] == 0
    assert tc.level_strings(b, th, 1) == tc.level_strings(b, th, -1) and len(tc.level_strings(b, th, 0)[3][0]) == 10
    for level in (2, -3):
        with pytest.raises(container.ContainerError, match=f"^no level {level} among 2$"):
            tc.level_strings(b, th, level)
        with pytest.raises(container.ContainerError, match=f"^frame 1, tile 2: no level {level} among 2$"):
            tc.level_strings(b, th, level, "frame 1, tile 2: ")
    for level in (-1, 0, "0"):
        tc.one_level(level, "PCT2")
    for level in (1, -2, None, "top"):
        with pytest.raises(container.ContainerError, match="a PCS2 container holds one level per tile: level must be -1 or 0, got"):
            tc.one_level(level, "PCS2")
    with pytest.raises(container.ContainerError, match="^a PCT2 container holds one level per tile: level must be -1 or 0, got 1$"):
        tc.one_level(1, "PCT2")


# -- the tile table --------------------------------------------------------------------------------------------------------------------

def test_one_clip_parser_and_one_table_for_tiles_and_clips(contract_one):
    from progressivecodec_amd import clip_rate, clips, frame_tiles, tiles
    bl = clip_blobs()
    args = (bl, SOURCE, 100, 150, T, 16, "p010", "bt2020", "full", "nearest")
    pcs1, pcs2 = clips.pack_clip(*args, contract=1), clip_rate.pack_clip(*args, contract=1)
    assert pcs1[:4] == b"PCS1" and pcs2[:4] == b"PCS2" and pcs1[4:] == pcs2[4:]
    h1, h2 = clips.parse_clip(pcs1), clip_rate.parse_clip(pcs2)
    assert h1 == h2                                                                      # the same header fields and table, apart from nothing
    assert (h1["fmt"], h1["matrix"], h1["range"], h1["upsample"], h1["bits"], h1["contract"], h1["F"]) == ("p010", "bt2020", "full", "nearest", 10, 1, 4)
    assert h1["grid"] == tiles.grid_of(100, 150, T, 16) and h1["payload_start"] == 42 + 16 * 24 and [len(r) for r in h1["table"]] == [6] * 4
    for k in range(4):                                                                   # a reused tile repeats its entry
        assert all(h1["table"][k][t] == h1["table"][s][t] for t, s in enumerate(SOURCE[k]))
    # the PCT2 container of frame k holds, tile by tile, the lengths of the clip's table row k
    for k in range(4):
        inner = frame_tiles.parse_frame_tiled(clip_rate.frame_container(pcs2, k))["inner"]
        hd = tiles.parse_tiled(inner)
        assert hd["magic"] == b"PCT2" and hd["grid"] == h2["grid"] and hd["contract"] == h2["contract"]
        assert [n for _, n in hd["table"]] == [n for _, n in h2["table"][k]]
        assert [tiles.tile_bytes(inner, hd, t) for t in range(6)] == [clip_rate.tile_blob(pcs2, h2, k, t) for t in range(6)]
    # each parser refuses the other's magic, in its own words
    from progressivecodec_amd.container import ContainerError
    with pytest.raises(ContainerError, match="^not a PCS1 container$"):
        clips.parse_clip(pcs2)
    with pytest.raises(ContainerError, match="^not a PCS2 container$"):
        clip_rate.parse_clip(pcs1)

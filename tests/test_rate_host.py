"""Rate-controlled tiled coding without a GPU: the restatement (tests/rate_contract.py) against its own definition and against
tests/tiles_contract.py, libpc_rate.so's C ABI up to the first device call, the allocator of progressivecodec_amd.rate against the
restatement and a brute-force optimum, and the PCT2 container up to the model."""
import ctypes as C
import os
import random
import re
import struct
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import rate_contract as RC
from tests import tiles_contract as TC
from tests.test_tiles_host import blob, pct1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from progressivecodec_amd import rate
    return rate, rate.lib()


# -- the library, no device ----------------------------------------------------------------------------------------------------------

def test_library_exports_every_declared_function():
    rate, L = _lib()
    hdr = open(os.path.join(ROOT, "progressivecodec_amd", "rate_csrc", "pc_rate.h")).read()
    declared = re.findall(r"PC_API\s+[\w\s\*]+?\b(pc_\w+)\s*\(", hdr)
    assert len(declared) == 5 and sorted(declared) == sorted(rate.EXPORTS)
    for name in declared:
        getattr(L, name)
    assert L.pc_rate_strerror(-1).decode() and L.pc_rate_strerror(-6).decode() and L.pc_rate_last_hip_error() == 0


def test_integer_weights_partition_den_squared_and_are_the_float_weights():
    for T in (64, 128):
        for O in [o for o in (0, 4, 16, 32, 64) if o <= T // 2]:
            S, den = T - O, RC.den_of(O)
            assert den == (2 * O if O else 1)
            for ny, nx in [(1, 1), (1, 3), (2, 3)]:
                H, W = (ny - 1) * S + T - (5 if ny > 1 else 3), (nx - 1) * S + T - (7 if nx > 1 else 0)      # partial last tiles
                assert TC.grid(H, W, T, O) == (ny, nx)
                cover = np.zeros((H, W), np.int64)
                for i in range(ny):
                    wy = RC.weights_int(i, ny, T, O)
                    for j in range(nx):
                        wx = RC.weights_int(j, nx, T, O)
                        h, w = min(T, H - i * S), min(T, W - j * S)
                        cover[i * S:i * S + h, j * S:j * S + w] += wy[:h, None] * wx[None, :w]
                assert (cover == den * den).all(), (T, O, ny, nx)
            for n in (1, 2, 3):
                for i in range(n):
                    a = RC.weights_int(i, n, T, O)
                    assert a.min() >= 1 and a.max() <= den
                    for u in range(T):
                        f = np.float32(a[u]) / np.float32(den)
                        assert f.view(np.uint32) == TC.weight(i, u, n, T, O).view(np.uint32), (T, O, n, i, u)


def test_tile_sse_restatement_on_a_case_small_enough_to_do_by_hand():
    T, O = 64, 4                                                      # S = 60: a 64 x 70 image has 1 x 2 tiles, the band at columns 60 .. 63
    H, W = 64, 70
    ref = np.zeros((3, H, W), np.uint8)
    x = np.zeros((2, 3, T, T), np.float32)
    x[0, 1, 5, 61] = 1.0                                              # tile 0, channel 1: e = 255 at local column 61 = S + 1: ax = 2 (4 - 1 - 1) + 1 = 5
    x[1, 2, 7, 2] = np.nan                                            # NaN -> 0: no error
    x[1, 0, 7, 3] = 2.0 / 255                                         # tile 1, channel 0: e = 2 at local column 3 < O: ax = 7
    x[1, 0, 9, 9] = 1.0                                               # local column 9 = image column 69, the last one: ax = den = 8
    x[1, 0, 9, 10] = 1.0                                              # image column 70: beyond the image, does not count
    got = RC.tile_sse(x, H, W, T, O, "nearest", ref, "chw")
    assert got == [[0, 8 * 5 * 255 * 255, 0], [8 * 7 * 4 + 8 * 8 * 255 * 255, 0, 0]]
    assert RC.tile_sse(x[1:], H, W, T, O, "nearest", ref, "chw", first_tile=1) == got[1:]
    assert RC.tile_sse(x, H, W, T, O, "nearest", ref.transpose(1, 2, 0), "hwc") == got


def test_workspace_size():
    _, L = _lib()
    for T, n in [(64, 1), (64, 6), (128, 5), (192, 3), (512, 40), (2048, 1), (2048, 7)]:
        assert L.pc_rate_workspace_size(T, n) == 24 * n * (T * T // 4 // 1024), (T, n)
    assert 2048 * 2048 // 4096 * (2 ** 21 - 1) <= 2 ** 31 - 1 < 2048 * 2048 // 4096 * 2 ** 21
    assert L.pc_rate_workspace_size(2048, 2 ** 21 - 1) == 24 * 1024 * (2 ** 21 - 1)
    for bad in [(0, 1), (32, 1), (96, 1), (-64, 1), (2112, 1), (4096, 1), (64, 0), (64, -1), (2048, 2 ** 21)]:
        assert L.pc_rate_workspace_size(*bad) == 0, bad


def _plan(L, x, st, sc, sh, ref, rl, rp, rr):
    wide = C.c_int(-1)
    return L.pc_rate_plan(x, st, sc, sh, ref, rl, rp, rr, C.byref(wide)), wide.value


def test_plan_is_host_only_and_each_precondition_is_broken_alone():
    """made-up pointer values: nothing may be dereferenced or launched (there is no GPU here)"""
    _, L = _lib()
    HWC, CHW = 0, 1
    Fp, R = 0x7000_0100_0000, 0x7000_0200_0000
    T, H, W = 64, 100, 152
    fs = (3 * T * T, T * T, T)
    assert _plan(L, Fp, *fs, R, HWC, 0, 3 * W) == (0, 1) and _plan(L, Fp, *fs, R, CHW, H * W, W) == (0, 1)
    assert _plan(L, Fp, fs[0] + 8, fs[1] + 4, T + 4, R, CHW, H * W + 4, W + 4) == (0, 1)
    for lay, rp, rr in [(HWC, 0, 3 * W), (CHW, H * W, W)]:
        for off in (4, 8, 12):
            assert _plan(L, Fp + off, *fs, R, lay, rp, rr) == (0, 0)                            # the floats: 16-byte aligned
        assert _plan(L, Fp, fs[0] + 2, fs[1], fs[2], R, lay, rp, rr) == (0, 0)                  # their strides: multiples of 4
        assert _plan(L, Fp, fs[0], fs[1] + 1, fs[2], R, lay, rp, rr) == (0, 0)
        assert _plan(L, Fp, fs[0], fs[1], T + 2, R, lay, rp, rr) == (0, 0)
        for off in (1, 2, 3):
            assert _plan(L, Fp, *fs, R + off, lay, rp, rr) == (0, 0)                            # ref: 4-byte aligned
        assert _plan(L, Fp, *fs, R, lay, rp, rr + 1) == (0, 0) and _plan(L, Fp, *fs, R, lay, rp, rr + 2) == (0, 0)
    assert _plan(L, Fp, *fs, R, CHW, H * W + 2, W) == (0, 0)                                    # the plane stride: planar only
    assert _plan(L, Fp, *fs, R, HWC, 77, 3 * W) == (0, 1)
    assert _plan(L, Fp, *fs, R, HWC, 0, 3 * 150) == (0, 0) and _plan(L, Fp, *fs, R, HWC, 0, 3 * 150 + 2) == (0, 1)
    assert _plan(L, None, *fs, R, HWC, 0, 3 * W)[0] == -1 and _plan(L, Fp, *fs, None, HWC, 0, 3 * W)[0] == -1
    assert _plan(L, Fp, *fs, R, 2, 0, 3 * W)[0] == -1 and _plan(L, Fp, *fs, R, -1, 0, 3 * W)[0] == -1
    assert L.pc_rate_plan(Fp, *fs, R, HWC, 0, 3 * W, None) == -1


def test_every_argument_error_returns_before_the_device():
    """fake device pointers: every call below must return PC_ERR_ARG without touching them (no GPU here)"""
    _, L = _lib()
    A, Fp, Wk, S = 0x7000_0000_1000, 0x7000_0100_0000, 0x7000_0200_0000, 0x7000_0300_0000
    H, W, T, O = 100, 150, 64, 16                                     # 2 x 3 tiles
    nbytes = L.pc_rate_workspace_size(T, 6)
    ok = dict(x=Fp, sxt=3 * T * T, sxc=T * T, sxh=T, H=H, W=W, T=T, O=O, first=0, n=6, rounding=0, ref=A, rl=1, rp=H * W, rr=W, ws=Wk,
              nbytes=nbytes, out=S, stream=None)
    for bad in [dict(x=None), dict(x=Fp + 1), dict(sxh=T - 1), dict(sxc=0), dict(sxt=0), dict(H=0), dict(W=0), dict(T=0), dict(T=32), dict(T=96),
                dict(T=2112, O=0, sxh=2112, nbytes=10 ** 9), dict(T=4096, O=0, sxh=4096, nbytes=10 ** 9), dict(O=-4), dict(O=2), dict(O=36), dict(first=-1), dict(n=0), dict(n=-1), dict(n=7),
                dict(first=1), dict(first=6, n=1), dict(first=2 ** 31 - 1, n=1), dict(rounding=2), dict(rounding=-1), dict(ref=None), dict(rl=2),
                dict(rl=-1), dict(rr=W - 1), dict(rp=0), dict(rl=0, rr=3 * W - 1), dict(ws=None), dict(ws=Wk + 4), dict(out=None),
                dict(out=S + 4), dict(nbytes=nbytes - 1), dict(nbytes=0), dict(H=2 ** 31 - 1, W=2 ** 31 - 1, O=0)]:
        assert L.pc_rate_tile_sse_u8(*dict(ok, **bad).values()) == -1, bad
    # T = 2048 itself is inside the limit: with a workspace that is too small it is refused for that reason alone
    big = dict(ok, T=2048, sxh=2048, H=3000, W=5000, n=6, nbytes=L.pc_rate_workspace_size(2048, 6))
    assert L.pc_rate_workspace_size(2048, 6) == 24 * 1024 * 6
    assert L.pc_rate_tile_sse_u8(*dict(big, nbytes=big["nbytes"] - 1).values()) == -1
    assert L.pc_rate_tile_sse_u8(*dict(big, n=7, nbytes=10 ** 9).values()) == -1                  # 2 x 3 tiles there too


def test_python_rejects_before_any_device_call(monkeypatch):
    from progressivecodec_amd import rate, tiles

    def touched(*a, **k):
        raise AssertionError("the device was reached")
    for name in ("device", "current_stream", "synchronize", "current_device", "_lazy_init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.setattr(rate, "lib", touched)
    g = tiles.grid_of(100, 150, 64, 16)
    x = torch.zeros(6, 3, 64, 64)
    ref = torch.zeros(100, 150, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU"):
        rate.tile_distortion(x, g, ref)
    with pytest.raises(ValueError, match="rounding"):
        rate.tile_distortion(x, g, ref, rounding="floor")
    with pytest.raises(ValueError, match="layout"):
        rate.tile_distortion(x, g, ref, ref_layout="cwh")
    with pytest.raises(TypeError, match="float32"):
        rate.tile_distortion(x.double(), g, ref)
    with pytest.raises(TypeError, match="uint8"):
        rate.tile_distortion(x, g, ref.float())
    with pytest.raises(ValueError, match="outside"):
        rate.tile_distortion(x, g, ref, first_tile=1)
    with pytest.raises(ValueError, match="outside"):
        rate.tile_distortion(x[:1], g, ref, first_tile=-1)
    with pytest.raises(ValueError, match="x_hat_tiles must be"):
        rate.tile_distortion(x[:, :, :63], g, ref)
    with pytest.raises(ValueError, match="x_hat_tiles must be"):
        rate.tile_distortion(x[0], g, ref)
    with pytest.raises(ValueError, match="grid"):
        rate.tile_distortion(x, g._replace(ny=3), ref)
    with pytest.raises(ValueError, match="2048"):
        rate.tile_distortion(x, tiles.grid_of(100, 150, 4096, 0), ref)
    with pytest.raises(ValueError, match="GPU"):
        rate.encode_tiled_to_size(None, ref, [0, 1], 10 ** 6, tile=64)
    with pytest.raises(ValueError, match="max_tiles_per_call"):
        rate.encode_tiled_to_size(None, ref, [0], 10 ** 6, tile=64, max_tiles_per_call=0)
    with pytest.raises(ValueError, match="rounding"):
        rate.encode_tiled_to_size(None, ref, [0], 10 ** 6, tile=64, rounding="x")
    with pytest.raises(ValueError, match="level"):
        rate.encode_tiled_to_size(None, ref, [], 10 ** 6, tile=64)


# -- the allocator -------------------------------------------------------------------------------------------------------------------

def instance(seed):
    """1-5 tiles, 1-4 levels, small values so that ties, equal rates, dominated and collinear levels are common; not monotone"""
    rng = random.Random(seed)
    n, nl = rng.randint(1, 5), rng.randint(1, 4)
    rates = [[rng.randint(1, 12) for _ in range(nl)] for _ in range(n)]
    dists = [[rng.randint(0, 20) for _ in range(nl)] for _ in range(n)]
    if seed % 5 == 0:                                                  # a monotone table, as a codec gives: rate up, distortion down
        rates = [sorted(r) for r in rates]
        dists = [sorted(d, reverse=True) for d in dists]
    imp = None if seed % 3 else [Fraction(rng.randint(1, 6), rng.randint(1, 4)) for _ in range(n)]
    return rates, dists, imp


def test_allocator_on_300_random_instances(capsys):
    rate, _ = _lib()
    worst, full = Fraction(1), 0
    for seed in range(300):
        rates, dists, imp = instance(seed)
        n, nl = len(rates), len(rates[0])
        lo = sum(min(r) for r in rates)
        hi = sum(max(r) for r in rates)
        # what the cheapest way to every tile's least distortion costs
        admit = sum(min(r for r, d in zip(rates[t], dists[t]) if d == min(dists[t])) for t in range(n))
        with pytest.raises(ValueError, match=rf"\b{lo}\b"):
            rate.allocate(rates, dists, lo - 1, imp)
        for budget in sorted({lo, lo + 1, (lo + hi) // 2, admit - 1, admit, hi, hi + 5}):
            if budget < lo:
                continue
            got = rate.allocate(rates, dists, budget, imp)
            case = (seed, budget, rates, dists, imp)
            assert got == RC.allocate(rates, dists, budget, imp), case
            assert len(got) == n and all(0 <= l < nl for l in got) and RC.spent(rates, got) <= budget, case
            d = RC.weighted(dists, got, imp)
            for l in range(nl):
                if RC.spent(rates, [l] * n) <= budget:
                    assert d <= RC.weighted(dists, [l] * n, imp), case
            best = RC.brute_force(rates, dists, budget, imp)
            assert best is not None and d >= best, case
            if budget >= admit:
                assert d == best == RC.weighted(dists, [min(range(nl), key=lambda l: (dists[t][l], rates[t][l])) for t in range(n)], imp), case
                full += 1
            elif best > 0:
                worst = max(worst, d / best)
            if imp is None:
                assert got == rate.allocate(rates, dists, budget, [1] * n) == rate.allocate(rates, dists, budget, [2.5] * n), case
    assert full >= 300
    with capsys.disabled():
        print(f"\nallocator gap: worst greedy / brute-force distortion over the 300 instances = {worst} = {float(worst):.4f}")


def test_allocator_hull_drops_dominated_and_non_convex_levels():
    rate, _ = _lib()
    # one tile; level 1 is dominated by level 0 (same rate, more distortion), level 3 lies above the chord 0 -> 4, level 2 ties level 0
    rates, dists = [[10, 10, 10, 20, 30]], [[100, 120, 100, 60, 0]]
    assert RC.hull(rates[0], dists[0]) == [0, 4] and rate._hull(rates[0], dists[0]) == [0, 4]
    assert rate.allocate(rates, dists, 19) == [0]
    assert rate.allocate(rates, dists, 29) == [3]                      # the step 0 -> 4 does not fit: greedy stays at 100, uniform level 3 gives 60
    assert rate.allocate(rates, dists, 30) == [4]
    # two such tiles: the one step that fits goes to tile 0 (100 in all), which beats the uniform level 1 (120)
    assert rate.allocate([[10, 20, 30], [10, 20, 30]], [[100, 60, 0], [100, 60, 0]], 40) == [2, 0]
    # collinear points are not vertices: 0 -> 1 -> 2 on one line leaves [0, 2]
    assert rate._hull([10, 20, 30], [100, 50, 0]) == [0, 2] == RC.hull([10, 20, 30], [100, 50, 0])
    with pytest.raises(TypeError):
        rate.allocate([[1.5]], [[1]], 10)
    with pytest.raises(TypeError):
        rate.allocate([[1]], [[1]], 10.0)
    with pytest.raises(ValueError):
        rate.allocate([[1, 2], [1]], [[1, 2], [1]], 10)
    with pytest.raises(ValueError):
        rate.allocate([[1]], [[1]], 10, importance=[0])
    with pytest.raises(ValueError):
        rate.allocate([], [], 10)


def test_importance_moves_the_one_upgrade_to_the_weighted_tile():
    rate, _ = _lib()
    rates = [[10, 20], [10, 20]]
    dists = [[100, 40], [100, 50]]                                     # tile 0 gains 60 per 10 bytes, tile 1 gains 50
    assert rate.allocate(rates, dists, 30) == [1, 0]                   # one upgrade fits
    assert rate.allocate(rates, dists, 30, importance=[1, 2]) == [0, 1]            # 60 against 100
    assert rate.allocate(rates, dists, 30, importance=[1, Fraction(6, 5)]) == [1, 0]    # 60 against 60: the tie goes to the lower tile
    assert rate.allocate(rates, dists, 30, importance=[1, 1.25]) == [0, 1]
    assert rate.allocate(rates, dists, 40, importance=[1, 2]) == [1, 1] and rate.allocate(rates, dists, 20, importance=[1, 2]) == [0, 0]


# -- PCT2 ----------------------------------------------------------------------------------------------------------------------------

def pct2(qualities_per_tile=((0,), (0.5,), (0,), (10,), (0.5,), (0,)), contract=1, H=100, W=150, T=64, O=16):
    from progressivecodec_amd import tiles
    blobs = [blob(T, t, contract, qualities=qs) for t, qs in enumerate(qualities_per_tile)]
    return tiles.pack_tiled(blobs, H, W, T, O, contract=contract, per_tile_levels=True), blobs


def test_pct2_round_trip_and_pct1_bytes_unchanged():
    from progressivecodec_amd import container, tiles
    buf, blobs = pct2()
    hd = tiles.parse_tiled(buf)
    g = hd["grid"]
    assert hd["magic"] == b"PCT2" and buf[:4] == b"PCT2" and buf[4] == 1
    assert (g.H, g.W, g.T, g.O, g.ny, g.nx) == (100, 150, 64, 16, 2, 3) and hd["contract"] == 1
    assert hd["payload_start"] == 33 + 16 * 6 and len(buf) == hd["payload_start"] + sum(map(len, blobs))
    off = hd["payload_start"]
    for t, b in enumerate(blobs):
        assert hd["table"][t] == (off, len(b))
        tb, th = tiles.tile_bytes(buf, hd, t)
        assert tb == b and len(th["qualities"]) == 1
        off += len(b)
    # the same tiles as PCT1: only the magic differs; PCT1 stays the default and is what it was
    one = tiles.pack_tiled(blobs, 100, 150, 64, 16, contract=1)
    assert one[:4] == b"PCT1" and one[4:] == buf[4:] and tiles.parse_tiled(one)["magic"] == b"PCT1"
    old, old_blobs = pct1()
    head = b"PCT1" + struct.pack("<BIIIIIII", 1, 1, 100, 150, 64, 16, 2, 3)
    table, o = b"", len(head) + 96
    for b in old_blobs:
        table += struct.pack("<QQ", o, len(b))
        o += len(b)
    assert old == head + table + b"".join(old_blobs) == tiles.pack_tiled(old_blobs, 100, 150, 64, 16, contract=1, per_tile_levels=False)
    with pytest.raises(container.ContainerError, match="6 tile containers"):
        tiles.pack_tiled(blobs[:5], 100, 150, 64, 16, contract=1, per_tile_levels=True)


def test_pct2_truncation_behaves_as_pct1s():
    from progressivecodec_amd import container, tiles
    buf, blobs = pct2()
    hd = tiles.parse_tiled(buf)
    for n in range(0, hd["payload_start"]):
        with pytest.raises(container.ContainerError):
            tiles.parse_tiled(buf[:n])
    for k in range(6):
        off, n = hd["table"][k]
        for end, whole in [(off, k - 1), (off + 1, k - 1), (off + n - 1, k - 1), (off + n, k)]:
            part = tiles.parse_tiled(buf[:end])
            for t in range(6):
                if t <= whole:
                    assert tiles.tile_bytes(buf[:end], part, t)[0] == blobs[t]
                else:
                    with pytest.raises(container.ContainerError, match="truncated"):
                        tiles.tile_bytes(buf[:end], part, t)
    cut = buf[:hd["table"][4][0] + 3]
    with pytest.raises(container.ContainerError, match="tile 4"):
        tiles.decode_tiled(None, cut, region=(70, 60, 10, 10))
    with pytest.raises(container.ContainerError, match="tile 4"):
        tiles.decode_tiled(None, cut)


def test_pct2_refusals_come_before_the_model(monkeypatch):
    from progressivecodec_amd import container, tiles
    monkeypatch.setattr(container, "build_contract_id", lambda: 1)     # the made-up containers' contract: the checks after it are reached
    buf, blobs = pct2()
    for level in (1, 2, -2):
        with pytest.raises(container.ContainerError, match="level must be -1 or 0"):
            tiles.decode_tiled(None, buf, level=level)
    # a tile with two levels
    two = tiles.pack_tiled(blobs[:4] + [blob(64, 4, 1, qualities=(0, 0.5))] + blobs[5:], 100, 150, 64, 16, contract=1, per_tile_levels=True)
    with pytest.raises(container.ContainerError, match="holds 2 levels"):
        tiles.decode_tiled(None, two)
    with pytest.raises(container.ContainerError, match="holds 2 levels"):
        tiles.decode_tiled(None, two, level=0, region=(70, 64, 30, 32))                 # tile 4 alone
    # differing mask policies: tile 2 re-packed under another policy
    y = [[bytes([2, s]) * (1 + s % 3)] for s in range(20)]
    other = container.pack([[y[:10], [bytes([2])]]], (1, 1), [0], image_size=(64, 64), mask_pol="two-levels", contract=1)
    mixed = tiles.pack_tiled(blobs[:2] + [other] + blobs[3:], 100, 150, 64, 16, contract=1, per_tile_levels=True)
    with pytest.raises(container.ContainerError, match="two-levels"):
        tiles.decode_tiled(None, mixed)
    # nothing above is wrong with the container itself: with a model (here: none) the decode goes on to use it
    with pytest.raises(AttributeError):
        tiles.decode_tiled(None, buf)
    with pytest.raises(AttributeError):
        tiles.decode_tiled(None, buf, level=0, region=(5, 6, 20, 30))
    # the same tiles under the PCT1 magic are refused as before: they disagree in quality
    with pytest.raises(container.ContainerError, match="was coded as"):
        tiles.decode_tiled(None, tiles.pack_tiled(blobs, 100, 150, 64, 16, contract=1))
    # PCT1 still has one version, and so has PCT2
    old, _ = pct1()
    for b in (old, buf):
        bad = bytearray(b)
        bad[4] = 2
        with pytest.raises(container.ContainerError, match="version"):
            tiles.parse_tiled(bytes(bad))
    with pytest.raises(container.ContainerError, match="not a PCT1"):
        tiles.parse_tiled(b"PCT3" + buf[4:])
    with pytest.raises(container.ContainerError, match="contract"):
        tiles.decode_tiled(None, pct2(contract=7)[0])

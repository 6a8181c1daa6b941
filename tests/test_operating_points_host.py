"""The operating points of tests/operating_points.py on the host: each point meets the condition it exists for (on the contract
oracle's own symbols, indexes and masks), the oracle agrees with the REAL reference's goldens there
(tests/golden/operating_points.json), and the product's host coder codes the oracle's planes -- index 63 rows, strings made
mostly of bypass nibbles, hyper-latents outside their CDF -- to the oracle's bytes and back.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import liboracle as lo
from oracle.codec_ref import bpp_of, psnr_of
from tests import operating_points as op
from tests.util import BPP_TOL, NORTH_STAR_PSNR_TOL_DB, PSNR_TOL_DB, tables_npz

RUNS = op.all_runs()
RUN_IDS = [f"{p}-{c}-q{q}-{pol}" for p, c, q, pol in RUNS]


def _runs_of(point):
    return [r for r in RUNS if r[0] == point and r[3] == op.MASK_POL]


def _sum_stats(point):
    tot = None
    for r in _runs_of(point):
        s = op.oracle_run(*r)["stats"]
        if tot is None:
            tot = {k: (np.array(v) if k == "idx_hist" else v) for k, v in s.items()}
        else:
            for k, v in s.items():
                tot[k] = tot[k] + np.array(v) if k == "idx_hist" else (max(tot[k], v) if k.startswith(("max_", "y_escape_max")) else tot[k] + v)
    return tot


def _msg(point, t):
    h = t["idx_hist"]
    nz = np.nonzero(h)[0]
    return (f"{point}: indexes {nz.min()}..{nz.max()}, histogram {h.tolist()}; y escapes {t['y_escapes']}/{t['n_coded']} = "
            f"{t['y_escapes'] / t['n_coded']:.4f} (longest {t['y_escape_max_nibbles']} nibbles, max |symbol| {t['max_abs_symbol']}); "
            f"z escapes {t['z_escapes']}/{t['n_z']} = {t['z_escapes'] / t['n_z']:.4f}")


def test_default_point_is_the_synthetic_state_dict_bit_for_bit():
    from progressivecodec_amd.synth import synthetic_state_dict
    a, b = op.point_state_dict("default"), synthetic_state_dict()
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].numpy().tobytes() == b[k].numpy().tobytes(), k
    # a point's edit moves only the tensors it names
    w = op.point_state_dict("wide")
    moved = {k for k in b if w[k].numpy().tobytes() != b[k].numpy().tobytes()}
    assert moved == {k for k in b if k.startswith("cc_scale_transforms") and k.endswith(".8.weight")}


def test_seed1_differs_from_default_in_every_string():
    for _, c, q, pol in _runs_of("seed1"):
        a, b = op.oracle_run("default", c, q, pol)["out"]["strings"], op.oracle_run("seed1", c, q, pol)["out"]["strings"]
        assert all(x != y for x, y in zip(a[1], b[1]))
        assert all(x != y for sa, sb in zip(a[0], b[0]) for x, y in zip(sa, sb))


def test_floor_condition():
    t = _sum_stats("floor")
    assert t["idx_hist"][1:].sum() == 0 and t["idx_hist"][0] == t["n_coded"], _msg("floor", t)
    partial = 0
    for r in _runs_of("floor"):
        o = op.oracle_run(*r)
        bound = o["taps"]["b0"]["scale"].new_tensor(0.11)
        for k in o["keys"]:
            assert (o["taps"][k]["scale"] <= bound).all(), _msg("floor", t)
        for i, m in enumerate(o["out"]["masks"]):
            q = r[2]
            if 0 < q < 10:
                sc = o["taps"][f"e{i}"]["scale"]
                for b in range(sc.shape[0]):
                    thr = lo.quantile(sc[b].numpy(), 1.0 - q * 0.1)
                    assert int((sc[b] == float(thr)).sum()) >= 2, f"quantile threshold of slice {i} image {b} is no tie"
                    partial += 0 < int(m[b].sum()) < m[b].numel()
    assert partial > 0, "no mask that is neither empty nor full"


def test_wide_condition():
    t = _sum_stats("wide")
    h = t["idx_hist"]
    assert h[63] > 0 and h[48:].sum() >= 0.01 * h.sum(), _msg("wide", t)
    smax = max(float(op.oracle_run(*r)["taps"][k]["scale"].max()) for r in _runs_of("wide") for k in op.oracle_run(*r)["keys"])
    assert smax > float(tables_npz()["scale_table"][-1]), f"largest predicted scale {smax}; " + _msg("wide", t)


def test_bypass_condition():
    t = _sum_stats("bypass")
    assert t["y_escapes"] >= 0.20 * t["n_coded"] and t["y_escape_max_nibbles"] >= 4 and t["max_abs_symbol"] < 2 ** 20, _msg("bypass", t)


def test_hyper_condition():
    t = _sum_stats("hyper")
    assert t["z_escapes"] >= 0.05 * t["n_z"], _msg("hyper", t)


def test_means_condition():
    t = _sum_stats("means")
    mumax, coarse = 0.0, 0
    for r in _runs_of("means"):
        o = op.oracle_run(*r)
        for i, k in enumerate(o["keys"]):
            mu = o["taps"][k]["mu"].abs()
            mumax = max(mumax, float(mu.max()))
            coded = torch.ones_like(mu, dtype=torch.bool) if i < 10 else o["out"]["masks"][i - 10] != 0
            coarse += int((coded & (mu >= 1024.0)).sum())          # float32 ulp(mu) >= 2^-13 from |mu| = 2^10 on
    assert mumax >= 1024.0 and coarse > 0, f"max |mu| {mumax}, symbols coded at ulp(mu) >= 2^-13: {coarse}; " + _msg("means", t)


def test_tables_rebuilt_by_update_at_seed1_equal_the_reference_tables():
    from progressivecodec_amd import entropy
    sd = {k: v.numpy() for k, v in op.point_state_dict("seed1").items()}
    ec, el, eo = op.eb_tables_of_seed(1)
    e = entropy.entropy_bottleneck_tables(sd)
    assert np.array_equal(e.cdf, ec) and np.array_equal(e.length, el) and np.array_equal(e.offset, eo)
    t0 = tables_npz()
    assert ec.shape != t0["eb_cdf"].shape or not np.array_equal(ec, t0["eb_cdf"]), "seed 1 must have tables of its own"
    orc = op.oracle("seed1")
    from oracle.codec_ref import entropy_bottleneck_tables
    o = entropy_bottleneck_tables(orc.sd)
    assert np.array_equal(o.cdf, ec) and np.array_equal(o.length, el) and np.array_equal(o.offset, eo)


@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_oracle_vs_reference_golden(run):
    """At every point: z strings, shape, mask popcounts and z escape counts identical to the reference's.  Image by image: an image
    all of whose y strings are identical has the identical byte count and its PSNR within 1e-4 dB; an image with a flipped symbol
    is held to the project's 2e-3 dB / 2e-3 relative bytes; at least half of the run's y strings are identical.
    At op.DEV_POINTS (bypass, means) the oracle cannot stay within these at any input seed or multiplier that keeps the point's
    condition (tests/operating_points.py): 0..4 of 20..40 y strings are identical, PSNR differs by up to
    4.8e-2 dB.  There bpp and PSNR are held to twice the oracle-vs-reference deviation recorded with the golden, and the share of
    identical strings is printed."""
    g = op.golden_record(*run)
    o = op.oracle_run(*run)
    ys, zs = o["out"]["strings"]
    B, _, H, W = o["x"].shape
    assert list(o["out"]["shape"]) == g["shape"]
    assert [op.sha(s) for s in zs] == g["z_sha"], "hyper-latent strings must match the reference exactly"
    assert [[int(m[b].sum().item()) for b in range(B)] for m in o["out"]["masks"]] == g["mask_sums"]
    n_str = sum(len(sl) for sl in ys)
    n_ok = sum(op.sha(s) == h for sl, hl in zip(ys, g["y_sha"]) for s, h in zip(sl, hl))
    bpp, psnr = bpp_of(o["out"]["strings"], B, H, W), psnr_of(o["x"], o["x_hat"])
    st = o["stats"]
    print(f"{run}: {n_ok}/{n_str} y strings identical to the reference; bpp {bpp:.6f} (ref {g['bpp']:.6f}); psnr {psnr:.6f} dB "
          f"(ref {g['psnr']:.6f}, |d| {abs(psnr - g['psnr']):.2e}); y escapes {st['y_escapes']} (ref {g['y_escapes']}), z escapes {st['z_escapes']} (ref {g['z_escapes']})")
    assert st["z_escapes"] == g["z_escapes"] and st["n_z"] == g["n_z"]
    if run[0] in op.DEV_POINTS:
        d = g["oracle_dev"]
        assert abs(bpp - g["bpp"]) <= 2.0 * d["bpp"] and abs(psnr - g["psnr"]) <= 2.0 * d["psnr"]
        assert (n_ok, n_str) == (d["y_identical"], d["y_strings"])
        return
    # op.DEV_CASES (hyper, 128x128): no flip-free input seed of a handful stays within 1e-4 dB; twice the recorded deviation instead
    north_star = 2.0 * g["oracle_dev"]["psnr"] if "oracle_dev" in g else NORTH_STAR_PSNR_TOL_DB
    for b in range(B):
        nbytes = sum(len(sl[b]) for sl in ys) + len(zs[b])
        p_b = psnr_of(o["x"][b], o["x_hat"][b])
        if all(op.sha(sl[b]) == hl[b] for sl, hl in zip(ys, g["y_sha"])):
            assert [len(sl[b]) for sl in ys] == [ll[b] for ll in g["y_len"]]
            assert nbytes == g["bytes_per_image"][b]
            assert abs(p_b - g["psnr_per_image"][b]) <= north_star, f"image {b}"
        else:
            assert abs(nbytes - g["bytes_per_image"][b]) <= BPP_TOL * g["bytes_per_image"][b], f"image {b}"
            assert abs(p_b - g["psnr_per_image"][b]) <= PSNR_TOL_DB, f"image {b}"
    if n_ok == n_str:
        assert bpp == g["bpp"] and abs(psnr - g["psnr"]) <= north_star
        assert st["idx_hist"] == g["idx_hist"] and st["y_escapes"] == g["y_escapes"] and st["y_escape_max_nibbles"] == g["y_escape_max_nibbles"]
    else:
        assert abs(bpp - g["bpp"]) <= BPP_TOL * max(1.0, g["bpp"])
        assert abs(psnr - g["psnr"]) <= PSNR_TOL_DB
    assert n_ok >= 0.5 * n_str


@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_host_coder_on_the_oracle_planes(run):
    """pc_rans_encode_batch / pc_rans_decode_batch_u8 / pc_rans_bound alone, on the oracle's symbols and indexes of every y slice
    and of z: the bytes equal the oracle's coder's, no string is longer than pc_rans_bound(n), the u8 decoder returns the symbols."""
    from progressivecodec_amd._lib import lib
    L = lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    o = op.oracle_run(*run)
    sd = op.point_sd(run[0])
    ys, zs = o["out"]["strings"]
    B = len(zs)
    z = o["taps"]["z_sym"].numpy()
    zi = np.ascontiguousarray(np.broadcast_to(np.arange(z.shape[1], dtype=np.int32).reshape(1, -1, 1, 1), z.shape))
    jobs = [("z", z, zi, "entropy_bottleneck", zs)]
    jobs += [(k, o["taps"][k]["sym"].numpy(), o["taps"][k]["idx"].numpy(), "gaussian_conditional", ys[s]) for s, k in enumerate(o["keys"])]
    for name, sym, idx, g, want in jobs:
        cdf = np.ascontiguousarray(sd[g + "._quantized_cdf"].numpy(), np.int32)
        ln = np.ascontiguousarray(sd[g + "._cdf_length"].numpy(), np.int32)
        off = np.ascontiguousarray(sd[g + "._offset"].numpy(), np.int32)
        sym = np.ascontiguousarray(sym, np.int32).reshape(B, -1)
        idx = np.ascontiguousarray(idx, np.int32).reshape(B, -1)
        n = sym.shape[1]
        stride = L.pc_rans_bound(n)
        out = np.zeros((B, stride), np.uint8)
        lens = np.zeros(B, np.uint64)
        tab = (P(cdf), cdf.shape[0], cdf.shape[1], P(ln), P(off))
        assert L.pc_rans_encode_batch(P(sym), P(idx), B, n, *tab, P(out), stride, P(lens), 0) == 0, name
        assert int(lens.max()) <= stride
        enc = [out[b, : int(lens[b])].tobytes() for b in range(B)]
        assert enc == list(want), f"{name}: the host coder's bytes differ from the oracle's"
        ptrs = (C.c_char_p * B)(*enc)
        cl = (C.c_size_t * B)(*[len(e) for e in enc])
        dec = np.full((B, n), 12345, np.int32)
        assert L.pc_rans_decode_batch_u8(ptrs, cl, B, P(np.ascontiguousarray(idx.astype(np.uint8))), n, *tab, P(dec), 0) == 0, name
        assert np.array_equal(dec, sym), f"{name}: the u8 decoder does not return the symbols"


@pytest.mark.parametrize("point", op.STRING_POINTS)
def test_reference_strings_decode_through_the_oracle(point):
    """the reference's own bytes (op.STRING_CASE at wide and hyper), decoded by the oracle.  The case's input seed is one at which
    the oracle's encoder reproduces every string -- asserted -- so the reference's bytes are the oracle's and the decoded picture
    must be the reference's: PSNR within 1e-4 dB, pixels within 2e-2 of the stored subsample (test_decode_strings_made_by_the_reference)"""
    import torch.nn.functional as F
    c = op.golden_strings(point)
    o = op.oracle_run(point, c["case"], c["quality"])
    ys = [[bytes.fromhex(h) for h in sl] for sl in c["y_hex"]]
    zs = [bytes.fromhex(h) for h in c["z_hex"]]
    assert o["out"]["strings"][1] == zs
    assert o["out"]["strings"][0] == ys, "this case is not flip-free: pick another input seed (operating_points.SEED_OVERRIDE)"
    dec = op.oracle(point).decompress([ys, zs], torch.Size(c["shape"]), c["quality"])["x_hat"]
    x_hat = F.pad(dec, o["unpad"]).clamp_(0, 1)
    p = -10.0 * math.log10(torch.mean((o["x"][0] - x_hat[0]) ** 2).item())
    d = c.get("oracle_dev")                       # op.DEV_CASES: twice the deviation recorded with the golden
    assert abs(p - c["psnr_per_image"][0]) <= (2.0 * d["psnr"] if d else NORTH_STAR_PSNR_TOL_DB)
    sub = x_hat.flatten()[::op.XHAT_SUB].numpy()
    assert np.abs(sub - np.asarray(c["x_hat_sub"], np.float32)).max() <= (2.0 * d["pixel"] if d else 2e-2)

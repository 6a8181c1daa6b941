"""The codec driver end to end at the operating points of tests/operating_points.py: scale indexes up to 63 and predicted scales
above the table, strings made mostly of bypass nibbles, hyper-latents outside their CDF, an all-ties scale plane, means where
float32 is coarse, and a second draw of the weights.

* GPU == contract oracle, bit for bit: every string, mask, x_hat, and the sym / idx / mu / scale planes.  No tolerance.
* the GPU decodes the REAL reference's strings at wide and hyper (a flip-free case, asserted); z strings, shapes and mask
  popcounts equal the reference goldens at every point.
* the composition paths (levels API, pipeline, schedule options, forward_single_quality, batch invariance) at wide and bypass;
  decode(encode(x)) against the encoder's own latent at floor and bypass."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import operating_points as op  # noqa: E402
from tests.util import LIK_RTOL, NORTH_STAR_PSNR_TOL_DB  # noqa: E402

RUNS = op.all_runs()
RUN_IDS = [f"{p}-{c}-q{q}-{pol}" for p, c, q, pol in RUNS]
HARSH = ("wide", "bypass")


def _u32(t):
    return (t.cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(t)).contiguous().numpy().view(np.uint32)


@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_bit_exact_vs_oracle_and_reference_golden(run):
    point, cname, q, pol = run
    o = op.oracle_run(*run)
    net = op.gpu_net(point)
    out = net.compress(o["xp"].cuda(), q, pol)
    B, _, Hp, Wp = o["xp"].shape
    h, w = Hp // 16, Wp // 16
    per, n_steps = 32 * h * w, len(o["keys"])
    sym = net.read_tap("sym", np.int32)[: 20 * B * per].reshape(20, B, 32, h, w)
    idx = net.read_tap("idx", np.int32)[: 20 * B * per].reshape(20, B, 32, h, w)
    mu = net.read_tap("mu")[: 20 * B * per].reshape(20, B, h, w, 32)
    scale = net.read_tap("scale")[: 20 * B * per].reshape(20, B, h, w, 32)
    ys, zs = out["strings"]
    rys, rzs = o["out"]["strings"]
    assert tuple(out["shape"]) == tuple(o["out"]["shape"]) and len(ys) == len(rys) == n_steps
    assert zs == rzs, "z strings differ"
    for s, k in enumerate(o["keys"]):
        t = o["taps"][k]
        assert np.array_equal(idx[s], t["idx"].numpy()), f"{k}: idx plane"
        assert np.array_equal(_u32(mu[s].transpose(0, 3, 1, 2).copy()), _u32(t["mu"])), f"{k}: mu plane"
        assert np.array_equal(_u32(scale[s].transpose(0, 3, 1, 2).copy()), _u32(t["scale"])), f"{k}: scale plane"
        assert np.array_equal(sym[s], t["sym"].numpy()), f"{k}: sym plane"
        assert ys[s] == rys[s], f"y strings of slice {s} differ"
    assert len(out["masks"]) == len(o["out"]["masks"])
    for m, rm in zip(out["masks"], o["out"]["masks"]):
        assert np.array_equal(m.cpu().numpy(), rm.numpy())
    dec = net.decompress(out["strings"], out["shape"], q, pol)["x_hat"].cpu()
    assert np.array_equal(_u32(dec), _u32(o["x_hat_padded"])), f"x_hat max abs diff {(dec - o['x_hat_padded']).abs().max().item()}"
    # the reference's word: exact where it must be, the flips reported (the toleranced comparison is the host test's, on the oracle)
    g = op.golden_record(*run)
    assert list(out["shape"]) == g["shape"]
    assert [op.sha(s) for s in zs] == g["z_sha"], "hyper-latent strings must match the reference exactly"
    assert [[int(m[b].sum().item()) for b in range(B)] for m in out["masks"]] == g["mask_sums"]
    first = [None] * B
    for s, (sl, hl) in enumerate(zip(ys, g["y_sha"])):
        for b in range(B):
            if first[b] is None and op.sha(sl[b]) != hl[b]:
                first[b] = s
    n_ok = sum(op.sha(s) == hh for sl, hl in zip(ys, g["y_sha"]) for s, hh in zip(sl, hl))
    print(f"{run}: {n_ok}/{sum(len(sl) for sl in ys)} y strings identical to the reference; first diverging slice per image {first}")


@pytest.mark.parametrize("point", op.STRING_POINTS)
def test_decode_strings_made_by_the_reference(point):
    """pc_codec_decompress fed the byte strings the REAL reference wrote at this point.  The case is flip-free (asserted: the GPU's own
    encoder reproduces every string), so the decode must succeed and give the reference's picture: PSNR within 1e-4 dB, pixels
    within 2e-2 of the stored subsample."""
    c = op.golden_strings(point)
    o = op.oracle_run(point, c["case"], c["quality"])
    net = op.gpu_net(point)
    own = net.compress(o["xp"].cuda(), c["quality"], op.MASK_POL)
    ys = [[bytes.fromhex(hh) for hh in sl] for sl in c["y_hex"]]
    zs = [bytes.fromhex(hh) for hh in c["z_hex"]]
    assert own["strings"][1] == zs, "hyper-latent strings must match the reference exactly"
    assert own["strings"][0] == ys, "this case is not flip-free: pick another input seed (operating_points.SEED_OVERRIDE)"
    dec = net.decompress([ys, zs], torch.Size(c["shape"]), c["quality"], op.MASK_POL)["x_hat"].cpu()
    x_hat = F.pad(dec, o["unpad"]).clamp_(0, 1)
    p = -10.0 * math.log10(torch.mean((o["x"][0] - x_hat[0]) ** 2).item())
    sub = x_hat.flatten()[::op.XHAT_SUB].numpy()
    dmax = np.abs(sub - np.asarray(c["x_hat_sub"], np.float32)).max()
    print(f"{point}: PSNR of the GPU decode of the reference's bytes {p:.6f} dB vs reference {c['psnr_per_image'][0]:.6f}, max pixel difference {dmax:.2e}")
    d = c.get("oracle_dev")                       # op.DEV_CASES: twice the deviation recorded with the golden
    assert abs(p - c["psnr_per_image"][0]) <= (2.0 * d["psnr"] if d else NORTH_STAR_PSNR_TOL_DB)
    assert dmax <= (2.0 * d["pixel"] if d else 2e-2)


@pytest.mark.parametrize("point", HARSH)
def test_composition_paths(point):
    from progressivecodec_amd import ChannelProgresssiveWACNN, CodecPipeline
    net = op.gpu_net(point)
    levels = [0, 0.5, 10]
    o = [op.oracle_run(point, "b2_64", q) for q in levels]
    x = o[0]["xp"].cuda()
    singles = [net.compress(x, q, op.MASK_POL) for q in levels]
    want_x = [net.decompress(s["strings"], s["shape"], q, op.MASK_POL)["x_hat"].clone() for s, q in zip(singles, levels)]
    for s, r in zip(singles, o):
        assert s["strings"] == r["out"]["strings"]
    # levels API
    datas = net.compress_levels(x, levels, op.MASK_POL)
    for q, d, s in zip(levels, datas, singles):
        assert d["strings"] == s["strings"], f"strings differ at level {q}"
        assert len(d["masks"]) == len(s["masks"]) and all(torch.equal(m, ms) for m, ms in zip(d["masks"], s["masks"]))
    outs = net.decompress_levels([d["strings"] for d in datas], datas[0]["shape"], levels, op.MASK_POL)
    for q, a, b in zip(levels, outs, want_x):
        assert torch.equal(a["x_hat"], b), f"x_hat differs at level {q}"
    # pipeline
    jobs = [{"x": x, "mask_pol": op.MASK_POL, "quality": q} for q in levels] + [{"x": x, "mask_pol": op.MASK_POL, "qualities": [float(q) for q in levels]}]
    pipe = CodecPipeline(op.point_sd(point), device="cuda:0", n_pairs=1)
    res = list(pipe.code(iter(jobs)))
    for i, (job, enc, dec) in enumerate(res[:3]):
        assert enc["strings"] == singles[i]["strings"] and torch.equal(dec["x_hat"], want_x[i])
    assert [d["strings"] for d in res[3][1]] == [s["strings"] for s in singles]
    assert all(torch.equal(d["x_hat"], b) for d, b in zip(res[3][2], want_x))
    del pipe
    # schedule options
    net2 = ChannelProgresssiveWACNN(device="cuda:0")
    net2.load_state_dict(op.point_sd(point))
    for opts in ({"serial_schedule": 1}, {"serial_schedule": 0, "lanes_enc": 2, "lanes_dec": 3}):
        for k, v in opts.items():
            net2.set_option(k, v)
        for s, q, b in zip(singles, levels, want_x):
            out = net2.compress(x, q, op.MASK_POL)
            assert out["strings"] == s["strings"], (opts, q)
            assert torch.equal(net2.decompress(out["strings"], out["shape"], q, op.MASK_POL)["x_hat"], b), (opts, q)
    del net2
    # an image alone and inside the batch
    for q, s in zip(levels, singles):
        one = net.compress(x[1:2].contiguous(), q, op.MASK_POL)
        assert all(sl[1] == s1[0] for sl, s1 in zip(s["strings"][0], one["strings"][0])) and s["strings"][1][1] == one["strings"][1][0], q
    # likelihood path
    for q, b in zip((0, 0.5), want_x):
        out = net.forward_single_quality(x, q, op.MASK_POL)
        ref = op.oracle(point).forward_single_quality(o[0]["xp"], q)
        ly, lz = out["likelihoods"]["y"].cpu(), out["likelihoods"]["z"].cpu()
        ry, rz = ref["likelihoods"]["y"], ref["likelihoods"]["z"]
        assert np.array_equal(_u32(out["x_hat"]), _u32(ref["x_hat"])) and torch.equal(out["x_hat"], b)
        assert ((ly - ry).abs() / ry).max().item() <= LIK_RTOL
        assert ((lz - rz).abs() / rz).max().item() <= 5e-6
        bits = lambda t: float(-torch.log2(t.double()).sum())
        assert abs(bits(ly) - bits(ry)) <= 1e-7 * bits(ry)
        assert abs(bits(lz) - bits(rz)) <= 1e-6 * bits(rz)


@pytest.mark.parametrize("point", ("floor", "bypass"))
def test_round_trip_equals_the_encoders_own_latent(point):
    """the decoder re-derives every mask and index from what it decoded: on a plane of ties (floor) or of escapes (bypass) its
    latent must be the encoder's, and the oracle's"""
    net = op.gpu_net(point)
    runs = [r for r in RUNS if r[0] == point]
    for run in runs:
        _, cname, q, pol = run
        o = op.oracle_run(*run)
        B, _, Hp, Wp = o["xp"].shape
        h, w = Hp // 16, Wp // 16
        name = "yhat_base" if q == 0 else "yhat_enh"
        out = net.compress(o["xp"].cuda(), q, pol)
        y_enc = net.read_latent(name, B, h, w).clone()
        x_hat = net.decompress(out["strings"], out["shape"], q, pol)["x_hat"].cpu()
        y_dec = net.read_latent(name, B, h, w)
        assert np.array_equal(_u32(y_dec), _u32(y_enc)), f"{run}: the decoder's latent is not the encoder's"
        assert np.array_equal(_u32(y_dec), _u32(o["y_hat"])), f"{run}: latent differs from the oracle's"
        assert np.array_equal(_u32(x_hat), _u32(o["x_hat_padded"]))

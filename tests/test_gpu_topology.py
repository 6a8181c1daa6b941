"""The topology switches of ChannelProgresssiveWACNN on the GPU (models/CHProg_cnn.py:29-49): every variant of tests/topology_contract.py
against the reference's strings (tests/golden/topology.json), the numeric-contract restatement (x_hat bit for bit, likelihoods within
an ulp), multi-level calls against per-level calls, CodecPipeline and compress_with_ac(overlap=True)."""
import functools
import json
import math
import os

import pytest
import torch

from tests.topology_contract import CASES, VARIANTS, TopologyCodec, strings_digest, variant_cfg, variant_sd
from tests.util import inputs

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def _gold():
    return json.load(open(os.path.join(GOLD, "topology.json")))


@functools.lru_cache(maxsize=None)
def _net(name):
    from progressivecodec_amd import ChannelProgresssiveWACNN
    net = ChannelProgresssiveWACNN(device="cuda:0", **VARIANTS[name])
    net.load_state_dict(variant_sd(name))
    return net


@functools.lru_cache(maxsize=None)
def _cdet(name):
    return TopologyCodec(variant_sd(name), variant_cfg(name), "cdet")


def _cpu(t):
    return t.detach().cpu()


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_strings_and_decode_match_reference(name):
    net = _net(name)
    for case, (B, H, W, seed, kind, q, pol) in zip(_gold()[name], CASES):
        x = inputs(B, H, W, seed, kind)
        o = net.compress(x.cuda(), q, pol)
        ys, zs = o["strings"]
        assert case["cdet_strings_equal"]
        assert strings_digest(ys) == case["y_digest"], (name, case["case"])
        assert strings_digest(zs) == case["z_digest"], (name, case["case"])
        d = net.decompress(o["strings"], o["shape"], q, pol)["x_hat"]
        psnr = -10.0 * math.log10(torch.mean((x - _cpu(d)) ** 2).item())
        assert abs(psnr - case["psnr"]) < 1e-4, (name, case["case"], psnr, case["psnr"])
        if not VARIANTS[name].get("u_net_post") and H == 64:            # the contract restates the chain, not the post-filter
            ref = _cdet(name).decompress(o["strings"], o["shape"], q, pol)["x_hat"]
            assert torch.equal(_cpu(d), ref), (name, case["case"])


@pytest.mark.parametrize("name", sorted(n for n in VARIANTS if not VARIANTS[n].get("u_net_post")))
def test_forward_matches_contract(name):
    net = _net(name)
    B, H, W, seed, kind, _, pol = CASES[0]
    x = inputs(B, H, W, seed, kind)
    for q in (0.0, 0.5, 10.0):
        g = net.forward_single_quality(x.cuda(), q, pol)
        r = _cdet(name).forward_single_quality(x, q, pol)
        assert torch.equal(_cpu(g["x_hat"]), r["x_hat"]), (name, q)
        # y: one float32 ulp (the HIP kernel and the contract round a double erfc from different libms); z: the EntropyBottleneck's
        # density network, untouched by the switches, at the tolerance of tests/test_gpu_codec.py
        for k, rtol in (("y", 3e-7), ("z", 5e-6)):
            a, b = _cpu(g["likelihoods"][k]), r["likelihoods"][k]
            assert a.shape == b.shape
            assert ((a - b).abs() / b).max().item() <= rtol, (name, q, k)


@pytest.mark.parametrize("name", ["cond_all_s2", "ref_defaults", "mu_rep_s5"])
def test_levels_equal_per_level_calls(name):
    net = _net(name)
    B, H, W, seed, kind, _, pol = CASES[3]
    x = inputs(B, H, W, seed, kind).cuda()
    qs = [0.5, 10.0, 0.0, 3.0]
    lv = net.compress_levels(x, qs, pol)
    per = [net.compress(x, q, pol) for q in qs]
    for a, b in zip(lv, per):
        assert a["strings"] == b["strings"]
    dl = net.decompress_levels([d["strings"] for d in lv], lv[0]["shape"], qs, pol)
    for a, b, q in zip(dl, per, qs):
        assert torch.equal(a["x_hat"], net.decompress(b["strings"], b["shape"], q, pol)["x_hat"]), (name, q)


@pytest.mark.parametrize("n_pairs", [1, 2])
def test_pipeline_equals_sequential(n_pairs):
    from progressivecodec_amd import CodecPipeline
    name = "cond_all_s2"
    pipe = CodecPipeline(variant_sd(name), device="cuda:0", n_pairs=n_pairs, **VARIANTS[name])
    jobs = [dict(x=inputs(2, 64, 64, 50 + i, "rand").cuda(), quality=q) for i, q in enumerate((0.5, 10.0, 0.0, 2.0))]
    jobs.append(dict(x=inputs(2, 64, 128, 60, "smooth").cuda(), qualities=[0.5, 10.0]))
    got = list(pipe.code(jobs))
    want = list(pipe.code_sequential(jobs))
    for (_, ea, da), (_, eb, db) in zip(got, want):
        if isinstance(ea, list):
            assert [e["strings"] for e in ea] == [e["strings"] for e in eb]
            assert all(torch.equal(a["x_hat"], b["x_hat"]) for a, b in zip(da, db))
        else:
            assert ea["strings"] == eb["strings"] and torch.equal(da["x_hat"], db["x_hat"])


def test_compress_with_ac_overlap():
    from progressivecodec_amd.harness import compress_with_ac
    net = _net("std_s3")
    imgs = [inputs(1, 64, 64, 70 + i, "smooth") for i in range(3)]
    a = compress_with_ac(net, imgs, [0, 0.5, 10])
    b = compress_with_ac(net, imgs, [0, 0.5, 10], overlap=True)
    assert a[0] == b[0]                                                   # bytes: the same strings
    assert all(abs(u - v) < 1e-5 for u, v in zip(a[1], b[1]))             # PSNR: the overlapped path reduces the MSE in another order

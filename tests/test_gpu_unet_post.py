"""The UNet post-filter on the GPU (ChannelProgresssiveWACNN(u_net_post=1/2); reference CHProg_cnn.py:277-284, layers/unet.py).

The stand-alone filter is checked bit for bit against the contract restatement (tests/unet_contract.py) and within the host test's
tolerance against the reference's refine outputs; the decode paths against the mode-0 decode followed by the stand-alone filter and its
clamp (the filter must change nothing else), against the reference's end-to-end fixtures, and against each other (levels, pipeline,
forward).  REM output never goes through the filter."""
import functools
from collections import OrderedDict
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_unet_post_host import REFINE_TOL  # noqa: E402
from tests.util import inputs, synth_sd  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POL = "point-based-std"


@functools.lru_cache(maxsize=None)
def sd_of(mode):
    from progressivecodec_amd.arch import CodecConfig
    from progressivecodec_amd.synth import synthetic_state_dict
    sd = OrderedDict(synth_sd())                              # (a copy: synth_sd's dict may be shared)
    if mode:
        for k, v in synthetic_state_dict(CodecConfig(u_net_post=mode)).items():
            if k.startswith("refine"):
                sd[k] = v
    return sd


@functools.lru_cache(maxsize=None)
def net_of(mode):
    from progressivecodec_amd import ChannelProgresssiveWACNN
    net = ChannelProgresssiveWACNN(device="cuda:0", u_net_post=mode)
    net.load_state_dict(sd_of(mode))
    net.update()
    return net


def bits(t):
    return (t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)).view(np.uint32)


def restated(x, mode, which, clamp=False):
    from tests import unet_contract as uc
    pre = "refine" if mode == 1 else f"refine.{which}"
    sd = {k: v for k, v in sd_of(mode).items() if k.startswith("refine")}
    return uc.refine(np.asarray(x, np.float32), uc.refine_weights(sd, pre), clamp=clamp)


CASES = [(1, 0), (2, 0), (2, 1)]


@pytest.mark.parametrize("mode,which", CASES)
@pytest.mark.parametrize("shape,seed,kind", [((2, 3, 64, 64), 31, "smooth"), ((1, 3, 64, 96), 32, "smooth"), ((1, 3, 256, 256), 5, "rand")])
def test_standalone_filter_bit_exact_vs_restatement(mode, which, shape, seed, kind):
    x = inputs(*shape[:1], *shape[2:], seed, kind)
    y = net_of(mode).post_filter(x.cuda(), which=which)
    torch.cuda.synchronize()
    assert np.array_equal(bits(y), restated(x.numpy(), mode, which).view(np.uint32))


def test_standalone_filter_outside_unit_range_and_in_place_form():
    g = torch.Generator().manual_seed(7)
    x = (torch.rand(1, 3, 64, 128, generator=g) * 3.0 - 1.0)
    y = net_of(1).post_filter(x.cuda())
    torch.cuda.synchronize()
    assert np.array_equal(bits(y), restated(x.numpy(), 1, 0).view(np.uint32))


def test_standalone_filter_refuses_bad_shapes():
    from progressivecodec_amd._lib import PcodecError
    for H, W in ((62, 64), (64, 66), (64, 30)):
        with pytest.raises(PcodecError):
            net_of(1).post_filter(torch.rand(1, 3, H, W, device="cuda:0"))
    with pytest.raises(PcodecError):
        net_of(1).post_filter(torch.rand(1, 3, 64, 64, device="cuda:0"), which=1)
    with pytest.raises(RuntimeError):
        net_of(0).post_filter(torch.rand(1, 3, 64, 64, device="cuda:0"))


@pytest.mark.parametrize("tag", ["64x64", "64x96"])
def test_standalone_filter_vs_reference_fixtures(tag):
    d = np.load(os.path.join(GOLD, f"unet_io_{tag}.npz"))
    x = torch.from_numpy(d["x"]).cuda()
    for key, mode, which in (("refine", 1, 0), ("refine0", 2, 0), ("refine1", 2, 1)):
        y = net_of(mode).post_filter(x, which=which).cpu().numpy()
        assert float(np.abs(y - d[key]).max()) < REFINE_TOL, key


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("q", [0.0, 0.5])
def test_decompress_is_mode0_decode_then_filter_and_clamp(mode, q):
    x = inputs(2, 64, 128, 41, "smooth").cuda()
    n0, n = net_of(0), net_of(mode)
    o0 = n0.compress(x, quality=q, mask_pol=POL)
    o = n.compress(x, quality=q, mask_pol=POL)
    assert o["strings"] == o0["strings"]
    x0 = n0.decompress(o0["strings"], o0["shape"], q, POL)["x_hat"]
    xh = n.decompress(o["strings"], o["shape"], q, POL)["x_hat"]
    want = n.post_filter(x0).clamp(0, 1)
    torch.cuda.synchronize()
    assert np.array_equal(bits(xh), bits(want))
    assert not np.array_equal(bits(xh), bits(x0))
    assert np.array_equal(bits(xh), restated(x0.cpu().numpy(), mode, mode - 1, clamp=True).view(np.uint32))


@pytest.mark.parametrize("case", json.load(open(os.path.join(GOLD, "unet_e2e.json"))), ids=lambda c: c["case"])
def test_end_to_end_vs_reference(case):
    import hashlib
    net = net_of(case["mode"])
    x = inputs(case["B"], case["H"], case["W"], case["seed"], case["kind"])
    o = net.compress(x.cuda(), quality=case["quality"], mask_pol=case["mask_pol"])
    ys, zs = o["strings"]
    assert [hashlib.sha256(s).hexdigest() for s in zs] == case["z_sha"]
    assert [[hashlib.sha256(s).hexdigest() for s in sl] for sl in ys] == case["y_sha"]
    xh = net.decompress(o["strings"], o["shape"], case["quality"], case["mask_pol"])["x_hat"].cpu()
    ref = torch.from_numpy(np.load(os.path.join(GOLD, "unet_e2e.npz"))[case["case"]])
    psnr = lambda a: -10.0 * math.log10(torch.mean((x - a.clamp(0, 1)) ** 2).item())
    assert abs(psnr(xh) - psnr(ref)) < 1e-4 and abs(psnr(xh) - case["psnr"]) < 1e-4


@pytest.mark.parametrize("mode", [1, 2])
def test_levels_equal_per_level_calls(mode):
    net = net_of(mode)
    x = inputs(2, 64, 128, 43, "smooth").cuda()
    levels = [0, 0.1, 0.5, 2, 10]
    outs = net.compress_levels(x, levels, mask_pol=POL)
    xl = net.decompress_levels([o["strings"] for o in outs], outs[0]["shape"], levels, mask_pol=POL)
    for i, q in enumerate(levels):
        o = net.compress(x, quality=q, mask_pol=POL)
        assert o["strings"] == outs[i]["strings"], q
        xs = net.decompress(o["strings"], o["shape"], q, POL)["x_hat"]
        got = xl[i]["x_hat"] if isinstance(xl[i], dict) else xl[i]
        torch.cuda.synchronize()
        assert np.array_equal(bits(got), bits(xs)), q


def test_pipeline_and_overlap_harness_equal_single_calls():
    from progressivecodec_amd import CodecPipeline
    from progressivecodec_amd.harness import compress_with_ac
    net = net_of(1)
    pipe = CodecPipeline.from_model(net)
    assert pipe.dec.cfg.u_net_post == 1
    xs = [inputs(1, 64, 128, 50 + i, "smooth").cuda() for i in range(3)]
    jobs = [dict(x=x, quality=0.5, mask_pol=POL) for x in xs]
    for job, enc, dec in pipe.code(jobs):
        o = net.compress(job["x"], quality=0.5, mask_pol=POL)
        want = net.decompress(o["strings"], o["shape"], 0.5, POL)["x_hat"]
        torch.cuda.synchronize()
        assert enc["strings"] == o["strings"]
        assert np.array_equal(bits(dec["x_hat"]), bits(want))
    imgs = [inputs(1, 64, 128, 60 + i, "smooth") for i in range(4)]
    _, _, _, rows1 = compress_with_ac(net, imgs, [0, 0.5, 2], shared_base=True)
    _, _, _, rows2 = compress_with_ac(net, imgs, [0, 0.5, 2], overlap=True, group_size=2)
    assert [r["bpp"] for r in rows1] == [r["bpp"] for r in rows2]
    assert max(abs(a["psnr"] - b["psnr"]) for a, b in zip(rows1, rows2)) < 1e-5     # (per-row averages are summed in another order)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("q", [0.0, 0.5])
def test_forward_single_quality_equals_decompress(mode, q):
    net = net_of(mode)
    x = inputs(1, 64, 128, 44, "smooth").cuda()
    f = net.forward_single_quality(x, q, mask_pol=POL)
    o = net.compress(x, quality=q, mask_pol=POL)
    d = net.decompress(o["strings"], o["shape"], q, POL)["x_hat"]
    torch.cuda.synchronize()
    assert np.array_equal(bits(f["x_hat"]), bits(d))


def test_rem_over_a_filtered_base_ignores_the_filter():
    from progressivecodec_amd import ChannelProgresssiveWACNN, PostRateProcessedNetwork
    from progressivecodec_amd.synth import synthetic_post_state_dict
    post = synthetic_post_state_dict(3, "big")
    res = []
    for mode in (0, 1):
        base = ChannelProgresssiveWACNN(device="cuda:0", u_net_post=mode)
        rem = PostRateProcessedNetwork(base, check_levels=[0.01, 0.25, 1.75])
        rem.load_state_dict(sd_of(mode), post)
        rem.update()
        x = inputs(1, 64, 128, 45, "smooth").cuda()
        o = rem.compress(x, quality=0.5, mask_pol=POL)
        d = rem.decompress(o["strings"], o["shape"], 0.5, POL)["x_hat"]
        torch.cuda.synchronize()
        res.append((o["strings"], bits(d)))
    assert res[0][0] == res[1][0] and np.array_equal(res[0][1], res[1][1])


def test_state_dict_round_trip_and_strict_loading():
    from progressivecodec_amd import ChannelProgresssiveWACNN
    n1 = net_of(1)
    sd = n1.state_dict()
    assert sum(k.startswith("refine.") for k in sd) == 62
    assert sum(k.startswith("refine.") for k, _ in n1.named_parameters()) == 62
    again = ChannelProgresssiveWACNN(device="cuda:0", u_net_post=1)
    again.load_state_dict(sd)
    x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(3)).cuda()
    assert np.array_equal(bits(again.post_filter(x)), bits(n1.post_filter(x)))
    with pytest.raises(RuntimeError):                         # refine.* unexpected for a mode-0 model
        ChannelProgresssiveWACNN(device="cuda:0").load_state_dict(sd)
    with pytest.raises(RuntimeError):                         # refine.* missing for a mode-1 model
        ChannelProgresssiveWACNN(device="cuda:0", u_net_post=1).load_state_dict(sd_of(0))
    with pytest.raises(RuntimeError):                         # strict=False cannot leave the filter without weights
        ChannelProgresssiveWACNN(device="cuda:0", u_net_post=1).load_state_dict(sd_of(0), strict=False)
    with pytest.raises(AssertionError):
        ChannelProgresssiveWACNN(device="cuda:0", u_net_post=3)

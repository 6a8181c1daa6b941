"""WACNN (reference models/cnn.py:23-340) on the GPU: compress / decompress / forward bit for bit against the numeric-contract back-end
of tests/wacnn_contract.py, the reference's own strings (tests/golden/wacnn.json, where the contract reproduces them), the single-stream
error paths, coexistence with ChannelProgresssiveWACNN, schedule options and compress_single_rate."""
import ctypes as C
import functools
import hashlib
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_codec import LIK_RTOL  # noqa: E402
from tests.test_wacnn_host import wacnn_cases, wacnn_sd  # noqa: E402
from tests.util import inputs, synth_sd  # noqa: E402

sha = lambda b: hashlib.sha256(b).hexdigest()


def all_cases():
    """the golden cases plus one more shape (B=2, 128x64: H > W)"""
    return [(c["B"], c["H"], c["W"], c["seed"], c["kind"]) for c in wacnn_cases()] + [(2, 128, 64, 61, "rand")]


@functools.lru_cache(maxsize=None)
def gpu_wacnn():
    from progressivecodec_amd import WACNN
    net = WACNN.from_state_dict(wacnn_sd())
    return net.eval()


@functools.lru_cache(maxsize=None)
def contract():
    from tests.wacnn_contract import WacnnCodec
    return WacnnCodec(wacnn_sd(), "cdet")


@functools.lru_cache(maxsize=None)
def contract_run(case):
    """(compress, decompress x_hat, forward) of the contract for all_cases()[case]"""
    B, H, W, seed, kind = all_cases()[case]
    x = inputs(B, H, W, seed, kind)
    o = contract().compress(x)
    return o, contract().decompress(o["strings"], o["shape"])["x_hat"], contract().forward(x)


@pytest.mark.parametrize("case", range(4))
def test_compress_decompress_forward_bit_exact_vs_contract(case):
    B, H, W, seed, kind = all_cases()[case]
    x = inputs(B, H, W, seed, kind)
    net = gpu_wacnn()
    co, cx, cf = contract_run(case)
    o = net.compress(x.cuda())
    assert len(o["strings"][0]) == 1 and len(o["strings"][1]) == B
    assert o["strings"][0][0] == co["strings"][0][0]
    assert o["strings"][1] == co["strings"][1]
    assert list(o["shape"]) == list(co["shape"]) == [H // 64, W // 64]
    x_hat = net.decompress(o["strings"], o["shape"])["x_hat"].cpu()
    assert torch.equal(x_hat, cx)
    f = net(x.cuda())
    assert torch.equal(f["x_hat"].cpu(), cf["x_hat"])                        # unclamped
    # y: one float32 ulp (LIK_RTOL); z: the EntropyBottleneck density network's bound of test_forward_single_quality_vs_oracle
    for k, tol in (("y", LIK_RTOL), ("z", 5e-6)):
        a, r = f["likelihoods"][k].cpu(), cf["likelihoods"][k]
        assert a.shape == r.shape
        assert ((a - r).abs() / r).max().item() <= tol, k
    bits = lambda t: float(-torch.log2(t.double()).sum())
    ly, ry = f["likelihoods"]["y"].cpu(), cf["likelihoods"]["y"]
    assert abs(bits(ly) - bits(ry)) <= 1e-7 * bits(ry)


@pytest.mark.parametrize("case", range(3))
def test_strings_and_psnr_equal_the_reference(case):
    c = wacnn_cases()[case]
    assert c["cdet_strings_equal"]                                           # the generator chose cases where the contract reproduces them
    x = inputs(c["B"], c["H"], c["W"], c["seed"], c["kind"])
    net = gpu_wacnn()
    o = net.compress(x.cuda())
    ys, zs = o["strings"]
    assert sha(ys[0]) == c["y_sha"] and [sha(s) for s in zs] == c["z_sha"]
    x_hat = net.decompress(o["strings"], o["shape"])["x_hat"].cpu()         # = decompress of the reference's strings
    psnr = -10.0 * math.log10(torch.mean((x - x_hat) ** 2).item())
    assert abs(psnr - c["psnr"]) < 1e-4
    assert abs(8.0 * (len(ys[0]) + sum(map(len, zs))) / (c["B"] * c["H"] * c["W"]) - c["bpp"]) < 1e-12


def test_bad_streams_raise_on_the_host():
    from progressivecodec_amd._lib import PcodecError
    c = wacnn_cases()[2]                                                     # B = 3
    x = inputs(c["B"], c["H"], c["W"], c["seed"], c["kind"])
    net = gpu_wacnn()
    o = net.compress(x.cuda())
    (y,), zs = o["strings"]
    zh, zw = o["shape"]
    good = net.decompress(o["strings"], o["shape"])["x_hat"].cpu()
    for strings, shape in (([[y[:-4]], zs], (zh, zw)),                      # truncated
                           ([[y[: len(y) // 2]], zs], (zh, zw)),
                           ([[y], zs[:2]], (zh, zw)),                        # another batch size
                           ([[y], zs + zs[:1]], (zh, zw)),
                           ([[y], zs], (zh, zw + 1)),                        # another shape
                           ([[y], zs], (zh + 1, zw))):
        with pytest.raises(PcodecError):
            net.decompress(strings, shape)
    assert torch.equal(net.decompress(o["strings"], o["shape"])["x_hat"].cpu(), good)      # the object is still sound


def test_two_models_in_one_process_and_entry_points_refuse_each_other():
    from progressivecodec_amd import ChannelProgresssiveWACNN
    from progressivecodec_amd._lib import lib
    c = wacnn_cases()[0]
    x = inputs(c["B"], c["H"], c["W"], c["seed"], c["kind"]).cuda()
    chan = ChannelProgresssiveWACNN(device="cuda:0")
    chan.load_state_dict(synth_sd())
    wac = gpu_wacnn()
    alone_w = wac.compress(x)["strings"]
    alone_c = chan.compress(x, quality=0.5, mask_pol="point-based-std")["strings"]
    w2 = wac.compress(x)["strings"]
    c2 = chan.compress(x, quality=0.5, mask_pol="point-based-std")["strings"]
    assert w2 == alone_w and c2 == alone_c
    assert sha(w2[0][0]) == c["y_sha"]
    L, B, H, W = lib(), c["B"], c["H"], c["W"]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    xp = C.c_void_p(x.data_ptr())
    out = torch.empty((B, 3, H, W), device="cuda")
    yl = torch.empty((B, 640, H // 16, W // 16), device="cuda")
    zl = torch.empty((B, 192, H // 64, W // 64), device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    assert L.pc_codec_compress(wac._h, xp, B, H, W, 0.0, 0, None, st) == -8
    assert L.pc_codec_forward(wac._h, xp, B, H, W, 0.0, 0, P(out), P(yl), P(zl), None, 0, st) == -8
    assert L.pc_codec_set_rem(wac._h, (C.c_double * 1)(0.5), 1) == -8
    assert L.pc_codec_wacnn_compress(chan._h, xp, B, H, W, st) == -8
    assert L.pc_codec_wacnn_forward(chan._h, xp, B, H, W, P(out), P(yl), P(zl), st) == -8
    zs = w2[1]
    zp = (C.c_char_p * B)(*zs)
    zlen = (C.c_size_t * B)(*map(len, zs))
    assert L.pc_codec_wacnn_decompress(chan._h, w2[0][0], len(w2[0][0]), zp, zlen, B, 1, 1, P(out), st) == -8
    assert L.pc_codec_set_model(chan._h, 1) == -8                           # finalised
    assert wac.compress(x)["strings"] == alone_w                            # nothing of the refused calls stuck


def test_schedule_options_do_not_change_results():
    from progressivecodec_amd import WACNN
    c = wacnn_cases()[2]
    x = inputs(c["B"], c["H"], c["W"], c["seed"], c["kind"]).cuda()
    ref = gpu_wacnn()
    o0 = ref.compress(x)
    d0 = ref.decompress(o0["strings"], o0["shape"])["x_hat"].cpu()
    f0 = ref(x)["x_hat"].cpu()
    for opts in ({"serial_schedule": 1}, {"lanes_enc": 2, "lanes_dec": 3}, {"lanes_enc": 3, "host_threads": 1}):
        net = WACNN.from_state_dict(wacnn_sd()).eval()
        for k, v in opts.items():
            net.set_option(k, v)
        o = net.compress(x)
        assert o["strings"] == o0["strings"], opts
        assert torch.equal(net.decompress(o["strings"], o["shape"])["x_hat"].cpu(), d0), opts
        assert torch.equal(net(x)["x_hat"].cpu(), f0), opts


def test_compress_single_rate_equals_per_call_coding():
    import torch.nn.functional as F
    from progressivecodec_amd import WACNN
    from progressivecodec_amd.harness import compress_single_rate, compute_padding
    from progressivecodec_amd.synth import synthetic_wacnn_state_dict
    nets = [gpu_wacnn()]
    n2 = WACNN(device="cuda:0")
    n2.load_state_dict(synthetic_wacnn_state_dict(seed=1))
    n2.update()
    nets.append(n2)
    imgs = [inputs(1, 176, 208, 71, "smooth"), inputs(1, 192, 192, 72, "rand")]          # > 160 pixels a side for MS-SSIM
    rows = compress_single_rate(nets, imgs, ms_ssim=True)
    assert len(rows) == 2
    for net, row in zip(nets, rows):
        bpp = psnr = 0.0
        for x in imgs:
            x = x.cuda()                                                    # the harness measures on the device
            h, w = x.shape[2:]
            pad, unpad = compute_padding(h, w)
            o = net.compress(F.pad(x, pad))
            x_hat = F.pad(net.decompress(o["strings"], o["shape"])["x_hat"], unpad).clamp_(0, 1)
            bpp += 8.0 * (sum(map(len, o["strings"][0])) + sum(map(len, o["strings"][1]))) / (h * w)
            psnr += -10.0 * math.log10(torch.mean((x - x_hat) ** 2).item())
        assert row[0] == pytest.approx(bpp / 2, rel=1e-12) and row[1] == pytest.approx(psnr / 2, rel=1e-9)
        assert 0.0 < row[2] <= 1.0
    assert rows[0][0] != rows[1][0]


def test_forward_refuses_training_mode_and_module_surface():
    from progressivecodec_amd import WACNN
    net = WACNN.from_state_dict(wacnn_sd())
    x = inputs(1, 64, 64, 3, "rand").cuda()
    with pytest.raises(NotImplementedError):
        net.train()(x)
    sd = net.state_dict()
    assert "g_s.8.weight" in sd and "h_mean_s.8.weight" in sd and "gaussian_conditional._quantized_cdf" in sd
    assert sum(p.numel() for p in net.parameters()) > 0
    assert net.update() is False
    assert net.eval().compress(x)["strings"] == gpu_wacnn().compress(x)["strings"]

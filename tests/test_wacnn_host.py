"""WACNN (reference models/cnn.py:23-340) on the host: the state-dict layout against the reference's key list, the contract of
tests/wacnn_contract.py against the reference's own strings, x_hat and likelihoods (tests/golden/make_golden_wacnn.py) -- exactly in
the numeric-contract back-end, which is the same on every CPU, to rounding in the ATen one, which is not -- the single-stream framing
through the library's coder, and the configuration check.  No GPU."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests.util import GOLD, inputs, tables_npz

sha = lambda b: hashlib.sha256(b).hexdigest()


@functools.lru_cache(maxsize=None)
def wacnn_cases():
    return json.load(open(os.path.join(GOLD, "wacnn.json")))


def wacnn_sd(seed=0):
    """synthetic WACNN weights with the CDF tables the reference built for them (tests/golden/tables.npz, asserted by the generator)"""
    from progressivecodec_amd.synth import synthetic_wacnn_state_dict
    sd = synthetic_wacnn_state_dict(seed)
    t = tables_npz()
    for p, k in (("gaussian_conditional", "gc"), ("entropy_bottleneck", "eb")):
        sd[p + "._quantized_cdf"] = torch.from_numpy(t[k + "_cdf"])
        sd[p + "._cdf_length"] = torch.from_numpy(t[k + "_len"])
        sd[p + "._offset"] = torch.from_numpy(t[k + "_off"])
    return sd


def test_param_spec_equals_reference_keys():
    from progressivecodec_amd.arch import wacnn_param_spec
    ref = json.load(open(os.path.join(GOLD, "wacnn_keys.json")))
    spec = wacnn_param_spec()
    assert list(spec) == [k for k, _ in ref]                                   # same keys, same order
    for k, shape in ref:
        if spec[k][2] not in ("table", "scale_table"):                         # buffers that stay empty until update()
            assert list(spec[k][0]) == shape, k


def _psnr(x, x_hat):
    return -10.0 * np.log10(torch.mean((x - x_hat) ** 2).item())


@pytest.mark.parametrize("case", range(3))
def test_contract_reproduces_reference_strings(case):
    """The numeric-contract back-end -- plain C plus exact elementwise ops, the same on every CPU, and what the GPU reproduces bit for
    bit -- gives the reference's own y and z strings (the generator chose cases where it does, wacnn.json: cdet_strings_equal).  Its
    x_hat differs from the reference's by float rounding only: the synthesis transform is the reference's arithmetic in another order."""
    from tests.wacnn_contract import WacnnCodec
    c = wacnn_cases()[case]
    assert c["cdet_strings_equal"]
    x = inputs(c["B"], c["H"], c["W"], c["seed"], c["kind"])
    codec = WacnnCodec(wacnn_sd(), "cdet")
    out = codec.compress(x)
    ys, zs = out["strings"]
    assert len(ys) == 1 and len(zs) == c["B"]
    assert sha(ys[0]) == c["y_sha"] and len(ys[0]) == c["y_len"]
    assert [sha(s) for s in zs] == c["z_sha"]
    assert list(out["shape"]) == c["shape"]
    nbytes = len(ys[0]) + sum(len(s) for s in zs)
    assert abs(8.0 * nbytes / (c["B"] * c["H"] * c["W"]) - c["bpp"]) < 1e-12
    x_hat = codec.decompress(out["strings"], out["shape"])["x_hat"]
    assert abs(_psnr(x, x_hat) - c["psnr"]) < 1e-5
    g = np.load(os.path.join(GOLD, "wacnn_xhat.npz"))
    dec = x_hat.numpy() if case < 2 else x_hat.numpy()[:, :, ::4, ::4]
    assert np.abs(dec - g[f"dec_{case}"]).max() <= 2e-3


@pytest.mark.parametrize("case", range(3))
def test_torch_contract_agrees_with_reference_to_rounding(case):
    """The ATen back-end follows the reference's own operations; its convolutions round as the CPU's oneDNN kernels do, which depends
    on the machine (an AVX2-only CPU and the AVX-512 one that made the fixtures differ in the last bits, and a symbol can flip).  Same
    bounds as the progressive model's contract test: PSNR within 2e-3 dB, bpp within 0.2 %."""
    from tests.wacnn_contract import WacnnCodec
    c = wacnn_cases()[case]
    torch.set_num_threads(8)
    x = inputs(c["B"], c["H"], c["W"], c["seed"], c["kind"])
    codec = WacnnCodec(wacnn_sd(), "torch")
    out = codec.compress(x)
    ys, zs = out["strings"]
    assert len(ys) == 1 and len(zs) == c["B"] and list(out["shape"]) == c["shape"]
    x_hat = codec.decompress(out["strings"], out["shape"])["x_hat"]
    assert abs(_psnr(x, x_hat) - c["psnr"]) < 2e-3
    assert abs(8.0 * (len(ys[0]) + sum(map(len, zs))) / (c["B"] * c["H"] * c["W"]) - c["bpp"]) < 2e-3 * c["bpp"]


@pytest.mark.parametrize("case", range(3))
def test_contract_forward_matches_reference(case):
    """forward (eval): x_hat unclamped and within rounding of the reference's, likelihoods of the same symbols"""
    from tests.wacnn_contract import WacnnCodec
    c = wacnn_cases()[case]
    x = inputs(c["B"], c["H"], c["W"], c["seed"], c["kind"])
    f = WacnnCodec(wacnn_sd(), "cdet").forward(x)
    g = np.load(os.path.join(GOLD, "wacnn_xhat.npz"))
    assert f["x_hat"].min() < 0 or f["x_hat"].max() > 1
    assert np.abs(f["x_hat"].numpy()[:, :, ::4, ::4] - g[f"fwd_xhat_{case}"]).max() <= 4e-3
    ly, ry = f["likelihoods"]["y"].numpy()[:, ::8, ::2, ::2], g[f"fwd_ylik_{case}"]
    assert (np.abs(ly - ry) / ry).max() <= 1e-3
    lz, rz = f["likelihoods"]["z"].numpy(), g[f"fwd_zlik_{case}"]
    assert (np.abs(lz - rz) / rz).max() <= 1e-5


def test_one_stream_over_all_slices_round_trips():
    """BufferedRansEncoder over ten slices of a batch = ONE encode call; ten decode_stream calls that carry the state read it back."""
    from progressivecodec_amd import entropy
    t = tables_npz()
    tab = entropy.CdfTables(t["gc_cdf"], t["gc_len"], t["gc_off"])
    rng = np.random.default_rng(5)
    B, per = 3, 32 * 4 * 8
    idx = rng.integers(0, 64, (10, B, per)).astype(np.int32)
    sym = np.round(rng.standard_normal((10, B, per)) * (1 + idx / 4)).astype(np.int32)
    sym[0, 0, :5] = [40, -40, 300, -300, 0]                                     # bypass-coded values too
    data = entropy.rans_encode(sym, idx, tab)
    dec = entropy.RansDecoder()
    dec.set_stream(data)
    for i in range(10):
        assert dec.decode_stream(idx[i].reshape(-1), tab, None, None) == sym[i].reshape(-1).tolist()
    per_image = [entropy.rans_encode(sym[:, b], idx[:, b], tab) for b in range(B)]
    assert data not in per_image and len(data) < sum(map(len, per_image)) + 8 * B


@pytest.mark.parametrize("kw", [dict(N=128), dict(M=192), dict(dim_chunk=16), dict(N=192, M=640)])
def test_unsupported_configuration_raises_before_any_hip_call(kw, monkeypatch):
    import progressivecodec_amd.model as model
    from progressivecodec_amd import WACNN
    from progressivecodec_amd.arch import wacnn_param_spec

    def no_lib():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(model, "lib", no_lib)
    with pytest.raises(NotImplementedError):
        WACNN(**kw)
    with pytest.raises(NotImplementedError):
        wacnn_param_spec(**kw)


def test_registry_mirrors_the_reference():
    import progressivecodec_amd as pc
    assert set(pc.models) == {"cnn", "channel", "rate"}
    assert pc.models["cnn"] is pc.WACNN and pc.models["channel"] is pc.ChannelProgresssiveWACNN
    assert pc.models["rate"] is pc.PostRateProcessedNetwork


def test_synthetic_weights_spread_the_scale_indices():
    """the recipe gives the coder real work: the reference's indices span 20+ of the 64 table rows in every golden case"""
    for c in wacnn_cases():
        hist = np.array(c["index_histogram"])
        assert (hist > 0).sum() >= 20 and c["y_len"] > 1000, c["case"]

"""Multi-level coding (compress_levels / decompress_levels) against one compress() / decompress() call per level, in every mode.

include/pcodec.h promises that every string, mask and x_hat of a levels call is bit-identical to what one single call per level returns.
The levels calls run two levels' enhancement chains side by side on two buffer sets (pc_codec.hip: second_level_set), so any state a chain
reads from a buffer that set 1 re-points is a way to be silently wrong.  These tests cross that promise with the axes the levels paths
branch on: the REM refinement (its three variants and the two-check-level branch), multiple_encoder, the mask policies, the schedule
options, cust_map, checkpoint_rep, NULL mask pointers, unsorted / duplicate level lists, odd decoder pairings and the large-image quantile
path.  One REM case is anchored to the CPU oracle, which a metamorphic check cannot replace (both paths wrong the same way).

The module builds its own codec objects: tests.util.gpu_codec() is shared with other modules, and no option is ever set on it.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.util import inputs, synth_sd  # noqa: E402

REM_LEVELS = [0.01, 0.25, 1.75]

# B = 2, 128x192.  LISTS[0] has coded levels below the first check level and in every refinement range; the encoder alternates buffer
# sets 0/1/0/1/0 over its five coded levels and the decoder's `rest` has 4 entries.  [0.5, 2] is the smallest list that uses set 1.
# The unsorted list leaves 3 entries in `rest`: one pair, then the last level alone on set 1.  [0.5, 0.5] repeats a level.
LISTS = {
    "mixed": [0, 0.005, 0.1, 0.5, 0, 2, 10],
    "pair": [0.5, 2],
    "unsorted": [2, 0.1, 0.5, 1],
    "duplicate": [0.5, 0.5],
}


def _plain():
    from progressivecodec_amd import ChannelProgresssiveWACNN
    net = ChannelProgresssiveWACNN(device="cuda:0")
    net.load_state_dict(synth_sd())
    return net


def _rem(check_levels, post_sd, **kw):
    from progressivecodec_amd import PostRateProcessedNetwork
    net = PostRateProcessedNetwork(_plain(), check_levels=check_levels, **kw)
    net.load_state_dict(synth_sd(), post_sd)
    return net


@functools.lru_cache(maxsize=None)
def net_of(name):
    """one object per name for this module; "*_sched" objects are the only ones options are set on (and reset after each test)"""
    from progressivecodec_amd.synth import synthetic_post_state_dict
    if name in ("plain", "plain_sched"):
        return _plain()
    if name in ("rem", "rem_sched"):
        from tests.test_oracle_vs_golden import rem_post_sd
        return _rem(REM_LEVELS, rem_post_sd())
    if name == "rem_mu_std_middle":
        return _rem(REM_LEVELS, synthetic_post_state_dict(3, "middle", mu_std=True), mu_std=True, dimension="middle")
    if name == "rem_two_checks":
        return _rem([0.1, 1.0], synthetic_post_state_dict(2, "big"))
    if name == "multiple_encoder":
        from progressivecodec_amd import ChannelProgresssiveWACNN
        from tests.test_oracle_vs_golden import multienc_sd
        net = ChannelProgresssiveWACNN(device="cuda:0", multiple_encoder=True)
        net.load_state_dict(multienc_sd())
        return net
    raise KeyError(name)


def _odd_rest_subset(levels):
    """indices of a reversed subset of `levels` with an even number of coded levels (>= 2): the decoder pipelines the first coded one with
    the base chain, and the odd number left in `rest` ends on a level decoded alone on buffer set 1"""
    idx = list(reversed(range(len(levels))))
    coded = [i for i in idx if levels[i] != 0]
    assert len(coded) >= 2
    if len(coded) % 2:
        idx.remove(coded[-1])
    return idx


def assert_levels_equal_singles(net, x, levels, pol, **state):
    """compress_levels == [compress(x, q) ...] and decompress_levels == per-level decompress: z and y strings byte for byte, shape,
    every mask and every x_hat bitwise.  A reversed subset whose decoder `rest` has odd length decodes to the same pictures.  `state`
    (cust_map / checkpoint_rep) goes to every call.  Returns the levels call's dictionaries and x_hats."""
    datas = net.compress_levels(x, levels, pol, **state)
    assert len(datas) == len(levels)
    singles = [net.compress(x, q, pol, **state) for q in levels]
    for q, d, s in zip(levels, datas, singles):
        assert d["strings"][1] == s["strings"][1], f"z strings differ at level {q}"
        assert len(d["strings"][0]) == len(s["strings"][0]) == (20 if q > 0 else 10), f"slice count at level {q}"
        for i, (a, b) in enumerate(zip(d["strings"][0], s["strings"][0])):
            assert a == b, f"y strings of slice {i} differ at level {q}"
        assert tuple(d["shape"]) == tuple(s["shape"])
        assert len(d["masks"]) == len(s["masks"]) == (10 if q > 0 else 0)
        for i, (m, ms) in enumerate(zip(d["masks"], s["masks"])):
            assert torch.equal(m, ms), f"mask of slice {i} differs at level {q}"
    outs = net.decompress_levels([d["strings"] for d in datas], datas[0]["shape"], levels, pol, **state)
    assert len(outs) == len(levels)
    x_hats = []
    for q, o, s in zip(levels, outs, singles):
        ref = net.decompress(s["strings"], s["shape"], q, pol, **state)["x_hat"]
        assert torch.equal(o["x_hat"], ref), f"x_hat differs at level {q}"
        x_hats.append(ref.clone())
    sub = _odd_rest_subset(levels)
    outs2 = net.decompress_levels([datas[i]["strings"] for i in sub], datas[0]["shape"], [levels[i] for i in sub], pol, **state)
    for j, i in enumerate(sub):
        assert torch.equal(outs2[j]["x_hat"], x_hats[i]), f"x_hat of level {levels[i]} differs in the subset {[levels[i] for i in sub]}"
    return datas, x_hats


def _x(B=2, H=128, W=192, seed=71):
    return inputs(B, H, W, seed).cuda()


# ------------------------------------------------------------------ every object x every list (point-based-std, default schedule)
OBJECTS = ["plain", "rem", "rem_mu_std_middle", "rem_two_checks", "multiple_encoder"]


@pytest.mark.parametrize("lst", list(LISTS))
@pytest.mark.parametrize("obj", OBJECTS)
def test_levels_equal_singles(obj, lst):
    assert_levels_equal_singles(net_of(obj), _x(), LISTS[lst], "point-based-std")


def test_rem_levels_differ_from_plain():
    """the REM switch is really on inside the levels calls: refined levels code different enhancement strings than the plain codec"""
    x = _x()
    rem = net_of("rem").compress_levels(x, [0.5, 2], "point-based-std")
    plain = net_of("plain").compress_levels(x, [0.5, 2], "point-based-std")
    for r, p in zip(rem, plain):
        assert r["strings"][1] == p["strings"][1] and r["strings"][0][:10] == p["strings"][0][:10]
        assert r["strings"][0][10:] != p["strings"][0][10:]
        assert "y_hat" not in r


# ------------------------------------------------------------------ mask policies
@pytest.mark.parametrize("pol", ["two-levels", "three-levels-std"])
@pytest.mark.parametrize("obj", ["plain", "rem"])
def test_mask_policies(obj, pol):
    assert_levels_equal_singles(net_of(obj), _x(seed=72), [0, 1, 2, 0.5], pol)


# ------------------------------------------------------------------ schedule options (a dedicated object each; options reset afterwards)
@pytest.mark.parametrize("opts", [{"serial_schedule": 1}, {"lanes_enc": 2, "lanes_dec": 3}, {"host_threads": 2}], ids=["serial", "lanes", "host_threads"])
@pytest.mark.parametrize("obj", ["plain", "rem"])
def test_schedule_options(obj, opts):
    net = net_of(obj + "_sched")
    base = net.base_net if obj == "rem" else net
    want = [d["strings"] for d in net_of(obj).compress_levels(_x(), LISTS["mixed"], "point-based-std")]
    try:
        for k, v in opts.items():
            base.set_option(k, v)
        datas, _ = assert_levels_equal_singles(net, _x(), LISTS["mixed"], "point-based-std")
    finally:
        for k in ("serial_schedule", "lanes_enc", "lanes_dec", "host_threads"):
            base.set_option(k, 0)
    assert [d["strings"] for d in datas] == want, "the schedule option changed the strings"


# ------------------------------------------------------------------ cust_map
class _RemWithCustMap:
    """The REM net with a cust_map: the refinement switched on around the base object's calls, which take the map.  (The reference's
    PostRateProcessedNetwork has no cust_map argument; the combination is reachable through the C ABI, which this exercises.)"""

    def __init__(self, rem):
        self.rem = rem

    def _call(self, fn, B, h, w, *a, **kw):
        self.rem._on(None, B, h, w)
        try:
            return fn(*a, **kw)
        finally:
            self.rem._off()

    def compress(self, x, q, pol, cust_map=None):
        return self._call(self.rem.base_net.compress, x.shape[0], x.shape[2] // 16, x.shape[3] // 16, x, q, pol, cust_map)

    def decompress(self, strings, shape, q, pol, cust_map=None):
        return self._call(self.rem.base_net.decompress, len(strings[1]), 4 * int(shape[0]), 4 * int(shape[1]), strings, shape, q, pol, cust_map)

    def compress_levels(self, x, qs, pol, cust_map=None):
        return self._call(self.rem.base_net.compress_levels, x.shape[0], x.shape[2] // 16, x.shape[3] // 16, x, qs, pol, cust_map=cust_map)

    def decompress_levels(self, spl, shape, qs, pol, cust_map=None):
        return self._call(self.rem.base_net.decompress_levels, len(spl[0][1]), 4 * int(shape[0]), 4 * int(shape[1]), spl, shape, qs, pol,
                          cust_map=cust_map)


@pytest.mark.parametrize("obj", ["plain", "rem"])
def test_cust_map(obj):
    net = net_of(obj)
    net = _RemWithCustMap(net) if obj == "rem" else net
    x = _x(seed=73)
    cm = torch.rand(2, 320, 8, 12, generator=torch.Generator().manual_seed(74)).cuda()
    datas, _ = assert_levels_equal_singles(net, x, LISTS["mixed"], "point-based-std", cust_map=cm)
    without = [d["strings"] for d in net_of(obj).compress_levels(x, LISTS["mixed"], "point-based-std")]
    assert [d["strings"] for d in datas] != without, "the custom map must change the enhancement strings"


def test_cust_map_shape_is_checked():
    net = net_of("plain")
    with pytest.raises(ValueError):
        net.compress_levels(_x(), [0.5, 2], "point-based-std", cust_map=torch.rand(2, 320, 8, 8).cuda())


# ------------------------------------------------------------------ REM with checkpoint_rep
def test_rem_checkpoint_rep():
    net = net_of("rem")
    x = _x(seed=75)
    rep = net.compress(x, 0.25, "point-based-std")["y_hat"]
    datas, x_hats = assert_levels_equal_singles(net, x, LISTS["mixed"], "point-based-std", checkpoint_rep=rep)
    without = net.compress_levels(x, LISTS["mixed"], "point-based-std")
    assert [d["strings"] for d in datas] != [d["strings"] for d in without], "the checkpoint representation must change the strings"
    with pytest.raises(ValueError):
        net.compress_levels(x, [0.5, 2], "point-based-std", checkpoint_rep=rep[:1])


# ------------------------------------------------------------------ masks_out NULL for a coded level (C ABI)
@pytest.mark.parametrize("obj", ["plain", "rem"])
def test_null_mask_pointer_for_a_coded_level(obj):
    from progressivecodec_amd._lib import check, lib
    from progressivecodec_amd.model import _MASK_POL
    net = net_of(obj)
    base = net.base_net if obj == "rem" else net
    x = _x(seed=76).contiguous()
    levels = [0.1, 0.5, 2, 0, 1]
    want = net.compress_levels(x, levels, "point-based-std")
    B, _, H, W = x.shape
    masks = [torch.full((10, B, 32, H // 16, W // 16), -1.0, device=x.device) if q > 0 else None for q in levels]
    masks[1] = None                                                     # coded level 0.5 (buffer set 1 in the encoder) gets no masks
    mp = (C.c_void_p * len(levels))(*[m.data_ptr() if m is not None else None for m in masks])
    qa = (C.c_double * len(levels))(*levels)
    if obj == "rem":
        net._on(None, B, H // 16, W // 16)
    try:
        check(lib().pc_codec_compress_levels(base._h, C.c_void_p(x.data_ptr()), B, H, W, qa, len(levels), _MASK_POL["point-based-std"], mp,
                                             base._stream()), "pc_codec_compress_levels")
    finally:
        if obj == "rem":
            net._off()
    strs = base._fetch_strings()
    n = len(strs)
    assert n == (10 + 10 * len(levels)) * B + B
    for lv, q in enumerate(levels):
        got = [strs[s * B:(s + 1) * B] for s in range(10)] + ([strs[(10 + 10 * lv + s) * B:(11 + 10 * lv + s) * B] for s in range(10)] if q > 0 else [])
        assert got == want[lv]["strings"][0], f"y strings differ at level {q}"
        if masks[lv] is not None:
            assert torch.equal(masks[lv], torch.stack(want[lv]["masks"])), f"masks differ at level {q}"
    assert strs[-B:] == want[0]["strings"][1]


# ------------------------------------------------------------------ large image: the per-tag scratch of the quantile path
@pytest.mark.parametrize("obj", ["plain", "rem"])
def test_large_image_quantile_path(obj):
    """B = 1, 512x640: a latent of 32x40, 40 960 keys per slice > PC_QUANTILE_SMALL_N (32768, pc_device.h) -- the mask thresholds (and the
    REM attention-mask thresholds) take the multi-workgroup quantile path, on per-tag scratch while two chains run side by side"""
    assert 32 * 40 * 32 > 32768
    assert_levels_equal_singles(net_of(obj), inputs(1, 512, 640, 77, "smooth").cuda(), [0.1, 0.5, 2], "point-based-std")


# ------------------------------------------------------------------ oracle anchor
def test_rem_levels_bit_exact_vs_oracle():
    """B = 1, 64x128, [0.1, 0.5]: 0.5 runs on buffer set 1 in the encoder and in the decoder.  Every string, mask and x_hat of the levels
    calls equals, bit for bit, the CPU contract oracle's per-level compress / decompress."""
    from tests.test_oracle_vs_golden import rem_oracle
    net = net_of("rem")
    x = inputs(1, 64, 128, 78)
    levels = [0.1, 0.5]
    datas = net.compress_levels(x.cuda(), levels, "point-based-std")
    outs = net.decompress_levels([d["strings"] for d in datas], datas[0]["shape"], levels, "point-based-std")
    orc = rem_oracle("cdet")
    for q, d, o in zip(levels, datas, outs):
        ref = orc.compress(x, q, "point-based-std")
        assert d["strings"][1] == ref["strings"][1], f"z strings differ from the oracle at level {q}"
        for s, (a, b) in enumerate(zip(d["strings"][0], ref["strings"][0])):
            assert a == b, f"y strings of slice {s} differ from the oracle at level {q}"
        assert len(d["strings"][0]) == len(ref["strings"][0]) == 20
        for m, rm in zip(d["masks"], ref["masks"]):
            assert np.array_equal(m.cpu().numpy(), rm.numpy()), f"masks differ from the oracle at level {q}"
        rdec = orc.decompress(ref["strings"], ref["shape"], q, "point-based-std")["x_hat"]
        assert np.array_equal(o["x_hat"].cpu().numpy().view(np.uint32), rdec.numpy().view(np.uint32)), f"x_hat differs from the oracle at level {q}"


# ------------------------------------------------------------------ REM through the harness
def test_rem_harness_shared_base_and_batching_give_the_same_rd_table():
    from progressivecodec_amd.harness import PR_LIST, compress_with_ac
    net = net_of("rem")
    imgs = [inputs(1, 64, 128, 31), inputs(1, 96, 72, 32, "smooth")]
    a = compress_with_ac(net, imgs, PR_LIST)
    b = compress_with_ac(net, imgs, PR_LIST, shared_base=True)
    assert a[0] == b[0] and a[1] == b[1]
    assert [(r["quality"], r["bpp"], r["psnr"]) for r in a[3]] == [(r["quality"], r["bpp"], r["psnr"]) for r in b[3]]
    c = compress_with_ac(net, imgs, PR_LIST, batch_same_size=True)
    assert [(r["quality"], r["bpp"]) for r in a[3]] == [(r["quality"], r["bpp"]) for r in c[3]]
    assert max(abs(r["psnr"] - s["psnr"]) for r, s in zip(a[3], c[3])) < 1e-5       # (means reduced on the GPU over different tensors)
    plain = compress_with_ac(net_of("plain"), imgs, PR_LIST, shared_base=True)
    assert plain[0] != b[0], "the REM must change the rates"


def test_codec_pipeline_refuses_the_rem_model():
    from progressivecodec_amd import CodecPipeline
    from progressivecodec_amd.harness import compress_with_ac
    with pytest.raises(TypeError, match="REM"):
        CodecPipeline.from_model(net_of("rem"))
    with pytest.raises(TypeError, match="REM"):
        compress_with_ac(net_of("rem"), [inputs(1, 64, 64, 33)], [0.5], overlap=True)

"""u_net_post (ChannelProgresssiveWACNN(u_net_post=1/2), CHProg_cnn.py:87-88,277-284) on the host: the state-dict layout against the
reference's own key list, and the contract restatement of the UNet post-filter (tests/unet_contract.py) against the reference's refine
outputs (tests/golden/make_golden_unet.py).  No GPU needed."""
import json
import os

import numpy as np
import pytest

from progressivecodec_amd.arch import CodecConfig, param_spec
from progressivecodec_amd.synth import synthetic_state_dict

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# max |restatement - reference| measured over the six fixture outputs: 8.6e-7 (float rounding of the two summation orders); asserted with margin
REFINE_TOL = 5e-6


@pytest.mark.parametrize("mode", [1, 2])
def test_param_spec_equals_the_reference_key_list(mode):
    ref = json.load(open(os.path.join(GOLD, "unet_keys.json")))[str(mode)]
    spec = param_spec(CodecConfig(u_net_post=mode))
    assert [k for k, _ in ref] == list(spec)
    assert all(tuple(s) == tuple(spec[k][0]) for k, s in ref if spec[k][2] != "table")     # (CDF tables: sized by update())


def test_mode_0_spec_is_unchanged():
    s0 = param_spec(CodecConfig())
    assert len(s0) == 1019 and not any(k.startswith("refine") for k in s0)
    s1 = param_spec(CodecConfig(u_net_post=1))
    assert list(s1)[:1019] == list(s0) and len(s1) == 1019 + 62
    assert len(param_spec(CodecConfig(u_net_post=2))) == 1019 + 124


def test_u_net_post_out_of_range_is_refused():
    with pytest.raises(AssertionError):
        CodecConfig(u_net_post=3).check_supported()


def test_synthetic_refine_weights_leave_work_for_the_clamp():
    """the synthetic refine recipe: a real share of every net's output strictly inside (0, 1), and the base weights unchanged"""
    from tests import unet_contract as uc
    sd0 = synthetic_state_dict(as_torch=False)
    sd2 = synthetic_state_dict(CodecConfig(u_net_post=2), as_torch=False)
    assert all(np.array_equal(sd0[k], sd2[k]) for k in sd0)
    x = np.load(os.path.join(GOLD, "unet_io_64x96.npz"))["x"]
    for pre in ("refine.0", "refine.1"):
        y = uc.refine(x, uc.refine_weights(sd2, pre))
        inside = float(((y > 0) & (y < 1)).mean())
        assert 0.5 < inside < 1.0, (pre, inside)


@pytest.mark.parametrize("tag", ["64x64", "64x96"])
def test_restatement_matches_the_reference_refine(tag):
    from tests import unet_contract as uc
    d = np.load(os.path.join(GOLD, f"unet_io_{tag}.npz"))
    sd1 = synthetic_state_dict(CodecConfig(u_net_post=1), as_torch=False)
    sd2 = synthetic_state_dict(CodecConfig(u_net_post=2), as_torch=False)
    for key, sd, pre in (("refine", sd1, "refine"), ("refine0", sd2, "refine.0"), ("refine1", sd2, "refine.1")):
        y = uc.refine(d["x"], uc.refine_weights(sd, pre))
        err = float(np.abs(y - d[key]).max())
        assert err < REFINE_TOL, (tag, key, err)

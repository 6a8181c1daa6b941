"""Layer 1 of the hyper-synthesis nets that run together is packed as ONE conv of n * 192 output channels (pc_codec.hip: load_hs_cat --
the module weights appended along the output channel, then pc_pack_conv_weight).  Here, on the host: that pack is the per-net packs
placed side by side along the output channel, for n = 2 and n = 4, in the layout the launcher picks for the layer -- so output channel
192 j + o of the wide layer reads exactly the weights of channel o of net j."""
import ctypes as C

import numpy as np
import pytest

from progressivecodec_amd._lib import lib

CIN, COUT, K = 192, 192, 3


def _pack(w, cout):
    out = np.empty(K * K * CIN * cout, np.float32)
    rc = lib().pc_pack_conv_weight(np.ascontiguousarray(w, np.float32).ctypes.data_as(C.c_void_p), 0, cout, CIN, K,
                                   out.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("n", [2, 4])
def test_concatenated_layer1_pack_is_the_per_net_packs_side_by_side(n):
    rng = np.random.default_rng(100 + n)
    ws = [rng.standard_normal((COUT, CIN, K, K)).astype(np.float32) for _ in range(n)]
    wide = _pack(np.concatenate(ws, axis=0), n * COUT).reshape(K * K, n * COUT, CIN)      # layout 1: [tap][Cout][Cin]
    for j, w in enumerate(ws):
        one = _pack(w, COUT).reshape(K * K, COUT, CIN)
        # the per-net pack itself is the module weight with K contiguous per output channel
        assert np.array_equal(one, w.transpose(2, 3, 0, 1).reshape(K * K, COUT, CIN))
        assert np.array_equal(wide[:, j * COUT:(j + 1) * COUT, :].view(np.uint32), one.view(np.uint32)), f"net {j} of {n}"
    # nothing else in the wide pack: the slices above cover it
    assert wide.shape[1] == n * COUT

#!/usr/bin/env python3
"""Golden fixtures for the single-rate model WACNN (/root/reference/src/compress/models/cnn.py:23-340), produced by the REAL reference
imported read-only through tests/golden/ref_env.py, on the build-owned synthetic weights (progressivecodec_amd.synth.
synthetic_wacnn_state_dict) and seeded inputs (tests/util.py:inputs).

Run once in the build container:   python3 tests/golden/make_golden_wacnn.py
Output (committed, data only):
  wacnn_keys.json   -- the reference WACNN(192, 320).state_dict() keys and shapes
  wacnn.json        -- per case: sha256 / length of the batch's y string and of every z string, shape, bpp, PSNR; whether the numeric-
                       contract back-end of tests/wacnn_contract.py reproduces the strings (cdet_strings_equal) -- the GPU tests compare
                       the GPU's strings with the reference's only where it does
  wacnn_xhat.npz    -- decompress x_hat (case 2 subsampled 4x), forward x_hat (unclamped, 4x subsampled), y likelihoods (channels 8x,
                       pixels 2x subsampled) and z likelihoods
The reference's CDF tables for these weights equal tests/golden/tables.npz (asserted): the GaussianConditional's depend on the scale
table only, and the EntropyBottleneck's tensors carry the same names -- hence the same synthetic values -- as the progressive model's.
"""
import hashlib
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import ref_env  # noqa: E402

ref_env.setup()
import numpy as np  # noqa: E402
import torch  # noqa: E402
from compress.models import WACNN  # noqa: E402

from progressivecodec_amd.synth import synthetic_wacnn_state_dict  # noqa: E402
from tests.util import inputs, tables_npz  # noqa: E402
from tests.wacnn_contract import WacnnCodec  # noqa: E402

torch.set_num_threads(8)
sha = lambda b: hashlib.sha256(b).hexdigest()

#: (B, H, W, seed, kind)
CASES = [(2, 64, 64, 41, "rand"), (1, 128, 192, 42, "smooth"), (3, 64, 128, 44, "smooth")]

torch.manual_seed(0)
net = WACNN(192, 320).eval()
json.dump([[k, list(v.shape)] for k, v in net.state_dict().items()], open(os.path.join(HERE, "wacnn_keys.json"), "w"))
net.load_state_dict(synthetic_wacnn_state_dict())
net.update(force=True)
sd = net.state_dict()
t = tables_npz()
for k, f in (("gaussian_conditional._quantized_cdf", "gc_cdf"), ("gaussian_conditional._cdf_length", "gc_len"),
             ("gaussian_conditional._offset", "gc_off"), ("entropy_bottleneck._quantized_cdf", "eb_cdf"),
             ("entropy_bottleneck._cdf_length", "eb_len"), ("entropy_bottleneck._offset", "eb_off")):
    assert np.array_equal(sd[k].numpy(), t[f]), k
cdet = WacnnCodec({k: v.clone() for k, v in sd.items()}, "cdet")

seen = []                                                                 # the scale indices compress() builds, for the histogram
_bi = net.gaussian_conditional.build_indexes
net.gaussian_conditional.build_indexes = lambda scales: seen.append(_bi(scales)) or seen[-1]

cases, arrays = [], {}
for n, (B, H, W, seed, kind) in enumerate(CASES):
    x = inputs(B, H, W, seed, kind)
    seen.clear()
    with torch.no_grad():
        o = net.compress(x)
    hist = np.bincount(torch.cat([i.reshape(-1) for i in seen]).numpy(), minlength=64)
    with torch.no_grad():
        d = net.decompress(o["strings"], o["shape"])
        f = net(x)
    ys, zs = o["strings"]
    x_hat = d["x_hat"]
    nbytes = sum(len(s) for s in ys) + sum(len(s) for s in zs)
    oc = cdet.compress(x)
    same = oc["strings"][0][0] == ys[0] and oc["strings"][1] == zs
    case = dict(case=n, B=B, H=H, W=W, seed=seed, kind=kind, shape=list(o["shape"]), y_sha=sha(ys[0]), y_len=len(ys[0]),
                z_sha=[sha(s) for s in zs], z_len=[len(s) for s in zs], bpp=8.0 * nbytes / (B * H * W),
                psnr=-10.0 * math.log10(torch.mean((x - x_hat) ** 2).item()), x_hat_sha=sha(x_hat.numpy().tobytes()),
                cdet_strings_equal=bool(same), index_histogram=hist.tolist())
    cases.append(case)
    arrays[f"dec_{n}"] = x_hat.numpy() if n < 2 else x_hat.numpy()[:, :, ::4, ::4].copy()
    arrays[f"fwd_xhat_{n}"] = f["x_hat"].numpy()[:, :, ::4, ::4].copy()
    arrays[f"fwd_ylik_{n}"] = f["likelihoods"]["y"].numpy()[:, ::8, ::2, ::2].copy()
    arrays[f"fwd_zlik_{n}"] = f["likelihoods"]["z"].numpy()
    print(n, B, H, W, kind, "y bytes", len(ys[0]), "bpp %.4f psnr %.4f" % (case["bpp"], case["psnr"]), "cdet strings equal:", same,
          "indexes used:", int((hist > 0).sum()), "max", int(np.nonzero(hist)[0].max()), flush=True)
json.dump(cases, open(os.path.join(HERE, "wacnn.json"), "w"), indent=0)
np.savez(os.path.join(HERE, "wacnn_xhat.npz"), **arrays)
print("done")

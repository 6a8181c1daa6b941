#!/usr/bin/env python3
"""Golden fixtures for the UNet post-filter -- ChannelProgresssiveWACNN(u_net_post=1 / 2) (/root/reference/src/compress/models/
CHProg_cnn.py:87-88,277-284; layers/unet.py) -- produced by the REAL reference imported read-only through tests/golden/ref_env.py, on the
build-owned synthetic weights (progressivecodec_amd.synth.synthetic_state_dict with the refine.* recipe) and seeded inputs.

Run once in the build container:   python3 tests/golden/make_golden_unet.py
Output (committed, data only):
  unet_keys.json        -- the reference's state_dict key list and shapes for u_net_post = 1 and 2
  unet_io_64x64.npz     -- x [2,3,64,64] and the unclamped outputs of refine (mode 1) and refine[0] / refine[1] (mode 2)
  unet_io_64x96.npz     -- the same at [1,3,64,96]
  unet_e2e.json / .npz  -- compress / decompress at 1x3x64x128, q in {0, 0.5}, both modes: string hashes, bpp, PSNR and x_hat
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
from compress.models import ChannelProgresssiveWACNN  # noqa: E402

from progressivecodec_amd.arch import CodecConfig  # noqa: E402
from progressivecodec_amd.synth import synthetic_state_dict  # noqa: E402
from tests.util import inputs  # noqa: E402

torch.set_num_threads(8)
sha = lambda b: hashlib.sha256(b).hexdigest()


def model(mode):
    torch.manual_seed(0)
    net = ChannelProgresssiveWACNN(
        N=192, M=640, division_dimension=[320, 640], dim_chunk=32,
        multiple_decoder=True, multiple_encoder=False, multiple_hyperprior=True,
        mask_policy="two-levels", lmbda_list=[0.0055, 0.04], joiner_policy="res",
        support_progressive_slices=5, delta_encode=True, u_net_post=mode).eval()
    net.load_state_dict(synthetic_state_dict(CodecConfig(u_net_post=mode)))
    net.update(force=True)
    return net


nets = {m: model(m) for m in (1, 2)}
json.dump({str(m): [[k, list(v.shape)] for k, v in n.state_dict().items()] for m, n in nets.items()},
          open(os.path.join(HERE, "unet_keys.json"), "w"))

for tag, (B, H, W, seed) in (("64x64", (2, 64, 64, 31)), ("64x96", (1, 64, 96, 32))):
    x = inputs(B, H, W, seed, "smooth")
    with torch.no_grad():
        out = dict(x=x.numpy(), refine=nets[1].refine(x).numpy(), refine0=nets[2].refine[0](x).numpy(), refine1=nets[2].refine[1](x).numpy())
    np.savez(os.path.join(HERE, f"unet_io_{tag}.npz"), **out)
    print(tag, {k: float(np.abs(v).mean()) for k, v in out.items()}, flush=True)

cases, arrays = [], {}
x = inputs(1, 64, 128, 33, "smooth")
for mode in (1, 2):
    for q in (0.0, 0.5):
        with torch.no_grad():
            o = nets[mode].compress(x, quality=q, mask_pol="point-based-std")
            d = nets[mode].decompress(o["strings"], o["shape"], q, mask_pol="point-based-std")
        ys, zs = o["strings"]
        x_hat = d["x_hat"]
        name = f"mode{mode}_q{q}"
        arrays[name] = x_hat.numpy()
        nbytes = sum(len(s) for sl in ys for s in sl) + sum(len(s) for s in zs)
        cases.append(dict(case=name, mode=mode, quality=q, B=1, H=64, W=128, seed=33, kind="smooth", mask_pol="point-based-std",
                          shape=list(o["shape"]), y_sha=[[sha(s) for s in sl] for sl in ys], z_sha=[sha(s) for s in zs],
                          bpp=8.0 * nbytes / (64 * 128), psnr=-10.0 * math.log10(torch.mean((x - x_hat.clamp(0, 1)) ** 2).item())))
        print(name, cases[-1]["bpp"], cases[-1]["psnr"], flush=True)
json.dump(cases, open(os.path.join(HERE, "unet_e2e.json"), "w"), indent=0)
np.savez(os.path.join(HERE, "unet_e2e.npz"), **arrays)
print("done")

#!/usr/bin/env python3
"""Golden fixtures for the topology switches of ChannelProgresssiveWACNN (models/CHProg_cnn.py:29-49), produced by the REAL reference
imported read-only through tests/golden/ref_env.py, on the build-owned synthetic weights of each variant (tests/topology_contract.py:
VARIANTS, variant_sd) and seeded inputs (tests/util.py:inputs).

Run once in the build container:   python3 tests/golden/make_golden_topology.py
Output (committed, data only):
  topology_keys.json -- per variant: the number of the reference state_dict() keys and the digest of its keys and shapes, in
                        order (tests/topology_contract.py:layout_digest)
  topology.json      -- per variant and case: digests of the y and z strings (strings_digest), the number of y slots, bpp and
                        PSNR of decompress, whether the numeric-contract back-end of tests/topology_contract.py reproduces the
                        strings (cdet_strings_equal)
"""
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
import torch  # noqa: E402
from compress.models.CHProg_cnn import ChannelProgresssiveWACNN  # noqa: E402

from tests.topology_contract import CASES, VARIANTS, TopologyCodec, layout_digest, strings_digest, variant_cfg, variant_sd  # noqa: E402
from tests.util import inputs  # noqa: E402

torch.set_num_threads(8)
# the reference's constructor defaults that differ from the canonical topology, pinned for every variant before its own switches
BASE = dict(multiple_encoder=False, multiple_hyperprior=True, delta_encode=True, support_progressive_slices=5, joiner_policy="res")

keys, out = {}, {}
for name, kw in VARIANTS.items():
    torch.manual_seed(0)
    net = ChannelProgresssiveWACNN(**{**BASE, **kw}).eval()
    layout = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    keys[name] = dict(n=len(layout), sha256=layout_digest(layout))
    sd = variant_sd(name)
    net.load_state_dict(sd)
    cdet = TopologyCodec({k: v.clone() for k, v in sd.items()}, variant_cfg(name), "cdet")
    cases = []
    for n, (B, H, W, seed, kind, q, pol) in enumerate(CASES):
        x = inputs(B, H, W, seed, kind)
        with torch.no_grad():
            o = net.compress(x, quality=q, mask_pol=pol)
            d = net.decompress(o["strings"], o["shape"], quality=q, mask_pol=pol)
        ys, zs = o["strings"]
        nbytes = sum(len(s) for sl in ys for s in sl) + sum(len(s) for s in zs)
        oc = cdet.compress(x, q, pol)
        same = oc["strings"][0] == ys and oc["strings"][1] == zs
        case = dict(case=n, B=B, H=H, W=W, seed=seed, kind=kind, quality=q, mask_pol=pol,
                    y_slots=len(ys), y_digest=strings_digest(ys), z_digest=strings_digest(zs), bpp=8.0 * nbytes / (B * H * W),
                    psnr=-10.0 * math.log10(torch.mean((x - d["x_hat"]) ** 2).item()), cdet_strings_equal=bool(same))
        cases.append(case)
        print(name, n, B, H, W, q, pol, "slots", len(ys), "bpp %.4f psnr %.4f" % (case["bpp"], case["psnr"]), "cdet equal:", same, flush=True)
    out[name] = cases
with open(os.path.join(HERE, "topology_keys.json"), "w") as f:
    f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in keys.items()) + "\n}\n")
with open(os.path.join(HERE, "topology.json"), "w") as f:                  # one case per line
    f.write("{\n" + ",\n".join(f"{json.dumps(k)}: [\n" + ",\n".join(json.dumps(c) for c in v) + "]" for k, v in out.items()) + "\n}\n")
print("done")

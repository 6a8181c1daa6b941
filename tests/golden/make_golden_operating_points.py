#!/usr/bin/env python3
"""Goldens of the REAL reference at the operating points of tests/operating_points.py (the default recipe, a second seed, and the
five edited weight sets that leave the 3.56 bpp / index 0..27 regime of every other golden).

Run once in the build container:   python3 tests/golden/make_golden_operating_points.py
Outputs (data only; inputs are regenerated from seeds):
  operating_points_tables.npz   the entropy-bottleneck tables after net.update(force=True), once per seed other than 0 (seed 0's
                                are tables.npz's; the Gaussian tables depend on the scale table alone and are asserted equal to
                                tables.npz's at every point)
  operating_points.json         records: per (point, case, quality, mask policy) the shape, sha256 + length of every string, mask
                                popcounts, bpp / PSNR as make_golden.py computes them, the histogram of the coded scale indexes and
                                the y / z escape counts (tests/operating_points.call_stats on the reference's own symbols), bytes and
                                PSNR per image; at op.DEV_POINTS / op.DEV_CASES also `oracle_dev`: how far the contract oracle (run here, on the
                                CPU) is from the reference in bpp and PSNR, and how many y strings the two share
  operating_points_strings_<point>.json   for op.STRING_CASE at op.STRING_POINTS: every byte string as hex, per-image PSNR
                                and a strided subsample of the reference's x_hat
"""
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import ref_env  # noqa: E402

net = ref_env.canonical_model()
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from compressai import ans  # noqa: E402  (built from the reference's vendored sources)

from tests import operating_points as op  # noqa: E402

torch.set_num_threads(8)
base_t = dict(np.load(os.path.join(HERE, "tables.npz")))

cap = {}


def capture(net):
    """record the indexes and symbols of every GaussianConditional.compress call of `net`"""
    gc = net.gaussian_conditional
    orig = gc.compress

    def _cmp(inp, idx, means=None, flag=1):
        cap.setdefault("cmp", []).append((idx.clone(), gc.quantize(inp, "symbols", means).clone()))
        return orig(inp, idx, means)

    gc.compress = _cmp


tables, records, strings = {}, [], []
runs = op.all_runs() + op.string_runs()
for point, (seed, _) in op.POINTS.items():
    if point != "default":
        net = ref_env.canonical_model()          # a model whose tables were built no longer loads a state dict with empty ones
    capture(net)
    gc, eb = net.gaussian_conditional, net.entropy_bottleneck
    net.load_state_dict(op.point_state_dict(point))
    net.update(force=True)
    for k, v in (("gc_cdf", gc._quantized_cdf), ("gc_len", gc._cdf_length), ("gc_off", gc._offset)):
        assert np.array_equal(v.numpy(), base_t[k]), (point, k)          # the scale table does not change
    ebt = (eb._quantized_cdf.numpy().copy(), eb._cdf_length.numpy().copy(), eb._offset.numpy().copy())
    if seed == 0:
        assert all(np.array_equal(a, base_t[k]) for a, k in zip(ebt, ("eb_cdf", "eb_len", "eb_off"))), point
    else:
        tables[f"eb_cdf_seed{seed}"], tables[f"eb_len_seed{seed}"], tables[f"eb_off_seed{seed}"] = ebt
    eb_lists = (ebt[0].tolist(), ebt[1].tolist(), ebt[2].tolist())
    for p, cname, q, pol in runs:
        if p != point:
            continue
        case = op.case_named(cname)
        _, B, H, W, iseed, kind, _ = case
        x, xp, unpad = op.case_input(case, point)
        cap.clear()
        with torch.no_grad():
            out = net.compress(xp, quality=q, mask_pol=pol)
            dec = net.decompress(out["strings"], out["shape"], q, mask_pol=pol)
        x_hat = F.pad(dec["x_hat"], unpad).clamp_(0, 1)                  # training/step.py:342-343
        ys, zs = out["strings"]
        zh, zw = out["shape"]
        C = ebt[0].shape[0]
        zidx = np.broadcast_to(np.arange(C).reshape(C, 1, 1), (C, zh, zw)).reshape(-1).tolist()
        z_sym = np.stack([np.asarray(ans.RansDecoder().decode_with_indexes(s, zidx, *eb_lists)).reshape(C, zh, zw) for s in zs])
        st = op.call_stats([s.numpy() for _, s in cap["cmp"]], [i.numpy() for i, _ in cap["cmp"]], [m.numpy() for m in out["masks"]],
                           z_sym, base_t["gc_len"], base_t["gc_off"], ebt[1], ebt[2])
        nbytes = sum(len(s) for sl in ys for s in sl) + sum(len(s) for s in zs)
        mse = torch.mean((x - x_hat) ** 2).item()
        per_image = dict(bytes_per_image=[sum(len(sl[b]) for sl in ys) + len(zs[b]) for b in range(B)],
                         psnr_per_image=[-10.0 * math.log10(torch.mean((x[b] - x_hat[b]) ** 2).item()) for b in range(B)])
        if cname == op.STRING_CASE[0]:
            extra = {}
            if op.has_dev(point, cname):
                o = op.oracle_run(point, cname, q, pol)
                assert o["out"]["strings"][0] == ys and o["out"]["strings"][1] == zs
                extra["oracle_dev"] = dict(psnr=abs(-10.0 * math.log10(torch.mean((x[0] - o["x_hat"][0]) ** 2).item()) - per_image["psnr_per_image"][0]),
                                           pixel=float((o["x_hat"] - x_hat).flatten()[::op.XHAT_SUB].abs().max()))
            strings.append(dict(**extra, point=point, case=cname, quality=q, seed=op.SEED_OVERRIDE.get((point, cname), iseed), shape=list(out["shape"]),
                                y_hex=[[s.hex() for s in sl] for sl in ys], z_hex=[s.hex() for s in zs],
                                psnr_per_image=per_image["psnr_per_image"], x_hat_sub=x_hat.flatten()[::op.XHAT_SUB].numpy().tolist()))
            print(point, cname, q, "strings stored", flush=True)
            continue
        rec = dict(point=point, case=cname, quality=q, mask_pol=pol, seed=op.SEED_OVERRIDE.get((point, cname), iseed), shape=list(out["shape"]),
                   y_sha=[[op.sha(s) for s in sl] for sl in ys], y_len=[[len(s) for s in sl] for sl in ys],
                   z_sha=[op.sha(s) for s in zs], z_len=[len(s) for s in zs],
                   mask_sums=[[int(m[b].sum().item()) for b in range(B)] for m in out["masks"]],
                   bpp=8.0 * nbytes / (B * H * W), psnr=-10.0 * math.log10(mse), **per_image, **st)
        if op.has_dev(point, cname):
            from oracle.codec_ref import bpp_of, psnr_of
            o = op.oracle_run(point, cname, q, pol)
            oys = o["out"]["strings"][0]
            rec["oracle_dev"] = dict(bpp=abs(bpp_of(o["out"]["strings"], B, H, W) - rec["bpp"]), psnr=abs(psnr_of(o["x"], o["x_hat"]) - rec["psnr"]),
                                     y_identical=sum(a == b for sa, sb in zip(oys, ys) for a, b in zip(sa, sb)), y_strings=sum(len(sl) for sl in ys))
        records.append(rec)
        print(point, cname, q, pol, "bpp %.4f psnr %.4f" % (rec["bpp"], rec["psnr"]), "y escapes %d / %d" % (st["y_escapes"], st["n_coded"]),
              "z escapes %d / %d" % (st["z_escapes"], st["n_z"]), flush=True)
np.savez_compressed(os.path.join(HERE, "operating_points_tables.npz"), **tables)
json.dump(dict(records=records), open(os.path.join(HERE, "operating_points.json"), "w"))
for c in strings:                                 # one file per point: each stays below the largest JSON fixture there is
    json.dump(c, open(os.path.join(HERE, f"operating_points_strings_{c['point']}.json"), "w"))
print("done")

#!/usr/bin/env python3
"""MS-SSIM on one GPU: progressivecodec_amd.metrics.ms_ssim (libpc_metrics.so) against the same definition composed from torch ops on
the GPU (grouped conv2d + avg_pool2d, float32), at three shapes:
  config2   32x3x256x256: bench.py's input (seed 1) against a perturbed copy
  config3   the 24 config3_images(), one call per orientation group (18 landscape 512x768, 6 portrait 768x512)
  frame4k   one 3x2160x3840 frame
Per shape: time per call (device events around `reps` calls after warm-up), the largest |difference| between the two, and the
algorithmic bytes / FLOPs of the kernels with the share of the larger of the HBM and VALU bounds.
usage: python tools/msssim_bench.py [reps] [--out FILE]      prints one JSON line"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from progressivecodec_amd import metrics
from progressivecodec_amd.harness import config3_images

HBM_BPS = 6.3e12          # measured copy rate (MI355X_MICROARCH: HBM3E, float4 copy)
VALU_FLOPS = 157.3e12     # FP32 vector peak (spec)
WEIGHTS = metrics.MS_WEIGHTS


def torch_ms_ssim(X, Y, data_range=1.0, win_size=11, sigma=1.5, K=(0.01, 0.03)):
    """the definition in torch ops, float32 on the GPU: the comparison point"""
    C = X.shape[1]
    c = torch.arange(win_size, dtype=torch.float32, device=X.device) - win_size // 2
    g = torch.exp(-(c ** 2) / (2 * sigma ** 2))
    g = g / g.sum()
    gh, gw = g.view(1, 1, -1, 1).repeat(C, 1, 1, 1), g.view(1, 1, 1, -1).repeat(C, 1, 1, 1)
    filt = lambda t: F.conv2d(F.conv2d(t, gh, groups=C), gw, groups=C)
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    w = torch.tensor(WEIGHTS, device=X.device)
    mcs = []
    for i in range(len(WEIGHTS)):
        mu1, mu2 = filt(X), filt(Y)
        s1, s2, s12 = filt(X * X) - mu1 * mu1, filt(Y * Y) - mu2 * mu2, filt(X * Y) - mu1 * mu2
        cs = ((2 * s12 + C2) / (s1 + s2 + C2)).flatten(2).mean(-1)
        ss = (((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * (2 * s12 + C2) / (s1 + s2 + C2)).flatten(2).mean(-1)
        if i < len(WEIGHTS) - 1:
            mcs.append(torch.relu(cs))
            pad = (X.shape[2] % 2, X.shape[3] % 2)
            X, Y = F.avg_pool2d(X, 2, 2, padding=pad), F.avg_pool2d(Y, 2, 2, padding=pad)
    m = torch.stack(mcs + [torch.relu(ss)])
    return torch.prod(m ** w.view(-1, 1, 1), dim=0).mean(1)


def work(shape, ws=11, levels=5):
    """algorithmic bytes and FLOPs of one call (the kernels' own schedule: X, Y read once per scale, pooled copies written once)"""
    B, C, H, W = shape
    byts = flops = 0
    for s in range(levels):
        n, no = B * C * H * W, B * C * (H - ws + 1) * (W - ws + 1)
        byts += 2 * 4 * n                                                    # X and Y read by the scale kernel
        flops += 3 * n + 2 * 5 * ws * B * C * (H - ws + 1) * W + 2 * 5 * ws * no + 20 * no   # products, H pass, W pass, maps + sums
        if s + 1 < levels:
            H, W = (H + 1) // 2, (W + 1) // 2
            byts += 2 * 4 * B * C * H * W                                    # pooled X and Y written (re-read by the next scale)
            flops += 2 * 4 * B * C * H * W
    return byts, flops


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps        # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reps", nargs="?", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 50:
        raise SystemExit("at least 50 timed calls per shape")
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the GPU only")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    x2 = torch.rand(32, 3, 256, 256, generator=g)
    y2 = (x2 + 0.05 * torch.randn(x2.shape, generator=torch.Generator().manual_seed(2))).clamp(0, 1)
    imgs = config3_images()
    land = torch.cat([x for x in imgs if x.shape[2] == 512]), torch.cat([x for x in imgs if x.shape[2] == 768])
    pert = lambda t, s: (t + 0.05 * torch.randn(t.shape, generator=torch.Generator().manual_seed(s))).clamp(0, 1)
    lo = torch.rand(1, 3, 270, 480, generator=torch.Generator().manual_seed(5))
    f4 = F.interpolate(lo, size=(2160, 3840), mode="bilinear", align_corners=False)
    shapes = {"config2": [(x2, y2)], "config3": [(land[0], pert(land[0], 3)), (land[1], pert(land[1], 4))], "frame4k": [(f4, pert(f4, 6))]}
    res = {"tool": "msssim_bench", "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    for name, pairs in shapes.items():
        pairs = [(x.to(dev), y.to(dev)) for x, y in pairs]
        ours = lambda: [metrics.ms_ssim(x, y, data_range=1.0, size_average=False) for x, y in pairs]
        ref = lambda: [torch_ms_ssim(x, y) for x, y in pairs]
        diff = max((o - r).abs().max().item() for o, r in zip(ours(), ref()))
        t_ours, t_ref = timed(ours, a.reps), timed(ref, a.reps)
        byts = flops = 0
        for x, _ in pairs:
            b, f = work(tuple(x.shape))
            byts, flops = byts + b, flops + f
        t_hbm, t_valu = byts / HBM_BPS * 1e6, flops / VALU_FLOPS * 1e6
        res[name] = {"shapes": [list(x.shape) for x, _ in pairs], "us_per_call": round(t_ours, 2), "torch_ops_us_per_call": round(t_ref, 2),
                     "speedup_vs_torch_ops": round(t_ref / t_ours, 2), "max_abs_diff_vs_torch_ops": diff,
                     "algorithmic_MB": round(byts / 1e6, 2), "algorithmic_GFLOP": round(flops / 1e9, 3),
                     "bound_us": round(max(t_hbm, t_valu), 2), "bound": "HBM" if t_hbm >= t_valu else "VALU",
                     "fraction_of_bound": round(max(t_hbm, t_valu) / t_ours, 3)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

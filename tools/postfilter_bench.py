#!/usr/bin/env python3
"""UNet post-filter timing (ChannelProgresssiveWACNN(u_net_post=1); layers/unet.py) on an MI355X: Config 2 (B = 32, 256 x 256) and one
3840 x 2160 frame.  Prints one JSON object:

  * pass_ms: HIP-event time of one model.post_filter() call (median of --reps), TFLOP/s over the algorithmic FLOPs and the share of the
    157.3 TFLOP/s f32 MFMA peak;
  * layers: every conv launch of one pass bracketed by HIP events (pc_codec_profile_begin / _intervals), in launch order with its name,
    shape, time, TFLOP/s and share of peak; the SE squeeze and max-pool launches are the pass time minus the conv sum ("non_conv_ms");
  * decompress_added_ms (Config 2 only): decompress() of the same strings at q = 0.5 by a u_net_post=1 object minus a u_net_post=0 one.

Run:  python3 tools/postfilter_bench.py [--reps N] > profiles/<tag>_postfilter.json   (under `rocprofv3 --kernel-trace --stats -- python3 ...`
for the per-kernel table of the profiler)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK = 157.3  # TFLOP/s, dense f32 MFMA


def layer_table():
    """(name, Cin, Cout, k, resolution divisor, pixel shuffle) of the conv launches of one pass, in launch order (pc_codec.hip: unet)"""
    t = []
    def cbr(n, ci, co, r):
        t.extend([(n + ".conv.0", ci, co, 3, r, False), (n + ".conv.2", co, co, 3, r, False), (n + ".up_dim", ci, co, 1, r, False)])
    cbr("conv1", 3, 32, 1)
    cbr("conv2", 32, 64, 2)
    cbr("conv3", 64, 128, 4)
    for i in range(4):
        t.extend([(f"context_refine.{i}.conv1", 128, 128, 3, 4, False), (f"context_refine.{i}.conv2", 128, 128, 3, 4, False)])
    t.append(("up3", 128, 256, 1, 4, True))
    cbr("up_conv3", 128, 64, 2)
    t.append(("up2", 64, 128, 1, 2, True))
    cbr("up_conv2", 64, 16, 1)
    t.append(("out conv3x3(16,3)", 16, 3, 3, 1, False))
    return t


def make(mode):
    from progressivecodec_amd import ChannelProgresssiveWACNN
    from progressivecodec_amd.arch import CodecConfig
    from progressivecodec_amd.synth import synthetic_state_dict
    net = ChannelProgresssiveWACNN(device="cuda:0", u_net_post=mode)
    net.load_state_dict(synthetic_state_dict(CodecConfig(u_net_post=mode)))
    net.update()
    return net


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), [round(t, 3) for t in ts]


def per_layer(net, x):
    from progressivecodec_amd._lib import check, lib
    L = lib()
    check(L.pc_profile_set_epoch(0), "pc_profile_set_epoch")
    check(L.pc_codec_profile_begin(net._h), "pc_codec_profile_begin")
    net.post_filter(x)
    torch.cuda.synchronize()
    nl, ms, fl = C.c_int64(), C.c_double(), C.c_double()
    check(L.pc_codec_profile_end(net._h, C.byref(nl), C.byref(ms), C.byref(fl)), "pc_codec_profile_end")
    n = C.c_size_t()
    check(L.pc_codec_profile_intervals(net._h, None, None, None, 0, C.byref(n)), "pc_codec_profile_intervals")
    t0, t1, f = (np.zeros(max(1, n.value)) for _ in range(3))
    check(L.pc_codec_profile_intervals(net._h, t0.ctypes.data_as(C.c_void_p), t1.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p),
                                       n.value, C.byref(n)), "pc_codec_profile_intervals")
    tab = layer_table()
    assert n.value == len(tab), (n.value, len(tab))
    rows = []
    for (name, ci, co, k, r, ps), a, b, fl_ in zip(tab, t0, t1, f):
        d = float(b - a)
        rows.append(dict(layer=name, cin=ci, cout=co, k=k, resolution=f"1/{r}" if r > 1 else "full", pixel_shuffle=ps, ms=round(d, 4),
                         gflop=round(fl_ / 1e9, 3), tflops=round(fl_ / d / 1e9, 2), frac_peak=round(fl_ / d / 1e9 / PEAK, 3)))
    return rows, float(fl.value), float(ms.value)


def run_shape(net, B, H, W, reps):
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(1)).cuda()
    for _ in range(2):
        net.post_filter(x)
    torch.cuda.synchronize()
    med, all_ms = timed(lambda: net.post_filter(x), reps)
    rows, flops, conv_ms = per_layer(net, x)
    med2, _ = timed(lambda: net.post_filter(x), reps)         # (after the bracketed pass: same figure expected)
    tfl = flops / med / 1e9
    return dict(B=B, H=H, W=W, pass_ms=round(med, 3), pass_ms_all=all_ms, pass_ms_again=round(med2, 3), gflop=round(flops / 1e9, 2),
                tflops=round(tfl, 2), frac_peak=round(tfl / PEAK, 3), conv_ms_sum_bracketed=round(conv_ms, 3),
                non_conv_ms=round(med - conv_ms, 3), layers=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    net1 = make(1)
    out = {"tool": "tools/postfilter_bench.py", "device": torch.cuda.get_device_name(0), "peak_tflops_f32_mfma": PEAK}
    from bench import source_hash
    out["source_hash"] = source_hash()
    out["config2"] = run_shape(net1, 32, 256, 256, a.reps)
    out["frame_4k"] = run_shape(net1, 1, 2160, 3840, max(3, a.reps // 2))
    # time added to decompress(): same strings, a u_net_post=0 object against a u_net_post=1 one (identical base weights)
    net0 = make(0)
    x = torch.rand(32, 3, 256, 256, generator=torch.Generator().manual_seed(2)).cuda()
    o = net0.compress(x, quality=0.5, mask_pol="point-based-std")
    res = {}
    for tag, net in (("u_net_post_0", net0), ("u_net_post_1", net1)):
        for _ in range(2):
            net.decompress(o["strings"], o["shape"], 0.5, "point-based-std")
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t = time.perf_counter()
            net.decompress(o["strings"], o["shape"], 0.5, "point-based-std")
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) * 1e3)
        res[tag] = round(float(np.median(ts)), 2)
    out["decompress_config2_q0.5_ms"] = res
    out["decompress_added_ms"] = round(res["u_net_post_1"] - res["u_net_post_0"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

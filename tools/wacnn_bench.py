#!/usr/bin/env python3
"""WACNN (the single-rate model) at the Config-2 shape: encode, decode and encode+decode MP/s (median of --runs after --warmup), each split
into host entropy-coding time (pc_codec_host_stats) and the rest (GPU chain, transfers, launch overhead); the conv family's algorithmic
FLOP/px and TFLOP/s (pc_codec_profile_*, serial schedule) beside the progressive model's at quality 0 in the same process.

    python tools/wacnn_bench.py [--batch 32] [--size 256] [--runs 5] [--warmup 2] [--out profiles/<name>.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from progressivecodec_amd import ChannelProgresssiveWACNN, WACNN  # noqa: E402
from progressivecodec_amd._lib import check, lib  # noqa: E402
from progressivecodec_amd.synth import synthetic_state_dict, synthetic_wacnn_state_dict  # noqa: E402


def host_stats(net):
    v = (C.c_double * 6)()
    check(lib().pc_codec_host_stats(net._h, v, 6), "pc_codec_host_stats")
    return list(v)


def conv_profile(net, fn):
    """run fn() once with the conv launches bracketed (serial schedule): launches, ms, algorithmic FLOPs"""
    n, ms, fl = C.c_int64(), C.c_double(), C.c_double()
    check(lib().pc_codec_profile_begin(net._h), "profile_begin")
    fn()
    torch.cuda.synchronize()
    check(lib().pc_codec_profile_end(net._h, C.byref(n), C.byref(ms), C.byref(fl)), "profile_end")
    return {"launches": n.value, "conv_ms": ms.value, "gflop": fl.value / 1e9, "tflops": fl.value / (ms.value * 1e-3) / 1e12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, S = a.batch, a.size
    px = B * S * S
    x = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(1)).cuda()     # Config 2's input
    net = WACNN(device="cuda:0")
    net.load_state_dict(synthetic_wacnn_state_dict())
    net.update()
    net.eval()
    enc, dec, enc_host, dec_host = [], [], [], []
    for r in range(a.warmup + a.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        o = net.compress(x)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        he = host_stats(net)[1]
        d = net.decompress(o["strings"], o["shape"])
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        hd = host_stats(net)[3]
        if r >= a.warmup:
            enc.append((t1 - t0) * 1e3); dec.append((t2 - t1) * 1e3); enc_host.append(he); dec_host.append(hd)
    st = host_stats(net)
    med = statistics.median
    te, td = med(enc), med(dec)
    res = {
        "shape": [B, 3, S, S], "runs": a.runs, "warmup": a.warmup,
        "encode_ms": te, "decode_ms": td, "encode_mp_s": px / te / 1e3, "decode_mp_s": px / td / 1e3, "enc_dec_mp_s": px / (te + td) / 1e3,
        "encode_host_rans_ms": med(enc_host), "encode_rest_ms": te - med(enc_host),
        "decode_host_rans_ms": med(dec_host), "decode_rest_ms": td - med(dec_host),
        "y_symbols_per_batch": int(st[4] - B * 192 * (S // 64) ** 2),
        "host_encode_msym_s": st[4] / med(enc_host) / 1e3, "host_decode_msym_s": st[5] / med(dec_host) / 1e3,
        "y_string_bytes": len(o["strings"][0][0]), "bpp": 8.0 * (len(o["strings"][0][0]) + sum(map(len, o["strings"][1]))) / px,
        "runs_encode_ms": enc, "runs_decode_ms": dec,
    }
    net.set_option("serial_schedule", 1)
    pw_e = conv_profile(net, lambda: net.compress(x))
    pw_d = conv_profile(net, lambda: net.decompress(o["strings"], o["shape"]))
    chan = ChannelProgresssiveWACNN(device="cuda:0")
    chan.load_state_dict(synthetic_state_dict())
    chan.update()
    chan.set_option("serial_schedule", 1)
    oc = chan.compress(x, quality=0.0, mask_pol="point-based-std")
    pc_e = conv_profile(chan, lambda: chan.compress(x, quality=0.0, mask_pol="point-based-std"))
    pc_d = conv_profile(chan, lambda: chan.decompress(oc["strings"], oc["shape"], 0.0, mask_pol="point-based-std"))
    res["conv_profile"] = {"wacnn_encode": pw_e, "wacnn_decode": pw_d, "channel_q0_encode": pc_e, "channel_q0_decode": pc_d}
    res["conv_flop_per_px"] = {"wacnn_encode": pw_e["gflop"] * 1e9 / px, "wacnn_decode": pw_d["gflop"] * 1e9 / px,
                               "channel_q0_encode": pc_e["gflop"] * 1e9 / px, "channel_q0_decode": pc_d["gflop"] * 1e9 / px}
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

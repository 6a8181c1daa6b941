"""Tiled image coding against what it replaces, on one 3x2160x3840 frame with T = 512: HIP events, warm,
median of 20 for the kernels; a host clock around a synchronise, median of 3, for the codec calls.

  cut             tiles.cut(u8)                       vs  F.pad to the grid, float().div(255), unfold / permute / contiguous into [n,3,T,T]
  stitch          tiles.stitch(x_hat_tiles, grid)     vs  clamp, per-band weights, fold by index arithmetic (zeros + one weighted add per
                  (+ ref: the distortion sums)            tile), mul(255), round, byte (+ the squared-error mean against the original)
  copy            a plain device copy (dst.copy_(src)) of the bytes each call moves: the rate this tool measures for the same traffic
  whole frame     pixels.encode_image + decode_image  vs  tiles.encode_tiled + decode_tiled
  region          tiles.decode_tiled(region = 512x512) vs the whole-frame pixels.decode_image: time, and the drop in free device memory
                  (torch.cuda.mem_get_info around the call in a fresh process each: the codec library's own allocations are invisible
                  to torch's allocator)

The torch sequences are written out below so that the comparison can be repeated.  Bytes moved: 8-bit in + float out for the cut;
float in (every tile where it covers the image, so the bands twice) + 8-bit out for the stitch.  The weights are synth.synthetic_state_dict's:
times and memory are meaningful with them, rate and distortion are not.  Prints one JSON line per measurement; --out FILE also
writes them all.

    python tools/tiles_bench.py --out profiles/tiles_io_times_mi355x.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
H, W, T = 2160, 3840, 512
QUALITIES = [0, 0.5, 10]
REGION = (824, 1664, 512, 512)                     # the frame's centre: it straddles tile edges, as a viewer's window would


def timed(fn, n=20, warm=5):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return round(statistics.median(ts), 2)


def walled(fn, n=3, warm=1):
    """seconds, median of n, a host clock around work that ends in a synchronise"""
    import torch
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return round(statistics.median(ts), 4)


def torch_cut(u8_chw, g):
    """the sequence tiles.cut replaces: pad to the grid, to float, divide, unfold into tiles"""
    import torch.nn.functional as F
    S = g.S
    Hg, Wg = (g.ny - 1) * S + g.T, (g.nx - 1) * S + g.T
    x = F.pad(u8_chw.float().div(255), (0, Wg - g.W, 0, Hg - g.H))
    t = x.unfold(1, g.T, S).unfold(2, g.T, S)                              # [3, ny, nx, T, T]
    return t.permute(1, 2, 0, 3, 4).reshape(g.n, 3, g.T, g.T).contiguous()


def torch_weights(g, device):
    """per-axis band weights [n_axis, T] as the definition gives them"""
    import torch

    def axis(n):
        w = torch.ones(n, g.T, dtype=torch.float32)
        if g.O:
            up = (2 * torch.arange(g.O, dtype=torch.float32) + 1) / (2 * g.O)
            w[1:, :g.O] = up
            w[:-1, g.S:] = up.flip(0)
        return w.to(device)
    return axis(g.ny), axis(g.nx)


def torch_stitch(x_tiles, g, wy, wx, ref_f=None):
    """the sequence tiles.stitch replaces: clamp, weigh, add every tile where it lies, crop, scale, round, byte (+ the mean squared
    error against the original as float planes, what harness.compute_psnr takes)"""
    import torch
    S = g.S
    Hg, Wg = (g.ny - 1) * S + g.T, (g.nx - 1) * S + g.T
    c = x_tiles.clamp(0, 1).view(g.ny, g.nx, 3, g.T, g.T)
    c = c * (wy[:, None, None, :, None] * wx[None, :, None, None, :])
    acc = torch.zeros((3, Hg, Wg), dtype=torch.float32, device=x_tiles.device)
    for i in range(g.ny):
        for j in range(g.nx):
            acc[:, i * S:i * S + g.T, j * S:j * S + g.T] += c[i, j]
    m = acc[:, :g.H, :g.W]
    out = m.mul(255).round().byte()
    if ref_f is None:
        return out
    return out, torch.mean((ref_f - m) ** 2, dim=(1, 2))


def model():
    from progressivecodec_amd import ChannelProgresssiveWACNN
    from progressivecodec_amd.synth import synthetic_state_dict
    net = ChannelProgresssiveWACNN(device="cuda:0")
    net.load_state_dict(synthetic_state_dict())
    net.update()
    return net


def frame():
    import torch
    g = torch.Generator().manual_seed(0)
    lo = torch.rand(1, 3, H // 8, W // 8, generator=g)
    x = torch.nn.functional.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False).clamp(0, 1)
    return x[0].mul(255).round().byte().permute(1, 2, 0).contiguous().cuda()                 # [H,W,3]


def child(mode, path):
    """one decode in a fresh process: its time and the drop in free device memory around it"""
    import torch
    from progressivecodec_amd import pixels, tiles
    net = model()
    buf = open(path, "rb").read()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    t0 = time.perf_counter()
    if mode == "whole":
        out = pixels.decode_image(net, buf)
    elif mode == "tiled":
        out = tiles.decode_tiled(net, buf)
    else:
        out = tiles.decode_tiled(net, buf, region=REGION)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    free1 = torch.cuda.mem_get_info(0)[0]
    print(json.dumps({"mode": mode, "first_call_seconds": round(dt, 4), "free_memory_drop_mib": round((free0 - free1) / 2 ** 20, 1),
                      "shape": list(out.shape)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--child")
    ap.add_argument("--file")
    ap.add_argument("--skip-codec", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.file)
    import torch
    from progressivecodec_amd import pixels, tiles
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)
    img = frame()
    chw = img.permute(2, 0, 1).contiguous()
    ref_f = chw.float().div(255)
    for O in (0, 32):
        g = tiles.grid_of(H, W, T, O)
        x, _ = tiles.cut(img, T, O)
        x_hat = (x + 0.02 * torch.randn_like(x)).contiguous()
        wy, wx = torch_weights(g, "cuda")
        cut_bytes = 3 * H * W + 4 * x.numel()
        st_bytes = 12 * (H + (g.ny - 1) * O) * (W + (g.nx - 1) * O) + 3 * H * W    # the tiles where they cover the image (bands twice)
        a = torch.empty(cut_bytes // 2, dtype=torch.uint8, device="cuda")
        b = torch.empty_like(a)
        a2 = torch.empty(st_bytes // 2, dtype=torch.uint8, device="cuda")
        b2 = torch.empty_like(a2)
        r = {"what": "kernels", "frame": [3, H, W], "tile": T, "overlap": O, "tiles": [g.ny, g.nx],
             "unit": "us, median of 20 (HIP events, warm)",
             "cut_hwc": timed(lambda: tiles.cut(img, T, O)),
             "cut_chw": timed(lambda: tiles.cut(chw, T, O, "chw")),
             "torch_cut": timed(lambda: torch_cut(chw, g)),
             "copy_of_cut_bytes": timed(lambda: b.copy_(a)),
             "stitch_hwc": timed(lambda: tiles.stitch(x_hat, g)),
             "stitch_chw": timed(lambda: tiles.stitch(x_hat, g, layout="chw")),
             "torch_stitch": timed(lambda: torch_stitch(x_hat, g, wy, wx)),
             "stitch_with_sums_chw": timed(lambda: tiles.stitch(x_hat, g, layout="chw", ref=chw)),
             "torch_stitch_with_mse": timed(lambda: torch_stitch(x_hat, g, wy, wx, ref_f)),
             "copy_of_stitch_bytes": timed(lambda: b2.copy_(a2)),
             "cut_bytes": cut_bytes, "stitch_bytes": st_bytes}
        r["cut_tb_per_s"] = round(cut_bytes / r["cut_hwc"] / 1e6, 3)
        r["stitch_tb_per_s"] = round(st_bytes / r["stitch_hwc"] / 1e6, 3)
        r["copy_tb_per_s"] = round(cut_bytes / r["copy_of_cut_bytes"] / 1e6, 3)
        r["cut_fraction_of_hbm_peak"] = round(cut_bytes / (r["cut_hwc"] * 1e-6) / HBM_PEAK, 4)
        r["stitch_fraction_of_hbm_peak"] = round(st_bytes / (r["stitch_hwc"] * 1e-6) / HBM_PEAK, 4)
        got = tiles.stitch(x_hat, g, layout="chw")
        want = torch_stitch(x_hat, g, wy, wx)
        r["stitch_bytes_that_differ_from_torch"] = int((got != want).sum())    # torch multiplies and adds unfused: last-bit ties only
        r["cut_equals_torch"] = bool(torch.equal(tiles.cut(chw, T, O, "chw")[0], torch_cut(chw.cpu(), g).cuda()))
        emit(r)
        del a, b, a2, b2
    if not args.skip_codec:
        net = model()
        with tempfile.TemporaryDirectory() as tmp:
            r = {"what": "codec, whole frame against tiles", "frame": [3, H, W], "tile": T, "qualities": QUALITIES,
                 "unit": "s, median of 3 (host clock around a synchronise, warm)", "weights": "synthetic: times only"}
            bufs = {}
            for name, enc, dec in [("whole", lambda: pixels.encode_image(net, img, QUALITIES), lambda b: pixels.decode_image(net, b)),
                                   ("tiled_o0", lambda: tiles.encode_tiled(net, img, QUALITIES, T, 0), lambda b: tiles.decode_tiled(net, b)),
                                   ("tiled_o32", lambda: tiles.encode_tiled(net, img, QUALITIES, T, 32), lambda b: tiles.decode_tiled(net, b))]:
                try:
                    bufs[name] = enc()
                    r[name + "_encode"] = walled(enc)
                    r[name + "_decode"] = walled(lambda: dec(bufs[name]))
                    r[name + "_bytes"] = len(bufs[name])
                    with open(os.path.join(tmp, name), "wb") as f:
                        f.write(bufs[name])
                except Exception as e:                                         # a finding, recorded as such
                    r[name + "_error"] = f"{type(e).__name__}: {e}"[:300]
            if "tiled_o32" in bufs:
                r["tiled_o32_decode_region_512"] = walled(lambda: tiles.decode_tiled(net, bufs["tiled_o32"], region=REGION))
                r["region"] = list(REGION)
            emit(r)
            del net
            torch.cuda.empty_cache()
            for mode, name in [("whole", "whole"), ("tiled", "tiled_o32"), ("region", "tiled_o32")]:
                if name not in bufs:
                    continue
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--file", os.path.join(tmp, name)],
                                   capture_output=True, text=True, timeout=600)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
                c = json.loads(line[-1]) if p.returncode == 0 and line else {"mode": mode, "error": (p.stderr or p.stdout)[-300:]}
                c["what"] = "fresh process: one decode, " + ("the whole frame" if mode != "region" else "region 512x512") + \
                            (" from one PCB1" if mode == "whole" else " from PCT1, overlap 32")
                emit(c)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

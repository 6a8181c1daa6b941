"""The image-domain layer against the torch sequences it replaces in harness.compress_with_ac: HIP events, warm,
median of 20, at Config 2's batch (32x3x256x256) and one 3x2160x3840 frame.

  ingest          pixels.to_model_input(u8)                      vs  F.pad(u8.float().div(255), pad)
  emit with sums  pixels.from_model_output(x_hat, geom, ref=u8)  vs  F.pad(x_hat, unpad).clamp_(0, 1); torch.mean((x - x_hat)**2) per image
                  + the read-back of the sums                        + the read-back (.item() / .tolist())

The torch side is the code of the default harness path, not of the new one.  Bandwidth = bytes that must move (u8 in + float out for
the ingest; float in + ref in + u8 out for the emit) / time, against the 8 TB/s HBM peak.  Prints one JSON line per shape;
--out FILE also writes the list.

    python tools/pixels_bench.py --out profiles/pixels_io_times_mi355x.json
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12


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


def main():
    import torch
    import torch.nn.functional as F
    from progressivecodec_amd import pixels
    from progressivecodec_amd.harness import compute_padding
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    rows = []
    for B, H, W in [(32, 256, 256), (1, 2160, 3840)]:
        u8 = torch.randint(0, 256, (B, 3, H, W), dtype=torch.uint8, device="cuda")
        hwc = u8.permute(0, 2, 3, 1).contiguous()
        pad, unpad = compute_padding(H, W, 64)
        geom = pixels.padding(H, W)
        x = u8.cpu().float().div(255).cuda()
        xp = F.pad(x, pad)
        x_hat = (xp + 0.02 * torch.randn_like(xp)).contiguous()

        def torch_emit(read=True):
            xh = F.pad(x_hat, unpad).clamp_(0, 1)
            m = torch.mean((x - xh) ** 2, dim=(1, 2, 3))
            return m.tolist() if read else m

        def new_emit(read=True, layout="chw", ref=u8, image=True):
            r = pixels.from_model_output(x_hat, geom, layout, ref=ref, image=image)
            d = r[1] if image else r
            return d.psnr() if read else d
        ib = B * 3 * H * W + 4 * B * 3 * geom.Hp * geom.Wp
        eb = (4 + 1 + 1) * B * 3 * H * W
        r = {"shape": [B, 3, H, W], "padded": [geom.Hp, geom.Wp], "unit": "us, median of 20 (HIP events, warm)",
             "ingest": timed(lambda: pixels.to_model_input(u8, "chw")),
             "ingest_hwc": timed(lambda: pixels.to_model_input(hwc, "hwc")),
             "torch_ingest": timed(lambda: F.pad(u8.float().div(255), pad, mode="constant", value=0)),
             "emit_with_sums_and_readback": timed(new_emit),
             "torch_emit_with_readback": timed(torch_emit),
             "emit_with_sums_device_only": timed(lambda: new_emit(False)),
             "emit_with_sums_device_only_hwc": timed(lambda: new_emit(False, "hwc", hwc)),
             "sums_only_device_only": timed(lambda: new_emit(False, image=False)),
             "torch_emit_device_only": timed(lambda: torch_emit(False)),
             "ingest_bytes": ib, "emit_bytes": eb}
        r["ingest_fraction_of_hbm_peak"] = round(ib / (r["ingest"] * 1e-6) / HBM_PEAK, 4)
        r["emit_fraction_of_hbm_peak"] = round(eb / (r["emit_with_sums_device_only"] * 1e-6) / HBM_PEAK, 4)
        r["psnr_max_abs_difference_db"] = max(abs(a - (-10 * math.log10(m))) for a, m in zip(new_emit(), torch_emit()))
        print(json.dumps(r), flush=True)
        rows.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

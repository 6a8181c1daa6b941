"""The YUV 4:2:0 layer against the torch sequences it replaces: HIP events, warm, median of 20, one 1080p and
one 2160p NV12 frame and one 2160p P010 frame, bt709, limited range.

  ingest          frames.to_model_input(planes, fmt)                  vs  the torch sequence below: offsets, scales, bilinear chroma
                                                                          (F.interpolate), the 3x3 matrix, clamp, F.pad
  emit            frames.from_model_output(x_hat, geom, fmt)          vs  un-pad, clamp, matrix, 2x2 mean (avg_pool2d), round, clamp,
                                                                          cast, re-interleave
  emit with sums  ... (x_hat, geom, fmt, ref=planes), device only     vs  the same plus the three squared-error means
  copy            dst.copy_(src) of a byte buffer with the same traffic (bytes read + bytes written = the bytes the call must move)

The torch sequences are what a user would write, not a restatement: they multiply by reciprocals, interpolate in float and so do
not give the same bits (the largest code difference is reported).  Bandwidth = bytes that must move (planes in + floats out for the
ingest; floats in + planes out, + the reference planes in with sums) / time, against the 8 TB/s HBM peak and the copy at the same
traffic.  Prints one JSON line per shape; --out FILE also writes the list.

    python tools/frames_bench.py --out profiles/frames_times_mi355x.json
"""
import argparse
import json
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


def codes_of(t, fmt):
    """plane -> float codes (P010: the word shifted down)"""
    import torch
    return t.to(torch.int32).bitwise_right_shift(6).float() if fmt == "p010" else t.float()


def words_of(t, fmt):
    import torch
    return t.to(torch.int32).bitwise_left_shift(6).to(torch.uint16) if fmt == "p010" else t.to(torch.uint8)


def main():
    import torch
    import torch.nn.functional as F
    from progressivecodec_amd import frames
    from progressivecodec_amd.harness import compute_padding
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    k = frames.coefficients("bt709")
    rows = []
    for fmt, H, W in [("nv12", 1080, 1920), ("nv12", 2160, 3840), ("p010", 2160, 3840)]:
        yo, ys, co, cs, top_code = frames.levels(fmt, "limited")
        es = 2 if fmt == "p010" else 1
        g = torch.Generator(device="cuda").manual_seed(H)
        # a smooth in-gamut picture: low-resolution noise enlarged, emitted once by the layer itself
        lo = torch.rand((1, 3, H // 40, W // 40), generator=g, device="cuda") * 0.8 + 0.1
        geom = frames.padding(H, W)
        pad, unpad = compute_padding(H, W, 64)
        rgb = F.pad(F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False), pad)
        planes = frames.from_model_output(rgb, geom, fmt)
        Y, UV = planes
        x_hat = (rgb + 0.02 * torch.randn(rgb.shape, generator=g, device="cuda")).contiguous()

        def torch_ingest():
            y = (codes_of(Y[0], fmt) - yo) / ys
            c = (codes_of(UV[0], fmt) - co) / cs
            c = F.interpolate(c.permute(2, 0, 1)[None], scale_factor=2, mode="bilinear", align_corners=False)[0]
            out = torch.stack((y + k.a * c[1], y - k.b * c[0] - k.c * c[1], y + k.d * c[0]))[None].clamp_(0, 1)
            return F.pad(out, pad)

        def torch_emit(sums=False):
            c = F.pad(x_hat, unpad).clamp_(0, 1)[0]
            yf = k.kr * c[0] + k.kg * c[1] + k.kb * c[2]
            yc = (yf * ys + yo).round_().clamp_(0, top_code)
            ch = torch.stack(((c[2] - yf) * k.ib, (c[0] - yf) * k.ir)) * cs
            cc = (F.avg_pool2d(ch[None], 2)[0] + co).round_().clamp_(0, top_code)
            out = (words_of(yc, fmt)[None], words_of(cc.permute(1, 2, 0), fmt).contiguous()[None])
            if not sums:
                return out
            return out, torch.stack((((yc - codes_of(Y[0], fmt)) ** 2).mean(), ((cc[0] - codes_of(UV[0, :, :, 0], fmt)) ** 2).mean(),
                                     ((cc[1] - codes_of(UV[0, :, :, 1], fmt)) ** 2).mean()))

        plane_bytes = es * (H * W + 2 * (H // 2) * (W // 2))
        fbytes = 4 * 3 * geom.Hp * geom.Wp
        wbytes = 4 * 3 * H * W
        ib, eb, sb = plane_bytes + fbytes, wbytes + plane_bytes, wbytes + 2 * plane_bytes

        def copy_of(total):
            src = torch.empty(total // 2, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            return timed(lambda: dst.copy_(src))

        x_new, _ = frames.to_model_input(planes, fmt)
        r = {"fmt": fmt, "shape": [H, W], "padded": [geom.Hp, geom.Wp], "matrix": "bt709", "range": "limited",
             "unit": "us, median of 20 (HIP events, warm)",
             "wide_ingest": frames.plan(frames.INGEST, planes, fmt, x_new, geom), "wide_emit": frames.plan(frames.EMIT, planes, fmt, x_hat, geom, ref=planes),
             "ingest": timed(lambda: frames.to_model_input(planes, fmt)),
             "ingest_nearest": timed(lambda: frames.to_model_input(planes, fmt, upsample="nearest")),
             "torch_ingest": timed(torch_ingest),
             "copy_ingest_traffic": copy_of(ib),
             "emit": timed(lambda: frames.from_model_output(x_hat, geom, fmt)),
             "torch_emit": timed(torch_emit),
             "copy_emit_traffic": copy_of(eb),
             "emit_with_sums_device_only": timed(lambda: frames.from_model_output(x_hat, geom, fmt, ref=planes)),
             "sums_only_device_only": timed(lambda: frames.from_model_output(x_hat, geom, fmt, ref=planes, image=False)),
             "torch_emit_with_sums_device_only": timed(lambda: torch_emit(True)),
             "copy_emit_with_sums_traffic": copy_of(sb),
             "ingest_bytes": ib, "emit_bytes": eb, "emit_with_sums_bytes": sb}
        r["ingest_fraction_of_hbm_peak"] = round(ib / (r["ingest"] * 1e-6) / HBM_PEAK, 4)
        r["emit_fraction_of_hbm_peak"] = round(eb / (r["emit"] * 1e-6) / HBM_PEAK, 4)
        r["emit_with_sums_fraction_of_hbm_peak"] = round(sb / (r["emit_with_sums_device_only"] * 1e-6) / HBM_PEAK, 4)
        r["ingest_max_abs_difference_from_torch"] = float((x_new - torch_ingest()).abs().max())
        new, old = frames.from_model_output(x_hat, geom, fmt), torch_emit()
        r["emit_max_code_difference_from_torch"] = max(int((codes_of(a, fmt) - codes_of(b, fmt)).abs().max()) for a, b in zip(new, old))
        print(json.dumps(r), flush=True)
        rows.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

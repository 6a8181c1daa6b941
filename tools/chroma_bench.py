"""The chroma layer against the torch sequences it replaces and against `frames`: HIP events, warm, one
2160 x 3840 frame, bt709, limited range, for nv12 centre, nv12 left, nv12 topleft, p210 left and i444.

  ingest          chroma.to_model_input(planes, fmt, siting=...)       vs  the torch sequence below: offsets, scales, the chroma
                                                                          planes enlarged per subsampled axis (F.interpolate for
                                                                          centre, the plane interleaved with the mean of itself and
                                                                          its shifted copy for co-sited), the 3x3 matrix, clamp, F.pad
  emit            chroma.from_model_output(x_hat, geom, fmt, siting=.) vs  un-pad, clamp, matrix, the chroma filter (avg_pool2d for
                                                                          centre, a [1, 2, 1] conv1d per co-sited axis with
                                                                          replicated edges), round, clamp, cast, re-interleave
  emit with sums  ... (ref=planes), device only                        vs  the same plus the three squared-error means
  copy            dst.copy_(src) of a byte buffer with the same traffic (bytes read + bytes written = the bytes the call must move)
  frames          for nv12 centre: frames.to_model_input / from_model_output of the same frame, the same work by the 4:2:0 kernels

Every pair (new against torch, new against frames) alternates: each side is the median of 20, taken five times; the figure is the
median of the five, the spread their max - min.  The copy is a median of 20.  The torch sequences are what a user would write, not
a restatement: they multiply by reciprocals and filter in float and so do not give the same bits (the largest code difference is
reported); against `frames` the outputs are compared for equality.  No speed is gated.  Prints one JSON line per case; --out FILE
also writes the list.

    python tools/chroma_bench.py --out profiles/chroma_times_mi355x.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
CASES = [("nv12", "centre"), ("nv12", "left"), ("nv12", "topleft"), ("p210", "left"), ("i444", "centre")]


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


def alternating(*fns):
    """the calls alternating, five medians of 20 each -> per call {median, spread (max - min), the five}"""
    runs = [[] for _ in fns]
    for _ in range(5):
        for ts, fn in zip(runs, fns):
            ts.append(timed(fn))
    return [{"median": statistics.median(ts), "spread": round(max(ts) - min(ts), 2), "five": ts} for ts in runs]


def main():
    import torch
    import torch.nn.functional as F
    from progressivecodec_amd import chroma, frames
    from progressivecodec_amd.harness import compute_padding
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--size", type=int, nargs=2, default=[2160, 3840])
    args = ap.parse_args()
    k = frames.coefficients("bt709")
    H, W = args.size
    rows = []
    for fmt, siting in CASES:
        f = chroma.FORMATS[fmt]
        semi = f.layout == chroma.SEMIPLANAR
        hco, vco = (f.sx == 2 and chroma.SITINGS[siting][0] == chroma.COSITED), (f.sy == 2 and chroma.SITINGS[siting][1] == chroma.COSITED)
        yo, ys, co, cs, top_code = frames.levels("p010" if f.bits == 10 else "nv12", "limited")
        es = 2 if f.bits == 10 else 1
        Hc, Wc = chroma.chroma_size(H, W, fmt)
        g = torch.Generator(device="cuda").manual_seed(H)
        lo = torch.rand((1, 3, H // 40, W // 40), generator=g, device="cuda") * 0.8 + 0.1
        geom = chroma.padding(H, W)
        pad, unpad = compute_padding(H, W, 64)
        rgb = F.pad(F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False), pad)
        planes = chroma.from_model_output(rgb, geom, fmt, siting=siting)
        x_hat = (rgb + 0.02 * torch.randn(rgb.shape, generator=g, device="cuda")).contiguous()

        def codes_of(t):
            return t.to(torch.int32).bitwise_right_shift(f.shift).float() if f.bits == 10 else t.float()

        def words_of(t):
            return t.to(torch.int32).bitwise_left_shift(f.shift).to(torch.uint16) if f.bits == 10 else t.to(torch.uint8)

        def chroma_planes():
            """[2, Hc, Wc] float codes"""
            if semi:
                return codes_of(planes[1][0]).permute(2, 0, 1)
            return torch.stack((codes_of(planes[1][0]), codes_of(planes[2][0])))

        def up_axis(c, dim, cosited, n):
            """one subsampled axis back to n luma samples: the two-tap rules of section 21 in float"""
            if not cosited:
                size = [2 * c.shape[1], c.shape[2]] if dim == 1 else [c.shape[1], 2 * c.shape[2]]
                return F.interpolate(c[None], size=size, mode="bilinear", align_corners=False)[0].narrow(dim, 0, n)
            nxt = torch.cat((c.narrow(dim, 1, c.shape[dim] - 1), c.narrow(dim, c.shape[dim] - 1, 1)), dim)
            return torch.stack((c, (c + nxt) * 0.5), dim + 1).flatten(dim, dim + 1).narrow(dim, 0, n)

        def torch_ingest():
            y = (codes_of(planes[0][0]) - yo) / ys
            c = (chroma_planes() - co) / cs
            if f.sx == 2:
                c = up_axis(c, 2, hco, W)
            if f.sy == 2:
                c = up_axis(c, 1, vco, H)
            out = torch.stack((y + k.a * c[1], y - k.b * c[0] - k.c * c[1], y + k.d * c[0]))[None].clamp_(0, 1)
            return F.pad(out, pad)

        w121 = torch.tensor([0.25, 0.5, 0.25], device="cuda")

        def down_axis(ch, dim, cosited):
            """one axis of the emit's filter on [2, h, w]"""
            if not cosited:
                return F.avg_pool2d(ch[None], (2, 1) if dim == 1 else (1, 2), ceil_mode=True)[0]
            p = F.pad(ch[None], (1, 1, 0, 0) if dim == 2 else (0, 0, 1, 1), mode="replicate")
            wt = w121.view(1, 1, 1, 3) if dim == 2 else w121.view(1, 1, 3, 1)
            return F.conv2d(p.transpose(0, 1), wt, stride=(1, 2) if dim == 2 else (2, 1)).transpose(0, 1)[0]

        def torch_emit(sums=False):
            c = F.pad(x_hat, unpad).clamp_(0, 1)[0]
            yf = k.kr * c[0] + k.kg * c[1] + k.kb * c[2]
            yc = (yf * ys + yo).round_().clamp_(0, top_code)
            ch = torch.stack(((c[2] - yf) * k.ib, (c[0] - yf) * k.ir)) * cs
            if f.sx == 2:
                ch = down_axis(ch, 2, hco)
            if f.sy == 2:
                ch = down_axis(ch, 1, vco)
            cc = (ch + co).round_().clamp_(0, top_code)
            if semi:
                out = (words_of(yc)[None], words_of(cc.permute(1, 2, 0)).contiguous()[None])
            else:
                out = (words_of(yc)[None], words_of(cc[0])[None], words_of(cc[1])[None])
            if not sums:
                return out
            rc = chroma_planes()
            return out, torch.stack((((yc - codes_of(planes[0][0])) ** 2).mean(), ((cc[0] - rc[0]) ** 2).mean(), ((cc[1] - rc[1]) ** 2).mean()))

        def out_codes(fr):
            return [codes_of(fr[0])] + ([codes_of(fr[1][..., 0]), codes_of(fr[1][..., 1])] if semi else [codes_of(fr[1]), codes_of(fr[2])])

        plane_bytes = es * (H * W + 2 * Hc * Wc)
        fbytes = 4 * 3 * geom.Hp * geom.Wp
        wbytes = 4 * 3 * H * W
        ib, eb, sb = plane_bytes + fbytes, wbytes + plane_bytes, wbytes + 2 * plane_bytes

        def copy_of(total):
            src = torch.empty(total // 2, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            return timed(lambda: dst.copy_(src))

        new_in = lambda: chroma.to_model_input(planes, fmt, siting=siting)                                   # noqa: E731
        new_out = lambda: chroma.from_model_output(x_hat, geom, fmt, siting=siting)                          # noqa: E731
        new_sums = lambda: chroma.from_model_output(x_hat, geom, fmt, siting=siting, ref=planes)             # noqa: E731
        x_new, _ = new_in()
        r = {"fmt": fmt, "siting": siting, "shape": [H, W], "padded": [geom.Hp, geom.Wp], "matrix": "bt709", "range": "limited",
             "unit": "us, median of 20 (HIP events, warm), taken five times, the sides of a pair alternating: median and max - min of "
                     "the five; the copies a median of 20",
             "wide_ingest": chroma.plan(chroma.INGEST, planes, fmt, x_new, geom),
             "wide_emit": chroma.plan(chroma.EMIT, planes, fmt, x_hat, geom, ref=planes),
             "ingest_bytes": ib, "emit_bytes": eb, "emit_with_sums_bytes": sb}
        r["ingest"], r["torch_ingest"] = alternating(new_in, torch_ingest)
        r["emit"], r["torch_emit"] = alternating(new_out, torch_emit)
        r["emit_with_sums_device_only"], r["torch_emit_with_sums_device_only"] = alternating(new_sums, lambda: torch_emit(True))
        r["copy_ingest_traffic"], r["copy_emit_traffic"], r["copy_emit_with_sums_traffic"] = copy_of(ib), copy_of(eb), copy_of(sb)
        for name, nbytes in (("ingest", ib), ("emit", eb), ("emit_with_sums_device_only", sb)):
            r[name + "_fraction_of_hbm_peak"] = round(nbytes / (r[name]["median"] * 1e-6) / HBM_PEAK, 4)
        r["ingest_max_abs_difference_from_torch"] = float((x_new - torch_ingest()).abs().max())
        r["emit_max_code_difference_from_torch"] = max(int((a - b).abs().max()) for a, b in zip(out_codes(new_out()), out_codes(torch_emit())))
        if (fmt, siting) == ("nv12", "centre"):
            old_in = lambda: frames.to_model_input(planes, fmt)                                              # noqa: E731
            old_out = lambda: frames.from_model_output(x_hat, geom, fmt)                                     # noqa: E731
            old_sums = lambda: frames.from_model_output(x_hat, geom, fmt, ref=planes)                        # noqa: E731
            fr = {}
            fr["chroma_ingest"], fr["frames_ingest"] = alternating(new_in, old_in)
            fr["chroma_emit"], fr["frames_emit"] = alternating(new_out, old_out)
            fr["chroma_emit_with_sums"], fr["frames_emit_with_sums"] = alternating(new_sums, old_sums)
            (a, da), (b, db) = new_sums(), old_sums()
            fr["same_bits"] = bool(torch.equal(x_new, old_in()[0]) and all(torch.equal(p, q) for p, q in zip(a, b)) and torch.equal(da.sse, db.sse))
            r["against_frames"] = fr
        print(json.dumps(r), flush=True)
        rows.append(r)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()

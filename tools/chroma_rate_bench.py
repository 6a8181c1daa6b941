"""Rate-controlled tiled coding of YUV frames of any subsampling and siting against what it replaces and against frame_rate (DESIGN.md
section 24): HIP events, warm, the median of five medians of 20 with the sides of a pair alternating and the spread (max - min of the
five) reported; one 2160 x 3840 frame, T = 512, O = 0 and 32, bt709, limited range; "nv12" at each siting, "p210" left, "i444".

  frame_tile_distortion   chroma_rate.frame_tile_distortion(x_hat_tiles, grid, planes, fmt, siting=...)   vs
     stitch_loop          at O = 0: one chroma_tiles.stitch_frame(tiles of the window's halo rectangle, window = the tile, ref=...,
                          image=False) per tile, what a user can write today (two launches per tile; under "left" / "topleft" it
                          reads the neighbour's last column / row, so its chroma sums are the stitch's, not the tile's own)
     torch_sequence       at O > 0: the torch restatement below (clamp, matrix, codes, the per-axis filters with the left / top
                          clamp, crop masks, weights, per-tile sums); exact at this size, compared with the kernel for equality
     copy                 dst.copy_(src) of a byte buffer with the same traffic: 12 bytes of floats per tile pixel inside the frame
                          (bands twice) and the original's samples under them.  The kernel is bound by these bytes.
  against frame_rate      on the centre "nv12" tiles, frame_rate.frame_tile_distortion alternating with this module's: the same work
  encode to a size        chroma_rate.encode_frame_tiled_to_size against chroma_tiles.encode_frame_tiled on one "p210" left frame,
                          a host clock around a synchronise, median of 3 (synthetic weights: times only)

Prints one JSON line per measurement; --out FILE also writes them all.

    python tools/chroma_rate_bench.py --out profiles/chroma_rate_times_mi355x.json

The figures above are whole Python calls.  Kernel times come from a trace, in a run of its own (--trace: the O = 0 calls of "nv12"
centre through frame_rate and through this module, "nv12" topleft, "p210" left and "i444", 200 times each, five distinct kernels),
folded without a GPU into the median duration per kernel after the first tenth of its dispatches:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o rate -- python tools/chroma_rate_bench.py --trace
    python tools/chroma_rate_bench.py --fold OUT/rate_kernel_trace.csv --out profiles/chroma_rate_kernel_times_mi355x.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.chroma_bench import alternating                                           # noqa: E402
from tools.chroma_tiles_bench import CASES, HBM_PEAK, PARAMS, T, smooth_frame         # noqa: E402
from tools.frame_rate_bench import as_tiles                                          # noqa: E402
from tools.rate_bench import inside_mask, int_weights                                # noqa: E402
from tools.tiles_bench import QUALITIES, model, timed, walled                        # noqa: E402

H, W = 2160, 3840


def axis_filter(u, dim, subsampled, cosited):
    """the emit's per-axis rule along dim for in-frame parts of even length: only the clamp at index 0 can bind -> (h, scale)"""
    import torch
    if not subsampled:
        return u, 1
    n = u.shape[dim]
    b, c = u.index_select(dim, torch.arange(0, n, 2, device=u.device)), u.index_select(dim, torch.arange(1, n, 2, device=u.device))
    if not cosited:
        return b + c, 2
    left = torch.arange(-1, n - 1, 2, device=u.device).clamp(min=0)
    return (u.index_select(dim, left) + c) + (b + b), 4


def torch_tile_distortion(x, ref_tiles, wl, wc, in_l, in_c, lv, k, f, hco, vco):
    """the sequence chroma_rate.frame_tile_distortion replaces -> float64 [n,3]"""
    import torch
    yo, ys, co, cs, top = lv
    c = x.clamp(0, 1)
    R, G, B = c[:, 0], c[:, 1], c[:, 2]
    Y = k.kr * R + k.kg * G + k.kb * B
    yq = (Y * ys + yo).round().clamp(0, top)
    out = [(((yq - ref_tiles[0]) ** 2).double() * in_l * wl).sum((1, 2))]
    for plane, ref in (((B - Y) * k.ib, ref_tiles[1]), ((R - Y) * k.ir, ref_tiles[2])):
        h, sh = axis_filter(plane * cs, 2, f.sx == 2, hco)
        v, sv = axis_filter(h, 1, f.sy == 2, vco)
        m = (v * (1.0 / (sh * sv)) + co).round().clamp(0, top)
        out.append((((m - ref) ** 2).double() * in_c * wc).sum((1, 2)))
    return torch.stack(out, 1)


def stitch_loop(x_hat, g, planes, fmt, siting):
    """what a user can write today at O = 0: the sums of every tile's own window, one stitch_frame call each -> int64 [n,3]"""
    import torch
    from progressivecodec_amd import chroma_tiles as kt
    out = []
    for t in range(g.n):
        i, j = divmod(t, g.nx)
        win = (i * g.S, j * g.S, min(g.T, g.H - i * g.S), min(g.T, g.W - j * g.S))
        ty0, tx0, nty, ntx = kt.covering(g, win, fmt, siting)
        idx = [(ty0 + a) * g.nx + tx0 + b for a in range(nty) for b in range(ntx)]
        part = x_hat[t:t + 1] if idx == [t] else x_hat[idx]
        out.append(kt.stitch_frame(part, g.with_rect((ty0, tx0, nty, ntx)), fmt, *PARAMS[:2], siting, window=win, ref=planes, image=False).sse[0])
    return torch.stack(out)


ROUNDS = 200
TRACED = [("nv12", "centre"), ("nv12", "topleft"), ("p210", "left"), ("i444", "centre")]


def trace():
    """the calls a kernel trace is taken of"""
    import torch
    from progressivecodec_amd import chroma_rate, frame_rate, tiles
    from progressivecodec_amd import chroma_tiles as kt
    g = tiles.grid_of(H, W, T, 0)
    for fmt, siting in TRACED:
        planes = smooth_frame(fmt, siting, H, W)
        x, _ = kt.cut_frame(planes, fmt, *PARAMS, siting, tile=T, overlap=0)
        for _ in range(ROUNDS):
            chroma_rate.frame_tile_distortion(x, g, planes, fmt, *PARAMS[:2], siting)
            if (fmt, siting) == TRACED[0]:
                frame_rate.frame_tile_distortion(x, g, planes, fmt, *PARAMS[:2])
        torch.cuda.synchronize()


def fold(path):
    import csv
    import statistics
    seq = {}
    for r in sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"])):
        n = r["Kernel_Name"]
        if "sse_kernel<" in n:
            args = n[n.index("sse_kernel<") + 11:n.index(">(")]
            key = ("frame_rate sse_kernel<%s>" if args.count(",") == 2 else "chroma_rate sse_kernel<%s>") % args
            seq.setdefault(key, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    return {"unit": "us, median kernel duration of a rocprofv3 kernel trace, the first tenth of each kernel's dispatches dropped; one run",
            "shape": [H, W], "tile": T, "overlap": 0, "calls": ["frame_rate nv12"] + ["chroma_rate %s %s" % c for c in TRACED],
            "kernels": {k: {"median": round(statistics.median(v[len(v) // 10:]) / 1e3, 2), "dispatches": len(v)} for k, v in seq.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--skip-codec", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--fold")
    args = ap.parse_args()
    if args.trace:
        return trace()
    if args.fold:
        r = fold(args.fold)
        print(json.dumps(r, indent=1))
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(r, fh, indent=1)
                fh.write("\n")
        return
    import torch
    from progressivecodec_amd import chroma, chroma_rate, frame_rate, frames, tiles
    from progressivecodec_amd import chroma_tiles as kt
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)
    unit = ("us, median of 20 (HIP events, warm), taken five times, the sides of a pair alternating: median and max - min of the five; "
            "the copies: one median of 20")
    k = frames.coefficients(PARAMS[0])
    for fmt, siting in CASES:
        f = chroma.FORMATS[fmt]
        es = 2 if f.bits == 10 else 1
        hs, vs = chroma.SITINGS[siting]
        hco, vco = f.sx == 2 and hs == chroma.COSITED, f.sy == 2 and vs == chroma.COSITED
        lv = frames.levels("p010" if f.bits == 10 else "nv12", PARAMS[1])
        planes = smooth_frame(fmt, siting, H, W)
        batched = tuple(p[None] for p in planes)
        code = lambda p: ((p.to(torch.int32) >> f.shift) & ((1 << f.bits) - 1)).float()                        # noqa: E731
        Yc = code(planes[0])
        Cb, Cr = (code(planes[1][..., 0]), code(planes[1][..., 1])) if f.layout == chroma.SEMIPLANAR else (code(planes[1]), code(planes[2]))
        for O in (0, 32):
            g = tiles.grid_of(H, W, T, O)
            x, _ = kt.cut_frame(planes, fmt, *PARAMS, siting, tile=T, overlap=O)
            gen = torch.Generator(device="cuda").manual_seed(O)
            x_hat = (x + 0.02 * torch.randn(x.shape, generator=gen, device="cuda")).contiguous()
            pixels_in = (H + (g.ny - 1) * O) * (W + (g.nx - 1) * O)               # tile pixels inside the frame, bands twice
            nbytes = 12 * pixels_in + es * (pixels_in + 2 * pixels_in // (f.sx * f.sy))
            call = lambda: chroma_rate.frame_tile_distortion(x_hat, g, planes, fmt, *PARAMS[:2], siting)        # noqa: E731
            r = {"what": "frame_tile_distortion", "fmt": fmt, "siting": siting, "shape": [H, W], "tile": T, "overlap": O, "tiles": [g.ny, g.nx],
                 "matrix": PARAMS[0], "range": PARAMS[1], "unit": unit, "wide": chroma_rate.plan(x_hat, batched, fmt, overlap=O),
                 "sse_exact": chroma_rate.sse_exact(g, fmt, siting), "bytes": nbytes}
            got = call()
            if O == 0:
                loop = lambda: stitch_loop(x_hat, g, planes, fmt, siting)                                      # noqa: E731
                r["frame_tile_distortion"], r["stitch_loop"] = alternating(call, loop)
                old = loop()
                r["luma_equals_stitch_loop"] = bool(torch.equal(got[:, 0], old[:, 0]))
                r["chroma_equals_stitch_loop"] = bool(torch.equal(got[:, 1:], old[:, 1:]))
                whole = kt.stitch_frame(x_hat, g, fmt, *PARAMS[:2], siting, ref=planes, image=False)
                r["sum_equals_stitch_frame_sse"] = [bool(a == b) for a, b in zip(got.sum(0).tolist(), whole.sse[0].tolist())]
                other = "stitch_loop"
            else:
                # the chroma planes cut per axis: rows by sy, columns by sx (not timed: the original, cut once)
                cut2 = lambda p: torch.nn.functional.pad(p, (0, (g.nx - 1) * g.S // f.sx + T // f.sx - p.shape[1], 0,                # noqa: E731
                                                             (g.ny - 1) * g.S // f.sy + T // f.sy - p.shape[0])) \
                    .unfold(0, T // f.sy, g.S // f.sy).unfold(1, T // f.sx, g.S // f.sx).reshape(g.n, T // f.sy, T // f.sx).contiguous()
                ref_tiles = (as_tiles(Yc, g, T, g.S), cut2(Cb), cut2(Cr))
                wy, wx = int_weights(g, "cuda")
                inside = inside_mask(g, "cuda")
                wl = (wy[:, None, :, None] * wx[None, :, None, :]).reshape(g.n, T, T)
                cy = (wy[:, 0::2] + wy[:, 1::2]) / 2 if f.sy == 2 else wy
                cx = (wx[:, 0::2] + wx[:, 1::2]) / 2 if f.sx == 2 else wx
                wc = (cy[:, None, :, None] * cx[None, :, None, :]).reshape(g.n, T // f.sy, T // f.sx)
                in_l, in_c = inside[:, 0], inside[:, 0, 0::f.sy, 0::f.sx]
                seq = lambda: torch_tile_distortion(x_hat, ref_tiles, wl, wc, in_l, in_c, lv, k, f, hco, vco)  # noqa: E731
                r["frame_tile_distortion"], r["torch_sequence"] = alternating(call, seq)
                old = seq()
                r["equals_torch"] = bool(torch.equal(got, old.to(torch.int64)))
                r["torch_max_relative_difference"] = float(((got.double() - old).abs() / got.double().clamp(min=1)).max())
                other = "torch_sequence"
                del ref_tiles, wl, wc, inside
            a = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
            b = torch.empty_like(a)
            r["copy_of_the_bytes"] = timed(lambda: b.copy_(a))
            del a, b
            us = r["frame_tile_distortion"]["median"]
            r["tb_per_s"] = round(nbytes / us / 1e6, 3)
            r["fraction_of_hbm_peak"] = round(nbytes / (us * 1e-6) / HBM_PEAK, 4)
            r["ratio_to_copy"] = round(us / r["copy_of_the_bytes"], 2)
            r["ratio_%s_to_new" % other] = round(r[other]["median"] / us, 1)
            r["bound"] = "bytes"
            emit(r)
            if (fmt, siting) == ("nv12", "centre"):
                fr = {"what": "chroma_rate against frame_rate, nv12 centre, the same tiles", "shape": [H, W], "tile": T, "overlap": O, "unit": unit}
                fr["chroma_rate"], fr["frame_rate"] = alternating(call, lambda: frame_rate.frame_tile_distortion(x_hat, g, planes, fmt, *PARAMS[:2]))
                fr["sums_equal"] = bool(torch.equal(got, frame_rate.frame_tile_distortion(x_hat, g, planes, fmt, *PARAMS[:2])))
                fr["difference_us"] = round(fr["chroma_rate"]["median"] - fr["frame_rate"]["median"], 2)
                fr["inside_the_pairs_spread"] = bool(abs(fr["difference_us"]) <= max(fr["chroma_rate"]["spread"], fr["frame_rate"]["spread"]))
                emit(fr)
            del x, x_hat
    if not args.skip_codec:
        net = model()
        fmt, siting = "p210", "left"
        planes = smooth_frame(fmt, siting, H, W)
        for O in (0, 32):
            r = {"what": "codec, encode_frame_tiled_to_size against encode_frame_tiled", "fmt": fmt, "siting": siting, "shape": [H, W], "tile": T,
                 "overlap": O, "qualities": QUALITIES, "unit": "s, median of 3 (host clock around a synchronise, warm)",
                 "weights": "synthetic: times only"}
            try:
                enc = lambda target: chroma_rate.encode_frame_tiled_to_size(net, planes, QUALITIES, target, fmt, *PARAMS, siting, tile=T, overlap=O)   # noqa: E731
                old = lambda: kt.encode_frame_tiled(net, planes, QUALITIES, fmt, *PARAMS, siting, tile=T, overlap=O)                                   # noqa: E731
                buf = old()
                r["encode_frame_tiled"] = walled(old)
                r["encode_frame_tiled_bytes"] = len(buf)
                _, plan = enc(10 ** 10)
                head = kt.HEADER_BYTES + tiles.HEADER_BYTES
                lo, hi = head + sum(min(v) for v in plan.rates), head + sum(max(v) for v in plan.rates)
                mid = (lo + hi) // 2
                out, plan = enc(mid)
                r["encode_frame_tiled_to_size"] = walled(lambda: enc(mid))
                r.update(target_bytes=mid, container_bytes=len(out), smallest=lo, largest=hi,
                         tiles_per_level=[plan.levels.count(l) for l in range(len(QUALITIES))], sse=plan.sse, sse_exact=plan.sse_exact)
                r["ratio"] = round(r["encode_frame_tiled_to_size"] / r["encode_frame_tiled"], 2)
                dec = kt.decode_frame_tiled(net, out)
                if O == 0:                                                     # luma: the plan's sum is the decoded frame's, exactly
                    ey = (dec[0].to(torch.int64) >> f_shift(fmt)) - (planes[0].to(torch.int64) >> f_shift(fmt))
                    r["plan_luma_sse_equals_decoded_frame"] = int((ey ** 2).sum()) == plan.sse[0]
                r["decode_frame_tiled_pct2"] = walled(lambda: kt.decode_frame_tiled(net, out))
            except Exception as e:                                             # a finding, recorded as such
                r["error"] = f"{type(e).__name__}: {e}"[:300]
            emit(r)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


def f_shift(fmt):
    from progressivecodec_amd import chroma
    return chroma.FORMATS[fmt].shift


if __name__ == "__main__":
    main()

"""Rate-controlled tiled coding of YUV 4:2:0 frames against what it replaces, on one 2160 x 3840 NV12 and one
P010 frame with T = 512 and O = 0 / 32, bt709, limited range: HIP events, warm, median of 20 for the kernel; a host clock around a
synchronise, median of 3, for the codec calls.

  frame_tile_distortion        frame_rate.frame_tile_distortion(x_hat_tiles, grid, planes, fmt)   vs
     (a) torch_sequence        the torch sequence below: clamp, the matrix, the luma code, the 2 x 2 chroma mean and its code, the
                               crop to the frame (masks), sub, square, the weight products, the per-tile sums
     (b) stitch_loop           at O = 0 only: one frame_tiles.stitch_frame(tile, window = the tile, ref=..., image=False) per tile, what
                               a user can write today (two launches per tile; without weights it is not the same quantity at O > 0)
     (c) copy                  a plain device copy (dst.copy_(src)) of the bytes the call must move: the rate this tool measures for
                               the same traffic
  encode_frame_tiled_to_size   vs frame_tiles.encode_frame_tiled with the same three levels (the encoder decodes every level once and
                               measures it)

The torch sequence is given the original's codes already cut into tiles and the weights and masks already built (none is timed),
which favours it; it sums in float64, which is exact at this size (every sum < 2^53), so its result is compared with the kernel's for
equality.  Bytes moved: 12 bytes of floats per tile pixel inside the frame (bands twice) and 1.5 elements of the original.  The
weights are synth.synthetic_state_dict's: times are meaningful with them, rate and distortion are not.  Prints one JSON line per
measurement; --out FILE also writes them all.

    python tools/frame_rate_bench.py --out profiles/frame_rate_times_mi355x.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.frame_tiles_bench import HBM_PEAK, PARAMS, QUALITIES, T, smooth_frame      # noqa: E402  (one frame, one clock)
from tools.rate_bench import inside_mask, int_weights                                # noqa: E402
from tools.tiles_bench import model, timed, walled                                   # noqa: E402

H, W = 2160, 3840


def as_tiles(plane, g, size, stride):
    """a float plane [h,w] -> [n,size,size]: the crops of the grid, zero beyond the plane (not timed: the original, cut once)"""
    import torch.nn.functional as F
    hg, wg = (g.ny - 1) * stride + size, (g.nx - 1) * stride + size
    p = F.pad(plane, (0, wg - plane.shape[1], 0, hg - plane.shape[0]))
    return p.unfold(0, size, stride).unfold(1, size, stride).reshape(g.n, size, size).contiguous()


def chroma_parts(g, wy, wx, inside):
    """the chroma weights cy * cx [n,T/2,T/2] (float64, exact integers) and the chroma mask, from the luma ones"""
    cy, cx = (wy[:, 0::2] + wy[:, 1::2]) / 2, (wx[:, 0::2] + wx[:, 1::2]) / 2
    w = (cy[:, None, :, None] * cx[None, :, None, :]).reshape(g.n, g.T // 2, g.T // 2)
    return w, inside[:, 0, 0::2, 0::2]


def torch_frame_tile_distortion(x, ref_tiles, wl, wc, in_l, in_c, lv, k):
    """the sequence frame_rate.frame_tile_distortion replaces -> float64 [n,3].  Every in-frame part here has even sizes, so the
    2 x 2 mean needs no edge clamp; it is written as four strided slices added in the contract's order (avg_pool2d adds the four in
    another order and so rounds otherwise)."""
    import torch
    yo, ys, co, cs, top = lv
    c = x.clamp(0, 1)
    R, G, B = c[:, 0], c[:, 1], c[:, 2]
    Y = k.kr * R + k.kg * G + k.kb * B
    yq = (Y * ys + yo).round().clamp(0, top)
    out = [(((yq - ref_tiles[0]) ** 2).double() * in_l * wl).sum((1, 2))]
    for plane, ref in (((B - Y) * k.ib, ref_tiles[1]), ((R - Y) * k.ir, ref_tiles[2])):
        u = plane * cs
        m = (((u[:, 0::2, 0::2] + u[:, 0::2, 1::2]) + (u[:, 1::2, 0::2] + u[:, 1::2, 1::2])) * 0.25 + co).round().clamp(0, top)
        out.append((((m - ref) ** 2).double() * in_c * wc).sum((1, 2)))
    return torch.stack(out, 1)


def stitch_loop(x_hat, g, planes, fmt):
    """what a user can write today at O = 0: the sums of every tile's own window, one stitch_frame call each -> int64 [n,3]"""
    import torch
    from progressivecodec_amd import frame_tiles
    out = []
    for t in range(g.n):
        i, j = divmod(t, g.nx)
        win = (i * g.S, j * g.S, min(g.T, g.H - i * g.S), min(g.T, g.W - j * g.S))
        out.append(frame_tiles.stitch_frame(x_hat[t:t + 1], g.with_rect((i, j, 1, 1)), fmt, *PARAMS[:2], window=win, ref=planes, image=False).sse[0])
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--skip-codec", action="store_true")
    args = ap.parse_args()
    import torch
    from progressivecodec_amd import frame_rate, frame_tiles, frames, tiles
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)
    k = frames.coefficients(PARAMS[0])
    for fmt in ("nv12", "p010"):
        es, sh = (2, 6) if fmt == "p010" else (1, 0)
        lv = frames.levels(fmt, PARAMS[1])
        planes = smooth_frame(fmt, H, W)
        batched = tuple(p[None] for p in planes)
        Yc = (planes[0].to(torch.int32) >> sh).float()
        Cb, Cr = ((planes[1][..., c].to(torch.int32) >> sh).float() for c in (0, 1))
        for O in (0, 32):
            g = tiles.grid_of(H, W, T, O)
            x, _ = frame_tiles.cut_frame(planes, fmt, *PARAMS, tile=T, overlap=O)
            gen = torch.Generator(device="cuda").manual_seed(O)
            x_hat = (x + 0.02 * torch.randn(x.shape, generator=gen, device="cuda")).contiguous()
            ref_tiles = (as_tiles(Yc, g, T, g.S), as_tiles(Cb, g, T // 2, g.S // 2), as_tiles(Cr, g, T // 2, g.S // 2))     # not timed
            wy, wx = int_weights(g, "cuda")
            inside = inside_mask(g, "cuda")
            wl = (wy[:, None, :, None] * wx[None, :, None, :]).reshape(g.n, T, T)
            wc, in_c = chroma_parts(g, wy, wx, inside)
            in_l = inside[:, 0]
            pixels_in = (H + (g.ny - 1) * O) * (W + (g.nx - 1) * O)               # tile pixels inside the frame, bands twice
            nbytes = 12 * pixels_in + es * (pixels_in + pixels_in // 2)
            a = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
            b = torch.empty_like(a)
            seq = lambda: torch_frame_tile_distortion(x_hat, ref_tiles, wl, wc, in_l, in_c, lv, k)      # noqa: E731
            call = lambda: frame_rate.frame_tile_distortion(x_hat, g, planes, fmt, *PARAMS[:2])         # noqa: E731
            r = {"what": "frame_tile_distortion", "fmt": fmt, "shape": [H, W], "tile": T, "overlap": O, "tiles": [g.ny, g.nx],
                 "matrix": PARAMS[0], "range": PARAMS[1], "unit": "us, median of 20 (HIP events, warm)",
                 "wide": frame_rate.plan(x_hat, batched, fmt, overlap=O),
                 "frame_tile_distortion": timed(call), "torch_sequence": timed(seq), "copy_of_the_bytes": timed(lambda: b.copy_(a)),
                 "bytes": nbytes}
            r["tb_per_s"] = round(nbytes / r["frame_tile_distortion"] / 1e6, 3)
            r["copy_tb_per_s"] = round(nbytes / r["copy_of_the_bytes"] / 1e6, 3)
            r["fraction_of_hbm_peak"] = round(nbytes / (r["frame_tile_distortion"] * 1e-6) / HBM_PEAK, 4)
            r["ratio_to_copy"] = round(r["frame_tile_distortion"] / r["copy_of_the_bytes"], 2)
            r["ratio_torch_to_new"] = round(r["torch_sequence"] / r["frame_tile_distortion"], 1)
            got = call()
            old = seq()
            r["equals_torch"] = bool(torch.equal(got, old.to(torch.int64)))
            r["torch_max_relative_difference"] = float(((got.double() - old).abs() / got.double().clamp(min=1)).max())
            if O == 0:
                r["stitch_loop"] = timed(lambda: stitch_loop(x_hat, g, planes, fmt))
                r["ratio_stitch_loop_to_new"] = round(r["stitch_loop"] / r["frame_tile_distortion"], 1)
                r["equals_stitch_loop"] = bool(torch.equal(got, stitch_loop(x_hat, g, planes, fmt)))
                whole = frame_tiles.stitch_frame(x_hat, g, fmt, *PARAMS[:2], ref=planes, image=False)
                r["sum_equals_stitch_frame_sse"] = bool(torch.equal(got.sum(0), whole.sse[0]))
            emit(r)
            del a, b
    if not args.skip_codec:
        net = model()
        for fmt in ("nv12", "p010"):
            planes = smooth_frame(fmt, H, W)
            for O in (0, 32):
                r = {"what": "codec, encode_frame_tiled_to_size against encode_frame_tiled", "fmt": fmt, "shape": [H, W], "tile": T, "overlap": O,
                     "qualities": QUALITIES, "unit": "s, median of 3 (host clock around a synchronise, warm)", "weights": "synthetic: times only"}
                try:
                    enc = lambda target: frame_rate.encode_frame_tiled_to_size(net, planes, QUALITIES, target, fmt, *PARAMS, tile=T, overlap=O)   # noqa: E731
                    old = lambda: frame_tiles.encode_frame_tiled(net, planes, QUALITIES, fmt, *PARAMS, tile=T, overlap=O)                          # noqa: E731
                    buf = old()
                    r["encode_frame_tiled"] = walled(old)
                    r["encode_frame_tiled_bytes"] = len(buf)
                    _, plan = enc(10 ** 10)
                    lo = 43 + sum(min(v) for v in plan.rates)
                    hi = 43 + sum(max(v) for v in plan.rates)
                    mid = (lo + hi) // 2
                    out, plan = enc(mid)
                    r["encode_frame_tiled_to_size"] = walled(lambda: enc(mid))
                    r.update(target_bytes=mid, container_bytes=len(out), smallest=lo, largest=hi,
                             tiles_per_level=[plan.levels.count(l) for l in range(len(QUALITIES))], sse=plan.sse)
                    r["ratio"] = round(r["encode_frame_tiled_to_size"] / r["encode_frame_tiled"], 2)
                    dec = frame_tiles.decode_frame_tiled(net, out)
                    if O == 0:                                                 # the plan's sums are the decoded frame's, exactly
                        sh = 6 if fmt == "p010" else 0
                        ey, ec = ((d.to(torch.int64) >> sh) - (p.to(torch.int64) >> sh) for d, p in zip(dec, planes))
                        r["plan_sse_equals_decoded_frame"] = [int((ey ** 2).sum()), int((ec[..., 0] ** 2).sum()), int((ec[..., 1] ** 2).sum())] == plan.sse
                    r["decode_frame_tiled_pct2"] = walled(lambda: frame_tiles.decode_frame_tiled(net, out))
                    r["decode_frame_tiled_pct1"] = walled(lambda: frame_tiles.decode_frame_tiled(net, buf))
                except Exception as e:                                         # a finding, recorded as such
                    r["error"] = f"{type(e).__name__}: {e}"[:300]
                emit(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

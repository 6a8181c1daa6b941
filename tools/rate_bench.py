"""Rate-controlled tiled coding against what it replaces, on one 3x2160x3840 frame with T = 512 and O = 0 / 32:
HIP events, warm, median of 20 for the kernel; a host clock around a synchronise, median of 3, for the codec calls.

  tile_distortion        rate.tile_distortion(x_hat_tiles, grid, ref)   vs  the torch sequence below: clamp, mul(255), round, the crop
                                                                            to the image (a mask), sub, square, the weight product,
                                                                            the per-tile sum
  copy                   a plain device copy (dst.copy_(src)) of the bytes the call must move: the rate this tool measures for the
                         same traffic
  encode_tiled_to_size   vs tiles.encode_tiled with the same three levels (the encoder decodes every level once and measures it)

The torch sequence is given the original already cut into tiles and the weights and the mask already built (neither is timed), which
favours it; it sums in float64, which is exact at this size (every sum < 2^53), so its result is compared with the kernel's for
equality.  Bytes moved: 12 bytes of floats and 3 bytes of the original per tile pixel inside the image (bands twice).  The weights are
synth.synthetic_state_dict's: times are meaningful with them, rate and distortion are not.  Prints one JSON line per measurement;
--out FILE also writes them all.

    python tools/rate_bench.py --out profiles/rate_times_mi355x.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.tiles_bench import HBM_PEAK, QUALITIES, H, T, W, frame, model, timed, walled      # noqa: E402  (one frame, one clock)


def int_weights(g, device):
    """per-axis integer weights [n_axis, T] (the numerators over den) as the definition gives them"""
    import torch
    den = 2 * g.O if g.O else 1

    def axis(n):
        w = torch.full((n, g.T), den, dtype=torch.float64)
        if g.O:
            up = 2 * torch.arange(g.O, dtype=torch.float64) + 1
            w[1:, :g.O] = up
            w[:-1, g.S:] = up.flip(0)
        return w.to(device)
    return axis(g.ny), axis(g.nx)


def inside_mask(g, device):
    """[n,1,T,T] float64: 1 where the tile's pixel lies inside the image"""
    import torch
    ys = torch.arange(g.ny)[:, None] * g.S + torch.arange(g.T)[None, :] < g.H          # [ny,T]
    xs = torch.arange(g.nx)[:, None] * g.S + torch.arange(g.T)[None, :] < g.W          # [nx,T]
    m = ys[:, None, :, None] & xs[None, :, None, :]
    return m.reshape(g.n, 1, g.T, g.T).double().to(device)


def torch_tile_distortion(x_tiles, ref_tiles, wy, wx, inside, g):
    """the sequence rate.tile_distortion replaces -> float64 [n,3]"""
    q = x_tiles.clamp(0, 1).mul(255).round()
    e = q - ref_tiles
    e2 = (e * e).double() * inside
    w = (wy[:, None, :, None] * wx[None, :, None, :]).reshape(g.n, 1, g.T, g.T)
    return (e2 * w).sum((2, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--skip-codec", action="store_true")
    args = ap.parse_args()
    import torch
    from progressivecodec_amd import rate, tiles
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)
    img = frame()
    chw = img.permute(2, 0, 1).contiguous()
    for O in (0, 32):
        g = tiles.grid_of(H, W, T, O)
        x, _ = tiles.cut(img, T, O)
        x_hat = (x + 0.02 * torch.randn_like(x)).contiguous()
        ref_tiles = x.mul(255).round()                                          # the original as tiles of floats: not timed
        wy, wx = int_weights(g, "cuda")
        inside = inside_mask(g, "cuda")
        pixels_in = (H + (g.ny - 1) * O) * (W + (g.nx - 1) * O)                  # tile pixels inside the image, bands twice
        nbytes = 15 * pixels_in
        a = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        b = torch.empty_like(a)
        r = {"what": "tile_distortion", "frame": [3, H, W], "tile": T, "overlap": O, "tiles": [g.ny, g.nx],
             "unit": "us, median of 20 (HIP events, warm)",
             "tile_distortion_hwc": timed(lambda: rate.tile_distortion(x_hat, g, img)),
             "tile_distortion_chw": timed(lambda: rate.tile_distortion(x_hat, g, chw, ref_layout="chw")),
             "torch_sequence": timed(lambda: torch_tile_distortion(x_hat, ref_tiles, wy, wx, inside, g)),
             "copy_of_the_bytes": timed(lambda: b.copy_(a)),
             "bytes": nbytes}
        r["tb_per_s"] = round(nbytes / r["tile_distortion_hwc"] / 1e6, 3)
        r["copy_tb_per_s"] = round(nbytes / r["copy_of_the_bytes"] / 1e6, 3)
        r["fraction_of_hbm_peak"] = round(nbytes / (r["tile_distortion_hwc"] * 1e-6) / HBM_PEAK, 4)
        r["ratio_to_copy"] = round(r["tile_distortion_hwc"] / r["copy_of_the_bytes"], 2)
        r["ratio_torch_to_new"] = round(r["torch_sequence"] / r["tile_distortion_hwc"], 1)
        got = rate.tile_distortion(x_hat, g, img)
        r["equals_torch"] = bool(torch.equal(got, torch_tile_distortion(x_hat, ref_tiles, wy, wx, inside, g).to(torch.int64)))
        r["equals_chw"] = bool(torch.equal(got, rate.tile_distortion(x_hat, g, chw, ref_layout="chw")))
        if O == 0:
            r["sum_equals_stitch_sse_u8"] = bool(torch.equal(got.sum(0), tiles.stitch(x_hat, g, ref=img, image=False).sse_u8[0]))
        emit(r)
        del a, b
    if not args.skip_codec:
        net = model()
        for O in (0, 32):
            r = {"what": "codec, encode_tiled_to_size against encode_tiled", "frame": [3, H, W], "tile": T, "overlap": O,
                 "qualities": QUALITIES, "unit": "s, median of 3 (host clock around a synchronise, warm)", "weights": "synthetic: times only"}
            try:
                buf = tiles.encode_tiled(net, img, QUALITIES, T, O)
                r["encode_tiled"] = walled(lambda: tiles.encode_tiled(net, img, QUALITIES, T, O))
                r["encode_tiled_bytes"] = len(buf)
                _, plan = rate.encode_tiled_to_size(net, img, QUALITIES, 10 ** 10, T, O)
                lo = 33 + sum(min(v) for v in plan.rates)
                hi = 33 + sum(max(v) for v in plan.rates)
                mid = (lo + hi) // 2
                out, plan = rate.encode_tiled_to_size(net, img, QUALITIES, mid, T, O)
                r["encode_tiled_to_size"] = walled(lambda: rate.encode_tiled_to_size(net, img, QUALITIES, mid, T, O))
                r.update(target_bytes=mid, container_bytes=len(out), smallest=lo, largest=hi,
                         tiles_per_level=[plan.levels.count(l) for l in range(len(QUALITIES))])
                r["ratio"] = round(r["encode_tiled_to_size"] / r["encode_tiled"], 2)
                r["decode_tiled_pct2"] = walled(lambda: tiles.decode_tiled(net, out))
                r["decode_tiled_pct1"] = walled(lambda: tiles.decode_tiled(net, buf))
            except Exception as e:                                             # a finding, recorded as such
                r["error"] = f"{type(e).__name__}: {e}"[:300]
            emit(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

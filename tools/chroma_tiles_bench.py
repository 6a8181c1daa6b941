"""Tiled coding of YUV frames of any subsampling and siting against the two-step sequences it replaces and against frame_tiles
(DESIGN.md section 23): HIP events, warm, the median of five medians of 20 with the sides of a pair alternating and the spread
(max - min of the five) reported; one 2160 x 3840 frame, T = 512, O = 0 and 32, bt709, limited range, linear upsampling; "nv12" at
each siting, "p210" left, "i444".

  cut               chroma_tiles.cut_frame(planes, fmt, siting)         vs  chroma.to_model_input, then torch: crop the padding, F.pad
                                                                            to the grid, unfold / permute / contiguous into [n,3,T,T]
  stitch            chroma_tiles.stitch_frame(x_hat_tiles, grid, ...)   vs  torch: clamp, per-band weights, one weighted add per tile
                                                                            into a float frame; then chroma.from_model_output of it
  stitch with sums  ... (ref=planes), device only                       vs  the same with ref=planes
  copy              dst.copy_(src) of a byte buffer with the same traffic (bytes read + bytes written = the bytes the call must move)
  frame_tiles       on the "nv12" centre frame, frame_tiles.cut_frame / stitch_frame alternating with this module's: the same work
  siting            the stitch under "left" and "topleft" alternating with "centre" on the same tiles: what the halo costs in a
                    blended kernel

The torch halves are what a user would write, not a restatement: the weighted adds are not fused, so codes may differ by one (the
count is reported).  Prints one JSON line per measurement; --out FILE also writes them all.

    python tools/chroma_tiles_bench.py --out profiles/chroma_tiles_times_mi355x.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.chroma_bench import alternating      # noqa: E402
from tools.tiles_bench import timed, torch_weights      # noqa: E402

HBM_PEAK = 8.0e12
T = 512
PARAMS = ("bt709", "limited", "linear")
CASES = [("nv12", "centre"), ("nv12", "left"), ("nv12", "topleft"), ("p210", "left"), ("i444", "centre")]


def smooth_frame(fmt, siting, H, W):
    """a smooth in-gamut picture: low-resolution noise enlarged, emitted once by the chroma layer itself -> planes without a batch axis"""
    import torch
    import torch.nn.functional as F
    from progressivecodec_amd import chroma
    g = torch.Generator(device="cuda").manual_seed(H)
    lo = torch.rand((1, 3, H // 40, W // 40), generator=g, device="cuda") * 0.8 + 0.1
    rgb = F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False)
    return tuple(p[0] for p in chroma.from_model_output(rgb, chroma.Geometry(H, W, H, W, 0, 0), fmt, siting=siting))


def two_step_cut(planes, fmt, siting, g):
    """what a user would write today: the whole-frame ingest, then torch slicing and padding into tiles"""
    import torch.nn.functional as F
    from progressivecodec_amd import chroma
    x, geom = chroma.to_model_input(planes, fmt, *PARAMS, siting=siting)
    S = g.S
    Hg, Wg = (g.ny - 1) * S + g.T, (g.nx - 1) * S + g.T
    x = F.pad(x[0, :, geom.top:geom.top + g.H, geom.left:geom.left + g.W], (0, Wg - g.W, 0, Hg - g.H))
    t = x.unfold(1, g.T, S).unfold(2, g.T, S)                              # [3, ny, nx, T, T]
    return t.permute(1, 2, 0, 3, 4).reshape(g.n, 3, g.T, g.T).contiguous()


def two_step_stitch(x_tiles, g, wy, wx, fmt, siting, ref=None):
    """what a user would write today: a torch blend of the tiles into a float frame, then the whole-frame emit"""
    import torch
    from progressivecodec_amd import chroma
    S = g.S
    Hg, Wg = (g.ny - 1) * S + g.T, (g.nx - 1) * S + g.T
    c = x_tiles.clamp(0, 1).view(g.ny, g.nx, 3, g.T, g.T)
    c = c * (wy[:, None, None, :, None] * wx[None, :, None, None, :])
    acc = torch.zeros((1, 3, Hg, Wg), dtype=torch.float32, device=x_tiles.device)
    for i in range(g.ny):
        for j in range(g.nx):
            acc[0, :, i * S:i * S + g.T, j * S:j * S + g.T] += c[i, j]
    return chroma.from_model_output(acc, chroma.Geometry(g.H, g.W, Hg, Wg, 0, 0), fmt, PARAMS[0], PARAMS[1], siting, ref=ref)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--size", type=int, nargs=2, default=[2160, 3840])
    args = ap.parse_args()
    import torch
    from progressivecodec_amd import chroma, frame_tiles, tiles
    from progressivecodec_amd import chroma_tiles as kt
    H, W = args.size
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    def copy_of(total):
        src = torch.empty(total // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        return timed(lambda: dst.copy_(src))

    def codes(t):
        return t.to(torch.int32)
    unit = ("us, median of 20 (HIP events, warm), taken five times, the sides of a pair alternating: median and max - min of the five; "
            "the copies: one median of 20")
    for fmt, siting in CASES:
        f = chroma.FORMATS[fmt]
        es = 2 if f.bits == 10 else 1
        planes = smooth_frame(fmt, siting, H, W)
        batched = tuple(p[None] for p in planes)
        Hc, Wc = chroma.chroma_size(H, W, fmt)
        plane_bytes = es * (H * W + 2 * Hc * Wc)
        for O in (0, 32):
            g = tiles.grid_of(H, W, T, O)
            x, _ = kt.cut_frame(planes, fmt, *PARAMS, siting, tile=T, overlap=O)
            gen = torch.Generator(device="cuda").manual_seed(O)
            x_hat = (x + 0.02 * torch.randn(x.shape, generator=gen, device="cuda")).contiguous()
            wy, wx = torch_weights(g, "cuda")
            cut_bytes = plane_bytes + 4 * x.numel()
            st_bytes = 12 * (H + (g.ny - 1) * O) * (W + (g.nx - 1) * O) + plane_bytes       # the tiles where they cover the frame (bands twice)
            out = kt.stitch_frame(x_hat, g, fmt, *PARAMS[:2], siting)
            r = {"what": "kernels", "fmt": fmt, "siting": siting, "shape": [H, W], "tile": T, "overlap": O, "tiles": [g.ny, g.nx],
                 "matrix": PARAMS[0], "range": PARAMS[1], "upsample": PARAMS[2], "unit": unit,
                 "wide_cut": kt.plan(kt.CUT, batched, fmt, x, overlap=O),
                 "wide_stitch": kt.plan(kt.STITCH, tuple(p[None] for p in out), fmt, x_hat, ref=batched),
                 "cut_bytes": cut_bytes, "stitch_bytes": st_bytes, "stitch_with_sums_bytes": st_bytes + plane_bytes}
            r["cut"], r["two_step_cut"] = alternating(lambda: kt.cut_frame(planes, fmt, *PARAMS, siting, tile=T, overlap=O),
                                                      lambda: two_step_cut(planes, fmt, siting, g))
            r["stitch"], r["two_step_stitch"] = alternating(lambda: kt.stitch_frame(x_hat, g, fmt, *PARAMS[:2], siting),
                                                            lambda: two_step_stitch(x_hat, g, wy, wx, fmt, siting))
            r["stitch_with_sums_device_only"], r["two_step_stitch_with_sums_device_only"] = alternating(
                lambda: kt.stitch_frame(x_hat, g, fmt, *PARAMS[:2], siting, ref=planes),
                lambda: two_step_stitch(x_hat, g, wy, wx, fmt, siting, ref=planes))
            r["copy_cut_traffic"] = copy_of(cut_bytes)
            r["copy_stitch_traffic"] = copy_of(st_bytes)
            r["copy_stitch_with_sums_traffic"] = copy_of(st_bytes + plane_bytes)
            r["cut_fraction_of_hbm_peak"] = round(cut_bytes / (r["cut"]["median"] * 1e-6) / HBM_PEAK, 4)
            r["stitch_fraction_of_hbm_peak"] = round(st_bytes / (r["stitch"]["median"] * 1e-6) / HBM_PEAK, 4)
            r["cut_equals_two_step"] = bool(torch.equal(x, two_step_cut(planes, fmt, siting, g)))
            old = two_step_stitch(x_hat, g, wy, wx, fmt, siting)
            r["stitch_codes_that_differ_from_two_step"] = int(sum((codes(a) != codes(b[0])).sum() for a, b in zip(out, old)))
            r["stitch_max_code_difference_from_two_step"] = int(max((codes(a) - codes(b[0])).abs().max() for a, b in zip(out, old))) >> f.shift
            emit(r)
            if (fmt, siting) == ("nv12", "centre"):
                # the same work through section 14's library, alternating
                fr = {"what": "chroma_tiles against frame_tiles, nv12 centre", "shape": [H, W], "tile": T, "overlap": O, "unit": unit}
                fr["chroma_tiles_cut"], fr["frame_tiles_cut"] = alternating(lambda: kt.cut_frame(planes, fmt, *PARAMS, siting, tile=T, overlap=O),
                                                                            lambda: frame_tiles.cut_frame(planes, fmt, *PARAMS, tile=T, overlap=O))
                fr["chroma_tiles_stitch"], fr["frame_tiles_stitch"] = alternating(lambda: kt.stitch_frame(x_hat, g, fmt, *PARAMS[:2], siting),
                                                                                  lambda: frame_tiles.stitch_frame(x_hat, g, fmt, *PARAMS[:2]))
                fr["chroma_tiles_stitch_with_sums"], fr["frame_tiles_stitch_with_sums"] = alternating(
                    lambda: kt.stitch_frame(x_hat, g, fmt, *PARAMS[:2], siting, ref=planes),
                    lambda: frame_tiles.stitch_frame(x_hat, g, fmt, *PARAMS[:2], ref=planes))
                a, b = kt.stitch_frame(x_hat, g, fmt, *PARAMS[:2], siting), frame_tiles.stitch_frame(x_hat, g, fmt, *PARAMS[:2])
                fr["planes_equal"] = bool(all(torch.equal(p, q) for p, q in zip(a, b)))
                fr["tiles_equal"] = bool(torch.equal(x, frame_tiles.cut_frame(planes, fmt, *PARAMS, tile=T, overlap=O)[0]))
                emit(fr)
                # what the halo costs in a blended kernel: the same tiles stitched under each siting, alternating
                hr = {"what": "the stitch under each siting, nv12, the same tiles", "shape": [H, W], "tile": T, "overlap": O, "unit": unit}
                hr["centre"], hr["left"], hr["topleft"] = alternating(*[(lambda s=s: kt.stitch_frame(x_hat, g, fmt, *PARAMS[:2], s))
                                                                        for s in ("centre", "left", "topleft")])
                hr["centre_with_sums"], hr["left_with_sums"], hr["topleft_with_sums"] = alternating(
                    *[(lambda s=s: kt.stitch_frame(x_hat, g, fmt, *PARAMS[:2], s, ref=planes)) for s in ("centre", "left", "topleft")])
                emit(hr)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

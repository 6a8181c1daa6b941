"""Clips of YUV frames of any subsampling and siting against what they replace and against clips: HIP events,
warm, the median of five medians of 20 with the sides of a pair alternating and the spread (max - min of the five) reported; 2160 x
3840 frames, T = 512, O = 0 and 32, bt709, limited range, linear upsampling; "nv12" at each siting, "p210" left, "i444".

  tile_changes   chroma_clips.tile_changes(cur, prev, fmt, siting)   vs  the torch sequence below: per plane the codes' `!=`, then per
                                                                         tile the sums over the footprint rectangles
                                                                     vs  a device copy of the bytes the call must read (both frames)
  cut_tiles      chroma_clips.cut_tiles of 16 scattered tiles        vs  16 calls of chroma_tiles.cut_frame(rect=(ty, tx, 1, 1)) and one
                                                                         torch.cat: what a user would write today
                                                                     vs  a device copy of the bytes the call must move
  clips          on the "nv12" centre frames, clips.tile_changes / clips.cut_tiles alternating with this module's: the same work
  codec          encode_clip with reuse on and off on an 8-frame 1080p "p210" left-sited clip -- one smooth frame with a 200 x 200 block
                 that moves 64 pixels per frame -- vs the loop of chroma_tiles.encode_frame_tiled over the same frames: a host clock
                 around a synchronise, times and bytes

The weights are synth.synthetic_state_dict's: times, byte counts and exactness are meaningful with them, rate and distortion are not.
Prints one JSON line per measurement; --out FILE also writes them all.

    python tools/chroma_clips_bench.py --out profiles/chroma_clips_times_mi355x.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.chroma_bench import alternating                   # noqa: E402
from tools.chroma_tiles_bench import CASES, HBM_PEAK, PARAMS, T, smooth_frame      # noqa: E402
from tools.clips_bench import walled_all                     # noqa: E402
from tools.tiles_bench import model, timed                   # noqa: E402

QUALITIES = [0, 0.5]
CLIP = dict(H=1080, W=1920, frames=8, block=200, step=64, fmt="p210", siting="left")
UNIT = ("us, median of 20 (HIP events, warm), taken five times, the sides of a pair alternating: median and max - min of the five; the "
        "copies: one median of 20")


def footprints(g, fmt, siting, linear=True):
    """per tile (luma (y0, y1, x0, x1), chroma (y0, y1, x0, x1)), half-open: chroma_clips.py's footprint, restated"""
    from progressivecodec_amd import chroma
    f, (hco, vco) = chroma.FORMATS[fmt], chroma.SITINGS[siting]

    def axis(i, L, sub, cosited):
        e = min(i * g.S + g.T, L)
        if sub == 1:
            return (i * g.S, e), (i * g.S, e)
        hi, lo = int(linear), int(linear and not cosited)
        return (i * g.S, e), (max(i * g.S // 2 - lo, 0), min(-(-e // 2) - 1 + hi, -(-L // 2) - 1) + 1)
    out = []
    for i in range(g.ny):
        for j in range(g.nx):
            (ly, cy), (lx, cx) = axis(i, g.H, f.sy, vco), axis(j, g.W, f.sx, hco)
            out.append((ly + lx, cy + cx))
    return out


def torch_tile_changes(cur, prev, fmt, rects):
    """the sequence chroma_clips.tile_changes replaces -> int64 [n,3]: the planes' codes compared, then one sum per tile and plane"""
    import torch
    from progressivecodec_amd import chroma
    f = chroma.FORMATS[fmt]
    code = (lambda t: (t.to(torch.int32) >> f.shift) & 1023) if f.bits == 10 else (lambda t: t)
    d = [code(a) != code(b) for a, b in zip(cur, prev)]
    du, dv = (d[1][..., 0], d[1][..., 1]) if f.layout == chroma.SEMIPLANAR else (d[1], d[2])
    out = []
    for lu, ch in rects:
        out.append(torch.stack([d[0][lu[0]:lu[1], lu[2]:lu[3]].sum(), du[ch[0]:ch[1], ch[2]:ch[3]].sum(), dv[ch[0]:ch[1], ch[2]:ch[3]].sum()]))
    return torch.stack(out)


def with_block(planes, fmt, y, x, size, luma, cb, cr):
    """a copy of a frame with a size x size block (y, x and size even) of flat colour"""
    import torch
    from progressivecodec_amd import chroma
    f = chroma.FORMATS[fmt]
    out = tuple(p.clone() for p in planes)
    v = [p.view(torch.int16) if p.dtype == torch.uint16 else p for p in out]         # written as int16: the same 16 bits
    luma, cb, cr = ((c << f.shift) - (65536 if (c << f.shift) >= 32768 else 0) for c in (luma, cb, cr))
    v[0][y:y + size, x:x + size] = luma
    rows, cols = slice(y // f.sy, (y + size) // f.sy), slice(x // f.sx, (x + size) // f.sx)
    if f.layout == chroma.SEMIPLANAR:
        v[1][rows, cols, 0] = cb
        v[1][rows, cols, 1] = cr
    else:
        v[1][rows, cols] = cb
        v[2][rows, cols] = cr
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--size", type=int, nargs=2, default=[2160, 3840])
    ap.add_argument("--skip-codec", action="store_true")
    args = ap.parse_args()
    import torch
    from progressivecodec_amd import chroma, chroma_tiles, clips, tiles
    from progressivecodec_amd import chroma_clips as kc
    H, W = args.size
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    def copy_of(total):
        src = torch.empty(total // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        return timed(lambda: dst.copy_(src))

    batched = lambda planes: tuple(p[None] for p in planes)                                                            # noqa: E731
    for fmt, siting in CASES:
        f = chroma.FORMATS[fmt]
        es = 2 if f.bits == 10 else 1
        top = 1 << (f.bits - 8)
        prev = smooth_frame(fmt, siting, H, W)
        cur = with_block(prev, fmt, 600, 1000, 200, 180 * top, 90 * top, 160 * top)
        Hc, Wc = chroma.chroma_size(H, W, fmt)
        plane_bytes = es * (H * W + 2 * Hc * Wc)
        for O in (0, 32):
            g = tiles.grid_of(H, W, T, O)
            rects = footprints(g, fmt, siting)
            call = lambda: kc.tile_changes(cur, prev, fmt, siting, T, O, PARAMS[2])           # noqa: E731
            seq = lambda: torch_tile_changes(cur, prev, fmt, rects)                             # noqa: E731
            r = {"what": "tile_changes", "fmt": fmt, "siting": siting, "shape": [H, W], "tile": T, "overlap": O, "tiles": [g.ny, g.nx],
                 "upsample": PARAMS[2], "unit": UNIT, "wide": kc.plan(kc.CHANGES, batched(cur), fmt, other=batched(prev), overlap=O),
                 "bytes": 2 * plane_bytes}
            r["tile_changes"], r["torch_sequence"] = alternating(call, seq)
            r["copy_of_the_bytes"] = copy_of(2 * plane_bytes)
            r["fraction_of_hbm_peak"] = round(2 * plane_bytes / (r["tile_changes"]["median"] * 1e-6) / HBM_PEAK, 4)
            r["ratio_to_copy"] = round(r["tile_changes"]["median"] / r["copy_of_the_bytes"], 2)
            r["ratio_torch_to_new"] = round(r["torch_sequence"]["median"] / r["tile_changes"]["median"], 1)
            got = call()
            r["equals_torch"] = bool(torch.equal(got, seq()))
            r["tiles_changed"] = int((got != 0).any(1).sum())
            emit(r)

            idx = [(7 * m + 3) % (g.ny * g.nx) for m in range(16)]
            out = torch.empty((len(idx), 3, T, T), dtype=torch.float32, device="cuda")
            new = lambda: kc.cut_tiles(cur, fmt, idx, *PARAMS, siting, T, O, out=out)           # noqa: E731
            old = lambda: torch.cat([chroma_tiles.cut_frame(cur, fmt, *PARAMS, siting, T, O, rect=(t // g.nx, t % g.nx, 1, 1))[0] for t in idx])  # noqa: E731
            cut_bytes = 4 * out.numel() + len(idx) * es * (T * T + 2 * (T // f.sx) * (T // f.sy))
            c = {"what": "cut_tiles", "fmt": fmt, "siting": siting, "shape": [H, W], "tile": T, "overlap": O, "k": len(idx), "tile_indices": idx,
                 "unit": UNIT + "; cut_tiles includes the upload of its k indices", "wide": kc.plan(kc.CUT, batched(cur), fmt, f32=out, overlap=O),
                 "bytes": cut_bytes}
            c["cut_tiles"], c["k_calls_of_cut_frame"] = alternating(new, old)
            c["copy_of_the_bytes"] = copy_of(cut_bytes)
            c["ratio_to_copy"] = round(c["cut_tiles"]["median"] / c["copy_of_the_bytes"], 2)
            c["ratio_loop_to_new"] = round(c["k_calls_of_cut_frame"]["median"] / c["cut_tiles"]["median"], 2)
            c["same_bits"] = bool(torch.equal(new().view(torch.int32), old().view(torch.int32)))
            emit(c)

            if (fmt, siting) == ("nv12", "centre"):
                # the same work through section 16's library, alternating: expected within the two spreads
                s = {"what": "chroma_clips against clips, nv12 centre", "shape": [H, W], "tile": T, "overlap": O, "unit": UNIT}
                s["chroma_clips_tile_changes"], s["clips_tile_changes"] = alternating(call, lambda: clips.tile_changes(cur, prev, fmt, T, O, PARAMS[2]))
                s["chroma_clips_cut_tiles"], s["clips_cut_tiles"] = alternating(new, lambda: clips.cut_tiles(cur, fmt, idx, *PARAMS, T, O, out=out))
                for name in ("tile_changes", "cut_tiles"):
                    a, b = s["chroma_clips_" + name], s["clips_" + name]
                    s[name + "_slower_by"] = round(a["median"] - b["median"], 2)
                    s[name + "_within_the_two_spreads"] = a["median"] - b["median"] <= a["spread"] + b["spread"]
                s["counts_equal"] = bool(torch.equal(call(), clips.tile_changes(cur, prev, fmt, T, O, PARAMS[2])))
                ours = new().clone()
                s["tiles_equal"] = bool(torch.equal(ours.view(torch.int32), clips.cut_tiles(cur, fmt, idx, *PARAMS, T, O).view(torch.int32)))
                emit(s)

    if not args.skip_codec:
        net = model()
        c = CLIP
        fmt, siting = c["fmt"], c["siting"]
        base = smooth_frame(fmt, siting, c["H"], c["W"])
        frames = [with_block(base, fmt, 400, 100 + c["step"] * k, c["block"], 800, 320, 680) for k in range(c["frames"])]
        kw = dict(siting=siting, tile=T, overlap=0)
        g = tiles.grid_of(c["H"], c["W"], T, 0)
        r = {"what": "codec, encode_clip against the loop of encode_frame_tiled", "clip": c, "tile": T, "overlap": 0,
             "tiles_per_frame": g.ny * g.nx, "qualities": QUALITIES, "unit": "s (host clock around a synchronise, warm), median of 3",
             "weights": "synthetic: times, bytes and exactness only"}
        try:
            loop_enc = lambda: [chroma_tiles.encode_frame_tiled(net, fr, QUALITIES, fmt, *PARAMS, **kw) for fr in frames]       # noqa: E731
            enc = lambda reuse: kc.encode_clip(net, frames, QUALITIES, fmt, *PARAMS, reuse=reuse, **kw)                       # noqa: E731
            alone = loop_enc()
            buf, plan = enc(True)
            every, plan_all = enc(False)
            r["frame_containers_equal_the_loop"] = all(kc.frame_container(buf, k) == alone[k] == kc.frame_container(every, k)
                                                       for k in range(c["frames"]))
            r.update(loop_bytes=sum(map(len, alone)), clip_bytes_reuse=len(buf), clip_bytes_no_reuse=len(every), tiles_coded_reuse=plan.n_coded,
                     tiles_coded_no_reuse=plan_all.n_coded, tiles_reused=plan.n_reused,
                     coded_per_frame=[sum(s == k for s in row) for k, row in enumerate(plan.source)])
            for name, fn in (("loop_encode", loop_enc), ("encode_clip_no_reuse", lambda: enc(False)), ("encode_clip_reuse", lambda: enc(True))):
                ts = walled_all(fn, 3)
                r[name + "_runs"], r[name] = ts, statistics.median(ts)
            r["loop_encode_spread"] = round(max(r["loop_encode_runs"]) - min(r["loop_encode_runs"]), 4)
            r["no_reuse_not_slower_than_loop_beyond_spread"] = r["encode_clip_no_reuse"] <= r["loop_encode"] + r["loop_encode_spread"]
            r["ratio_loop_to_no_reuse"] = round(r["loop_encode"] / r["encode_clip_no_reuse"], 3)
            r["ratio_loop_to_reuse"] = round(r["loop_encode"] / r["encode_clip_reuse"], 2)
        except Exception as e:                                                     # a finding, recorded as such
            r["error"] = f"{type(e).__name__}: {e}"[:300]
        emit(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

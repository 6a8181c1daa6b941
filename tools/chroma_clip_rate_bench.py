"""Rate-controlled clips of YUV frames of any subsampling and siting against what they replace, bt709, limited
range, linear upsampling, T = 512: HIP events, warm, the median of five medians of 20 with the sides of a pair alternating and the
spread (max - min of the five) reported, around the whole Python call for the kernel; a host clock around a synchronise for the codec.

  (i)  jobs    chroma_clip_rate.tile_distortion_jobs of 16 scattered (frame, tile) jobs over eight 2160 x 3840 frames, for "nv12" centre /
               left / topleft, "p210" left and "i444" centre at O = 0 and 32   vs   the loop of 16 single-tile
               chroma_rate.frame_tile_distortion calls it replaces, equal integers asserted on every row; and, for centre-sited "nv12",
               vs clip_rate.tile_distortion_jobs (the same work through section 17's library)
  (ii) codec   chroma_clip_rate.encode_clip_to_size with reuse on and off on section 25's 8-frame 1080p "p210" left-sited clip (one
               smooth frame with a 200 x 200 block that moves 64 pixels per frame), three levels   vs   the loop of
               chroma_rate.encode_frame_tiled_to_size with an eighth of the budget per frame: times, bytes, tiles coded and the
               per-plane SSE summed over the frames, from the plans.  Budget A is halfway between the minimum and the maximum of the
               reuse plan; where a method cannot fit it that is recorded with its minimum.  Budget B is halfway between the minimum
               and the maximum of the loop; the times are taken there.

Nothing here is a bar: the numbers are reported as measured.  The weights are synth.synthetic_state_dict's, with which times, byte
counts and exactness are meaningful and rate and distortion are not.  Prints one JSON line per measurement; --out FILE also writes them.

    python tools/chroma_clip_rate_bench.py --out profiles/chroma_clip_rate_times_mi355x.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.chroma_bench import alternating                                           # noqa: E402
from tools.chroma_clips_bench import CLIP, UNIT, with_block                          # noqa: E402  (section 25's clip)
from tools.chroma_tiles_bench import PARAMS, T, smooth_frame                         # noqa: E402
from tools.clips_bench import walled_all                                             # noqa: E402
from tools.tiles_bench import QUALITIES, model                                       # noqa: E402

H, W = 2160, 3840
K, NF = 16, 8
CASES = [("nv12", "centre"), ("nv12", "left"), ("nv12", "topleft"), ("p210", "left"), ("i444", "centre")]


def moving_block(fmt, siting, H, W, n, block=200, step=64):
    from progressivecodec_amd import chroma
    top = 1 << (chroma.FORMATS[fmt].bits - 8)
    base = smooth_frame(fmt, siting, H, W)
    return [with_block(base, fmt, 400, 100 + step * k, block, 200 * top, 80 * top, 170 * top) for k in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--skip-codec", action="store_true")
    args = ap.parse_args()
    import torch
    from progressivecodec_amd import chroma_clip_rate as cr
    from progressivecodec_amd import chroma_rate, clip_rate, tiles
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    # (i) the distortion of scattered jobs
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand((K, 3, T, T), generator=gen, device="cuda")
    for fmt, siting in CASES:
        clip = moving_block(fmt, siting, H, W, NF)
        table = [tuple(p[None] for p in f) for f in clip]
        for O in (0, 32):
            g = tiles.grid_of(H, W, T, O)
            n = g.ny * g.nx
            jobs = [(m % NF, (7 * m + 3) % n) for m in range(K)]
            new = lambda: cr.tile_distortion_jobs(x, g, clip, jobs, fmt, *PARAMS[:2], siting)                                      # noqa: E731
            old = lambda: [chroma_rate.frame_tile_distortion(x[m:m + 1], g, clip[f], fmt, *PARAMS[:2], siting, first_tile=t)       # noqa: E731
                           for m, (f, t) in enumerate(jobs)]
            r = {"what": "tile_distortion_jobs", "fmt": fmt, "siting": siting, "shape": [H, W], "tile": T, "overlap": O, "k": K, "frames": NF,
                 "jobs": jobs, "unit": UNIT + "; the new call includes the upload of its frame table and its k jobs",
                 "wide": cr.plan(x, table, fmt, overlap=O)}
            r["tile_distortion_jobs"], r["k_calls_of_frame_tile_distortion"] = alternating(new, old)
            r["ratio_loop_to_new"] = round(r["k_calls_of_frame_tile_distortion"]["median"] / r["tile_distortion_jobs"]["median"], 2)
            got, want = new(), torch.cat(old())
            assert torch.equal(got, want), (fmt, siting, O)                           # equal integers on every row
            r["equal"] = True
            emit(r)
            if (fmt, siting) == ("nv12", "centre"):
                other = lambda: clip_rate.tile_distortion_jobs(x, g, clip, jobs, fmt, *PARAMS[:2])                                 # noqa: E731
                s = {"what": "chroma_clip_rate against clip_rate, nv12 centre", "shape": [H, W], "tile": T, "overlap": O, "k": K, "unit": UNIT}
                s["chroma_clip_rate"], s["clip_rate"] = alternating(new, other)
                s["slower_by"] = round(s["chroma_clip_rate"]["median"] - s["clip_rate"]["median"], 2)
                s["within_the_two_spreads"] = s["slower_by"] <= s["chroma_clip_rate"]["spread"] + s["clip_rate"]["spread"]
                assert torch.equal(new(), other())
                s["equal"] = True
                emit(s)
        del clip, table

    # (ii) through the codec
    if not args.skip_codec:
        net = model()
        c = CLIP
        F, fmt, siting = c["frames"], c["fmt"], c["siting"]
        frames = moving_block(fmt, siting, c["H"], c["W"], F, c["block"], c["step"])
        kw = dict(siting=siting, tile=T, overlap=0)
        g = tiles.grid_of(c["H"], c["W"], T, 0)
        r = {"what": "codec, encode_clip_to_size against the loop of encode_frame_tiled_to_size", "clip": c, "tile": T, "overlap": 0,
             "tiles_per_frame": g.ny * g.nx, "qualities": QUALITIES, "unit": "s (host clock around a synchronise, warm)",
             "weights": "synthetic: times, bytes and exactness only"}
        try:
            enc = lambda target, reuse: cr.encode_clip_to_size(net, frames, QUALITIES, target, fmt, *PARAMS, reuse=reuse, **kw)          # noqa: E731
            loop = lambda target: [chroma_rate.encode_frame_tiled_to_size(net, f, QUALITIES, target // F, fmt, *PARAMS, **kw)            # noqa: E731
                                   for f in frames]
            fixed = 47 + 16 * F * g.ny * g.nx
            free = enc(10 ** 9, True)[1]
            free_all = enc(10 ** 9, False)[1]
            per_frame = [p for _, p in loop(8 * 10 ** 9)]
            lo = {"reuse": fixed + sum(min(v) for v in free.rates), "no_reuse": fixed + sum(min(v) for v in free_all.rates),
                  "loop": F * max(48 + sum(min(v) for v in p.rates) for p in per_frame)}
            hi = {"reuse": fixed + sum(max(v) for v in free.rates), "no_reuse": fixed + sum(max(v) for v in free_all.rates),
                  "loop": F * max(48 + sum(max(v) for v in p.rates) for p in per_frame)}
            r.update(minimum_bytes=lo, maximum_bytes=hi, tiles_coded_reuse=free.n_coded, tiles_coded_no_reuse=free_all.n_coded,
                     tiles_coded_loop=F * g.ny * g.nx, tiles_reused=free.n_reused, sse_exact=free.sse_exact)
            total = lambda sse: [sum(row[p] for row in sse) for p in range(3)]                                                       # noqa: E731
            for name, budget in (("budget_a_halfway_of_the_reuse_plan", (lo["reuse"] + hi["reuse"]) // 2),
                                 ("budget_b_halfway_of_the_loop", (lo["loop"] + hi["loop"]) // 2)):
                b = {"target_bytes": budget}
                for label, reuse in (("reuse", True), ("no_reuse", False)):
                    if budget < lo[label]:
                        b[label] = {"fits": False, "minimum": lo[label]}
                        continue
                    buf, plan = enc(budget, reuse)
                    b[label] = {"fits": True, "bytes": len(buf), "sse_y_cb_cr": total(plan.sse), "levels_histogram":
                                [plan.levels.count(l) for l in range(len(QUALITIES))]}
                if budget < lo["loop"]:
                    b["loop"] = {"fits": False, "minimum": lo["loop"]}
                else:
                    got = loop(budget)
                    b["loop"] = {"fits": True, "bytes": sum(len(v) for v, _ in got), "sse_y_cb_cr": total([p.sse for _, p in got]),
                                 "levels_histogram": [sum(p.levels.count(l) for _, p in got) for l in range(len(QUALITIES))]}
                r[name] = b
            budget = (lo["loop"] + hi["loop"]) // 2
            ts = walled_all(lambda: loop(budget), 5)
            r["loop_runs"], r["loop"], r["loop_spread"] = ts, statistics.median(ts), round(max(ts) - min(ts), 4)
            ts = walled_all(lambda: enc(budget, True), 5)
            r["encode_clip_to_size_reuse_runs"], r["encode_clip_to_size_reuse"] = ts, statistics.median(ts)
            r["encode_clip_to_size_no_reuse"] = statistics.median(walled_all(lambda: enc(budget, False), 3))
            r["ratio_loop_to_reuse"] = round(r["loop"] / r["encode_clip_to_size_reuse"], 2)
            r["ratio_loop_to_no_reuse"] = round(r["loop"] / r["encode_clip_to_size_no_reuse"], 3)
        except Exception as e:                                                     # a finding, recorded as such
            r["error"] = f"{type(e).__name__}: {e}"[:300]
        emit(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

"""Rate-controlled clips against what they replace, bt709, limited range, linear upsampling, T = 512: HIP events,
warm, median of 20, around the whole Python call for the kernel; a host clock around a synchronise for the codec calls.

  (i)  jobs    clip_rate.tile_distortion_jobs of k scattered (frame, tile) jobs (k = 1, 4, 16, 32) spread over min(k, 8) 2160 x 3840
               NV12 and P010 frames   vs   k calls of frame_rate.frame_tile_distortion(first_tile=t) on one tile each -- the only thing
               that replaces it today; the results compared for equality
  (ii) codec   clip_rate.encode_clip_to_size with reuse on and off on section 16's 8-frame 1080p NV12 clip (one smooth frame with a
               200 x 200 block that moves 64 pixels per frame), three levels   vs   the loop of frame_rate.encode_frame_tiled_to_size
               with an eighth of the budget per frame: times, bytes, tiles coded and the per-plane SSE summed over the frames, from
               the plans.  Budget A is halfway between the minimum and the maximum of the reuse plan; where a method cannot fit it
               (it stores every static tile eight times) that is recorded with its minimum.  Budget B is halfway between the
               minimum and the maximum of the loop, which all three fit; the times are taken there.

The bars are relative and are judged here: the jobs call must beat the loop at k = 16; encode_clip_to_size with
reuse must beat the loop by more than the loop's run-to-run spread (max - min of five runs).  The SSE comparison is a report at equal
bytes, not a bar: the weights are synth.synthetic_state_dict's, with which times, byte counts and exactness are meaningful and rate
and distortion are not.  Prints one JSON line per measurement; --out FILE also writes them all.

    python tools/clip_rate_bench.py --out profiles/clip_rate_times_mi355x.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.clips_bench import CLIP, walled_all, with_block                            # noqa: E402  (section 16's clip, one clock)
from tools.frame_tiles_bench import PARAMS, QUALITIES, T, smooth_frame                # noqa: E402
from tools.tiles_bench import model, timed                                           # noqa: E402

H, W = 2160, 3840
KS = (1, 4, 16, 32)


def moving_block(fmt, H, W, n, block=200, step=64):
    sh = 6 if fmt == "p010" else 0
    base = smooth_frame(fmt, H, W)
    return [with_block(base, 400, 100 + step * f, block, 200 << sh, 80 << sh, 170 << sh) for f in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--skip-codec", action="store_true")
    args = ap.parse_args()
    import torch
    from progressivecodec_amd import clip_rate, frame_rate, tiles
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    # (i) the distortion of scattered jobs
    g = tiles.grid_of(H, W, T, 0)
    n = g.ny * g.nx
    for fmt in ("nv12", "p010"):
        clip = moving_block(fmt, H, W, 8)
        gen = torch.Generator(device="cuda").manual_seed(1)
        tiles_all = torch.rand((max(KS), 3, T, T), generator=gen, device="cuda")
        for k in KS:
            nf = min(k, 8)
            jobs = [(m % nf, (7 * m + 3) % n) for m in range(k)]
            x = tiles_all[:k]
            new = lambda: clip_rate.tile_distortion_jobs(x, g, clip[:nf], jobs, fmt, *PARAMS[:2])                                   # noqa: E731
            old = lambda: [frame_rate.frame_tile_distortion(x[m:m + 1], g, clip[f], fmt, *PARAMS[:2], first_tile=t)                 # noqa: E731
                           for m, (f, t) in enumerate(jobs)]
            r = {"what": "tile_distortion_jobs", "fmt": fmt, "shape": [H, W], "tile": T, "overlap": 0, "k": k, "frames": nf, "jobs": jobs,
                 "unit": "us, median of 20 (HIP events, warm); the new call includes the upload of its frame table and its k jobs",
                 "wide": clip_rate.plan(x, [tuple(p[None] for p in f) for f in clip[:nf]], fmt),
                 "tile_distortion_jobs": timed(new), "k_calls_of_frame_tile_distortion": timed(old)}
            r["ratio_loop_to_new"] = round(r["k_calls_of_frame_tile_distortion"] / r["tile_distortion_jobs"], 2)
            r["equal"] = bool(torch.equal(new(), torch.cat(old())))
            if k == 16:
                r["bar_new_is_faster_at_16"] = r["tile_distortion_jobs"] < r["k_calls_of_frame_tile_distortion"]
            emit(r)
        del clip

    # (ii) through the codec
    if not args.skip_codec:
        net = model()
        c = CLIP
        F = c["frames"]
        frames = moving_block("nv12", c["H"], c["W"], F, c["block"], c["step"])
        kw = dict(tile=T, overlap=0)
        g = tiles.grid_of(c["H"], c["W"], T, 0)
        r = {"what": "codec, encode_clip_to_size against the loop of encode_frame_tiled_to_size", "fmt": "nv12", "clip": c, "tile": T,
             "overlap": 0, "tiles_per_frame": g.ny * g.nx, "qualities": QUALITIES, "unit": "s (host clock around a synchronise, warm)",
             "weights": "synthetic: times, bytes and exactness only"}
        try:
            enc = lambda target, reuse: clip_rate.encode_clip_to_size(net, frames, QUALITIES, target, "nv12", *PARAMS, reuse=reuse, **kw)     # noqa: E731
            loop = lambda target: [frame_rate.encode_frame_tiled_to_size(net, f, QUALITIES, target // F, "nv12", *PARAMS, **kw)               # noqa: E731
                                   for f in frames]
            fixed = 42 + 16 * F * g.ny * g.nx
            free = enc(10 ** 9, True)[1]
            free_all = enc(10 ** 9, False)[1]
            per_frame = [p for _, p in loop(8 * 10 ** 9)]
            lo = {"reuse": fixed + sum(min(v) for v in free.rates), "no_reuse": fixed + sum(min(v) for v in free_all.rates),
                  "loop": F * max(43 + sum(min(v) for v in p.rates) for p in per_frame)}
            hi = {"reuse": fixed + sum(max(v) for v in free.rates), "no_reuse": fixed + sum(max(v) for v in free_all.rates),
                  "loop": F * max(43 + sum(max(v) for v in p.rates) for p in per_frame)}
            r.update(minimum_bytes=lo, maximum_bytes=hi, tiles_coded_reuse=free.n_coded, tiles_coded_no_reuse=free_all.n_coded,
                     tiles_coded_loop=F * g.ny * g.nx, tiles_reused=free.n_reused)
            total = lambda sse: [sum(row[p] for row in sse) for p in range(3)]                                                       # noqa: E731
            for name, budget in (("budget_a_halfway_of_the_reuse_plan", (lo["reuse"] + hi["reuse"]) // 2),
                                 ("budget_b_halfway_of_the_loop", (lo["loop"] + hi["loop"]) // 2)):
                b = {"target_bytes": budget}
                for label, fn in (("reuse", lambda: enc(budget, True)), ("no_reuse", lambda: enc(budget, False))):
                    if budget < lo[label]:
                        b[label] = {"fits": False, "minimum": lo[label]}
                        continue
                    buf, plan = fn()
                    b[label] = {"fits": True, "bytes": len(buf), "sse_y_cb_cr": total(plan.sse), "levels_histogram":
                                [plan.levels.count(l) for l in range(len(QUALITIES))]}
                if budget < lo["loop"]:
                    b["loop"] = {"fits": False, "minimum": lo["loop"]}
                else:
                    got = loop(budget)
                    b["loop"] = {"fits": True, "bytes": sum(len(x) for x, _ in got), "sse_y_cb_cr": total([p.sse for _, p in got]),
                                 "levels_histogram": [sum(p.levels.count(l) for _, p in got) for l in range(len(QUALITIES))]}
                r[name] = b
            budget = (lo["loop"] + hi["loop"]) // 2
            ts = walled_all(lambda: loop(budget), 5)
            r["loop_runs"] = ts
            r["loop"] = statistics.median(ts)
            r["loop_spread"] = round(max(ts) - min(ts), 4)
            ts = walled_all(lambda: enc(budget, True), 5)
            r["encode_clip_to_size_reuse_runs"] = ts
            r["encode_clip_to_size_reuse"] = statistics.median(ts)
            r["encode_clip_to_size_no_reuse"] = statistics.median(walled_all(lambda: enc(budget, False), 3))
            r["ratio_loop_to_reuse"] = round(r["loop"] / r["encode_clip_to_size_reuse"], 2)
            r["ratio_loop_to_no_reuse"] = round(r["loop"] / r["encode_clip_to_size_no_reuse"], 3)
            r["bar_reuse_beats_the_loop_by_more_than_its_spread"] = r["encode_clip_to_size_reuse"] < r["loop"] - r["loop_spread"]
        except Exception as e:                                                     # a finding, recorded as such
            r["error"] = f"{type(e).__name__}: {e}"[:300]
        emit(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

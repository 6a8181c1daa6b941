"""Tolerant rate-controlled clips against what they replace, bt709, limited range, linear upsampling, T = 512:
HIP events, warm, median of 20, around the whole Python call for the kernel; a host clock around a synchronise for the codec calls.

  (i)  runs    clip_tol_rate.tile_distortion_runs of 16 scattered decoded tiles of eight 2160 x 3840 frames, NV12 and P010, O = 0 and
               32, each against a run of r = 1, 4, 8 frames   vs   the sequence it replaces, written out here: the decoded tiles
               repeated with index_select, one copy per frame of the run, and ONE clip_rate.tile_distortion_jobs over the 16 r
               (frame, tile) jobs; the results compared for equality.  Each side is the median of 20, taken five times, the two
               sides alternating: the figure is the median of the five, the spread their max - min.
  (ii) codec   section 18's noisy 8-frame 1080p NV12 clip (a moving block and a seeded 0 or +1 on every sample of every frame), three
               levels, at one target both encoders can meet:  clip_rate.encode_clip_to_size  (whose exact test must code all 96
               tiles)   vs   clip_tol_rate.encode_clip_to_size(max_abs=1): encode time, tiles coded, bytes, predicted and the SSE
               summed over the clip, five runs each.

The bars are relative and are judged here: at r = 4 and r = 8 the run call's median must lie below the replaced
sequence's by more than that sequence's spread; at r = 1 the ratio is reported whichever way it falls.  The tolerant encode must be
faster than clip_rate.encode_clip_to_size by more than that call's spread.  The weights are synth.synthetic_state_dict's: times, counts
and exactness are meaningful with them, rate and distortion are not.  Prints one JSON line per measurement; --out FILE also writes them
all.

    python tools/clip_tol_rate_bench.py --out profiles/clip_tol_rate_times_mi355x.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.clip_rate_bench import moving_block                                       # noqa: E402
from tools.clip_tol_bench import with_noise                                          # noqa: E402
from tools.clips_bench import CLIP, walled_all, with_block                           # noqa: E402  (section 16's clip, one clock)
from tools.frame_tiles_bench import PARAMS, QUALITIES, T, smooth_frame               # noqa: E402
from tools.tiles_bench import model, timed                                           # noqa: E402

H, W, FRAMES, K = 2160, 3840, 8, 16
RS = (1, 4, 8)


def five(new, old):
    """the two calls alternating, five medians of 20 each -> per call (median, max - min, the five)"""
    a, b = [], []
    for _ in range(5):
        a.append(timed(new))
        b.append(timed(old))
    return [(statistics.median(ts), round(max(ts) - min(ts), 2), ts) for ts in (a, b)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--skip-codec", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    args = ap.parse_args()
    import torch
    from progressivecodec_amd import clip_rate, clip_tol_rate, tiles
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    # (i) the distortion of runs
    for fmt in () if args.skip_kernel else ("nv12", "p010"):
        clip = moving_block(fmt, H, W, FRAMES)
        gen = torch.Generator(device="cuda").manual_seed(1)
        x = torch.rand((K, 3, T, T), generator=gen, device="cuda")
        for O in (0, 32):
            g = tiles.grid_of(H, W, T, O)
            n = g.ny * g.nx
            tile_ids = [(7 * m + 3) % n for m in range(K)]
            for r_len in RS:
                runs = [[(m + j) % FRAMES for j in range(r_len)] for m in range(K)]
                jobs = [(f, t) for t, run in zip(tile_ids, runs) for f in run]
                owner = torch.tensor([m for m, run in enumerate(runs) for _ in run], device="cuda")
                new = lambda: clip_tol_rate.tile_distortion_runs(x, g, clip, tile_ids, runs, fmt, *PARAMS[:2])[0]                  # noqa: E731
                old = lambda: clip_rate.tile_distortion_jobs(x.index_select(0, owner), g, clip, jobs, fmt, *PARAMS[:2])            # noqa: E731
                r = {"what": "tile_distortion_runs", "fmt": fmt, "shape": [H, W], "frames": FRAMES, "tile": T, "overlap": O, "tiles": K,
                     "run_length": r_len, "entries": len(jobs),
                     "unit": "us, median of 20 (HIP events, warm), taken five times: median and max - min of the five; both calls "
                             "include the upload of their frame table and their index tables",
                     "wide": clip_tol_rate.plan(x, [tuple(p[None] for p in f) for f in clip], fmt, overlap=O)}
                both = five(new, old)
                r["tile_distortion_runs"], r["tile_distortion_runs_spread"], r["tile_distortion_runs_five"] = both[0]
                r["index_select_and_tile_distortion_jobs"], r["replaced_spread"], r["replaced_five"] = both[1]
                r["ratio_replaced_to_new"] = round(r["index_select_and_tile_distortion_jobs"] / r["tile_distortion_runs"], 3)
                r["equal"] = bool(torch.equal(new(), old()))
                if r_len > 1:
                    r["bar_new_is_faster_by_more_than_the_replaced_spread"] = (
                        r["tile_distortion_runs"] < r["index_select_and_tile_distortion_jobs"] - r["replaced_spread"])
                r["counters"] = "none collected: the ratios are read from these event times alone"
                emit(r)
        del clip

    # (ii) through the codec
    if not args.skip_codec:
        net = model()
        c = CLIP
        F = c["frames"]
        base = smooth_frame("nv12", c["H"], c["W"])
        clean = [with_block(base, 400, 100 + c["step"] * f, c["block"], 200, 80, 170) for f in range(F)]
        frames = [with_noise(f, "nv12", 0, 1, 200 + k) for k, f in enumerate(clean)]
        kw = dict(tile=T, overlap=0)
        g = tiles.grid_of(c["H"], c["W"], T, 0)
        n = g.ny * g.nx
        r = {"what": "codec, clip_tol_rate.encode_clip_to_size(max_abs=1) against clip_rate.encode_clip_to_size on a noisy clip", "fmt": "nv12",
             "clip": c, "noise": "a seeded 0 or +1 on every sample's code of every frame", "tile": T, "overlap": 0, "tiles_per_frame": n,
             "qualities": QUALITIES, "unit": "s (host clock around a synchronise, warm)", "weights": "synthetic: times, counts and exactness only"}
        try:
            tol = clip_tol_rate.Tolerance(1)
            enc_exact = lambda target: clip_rate.encode_clip_to_size(net, frames, QUALITIES, target, "nv12", *PARAMS, **kw)                 # noqa: E731
            enc_tol = lambda target: clip_tol_rate.encode_clip_to_size(net, frames, QUALITIES, target, "nv12", *PARAMS, tolerance=tol, **kw)  # noqa: E731
            fixed = 42 + 16 * F * n
            free_exact, free_tol = enc_exact(10 ** 9)[1], enc_tol(10 ** 9)[1]
            lo = {"exact": fixed + sum(min(v) for v in free_exact.rates), "tolerant": fixed + sum(min(v) for v in free_tol.rates)}
            hi = {"exact": fixed + sum(max(v) for v in free_exact.rates), "tolerant": fixed + sum(max(v) for v in free_tol.rates)}
            target = max((lo["exact"] + hi["exact"]) // 2, lo["tolerant"])           # both can meet it: lo["tolerant"] <= lo["exact"]
            r.update(minimum_bytes=lo, maximum_bytes=hi, target_bytes=target, tiles_in_all=F * n)
            total = lambda sse: [sum(row[p] for row in sse) for p in range(3)]                                                    # noqa: E731
            for label, fn in (("exact", enc_exact), ("tolerant", enc_tol)):
                buf, plan = fn(target)
                ts = walled_all(lambda: fn(target), 5)
                r[label] = {"tiles_coded": plan.n_coded, "bytes": len(buf), "fits": len(buf) <= target, "predicted": plan.predicted,
                            "sse_y_cb_cr": total(plan.sse), "levels_histogram": [plan.levels.count(l) for l in range(len(QUALITIES))],
                            "encode_runs": ts, "encode": statistics.median(ts), "encode_spread": round(max(ts) - min(ts), 4)}
                if label == "tolerant":
                    r[label].update(worst=plan.worst, entries=sum(len(run) for run in plan.runs),
                                    longest_run=max(len(run) for run in plan.runs))
                    r["decodes"] = len(clip_rate.decode_clip(net, buf)) == F
            r["ratio_encode"] = round(r["exact"]["encode"] / r["tolerant"]["encode"], 2)
            r["bar_tolerant_is_faster_by_more_than_the_exact_spread"] = r["tolerant"]["encode"] < r["exact"]["encode"] - r["exact"]["encode_spread"]
            r["sse_note"] = ("the tolerant plan's sse is the decoded clip's true SSE against the frames shown, reused tiles included; the "
                             "exact plan codes every tile from its own frame")
        except Exception as e:                                                     # a finding, recorded as such
            r["error"] = f"{type(e).__name__}: {e}"[:300]
        emit(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

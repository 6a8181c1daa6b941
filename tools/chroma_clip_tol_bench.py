"""Tolerant clips of YUV frames of any subsampling and siting against what they replace, bt709, limited range,
linear upsampling, T = 512: HIP events, warm, the median of five medians of 20 with the arms of a comparison alternating in one
process and the spread (max - min of the five) reported; a host clock around a synchronise for the codec calls.

  (i)  scan    chroma_clip_tol.scan_clip(max_abs=1) on eight 2160 x 3840 frames, O = 0 and 32, "nv12" at each siting, "p210" left and
               "i444" centre -- section 18's clip: one smooth frame, a 200 x 200 block that moves 64 pixels per frame, and seeded noise
               of one code on every sample of frames 1 .. 7   vs
     (a) torch_sequence  the torch sequence below, which is what a user would write today: per frame, per tile and plane, the
                         footprint of the frame and of the tile's anchor frame gathered, their difference, three reductions, the
                         decision on the device, and ONE host synchronisation per frame to learn the anchors the next frame is
                         gathered by; source and stats compared with the scan's, on every row
     (b) clip_changes    chroma_clips.clip_changes on the same clip: the same loads and one launch pair per frame, too, but the
                         exact-only test of section 25 against the PREVIOUS frame (three counts instead of nine numbers, no decision)
     (c) clip_tol        for centre-sited "nv12", clip_tol.scan_clip: section 18's scan, the same work
  (ii) codec   section 25's 8-frame 1080p "p210" left-sited moving-block clip with a seeded dither of one code (0 or +1) on every
               sample of every frame:  chroma_clips.encode_clip  vs  chroma_clip_tol.encode_clip(max_abs=1): times (median of 5),
               bytes, tiles coded, decode time, plan.worst, the run-to-run spread beside every difference

The tool asserts the exactness flags, not the times.  The weights are synth.synthetic_state_dict's: times, byte counts and exactness
are meaningful with them, rate and distortion are not.  Prints one JSON line per measurement; --out FILE also writes them all.

    python tools/chroma_clip_tol_bench.py --out profiles/chroma_clip_tol_times_mi355x.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.chroma_bench import alternating                                          # noqa: E402
from tools.chroma_clips_bench import CLIP, QUALITIES, footprints, with_block        # noqa: E402  (section 25's clip)
from tools.chroma_tiles_bench import CASES, PARAMS, T, smooth_frame                 # noqa: E402
from tools.clips_bench import walled_all                                            # noqa: E402
from tools.tiles_bench import model                                                 # noqa: E402

H, W, FRAMES = 2160, 3840, 8
UNIT = "us, median of 20 (HIP events, warm), taken five times, the arms alternating: median and max - min of the five"


def _codes(p, f):
    import torch
    v = (p.view(torch.int16).to(torch.int32) & 0xFFFF) if p.dtype == torch.uint16 else p.to(torch.int32)
    return (v >> f.shift) & ((1 << f.bits) - 1)


def with_noise(planes, fmt, lo, hi, seed):
    """a copy of a frame with a seeded integer in [lo, hi] added to every sample's code (the codes of the frames used here lie well
    inside the code range)"""
    import torch
    from progressivecodec_amd import chroma
    f = chroma.FORMATS[fmt]
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for p in planes:
        v = (_codes(p, f) + torch.randint(lo, hi + 1, p.shape, generator=g, device="cuda", dtype=torch.int32)) << f.shift
        out.append(v.to(torch.int16).view(torch.uint16) if p.dtype == torch.uint16 else v.to(torch.uint8))
    return tuple(out)


def codes_of(frames, fmt):
    """the clip's code planes as int32 [F,H,W], [F,Hc,Wc], [F,Hc,Wc]"""
    import torch
    from progressivecodec_amd import chroma
    f = chroma.FORMATS[fmt]
    y = torch.stack([_codes(fr[0], f) for fr in frames])
    if f.layout == chroma.SEMIPLANAR:
        uv = torch.stack([_codes(fr[1], f) for fr in frames])
        return y, uv[..., 0].contiguous(), uv[..., 1].contiguous()
    return y, torch.stack([_codes(fr[1], f) for fr in frames]), torch.stack([_codes(fr[2], f) for fr in frames])


def torch_scan(frames, fmt, rects, max_abs):
    """the sequence chroma_clip_tol.scan_clip replaces -> (source [F][n], stats int64 [F,n,3,3]): max_abs only, no MSE condition, no
    max_run"""
    import torch
    planes = codes_of(frames, fmt)
    n, F = len(rects), len(frames)
    anchor = [0] * n
    source = [[0] * n]
    stats = [torch.zeros((n, 3, 3), dtype=torch.int64, device="cuda")]
    for k in range(1, F):
        rows = []
        for t, (lu, ch) in enumerate(rects):
            for p, r in ((0, lu), (1, ch), (2, ch)):
                d = (planes[p][k, r[0]:r[1], r[2]:r[3]] - planes[p][anchor[t], r[0]:r[1], r[2]:r[3]]).abs()
                rows.append(torch.stack([(d != 0).sum(), (d.to(torch.int64) * d).sum(), d.max().to(torch.int64)]))
        st = torch.stack(rows).view(n, 3, 3)
        reuse = (st[:, :, 2] <= max_abs).all(dim=1).tolist()                         # the host synchronisation of the frame
        anchor = [a if r else k for a, r in zip(anchor, reuse)]
        source.append(list(anchor))
        stats.append(st)
    return source, torch.stack(stats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--size", type=int, nargs=2, default=[H, W])
    ap.add_argument("--skip-codec", action="store_true")
    args = ap.parse_args()
    import torch
    from progressivecodec_amd import chroma, clip_tol, clips, tiles
    from progressivecodec_amd import chroma_clip_tol as ct
    from progressivecodec_amd import chroma_clips as kc
    Hh, Ww = args.size
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    # (i) the scan
    tol = ct.Tolerance(1)
    for fmt, siting in CASES:
        f = chroma.FORMATS[fmt]
        top = 1 << (f.bits - 8)
        base = smooth_frame(fmt, siting, Hh, Ww)
        frames = [with_block(base, fmt, 600, 1000 + 64 * k, 200, 180 * top, 90 * top, 160 * top) for k in range(FRAMES)]
        frames = [frames[0]] + [with_noise(fr, fmt, -1, 1, 100 + k) for k, fr in enumerate(frames[1:])]
        for O in (0, 32):
            g = tiles.grid_of(Hh, Ww, T, O)
            rects = footprints(g, fmt, siting)
            call = lambda: ct.scan_clip(frames, fmt, tol, siting, T, O, PARAMS[2])            # noqa: E731
            seq = lambda: torch_scan(frames, fmt, rects, 1)                                   # noqa: E731
            exact = lambda: kc.clip_changes(frames, fmt, siting, T, O, PARAMS[2])             # noqa: E731
            r = {"what": "scan_clip", "fmt": fmt, "siting": siting, "shape": [Hh, Ww], "frames": FRAMES, "tile": T, "overlap": O,
                 "tiles": [g.ny, g.nx], "upsample": PARAMS[2], "tolerance": list(tol),
                 "unit": UNIT + "; scan_clip includes the upload of its frame table",
                 "wide": ct.plan([tuple(p[None] for p in fr) for fr in frames], fmt, overlap=O)}
            arms = [call, seq, exact]
            if (fmt, siting) == ("nv12", "centre"):
                arms.append(lambda: clip_tol.scan_clip(frames, fmt, tol, T, O, PARAMS[2]))
            times = alternating(*arms)
            r["scan_clip"], r["torch_sequence"], r["clip_changes"] = times[:3]
            r["ratio_torch_to_scan"] = round(r["torch_sequence"]["median"] / r["scan_clip"]["median"], 1)
            r["ratio_scan_to_clip_changes"] = round(r["scan_clip"]["median"] / r["clip_changes"]["median"], 3)
            source, stats = call()
            want_source, want_stats = seq()
            r["source_equals_torch"] = source.tolist() == want_source
            r["stats_equal_torch"] = bool(torch.equal(stats, want_stats))
            r["tiles_coded"] = int(sum(s == k for k, row in enumerate(source.tolist()) for s in row))
            exact_source = clips.source_table((exact() != 0).any(dim=2).tolist())
            r["tiles_coded_by_the_exact_test"] = int(sum(s == k for k, row in enumerate(exact_source) for s in row))
            if len(times) == 4:
                r["clip_tol_scan_clip"] = times[3]
                a, b = r["scan_clip"], times[3]
                r["slower_than_clip_tol_by"] = round(a["median"] - b["median"], 2)
                r["within_the_larger_spread"] = a["median"] - b["median"] <= max(a["spread"], b["spread"])
                s18 = clip_tol.scan_clip(frames, fmt, tol, T, O, PARAMS[2])
                r["equals_clip_tol"] = bool(torch.equal(source, s18[0]) and torch.equal(stats, s18[1]))
                assert r["equals_clip_tol"], r
            r["counters"] = "none collected: the ratios are read from these event times alone"
            emit(r)
            assert r["source_equals_torch"] and r["stats_equal_torch"], r

    # (ii) through the codec
    if not args.skip_codec:
        net = model()
        c = CLIP
        fmt, siting = c["fmt"], c["siting"]
        base = smooth_frame(fmt, siting, c["H"], c["W"])
        clean = [with_block(base, fmt, 400, 100 + c["step"] * k, c["block"], 800, 320, 680) for k in range(c["frames"])]
        frames = [with_noise(fr, fmt, 0, 1, 200 + k) for k, fr in enumerate(clean)]
        kw = dict(siting=siting, tile=T, overlap=0)
        g = tiles.grid_of(c["H"], c["W"], T, 0)
        n = g.ny * g.nx
        r = {"what": "codec, chroma_clip_tol.encode_clip(max_abs=1) against chroma_clips.encode_clip on a noisy clip", "clip": c,
             "noise": "a seeded 0 or +1 on every sample's code of every frame", "tile": T, "overlap": 0, "tiles_per_frame": n,
             "qualities": QUALITIES, "unit": "s (host clock around a synchronise, warm), median of 5", "weights": "synthetic: times, bytes and exactness only"}
        enc_exact = lambda: kc.encode_clip(net, frames, QUALITIES, fmt, *PARAMS, **kw)                                        # noqa: E731
        enc_tol = lambda: ct.encode_clip(net, frames, QUALITIES, fmt, *PARAMS, tolerance=ct.Tolerance(1), **kw)               # noqa: E731
        _, plan_clean = kc.encode_clip(net, clean, QUALITIES, fmt, *PARAMS, **kw)
        exact, plan_exact = enc_exact()
        buf, plan = enc_tol()
        r.update(tiles_in_all=c["frames"] * n, tiles_coded_noise_free=plan_clean.n_coded, tiles_coded_exact=plan_exact.n_coded,
                 tiles_coded_tolerant=plan.n_coded, bytes_exact=len(exact), bytes_tolerant=len(buf), worst=plan.worst,
                 coded_per_frame=[sum(s == k for s in row) for k, row in enumerate(plan.source)])
        r["exact_codes_every_tile"] = plan_exact.n_coded == c["frames"] * n
        r["tolerant_codes_the_noise_free_tiles"] = plan.source == plan_clean.source
        every, _ = kc.encode_clip(net, frames, QUALITIES, fmt, *PARAMS, reuse=False, **kw)
        hd = kc.parse_clip(every)
        blobs = [[kc.clip_tile_bytes(every, hd, k, t)[0] for t in range(n)] for k in range(c["frames"])]
        r["container_is_the_selected_blobs"] = buf == kc.pack_clip(blobs, plan.source, c["H"], c["W"], T, 0, fmt, *PARAMS, siting)
        for name, fn in (("encode_exact", enc_exact), ("encode_tolerant", enc_tol)):
            ts = walled_all(fn, 5)
            r[name + "_runs"], r[name], r[name + "_spread"] = ts, statistics.median(ts), round(max(ts) - min(ts), 4)
        r["faster_by_more_than_the_spread"] = r["encode_tolerant"] < r["encode_exact"] - max(r["encode_exact_spread"], r["encode_tolerant_spread"])
        r["smaller"] = len(buf) < len(exact)
        r["ratio_encode"] = round(r["encode_exact"] / r["encode_tolerant"], 2)
        r["ratio_bytes"] = round(len(exact) / len(buf), 2)
        for name, b in (("decode_exact", exact), ("decode_tolerant", buf)):
            ts = walled_all(lambda: kc.decode_clip(net, b), 5)
            r[name + "_runs"], r[name], r[name + "_spread"] = ts, statistics.median(ts), round(max(ts) - min(ts), 4)
        r["ratio_decode"] = round(r["decode_exact"] / r["decode_tolerant"], 2)
        emit(r)
        assert r["tolerant_codes_the_noise_free_tiles"] and r["container_is_the_selected_blobs"] and r["worst"] == [1, 1, 1], r
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

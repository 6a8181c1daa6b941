"""Tolerant clips against what they replace, bt709, limited range, linear upsampling, T = 512: HIP events, warm,
median of 20 for the scan; a host clock around a synchronise for the codec calls.

  (i)  scan    clip_tol.scan_clip(max_abs=1) on eight 2160 x 3840 frames, NV12 and P010, O = 0 and 32 -- one smooth frame, a 200 x 200
               block that moves 64 pixels per frame, and seeded noise of one code on every sample of frames 1 .. 7   vs
     (a) torch_sequence  the torch sequence below, which is what stands in for the scan without it: per frame, per tile and plane,
                         the footprint of the frame and of the tile's anchor frame gathered, their difference, three reductions, the
                         decision on the device, and ONE host synchronisation to learn the anchors the next frame is gathered by;
                         source and stats compared with the scan's, all of them
     (b) clip_changes    clips.clip_changes on the same clip in the same run: the same loads and one launch pair per frame, too, but
                         the exact-only test of section 16 against the PREVIOUS frame (three counts instead of nine numbers, no decision)
  (ii) codec   section 16's 8-frame 1080p moving-block NV12 clip with a seeded dither of one code (0 or +1) on every sample of every
               frame, so that two frames of a static tile never differ by more than one code:  clips.encode_clip  (which must code
               all 96 tiles of it)   vs   clip_tol.encode_clip(max_abs=1)  (which must code the 34 of the noise-free clip): times,
               bytes, tiles coded, decode time, plan.worst

The bars are relative and are judged here: the scan must beat the torch sequence with identical source and
stats; the tolerant encode must be faster than clips.encode_clip on the same noisy clip by more than that call's run-to-run spread
(max - min of its runs) observed here, and smaller in bytes.  The ratio to clip_changes is reported, not gated.  The weights are
synth.synthetic_state_dict's: times, byte counts and exactness are meaningful with them, rate and distortion are not.  Prints one
JSON line per measurement; --out FILE also writes them all.

    python tools/clip_tol_bench.py --out profiles/clip_tol_times_mi355x.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.clips_bench import CLIP, footprints, walled_all, with_block              # noqa: E402  (section 16's clip, one clock)
from tools.frame_tiles_bench import PARAMS, QUALITIES, T, smooth_frame             # noqa: E402
from tools.tiles_bench import model, timed                                         # noqa: E402

H, W, FRAMES = 2160, 3840, 8


def with_noise(planes, fmt, lo, hi, seed):
    """a copy of an NV12 / P010 frame with a seeded integer in [lo, hi] added to every sample's code (the codes of the frames used
    here lie well inside the code range)"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    sh = 6 if fmt == "p010" else 0
    out = []
    for p in planes:
        v = (p.view(torch.int16).to(torch.int32) & 0xFFFF) if p.dtype == torch.uint16 else p.to(torch.int32)
        v = ((v >> sh) + torch.randint(lo, hi + 1, p.shape, generator=g, device="cuda", dtype=torch.int32)) << sh
        out.append(v.to(torch.int16).view(torch.uint16) if p.dtype == torch.uint16 else v.to(torch.uint8))
    return tuple(out)


def codes_of(frames, fmt):
    """the clip's code planes as int32 [F,H,W], [F,Hc,Wc], [F,Hc,Wc]"""
    import torch
    sh = 6 if fmt == "p010" else 0
    wide = lambda p: ((p.view(torch.int16).to(torch.int32) & 0xFFFF) if p.dtype == torch.uint16 else p.to(torch.int32)) >> sh   # noqa: E731
    y = torch.stack([wide(f[0]) for f in frames])
    uv = torch.stack([wide(f[1]) for f in frames])
    return y, uv[..., 0].contiguous(), uv[..., 1].contiguous()


def torch_scan(frames, fmt, rects, max_abs):
    """the sequence clip_tol.scan_clip replaces -> (source [F][n], stats int64 [F,n,3,3]): max_abs only, no MSE condition, no max_run"""
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
    ap.add_argument("--skip-codec", action="store_true")
    args = ap.parse_args()
    import torch
    from progressivecodec_amd import clip_tol, clips, tiles
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    # (i) the scan
    tol = clip_tol.Tolerance(1)
    for fmt in ("nv12", "p010"):
        es, sh = (2, 6) if fmt == "p010" else (1, 0)
        base = smooth_frame(fmt, H, W)
        frames = [with_block(base, 600, 1000 + 64 * k, 200, 180 << sh, 90 << sh, 160 << sh) for k in range(FRAMES)]
        frames = [frames[0]] + [with_noise(f, fmt, -1, 1, 100 + k) for k, f in enumerate(frames[1:])]
        for O in (0, 32):
            g = tiles.grid_of(H, W, T, O)
            rects = footprints(g, 1)
            nbytes = 2 * (FRAMES - 1) * es * (H * W + H * W // 2)                   # per step the frame and the anchors' footprints: about two frames
            call = lambda: clip_tol.scan_clip(frames, fmt, tol, T, O, PARAMS[2])    # noqa: E731
            seq = lambda: torch_scan(frames, fmt, rects, 1)                         # noqa: E731
            exact = lambda: clips.clip_changes(frames, fmt, T, O, PARAMS[2])        # noqa: E731
            r = {"what": "scan_clip", "fmt": fmt, "shape": [H, W], "frames": FRAMES, "tile": T, "overlap": O, "tiles": [g.ny, g.nx],
                 "upsample": PARAMS[2], "tolerance": list(tol), "unit": "us, median of 20 (HIP events, warm); scan_clip includes the upload of its frame table",
                 "wide": clip_tol.plan([tuple(p[None] for p in f) for f in frames], fmt, overlap=O),
                 "scan_clip": timed(call), "clip_changes": timed(exact), "torch_sequence": timed(seq, n=5, warm=1),
                 "torch_sequence_runs": "median of 5, one warm-up", "bytes_read_nominal": nbytes}
            r["tb_per_s_nominal"] = round(nbytes / r["scan_clip"] / 1e6, 3)
            r["ratio_torch_to_scan"] = round(r["torch_sequence"] / r["scan_clip"], 1)
            r["ratio_scan_to_clip_changes"] = round(r["scan_clip"] / r["clip_changes"], 3)
            r["beats_torch"] = r["scan_clip"] < r["torch_sequence"]
            source, stats = call()
            want_source, want_stats = seq()
            r["source_equals_torch"] = source.tolist() == want_source
            r["stats_equal_torch"] = bool(torch.equal(stats, want_stats))
            r["tiles_coded"] = int(sum(s == k for k, row in enumerate(source.tolist()) for s in row))
            exact_source = clips.source_table((exact() != 0).any(dim=2).tolist())
            r["tiles_coded_by_the_exact_test"] = int(sum(s == k for k, row in enumerate(exact_source) for s in row))
            r["counters"] = "none collected: the ratios are read from these event times alone"
            emit(r)

    # (ii) through the codec
    if not args.skip_codec:
        net = model()
        c = CLIP
        base = smooth_frame("nv12", c["H"], c["W"])
        clean = [with_block(base, 400, 100 + c["step"] * f, c["block"], 200, 80, 170) for f in range(c["frames"])]
        frames = [with_noise(f, "nv12", 0, 1, 200 + k) for k, f in enumerate(clean)]
        kw = dict(tile=T, overlap=0)
        g = tiles.grid_of(c["H"], c["W"], T, 0)
        n = g.ny * g.nx
        r = {"what": "codec, clip_tol.encode_clip(max_abs=1) against clips.encode_clip on a noisy clip", "fmt": "nv12", "clip": c,
             "noise": "a seeded 0 or +1 on every sample's code of every frame", "tile": T, "overlap": 0, "tiles_per_frame": n,
             "qualities": QUALITIES, "unit": "s (host clock around a synchronise, warm)", "weights": "synthetic: times, bytes and exactness only"}
        try:
            enc_exact = lambda: clips.encode_clip(net, frames, QUALITIES, "nv12", *PARAMS, **kw)                                  # noqa: E731
            enc_tol = lambda: clip_tol.encode_clip(net, frames, QUALITIES, "nv12", *PARAMS, tolerance=clip_tol.Tolerance(1), **kw)   # noqa: E731
            _, plan_clean = clips.encode_clip(net, clean, QUALITIES, "nv12", *PARAMS, **kw)
            exact, plan_exact = enc_exact()
            buf, plan = enc_tol()
            r.update(tiles_in_all=c["frames"] * n, tiles_coded_noise_free=plan_clean.n_coded, tiles_coded_exact=plan_exact.n_coded,
                     tiles_coded_tolerant=plan.n_coded, bytes_exact=len(exact), bytes_tolerant=len(buf), worst=plan.worst,
                     coded_per_frame=[sum(s == f for s in row) for f, row in enumerate(plan.source)])
            r["exact_codes_every_tile"] = plan_exact.n_coded == c["frames"] * n
            r["tolerant_codes_the_noise_free_tiles"] = plan.source == plan_clean.source
            every, _ = clips.encode_clip(net, frames, QUALITIES, "nv12", *PARAMS, reuse=False, **kw)
            hd = clips.parse_clip(every)
            blobs = [[clips.clip_tile_bytes(every, hd, f, t)[0] for t in range(n)] for f in range(c["frames"])]
            r["container_is_the_selected_blobs"] = buf == clips.pack_clip(blobs, plan.source, c["H"], c["W"], T, 0, "nv12", *PARAMS)
            ts = walled_all(enc_exact, 5)
            r["encode_exact_runs"] = ts
            r["encode_exact"] = statistics.median(ts)
            r["encode_exact_spread"] = round(max(ts) - min(ts), 4)
            ts = walled_all(enc_tol, 5)
            r["encode_tolerant_runs"] = ts
            r["encode_tolerant"] = statistics.median(ts)
            r["faster_by_more_than_the_spread"] = r["encode_tolerant"] < r["encode_exact"] - r["encode_exact_spread"]
            r["smaller"] = len(buf) < len(exact)
            r["ratio_encode"] = round(r["encode_exact"] / r["encode_tolerant"], 2)
            r["ratio_bytes"] = round(len(exact) / len(buf), 2)
            r["decode_exact"] = statistics.median(walled_all(lambda: clips.decode_clip(net, exact), 3))
            r["decode_tolerant"] = statistics.median(walled_all(lambda: clips.decode_clip(net, buf), 3))
            r["ratio_decode"] = round(r["decode_exact"] / r["decode_tolerant"], 2)
        except Exception as e:                                                     # a finding, recorded as such
            r["error"] = f"{type(e).__name__}: {e}"[:300]
        emit(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

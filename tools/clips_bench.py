"""Clips of YUV 4:2:0 frames against what they replace, bt709, limited range, linear upsampling, T = 512: HIP
events, warm, median of 20 for the kernels; a host clock around a synchronise for the codec calls.

  (i)   tile_changes   clips.tile_changes(cur, prev, fmt) on a 2160 x 3840 NV12 and P010 frame pair, O = 0 and 32   vs
     (a) torch_sequence  the torch sequence below: per plane the codes' `!=`, then per tile the sums over the footprint rectangles
     (b) copy            a plain device copy (dst.copy_(src)) of the bytes the call must read: both frames, once
  (ii)  cut_tiles      clips.cut_tiles of k scattered tiles (k = 1, 4, 16) of the 2160p NV12 frame   vs   k calls of
                       frame_tiles.cut_frame(rect=(ty, tx, 1, 1)); both results compared bit for bit
  (iii) codec          clips.encode_clip / decode_clip with reuse on and off on an 8-frame 1080p NV12 clip -- one smooth frame with a
                       200 x 200 block that moves 64 pixels per frame --   vs   the loop of frame_tiles.encode_frame_tiled /
                       decode_frame_tiled over the same frames: times, bytes, tiles coded, and the exactness of every frame

The bars are relative and are judged here: tile_changes must beat the torch sequence; encode_clip(reuse=False)
must not be slower than the loop of encode_frame_tiled beyond the run-to-run spread (max - min of the loop's runs) this tool observes
and records.  The weights are synth.synthetic_state_dict's: times, byte counts and exactness are meaningful with them, rate and
distortion are not.  Prints one JSON line per measurement; --out FILE also writes them all.

    python tools/clips_bench.py --out profiles/clips_times_mi355x.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.frame_tiles_bench import HBM_PEAK, PARAMS, QUALITIES, T, smooth_frame      # noqa: E402  (one frame, one clock)
from tools.tiles_bench import model, timed                                           # noqa: E402

H, W = 2160, 3840
CLIP = dict(H=1080, W=1920, frames=8, block=200, step=64)


def footprints(g, halo):
    """per tile (luma (y0, y1, x0, x1), chroma (y0, y1, x0, x1)), half-open: clips.py's footprint, restated"""
    def axis(i, L):
        e = min(i * g.S + g.T, L)
        return (i * g.S, e), (max(i * g.S // 2 - halo, 0), min(-(-e // 2) - 1 + halo, -(-L // 2) - 1) + 1)
    out = []
    for i in range(g.ny):
        for j in range(g.nx):
            (ly, cy), (lx, cx) = axis(i, g.H), axis(j, g.W)
            out.append((ly + lx, cy + cx))
    return out


def torch_tile_changes(cur, prev, fmt, rects):
    """the sequence clips.tile_changes replaces -> int64 [n,3]: the planes' codes compared, then one sum per tile and plane"""
    import torch
    if fmt == "p010":
        code = lambda t: t.to(torch.int32) >> 6                                      # noqa: E731
        dy, duv = code(cur[0]) != code(prev[0]), code(cur[1]) != code(prev[1])
    else:
        dy, duv = cur[0] != prev[0], cur[1] != prev[1]
    out = []
    for lu, ch in rects:
        c = duv[ch[0]:ch[1], ch[2]:ch[3]]
        out.append(torch.stack([dy[lu[0]:lu[1], lu[2]:lu[3]].sum(), c[..., 0].sum(), c[..., 1].sum()]))
    return torch.stack(out)


def with_block(planes, y, x, size, luma, cb, cr):
    """a copy of an NV12 / P010 frame with a size x size block (y, x and size even) of flat colour"""
    import torch
    out = tuple(p.clone() for p in planes)
    yv, cv = (p.view(torch.int16) if p.dtype == torch.uint16 else p for p in out)   # the values fit 15 bits
    yv[y:y + size, x:x + size] = luma
    cv[y // 2:(y + size) // 2, x // 2:(x + size) // 2, 0] = cb
    cv[y // 2:(y + size) // 2, x // 2:(x + size) // 2, 1] = cr
    return out


def walled_all(fn, n, warm=1):
    """seconds of n runs, a host clock around work that ends in a synchronise"""
    import torch
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(round(time.perf_counter() - t0, 4))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--skip-codec", action="store_true")
    args = ap.parse_args()
    import torch
    from progressivecodec_amd import clips, frame_tiles, tiles
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    # (i) which tiles changed
    for fmt in ("nv12", "p010"):
        es, sh = (2, 6) if fmt == "p010" else (1, 0)
        prev = smooth_frame(fmt, H, W)
        cur = with_block(prev, 600, 1000, 200, 180 << sh, 90 << sh, 160 << sh)
        for O in (0, 32):
            g = tiles.grid_of(H, W, T, O)
            rects = footprints(g, 1)
            nbytes = 2 * es * (H * W + H * W // 2)
            a = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
            b = torch.empty_like(a)
            call = lambda: clips.tile_changes(cur, prev, fmt, T, O, PARAMS[2])      # noqa: E731
            seq = lambda: torch_tile_changes(cur, prev, fmt, rects)                 # noqa: E731
            r = {"what": "tile_changes", "fmt": fmt, "shape": [H, W], "tile": T, "overlap": O, "tiles": [g.ny, g.nx], "upsample": PARAMS[2],
                 "unit": "us, median of 20 (HIP events, warm)",
                 "wide": clips.plan(clips.CHANGES, tuple(p[None] for p in cur), fmt, other=tuple(p[None] for p in prev), overlap=O),
                 "tile_changes": timed(call), "torch_sequence": timed(seq), "copy_of_the_bytes": timed(lambda: b.copy_(a)), "bytes": nbytes}
            r["tb_per_s"] = round(nbytes / r["tile_changes"] / 1e6, 3)
            r["copy_tb_per_s"] = round(nbytes / r["copy_of_the_bytes"] / 1e6, 3)
            r["fraction_of_hbm_peak"] = round(nbytes / (r["tile_changes"] * 1e-6) / HBM_PEAK, 4)
            r["ratio_to_copy"] = round(r["tile_changes"] / r["copy_of_the_bytes"], 2)
            r["ratio_torch_to_new"] = round(r["torch_sequence"] / r["tile_changes"], 1)
            r["beats_torch"] = r["tile_changes"] < r["torch_sequence"]
            got = call()
            r["equals_torch"] = bool(torch.equal(got, seq()))
            r["tiles_changed"] = int((got != 0).any(1).sum())
            emit(r)
            del a, b

    # (ii) the cut of scattered tiles
    planes = smooth_frame("nv12", H, W)
    for O in (0, 32):
        g = tiles.grid_of(H, W, T, O)
        scattered = [(7 * m + 3) % (g.ny * g.nx) for m in range(16)]
        for k in (1, 4, 16):
            idx = scattered[:k]
            out = torch.empty((k, 3, T, T), dtype=torch.float32, device="cuda")
            new = lambda: clips.cut_tiles(planes, "nv12", idx, *PARAMS, tile=T, overlap=O, out=out)                          # noqa: E731
            old = lambda: [frame_tiles.cut_frame(planes, "nv12", *PARAMS, tile=T, overlap=O, rect=(t // g.nx, t % g.nx, 1, 1))[0]   # noqa: E731
                           for t in idx]
            r = {"what": "cut_tiles", "fmt": "nv12", "shape": [H, W], "tile": T, "overlap": O, "k": k, "tile_indices": idx,
                 "unit": "us, median of 20 (HIP events, warm); cut_tiles includes the upload of its k indices",
                 "wide": clips.plan(clips.CUT, tuple(p[None] for p in planes), "nv12", f32=out, overlap=O),
                 "cut_tiles": timed(new), "k_calls_of_cut_frame": timed(old)}
            r["ratio_loop_to_new"] = round(r["k_calls_of_cut_frame"] / r["cut_tiles"], 2)
            r["same_bits"] = bool(torch.equal(new().view(torch.int32), torch.cat(old()).view(torch.int32)))
            emit(r)

    # (iii) through the codec
    if not args.skip_codec:
        net = model()
        c = CLIP
        base = smooth_frame("nv12", c["H"], c["W"])
        frames = [with_block(base, 400, 100 + c["step"] * f, c["block"], 200, 80, 170) for f in range(c["frames"])]
        kw = dict(tile=T, overlap=0)
        g = tiles.grid_of(c["H"], c["W"], T, 0)
        r = {"what": "codec, encode_clip / decode_clip against the loop of encode_frame_tiled / decode_frame_tiled", "fmt": "nv12",
             "clip": c, "tile": T, "overlap": 0, "tiles_per_frame": g.ny * g.nx, "qualities": QUALITIES,
             "unit": "s (host clock around a synchronise, warm)", "weights": "synthetic: times, bytes and exactness only"}
        try:
            loop_enc = lambda: [frame_tiles.encode_frame_tiled(net, f, QUALITIES, "nv12", *PARAMS, **kw) for f in frames]          # noqa: E731
            enc = lambda reuse: clips.encode_clip(net, frames, QUALITIES, "nv12", *PARAMS, reuse=reuse, **kw)                      # noqa: E731
            alone = loop_enc()
            buf, plan = enc(True)
            every, plan_all = enc(False)
            r["frame_containers_equal_the_loop"] = all(clips.frame_container(buf, f) == alone[f] == clips.frame_container(every, f)
                                                       for f in range(c["frames"]))
            r.update(loop_bytes=sum(map(len, alone)), clip_bytes_reuse=len(buf), clip_bytes_no_reuse=len(every),
                     tiles_coded_reuse=plan.n_coded, tiles_coded_no_reuse=plan_all.n_coded, tiles_reused=plan.n_reused,
                     coded_per_frame=[sum(s == f for s in row) for f, row in enumerate(plan.source)])
            ts = walled_all(loop_enc, 5)
            r["loop_encode_runs"] = ts
            r["loop_encode"] = statistics.median(ts)
            r["loop_encode_spread"] = round(max(ts) - min(ts), 4)
            ts = walled_all(lambda: enc(False), 5)
            r["encode_clip_no_reuse_runs"] = ts
            r["encode_clip_no_reuse"] = statistics.median(ts)
            r["encode_clip_reuse"] = statistics.median(walled_all(lambda: enc(True), 3))
            r["no_reuse_not_slower_than_loop_beyond_spread"] = r["encode_clip_no_reuse"] <= r["loop_encode"] + r["loop_encode_spread"]
            r["ratio_loop_to_no_reuse"] = round(r["loop_encode"] / r["encode_clip_no_reuse"], 3)
            r["ratio_loop_to_reuse"] = round(r["loop_encode"] / r["encode_clip_reuse"], 2)
            loop_dec = lambda: [frame_tiles.decode_frame_tiled(net, b) for b in alone]                                             # noqa: E731
            want = loop_dec()
            same = lambda got: all(torch.equal(x, y) for a, b in zip(got, want) for x, y in zip(a, b))                             # noqa: E731
            r["decoded_frames_equal_the_loop"] = same(clips.decode_clip(net, buf)) and same(clips.decode_clip(net, every))
            r["loop_decode"] = statistics.median(walled_all(loop_dec, 3))
            r["decode_clip_reuse"] = statistics.median(walled_all(lambda: clips.decode_clip(net, buf), 3))
            r["decode_clip_no_reuse"] = statistics.median(walled_all(lambda: clips.decode_clip(net, every), 3))
            r["ratio_loop_decode_to_reuse"] = round(r["loop_decode"] / r["decode_clip_reuse"], 2)
        except Exception as e:                                                     # a finding, recorded as such
            r["error"] = f"{type(e).__name__}: {e}"[:300]
        emit(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

"""Tiled coding of YUV 4:2:0 frames against the two-step sequences it replaces: HIP events, warm, median of 20,
one 1080p and one 2160p NV12 frame and one 2160p P010 frame, T = 512, O = 0 and 32, bt709, limited range, linear upsampling.

  cut               frame_tiles.cut_frame(planes, fmt)            vs  frames.to_model_input, then torch: crop the padding, F.pad to the
                                                                      grid, unfold / permute / contiguous into [n,3,T,T]
  stitch            frame_tiles.stitch_frame(x_hat_tiles, grid)   vs  torch: clamp, per-band weights, one weighted add per tile into a
                                                                      float frame; then frames.from_model_output of that frame
  stitch with sums  ... (ref=planes), device only                 vs  the same with ref=planes
  copy              dst.copy_(src) of a byte buffer with the same traffic (bytes read + bytes written = the bytes the call must move:
                    planes in + tiles out; the tiles where they cover the frame (bands twice) in + planes out, + the reference planes)
  separate calls    frames.to_model_input / from_model_output of the whole frame and tiles.cut / tiles.stitch of a uint8 RGB image of
                    the same size, each on its own: what the project offered before, neither of which does the whole job
  codec             fresh processes (the codec library's own allocations are invisible to torch's allocator: the drop in free
                    device memory around the call, torch.cuda.mem_get_info): encode_frame_tiled with max_tiles_per_call = 8 against
                    frames.encode_frame of the same 2160p frame; decode_frame_tiled of a 512 x 512 region against the whole frame

The torch halves are what a user would write, not a restatement: the weighted adds are not fused, so codes may differ by one (the
count is reported).  The weights are synth.synthetic_state_dict's: times and memory are meaningful with them, rate and distortion are
not.  Prints one JSON line per measurement; --out FILE also writes them all.

    python tools/frame_tiles_bench.py --out profiles/frame_tiles_times_mi355x.json
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.tiles_bench import model, timed, torch_weights, walled      # noqa: E402

HBM_PEAK = 8.0e12
T = 512
QUALITIES = [0, 0.5, 10]
REGION = (824, 1664, 512, 512)                     # the 2160p frame's centre: it straddles tile edges, as a viewer's window would
PARAMS = ("bt709", "limited", "linear")


def smooth_frame(fmt, H, W):
    """a smooth in-gamut picture: low-resolution noise enlarged, emitted once by the frames layer itself -> planes without a batch axis"""
    import torch
    import torch.nn.functional as F
    from progressivecodec_amd import frames
    g = torch.Generator(device="cuda").manual_seed(H)
    lo = torch.rand((1, 3, H // 40, W // 40), generator=g, device="cuda") * 0.8 + 0.1
    rgb = F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False)
    return tuple(p[0] for p in frames.from_model_output(rgb, frames.Geometry(H, W, H, W, 0, 0), fmt))


def two_step_cut(planes, fmt, g):
    """what a user would write today: the whole-frame ingest, then torch slicing and padding into tiles"""
    import torch.nn.functional as F
    from progressivecodec_amd import frames
    x, geom = frames.to_model_input(planes, fmt, *PARAMS)
    S = g.S
    Hg, Wg = (g.ny - 1) * S + g.T, (g.nx - 1) * S + g.T
    x = F.pad(x[0, :, geom.top:geom.top + g.H, geom.left:geom.left + g.W], (0, Wg - g.W, 0, Hg - g.H))
    t = x.unfold(1, g.T, S).unfold(2, g.T, S)                              # [3, ny, nx, T, T]
    return t.permute(1, 2, 0, 3, 4).reshape(g.n, 3, g.T, g.T).contiguous()


def two_step_stitch(x_tiles, g, wy, wx, fmt, ref=None):
    """what a user would write today: a torch blend of the tiles into a float frame, then the whole-frame emit"""
    import torch
    from progressivecodec_amd import frames
    S = g.S
    Hg, Wg = (g.ny - 1) * S + g.T, (g.nx - 1) * S + g.T
    c = x_tiles.clamp(0, 1).view(g.ny, g.nx, 3, g.T, g.T)
    c = c * (wy[:, None, None, :, None] * wx[None, :, None, None, :])
    acc = torch.zeros((1, 3, Hg, Wg), dtype=torch.float32, device=x_tiles.device)
    for i in range(g.ny):
        for j in range(g.nx):
            acc[0, :, i * S:i * S + g.T, j * S:j * S + g.T] += c[i, j]
    return frames.from_model_output(acc, frames.Geometry(g.H, g.W, Hg, Wg, 0, 0), fmt, PARAMS[0], PARAMS[1], ref=ref)


def child(mode, path, fmt, H, W):
    """one codec call in a fresh process: its time and the drop in free device memory around it"""
    import torch
    from progressivecodec_amd import frame_tiles, frames
    net = model()
    planes = smooth_frame(fmt, H, W)
    buf = open(path, "rb").read() if path else None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    free0 = torch.cuda.mem_get_info(0)[0]
    t0 = time.perf_counter()
    if mode == "encode_tiled":
        out = frame_tiles.encode_frame_tiled(net, planes, QUALITIES, fmt, *PARAMS, tile=T, overlap=32, max_tiles_per_call=8)
    elif mode == "encode_whole":
        out = frames.encode_frame(net, planes, QUALITIES, fmt, *PARAMS)
    elif mode == "decode_tiled":
        out = frame_tiles.decode_frame_tiled(net, buf, max_tiles_per_call=8)
    else:
        out = frame_tiles.decode_frame_tiled(net, buf, region=REGION, max_tiles_per_call=8)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    free1 = torch.cuda.mem_get_info(0)[0]
    print(json.dumps({"mode": mode, "first_call_seconds": round(dt, 4), "free_memory_drop_mib": round((free0 - free1) / 2 ** 20, 1),
                      "torch_peak_above_start_mib": round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1),
                      "result": len(out) if isinstance(out, bytes) else [list(p.shape) for p in out]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--child")
    ap.add_argument("--file")
    ap.add_argument("--skip-codec", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.file, "nv12", 2160, 3840)
    import torch
    from progressivecodec_amd import frame_tiles, frames, tiles
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
    for fmt, H, W in [("nv12", 1080, 1920), ("nv12", 2160, 3840), ("p010", 2160, 3840)]:
        es = 2 if fmt == "p010" else 1
        planes = smooth_frame(fmt, H, W)
        batched = tuple(p[None] for p in planes)
        plane_bytes = es * (H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2))
        geom = frames.padding(H, W)
        rgb8 = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda")
        x_frame = torch.rand((1, 3, geom.Hp, geom.Wp), device="cuda")
        for O in (0, 32):
            g = tiles.grid_of(H, W, T, O)
            x, _ = frame_tiles.cut_frame(planes, fmt, *PARAMS, tile=T, overlap=O)
            gen = torch.Generator(device="cuda").manual_seed(O)
            x_hat = (x + 0.02 * torch.randn(x.shape, generator=gen, device="cuda")).contiguous()
            wy, wx = torch_weights(g, "cuda")
            cut_bytes = plane_bytes + 4 * x.numel()
            st_bytes = 12 * (H + (g.ny - 1) * O) * (W + (g.nx - 1) * O) + plane_bytes       # the tiles where they cover the frame (bands twice)
            out = frame_tiles.stitch_frame(x_hat, g, fmt, *PARAMS[:2])
            r = {"what": "kernels", "fmt": fmt, "shape": [H, W], "tile": T, "overlap": O, "tiles": [g.ny, g.nx], "matrix": PARAMS[0],
                 "range": PARAMS[1], "upsample": PARAMS[2], "unit": "us, median of 20 (HIP events, warm)",
                 "wide_cut": frame_tiles.plan(frame_tiles.CUT, batched, fmt, x, overlap=O),
                 "wide_stitch": frame_tiles.plan(frame_tiles.STITCH, tuple(p[None] for p in out), fmt, x_hat, ref=batched),
                 "cut": timed(lambda: frame_tiles.cut_frame(planes, fmt, *PARAMS, tile=T, overlap=O)),
                 "two_step_cut": timed(lambda: two_step_cut(planes, fmt, g)),
                 "copy_cut_traffic": copy_of(cut_bytes),
                 "stitch": timed(lambda: frame_tiles.stitch_frame(x_hat, g, fmt, *PARAMS[:2])),
                 "two_step_stitch": timed(lambda: two_step_stitch(x_hat, g, wy, wx, fmt)),
                 "copy_stitch_traffic": copy_of(st_bytes),
                 "stitch_with_sums_device_only": timed(lambda: frame_tiles.stitch_frame(x_hat, g, fmt, *PARAMS[:2], ref=planes)),
                 "sums_only_device_only": timed(lambda: frame_tiles.stitch_frame(x_hat, g, fmt, *PARAMS[:2], ref=planes, image=False)),
                 "two_step_stitch_with_sums_device_only": timed(lambda: two_step_stitch(x_hat, g, wy, wx, fmt, ref=planes)),
                 "copy_stitch_with_sums_traffic": copy_of(st_bytes + plane_bytes),
                 # the separate calls the project had before, each on its own (neither does the whole job)
                 "frames_to_model_input": timed(lambda: frames.to_model_input(planes, fmt, *PARAMS)),
                 "frames_from_model_output": timed(lambda: frames.from_model_output(x_frame, geom, fmt, *PARAMS[:2])),
                 "tiles_cut_u8_rgb": timed(lambda: tiles.cut(rgb8, T, O)),
                 "tiles_stitch_u8_rgb": timed(lambda: tiles.stitch(x_hat, g)),
                 "cut_bytes": cut_bytes, "stitch_bytes": st_bytes, "stitch_with_sums_bytes": st_bytes + plane_bytes}
            r["cut_fraction_of_hbm_peak"] = round(cut_bytes / (r["cut"] * 1e-6) / HBM_PEAK, 4)
            r["stitch_fraction_of_hbm_peak"] = round(st_bytes / (r["stitch"] * 1e-6) / HBM_PEAK, 4)
            r["stitch_with_sums_fraction_of_hbm_peak"] = round((st_bytes + plane_bytes) / (r["stitch_with_sums_device_only"] * 1e-6) / HBM_PEAK, 4)
            r["cut_equals_two_step"] = bool(torch.equal(x, two_step_cut(planes, fmt, g)))
            old = two_step_stitch(x_hat, g, wy, wx, fmt)
            r["stitch_codes_that_differ_from_two_step"] = int(sum((codes(a) != codes(b[0])).sum() for a, b in zip(out, old)))
            r["stitch_max_code_difference_from_two_step"] = int(max((codes(a) - codes(b[0])).abs().max() for a, b in zip(out, old))) >> (6 if es == 2 else 0)
            emit(r)
    if not args.skip_codec:
        fmt, H, W = "nv12", 2160, 3840
        with tempfile.TemporaryDirectory() as tmp:
            net = model()
            planes = smooth_frame(fmt, H, W)
            r = {"what": "codec, 2160p NV12, tile 512, overlap 32, max_tiles_per_call 8", "qualities": QUALITIES,
                 "unit": "s, median of 3 (host clock around a synchronise, warm)", "weights": "synthetic: times only", "region": list(REGION)}
            path = os.path.join(tmp, "pcg1")
            try:
                buf = frame_tiles.encode_frame_tiled(net, planes, QUALITIES, fmt, *PARAMS, tile=T, overlap=32, max_tiles_per_call=8)
                with open(path, "wb") as f:
                    f.write(buf)
                r["bytes"] = len(buf)
                r["encode_frame_tiled"] = walled(lambda: frame_tiles.encode_frame_tiled(net, planes, QUALITIES, fmt, *PARAMS, tile=T, overlap=32, max_tiles_per_call=8))
                r["decode_frame_tiled"] = walled(lambda: frame_tiles.decode_frame_tiled(net, buf, max_tiles_per_call=8))
                r["decode_frame_tiled_region_512"] = walled(lambda: frame_tiles.decode_frame_tiled(net, buf, region=REGION, max_tiles_per_call=8))
            except Exception as e:                                             # a finding, recorded as such
                r["error"] = f"{type(e).__name__}: {e}"[:300]
            emit(r)
            del net
            torch.cuda.empty_cache()
            for mode in ("encode_tiled", "encode_whole", "decode_tiled", "decode_region"):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", mode] + (["--file", path] if mode.startswith("decode") else [])
                try:
                    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
                except subprocess.TimeoutExpired:
                    emit({"mode": mode, "what": "fresh process: one call", "error": "no result within 300 s"})
                    break                                                      # nothing more is started on the device after a hang
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
                c = json.loads(line[-1]) if p.returncode == 0 and line else {"mode": mode, "returncode": p.returncode, "error": (p.stderr or p.stdout)[-300:]}
                c["what"] = "fresh process: one call"
                emit(c)
                if p.returncode < 0 or p.returncode in (134, 139):
                    break                                                      # nor after a process that died of a signal
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

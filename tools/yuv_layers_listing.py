"""What the six YUV modules compute and call, as text: frames / frame_tiles / frame_rate and chroma / chroma_tiles / chroma_rate (DESIGN.md
section 26).  The public API alone, so the same file runs against two trees -- each in a fresh process -- and `diff` of the two
listings says whether the Python layers of one compute and call what the other's do.

One 100 x 150 frame per case, tile 64, overlap 0 and 16, qualities [0.05, 0.5, 2], max_tiles_per_call 4, synthetic weights; "nv12",
"i420" and "p010" through the 4:2:0 stack, "nv12" centre, "nv12" topleft, "p210" left and "i444" centre through the chroma stack.
Every public function of the six modules is called; every line is the SHA-256 of a container or of decoded planes, the repr of a plan
or of another small result, the sequence of model calls (method, batch, qualities) or the sequence of C entry points with their
integer and float arguments (no pointers, no workspace sizes in bytes, no stream), recorded by a proxy over each module's `lib`.

    python tools/yuv_layers_listing.py --out listing.txt
    python tools/yuv_layers_listing.py --small-calls        # host dispatch: 1000 back-to-back calls, one synchronise, wall time

--small-calls prints one JSON line: per call the median of five batches of 1000, in microseconds per call, on one 64 x 64 "nv12" frame
with T = 64: frames.to_model_input, chroma_tiles.cut_frame, chroma_rate.frame_tile_distortion.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, T = 100, 150, 64
QUALITIES = [0.05, 0.5, 2]
STEP = 4
YUV420 = ["nv12", "i420", "p010"]
SITED = [("nv12", "centre"), ("nv12", "topleft"), ("p210", "left"), ("i444", "centre")]
_VALUES = (C.c_int, C.c_int64, C.c_float)               # argument types that are listed; pointers, c_size_t and the stream are not


class Lib:
    """a library whose calls are listed"""

    def __init__(self, real, calls):
        self._real, self._calls = real, calls

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args):
            self._calls.append(f"{name}({', '.join(repr(a) for a, t in zip(args, fn.argtypes) if t in _VALUES)})")
            return fn(*args)
        return call


class Model:
    """a model whose calls are listed"""

    def __init__(self, real, calls):
        self._real, self._calls = real, calls

    def __getattr__(self, name):
        return getattr(self._real, name)

    def compress_levels(self, x, qualities, **kw):
        self._calls.append(f"compress_levels({x.shape[0]}, {list(qualities)})")
        return self._real.compress_levels(x, qualities, **kw)

    def decompress_levels(self, strings, shape, qualities, mask_pol):
        self._calls.append(f"decompress_levels({len(strings[0][1])}, {list(qualities)})")
        return self._real.decompress_levels(strings, shape, qualities, mask_pol)

    def decompress(self, strings, shape, quality, mask_pol):
        self._calls.append(f"decompress({len(strings[1])}, {quality})")
        return self._real.decompress(strings, shape, quality, mask_pol)


def sha(*things):
    import torch
    h = hashlib.sha256()
    for t in things:
        h.update(t.contiguous().cpu().numpy().tobytes() if torch.is_tensor(t) else bytes(t))
    return h.hexdigest()


def frame_of(fmt, h, w, seed=0):
    """a smooth frame of `fmt` on the device: codes inside the limited range, 10-bit codes where the format holds them"""
    import torch
    from progressivecodec_amd import chroma
    f = chroma.FORMATS[fmt]
    hc, wc = chroma.chroma_size(h, w, fmt)
    g = torch.Generator().manual_seed(seed)

    def plane(ph, pw, lo, span):
        low = torch.rand(1, 1, max(ph // 8, 2), max(pw // 8, 2), generator=g)
        v = torch.nn.functional.interpolate(low, size=(ph, pw), mode="bilinear", align_corners=False)[0, 0]
        code = (v * span + lo).round().to(torch.int32) << (f.bits - 8)
        return (code << f.shift).to(torch.uint16 if f.bits == 10 else torch.uint8)
    y, u, v = plane(h, w, 16, 219), plane(hc, wc, 16, 224), plane(hc, wc, 16, 224)
    planes = (y, u, v) if f.layout == chroma.PLANAR else (y, torch.stack([u, v], -1))
    return tuple(p.cuda() for p in planes)


def model():
    from progressivecodec_amd import ChannelProgresssiveWACNN
    from progressivecodec_amd.synth import synthetic_state_dict
    net = ChannelProgresssiveWACNN(device="cuda:0")
    net.load_state_dict(synthetic_state_dict())
    net.update()
    return net


def listing():
    import torch
    from progressivecodec_amd import chroma, chroma_rate, chroma_tiles, frame_rate, frame_tiles, frames, tiles
    calls, lines = [], []
    for mod in (frames, frame_tiles, frame_rate, chroma, chroma_tiles, chroma_rate):
        mod.lib = (lambda proxy: lambda: proxy)(Lib(mod.lib(), calls))
    net = Model(model(), calls)

    def say(case, what, *values):
        lines.append(f"{case} {what}: " + " ".join(str(v) for v in values))
        for kind, pick in (("model calls", lambda c: not c.startswith("pc_")), ("C calls", lambda c: c.startswith("pc_"))):
            if any(pick(c) for c in calls):
                lines.append(f"{case} {what} {kind}: " + "; ".join(c for c in calls if pick(c)))
        del calls[:]

    def head(hd):
        return {k: (sha(v) if isinstance(v, bytes) else v) for k, v in hd.items() if k not in ("pcb1", "tiled")}

    for F, FT, FR, fmt, siting in [(frames, frame_tiles, frame_rate, f, None) for f in YUV420] + \
                                  [(chroma, chroma_tiles, chroma_rate, f, s) for f, s in SITED]:
        s = () if siting is None else (siting,)                                  # the stack's siting argument, where it has one
        other = ("p010" if fmt != "p010" else "nv12",) if siting is None else (("nv12", "left") if (fmt, siting) != ("nv12", "left") else ("i444", "centre"))
        case = f"{F.__name__.rsplit('.', 1)[1]} {fmt}" + (f" {siting}" if siting else "")
        planes = frame_of(fmt, H, W)
        batched = tuple(p.unsqueeze(0) for p in planes)
        say(case, "constants", F.bits_of(fmt), F.chroma_size(H, W, *(() if siting is None else (fmt,))), frames.levels(fmt, "limited") if siting is None else "",
            frames.coefficients("bt709"), [tuple(t.shape) for t in F.empty_frame(fmt, 2, 5, 7, "cuda:0")])
        x, geom = F.to_model_input(planes, fmt, "bt709", "limited", "linear", *s)
        say(case, "to_model_input", sha(x), geom)
        out, dist = F.from_model_output(x, geom, fmt, "bt709", "limited", *s, ref=batched)
        say(case, "from_model_output", sha(*out), dist.sse.tolist(), dist.psnr_y(), dist.psnr_cb(), dist.psnr_cr())
        say(case, "from_model_output sums alone", F.from_model_output(x, geom, fmt, "bt601", "full", *s, ref=batched, image=False).sse.tolist())
        say(case, "plan", F.plan(F.INGEST, batched, fmt, x, geom), F.plan(F.EMIT, out, fmt, x, geom, ref=batched), F.plan(F.EMIT, None, fmt, x, geom, ref=batched))
        buf = F.encode_frame(net, planes, QUALITIES, fmt, "bt709", "limited", "linear", *s)
        hd = F.parse_frame(buf)
        say(case, "encode_frame", len(buf), sha(buf), head(hd))
        say(case, "pack_frame", sha(F.pack_frame(hd["blob"], fmt, "bt2020", "full", "nearest", *s, H, W)))
        say(case, "decode_frame", sha(*F.decode_frame(net, buf)), sha(*F.decode_frame(net, buf, 0, *other)))
        for O in (0, 16):
            at = f"O={O}"
            region = (32, T - O, 40, 52)                                          # x0 on a tile origin
            xt, g = FT.cut_frame(planes, fmt, "bt709", "limited", "linear", *s, T, O)
            part, gp = FT.cut_frame(planes, fmt, "bt601", "full", "nearest", *s, tile=T, overlap=O, rect=(0, 1, 2, 2))
            say(case, f"{at} cut_frame", sha(xt), g, sha(part), gp)
            out, dist = FT.stitch_frame(xt, g, fmt, "bt709", "limited", *s, ref=planes)
            say(case, f"{at} stitch_frame", sha(*out), dist.sse.tolist(), dist.psnr_cb())
            win, dist = FT.stitch_frame(xt, g, fmt, "bt709", "limited", *s, window=region, ref=planes)
            say(case, f"{at} stitch_frame window", sha(*win), dist.sse.tolist(), FT.stitch_frame(xt, g, fmt, "bt709", "limited", *s, window=region, ref=planes, image=False).sse.tolist())
            say(case, f"{at} windows", [FT.admissible(w, H, W, *(() if siting is None else (fmt,))) for w in ((0, 0, H, W), region, (1, 2, 4, 4), (2, 3, 4, 4), (96, 148, 3, 2))],
                *([chroma_tiles.halo_window(region, fmt, siting), chroma_tiles.covering(g, region, fmt, siting), chroma_rate.sse_exact(g, fmt, siting)] if siting else [g.covering(region)]))
            say(case, f"{at} tiled plan", FT.plan(FT.CUT, batched, fmt, xt, O), FT.plan(FT.STITCH, tuple(p.unsqueeze(0) for p in win), fmt, xt, O, region[1]),
                FR.plan(xt, batched, fmt, O))
            buf = FT.encode_frame_tiled(net, planes, QUALITIES, fmt, "bt709", "limited", "linear", *s, tile=T, overlap=O, max_tiles_per_call=STEP)
            hd = FT.parse_frame_tiled(buf)
            say(case, f"{at} encode_frame_tiled", len(buf), sha(buf), head(hd))
            say(case, f"{at} pack_frame_tiled", sha(FT.pack_frame_tiled(hd["inner"], fmt, "bt601", "full", "nearest", *s)))
            say(case, f"{at} decode_frame_tiled", sha(*FT.decode_frame_tiled(net, buf, max_tiles_per_call=STEP)))
            say(case, f"{at} decode_frame_tiled region", sha(*FT.decode_frame_tiled(net, buf, 1, region, max_tiles_per_call=STEP)))
            say(case, f"{at} decode_frame_tiled region as {other}", sha(*FT.decode_frame_tiled(net, buf, 0, region, *other, max_tiles_per_call=STEP)))
            say(case, f"{at} frame_tile_distortion", FR.frame_tile_distortion(xt.flip(0), g, planes, fmt, "bt709", "limited", *s).tolist(),
                FR.frame_tile_distortion(xt[1:4] * 0.5, g, planes, fmt, "bt601", "full", *s, first_tile=1).tolist())
            _, top = FR.encode_frame_tiled_to_size(net, planes, QUALITIES, 1 << 30, fmt, "bt709", "limited", "linear", *s, tile=T, overlap=O, max_tiles_per_call=STEP)
            fixed = FT.HEADER_BYTES + tiles.HEADER_BYTES
            budget = fixed + (sum(min(r) for r in top.rates) + sum(max(r) for r in top.rates)) // 2
            say(case, f"{at} encode_frame_tiled_to_size unbounded", top)
            buf, plan = FR.encode_frame_tiled_to_size(net, planes, QUALITIES, budget, fmt, "bt709", "limited", "linear", *s, tile=T, overlap=O,
                                                      plane_weights=(4, 1, 1), importance=[[1, 2, 1], [1, 1, 3]], max_tiles_per_call=STEP)
            say(case, f"{at} encode_frame_tiled_to_size {budget}", len(buf), sha(buf), plan)
            say(case, f"{at} decode_frame_tiled of it", sha(*FT.decode_frame_tiled(net, buf, region=region, max_tiles_per_call=STEP)))
    torch.cuda.synchronize()
    return lines


def small_calls(n=1000, batches=5):
    import torch
    from progressivecodec_amd import chroma_rate, chroma_tiles, frames
    planes = frame_of("nv12", 64, 64)
    xt, g = chroma_tiles.cut_frame(planes, "nv12", tile=T)
    cases = {"frames.to_model_input": lambda: frames.to_model_input(planes, "nv12"),
             "chroma_tiles.cut_frame": lambda: chroma_tiles.cut_frame(planes, "nv12", tile=T),
             "chroma_rate.frame_tile_distortion": lambda: chroma_rate.frame_tile_distortion(xt, g, planes, "nv12")}
    out = {}
    for name, fn in cases.items():
        times = []
        for _ in range(batches + 1):                                             # the first batch warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / n * 1e6)
        out[name] = {"us_per_call": round(sorted(times[1:])[batches // 2], 3), "batches": [round(t, 3) for t in times[1:]]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small-calls", action="store_true")
    a = ap.parse_args()
    if a.small_calls:
        print(json.dumps(small_calls()))
        return
    text = "\n".join(listing()) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()

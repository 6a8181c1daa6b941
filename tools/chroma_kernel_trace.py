"""Kernel times of the chroma layer beside `frames`' on the same 2160 x 3840 NV12 frame: what
tools/chroma_bench.py cannot show, because its figures are whole Python calls.  Two steps, the trace in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o chroma -- python tools/chroma_kernel_trace.py
    python tools/chroma_kernel_trace.py --fold OUT/chroma_kernel_trace.csv --out profiles/chroma_kernel_times_mi355x.json

The first runs, 200 times: chroma (centre) ingest, emit, emit with sums; the same three of frames; then chroma "left" and "topleft".
The second (no GPU needed) folds the dispatch trace: per kernel the median duration after the first tenth of its dispatches; the
chroma kernels that serve two or three sitings are split by the order of the calls above.
"""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUNDS = 200
H, W = 2160, 3840


def run():
    import torch
    import torch.nn.functional as F
    from progressivecodec_amd import chroma, frames
    from progressivecodec_amd.harness import compute_padding
    g = torch.Generator(device="cuda").manual_seed(H)
    lo = torch.rand((1, 3, H // 40, W // 40), generator=g, device="cuda") * 0.8 + 0.1
    geom = chroma.padding(H, W)
    pad, _ = compute_padding(H, W, 64)
    rgb = F.pad(F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False), pad)
    planes = frames.from_model_output(rgb, geom, "nv12")
    x_hat = (rgb + 0.02 * torch.randn(rgb.shape, generator=g, device="cuda")).contiguous()
    for _ in range(ROUNDS):
        for mod in (chroma, frames):
            mod.to_model_input(planes, "nv12")
            mod.from_model_output(x_hat, geom, "nv12")
            mod.from_model_output(x_hat, geom, "nv12", ref=planes)
        for siting in ("left", "topleft"):
            chroma.to_model_input(planes, "nv12", siting=siting)
            chroma.from_model_output(x_hat, geom, "nv12", siting=siting)
            chroma.from_model_output(x_hat, geom, "nv12", siting=siting, ref=planes)
    torch.cuda.synchronize()


def fold(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    seq = {}
    for r in rows:
        n = r["Kernel_Name"]
        if "emit_kernel" in n or "ingest_kernel" in n:
            key = n[:n.index(">(") + 1].replace("(anonymous namespace)::", "").replace("void ", "")
            seq.setdefault(key, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    out = {"unit": "us, median kernel duration of a rocprofv3 kernel trace, the first tenth of each kernel's dispatches dropped; one run",
           "shape": [H, W], "fmt": "nv12", "kernels": {}}
    for key, v in seq.items():
        # chroma's kernels carry SX, SY = 2, 2 in their names; the ingest serves all three sitings, the two-row emit centre and
        # left, the three-row emit topleft alone; frames' kernels have one caller (and one dispatch more, which made the frame)
        labels = {3: ("centre", "left", "topleft"), 2: ("centre", "left"), 1: ("topleft",)}[len(v) // ROUNDS] if ", 2, 2, " in key else ("frames",)
        v = v[len(v) % ROUNDS:]
        n = len(v) // 10 // len(labels) * len(labels)
        out["kernels"][key] = {s: round(statistics.median(v[n:][i::len(labels)]) / 1e3, 2) for i, s in enumerate(labels)}
        out["kernels"][key]["dispatches"] = len(v)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fold")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not args.fold:
        return run()
    r = fold(args.fold)
    print(json.dumps(r, indent=1))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(r, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()

"""The gfx950 device code of the four chroma libraries (chroma, chroma_tiles, chroma_rate, chroma_clips), kernel by kernel, as hashes:
DESIGN.md section 27.  Needs hipcc and llvm-objdump, no GPU.  Each library's .hip is compiled for the device alone with lib.mk's
FLAGS and -Rpass-analysis=kernel-resource-usage; per kernel the listing holds the SHA-256 of its disassembly (instructions alone:
no addresses, no encodings) and its resource line.  The same file runs against two trees, and --compare says which kernels differ.

    python tools/chroma_items_listing.py --tree PARENT --out parent.json
    python tools/chroma_items_listing.py --out branch.json
    python tools/chroma_items_listing.py --compare parent.json branch.json --out profiles/chroma_items_ab.json

It hashes and compares, nothing else.
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBS = {"chroma": "chroma_hip", "chroma_tiles": "chroma_tiles_hip", "chroma_rate": "chroma_rate_hip", "chroma_clips": "chroma_clips_kernels"}
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/llvm/bin/llvm-objdump")
RESOURCES = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
             "LDS Size [bytes/block]")


def plain(symbol):
    """a kernel's name without the suffix the compiler gives an unnamed-namespace symbol per translation unit"""
    return re.sub(r"(\.intern\.|__intern__)[0-9a-f]+", "", symbol)


def flags_of(tree):
    mk = open(os.path.join(tree, "progressivecodec_amd", "image_csrc", "lib.mk")).read()
    return re.search(r"^FLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split()


def kernels_of(tree, lib, tmp):
    pkg = os.path.join(tree, "progressivecodec_amd")
    obj = os.path.join(tmp, lib + ".co")
    cmd = [HIPCC] + flags_of(tree) + ["-I" + os.path.join(tree, "include"), "-I" + os.path.join(pkg, "image_csrc"), "--cuda-device-only",
                                     "--no-gpu-bundle-output", "-Rpass-analysis=kernel-resource-usage", "-c",
                                     os.path.join(pkg, LIBS[lib], "pc_%s.hip" % lib), "-o", obj]
    remarks = subprocess.run(cmd, check=True, stderr=subprocess.PIPE, text=True).stderr
    warnings = [ln for ln in remarks.splitlines() if " warning: " in ln]
    resources, name = {}, None
    for ln in remarks.splitlines():
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = plain(m.group(2))
            resources[name] = {}
        elif m.group(1) in RESOURCES:
            resources[name][m.group(1)] = int(m.group(2))
    text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", obj], check=True, stdout=subprocess.PIPE, text=True).stdout
    out, name = {}, None
    for ln in text.splitlines():
        m = re.match(r"<(\S+)>:$", ln)
        if m:
            name = plain(m.group(1))
            out[name] = []
        elif name is not None and ln.strip():
            out[name].append(re.sub(r"\s+", " ", ln.split("//")[0]).strip())
    kernels = {}
    for name, lines in out.items():
        if name in resources:                                                     # kernels alone: every other symbol has no resource line
            kernels[name] = {"instructions": len(lines), "sha256": hashlib.sha256("\n".join(lines).encode()).hexdigest(), **resources[name]}
    assert set(kernels) == set(resources), sorted(set(resources) - set(kernels))
    return kernels, warnings


def listing(tree):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for lib in LIBS:
            kernels, warnings = kernels_of(tree, lib, tmp)
            out[lib] = {"kernels": kernels, "warnings": warnings}
    return out


def compare(a, b):
    out = {"libraries": {}, "identical": True}
    for lib in LIBS:
        ka, kb = a[lib]["kernels"], b[lib]["kernels"]
        differing = sorted(n for n in set(ka) | set(kb) if ka.get(n) != kb.get(n))
        out["libraries"][lib] = {"kernels": len(kb), "differing": {n: {"parent": ka.get(n), "branch": kb.get(n)} for n in differing},
                                 "warnings": {"parent": a[lib]["warnings"], "branch": b[lib]["warnings"]},
                                 "per_kernel": {n: {"parent": ka[n], "branch": kb[n]} for n in sorted(ka) if n in kb}}
        out["identical"] = out["identical"] and not differing
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--compare", nargs=2, metavar=("PARENT", "BRANCH"))
    ap.add_argument("--out")
    a = ap.parse_args()
    result = compare(*(json.load(open(p)) for p in a.compare)) if a.compare else listing(a.tree)
    text = json.dumps(result, indent=1, sort_keys=True) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    if a.compare:
        for lib, r in result["libraries"].items():
            print("%-13s %3d kernels, %d differ" % (lib, r["kernels"], len(r["differing"])), file=sys.stderr)
        sys.exit(0 if result["identical"] else 1)


if __name__ == "__main__":
    main()

"""The structure of the image-side libraries (progressivecodec_amd/*_csrc, image_csrc/): ten libraries, each linked on
its own, that share headers and one build rule instead of restating them.  Runs on the CPU; reads sources only."""
import glob
import os
import re

from tests import image_shared
from tests.image_shared import LIBS, PKG

# what a definition of each shared name looks like
DEFINITIONS = {
    "load4": r"\bvoid load4\(",
    "struct Planes": r"\bstruct Planes\b",
    "struct Levels": r"\bstruct Levels\b",
    "to_rgb": r"\bvoid to_rgb\(",
    "frame_ok": r"\bbool frame_ok\(",
    "geo_of": r"\bbool geo_of\(",
    "axis_tiles": r"\bint64_t axis_tiles\(",
    "define HIPCHK": r"#\s*define HIPCHK\b",
    # image_csrc/pc_chroma_items.h: what the libraries of the twelve formats share
    "ingest_item": r"\bvoid ingest_item\(",
    "struct Taps": r"\bstruct Taps \{\s*int\b",           # the ingest's integer weights; pc_metrics.hip's Taps is a window of floats
    "code_of": r"\bunsigned code_of\(",
    "word_of": r"\bunsigned word_of\(",
    "struct Fmt": r"\bstruct Fmt\b",
    "format_of": r"\bbool format_of\(",
    "with_format": r"\bvoid with_format\(",
    "axis_taps": r"\bvoid axis_taps\(",
    "picture_ok": r"\bbool picture_ok\(",
    "site_ok": r"\bbool site_ok\(",
    "depth_levels": r"\bbool depth_levels\(",
}

YUV_LIBS = {"frames": "PC_FRAMES", "frame_tiles": "PC_FT", "frame_rate": "PC_FR", "clips": "PC_CL", "clip_rate": "PC_CR", "clip_tol": "PC_CT"}


def _code(path):
    txt = open(path).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def test_shared_names_are_defined_once_under_image_csrc():
    shared = {p: _code(p) for p in glob.glob(os.path.join(PKG, "image_csrc", "*.h"))}
    sources = sorted(glob.glob(os.path.join(PKG, "*_csrc", "*.hip")))
    assert len(sources) == len(LIBS) == 10 and not glob.glob(os.path.join(PKG, "image_csrc", "*.hip"))
    # every library's source: the ten, and the later ones whose directories the pins of the ten do not count
    later = sorted(glob.glob(os.path.join(PKG, "*_hip", "*.hip"))) + sorted(glob.glob(os.path.join(PKG, "chroma_clips_kernels", "*.hip")))
    assert [os.path.basename(p) for p in later] == ["pc_chroma.hip", "pc_chroma_rate.hip", "pc_chroma_tiles.hip", "pc_clip_tol_rate.hip",
                                                    "pc_chroma_clips.hip"]
    for name, pattern in DEFINITIONS.items():
        homes = [p for p, txt in shared.items() if re.search(pattern, txt)]
        assert len(homes) == 1, (name, homes)
        for src in sources + later:
            assert not re.search(pattern, _code(src)), (name, src)
    # code_of had a second name in pc_chroma_rate.hip; it is gone, from the headers too
    for path in sources + later + list(shared):
        assert not re.search(r"\bcode_in\b", open(path).read()), path
    # and every library's source reaches them through the host header
    for src in sources + later:
        assert '#include "pc_image_host.h"' in open(src).read(), src


def test_image_csrc_is_headers_and_one_build_rule():
    """no library of its own: nothing to compile, nothing to link against"""
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(PKG, "image_csrc", "*")) if not p.endswith((".o", ".so")))
    assert "lib.mk" in names and all(n == "lib.mk" or n.endswith(".h") for n in names), names
    assert not os.path.exists(os.path.join(PKG, "libpc_image.so"))
    import bench
    import inspect
    assert "image" not in inspect.getsource(bench.source_hash)


def test_every_makefile_is_its_name_and_the_shared_rule():
    rules = {name: image_shared.build_rule(name) for name in LIBS}                    # asserts NAME := ... and the include
    assert len(set(rules.values())) == 1
    texts = {name: image_shared.uncommented(os.path.join(PKG, name + "_csrc", "Makefile")) for name in LIBS}
    for a in LIBS:
        for b in LIBS:
            assert texts[a].replace("NAME := " + a, "NAME := " + b) == texts[b], (a, b)
        assert "include ../image_csrc/lib.mk" in texts[a]
    top = open(os.path.join(PKG, "csrc", "Makefile")).read()
    for name in LIBS:
        assert re.search(r"^%s:\n\t\$\(MAKE\) -C \.\./%s_csrc$" % (name, name), top, re.M), name
        assert "$(MAKE) -C ../%s_csrc clean" % name in top


def test_lib_mk_keeps_the_flags_and_links_no_library_of_the_project():
    mk = image_shared.uncommented(os.path.join(PKG, "image_csrc", "lib.mk"))
    flags = re.search(r"^FLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).split()
    assert flags == "-O3 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden --offload-arch=$(ARCH) -Wall -Wno-unused-function".split()
    assert "-ffp-contract=off" in mk and "--offload-arch=$(ARCH)" in mk and "-fvisibility=hidden" in mk
    assert not re.search(r"-lpc|libpc(?!_\$\(NAME\)\.so)", mk)
    assert re.search(r"^OUT\s*:=\s*\.\./libpc_\$\(NAME\)\.so$", mk, re.M)
    # the shared headers are prerequisites of every object
    assert re.search(r"^SHARED\s*:=\s*\$\(wildcard \.\./image_csrc/\*\.h\)$", mk, re.M)
    assert re.search(r"^pc_\$\(NAME\)\.o:.*\$\(SHARED\)", mk, re.M)


def test_one_frame_record_and_one_set_of_enum_values():
    shared = open(os.path.join(PKG, "image_csrc", "pc_yuv_frame.h")).read()
    values = dict((k, int(v)) for k, v in re.findall(r"\b(PC_YUV_\w+) = (\d+)", shared))
    assert values == {"PC_YUV_NV12": 0, "PC_YUV_I420": 1, "PC_YUV_P010": 2, "PC_YUV_LIMITED": 0, "PC_YUV_FULL": 1,
                      "PC_YUV_NEAREST": 0, "PC_YUV_LINEAR": 1}
    from progressivecodec_amd import frames
    assert frames.FORMATS == {"nv12": 0, "i420": 1, "p010": 2} and frames.RANGES == {"limited": 0, "full": 1}
    assert frames.UPSAMPLES == {"nearest": 0, "linear": 1}
    for lib, prefix in YUV_LIBS.items():
        hdr = open(os.path.join(PKG, lib + "_csrc", "pc_%s.h" % lib)).read()
        image_shared.assert_frame_is_shared(hdr, "pc_frame" if lib == "frames" else prefix.lower() + "_frame")
        found = dict(re.findall(r"\b(%s_(?:NV12|I420|P010|LIMITED|FULL|NEAREST|LINEAR)) = (\w+)" % prefix, hdr))
        assert {"NV12", "I420", "P010"} <= {k[len(prefix) + 1:] for k in found}, lib
        for k, v in found.items():
            assert v == "PC_YUV_" + k[len(prefix) + 1:], (lib, k, v)
    # the other libraries have no frame and no format
    for lib in set(LIBS) - set(YUV_LIBS):
        assert "pc_yuv_frame.h" not in open(os.path.join(PKG, lib + "_csrc", "pc_%s.h" % lib)).read()

"""What the host tests of the image-side libraries read out of progressivecodec_amd/image_csrc/: the one build rule (lib.mk) and the one
frame record (pc_yuv_frame.h).  No test lives here."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "progressivecodec_amd")
LIBS = ["pixels", "tiles", "rate", "frames", "frame_tiles", "frame_rate", "clips", "clip_rate", "clip_tol", "metrics"]


def uncommented(path):
    return "".join(l for l in open(path) if not l.startswith("#"))


def build_rule(name):
    """The build rule library `name` is built by, comments stripped: its Makefile must hand over to image_csrc/lib.mk."""
    mk = uncommented(os.path.join(PKG, name + "_csrc", "Makefile"))
    assert mk == "NAME := %s\ninclude ../image_csrc/lib.mk\n" % name, mk
    return uncommented(os.path.join(PKG, "image_csrc", "lib.mk"))


def shared_frame_members():
    txt = open(os.path.join(PKG, "image_csrc", "pc_yuv_frame.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct pc_frame \{(.*?)\} pc_frame;", txt, re.S).group(1), flags=re.S)
    members = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = (C.c_void_p, decl[len("void*"):]) if decl.startswith("void*") else (C.c_int64, decl[len("int64_t"):])
            assert decl.startswith(("void*", "int64_t")), decl
            members += [(n.strip(), ctype) for n in names.split(",")]
    return members


def assert_frame_is_shared(header_text, type_name):
    """`type_name` is a typedef of the shared pc_frame, and frames.Frame lays that record out field for field."""
    from progressivecodec_amd import frames
    assert '#include "pc_yuv_frame.h"' in header_text
    if type_name != "pc_frame":
        assert re.search(r"^typedef pc_frame %s;" % type_name, header_text, re.M)
    assert not re.search(r"typedef struct \w*frame\b", header_text)
    members = shared_frame_members()
    assert members == list(frames.Frame._fields_) and len(members) == 9
    assert C.sizeof(frames.Frame) == 72 and [getattr(frames.Frame, n).offset for n, _ in members] == list(range(0, 72, 8))

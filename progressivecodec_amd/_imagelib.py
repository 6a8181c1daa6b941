"""What the image-side modules share in loading their libraries: the "library missing" ImportError, CDLL, a prototype table applied
in one loop, and the base error class that formats a status code with the library's own strerror and its last HIP error.  Each module
keeps its own LIB_PATH, EXPORTS, lib() and error class and defines them through this one; each library is still a file of its own
that links no other.  The thirteen modules that shared this when it was written:

  pixels, tiles, rate, metrics
  frames, frame_tiles, frame_rate
  clips, clip_rate, clip_tol, clip_tol_rate
  chroma, chroma_tiles

and since then also:

  chroma_rate, chroma_clips, chroma_clip_rate, chroma_clip_tol, chroma_clip_tol_rate
"""
import ctypes as C
import os

from ._lib import ERRORS

PC_ERR_HIP = -6                           # pcodec.h

_HERE = os.path.dirname(os.path.abspath(__file__))
_loaded = {}


def lib_path(name):
    return os.path.join(_HERE, f"libpc_{name}.so")


def load(path, prototypes):
    """The library at `path`, loaded once per path.  prototypes() -> {function: (restype, argtypes)}; a restype of None leaves ctypes'
    default (int), argtypes of None leaves the function unprototyped."""
    L = _loaded.get(path)
    if L is None:
        if not os.path.exists(path):
            raise ImportError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950).  progressivecodec_amd has no CPU fallback.")
        L = C.CDLL(path)
        for name, (restype, argtypes) in prototypes().items():
            fn = getattr(L, name)
            if restype is not None:
                fn.restype = restype
            if argtypes is not None:
                fn.argtypes = argtypes
        _loaded[path] = L
    return L


class ImageLibError(RuntimeError):
    """Base of the modules' error classes.  A subclass sets _lib (the module's lib, as a staticmethod) and _prefix ("pc_tiles"): the
    library exports <prefix>_strerror and <prefix>_last_hip_error."""
    _lib = None
    _prefix = None

    def __init__(self, code, where=""):
        L = self._lib()
        hip = getattr(L, self._prefix + "_last_hip_error")() if code == PC_ERR_HIP else 0
        msg = getattr(L, self._prefix + "_strerror")(code).decode()
        super().__init__(f"{where}: {ERRORS.get(code, code)} ({msg})" + (f" hipError={hip}" if hip else ""))

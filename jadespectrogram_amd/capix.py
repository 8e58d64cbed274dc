"""ctypes binding of the companion C-ABI declared in include/jsgx.h (libjsgx.so: hand-written HIP for gfx950).

Plumbing only, as capi is for libjsg.so, and with NO CPU fallback: a missing library fails loudly, and without a usable MI355X the
launch returns JSGX_ERR_NO_DEVICE.  The two libraries share nothing but device memory.
"""
from __future__ import annotations

import ctypes as C
import os

from .capi import JsgError

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "libjsgx.so")

JSGX_ABI_VERSION = 1
JSGX_OK = 0
JSGX_ERR_INVALID = -2
JSGX_ERR_HIP = -4
JSGX_ERR_NO_DEVICE = -5

BEAT_MAX_PERIOD, BEAT_MAX_FRAMES, BEAT_THREADS, BEAT_LDS_BYTES = 1024, 1 << 24, 256, 31008
BEAT_LOG_TABLE = 2 * BEAT_MAX_PERIOD + 1
EXP_REL_BOUND = 1.0e-7


class BeatArgs(C.Structure):
    _fields_ = [("in_", C.c_void_p), ("in_pitch", C.c_int64), ("rows", C.c_int32), ("n_frames", C.c_int32), ("period", C.c_void_p),
                ("period_all", C.c_int32), ("smooth", C.c_int32), ("log_table", C.c_void_p), ("tightness", C.c_float), ("normalise", C.c_int32),
                ("beats", C.c_void_p), ("beats_pitch", C.c_int64), ("max_beats", C.c_int32), ("reserved0", C.c_int32), ("n_beats", C.c_void_p),
                ("local_score", C.c_void_p), ("local_pitch", C.c_int64), ("cum_score", C.c_void_p), ("cum_pitch", C.c_int64)]


# every symbol include/jsgx.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SIGNATURES = {
    "jsgx_abi_version": (C.c_int, []),
    "jsgx_last_error": (C.c_char_p, []),
    "jsgx_log_table_build": (C.c_int, [C.c_int32, _P]),
    "jsgx_beat_scratch_bytes": (C.c_int64, [C.POINTER(BeatArgs)]),
    "jsgx_beat_launch": (C.c_int, [C.POINTER(BeatArgs), _P, C.c_int64, _P]),
    "jsgx_beat_plan": (C.c_int, [C.POINTER(BeatArgs), C.c_int32, C.c_char_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
}

_lib = None


def lib() -> C.CDLL:
    """Load libjsgx.so (once).  Raises if the HIP extension has not been built -- no silent fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  jadespectrogram_amd has no CPU fallback.")
        # one HIP runtime per process: torch first, for the reason capi.lib() gives
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)   # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc: int) -> int:
    if rc < 0:
        msg = lib().jsgx_last_error()
        raise JsgError(rc, msg.decode() if msg else "")
    return rc

"""YIN, host side (include/jsg.h section 2i): the frame count at its edges, every refusal of the launch in its stated order (all
decided without a device), the plan swept over the corners of the accepted range, the symbols and the exports.  CPU only."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

import yin_ref as yr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# never dereferenced: every call below is refused, or only planned
IN, F0, APER, CMND = (i << 44 for i in range(1, 5))
L, W, LO, HI, HOP = 3000, 256, 8, 200, 64
T = yr.frames(L, W, HI, HOP)
PATHS = {"yin_lags1", "yin_lags2", "yin_lags4", "yin_lags8"}
LDS_MAX = 163840


def valid_args(jsg, **kw):
    a = dict(in_=IN, in_pitch=L, rows=2, window=W, in_samples=L, tau_min=LO, tau_max=HI, hop=HOP, n_frames=T, threshold=0.1, sample_rate=8000.0,
             f0=F0, aper=APER, out_pitch=T, cmnd=CMND, cmnd_frame_pitch=HI + 1, cmnd_row_pitch=T * (HI + 1), chunk_frames=0)
    a.update(kw)
    return jsg.capi.YinArgs(**a)


def plan(jsg, a):
    name, frames, lds = C.create_string_buffer(32), C.c_int32(-1), C.c_int32(-1)
    rc = jsg.capi.lib().jsg_yin_plan(C.byref(a), name, 32, C.byref(frames), C.byref(lds))
    return rc, name.value.decode(), frames.value, lds.value


def test_frames_at_the_edges(jsg):
    lib, bad = jsg.capi.lib(), jsg.capi.JSG_ERR_INVALID
    for n, w, hi, hop in itertools.product((1, 2, 455, 456, 457, 519, 520, 3000, 2 ** 31 - 1), (1, 256, 8192), (1, 200, 8192), (1, 64, 2 ** 20)):
        assert lib.jsg_yin_frames(n, w, hi, hop) == yr.frames(n, w, hi, hop), (n, w, hi, hop)
    assert lib.jsg_yin_frames(455, 256, 200, 64) == 0 and lib.jsg_yin_frames(456, 256, 200, 64) == 1 and lib.jsg_yin_frames(520, 256, 200, 64) == 2
    assert lib.jsg_yin_frames(2, 1, 1, 1) == 1 and lib.jsg_yin_frames(2 ** 31 - 1, 1, 1, 1) == 2 ** 31 - 2
    assert jsg.yin_frames(L, W, HI, HOP) == T == 40
    for args, message in (((0, 1, 1, 1), "in_samples must be in 1..2^31-1"), ((2 ** 31, 1, 1, 1), "in_samples must be in 1..2^31-1"),
                          ((10, 0, 1, 1), "window must be in 1..8192"), ((10, 8193, 1, 1), "window must be in 1..8192"),
                          ((10, 1, 0, 1), "tau_max must be in 1..8192"), ((10, 1, 8193, 1), "tau_max must be in 1..8192"),
                          ((10, 1, 1, 0), "hop must be in 1..2^20"), ((10, 1, 1, 2 ** 20 + 1), "hop must be in 1..2^20")):
        assert lib.jsg_yin_frames(*args) == bad and lib.jsg_last_error(None) == b"jsg_yin_frames: " + message.encode()
    with pytest.raises(jsg.JsgError):
        jsg.yin_frames(10, 0, 1, 1)


# in the order of the header: a call with two defects is refused for the earlier one
REFUSED = [
    ("null in", dict(in_=None), "null in"),
    ("no output", dict(f0=None, aper=None, cmnd=None), "f0, aper and cmnd are all null"),
    ("misaligned in", dict(in_=IN + 2), "pointers must be 4-byte aligned"),
    ("misaligned cmnd", dict(cmnd=CMND + 1), "pointers must be 4-byte aligned"),
    ("no rows", dict(rows=0), "rows must be in 1..65535"),
    ("65536 rows", dict(rows=65536), "rows must be in 1..65535"),
    ("no samples", dict(in_samples=0), "in_samples must be in 1..2^31-1"),
    ("2^31 samples", dict(in_samples=2 ** 31, in_pitch=2 ** 31), "in_samples must be in 1..2^31-1"),
    ("window 0", dict(window=0), "window must be in 1..8192"),
    ("window 8193", dict(window=8193), "window must be in 1..8192"),
    ("tau_max 0", dict(tau_max=0), "tau_max must be in 1..8192"),
    ("tau_max 8193", dict(tau_max=8193), "tau_max must be in 1..8192"),
    ("tau_min 0", dict(tau_min=0), "tau_min must be in 1..tau_max"),
    ("tau_min above tau_max", dict(tau_min=HI + 1), "tau_min must be in 1..tau_max"),
    ("hop 0", dict(hop=0), "hop must be in 1..2^20"),
    ("hop above 2^20", dict(hop=2 ** 20 + 1), "hop must be in 1..2^20"),
    ("no frames", dict(n_frames=0), "n_frames must be in 1..jsg_yin_frames"),
    ("a frame too many", dict(n_frames=T + 1, out_pitch=T + 1, cmnd_row_pitch=(T + 1) * (HI + 1)), "n_frames must be in 1..jsg_yin_frames"),
    ("a row too short", dict(in_samples=W + HI - 1, n_frames=1), "n_frames must be in 1..jsg_yin_frames"),
    ("chunk -1", dict(chunk_frames=-1), "chunk_frames must be 0 or in 1..65536"),
    ("chunk 65537", dict(chunk_frames=65537), "chunk_frames must be 0 or in 1..65536"),
    ("threshold 0", dict(threshold=0.0), "threshold must be finite and > 0"),
    ("threshold nan", dict(threshold=float("nan")), "threshold must be finite and > 0"),
    ("threshold inf", dict(threshold=float("inf")), "threshold must be finite and > 0"),
    ("rate negative", dict(sample_rate=-1.0), "sample_rate must be finite and > 0"),
    ("rate inf", dict(sample_rate=float("inf")), "sample_rate must be finite and > 0"),
    ("in_pitch", dict(in_pitch=L - 1), "in_pitch smaller than in_samples"),
    ("out_pitch", dict(out_pitch=T - 1), "out_pitch smaller than n_frames"),
    ("cmnd_frame_pitch", dict(cmnd_frame_pitch=HI), "cmnd_frame_pitch smaller than tau_max + 1"),
    ("cmnd_row_pitch", dict(cmnd_row_pitch=T * (HI + 1) - 1), "cmnd_row_pitch smaller than (n_frames-1)*cmnd_frame_pitch + tau_max + 1"),
    ("f0 inside in", dict(f0=IN + 4 * (L + 10)), "an output overlaps in"),
    ("cmnd ends in in", dict(cmnd=IN - 4 * 2 * T * (HI + 1) + 4), "an output overlaps in"),
]


@pytest.mark.parametrize("i", range(len(REFUSED)), ids=[r[0] for r in REFUSED])
def test_refusals_in_their_order(jsg, i):
    lib, bad = jsg.capi.lib(), jsg.capi.JSG_ERR_INVALID
    _, change, message = REFUSED[i]
    a = valid_args(jsg, **change)
    buf = C.create_string_buffer(32)
    for who, call in (("jsg_yin_launch", lambda a: lib.jsg_yin_launch(C.byref(a), None)),
                      ("jsg_yin_plan", lambda a: lib.jsg_yin_plan(C.byref(a), None, 0, None, None)),
                      ("jsg_yin_kernel_name", lambda a: lib.jsg_yin_kernel_name(C.byref(a), buf, 32))):
        assert call(a) == bad and lib.jsg_last_error(None) == f"{who}: {message}".encode()
    # with any later defect on top, the earlier one is still the one reported
    for _, later, later_message in REFUSED[i + 1:]:
        if later_message == message or set(later) & set(change):
            continue
        both = valid_args(jsg, **dict(later, **change))
        assert lib.jsg_yin_launch(C.byref(both), None) == bad
        assert lib.jsg_last_error(None) == f"jsg_yin_launch: {message}".encode(), (REFUSED[i][0], later)


def test_null_arguments_and_what_one_row_ignores(jsg):
    lib, bad = jsg.capi.lib(), jsg.capi.JSG_ERR_INVALID
    assert lib.jsg_yin_launch(None, None) == bad and lib.jsg_last_error(None) == b"jsg_yin_launch: null argument"
    assert lib.jsg_yin_plan(None, None, 0, None, None) == bad
    buf = C.create_string_buffer(32)
    a = valid_args(jsg)
    assert lib.jsg_yin_kernel_name(C.byref(a), None, 32) == bad and lib.jsg_yin_kernel_name(C.byref(a), buf, 23) == bad
    assert lib.jsg_yin_plan(C.byref(a), buf, 23, None, None) == bad
    # one row: the row pitches are not looked at; outputs that are not given: neither are their pitches
    one = valid_args(jsg, rows=1, in_pitch=0, out_pitch=0, cmnd_row_pitch=0)
    assert plan(jsg, one)[0] == jsg.capi.JSG_OK
    assert plan(jsg, valid_args(jsg, f0=None, aper=None, out_pitch=0))[0] == jsg.capi.JSG_OK
    assert plan(jsg, valid_args(jsg, cmnd=None, cmnd_frame_pitch=0, cmnd_row_pitch=0))[0] == jsg.capi.JSG_OK
    assert plan(jsg, valid_args(jsg, aper=None, cmnd=None))[0] == jsg.capi.JSG_OK
    # outputs next to the input, not inside it
    assert plan(jsg, valid_args(jsg, f0=IN + 4 * 2 * L))[0] == jsg.capi.JSG_OK
    assert plan(jsg, valid_args(jsg, cmnd=IN - 4 * 2 * T * (HI + 1)))[0] == jsg.capi.JSG_OK


def test_no_device_comes_after_the_refusals(jsg):
    lib = jsg.capi.lib()
    if lib.jsg_device_count() > 0:
        pytest.skip("a GPU is present")
    assert lib.jsg_yin_launch(C.byref(valid_args(jsg)), None) == jsg.capi.JSG_ERR_NO_DEVICE
    assert lib.jsg_yin_launch(C.byref(valid_args(jsg, hop=0)), None) == jsg.capi.JSG_ERR_INVALID


CORNERS = (1, 63, 64, 65, 8192)


@pytest.mark.parametrize("hop", [1, 64, 2 ** 20])
def test_plan_over_the_corners(jsg, hop):
    seen = set()
    for w, hi, chunk, frames in itertools.product(CORNERS, CORNERS, (0, 1, 3, 65536), (1, 2, 40, 100000)):
        n = (frames - 1) * hop + w + hi
        if n >= 2 ** 31:
            continue
        a = valid_args(jsg, rows=1, window=w, tau_min=1, tau_max=hi, hop=hop, in_samples=n, n_frames=frames, chunk_frames=chunk,
                       cmnd_frame_pitch=hi + 1, f0=None, aper=None)
        rc, name, F, lds = plan(jsg, a)
        assert rc == jsg.capi.JSG_OK, (w, hi, chunk, frames)
        seen.add(name)
        assert name == {1: "yin_lags1", 63: "yin_lags1", 64: "yin_lags1", 65: "yin_lags2", 8192: "yin_lags8"}[hi]
        assert 1 <= F <= frames and (chunk == 0 or F <= chunk) and 0 < lds <= LDS_MAX, (w, hi, chunk, frames, F, lds)
        S = min(hop, w + hi)
        assert lds == 4 * ((F - 1) * S + w + hi + 1024 + F * (hi + 1))
        one = w + hi + 1024 + hi + 1
        assert lds <= (40960 if one <= 10240 else 81920 if one <= 20480 else LDS_MAX)   # four, two or one workgroup per compute unit, by what one frame needs
    assert seen == {"yin_lags1", "yin_lags2", "yin_lags8"}
    for hi, name in ((128, "yin_lags2"), (129, "yin_lags4"), (200, "yin_lags4"), (256, "yin_lags4"), (257, "yin_lags8"), (1000, "yin_lags8")):
        assert plan(jsg, valid_args(jsg, tau_max=hi, cmnd=None, n_frames=20))[1] == name, hi
    # the default: 16 frames where they fit, else a whole number of rounds of the four waves
    assert plan(jsg, valid_args(jsg))[2] == 16
    big = dict(in_samples=40 * 512 + 2048, in_pitch=40 * 512 + 2048, hop=512, n_frames=40, cmnd=None)
    assert plan(jsg, valid_args(jsg, window=1024, tau_max=1024, **big))[1:] == ("yin_lags8", 4, 4 * (3 * 512 + 2048 + 1024 + 4 * 1025))
    assert plan(jsg, valid_args(jsg, window=1536, tau_max=512, **big))[1:] == ("yin_lags8", 4, 4 * (3 * 512 + 2048 + 1024 + 4 * 513))


def test_symbols_and_exports(jsg):
    lib = jsg.capi.lib()
    for name in ("jsg_yin_frames", "jsg_yin_launch", "jsg_yin_plan", "jsg_yin_kernel_name"):
        assert hasattr(lib, name) and name in jsg.capi.SIGNATURES
    for name in ("yin_frames", "yin_launch", "yin_plan", "yin_kernel_name", "yin", "yin_cmnd"):
        assert callable(getattr(jsg, name)) and name in jsg.__all__
    hdr = open(os.path.join(ROOT, "include", "jsg.h")).read()
    assert "section 2i" in hdr and "#define JSG_ABI_VERSION 6 " in hdr and lib.jsg_abi_version() == 6
    assert jsg.capi.YIN_MAX_WINDOW == 8192 and jsg.capi.YIN_MAX_LAG == 8192


def test_struct_layout_matches_the_header(jsg, tmp_path):
    import re
    import shutil
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsg.h")).read(), flags=re.S)
    body = re.search(r"typedef struct jsg_yin_args \{(.*?)\} jsg_yin_args;", hdr, flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*$", piece).group(1) for decl in body.split(";") if decl.strip() for piece in decl.split(",")]
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "jsg.h"', "int main(void) {", '    printf("%zu\\n", sizeof(jsg_yin_args));']
    lines += [f'    printf("{f} %zu %zu\\n", offsetof(jsg_yin_args, {f}), sizeof(((jsg_yin_args*)0)->{f}));' for f in names]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)])
    out = subprocess.check_output([str(tmp_path / "layout")], text=True).split("\n")
    cls = jsg.capi.YinArgs
    assert out[0] == str(C.sizeof(cls))
    assert [f for f, _ in cls._fields_] == ["in_" if f == "in" else f for f in names]
    for (f, _), c_name, line in zip(cls._fields_, names, out[1:]):
        assert line == f"{c_name} {getattr(cls, f).offset} {getattr(cls, f).size}"


def test_python_wrapper_refuses_a_frame_without_a_window(jsg):
    import numpy as np
    with pytest.raises(jsg.JsgError) as ei:                   # tau_max = ceil(22050 / 10) = 2205 > 2048: refused before any device is asked for
        jsg.yin(np.zeros(8192, np.float32), 22050.0, 10.0, 2000.0, frame_length=2048)
    assert ei.value.code == jsg.capi.JSG_ERR_INVALID
    with pytest.raises(jsg.JsgError):
        jsg.yin_cmnd(np.zeros(8192, np.float32), 22050.0, 22050.0 / 2048, 2000.0, frame_length=2048)          # tau_max == frame_length: no window

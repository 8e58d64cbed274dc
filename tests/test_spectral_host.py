"""Spectral shape descriptors, host side (include/jsg.h section 2l): every refusal of the launch in its stated order (all decided
without a device, the same from the plan and the name query), the plan on both sides of every path boundary, the symbols, the exports,
the defines, the Python signatures and docstrings, the struct layout and the kernels' notes.  CPU only."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

import spectral_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# never dereferenced: every call below is refused, or only planned
IN, FREQS, OUT = (i << 50 for i in range(1, 4))           # apart by more than the largest plane (2^49 bytes)
OUTS = ("energy", "centroid", "spread", "rolloff", "rolloff_bin", "flatness_db", "crest")
BAD = -2
T, K = 40, 257
ONE = 4 * 2 * T                 # bytes of one output of the default call: two rows of T


def args(jsg, **kw):
    a = dict(in_=IN, frame_pitch=K, row_pitch=T * K, rows=2, n_bins=K, n_frames=T, freqs=FREQS, roll_percent=0.85, reserved0=0, out_pitch=T)
    a.update({name: OUT + i * (1 << 30) for i, name in enumerate(OUTS)})
    a.update(kw)
    return jsg.capi.SpectralArgs(**a)


def plan(jsg, a):
    name, lanes, frames, lds = C.create_string_buffer(32), C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    rc = jsg.capi.lib().jsg_spectral_shape_plan(C.byref(a), name, 32, C.byref(lanes), C.byref(frames), C.byref(lds))
    return rc, name.value.decode(), lanes.value, frames.value, lds.value


NO_OUT = {name: None for name in OUTS}
# in the order of the header: a call with two defects is refused for the earlier one
REFUSED = [
    ("null in", dict(in_=None), "null in"),
    ("null freqs", dict(freqs=None), "null freqs"),
    ("no output", NO_OUT, "all outputs null"),
    ("misaligned in", dict(in_=IN + 2), "pointers must be 4-byte aligned"),
    ("misaligned freqs", dict(freqs=FREQS + 1), "pointers must be 4-byte aligned"),
    ("misaligned energy", dict(energy=OUT + 3), "pointers must be 4-byte aligned"),
    ("misaligned bin", dict(rolloff_bin=OUT + (4 << 30) + 2), "pointers must be 4-byte aligned"),
    ("no rows", dict(rows=0), "rows must be in 1..65535"),
    ("65536 rows", dict(rows=65536), "rows must be in 1..65535"),
    ("no bins", dict(n_bins=0), "n_bins must be in 1..65536"),
    ("65537 bins", dict(n_bins=65537, frame_pitch=65537, row_pitch=T * 65537), "n_bins must be in 1..65536"),
    ("no frames", dict(n_frames=0), "n_frames must be in 1..2^31-1"),
    ("2^31 frames", dict(n_frames=2 ** 31, row_pitch=2 ** 41, out_pitch=2 ** 31), "n_frames must be in 1..2^31-1"),
    ("roll 0", dict(roll_percent=0.0), "roll_percent must be in (0, 1]"),
    ("roll above 1", dict(roll_percent=1.0000001), "roll_percent must be in (0, 1]"),
    ("roll negative", dict(roll_percent=-0.5), "roll_percent must be in (0, 1]"),
    ("roll NaN", dict(roll_percent=float("nan")), "roll_percent must be in (0, 1]"),
    ("frame_pitch", dict(frame_pitch=K - 1), "frame_pitch smaller than n_bins"),
    ("row_pitch", dict(row_pitch=T * K - 1), "row_pitch smaller than (n_frames-1)*frame_pitch + n_bins"),
    ("out_pitch", dict(out_pitch=T - 1), "out_pitch smaller than n_frames"),
    ("energy inside in", dict(energy=IN + 4 * 100), "an output overlaps in"),
    ("crest ends in in", dict(crest=IN - ONE + 4), "an output overlaps in"),
    ("bin inside freqs", dict(rolloff_bin=FREQS + 4 * (K - 1)), "an output overlaps freqs"),
    ("spread ends in freqs", dict(spread=FREQS - ONE + 4), "an output overlaps freqs"),
]
CALLS = (("jsg_spectral_shape_launch", lambda lib, a, buf: lib.jsg_spectral_shape_launch(C.byref(a), None)),
         ("jsg_spectral_shape_plan", lambda lib, a, buf: lib.jsg_spectral_shape_plan(C.byref(a), None, 0, None, None, None)),
         ("jsg_spectral_shape_kernel_name", lambda lib, a, buf: lib.jsg_spectral_shape_kernel_name(C.byref(a), buf, 32)))


@pytest.mark.parametrize("i", range(len(REFUSED)), ids=[r[0] for r in REFUSED])
def test_refusals_in_their_order(jsg, i):
    lib = jsg.capi.lib()
    _, change, message = REFUSED[i]
    a = args(jsg, **change)
    buf = C.create_string_buffer(32)
    for who, call in CALLS:
        assert call(lib, a, buf) == BAD and lib.jsg_last_error(None) == f"{who}: {message}".encode()
    # with any later defect on top, the earlier one is still the one reported
    who, call = CALLS[0]
    for _, later, later_message in REFUSED[i + 1:]:
        if later_message == message or set(later) & set(change):
            continue
        both = args(jsg, **dict(later, **change))
        assert call(lib, both, buf) == BAD
        assert lib.jsg_last_error(None) == f"{who}: {message}".encode(), (REFUSED[i][0], later)


def test_null_arguments_and_what_passes(jsg):
    lib = jsg.capi.lib()
    assert lib.jsg_spectral_shape_launch(None, None) == BAD and lib.jsg_last_error(None) == b"jsg_spectral_shape_launch: null argument"
    assert lib.jsg_spectral_shape_plan(None, None, 0, None, None, None) == BAD and lib.jsg_last_error(None) == b"jsg_spectral_shape_plan: null argument"
    buf = C.create_string_buffer(32)
    a = args(jsg)
    assert lib.jsg_spectral_shape_kernel_name(C.byref(a), None, 32) == BAD and lib.jsg_spectral_shape_kernel_name(C.byref(a), buf, 23) == BAD
    assert lib.jsg_spectral_shape_plan(C.byref(a), buf, 23, None, None, None) == BAD
    # one row: the row pitches are not looked at
    assert plan(jsg, args(jsg, rows=1, row_pitch=0, out_pitch=0))[0] == 0
    # each output alone passes; outputs next to the input and the table, not inside them
    for name in OUTS:
        assert plan(jsg, args(jsg, **dict(NO_OUT, **{name: OUT})))[0] == 0, name
    assert plan(jsg, args(jsg, energy=IN + 4 * 2 * T * K))[0] == 0 and plan(jsg, args(jsg, energy=IN - ONE))[0] == 0
    assert plan(jsg, args(jsg, crest=FREQS + 4 * K))[0] == 0 and plan(jsg, args(jsg, crest=FREQS - ONE))[0] == 0
    # the ends of the ranges
    assert plan(jsg, args(jsg, roll_percent=1.0))[0] == 0 and plan(jsg, args(jsg, roll_percent=1e-45))[0] == 0
    assert plan(jsg, args(jsg, n_bins=65536, frame_pitch=65536, row_pitch=T * 65536))[0] == 0
    assert plan(jsg, args(jsg, rows=65535, n_frames=1, n_bins=5, frame_pitch=5, row_pitch=5, out_pitch=1))[0] == 0
    assert plan(jsg, args(jsg, rows=1, n_frames=2 ** 31 - 1))[0] == 0


def test_no_device_comes_after_the_refusals(jsg):
    lib = jsg.capi.lib()
    if lib.jsg_device_count() > 0:
        pytest.skip("a GPU is present")
    assert lib.jsg_spectral_shape_launch(C.byref(args(jsg)), None) == jsg.capi.JSG_ERR_NO_DEVICE
    assert lib.jsg_spectral_shape_launch(C.byref(args(jsg, rows=0)), None) == BAD


def test_plan_on_both_sides_of_every_boundary(jsg):
    seen = set()
    edges = sorted({1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 63, 65536} | {64 * n + d for n in sr.REGS for d in (0, 1)} | {n // 2 + 1 for n in (512, 1024, 2048, 4096, 8192)})
    for bins in edges:
        for frames in (1, 7, 2 ** 31 - 1):
            a = args(jsg, rows=1, n_bins=bins, frame_pitch=bins, n_frames=frames)
            got = plan(jsg, a)
            assert got == (0,) + sr.plan(bins) + (0,), (bins, got)
            assert plan(jsg, a) == got                   # stable
            buf = C.create_string_buffer(32)
            assert jsg.capi.lib().jsg_spectral_shape_kernel_name(C.byref(a), buf, 32) == 0 and buf.value.decode() == got[1]
        seen.add(got[1])
        # by the bins alone: not by which outputs are given, the percentage or the pitches
        assert plan(jsg, args(jsg, n_bins=bins, frame_pitch=bins + 3, row_pitch=T * (bins + 3) + 1, roll_percent=0.5, **dict(NO_OUT, crest=OUT)))[1:] == got[1:]
    assert seen == {f"spectral_regs{n}" for n in sr.REGS} | {"spectral_stream"}
    # the engine's transforms stay in registers: 65 values per lane hold the 4097 bins of 8192 points
    assert plan(jsg, args(jsg, n_bins=4097, frame_pitch=4097, row_pitch=T * 4097))[1:] == ("spectral_regs65", 64, 1, 0)
    assert plan(jsg, args(jsg, n_bins=128, frame_pitch=128, row_pitch=T * 128))[1:] == ("spectral_regs2", 64, 8, 0)


def test_symbols_and_exports(jsg):
    lib = jsg.capi.lib()
    for name in ("jsg_spectral_shape_launch", "jsg_spectral_shape_plan", "jsg_spectral_shape_kernel_name"):
        assert hasattr(lib, name) and name in jsg.capi.SIGNATURES
    assert len(jsg.capi.SIGNATURES) == 146
    names = ("spectral_shape_launch", "spectral_shape_plan", "spectral_shape_kernel_name", "fft_frequencies", "spectral_shape", "spectral_centroid",
             "spectral_bandwidth", "spectral_rolloff", "spectral_flatness", "spectral_crest", "spectral_shape_audio")
    for name in names:
        assert callable(getattr(jsg, name)) and name in jsg.__all__
    hdr = open(os.path.join(ROOT, "include", "jsg.h")).read()
    assert "2l. Spectral shape descriptors" in hdr and "section 2l" in hdr
    assert "#define JSG_ABI_VERSION 6 " in hdr and lib.jsg_abi_version() == 6
    assert re.search(rf"#define JSG_SPECTRAL_MAX_BINS {jsg.capi.SPECTRAL_MAX_BINS}\b", hdr) and jsg.capi.SPECTRAL_MAX_BINS == 65536
    sig = inspect.signature(jsg.spectral_shape_launch)
    assert list(sig.parameters) == ["d_S", "d_freqs", "d_energy", "d_centroid", "d_spread", "d_rolloff", "d_rolloff_bin", "d_flatness_db", "d_crest", "roll_percent", "stream"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [None] * 7 + [0.85, None]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in list(sig.parameters.values())[2:])
    sig = inspect.signature(jsg.spectral_shape)
    assert list(sig.parameters) == ["S", "freqs", "sr", "roll_percent"] and [p.default for p in list(sig.parameters.values())[1:]] == [None, None, 0.85]
    sig = inspect.signature(jsg.spectral_shape_audio)
    assert list(sig.parameters) == ["x", "sr", "n_fft", "hop", "roll_percent"] and [p.default for p in list(sig.parameters.values())[2:]] == [2048, 512, 0.85]
    assert list(inspect.signature(jsg.fft_frequencies).parameters) == ["sr", "n_fft"]
    assert list(inspect.signature(jsg.spectral_rolloff).parameters) == ["S", "freqs", "sr", "roll_percent"]
    for fn in (jsg.spectral_shape, jsg.spectral_centroid, jsg.spectral_bandwidth, jsg.spectral_rolloff, jsg.spectral_flatness, jsg.spectral_crest, jsg.spectral_shape_audio):
        text = " ".join(fn.__doc__.split()).lower()
        assert "axis -2" in text and "not measured" in text and "power" in text and "centring" in text, fn.__name__
    for fn in (jsg.spectral_shape, jsg.spectral_flatness, jsg.spectral_shape_audio):
        text = " ".join(fn.__doc__.split())
        assert "1e-11" in text and "1e-10" in text, fn.__name__


def test_fft_frequencies(jsg):
    import numpy as np
    for srate, n in ((22050, 2048), (48000.0, 512), (44100, 8192), (8000, 2)):
        f = jsg.fft_frequencies(srate, n)
        assert f.dtype == np.float32 and f.shape == (n // 2 + 1,) and f[0] == 0 and f[-1] == np.float32(srate / 2)
        assert np.array_equal(f, np.array([np.float32(k * float(srate) / n) for k in range(n // 2 + 1)], np.float32))


def test_struct_layout_matches_the_header(jsg, tmp_path):
    import shutil
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler")
    struct, cls = "jsg_spectral_args", jsg.capi.SpectralArgs
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsg.h")).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*$", piece).group(1) for decl in body.split(";") if decl.strip() for piece in decl.split(",")]
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "jsg.h"', "int main(void) {", f'    printf("%zu\\n", sizeof({struct}));']
    lines += [f'    printf("{f} %zu %zu\\n", offsetof({struct}, {f}), sizeof((({struct}*)0)->{f}));' for f in names]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)])
    out = subprocess.check_output([str(tmp_path / "layout")], text=True).split("\n")
    assert out[0] == str(C.sizeof(cls))
    assert [f for f, _ in cls._fields_] == ["in_" if f == "in" else f for f in names]
    for (f, _), c_name, line in zip(cls._fields_, names, out[1:]):
        assert line == f"{c_name} {getattr(cls, f).offset} {getattr(cls, f).size}"


def test_kernel_notes(jsg, tmp_path):
    """No private segment (no scratch), no spilled register of either kind and no LDS in any kernel of the unit; its kernels are the seven
    register paths the plan names and the streaming one."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    obj = os.path.join(ROOT, "jadespectrogram_amd", "build", "jsg_spectral.o")
    if not os.path.exists(obj):
        from jadespectrogram_amd import _build
        _build.build_lib()
    co = kernel_regs.code_object(obj, str(tmp_path))
    notes = subprocess.check_output([os.path.join(kernel_regs.LLVM, "llvm-readelf"), "--notes", co]).decode()
    found = {}
    for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
        g = lambda k: re.search(rf"\.{k}:\s+(\S+)", blk).group(1)
        found[g("name")] = (int(g("private_segment_fixed_size")), int(g("group_segment_fixed_size")), int(g("vgpr_spill_count")), int(g("sgpr_spill_count")), int(g("vgpr_count")))
    assert len(found) == 8 and sum("spectral_regs_kernel" in k for k in found) == 7 and sum("spectral_stream_kernel" in k for k in found) == 1
    for name, (private, lds, vspill, sspill, vgprs) in found.items():
        assert private == 0 and lds == 0 and vspill == 0 and sspill == 0 and vgprs <= 256, name

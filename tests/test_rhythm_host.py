"""Onset strength, tempogram and tempo, host side (include/jsg.h section 2j): the frame count, every refusal of the three launches in
its stated order (all decided without a device), the tempogram plan swept over the corners of the accepted range, the prior table, the
symbols, the exports, the struct layouts and the kernels' notes.  CPU only."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import rhythm_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# never dereferenced: every call below is refused, or only planned
IN, OUT, WIN, PRIOR, BPM, LAG, PROFILE = (i << 44 for i in range(1, 8))
LDS_MAX = 163840
BAD = -2


def onset_args(jsg, **kw):
    a = dict(in_=IN, frame_pitch=128, row_pitch=40 * 128, rows=2, n_bands=128, n_frames=40, lag=1, max_size=1, out=OUT, out_pitch=40)
    a.update(kw)
    return jsg.capi.OnsetArgs(**a)


def tempogram_args(jsg, **kw):
    a = dict(in_=IN, in_pitch=600, rows=2, win_length=384, n_in=600, hop=1, n_frames=600, lags=384, normalise=1, window=WIN, out=OUT,
             frame_pitch=384, row_pitch=600 * 384, chunk_frames=0)
    a.update(kw)
    return jsg.capi.TempogramArgs(**a)


def tempo_args(jsg, **kw):
    a = dict(in_=IN, frame_pitch=384, row_pitch=600 * 384, rows=2, lags=384, n_frames=600, frame_rate=43.0, prior=PRIOR, bpm=BPM, lag=LAG,
             profile=PROFILE, profile_pitch=384)
    a.update(kw)
    return jsg.capi.TempoArgs(**a)


def plan(jsg, a):
    name, frames, lds = C.create_string_buffer(32), C.c_int32(-1), C.c_int32(-1)
    rc = jsg.capi.lib().jsg_tempogram_plan(C.byref(a), name, 32, C.byref(frames), C.byref(lds))
    return rc, name.value.decode(), frames.value, lds.value


def test_tempogram_frames(jsg):
    lib = jsg.capi.lib()
    for n, hop in itertools.product((1, 2, 3, 599, 600, 601, 2 ** 31 - 1), (1, 2, 3, 600, 2 ** 20)):
        assert lib.jsg_tempogram_frames(n, hop) == rr.frames(n, hop) == 1 + (n - 1) // hop
    assert jsg.tempogram_frames(600) == 600 and jsg.tempogram_frames(600, 7) == 86
    for args, message in (((0, 1), "n_in must be in 1..2^31-1"), ((2 ** 31, 1), "n_in must be in 1..2^31-1"), ((10, 0), "hop must be in 1..2^20"),
                          ((10, 2 ** 20 + 1), "hop must be in 1..2^20")):
        assert lib.jsg_tempogram_frames(*args) == BAD and lib.jsg_last_error(None) == b"jsg_tempogram_frames: " + message.encode()
    with pytest.raises(jsg.JsgError):
        jsg.tempogram_frames(0)


# in the order of the header: a call with two defects is refused for the earlier one
ONSET_REFUSED = [
    ("null in", dict(in_=None), "null in"),
    ("null out", dict(out=None), "null out"),
    ("misaligned in", dict(in_=IN + 2), "pointers must be 4-byte aligned"),
    ("misaligned out", dict(out=OUT + 1), "pointers must be 4-byte aligned"),
    ("no rows", dict(rows=0), "rows must be in 1..65535"),
    ("65536 rows", dict(rows=65536), "rows must be in 1..65535"),
    ("no bands", dict(n_bands=0), "n_bands must be in 1..65536"),
    ("65537 bands", dict(n_bands=65537, frame_pitch=65537, row_pitch=40 * 65537), "n_bands must be in 1..65536"),
    ("no frames", dict(n_frames=0), "n_frames must be in 1..2^31-1"),
    ("2^31 frames", dict(n_frames=2 ** 31, row_pitch=2 ** 40, out_pitch=2 ** 31), "n_frames must be in 1..2^31-1"),
    ("lag 0", dict(lag=0), "lag must be in 1..4096"),
    ("lag 4097", dict(lag=4097), "lag must be in 1..4096"),
    ("max_size 0", dict(max_size=0), "max_size must be in 1..255"),
    ("max_size 256", dict(max_size=256), "max_size must be in 1..255"),
    ("frame_pitch", dict(frame_pitch=127), "frame_pitch smaller than n_bands"),
    ("row_pitch", dict(row_pitch=40 * 128 - 1), "row_pitch smaller than (n_frames-1)*frame_pitch + n_bands"),
    ("out_pitch", dict(out_pitch=39), "out_pitch smaller than n_frames"),
    ("out inside in", dict(out=IN + 4 * 100), "out overlaps in"),
    ("out ends in in", dict(out=IN - 4 * 80 + 4), "out overlaps in"),
]
TEMPOGRAM_REFUSED = [
    ("null in", dict(in_=None), "null in"),
    ("null window", dict(window=None), "null window"),
    ("null out", dict(out=None), "null out"),
    ("misaligned window", dict(window=WIN + 2), "pointers must be 4-byte aligned"),
    ("misaligned out", dict(out=OUT + 1), "pointers must be 4-byte aligned"),
    ("no rows", dict(rows=0), "rows must be in 1..65535"),
    ("65536 rows", dict(rows=65536), "rows must be in 1..65535"),
    ("no samples", dict(n_in=0), "n_in must be in 1..2^31-1"),
    ("2^31 samples", dict(n_in=2 ** 31, in_pitch=2 ** 31), "n_in must be in 1..2^31-1"),
    ("window 1", dict(win_length=1, lags=1), "win_length must be in 2..4096"),
    ("window 4097", dict(win_length=4097), "win_length must be in 2..4096"),
    ("lags 0", dict(lags=0), "lags must be in 1..win_length"),
    ("lags above the window", dict(lags=385, frame_pitch=385, row_pitch=600 * 385), "lags must be in 1..win_length"),
    ("hop 0", dict(hop=0), "hop must be in 1..2^20"),
    ("hop above 2^20", dict(hop=2 ** 20 + 1), "hop must be in 1..2^20"),
    ("no frames", dict(n_frames=0), "n_frames must be in 1..jsg_tempogram_frames"),
    ("a frame too many", dict(n_frames=601, row_pitch=601 * 384), "n_frames must be in 1..jsg_tempogram_frames"),
    ("normalise 2", dict(normalise=2), "normalise must be 0 or 1"),
    ("chunk -1", dict(chunk_frames=-1), "chunk_frames must be 0 or in 1..65536"),
    ("chunk 65537", dict(chunk_frames=65537), "chunk_frames must be 0 or in 1..65536"),
    ("in_pitch", dict(in_pitch=599), "in_pitch smaller than n_in"),
    ("frame_pitch", dict(frame_pitch=383), "frame_pitch smaller than lags"),
    ("row_pitch", dict(row_pitch=600 * 384 - 1), "row_pitch smaller than (n_frames-1)*frame_pitch + lags"),
    ("out inside in", dict(out=IN + 4 * 700), "out overlaps in"),
    ("out ends in the window", dict(out=WIN - 4 * 2 * 600 * 384 + 4), "out overlaps window"),
]
TEMPO_REFUSED = [
    ("null in", dict(in_=None), "null in"),
    ("null prior", dict(prior=None), "null prior"),
    ("no output", dict(bpm=None, lag=None, profile=None), "bpm, lag and profile are all null"),
    ("misaligned prior", dict(prior=PRIOR + 2), "pointers must be 4-byte aligned"),
    ("misaligned lag", dict(lag=LAG + 1), "pointers must be 4-byte aligned"),
    ("no rows", dict(rows=0), "rows must be in 1..65535"),
    ("65536 rows", dict(rows=65536), "rows must be in 1..65535"),
    ("one lag", dict(lags=1), "lags must be in 2..4096"),
    ("4097 lags", dict(lags=4097, frame_pitch=4097, row_pitch=600 * 4097, profile_pitch=4097), "lags must be in 2..4096"),
    ("no frames", dict(n_frames=0), "n_frames must be in 1..2^31-1"),
    ("2^31 frames", dict(n_frames=2 ** 31, row_pitch=2 ** 41), "n_frames must be in 1..2^31-1"),
    ("rate 0", dict(frame_rate=0.0), "frame_rate must be finite and > 0"),
    ("rate nan", dict(frame_rate=float("nan")), "frame_rate must be finite and > 0"),
    ("rate inf", dict(frame_rate=float("inf")), "frame_rate must be finite and > 0"),
    ("frame_pitch", dict(frame_pitch=383), "frame_pitch smaller than lags"),
    ("row_pitch", dict(row_pitch=600 * 384 - 1), "row_pitch smaller than (n_frames-1)*frame_pitch + lags"),
    ("profile_pitch", dict(profile_pitch=383), "profile_pitch smaller than lags"),
    ("bpm inside in", dict(bpm=IN + 4 * 1000), "an output overlaps in"),
    ("profile ends in the prior", dict(profile=PRIOR - 4 * 2 * 384 + 4), "an output overlaps prior"),
]
FAMILIES = {
    "onset": (ONSET_REFUSED, onset_args, (("jsg_onset_strength_launch", lambda lib, a, buf: lib.jsg_onset_strength_launch(C.byref(a), None)),)),
    "tempogram": (TEMPOGRAM_REFUSED, tempogram_args, (("jsg_tempogram_launch", lambda lib, a, buf: lib.jsg_tempogram_launch(C.byref(a), None)),
                                                      ("jsg_tempogram_plan", lambda lib, a, buf: lib.jsg_tempogram_plan(C.byref(a), None, 0, None, None)),
                                                      ("jsg_tempogram_kernel_name", lambda lib, a, buf: lib.jsg_tempogram_kernel_name(C.byref(a), buf, 32)))),
    "tempo": (TEMPO_REFUSED, tempo_args, (("jsg_tempo_launch", lambda lib, a, buf: lib.jsg_tempo_launch(C.byref(a), None)),)),
}
CASES = [(family, i) for family, (refused, _, _) in FAMILIES.items() for i in range(len(refused))]


@pytest.mark.parametrize("family,i", CASES, ids=[f"{family}: {FAMILIES[family][0][i][0]}" for family, i in CASES])
def test_refusals_in_their_order(jsg, family, i):
    lib = jsg.capi.lib()
    refused, make, calls = FAMILIES[family]
    _, change, message = refused[i]
    a = make(jsg, **change)
    buf = C.create_string_buffer(32)
    for who, call in calls:
        assert call(lib, a, buf) == BAD and lib.jsg_last_error(None) == f"{who}: {message}".encode()
    # with any later defect on top, the earlier one is still the one reported
    who, call = calls[0]
    for _, later, later_message in refused[i + 1:]:
        if later_message == message or set(later) & set(change):
            continue
        both = make(jsg, **dict(later, **change))
        assert call(lib, both, buf) == BAD
        assert lib.jsg_last_error(None) == f"{who}: {message}".encode(), (refused[i][0], later)


def test_null_arguments_and_what_one_row_ignores(jsg):
    lib = jsg.capi.lib()
    assert lib.jsg_onset_strength_launch(None, None) == BAD and lib.jsg_last_error(None) == b"jsg_onset_strength_launch: null argument"
    assert lib.jsg_tempogram_launch(None, None) == BAD and lib.jsg_last_error(None) == b"jsg_tempogram_launch: null argument"
    assert lib.jsg_tempo_launch(None, None) == BAD and lib.jsg_last_error(None) == b"jsg_tempo_launch: null argument"
    assert lib.jsg_tempogram_plan(None, None, 0, None, None) == BAD
    buf = C.create_string_buffer(32)
    a = tempogram_args(jsg)
    assert lib.jsg_tempogram_kernel_name(C.byref(a), None, 32) == BAD and lib.jsg_tempogram_kernel_name(C.byref(a), buf, 23) == BAD
    assert lib.jsg_tempogram_plan(C.byref(a), buf, 23, None, None) == BAD
    # one row: the row pitches are not looked at
    assert plan(jsg, tempogram_args(jsg, rows=1, in_pitch=0, row_pitch=0))[0] == 0
    # an output next to an input, not inside it
    assert plan(jsg, tempogram_args(jsg, out=IN + 4 * 2 * 600))[0] == 0
    assert plan(jsg, tempogram_args(jsg, out=WIN - 4 * 2 * 600 * 384))[0] == 0
    assert plan(jsg, tempogram_args(jsg, out=WIN + 4 * 384))[0] == 0


def test_no_device_comes_after_the_refusals(jsg):
    lib = jsg.capi.lib()
    if lib.jsg_device_count() > 0:
        pytest.skip("a GPU is present")
    for make, call in ((onset_args, lib.jsg_onset_strength_launch), (tempogram_args, lib.jsg_tempogram_launch), (tempo_args, lib.jsg_tempo_launch)):
        assert call(C.byref(make(jsg)), None) == jsg.capi.JSG_ERR_NO_DEVICE
        assert call(C.byref(make(jsg, rows=0)), None) == BAD
    one = tempo_args(jsg, rows=1, row_pitch=0, profile_pitch=0, bpm=None, profile=None)
    assert lib.jsg_tempo_launch(C.byref(one), None) == jsg.capi.JSG_ERR_NO_DEVICE


CORNERS = (2, 63, 64, 65, 384, 4096)


@pytest.mark.parametrize("hop", [1, 64, 2 ** 20])
def test_plan_over_the_corners(jsg, hop):
    seen = set()
    for Wn, chunk, frames in itertools.product(CORNERS, (0, 1, 3, 65536), (1, 2, 40, 2000)):
        for Lg in sorted({1, max(1, Wn // 2), Wn, min(Wn, 64), min(Wn, 65), min(Wn, 128), min(Wn, 129), min(Wn, 256), min(Wn, 257)}):
            n = (frames - 1) * hop + 1
            a = tempogram_args(jsg, rows=1, win_length=Wn, lags=Lg, hop=hop, n_in=n, n_frames=frames, chunk_frames=chunk, frame_pitch=Lg)
            rc, name, F, lds = plan(jsg, a)
            assert rc == 0, (Wn, Lg, chunk, frames)
            seen.add(name)
            NL = 1 if Lg <= 64 else 2 if Lg <= 128 else 4 if Lg <= 256 else 8
            assert name == f"tempogram_lags{NL}"
            assert 1 <= F <= frames and (chunk == 0 or F <= chunk) and 0 < lds <= LDS_MAX, (Wn, Lg, chunk, frames, F, lds)
            S, Wp = min(hop, Wn), (Wn + 3) // 4 * 4
            assert lds == 4 * (F * (Wp + Lg) + 64 + Wn + (F - 1) * S + Wn)
            one = Wp + Lg + 64 + 2 * Wn
            assert lds <= (40960 if one <= 10240 else 81920 if one <= 20480 else LDS_MAX)   # four, two or one workgroup per compute unit
    assert seen == {"tempogram_lags1", "tempogram_lags2", "tempogram_lags4", "tempogram_lags8"}
    # the default at the usual size: 384 lags are one block of lanes, so the frames come in rounds of four; 40 KiB hold 12
    assert plan(jsg, tempogram_args(jsg))[1:] == ("tempogram_lags8", 12, 4 * (12 * 768 + 64 + 384 + 11 + 384))
    assert plan(jsg, tempogram_args(jsg, win_length=64, lags=64, frame_pitch=64, row_pitch=600 * 64))[1:3] == ("tempogram_lags1", 16)


def test_prior_against_numpy(jsg):
    for lags, rate, start, std, top in ((384, rr.FRAME_RATE, 120.0, 1.0, 320.0), (4096, 100.0, 90.0, 0.5, 0.0), (2, 1.0, 60.0, 2.0, -1.0), (1, 5.0, 120.0, 1.0, 320.0)):
        got = jsg.tempo_prior(lags, rate, start, std, top)
        want = rr.prior64(lags, rate, start, std, top)
        assert got.dtype == np.float32 and got.shape == (lags,) and got[0] == 0
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - want) <= ulp).all()
        if top > 0:
            assert (got[1:][60.0 * rate / np.arange(1, lags) > top] == 0).all()
    assert jsg.tempo_prior(384, rr.FRAME_RATE)[1:9].max() == 0 and jsg.tempo_prior(384, rr.FRAME_RATE)[9] > 0       # 60 * 43.07 / 8 = 323 bpm
    lib = jsg.capi.lib()
    out = np.zeros(4, np.float32)
    for args, message in (((0, 1.0, 120.0, 1.0, 0.0), "lags must be in 1..4096"), ((4097, 1.0, 120.0, 1.0, 0.0), "lags must be in 1..4096"),
                          ((4, 0.0, 120.0, 1.0, 0.0), "frame_rate must be finite and > 0"), ((4, 1.0, -1.0, 1.0, 0.0), "start_bpm must be finite and > 0"),
                          ((4, 1.0, 120.0, float("nan"), 0.0), "std_bpm must be finite and > 0"), ((4, 1.0, 120.0, 1.0, float("inf")), "max_bpm must be finite")):
        assert lib.jsg_tempo_prior_build(*args, out.ctypes.data) == BAD and lib.jsg_last_error(None) == b"jsg_tempo_prior_build: " + message.encode()
    assert lib.jsg_tempo_prior_build(4, 1.0, 120.0, 1.0, 0.0, None) == BAD


def test_symbols_and_exports(jsg):
    lib = jsg.capi.lib()
    for name in ("jsg_onset_strength_launch", "jsg_tempogram_frames", "jsg_tempogram_launch", "jsg_tempogram_plan", "jsg_tempogram_kernel_name",
                 "jsg_tempo_prior_build", "jsg_tempo_launch"):
        assert hasattr(lib, name) and name in jsg.capi.SIGNATURES
    for name in ("onset_strength", "onset_strength_launch", "tempogram", "tempogram_launch", "tempogram_frames", "tempogram_plan", "tempogram_kernel_name",
                 "tempo_prior", "tempo_launch", "tempo", "estimate_tempo"):
        assert callable(getattr(jsg, name)) and name in jsg.__all__
    hdr = open(os.path.join(ROOT, "include", "jsg.h")).read()
    assert "section 2j" in hdr and "#define JSG_ABI_VERSION 6 " in hdr and lib.jsg_abi_version() == 6
    assert "#define JSG_TEMPOGRAM_MAX_WINDOW 4096" in hdr and jsg.capi.TEMPOGRAM_MAX_WINDOW == 4096
    assert (jsg.capi.ONSET_MAX_BANDS, jsg.capi.ONSET_MAX_LAG, jsg.capi.ONSET_MAX_SIZE) == (65536, 4096, 255)
    import inspect
    sig = inspect.signature(jsg.estimate_tempo)
    assert list(sig.parameters) == ["x", "sr", "n_fft", "hop", "n_mels", "win_length", "start_bpm", "std_bpm", "max_bpm"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [2048, 512, 128, 384, 120, 1, 320]


@pytest.mark.parametrize("struct,cls", [("jsg_onset_args", "OnsetArgs"), ("jsg_tempogram_args", "TempogramArgs"), ("jsg_tempo_args", "TempoArgs")])
def test_struct_layout_matches_the_header(jsg, tmp_path, struct, cls):
    import shutil
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsg.h")).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*$", piece).group(1) for decl in body.split(";") if decl.strip() for piece in decl.split(",")]
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "jsg.h"', "int main(void) {", f'    printf("%zu\\n", sizeof({struct}));']
    lines += [f'    printf("{f} %zu %zu\\n", offsetof({struct}, {f}), sizeof((({struct}*)0)->{f}));' for f in names]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)])
    out = subprocess.check_output([str(tmp_path / "layout")], text=True).split("\n")
    cls = getattr(jsg.capi, cls)
    assert out[0] == str(C.sizeof(cls))
    assert [f for f, _ in cls._fields_] == ["in_" if f == "in" else f for f in names]
    for (f, _), c_name, line in zip(cls._fields_, names, out[1:]):
        assert line == f"{c_name} {getattr(cls, f).offset} {getattr(cls, f).size}"


def test_kernel_notes(jsg, tmp_path):
    """No private segment (no scratch, no spills) in any kernel of the unit, static LDS only in the tempo kernel, and the unit's kernels are
    the ones the plan names."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    obj = os.path.join(ROOT, "jadespectrogram_amd", "build", "jsg_rhythm.o")
    if not os.path.exists(obj):
        from jadespectrogram_amd import _build
        _build.build_lib()
    co = kernel_regs.code_object(obj, str(tmp_path))
    notes = subprocess.check_output([os.path.join(kernel_regs.LLVM, "llvm-readelf"), "--notes", co]).decode()
    found = {}
    for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
        g = lambda k: re.search(rf"\.{k}:\s+(\S+)", blk).group(1)
        found[g("name")] = (int(g("private_segment_fixed_size")), int(g("group_segment_fixed_size")), int(g("vgpr_spill_count")), int(g("sgpr_spill_count")))
    assert len(found) == 7 and sum("tempogram_kernel" in k for k in found) == 4 and sum("onset_kernel" in k for k in found) == 2
    for name, (private, lds, vspill, sspill) in found.items():
        assert private == 0 and vspill == 0 and sspill == 0, name
        assert lds == (48 if "tempo_kernel" in name else 0), name               # the tempogram kernel's LDS is dynamic: jsg_tempogram_plan

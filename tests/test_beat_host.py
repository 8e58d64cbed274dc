"""The companion library libjsgx.so, host side (include/jsgx.h): every refusal of the beat tracker in its stated order (all decided
without a device), the logarithm table, the plan over every period, the scratch size, the exports, the struct layout, the library
boundary (libjsg.so stays as it is), the Python names, the kernel's notes, and the host entry points from a stand-alone C++ program under
the address and undefined-behaviour sanitizers.  CPU only."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import beat_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# never dereferenced: every call below is refused, sized or planned
IN, PERIOD, LOG, BEATS, NBEATS, LOCAL, CUM, SCRATCH = (i << 44 for i in range(1, 9))
BAD = -2


@pytest.fixture(scope="module")
def capix(jsg):
    if not os.path.exists(jsg.capix.LIB_PATH):
        from jadespectrogram_amd import _build
        _build.build_lib()
    jsg.capix.lib()
    return jsg.capix


def args(capix, **kw):
    a = dict(in_=IN, in_pitch=600, rows=2, n_frames=600, period=PERIOD, period_all=0, smooth=1, log_table=LOG, tightness=100.0, normalise=1, beats=BEATS,
             beats_pitch=600, max_beats=600, reserved0=0, n_beats=NBEATS, local_score=LOCAL, local_pitch=600, cum_score=CUM, cum_pitch=600)
    a.update(kw)
    return capix.BeatArgs(**a)


# in the order of the header: a call with two defects is refused for the earlier one
REFUSED = [
    ("null in", dict(in_=None), "null in"),
    ("null log_table", dict(log_table=None), "null log_table"),
    ("null beats", dict(beats=None), "null beats"),
    ("null n_beats", dict(n_beats=None), "null n_beats"),
    ("misaligned period", dict(period=PERIOD + 2), "pointers must be 4-byte aligned"),
    ("misaligned cum_score", dict(cum_score=CUM + 1), "pointers must be 4-byte aligned"),
    ("no rows", dict(rows=0), "rows must be in 1..65535"),
    ("65536 rows", dict(rows=65536), "rows must be in 1..65535"),
    ("no frames", dict(n_frames=0), "n_frames must be in 1..2^24"),
    ("2^24 + 1 frames", dict(n_frames=2 ** 24 + 1, in_pitch=2 ** 25, local_pitch=2 ** 25, cum_pitch=2 ** 25), "n_frames must be in 1..2^24"),
    ("scalar period 0", dict(period=None, period_all=0), "period_all must be in 1..1024 (period is null)"),
    ("scalar period 1025", dict(period=None, period_all=1025), "period_all must be in 1..1024 (period is null)"),
    ("tightness 0", dict(tightness=0.0), "tightness must be finite and > 0"),
    ("tightness nan", dict(tightness=float("nan")), "tightness must be finite and > 0"),
    ("tightness inf", dict(tightness=float("inf")), "tightness must be finite and > 0"),
    ("smooth 2", dict(smooth=2), "smooth must be 0 or 1"),
    ("normalise -1", dict(normalise=-1), "normalise must be 0 or 1"),
    ("max_beats 0", dict(max_beats=0), "max_beats must be in 1..2^24"),
    ("max_beats 2^24 + 1", dict(max_beats=2 ** 24 + 1, beats_pitch=2 ** 25), "max_beats must be in 1..2^24"),
    ("reserved0", dict(reserved0=1), "reserved0 must be 0"),
    ("in_pitch", dict(in_pitch=599), "in_pitch smaller than n_frames"),
    ("beats_pitch", dict(beats_pitch=599), "beats_pitch smaller than max_beats"),
    ("local_pitch", dict(local_pitch=599), "local_pitch smaller than n_frames"),
    ("cum_pitch", dict(cum_pitch=599), "cum_pitch smaller than n_frames"),
    ("n_beats inside in", dict(n_beats=IN + 4 * 700), "an output overlaps in"),
    ("beats end in period", dict(beats=PERIOD - 4 * 1200 + 4), "an output overlaps period"),
    ("local_score inside log_table", dict(local_score=LOG + 4 * 2048), "an output overlaps log_table"),
]
LAUNCH_ONLY = [
    ("null scratch", (None, 1 << 40), "null scratch"),
    ("misaligned scratch", (SCRATCH + 2, 1 << 40), "scratch must be 4-byte aligned"),
    ("short scratch", (SCRATCH, 2 * 4 * 2 * 600 - 1), "scratch smaller than jsgx_beat_scratch_bytes"),
]
CALLS = (("jsgx_beat_launch", lambda lib, a: lib.jsgx_beat_launch(C.byref(a), SCRATCH, 1 << 40, None)),
         ("jsgx_beat_scratch_bytes", lambda lib, a: lib.jsgx_beat_scratch_bytes(C.byref(a))),
         ("jsgx_beat_plan", lambda lib, a: lib.jsgx_beat_plan(C.byref(a), 47, None, 0, None, None)))


@pytest.mark.parametrize("i", range(len(REFUSED)), ids=[r[0] for r in REFUSED])
def test_refusals_in_their_order(capix, i):
    lib = capix.lib()
    _, change, message = REFUSED[i]
    a = args(capix, **change)
    for who, call in CALLS:
        assert call(lib, a) == BAD and lib.jsgx_last_error() == f"{who}: {message}".encode()
    # with any later defect on top, the earlier one is still the one reported -- also ahead of what only the launch refuses
    who, call = CALLS[0]
    for _, later, later_message in REFUSED[i + 1:]:
        if later_message == message or set(later) & set(change):
            continue
        assert call(lib, args(capix, **dict(later, **change))) == BAD
        assert lib.jsgx_last_error() == f"{who}: {message}".encode(), (REFUSED[i][0], later)
    assert lib.jsgx_beat_launch(C.byref(a), None, 0, None) == BAD and lib.jsgx_last_error() == f"jsgx_beat_launch: {message}".encode()


def test_what_only_the_launch_refuses_and_what_passes(capix):
    lib = capix.lib()
    a = args(capix)
    for k, (_, (scratch, size), message) in enumerate(LAUNCH_ONLY):
        assert lib.jsgx_beat_launch(C.byref(a), scratch, size, None) == BAD and lib.jsgx_last_error() == f"jsgx_beat_launch: {message}".encode()
    assert lib.jsgx_beat_launch(C.byref(a), None, 0, None) == BAD and lib.jsgx_last_error() == b"jsgx_beat_launch: null scratch"
    assert lib.jsgx_beat_launch(C.byref(a), SCRATCH + 1, 0, None) == BAD and lib.jsgx_last_error() == b"jsgx_beat_launch: scratch must be 4-byte aligned"
    for call in (lib.jsgx_beat_launch(None, SCRATCH, 1 << 40, None), lib.jsgx_beat_scratch_bytes(None), lib.jsgx_beat_plan(None, 47, None, 0, None, None)):
        assert call == BAD and lib.jsgx_last_error().endswith(b": null argument")
    with pytest.raises(capix.JsgError, match="null argument"):
        capix.check(lib.jsgx_beat_scratch_bytes(None))
    # one row: the pitches are not looked at; optional outputs may be missing; a device period makes period_all irrelevant
    ok = lambda **kw: lib.jsgx_beat_scratch_bytes(C.byref(args(capix, **kw)))
    assert ok(rows=1, in_pitch=0, beats_pitch=0, local_pitch=0, cum_pitch=0) == 2 * 4 * 600
    assert ok(local_score=None, cum_score=None, local_pitch=0, cum_pitch=0) == 2 * 4 * 2 * 600
    assert ok(period_all=-5) > 0 and ok(period=None, period_all=1) > 0 and ok(period=None, period_all=1024) > 0
    # an output next to an input, not inside it
    assert ok(n_beats=IN + 4 * 1200) > 0 and ok(beats=PERIOD - 4 * 1200) > 0 and ok(local_score=LOG + 4 * 2049) > 0


def test_scratch_bytes(capix):
    lib = capix.lib()
    for rows, T in ((1, 1), (2, 600), (8, 4096), (65535, 2 ** 24)):
        for smooth in (0, 1):
            a = args(capix, rows=rows, n_frames=T, in_pitch=T, beats_pitch=T, max_beats=T, local_pitch=T, cum_pitch=T, smooth=smooth)
            assert lib.jsgx_beat_scratch_bytes(C.byref(a)) == 4 * rows * T * (1 + smooth)


def test_no_device_comes_after_the_refusals(capix):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = capix.lib()
    assert lib.jsgx_beat_launch(C.byref(args(capix)), SCRATCH, 1 << 40, None) == capix.JSGX_ERR_NO_DEVICE
    assert lib.jsgx_last_error() == b"jsgx_beat_launch: no HIP device"
    assert lib.jsgx_beat_launch(C.byref(args(capix, rows=0)), SCRATCH, 1 << 40, None) == BAD
    assert lib.jsgx_beat_launch(C.byref(args(capix)), SCRATCH, 16, None) == BAD
    one = args(capix, rows=1, period=None, period_all=47, local_score=None, cum_score=None, smooth=0)
    assert lib.jsgx_beat_launch(C.byref(one), SCRATCH, 4 * 600, None) == capix.JSGX_ERR_NO_DEVICE


def test_log_table_against_numpy(jsg, capix):
    lib = capix.lib()
    full = jsg.beat_log_table()
    assert full.dtype == np.float32 and full.shape == (2049,) == (capix.BEAT_LOG_TABLE,)
    assert np.array_equal(full.view(np.uint32), br.log_table().view(np.uint32))
    for n in (1, 2, 1000):
        out = np.full(n + 2, -1.0, np.float32)
        assert lib.jsgx_log_table_build(n, out[1:].ctypes.data) == 0
        assert np.array_equal(out[1:n + 1].view(np.uint32), br.log_table()[:n].view(np.uint32)) and out[0] == -1 and out[-1] == -1
    out = np.zeros(4, np.float32)
    for n, message in ((0, "n must be in 1..2049"), (2050, "n must be in 1..2049"), (-1, "n must be in 1..2049")):
        assert lib.jsgx_log_table_build(n, out.ctypes.data) == BAD and lib.jsgx_last_error() == b"jsgx_log_table_build: " + message.encode()
    assert lib.jsgx_log_table_build(4, None) == BAD and lib.jsgx_last_error() == b"jsgx_log_table_build: null out"
    with pytest.raises(jsg.JsgError):
        jsg.beat_log_table(0)


def test_plan_over_every_period(jsg, capix):
    lib = capix.lib()
    a = args(capix)
    seen = {}
    for P in range(1, 1025):
        name, threads, lds = C.create_string_buffer(32), C.c_int32(-1), C.c_int32(-1)
        assert lib.jsgx_beat_plan(C.byref(a), P, name, 32, C.byref(threads), C.byref(lds)) == 0
        form = name.value.decode()
        assert form == ("beat_frames" if br.form(P)[1] == 1 else "beat_split")
        assert threads.value == 256 == capix.BEAT_THREADS and 0 < lds.value == capix.BEAT_LDS_BYTES <= 163840
        seen.setdefault(form, []).append(P)
    # the boundary between the two forms: a = (P + 1) // 2 reaches the 256 lanes at P = 511
    assert (seen["beat_split"][0], seen["beat_split"][-1], seen["beat_frames"][0], seen["beat_frames"][-1]) == (1, 510, 511, 1024)
    assert jsg.beat_plan(510) == ("beat_split", 256, capix.BEAT_LDS_BYTES) and jsg.beat_plan(511)[0] == "beat_frames"
    buf = C.create_string_buffer(32)
    for P in (0, -1, 1025):
        assert lib.jsgx_beat_plan(C.byref(a), P, buf, 32, None, None) == BAD and lib.jsgx_last_error() == b"jsgx_beat_plan: period must be in 1..1024"
    assert lib.jsgx_beat_plan(C.byref(a), 47, buf, 15, None, None) == BAD and lib.jsgx_last_error() == b"jsgx_beat_plan: bad argument"
    assert lib.jsgx_beat_plan(C.byref(a), 47, buf, 16, None, None) == 0 and buf.value == b"beat_split"
    with pytest.raises(jsg.JsgError):
        jsg.beat_plan(1025)


def test_exports_and_the_library_boundary(jsg, capix):
    """libjsgx.so exports exactly the functions of capix.SIGNATURES, all jsgx_*; libjsg.so, its header and its binding are as they were."""
    out = subprocess.check_output(["nm", "-D", "--defined-only", capix.LIB_PATH]).decode()
    functions = {line.split()[-1] for line in out.splitlines() if len(line.split()) == 3 and line.split()[1] == "T"} - {"_init", "_fini"}
    assert functions == set(capix.SIGNATURES) and all(f.startswith("jsgx_") for f in functions)
    hdr = open(os.path.join(ROOT, "include", "jsgx.h")).read()
    assert set(re.findall(r"\b(jsgx_\w+)\(", hdr)) - {"jsgx_exp"} == set(capix.SIGNATURES)       # jsgx_exp: the routine the comment states
    assert not re.search(r"\bjsg_\w+\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "#define JSGX_ABI_VERSION 1\n" in hdr and capix.lib().jsgx_abi_version() == 1 == capix.JSGX_ABI_VERSION
    assert "#define JSGX_BEAT_MAX_PERIOD 1024\n" in hdr and capix.BEAT_MAX_PERIOD == 1024
    assert f"#define JSGX_BEAT_LDS_BYTES {capix.BEAT_LDS_BYTES} " in hdr and f"#define JSGX_EXP_REL_BOUND {br.EXP_REL_BOUND:.1e} ".replace("e-07", "e-7") in hdr
    assert capix.EXP_REL_BOUND == br.EXP_REL_BOUND
    # the engine's library: 146 entry points, ABI 6, no word of the companion in its header
    assert len(jsg.capi.SIGNATURES) == 146 and not any(name.startswith("jsgx") for name in jsg.capi.SIGNATURES)
    assert "jsgx" not in open(os.path.join(ROOT, "include", "jsg.h")).read().lower()
    assert jsg.capi.lib().jsg_abi_version() == 6
    out = subprocess.check_output(["nm", "-D", "--defined-only", jsg.capi.LIB_PATH]).decode()
    assert "jsgx" not in out
    # libjsgx.so does not link against libjsg.so
    needed = subprocess.check_output(["readelf", "-d", capix.LIB_PATH]).decode()
    assert "libjsg.so" not in needed and "libamdhip64" in needed


def test_python_names(jsg):
    want = {
        "beat_log_table": ["n"],
        "beat_scratch_bytes": ["d_in", "d_log_table", "d_beats", "d_n_beats", "d_period", "period", "tightness", "smooth", "normalise", "max_beats", "d_local_score", "d_cum_score"],
        "beat_launch": ["d_in", "d_log_table", "d_beats", "d_n_beats", "d_period", "period", "tightness", "smooth", "normalise", "max_beats", "d_local_score", "d_cum_score",
                        "d_scratch", "stream"],
        "beat_plan": ["period", "n_frames", "rows"],
        "beat_track": ["onset_envelope", "period", "bpm", "frame_rate", "tightness", "smooth", "normalise", "max_beats"],
        "beat_track_audio": ["x", "sr", "n_fft", "hop", "n_mels", "win_length", "start_bpm", "std_bpm", "max_bpm", "tightness", "smooth", "normalise", "max_beats"],
    }
    for name, params in want.items():
        assert callable(getattr(jsg, name)) and name in jsg.__all__
        assert list(inspect.signature(getattr(jsg, name)).parameters) == params, name
    sig = inspect.signature(jsg.beat_track)
    assert [p.default for p in sig.parameters.values()][1:] == [None, None, None, 100.0, True, True, None]
    sig = inspect.signature(jsg.beat_track_audio)
    assert [p.default for p in sig.parameters.values()][2:5] == [2048, 512, 128]
    assert "capix" in jsg.__all__ and jsg.capix.JsgError is jsg.JsgError


def test_struct_layout_matches_the_header(capix, tmp_path):
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsgx.h")).read(), flags=re.S)
    body = re.search(r"typedef struct jsgx_beat_args \{(.*?)\} jsgx_beat_args;", hdr, flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*$", decl).group(1) for decl in body.split(";") if decl.strip()]
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "jsgx.h"', "int main(void) {", '    printf("%zu\\n", sizeof(jsgx_beat_args));']
    lines += [f'    printf("{f} %zu %zu\\n", offsetof(jsgx_beat_args, {f}), sizeof(((jsgx_beat_args*)0)->{f}));' for f in names]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)])
    out = subprocess.check_output([str(tmp_path / "layout")], text=True).split("\n")
    assert out[0] == str(C.sizeof(capix.BeatArgs))
    assert [f for f, _ in capix.BeatArgs._fields_] == ["in_" if f == "in" else f for f in names]
    for (f, _), c_name, line in zip(capix.BeatArgs._fields_, names, out[1:]):
        assert line == f"{c_name} {getattr(capix.BeatArgs, f).offset} {getattr(capix.BeatArgs, f).size}"


def test_kernel_notes(capix, tmp_path):
    """One kernel, no private segment (no scratch memory, no spills), and the static LDS the header and the plan state."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    obj = os.path.join(ROOT, "jadespectrogram_amd", "build", "jsgx_beat.o")
    if not os.path.exists(obj):
        from jadespectrogram_amd import _build
        _build.build_lib()
    co = kernel_regs.code_object(obj, str(tmp_path))
    notes = subprocess.check_output([os.path.join(kernel_regs.LLVM, "llvm-readelf"), "--notes", co]).decode()
    found = {}
    for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
        g = lambda k: re.search(rf"\.{k}:\s+(\S+)", blk).group(1)
        found[g("name")] = (int(g("private_segment_fixed_size")), int(g("group_segment_fixed_size")), int(g("vgpr_spill_count")), int(g("sgpr_spill_count")),
                            int(g("max_flat_workgroup_size")))
    assert len(found) == 1 and "beat_kernel" in next(iter(found))
    assert next(iter(found.values())) == (0, capix.BEAT_LDS_BYTES, 0, 0, capix.BEAT_THREADS)


def test_host_entry_points_under_asan_ubsan(capix):
    """tests/cpp/jsgx_beat_host_test.cpp (its own main: the table, the plan of every period, the scratch size, the refusals) built together
    with csrc/jsgx_beat_host.cpp under the address and undefined-behaviour sanitizers and run as a child process; the same program against
    the shipped library gives the same verdict."""
    d = tempfile.gettempdir()
    drv = os.path.join(ROOT, "tests", "cpp", "jsgx_beat_host_test.cpp")
    host = os.path.join(ROOT, "jadespectrogram_amd", "csrc", "jsgx_beat_host.cpp")
    common = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]
    san = os.path.join(d, "jsgx_beat_host_san")
    subprocess.check_call(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", host, drv, "-o", san])
    libdir = os.path.dirname(capix.LIB_PATH)
    shipped = os.path.join(d, "jsgx_beat_host_lib")
    subprocess.check_call(common + [drv, "-o", shipped, "-L", libdir, "-ljsgx", f"-Wl,-rpath,{libdir}"])
    for exe in (san, shipped):
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == "ok" and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr

"""Sections 15 and 16 of the companion library, host side (include/jsgx.h): every refusal of the segment aggregation and of the time-delay
embedding in its stated order (all decided without a device), what passes, the plan, the segment lengths of the GPU test against the
header's thresholds, the struct layouts against a C program, the header's constants, the exported symbols, the Python names, the kernels'
notes, and the host entry points from a stand-alone C++ program under the address and undefined-behaviour sanitizers.  CPU only."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import sync_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, F, M, S = 1000, 65, 40, 30
# never dereferenced: every call below is refused or planned
X, BOUNDS, N_BOUNDS, SEGMENTS, N_SEGMENTS, OUT = (i << 44 for i in range(1, 7))
BAD = -2
X_PAIR, OUT_PAIR = N * (F + 3) + 7, S * (F + 1) + 5
X_SPAN, OUT_SPAN, B_SPAN, SEG_SPAN = 2 * X_PAIR + (N - 1) * (F + 3) + F, 2 * OUT_PAIR + (S - 1) * (F + 1) + F, 2 * (M + 2) + M, 2 * (S + 3) + S + 1
STACK_OUT_PAIR = N * (5 * F + 1) + 5


@pytest.fixture(scope="module")
def capix(jsg):
    if not os.path.exists(jsg.capix.LIB_PATH):
        from jadespectrogram_amd import _build
        _build.build_lib()
    jsg.capix.lib()
    return jsg.capix


def sync_args(capix, **kw):       # 3 planes of 1000 frames of 65 features, 40 boundaries, 30 segments taken
    a = dict(x=X, x_frame_pitch=F + 3, x_pair_pitch=X_PAIR, bounds=BOUNDS, bounds_pitch=M + 2, n_bounds=N_BOUNDS, segments=SEGMENTS, segments_pitch=S + 3,
             n_segments=N_SEGMENTS, out=OUT, out_frame_pitch=F + 1, out_pair_pitch=OUT_PAIR, pairs=3, n_frames=N, n_features=F, max_bounds=M, bounds_all=0,
             max_segments=S, aggregate=3, pad=1)
    a.update(kw)
    return capix.SyncArgs(**a)


def stack_args(capix, **kw):
    a = dict(x=X, x_frame_pitch=F + 3, x_pair_pitch=X_PAIR, out=OUT, out_frame_pitch=5 * F + 1, out_pair_pitch=STACK_OUT_PAIR, pairs=3, n_frames=N, n_features=F,
             n_steps=5, delay=-3, mode=1, fill=1.5)
    a.update(kw)
    return capix.StackMemoryArgs(**a)


# in the order of the header: a call with two defects is refused for the earlier one
REFUSED = [
    ("null x", dict(x=None), "null x"),
    ("null out", dict(out=None), "null out"),
    ("null segments", dict(segments=None), "null segments"),
    ("null n_segments", dict(n_segments=None), "null n_segments"),
    ("null bounds", dict(bounds=None, max_bounds=M), "null bounds with max_bounds > 0"),
    ("misaligned x", dict(x=X + 2), "pointers must be 4-byte aligned"),
    ("misaligned n_bounds", dict(n_bounds=N_BOUNDS + 1), "pointers must be 4-byte aligned"),
    ("misaligned segments", dict(segments=SEGMENTS + 3), "pointers must be 4-byte aligned"),
    ("no pairs", dict(pairs=0), "pairs must be in 1..65535"),
    ("65536 pairs", dict(pairs=65536), "pairs must be in 1..65535"),
    ("no frames", dict(n_frames=0), "n_frames must be in 1..16777216"),
    ("too many frames", dict(n_frames=(1 << 24) + 1), "n_frames must be in 1..16777216"),
    ("no features", dict(n_features=0), "n_features must be in 1..65536"),
    ("too many features", dict(n_features=65537), "n_features must be in 1..65536"),
    ("negative max_bounds", dict(max_bounds=-1), "max_bounds must be in 0..1048576"),
    ("max_bounds", dict(max_bounds=(1 << 20) + 1), "max_bounds must be in 0..1048576"),
    ("bounds_all", dict(n_bounds=None, bounds_all=M + 1), "bounds_all must be in 0..max_bounds"),
    ("no max_segments", dict(max_segments=0), "max_segments must be in 1..1048577"),
    ("max_segments", dict(max_segments=(1 << 20) + 2), "max_segments must be in 1..1048577"),
    ("aggregate", dict(aggregate=4), "aggregate must be in 0..3"),
    ("negative aggregate", dict(aggregate=-1), "aggregate must be in 0..3"),
    ("pad", dict(pad=2), "pad must be 0 or 1"),
    ("reserved0", dict(reserved0=1), "reserved0 and reserved1 must be 0"),
    ("reserved1", dict(reserved1=1), "reserved0 and reserved1 must be 0"),
    ("x_frame_pitch", dict(x_frame_pitch=F - 1), "x_frame_pitch smaller than n_features"),
    ("x_pair_pitch", dict(x_pair_pitch=X_PAIR - 11), "x_pair_pitch does not cover a plane"),
    ("out_frame_pitch", dict(out_frame_pitch=F - 1), "out_frame_pitch smaller than n_features"),
    ("out_pair_pitch", dict(out_pair_pitch=(S - 1) * (F + 1) + F - 1), "out_pair_pitch does not cover a plane"),
    ("bounds_pitch", dict(bounds_pitch=M - 1), "bounds_pitch neither 0 nor >= max_bounds"),
    ("segments_pitch", dict(segments_pitch=S), "segments_pitch smaller than max_segments + 1"),
    ("out ends in x", dict(out=X - 4 * OUT_SPAN + 4), "out overlaps x"),
    ("out inside bounds", dict(out=BOUNDS + 4 * (B_SPAN - 1)), "out overlaps bounds"),
    ("out ends in n_bounds", dict(out=N_BOUNDS - 4 * OUT_SPAN + 4 * 3), "out overlaps n_bounds"),
    ("segments inside x", dict(segments=X + 4 * (X_SPAN - 1)), "segments overlaps x"),
    ("segments ends in bounds", dict(segments=BOUNDS - 4 * SEG_SPAN + 4), "segments overlaps bounds"),
    ("segments inside n_bounds", dict(segments=N_BOUNDS + 8), "segments overlaps n_bounds"),
    ("n_segments inside x", dict(n_segments=X + 4 * 1000), "n_segments overlaps x"),
    ("n_segments ends in bounds", dict(n_segments=BOUNDS - 8), "n_segments overlaps bounds"),
    ("n_segments is n_bounds", dict(n_segments=N_BOUNDS), "n_segments overlaps n_bounds"),
    ("segments inside out", dict(segments=OUT + 4 * (OUT_SPAN - 1)), "out overlaps segments"),
    ("n_segments inside out", dict(n_segments=OUT + 4 * 100), "out overlaps n_segments"),
    ("n_segments inside segments", dict(n_segments=SEGMENTS + 4 * (SEG_SPAN - 1)), "segments overlaps n_segments"),
]

STACK_REFUSED = [
    ("null x", dict(x=None), "null x"),
    ("null out", dict(out=None), "null out"),
    ("misaligned out", dict(out=OUT + 2), "pointers must be 4-byte aligned"),
    ("no pairs", dict(pairs=0), "pairs must be in 1..65535"),
    ("too many frames", dict(n_frames=(1 << 24) + 1), "n_frames must be in 1..16777216"),
    ("no features", dict(n_features=0), "n_features must be in 1..65536"),
    ("no steps", dict(n_steps=0), "n_steps must be in 1..256"),
    ("257 steps", dict(n_steps=257), "n_steps must be in 1..256"),
    ("too wide", dict(n_steps=17, n_features=65536), "n_steps * n_features must be at most 1048576"),
    ("no delay", dict(delay=0), "delay must be non-zero and within +-16777216"),
    ("a long delay", dict(delay=-(1 << 24) - 1), "delay must be non-zero and within +-16777216"),
    ("mode", dict(mode=2), "mode must be 0 or 1"),
    ("reserved0", dict(reserved0=1), "reserved0 must be 0"),
    ("x_frame_pitch", dict(x_frame_pitch=F - 1), "x_frame_pitch smaller than n_features"),
    ("x_pair_pitch", dict(x_pair_pitch=5), "x_pair_pitch does not cover a plane"),
    ("out_frame_pitch", dict(out_frame_pitch=5 * F - 1), "out_frame_pitch smaller than n_steps * n_features"),
    ("out_pair_pitch", dict(out_pair_pitch=(N - 1) * (5 * F + 1) + 5 * F - 1), "out_pair_pitch does not cover a plane"),
    ("out inside x", dict(out=X + 4 * (X_SPAN - 1)), "out overlaps x"),
]


def in_order(lib, table, call, who, i):
    _, change, message = table[i]
    assert call(change) == BAD and lib.jsgx_last_error() == f"{who}: {message}".encode(), lib.jsgx_last_error()
    # with any later defect on top, the earlier one is still the one reported
    for _, later, later_message in table[i + 1:]:
        if later_message == message or set(later) & set(change):
            continue
        assert call(dict(later, **change)) == BAD
        assert lib.jsgx_last_error() == f"{who}: {message}".encode(), (table[i][0], later)


@pytest.mark.parametrize("i", range(len(REFUSED)), ids=[r[0] for r in REFUSED])
def test_refusals_in_their_order(capix, i):
    lib = capix.lib()
    in_order(lib, REFUSED, lambda change: lib.jsgx_sync_launch(C.byref(sync_args(capix, **change)), None), "jsgx_sync_launch", i)
    in_order(lib, REFUSED, lambda change: lib.jsgx_sync_plan(C.byref(sync_args(capix, **change)), None, 0, None, None, None), "jsgx_sync_plan", i)


@pytest.mark.parametrize("i", range(len(STACK_REFUSED)), ids=[r[0] for r in STACK_REFUSED])
def test_stack_memory_refusals_in_their_order(capix, i):
    lib = capix.lib()
    in_order(lib, STACK_REFUSED, lambda change: lib.jsgx_stack_memory_launch(C.byref(stack_args(capix, **change)), None), "jsgx_stack_memory_launch", i)


def test_what_passes(capix):
    lib = capix.lib()
    ok = lambda **kw: lib.jsgx_sync_plan(C.byref(sync_args(capix, **kw)), None, 0, None, None, None)
    assert ok() == 0
    # a buffer next to another, not inside it
    assert ok(out=X - 4 * OUT_SPAN) == 0 and ok(out=X + 4 * X_SPAN) == 0 and ok(segments=BOUNDS + 4 * B_SPAN) == 0 and ok(n_segments=SEGMENTS + 4 * SEG_SPAN) == 0
    assert ok(n_segments=N_BOUNDS + 12) == 0 and ok(n_segments=N_BOUNDS - 12) == 0
    # no boundaries at all; one list for every pair; the count on the host; bounds_all not looked at with n_bounds
    assert ok(bounds=None, max_bounds=0) == 0 and ok(bounds_pitch=0) == 0 and ok(n_bounds=None, bounds_all=M) == 0 and ok(n_bounds=None, bounds_all=0) == 0
    assert ok(bounds_all=-5) == 0
    # one pair: no pair pitch is looked at; the ends of the ranges
    assert ok(pairs=1, x_pair_pitch=0, out_pair_pitch=0, bounds_pitch=0, segments_pitch=0) == 0
    assert ok(aggregate=0, pad=0, max_segments=1, out_pair_pitch=F, segments_pitch=2) == 0
    assert ok(max_bounds=1 << 20, bounds_pitch=1 << 20, max_segments=(1 << 20) + 1, segments_pitch=(1 << 20) + 2, out_pair_pitch=((1 << 20) + 1) * (F + 1), out=1 << 58) == 0
    for call in (lib.jsgx_sync_launch(None, None), lib.jsgx_sync_plan(None, None, 0, None, None, None), lib.jsgx_stack_memory_launch(None, None)):
        assert call == BAD and lib.jsgx_last_error().endswith(b": null argument")
    assert lib.jsgx_sync_plan(C.byref(sync_args(capix)), C.create_string_buffer(15), 15, None, None, None) == BAD
    assert lib.jsgx_last_error() == b"jsgx_sync_plan: bad argument"
    import torch
    if torch.cuda.is_available():           # with a device the calls below would launch on pointers that are no memory
        return
    NO_DEVICE = capix.JSGX_ERR_NO_DEVICE
    assert lib.jsgx_sync_launch(C.byref(sync_args(capix)), None) == NO_DEVICE and lib.jsgx_last_error() == b"jsgx_sync_launch: no HIP device"
    assert lib.jsgx_sync_launch(C.byref(sync_args(capix, bounds=None, max_bounds=0, pad=0)), None) == NO_DEVICE
    stack = lambda **kw: lib.jsgx_stack_memory_launch(C.byref(stack_args(capix, **kw)), None)
    assert stack() == NO_DEVICE and lib.jsgx_last_error() == b"jsgx_stack_memory_launch: no HIP device"
    assert stack(out=X + 4 * X_SPAN) == NO_DEVICE and stack(pairs=1, x_pair_pitch=0, out_pair_pitch=0) == NO_DEVICE
    assert stack(delay=1 << 24, n_steps=256, n_features=4096, x_frame_pitch=4096, x_pair_pitch=N * 4096, out_frame_pitch=1 << 20, out_pair_pitch=N << 20, out=1 << 58) == NO_DEVICE
    assert stack(mode=0, fill=float("nan"), n_steps=1, delay=-(1 << 24)) == NO_DEVICE


def test_the_plan_and_the_constants(jsg, capix):
    names = {"mean": "sync_mean", "min": "sync_min", "max": "sync_max", "median": "sync_median"}
    for frames in (1, 64, 1025, 1 << 24):
        for feats in (1, 65, 65536):
            for P in (1, 3, 65535):
                for bounds in (0, 1, 700, 1 << 20):
                    for pad in (False, True):
                        for agg, name in names.items():
                            lds = capix.SYNC_LDS_BYTES + (capix.SYNC_LDS_TILE if agg == "median" else 0)
                            assert jsg.sync_plan(frames, feats, agg, P, bounds, pad) == (name, capix.SYNC_THREADS, lds, 2 if bounds + 2 * pad >= 2 else 1)
    hdr = open(os.path.join(ROOT, "include", "jsgx.h")).read()
    for name, value in (("JSGX_SYNC_MEAN", 0), ("JSGX_SYNC_MIN", 1), ("JSGX_SYNC_MAX", 2), ("JSGX_SYNC_MEDIAN", 3), ("JSGX_SYNC_CHUNK", capix.SYNC_CHUNK),
                        ("JSGX_SYNC_WAVE_MAX", capix.SYNC_WAVE_MAX), ("JSGX_SYNC_STAGE", capix.SYNC_STAGE), ("JSGX_SYNC_THREADS", capix.SYNC_THREADS),
                        ("JSGX_SYNC_MAX_FRAMES", capix.SYNC_MAX_FRAMES), ("JSGX_SYNC_MAX_FEATURES", capix.SYNC_MAX_FEATURES), ("JSGX_SYNC_MAX_BOUNDS", capix.SYNC_MAX_BOUNDS),
                        ("JSGX_SYNC_MAX_SEGMENTS", capix.SYNC_MAX_SEGMENTS), ("JSGX_SYNC_LDS_BYTES", capix.SYNC_LDS_BYTES), ("JSGX_SYNC_LDS_TILE", capix.SYNC_LDS_TILE),
                        ("JSGX_STACK_CONSTANT", 0), ("JSGX_STACK_EDGE", 1), ("JSGX_STACK_MAX_STEPS", capix.STACK_MAX_STEPS), ("JSGX_STACK_MAX_DELAY", capix.STACK_MAX_DELAY),
                        ("JSGX_STACK_MAX_WIDTH", capix.STACK_MAX_WIDTH), ("JSGX_STACK_THREADS", capix.STACK_THREADS), ("JSGX_ABI_VERSION", 1)):
        assert re.search(rf"#define {name} {value}\b", hdr), name
    assert "#define JSGX_SYNC_NAN_BITS 0x7FC00000u" in hdr and capix.SYNC_NAN_BITS == sr.NAN_BITS == 0x7FC00000
    assert (capix.SYNC_CHUNK, capix.SYNC_WAVE_MAX, capix.SYNC_STAGE) == (sr.CHUNK, sr.WAVE_MAX, sr.STAGE)
    assert (capix.SYNC_MEAN, capix.SYNC_MIN, capix.SYNC_MAX, capix.SYNC_MEDIAN) == (sr.MEAN, sr.MIN, sr.MAX, sr.MEDIAN) and (capix.STACK_CONSTANT, capix.STACK_EDGE) == (sr.CONSTANT, sr.EDGE)
    assert capix.SYNC_LDS_TILE == 4 * 64 * capix.SYNC_STAGE and 4 * capix.SYNC_WAVE_MAX <= capix.SYNC_STAGE and capix.SYNC_LDS_BYTES + capix.SYNC_LDS_TILE <= 163840
    for kernel in ("sync_segments", "sync_aggregate", "stack_memory", "sync_mean", "sync_min", "sync_max", "sync_median"):
        assert f'"{kernel}"' in hdr
    assert capix.lib().jsgx_abi_version() == 1


def test_the_gpu_lengths_straddle_every_threshold(capix):
    """The form that serves a segment depends on its length alone (and on its neighbours' in the workgroup): every JSGX_SYNC_* length at
    which the kernel changes its way is in the GPU test's list with its successor, and so are the lengths the contract names."""
    thresholds = {capix.SYNC_CHUNK, capix.SYNC_WAVE_MAX, capix.SYNC_STAGE}
    assert set(sr.THRESHOLDS) == thresholds
    for t in thresholds:
        assert {t, t + 1} <= set(sr.LENGTHS), t
    assert {1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 512, 513} <= set(sr.LENGTHS)
    assert max(sr.LENGTHS) > 2 * capix.SYNC_CHUNK and sr.WHOLE > 4 * capix.SYNC_CHUNK          # a third chunk, and a second round of the four wavefronts
    assert set(sr.N_SET) == {1, 63, 64, 65, 257, 1025} and set(sr.F_SET) == {1, 63, 64, 65, 130}


def test_struct_layouts_match_the_header(capix, tmp_path):
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsgx.h")).read(), flags=re.S)
    for struct, ctype, size in (("jsgx_sync_args", capix.SyncArgs, 136), ("jsgx_stack_memory_args", capix.StackMemoryArgs, 80)):
        body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", hdr, flags=re.S).group(1)
        names = [re.search(r"(\w+)\s*(\[\d+\])?\s*$", decl).group(1) for decl in body.split(";") if decl.strip()]
        lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "jsgx.h"', "int main(void) {", f'    printf("%zu\\n", sizeof({struct}));']
        lines += [f'    printf("{f} %zu %zu\\n", offsetof({struct}, {f}), sizeof((({struct}*)0)->{f}));' for f in names]
        src = tmp_path / f"{struct}.c"
        src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / struct), str(src)])
        out = subprocess.check_output([str(tmp_path / struct)], text=True).split("\n")
        assert out[0] == str(C.sizeof(ctype)) == str(size)
        assert [f for f, _ in ctype._fields_] == names
        offset = 0
        for (f, _), name, line in zip(ctype._fields_, names, out[1:]):
            assert line == f"{name} {getattr(ctype, f).offset} {getattr(ctype, f).size}"
            assert getattr(ctype, f).offset == offset, f"padding in front of {f}"
            offset += getattr(ctype, f).size
        assert offset == size          # none behind the last field either


def test_python_names(jsg):
    want = {
        "sync_launch": ["d_x", "d_bounds", "d_n_bounds", "d_segments", "d_n_segments", "d_out", "aggregate", "pad", "bounds_all", "stream"],
        "sync_plan": ["n_frames", "n_features", "aggregate", "pairs", "max_bounds", "pad"],
        "sync": ["data", "idx", "aggregate", "pad", "n_idx", "max_segments"],
        "stack_memory_launch": ["d_x", "d_out", "n_steps", "delay", "mode", "constant_values", "stream"],
        "stack_memory": ["data", "n_steps", "delay", "mode", "constant_values"],
        "beat_sync_audio": ["x", "sr", "n_fft", "hop", "n_mels", "aggregate", "pad", "kw"],
    }
    for name, params in want.items():
        assert callable(getattr(jsg, name)) and name in jsg.__all__
        assert list(inspect.signature(getattr(jsg, name)).parameters) == params, name
    assert [p.default for p in inspect.signature(jsg.sync).parameters.values()][2:] == ["mean", True, None, None]
    assert [p.default for p in inspect.signature(jsg.stack_memory).parameters.values()][1:] == [2, 1, "constant", 0.0]
    assert inspect.signature(jsg.beat_sync_audio).parameters["aggregate"].default == "median"
    for fn in (jsg.sync, jsg.stack_memory):          # the deliberate differences are stated, and that librosa itself was not run
        doc = " ".join(fn.__doc__.split())
        assert "frame-major" in doc and "float32" in doc and "Agreement with librosa itself was not measured" in doc
    doc = " ".join(jsg.sync.__doc__.split())
    assert "clipped" in doc and "non-decreasing" in doc and "librosa sorts" in doc and '"mean", "min", "max", "median"' in doc
    with pytest.raises(jsg.JsgError):
        jsg.spectrogram._host_segments([5, 3], 10, True)
    c, u = jsg.spectrogram._host_segments([-4, 2, 2, 7, 99], 10, True)
    assert c.tolist() == [0, 2, 2, 7, 10] and u.tolist() == sr.segments([-4, 2, 2, 7, 99], 5, 10, True)[1].tolist() == [0, 2, 7, 10]
    assert jsg.spectrogram._host_segments([], 10, False)[1].size == 0 and jsg.spectrogram._host_segments([], 10, True)[1].tolist() == [0, 10]
    symbols = {"jsgx_sync_launch", "jsgx_sync_plan", "jsgx_stack_memory_launch"}
    assert symbols <= set(jsg.capix.SIGNATURES)
    assert shutil.which("nm"), "nm (binutils) lists the exported symbols"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", jsg.capix.LIB_PATH], text=True)
    functions = {line.split()[-1] for line in exported.splitlines() if " T " in line}
    assert symbols <= functions and functions == set(jsg.capix.SIGNATURES)


def test_kernel_notes(capix, tmp_path):
    """The new object: its six kernels (the aggregate once for each of the four), no private segment (no scratch memory, no spills), the
    static LDS the header states (the median's tile is dynamic and not in the notes), workgroups of 256 lanes."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    obj = os.path.join(ROOT, "jadespectrogram_amd", "build", "jsgx_sync.o")
    if not os.path.exists(obj):
        from jadespectrogram_amd import _build
        _build.build_lib()
    co = kernel_regs.code_object(obj, str(tmp_path))
    notes = subprocess.check_output([os.path.join(kernel_regs.LLVM, "llvm-readelf"), "--notes", co]).decode()
    found = {}
    for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
        g = lambda k: re.search(rf"\.{k}:\s+(\S+)", blk).group(1)
        name = subprocess.check_output(["c++filt", g("name")]).decode().strip()
        found[name.split("(anonymous namespace)::")[1].split("(")[0]] = (int(g("private_segment_fixed_size")), int(g("group_segment_fixed_size")), int(g("vgpr_spill_count")),
                                                                         int(g("sgpr_spill_count")), int(g("max_flat_workgroup_size")))
        assert int(g("vgpr_count")) <= 128, name           # four wavefronts of a SIMD keep their registers
    aggregate = (0, capix.SYNC_LDS_BYTES, 0, 0, capix.SYNC_THREADS)
    assert found == {"sync_segments_kernel": (0, 48, 0, 0, capix.SYNC_THREADS), "stack_memory_kernel": (0, 0, 0, 0, capix.STACK_THREADS),
                     **{f"sync_aggregate_kernel<{a}>": aggregate for a in range(4)}}
    with open(os.path.join(ROOT, "tools", "kernel_regs.py")) as f:
        text = f.read()
    assert all(k in text for k in ("sync_segments_kernel", "sync_aggregate_kernel", "stack_memory_kernel", "jsgx_sync.o"))


def test_host_entry_points_under_asan_ubsan(capix):
    """tests/cpp/jsgx_sync_host_test.cpp (its own main: the refusals of both sections in their order, the plan over shapes up to the limits,
    planes more than 2^31 elements apart) built together with the host units it calls under the address and undefined-behaviour
    sanitizers and run as a child process; the same program against the shipped library, there with the refusals of the launches, gives
    the same verdict."""
    d = tempfile.gettempdir()
    drv = os.path.join(ROOT, "tests", "cpp", "jsgx_sync_host_test.cpp")
    hosts = [os.path.join(ROOT, "jadespectrogram_amd", "csrc", f) for f in ("jsgx_beat_host.cpp", "jsgx_sync_host.cpp")]
    common = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]
    san = os.path.join(d, "jsgx_sync_host_san")
    subprocess.check_call(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"] + hosts + [drv, "-o", san])
    libdir = os.path.dirname(capix.LIB_PATH)
    shipped = os.path.join(d, "jsgx_sync_host_lib")
    subprocess.check_call(common + ["-DJSGX_SYNC_TEST_LAUNCHES", drv, "-o", shipped, "-L", libdir, "-ljsgx", f"-Wl,-rpath,{libdir}"])
    for exe in (san, shipped):
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == "ok" and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr

"""Section 14 of the companion library, host side (include/jsgx.h): every refusal of the peak picking in its stated order (all decided
without a device), what passes, the plan and the scratch arithmetic up to the limits, the forms the plan can return against the shape
list of the GPU test, the struct layout against a C program, the header's constants, the exported symbols, the Python names, the kernels'
notes, and the host entry points from a stand-alone C++ program under the address and undefined-behaviour sanitizers.  CPU only."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import peak_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = pr.BLOCK
T = 2 * B + 5
# never dereferenced: every call below is refused or planned
IN, ENERGY, CAND, PEAKS, BACK, N_PEAKS, SCRATCH = (i << 44 for i in range(1, 8))
BAD = -2
NEED = 3 * 3 * (32 + 4 * 4 + B)            # three rows of three blocks, four entering offsets
IN_SPAN, ENERGY_SPAN, PEAKS_SPAN, CAND_SPAN = 2 * (T + 3) + T, 2 * (T + 1) + T, 2 * 104 + 100, 2 * (T + 2) + T
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def capix(jsg):
    if not os.path.exists(jsg.capix.LIB_PATH):
        from jadespectrogram_amd import _build
        _build.build_lib()
    jsg.capix.lib()
    return jsg.capix


def peak_args(capix, **kw):       # 3 rows of 2B + 5 frames, every optional buffer given
    a = dict(in_=IN, in_pitch=T + 3, energy=ENERGY, energy_pitch=T + 1, candidate=CAND, candidate_pitch=T + 2, peaks=PEAKS, backtracked=BACK, peaks_pitch=104,
             n_peaks=N_PEAKS, rows=3, n_frames=T, pre_max=3, post_max=1, pre_avg=5, post_avg=5, delta=0.07, wait=3, normalise=1, max_peaks=100)
    a.update(kw)
    return capix.PeakArgs(**a)


# in the order of the header: a call with two defects is refused for the earlier one.  "scratch" and "scratch_bytes" are the launch's own.
REFUSED = [
    ("null in", dict(in_=None), "null in"),
    ("null peaks", dict(peaks=None), "null peaks"),
    ("null n_peaks", dict(n_peaks=None), "null n_peaks"),
    ("misaligned in", dict(in_=IN + 2), "pointers must be 4-byte aligned"),
    ("misaligned energy", dict(energy=ENERGY + 1), "pointers must be 4-byte aligned"),
    ("misaligned backtracked", dict(backtracked=BACK + 3), "pointers must be 4-byte aligned"),
    ("no rows", dict(rows=0), "rows must be in 1..65535"),
    ("65536 rows", dict(rows=65536), "rows must be in 1..65535"),
    ("no frames", dict(n_frames=0), "n_frames must be in 1..16777216"),
    ("too many frames", dict(n_frames=(1 << 24) + 1), "n_frames must be in 1..16777216"),
    ("pre_max", dict(pre_max=257), "pre_max must be in 0..256"),
    ("negative post_max", dict(post_max=-1), "post_max must be in 0..256"),
    ("pre_avg", dict(pre_avg=1000), "pre_avg must be in 0..256"),
    ("post_avg", dict(post_avg=257), "post_avg must be in 0..256"),
    ("delta a NaN", dict(delta=NAN), "delta must be finite"),
    ("infinite delta", dict(delta=-INF), "delta must be finite"),
    ("negative wait", dict(wait=-1), "wait must be in 0..16777216"),
    ("wait", dict(wait=(1 << 24) + 1), "wait must be in 0..16777216"),
    ("normalise", dict(normalise=2), "normalise must be 0 or 1"),
    ("no max_peaks", dict(max_peaks=0), "max_peaks must be in 1..16777216"),
    ("max_peaks", dict(max_peaks=(1 << 24) + 1), "max_peaks must be in 1..16777216"),
    ("backtracked without energy", dict(energy=None), "energy and backtracked go together"),
    ("energy without backtracked", dict(backtracked=None), "energy and backtracked go together"),
    ("in_pitch", dict(in_pitch=T - 1), "in_pitch smaller than n_frames"),
    ("energy_pitch", dict(energy_pitch=T - 1), "energy_pitch smaller than n_frames"),
    ("candidate_pitch", dict(candidate_pitch=0), "candidate_pitch smaller than n_frames"),
    ("peaks_pitch", dict(peaks_pitch=99), "peaks_pitch smaller than max_peaks"),
    ("peaks ends in in", dict(peaks=IN - 4 * PEAKS_SPAN + 4), "peaks overlaps in"),
    ("peaks inside energy", dict(peaks=ENERGY + 4 * (ENERGY_SPAN - 1)), "peaks overlaps energy"),
    ("backtracked inside in", dict(backtracked=IN + 4 * 1000), "backtracked overlaps in"),
    ("backtracked is energy", dict(backtracked=ENERGY), "backtracked overlaps energy"),
    ("n_peaks inside in", dict(n_peaks=IN + 4 * (IN_SPAN - 1)), "n_peaks overlaps in"),
    ("n_peaks ends in energy", dict(n_peaks=ENERGY - 8), "n_peaks overlaps energy"),
    ("candidate inside in", dict(candidate=IN + 4 * IN_SPAN - 1), "candidate overlaps in"),
    ("candidate ends in energy", dict(candidate=ENERGY - CAND_SPAN + 1), "candidate overlaps energy"),
    ("backtracked inside peaks", dict(backtracked=PEAKS + 4 * (PEAKS_SPAN - 1)), "peaks overlaps backtracked"),
    ("n_peaks inside peaks", dict(n_peaks=PEAKS + 4 * 50), "peaks overlaps n_peaks"),
    ("candidate ends in peaks", dict(candidate=PEAKS - CAND_SPAN + 1), "peaks overlaps candidate"),
    ("n_peaks ends in backtracked", dict(n_peaks=BACK - 8), "backtracked overlaps n_peaks"),
    ("candidate inside backtracked", dict(candidate=BACK + 4 * PEAKS_SPAN - 1), "backtracked overlaps candidate"),
    ("candidate inside n_peaks", dict(candidate=N_PEAKS + 11), "n_peaks overlaps candidate"),
    ("null scratch", dict(scratch=None), "null scratch"),
    ("misaligned scratch", dict(scratch=SCRATCH + 2), "scratch must be 4-byte aligned"),
    ("small scratch", dict(scratch_bytes=NEED - 1), "scratch smaller than jsgx_peak_scratch_bytes"),
    ("scratch ends in in", dict(scratch=IN - NEED + 4), "scratch overlaps in"),
    ("scratch inside energy", dict(scratch=ENERGY + 4 * (ENERGY_SPAN - 1)), "scratch overlaps energy"),
    ("scratch inside peaks", dict(scratch=PEAKS + 4 * 5), "scratch overlaps peaks"),
    ("scratch inside backtracked", dict(scratch=BACK + 4 * (PEAKS_SPAN - 1)), "scratch overlaps backtracked"),
    ("scratch inside n_peaks", dict(scratch=N_PEAKS + 8), "scratch overlaps n_peaks"),
    ("scratch ends in candidate", dict(scratch=CAND - NEED + 4), "scratch overlaps candidate"),
]


def launch(lib, capix, change):
    change = dict(change)
    scratch, scratch_bytes = change.pop("scratch", SCRATCH), change.pop("scratch_bytes", NEED)
    return lib.jsgx_peak_launch(C.byref(peak_args(capix, **change)), scratch, scratch_bytes, None)


@pytest.mark.parametrize("i", range(len(REFUSED)), ids=[r[0] for r in REFUSED])
def test_refusals_in_their_order(capix, i):
    lib = capix.lib()
    _, change, message = REFUSED[i]
    assert launch(lib, capix, change) == BAD and lib.jsgx_last_error() == f"jsgx_peak_launch: {message}".encode(), lib.jsgx_last_error()
    if not set(change) & {"scratch", "scratch_bytes"}:          # what the launch refuses before it looks at the scratch, the other two calls refuse alike
        a = peak_args(capix, **change)
        assert lib.jsgx_peak_plan(C.byref(a), None, 0, None, None, None, None) == BAD and lib.jsgx_last_error() == f"jsgx_peak_plan: {message}".encode()
        assert lib.jsgx_peak_scratch_bytes(C.byref(a)) == BAD and lib.jsgx_last_error() == f"jsgx_peak_scratch_bytes: {message}".encode()
    # with any later defect on top, the earlier one is still the one reported
    for _, later, later_message in REFUSED[i + 1:]:
        if later_message == message or set(later) & set(change):
            continue
        assert launch(lib, capix, dict(later, **change)) == BAD
        assert lib.jsgx_last_error() == f"jsgx_peak_launch: {message}".encode(), (REFUSED[i][0], later)


def test_what_passes(capix):
    lib = capix.lib()
    size = lambda **kw: lib.jsgx_peak_scratch_bytes(C.byref(peak_args(capix, **kw)))
    assert size() == NEED
    # a buffer next to another, not inside it; candidate is bytes and may lie anywhere
    assert size(peaks=IN - 4 * PEAKS_SPAN) == NEED and size(n_peaks=IN + 4 * IN_SPAN) == NEED and size(candidate=IN + 4 * IN_SPAN) == NEED
    assert size(backtracked=PEAKS + 4 * PEAKS_SPAN) == NEED and size(candidate=N_PEAKS + 12) == NEED and size(candidate=CAND + 1) == NEED
    assert size(energy=IN) == NEED          # the envelope as its own energy: two inputs
    # the optional buffers absent: their pitches are not looked at; one row: no pitch is; the ends of the ranges
    assert size(energy=None, backtracked=None, candidate=None, energy_pitch=0, candidate_pitch=0) == NEED
    assert size(rows=1, in_pitch=0, energy_pitch=0, candidate_pitch=0, peaks_pitch=0) == NEED // 3
    assert size(pre_max=256, post_max=256, pre_avg=256, post_avg=256, delta=-3e38, normalise=0, max_peaks=1 << 24, peaks_pitch=1 << 24) == NEED
    assert size(pre_max=0, post_max=0, pre_avg=0, post_avg=0, wait=0) == 3 * 3 * (32 + 4 + B) and size(wait=1 << 24) == 3 * 3 * (32 + 4 * B + B)
    assert size(n_frames=B) == 0 and size(n_frames=B + 1) == 3 * 2 * (32 + 16 + B) and size(n_frames=1) == 0
    for call in (lib.jsgx_peak_launch(None, SCRATCH, NEED, None), lib.jsgx_peak_plan(None, None, 0, None, None, None, None), lib.jsgx_peak_scratch_bytes(None)):
        assert call == BAD and lib.jsgx_last_error().endswith(b": null argument")
    assert lib.jsgx_peak_plan(C.byref(peak_args(capix)), C.create_string_buffer(15), 15, None, None, None, None) == BAD
    assert lib.jsgx_last_error() == b"jsgx_peak_plan: bad argument"
    import torch
    if torch.cuda.is_available():           # with a device the calls below would launch on pointers that are no memory
        return
    NO_DEVICE = capix.JSGX_ERR_NO_DEVICE
    assert launch(lib, capix, {}) == NO_DEVICE and lib.jsgx_last_error() == b"jsgx_peak_launch: no HIP device"
    # a larger scratch, one that touches no buffer, and none where a row is one block
    assert launch(lib, capix, dict(scratch_bytes=NEED + 4096)) == NO_DEVICE and launch(lib, capix, dict(scratch=IN - NEED)) == NO_DEVICE
    assert launch(lib, capix, dict(n_frames=B, scratch=None, scratch_bytes=0)) == NO_DEVICE
    assert launch(lib, capix, dict(n_frames=200, scratch=IN + 2, scratch_bytes=-1)) == NO_DEVICE          # not looked at


def test_the_plan_and_the_scratch_over_shapes(jsg, capix):
    for frames in (1, 2, 64, 65, B - 1, B, B + 1, 2 * B, 3 * B + 7, 1 << 24):
        for R in (1, 3, 65535):
            for wait in (0, 1, B - 2, B - 1, B, 1 << 24):
                blocks = -(-frames // B)
                assert jsg.peak_plan(frames, R, wait) == ("peak_single" if blocks == 1 else "peak_blocked", capix.PEAK_THREADS, capix.PEAK_LDS_BYTES, 1 if blocks == 1 else 5, blocks)
                a = capix.PeakArgs(in_=1 << 50, in_pitch=frames, peaks=1 << 58, peaks_pitch=7, n_peaks=1 << 40, rows=R, n_frames=frames, wait=wait, max_peaks=7)
                need = capix.lib().jsgx_peak_scratch_bytes(C.byref(a))
                assert need == (0 if blocks == 1 else R * blocks * (32 + 4 * min(wait + 1, B) + B))
                assert need <= R * (16 * frames + 32 * blocks)          # what the header promises
    hdr = open(os.path.join(ROOT, "include", "jsgx.h")).read()
    for name, value in (("JSGX_PEAK_BLOCK", capix.PEAK_BLOCK), ("JSGX_PEAK_MAX_REACH", capix.PEAK_MAX_REACH), ("JSGX_PEAK_MAX_FRAMES", capix.PEAK_MAX_FRAMES),
                        ("JSGX_PEAK_THREADS", capix.PEAK_THREADS), ("JSGX_PEAK_SHORT", capix.PEAK_SHORT), ("JSGX_PEAK_LDS_LIMIT", capix.PEAK_LDS_LIMIT), ("JSGX_ABI_VERSION", 1)):
        assert re.search(rf"#define {name} {value}\b", hdr), name
    assert "#ifndef JSGX_PEAK_BLOCK" in hdr
    assert (capix.PEAK_BLOCK, capix.PEAK_MAX_REACH, capix.PEAK_MAX_FRAMES, capix.PEAK_SHORT) == (pr.BLOCK, pr.MAX_REACH, pr.MAX_FRAMES, pr.SHORT)
    assert capix.PEAK_LDS_BYTES == 2 * B * (B.bit_length() - 1) + 2 * (B + 4) + 2 * B <= capix.PEAK_LDS_LIMIT == 163840
    assert f"{capix.PEAK_LDS_BYTES} bytes at B = {B}" in hdr
    for kernel in ("peak_single", "peak_blocked", "peak_stats", "peak_row", "peak_cand", "peak_carry", "peak_emit"):
        assert f'"{kernel}"' in hdr
    assert capix.lib().jsgx_abi_version() == 1


def test_the_gpu_shapes_cover_every_form(capix):
    """The form is a function of the frame count alone (not of the rows, the wait or the reaches); a listed shape runs each form, both
    sides of the change between them are listed, and so are both sides of the count up to which a wavefront takes a row."""
    lib = capix.lib()
    name, launches, blocks = C.create_string_buffer(16), C.c_int32(), C.c_int32()
    a = peak_args(capix, energy=None, backtracked=None, candidate=None)

    def form(R, frames, wait=3, reach=3):
        a.rows, a.n_frames, a.in_pitch, a.wait, a.pre_max, a.post_avg = R, frames, frames, wait, reach, reach
        assert lib.jsgx_peak_plan(C.byref(a), name, 16, None, None, C.byref(launches), C.byref(blocks)) == 0, lib.jsgx_last_error()
        return name.value.decode(), launches.value

    by_T = {frames: form(1, frames) for frames in range(1, max(pr.T_SET) + 1)}
    for R in pr.ROWS_SET + (300,):
        for wait in (0, 5, B, 1 << 24):
            for reach in (0, 256):
                for frames in (1, 64, 65, B, B + 1, 3 * B + 7):
                    assert form(R, frames, wait, reach) == by_T[frames]
    listed = {s[1] for s in pr.SHAPES}
    assert set(by_T.values()) == {form(*s) for s in pr.SHAPES} == {("peak_single", 1), ("peak_blocked", 5)}, "a form no listed shape runs"
    changes = [frames for frames in range(2, max(pr.T_SET) + 1) if by_T[frames] != by_T[frames - 1]]
    assert changes == [B + 1] and all(frames in listed and frames - 1 in listed for frames in changes)
    assert {pr.SHORT, pr.SHORT + 1} <= listed and pr.MANY_SHORT[1] <= pr.SHORT and pr.MANY_SHORT[0] > 256          # short rows by the hundred: a wavefront a row
    assert {B - 1, 2 * B, 2 * B + 1} <= listed and max(listed) > 3 * B and max(listed) % B
    assert set(pr.ROWS_SET) == {s[0] for s in pr.SHAPES}


def test_struct_layout_matches_the_header(capix, tmp_path):
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler")
    struct, ctype = "jsgx_peak_args", capix.PeakArgs
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsgx.h")).read(), flags=re.S)
    body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", hdr, flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*(\[\d+\])?\s*$", decl).group(1) for decl in body.split(";") if decl.strip()]
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "jsgx.h"', "int main(void) {", f'    printf("%zu\\n", sizeof({struct}));']
    lines += [f'    printf("{f} %zu %zu\\n", offsetof({struct}, {f}), sizeof((({struct}*)0)->{f}));' for f in names]
    lines += ['    printf("%d %d\\n", JSGX_PEAK_LDS_BYTES, JSGX_PEAK_LOG2_BLOCK);']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)])
    out = subprocess.check_output([str(tmp_path / "layout")], text=True).split("\n")
    assert out[0] == str(C.sizeof(ctype)) == "120"
    assert [f for f, _ in ctype._fields_] == ["in_" if f == "in" else f for f in names]
    offset = 0
    for (f, _), name, line in zip(ctype._fields_, names, out[1:]):
        assert line == f"{name} {getattr(ctype, f).offset} {getattr(ctype, f).size}"
        assert getattr(ctype, f).offset == offset, f"padding in front of {f}"
        offset += getattr(ctype, f).size
    assert out[1 + len(names)] == f"{capix.PEAK_LDS_BYTES} {capix.PEAK_LOG2_BLOCK}"


def test_python_names(jsg):
    launch_kw = ["pre_max", "post_max", "pre_avg", "post_avg", "delta", "wait", "normalise", "d_energy", "d_backtracked", "d_candidate"]
    want = {
        "peak_launch": ["d_in", "d_peaks", "d_n_peaks"] + launch_kw + ["d_scratch", "stream"],
        "peak_scratch_bytes": ["d_in", "d_peaks", "d_n_peaks"] + launch_kw,
        "peak_plan": ["n_frames", "rows", "wait"],
        "peak_pick": ["x", "pre_max", "post_max", "pre_avg", "post_avg", "delta", "wait", "normalise", "max_peaks"],
        "onset_backtrack": ["events", "energy"],
        "onset_detect": ["onset_envelope", "sr", "hop_length", "backtrack", "energy", "normalise", "units", "pre_max", "post_max", "pre_avg", "post_avg", "wait", "delta"],
        "onset_detect_audio": ["x", "sr", "n_fft", "hop", "n_mels", "kw"],
    }
    for name, params in want.items():
        assert callable(getattr(jsg, name)) and name in jsg.__all__
        assert list(inspect.signature(getattr(jsg, name)).parameters) == params, name
    detect = inspect.signature(jsg.onset_detect).parameters
    assert [p.default for p in detect.values()][1:] == [22050, 512, False, None, True, "frames", 0.03, 0.0, 0.10, 0.10, 0.03, 0.07]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in list(detect.values())[1:])
    pick = inspect.signature(jsg.peak_pick).parameters
    assert [pick[k].default for k in ("normalise", "max_peaks")] == [False, None] and all(pick[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("normalise", "max_peaks"))
    assert [p.default for p in inspect.signature(jsg.onset_detect_audio).parameters.values()][2:5] == [2048, 512, 128]
    # the seconds of the defaults at 22050 / 512 are the reaches (1, 0, 4, 4) and wait 1
    assert [int(v * 22050 // 512) for v in (0.03, 0.0, 0.10, 0.10, 0.03)] == [1, 0, 4, 4, 1]
    symbols = {"jsgx_peak_launch", "jsgx_peak_plan", "jsgx_peak_scratch_bytes"}
    assert symbols <= set(jsg.capix.SIGNATURES)
    assert shutil.which("nm"), "nm (binutils) lists the exported symbols"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", jsg.capix.LIB_PATH], text=True)
    functions = {line.split()[-1] for line in exported.splitlines() if " T " in line}
    assert symbols <= functions and functions == set(jsg.capix.SIGNATURES)


def test_kernel_notes(capix, tmp_path):
    """The new object: its seven kernels ("peak_single" once a workgroup a row, once a wavefront a row), no private segment (no scratch
    memory, no spills), the stated LDS in the three that build the tables and the reduction's slots alone in the two that reduce."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    obj = os.path.join(ROOT, "jadespectrogram_amd", "build", "jsgx_peak.o")
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
        assert int(g("vgpr_count")) <= 64, name           # eight wavefronts of a SIMD keep their registers
    tables, slots = (0, capix.PEAK_LDS_BYTES, 0, 0, capix.PEAK_THREADS), (0, 48, 0, 0, capix.PEAK_THREADS)
    assert found == {"peak_stats_kernel": slots, "peak_row_kernel": slots, "peak_cand_kernel": tables, "peak_carry_kernel": (0, 0, 0, 0, 64), "peak_emit_kernel": tables,
                     f"peak_single_kernel<{B}, 256>": tables, "peak_single_kernel<64, 64>": tables}


def test_host_entry_points_under_asan_ubsan(capix):
    """tests/cpp/jsgx_peak_host_test.cpp (its own main: the refusals in their order, the plan and the scratch over shapes up to the limits,
    rows more than 2^31 elements apart) built together with the host units it calls under the address and undefined-behaviour sanitizers
    and run as a child process; the same program against the shipped library, there with the refusals of the launch, gives the same
    verdict."""
    d = tempfile.gettempdir()
    drv = os.path.join(ROOT, "tests", "cpp", "jsgx_peak_host_test.cpp")
    hosts = [os.path.join(ROOT, "jadespectrogram_amd", "csrc", f) for f in ("jsgx_beat_host.cpp", "jsgx_peak_host.cpp")]
    common = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]
    san = os.path.join(d, "jsgx_peak_host_san")
    subprocess.check_call(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"] + hosts + [drv, "-o", san])
    libdir = os.path.dirname(capix.LIB_PATH)
    shipped = os.path.join(d, "jsgx_peak_host_lib")
    subprocess.check_call(common + ["-DJSGX_PEAK_TEST_LAUNCHES", drv, "-o", shipped, "-L", libdir, "-ljsgx", f"-Wl,-rpath,{libdir}"])
    for exe in (san, shipped):
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == "ok" and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr

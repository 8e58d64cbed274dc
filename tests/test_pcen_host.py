"""Section 13 of the companion library, host side (include/jsgx.h): every refusal of the per-channel energy normalisation in its stated
order (all decided without a device), the plan and the scratch arithmetic up to the limits, the forms the plan can return against the shape
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

import pcen_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# never dereferenced: every call below is refused or planned
IN, DECAY, STATE_IN, STATE_OUT, SMOOTH, OUT, SCRATCH = (i << 44 for i in range(1, 8))
BAD = -2
NEED = 4 * 3 * 3 * 40            # three rows of three chunks of 40 bands
IN_SPAN, OUT_SPAN, SMOOTH_SPAN = 2 * 600 * 44 + 599 * 44 + 40, 2 * 600 * 41 + 599 * 41 + 40, 3 * 600 * 40
STATE_IN_SPAN, STATE_OUT_SPAN = 2 * 40 + 40, 2 * 48 + 40
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def capix(jsg):
    if not os.path.exists(jsg.capix.LIB_PATH):
        from jadespectrogram_amd import _build
        _build.build_lib()
    jsg.capix.lib()
    return jsg.capix


def pcen_args(capix, **kw):       # 3 rows of 600 frames x 40 bands, every optional buffer given
    a = dict(in_=IN, frame_pitch=44, row_pitch=600 * 44, decay=DECAY, state_in=STATE_IN, state_in_pitch=40, state_out=STATE_OUT, state_out_pitch=48,
             smooth_out=SMOOTH, smooth_frame_pitch=40, smooth_row_pitch=600 * 40, out=OUT, out_frame_pitch=41, out_row_pitch=600 * 41, rows=3, n_bands=40,
             n_frames=600, b=0.05, gain=0.98, bias=2.0, power=0.5, eps=1e-6)
    a.update(kw)
    return capix.PcenArgs(**a)


# in the order of the header: a call with two defects is refused for the earlier one.  "scratch" and "scratch_bytes" are the launch's own.
REFUSED = [
    ("null in", dict(in_=None), "null in"),
    ("null decay", dict(decay=None), "null decay"),
    ("null out", dict(out=None), "null out"),
    ("misaligned in", dict(in_=IN + 2), "pointers must be 4-byte aligned"),
    ("misaligned state_in", dict(state_in=STATE_IN + 1), "pointers must be 4-byte aligned"),
    ("misaligned smooth_out", dict(smooth_out=SMOOTH + 3), "pointers must be 4-byte aligned"),
    ("no rows", dict(rows=0), "rows must be in 1..65535"),
    ("65536 rows", dict(rows=65536), "rows must be in 1..65535"),
    ("no bands", dict(n_bands=0), "n_bands must be in 1..65536"),
    ("65537 bands", dict(n_bands=65537), "n_bands must be in 1..65536"),
    ("no frames", dict(n_frames=0), "n_frames must be in 1..2147483647"),
    ("negative frames", dict(n_frames=-1), "n_frames must be in 1..2147483647"),
    ("too many chains", dict(n_frames=(1 << 31) - 1, n_bands_and_rows=True), "rows * chunks * n_bands must be at most 2^36"),
    ("frame_pitch", dict(frame_pitch=39), "frame_pitch smaller than n_bands"),
    ("row_pitch", dict(row_pitch=599 * 44 + 39), "row_pitch does not cover a plane"),
    ("state_in_pitch", dict(state_in_pitch=39), "state_in_pitch smaller than n_bands"),
    ("state_out_pitch", dict(state_out_pitch=39), "state_out_pitch smaller than n_bands"),
    ("smooth_frame_pitch", dict(smooth_frame_pitch=39), "smooth_frame_pitch smaller than n_bands"),
    ("smooth_row_pitch", dict(smooth_row_pitch=599 * 40 + 39), "smooth_row_pitch does not cover a plane"),
    ("out_frame_pitch", dict(out_frame_pitch=39), "out_frame_pitch smaller than n_bands"),
    ("out_row_pitch", dict(out_row_pitch=599 * 41 + 39), "out_row_pitch does not cover a plane"),
    ("b of zero", dict(b=0.0), "b must be in (0, 1]"),
    ("b above one", dict(b=1.5), "b must be in (0, 1]"),
    ("b a NaN", dict(b=NAN), "b must be in (0, 1]"),
    ("negative gain", dict(gain=-0.5), "gain must be finite and not negative"),
    ("infinite gain", dict(gain=INF), "gain must be finite and not negative"),
    ("negative bias", dict(bias=-1.0), "bias must be finite and not negative"),
    ("bias a NaN", dict(bias=NAN), "bias must be finite and not negative"),
    ("power of zero", dict(power=0.0), "power must be finite and positive"),
    ("infinite power", dict(power=INF), "power must be finite and positive"),
    ("eps of zero", dict(eps=0.0), "eps must be finite and positive"),
    ("eps a NaN", dict(eps=NAN), "eps must be finite and positive"),
    ("out ends in in", dict(out=IN - 4 * OUT_SPAN + 4), "out overlaps in"),
    ("out inside decay", dict(out=DECAY + 4 * 255), "out overlaps decay"),
    ("out inside state_in", dict(out=STATE_IN + 4 * (STATE_IN_SPAN - 1)), "out overlaps state_in"),
    ("smooth_out inside in", dict(smooth_out=IN + 4 * 1000), "smooth_out overlaps in"),
    ("smooth_out ends in decay", dict(smooth_out=DECAY - 4 * SMOOTH_SPAN + 4), "smooth_out overlaps decay"),
    ("smooth_out is state_in", dict(smooth_out=STATE_IN), "smooth_out overlaps state_in"),
    ("state_out inside in", dict(state_out=IN + 4 * (IN_SPAN - 1)), "state_out overlaps in"),
    ("state_out inside decay", dict(state_out=DECAY + 4 * 100), "state_out overlaps decay"),
    ("state_out is state_in", dict(state_out=STATE_IN), "state_out overlaps state_in"),
    ("out inside smooth_out", dict(out=SMOOTH + 4 * (SMOOTH_SPAN - 1)), "out overlaps smooth_out"),
    ("state_out inside out", dict(state_out=OUT + 4 * 7), "out overlaps state_out"),
    ("state_out ends in smooth_out", dict(state_out=SMOOTH - 4 * STATE_OUT_SPAN + 4), "smooth_out overlaps state_out"),
    ("null scratch", dict(scratch=None), "null scratch"),
    ("misaligned scratch", dict(scratch=SCRATCH + 2), "scratch must be 4-byte aligned"),
    ("small scratch", dict(scratch_bytes=NEED - 1), "scratch smaller than jsgx_pcen_scratch_bytes"),
    ("scratch ends in in", dict(scratch=IN - NEED + 4), "scratch overlaps in"),
    ("scratch inside decay", dict(scratch=DECAY + 4 * 255), "scratch overlaps decay"),
    ("scratch inside state_in", dict(scratch=STATE_IN + 4 * 5), "scratch overlaps state_in"),
    ("scratch inside out", dict(scratch=OUT + 4 * (OUT_SPAN - 1)), "scratch overlaps out"),
    ("scratch inside smooth_out", dict(scratch=SMOOTH + 4 * 10), "scratch overlaps smooth_out"),
    ("scratch ends in state_out", dict(scratch=STATE_OUT - NEED + 4), "scratch overlaps state_out"),
]


def expand(change):
    """The one entry that changes three fields at once: the largest rows and bands with the largest frame count."""
    change = dict(change)
    if change.pop("n_bands_and_rows", False):
        change.update(rows=65535, n_bands=65536)
    return change


def launch(lib, capix, change):
    change = expand(change)
    scratch, scratch_bytes = change.pop("scratch", SCRATCH), change.pop("scratch_bytes", NEED)
    return lib.jsgx_pcen_launch(C.byref(pcen_args(capix, **change)), scratch, scratch_bytes, None)


@pytest.mark.parametrize("i", range(len(REFUSED)), ids=[r[0] for r in REFUSED])
def test_refusals_in_their_order(capix, i):
    lib = capix.lib()
    _, change, message = REFUSED[i]
    change = expand(change)
    assert launch(lib, capix, change) == BAD and lib.jsgx_last_error() == f"jsgx_pcen_launch: {message}".encode(), lib.jsgx_last_error()
    if not set(change) & {"scratch", "scratch_bytes"}:          # what the launch refuses before it looks at the scratch, the other two calls refuse alike
        a = pcen_args(capix, **change)
        assert lib.jsgx_pcen_plan(C.byref(a), None, 0, None, None, None, None) == BAD and lib.jsgx_last_error() == f"jsgx_pcen_plan: {message}".encode()
        assert lib.jsgx_pcen_scratch_bytes(C.byref(a)) == BAD and lib.jsgx_last_error() == f"jsgx_pcen_scratch_bytes: {message}".encode()
    # with any later defect on top, the earlier one is still the one reported
    for _, later, later_message in REFUSED[i + 1:]:
        later = expand(later)
        if later_message == message or set(later) & set(change):
            continue
        assert launch(lib, capix, dict(later, **change)) == BAD
        assert lib.jsgx_last_error() == f"jsgx_pcen_launch: {message}".encode(), (REFUSED[i][0], later)


def test_what_passes(capix):
    lib = capix.lib()
    size = lambda **kw: lib.jsgx_pcen_scratch_bytes(C.byref(pcen_args(capix, **kw)))
    assert size() == NEED
    # a buffer next to another, not inside it
    assert size(out=IN - 4 * OUT_SPAN) == NEED and size(out=DECAY + 4 * 256) == NEED and size(state_out=IN + 4 * IN_SPAN) == NEED
    assert size(smooth_out=DECAY - 4 * SMOOTH_SPAN) == NEED and size(state_out=SMOOTH - 4 * STATE_OUT_SPAN) == NEED
    # the optional buffers absent: their pitches are not looked at; one row: nor are the row pitches; the ends of the ranges
    assert size(state_in=None, state_out=None, smooth_out=None, state_in_pitch=0, state_out_pitch=0, smooth_frame_pitch=0, smooth_row_pitch=0) == NEED
    assert size(rows=1, row_pitch=0, out_row_pitch=0, smooth_row_pitch=0, state_in_pitch=0, state_out_pitch=0) == NEED // 3
    assert size(b=1.0, gain=0.0, bias=0.0, power=1e-30, eps=1e-45) == NEED
    assert size(n_frames=256) == 0 and size(n_frames=257) == 4 * 3 * 2 * 40 and size(n_frames=1) == 0
    for call in (lib.jsgx_pcen_launch(None, SCRATCH, NEED, None), lib.jsgx_pcen_plan(None, None, 0, None, None, None, None), lib.jsgx_pcen_scratch_bytes(None)):
        assert call == BAD and lib.jsgx_last_error().endswith(b": null argument")
    assert lib.jsgx_pcen_plan(C.byref(pcen_args(capix)), C.create_string_buffer(15), 15, None, None, None, None) == BAD
    assert lib.jsgx_last_error() == b"jsgx_pcen_plan: bad argument"
    import torch
    if torch.cuda.is_available():           # with a device the calls below would launch on pointers that are no memory
        return
    NO_DEVICE = capix.JSGX_ERR_NO_DEVICE
    assert launch(lib, capix, {}) == NO_DEVICE and lib.jsgx_last_error() == b"jsgx_pcen_launch: no HIP device"
    # a larger scratch, one that touches no buffer, and none where a row is one chunk
    assert launch(lib, capix, dict(scratch_bytes=NEED + 4096)) == NO_DEVICE and launch(lib, capix, dict(scratch=IN - NEED)) == NO_DEVICE
    assert launch(lib, capix, dict(n_frames=256, scratch=None, scratch_bytes=0)) == NO_DEVICE
    assert launch(lib, capix, dict(n_frames=200, scratch=IN + 2, scratch_bytes=-1)) == NO_DEVICE          # not looked at


def test_the_plan_and_the_scratch_over_shapes(jsg, capix):
    chunk = capix.PCEN_CHUNK
    most = (1 << 31) - 1
    for T in (1, 2, chunk - 1, chunk, chunk + 1, 1000, 1 << 24, most):
        for B in (1, 40, 64, 65, capix.PCEN_MAX_BANDS):
            for R in (1, 3, 65535):
                chunks = -(-T // chunk)
                if R * chunks * B > capix.PCEN_MAX_CHAINS:
                    with pytest.raises(jsg.JsgError, match="rows \\* chunks \\* n_bands must be at most 2\\^36"):
                        jsg.pcen_plan(T, B, R)
                    continue
                assert jsg.pcen_plan(T, B, R) == ("pcen_single" if chunks == 1 else "pcen_chunked", capix.PCEN_THREADS, 0, 1 if chunks == 1 else 3, chunks)
                a = capix.PcenArgs(in_=1 << 50, frame_pitch=B, row_pitch=T * B, decay=1 << 40, out=1 << 58, out_frame_pitch=B, out_row_pitch=T * B, rows=R, n_bands=B,
                                   n_frames=T, b=0.5, gain=1.0, bias=0.0, power=1.0, eps=1.0)
                assert capix.lib().jsgx_pcen_scratch_bytes(C.byref(a)) == (0 if chunks == 1 else 4 * R * chunks * B)
    hdr = open(os.path.join(ROOT, "include", "jsgx.h")).read()
    for name, value in (("JSGX_PCEN_CHUNK", capix.PCEN_CHUNK), ("JSGX_PCEN_MAX_BANDS", capix.PCEN_MAX_BANDS), ("JSGX_PCEN_MAX_CHAINS", capix.PCEN_MAX_CHAINS),
                        ("JSGX_PCEN_THREADS", capix.PCEN_THREADS), ("JSGX_ABI_VERSION", 1)):
        assert re.search(rf"#define {name} {value}\b", hdr), name
    assert (capix.PCEN_CHUNK, capix.PCEN_MAX_BANDS, capix.PCEN_MAX_CHAINS) == (256, 65536, 1 << 36) == (pr.CHUNK, 65536, 1 << 36)
    for kernel in ("pcen_single", "pcen_chunked", "pcen_scan", "pcen_carry", "pcen_apply"):
        assert f'"{kernel}"' in hdr
    assert capix.lib().jsgx_abi_version() == 1


def test_the_gpu_shapes_cover_every_form(capix):
    """Every form the plan can return over every band count, both row counts of the GPU test and frame counts on both sides of every chunk
    boundary up to its longest plane: the form is a function of the frame count alone, a listed shape runs each form, and wherever the form
    or the number of chunks changes between T - 1 and T both frame counts are listed.  The lanes are dealt to (row, chunk, part, band) by one
    rule for every band count, so the band counts carry no form of their own; what the list owes them is the counts around a wavefront."""
    lib = capix.lib()
    name, launches, chunks = C.create_string_buffer(16), C.c_int32(), C.c_int32()
    a = pcen_args(capix, state_in=None, state_out=None, smooth_out=None)

    def form(R, T, B):
        a.rows, a.n_frames, a.n_bands = R, T, B
        a.frame_pitch, a.row_pitch, a.out_frame_pitch, a.out_row_pitch = B, T * B, B, T * B
        assert lib.jsgx_pcen_plan(C.byref(a), name, 16, None, None, C.byref(launches), C.byref(chunks)) == 0, lib.jsgx_last_error()
        return name.value.decode(), launches.value

    listed_T = {s[1] for s in pr.SHAPES}
    frames = (1, 2, 255, 256, 257, 511, 512, 513, 1000)
    forms = {}
    for B in range(1, capix.PCEN_MAX_BANDS + 1):
        for T in (256, 257):
            forms.setdefault((T, form(1, T, B)), B)
    assert set(forms) == {(256, ("pcen_single", 1)), (257, ("pcen_chunked", 3))}, "a form that depends on the band count: list band counts on both sides of it"
    by_T = {T: form(1, T, 40) for T in range(1, max(pr.T_SET) + 1)}
    for R in pr.ROWS_SET:
        for B in (1, 40, 64, 200):
            for T in frames:
                assert form(R, T, B) == by_T[T], (R, T, B)
    assert set(by_T.values()) == {form(*s) for s in pr.SHAPES}, "a form no listed shape runs"
    changes = [T for T in range(2, max(pr.T_SET) + 1) if by_T[T] != by_T[T - 1]]
    assert changes == [257] and all(T in listed_T and T - 1 in listed_T for T in changes)
    # what the band counts owe: one, the counts next to a wavefront and a count that does not divide it; and the parts of "pcen_apply" (64 frames)
    assert {1, 63, 64, 65} <= {s[2] for s in pr.SHAPES} and any(64 % s[2] for s in pr.SHAPES if s[2] < 64)
    assert {64, 65} <= listed_T and any(128 < T < 192 for T in listed_T) and any(192 < T < 256 for T in listed_T)
    assert {1, 3} == {s[0] for s in pr.SHAPES}


def test_struct_layout_matches_the_header(capix, tmp_path):
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler")
    struct, ctype = "jsgx_pcen_args", capix.PcenArgs
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsgx.h")).read(), flags=re.S)
    body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", hdr, flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*(\[\d+\])?\s*$", decl).group(1) for decl in body.split(";") if decl.strip()]
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "jsgx.h"', "int main(void) {", f'    printf("%zu\\n", sizeof({struct}));']
    lines += [f'    printf("{f} %zu %zu\\n", offsetof({struct}, {f}), sizeof((({struct}*)0)->{f}));' for f in names]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)])
    out = subprocess.check_output([str(tmp_path / "layout")], text=True).split("\n")
    assert out[0] == str(C.sizeof(ctype)) == "144"
    assert [f for f, _ in ctype._fields_] == ["in_" if f == "in" else f for f in names]
    offset = 0
    for (f, _), name, line in zip(ctype._fields_, names, out[1:]):
        assert line == f"{name} {getattr(ctype, f).offset} {getattr(ctype, f).size}"
        assert getattr(ctype, f).offset == offset, f"padding in front of {f}"
        offset += getattr(ctype, f).size


def test_python_names(jsg):
    launch_kw = ["b", "gain", "bias", "power", "eps", "d_state_in", "d_state_out", "d_smooth"]
    want = {
        "pcen": ["plane", "sr", "hop_length", "gain", "bias", "power", "time_constant", "eps", "b", "state", "return_state", "return_smooth"],
        "pcen_coefficient": ["time_constant", "sr", "hop_length"],
        "pcen_launch": ["d_in", "d_decay", "d_out"] + launch_kw + ["d_scratch", "stream"],
        "pcen_scratch_bytes": ["d_in", "d_decay", "d_out"] + launch_kw,
        "pcen_plan": ["n_frames", "n_bands", "rows"],
        "pcen_decay": ["b"],
        "pcen_audio": ["x", "sr", "n_fft", "hop", "n_mels", "fmin", "fmax", "kw"],
    }
    for name, params in want.items():
        assert callable(getattr(jsg, name)) and name in jsg.__all__
        assert list(inspect.signature(getattr(jsg, name)).parameters) == params, name
    pcen = inspect.signature(jsg.pcen).parameters
    assert [p.default for p in pcen.values()][1:] == [22050, 512, 0.98, 2.0, 0.5, 0.4, 1e-6, None, None, False, False]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in list(pcen.values())[1:])
    launch_params = inspect.signature(jsg.pcen_launch).parameters
    assert launch_params["b"].default is inspect.Parameter.empty and launch_params["b"].kind is inspect.Parameter.KEYWORD_ONLY
    assert [launch_params[k].default for k in ("gain", "bias", "power", "eps")] == [0.98, 2.0, 0.5, 1e-6]
    symbols = {"jsgx_pcen_launch", "jsgx_pcen_plan", "jsgx_pcen_scratch_bytes", "jsgx_pcen_decay_build"}
    assert symbols <= set(jsg.capix.SIGNATURES)
    assert shutil.which("nm"), "nm (binutils) lists the exported symbols"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", jsg.capix.LIB_PATH], text=True)
    functions = {line.split()[-1] for line in exported.splitlines() if " T " in line}
    assert symbols <= functions and functions == set(jsg.capix.SIGNATURES)


def test_kernel_notes(capix, tmp_path):
    """The new object: its four kernels (the apply pass once with the entering state read directly, once from the scratch), no private
    segment (no scratch memory, no spills), no LDS and 256 lanes a workgroup."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    obj = os.path.join(ROOT, "jadespectrogram_amd", "build", "jsgx_pcen.o")
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
        assert int(g("vgpr_count")) <= 128, name           # four wavefronts of a SIMD or more keep their registers (512 a lane)
    plain = (0, 0, 0, 0, capix.PCEN_THREADS)
    assert found == {"pcen_scan_kernel": plain, "pcen_carry_kernel": plain, "pcen_apply_kernel<true>": plain, "pcen_apply_kernel<false>": plain}


def test_host_entry_points_under_asan_ubsan(capix):
    """tests/cpp/jsgx_pcen_host_test.cpp (its own main: the table, the refusals in their order, the plan and the scratch over shapes up to the
    limits, rows more than 2^31 elements apart) built together with the host units it calls under the address and undefined-behaviour
    sanitizers and run as a child process; the same program against the shipped library, there with the refusals of the launch, gives the
    same verdict."""
    d = tempfile.gettempdir()
    drv = os.path.join(ROOT, "tests", "cpp", "jsgx_pcen_host_test.cpp")
    hosts = [os.path.join(ROOT, "jadespectrogram_amd", "csrc", f) for f in ("jsgx_beat_host.cpp", "jsgx_pcen_host.cpp")]
    common = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]
    san = os.path.join(d, "jsgx_pcen_host_san")
    subprocess.check_call(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"] + hosts + [drv, "-o", san])
    libdir = os.path.dirname(capix.LIB_PATH)
    shipped = os.path.join(d, "jsgx_pcen_host_lib")
    subprocess.check_call(common + ["-DJSGX_PCEN_TEST_LAUNCHES", drv, "-o", shipped, "-L", libdir, "-ljsgx", f"-Wl,-rpath,{libdir}"])
    for exe in (san, shipped):
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == "ok" and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr

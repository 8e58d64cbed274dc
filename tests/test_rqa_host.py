"""Section 9 of the companion library, host side (include/jsgx.h): every refusal of the recurrence quantification alignment in its stated
order (all decided without a device), the scratch formula and the plan over shapes, the struct layout against a C program, the Python
names, the kernels' notes, and the host entry points from a stand-alone C++ program under the address and undefined-behaviour sanitizers.
CPU only."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# never dereferenced: every call below is refused, sized or planned
SIM, SCORE, STEP, PATH_I, PATH_J, LEN, END, TOTAL, SCRATCH = (i << 44 for i in range(1, 10))
BAD = -2


@pytest.fixture(scope="module")
def capix(jsg):
    if not os.path.exists(jsg.capix.LIB_PATH):
        from jadespectrogram_amd import _build
        _build.build_lib()
    jsg.capix.lib()
    return jsg.capix


def rqa_args(capix, **kw):      # 3 pairs of 100 x 300, every output
    a = dict(sim=SIM, sim_pitch=300, sim_pair_pitch=30000, pairs=3, n=100, m=300, knight=1, gap_onset=1.0, gap_extend=0.5, reserved0=0, max_path=100,
             score=SCORE, score_pitch=304, score_pair_pitch=30400, step=STEP, step_pitch=301, step_pair_pitch=30100, path_i=PATH_I, path_j=PATH_J,
             path_pitch=100, path_len=LEN, end=END, total=TOTAL)
    a.update(kw)
    return capix.RqaArgs(**a)


# in the order of the header: a call with two defects is refused for the earlier one
REFUSED = [
    ("null sim", dict(sim=None), "null sim"),
    ("null score", dict(score=None), "null score"),
    ("path_i alone", dict(path_j=None), "path_i and path_j go together"),
    ("path_j alone", dict(path_i=None), "path_i and path_j go together"),
    ("paths without path_len", dict(path_len=None), "null path_len with paths"),
    ("misaligned sim", dict(sim=SIM + 2), "pointers must be 4-byte aligned"),
    ("misaligned end", dict(end=END + 1), "pointers must be 4-byte aligned"),
    ("misaligned total", dict(total=TOTAL + 3), "pointers must be 4-byte aligned"),
    ("no pairs", dict(pairs=0), "pairs must be in 1..65535"),
    ("65536 pairs", dict(pairs=65536), "pairs must be in 1..65535"),
    ("n 0", dict(n=0), "n must be in 1..65536"),
    ("n 65537", dict(n=65537), "n must be in 1..65536"),
    ("m 0", dict(m=0), "m must be in 1..65536"),
    ("m 65537", dict(m=65537), "m must be in 1..65536"),
    ("knight 2", dict(knight=2), "knight must be 0 or 1"),
    ("knight -1", dict(knight=-1), "knight must be 0 or 1"),
    ("gap_onset negative", dict(gap_onset=-1.0), "gap_onset must be finite and >= 0"),
    ("gap_onset NaN", dict(gap_onset=float("nan")), "gap_onset must be finite and >= 0"),
    ("gap_extend infinite", dict(gap_extend=float("inf")), "gap_extend must be finite and >= 0"),
    ("gap_extend negative", dict(gap_extend=-0.25), "gap_extend must be finite and >= 0"),
    ("reserved0", dict(reserved0=7), "reserved0 must be 0"),
    ("max_path", dict(max_path=99), "max_path smaller than min(n, m)"),
    ("sim_pitch", dict(sim_pitch=299), "sim_pitch smaller than m"),
    ("sim_pair_pitch", dict(sim_pair_pitch=29999), "sim_pair_pitch does not cover a plane"),
    ("score_pitch", dict(score_pitch=299), "score_pitch smaller than m"),
    ("score_pair_pitch", dict(score_pair_pitch=99 * 304 + 299), "score_pair_pitch does not cover a plane"),
    ("step_pitch", dict(step_pitch=299), "step_pitch smaller than m"),
    ("step_pair_pitch", dict(step_pair_pitch=99 * 301 + 299), "step_pair_pitch does not cover a plane"),
    ("path_pitch", dict(path_pitch=99), "path_pitch smaller than max_path"),
    ("score ends in sim", dict(score=SIM - 4 * (2 * 30400 + 99 * 304 + 300) + 4), "score overlaps sim"),
    ("step inside sim", dict(step=SIM + 4 * 89999 + 3), "an output overlaps sim"),
    ("total inside sim", dict(total=SIM + 4 * 89999), "an output overlaps sim"),
    ("end ends in score", dict(end=SCORE - 8 * 3 + 4), "two outputs overlap"),
    ("path_j inside path_i", dict(path_j=PATH_I + 4 * 299), "two outputs overlap"),
    ("path_len inside step", dict(path_len=STEP + 2 * 30100 + 99 * 301 + 297), "two outputs overlap"),
]
CALLS = (("jsgx_rqa_launch", lambda lib, a: lib.jsgx_rqa_launch(C.byref(a), SCRATCH, 1 << 50, None)),
         ("jsgx_rqa_scratch_bytes", lambda lib, a: lib.jsgx_rqa_scratch_bytes(C.byref(a))),
         ("jsgx_rqa_plan", lambda lib, a: lib.jsgx_rqa_plan(C.byref(a), None, 0, None, None, None, None, None)))


@pytest.mark.parametrize("i", range(len(REFUSED)), ids=[r[0] for r in REFUSED])
def test_refusals_in_their_order(capix, i):
    lib = capix.lib()
    _, change, message = REFUSED[i]
    a = rqa_args(capix, **change)
    for who, call in CALLS:
        assert call(lib, a) == BAD and lib.jsgx_last_error() == f"{who}: {message}".encode(), (who, REFUSED[i][0], lib.jsgx_last_error())
    # with any later defect on top, the earlier one is still the one reported
    who, call = CALLS[0]
    for _, later, later_message in REFUSED[i + 1:]:
        if later_message == message or set(later) & set(change):
            continue
        assert call(lib, rqa_args(capix, **dict(later, **change))) == BAD
        assert lib.jsgx_last_error() == f"{who}: {message}".encode(), (REFUSED[i][0], later)
    # ... also ahead of what only the launch refuses
    assert lib.jsgx_rqa_launch(C.byref(a), None, 0, None) == BAD and lib.jsgx_last_error() == f"jsgx_rqa_launch: {message}".encode()


def test_what_only_the_launch_refuses_and_what_passes(capix):
    lib = capix.lib()
    a = rqa_args(capix)
    need = 8 * 3 * 10 + 8 * 3 * 100
    for scratch, size, message in ((None, 1 << 40, "null scratch"), (SCRATCH + 2, 1 << 40, "scratch must be 4-byte aligned"),
                                   (SCRATCH, need - 1, "scratch smaller than jsgx_rqa_scratch_bytes"), (None, 0, "null scratch")):
        assert lib.jsgx_rqa_launch(C.byref(a), scratch, size, None) == BAD and lib.jsgx_last_error() == f"jsgx_rqa_launch: {message}".encode()
    for call in (lib.jsgx_rqa_launch(None, SCRATCH, 1 << 40, None), lib.jsgx_rqa_scratch_bytes(None), lib.jsgx_rqa_plan(None, None, 0, None, None, None, None, None)):
        assert call == BAD and lib.jsgx_last_error().endswith(b": null argument")
    assert lib.jsgx_rqa_plan(C.byref(a), C.create_string_buffer(15), 15, None, None, None, None, None) == BAD and lib.jsgx_last_error() == b"jsgx_rqa_plan: bad argument"
    size = lambda **kw: lib.jsgx_rqa_scratch_bytes(C.byref(rqa_args(capix, **kw)))
    assert size() == need
    # the step plane is one of bytes: any alignment; penalties of zero; an output next to the input or to another output, not inside it
    assert size(step=STEP + 1) == need and size(gap_onset=0.0, gap_extend=0.0) == need and size(knight=0) == need
    assert size(score=SIM - 4 * (2 * 30400 + 99 * 304 + 300)) == need and size(step=SIM + 4 * 90000) == need and size(end=SCORE - 8 * 3) == need
    assert size(path_j=PATH_I + 4 * 300) == need and size(path_len=STEP + 2 * 30100 + 99 * 301 + 301) == need
    # one pair: the pair pitches are not looked at
    assert size(pairs=1, sim_pair_pitch=0, score_pair_pitch=0, step_pair_pitch=0, path_pitch=0) == need // 3
    # without a step plane its pitches are not looked at
    assert size(step=None, step_pitch=0, step_pair_pitch=0) == need
    # the parts of the scratch: the tiles' best cells for any of path_len, end and total, the reversed paths for the paths
    no_paths = dict(path_i=None, path_j=None, max_path=0, path_pitch=0)
    assert size(**no_paths) == 8 * 3 * 10 and size(path_len=None, total=None, **no_paths) == 8 * 3 * 10 and size(path_len=None, end=None, **no_paths) == 8 * 3 * 10
    assert size(path_len=None, end=None, total=None, **no_paths) == 0
    import torch
    if not torch.cuda.is_available():           # with a device these calls would launch on pointers that are no memory
        assert lib.jsgx_rqa_launch(C.byref(a), SCRATCH, need, None) == capix.JSGX_ERR_NO_DEVICE and lib.jsgx_last_error() == b"jsgx_rqa_launch: no HIP device"
        # the score alone: the scratch is not looked at
        assert lib.jsgx_rqa_launch(C.byref(rqa_args(capix, path_len=None, end=None, total=None, **no_paths)), None, 0, None) == capix.JSGX_ERR_NO_DEVICE


def test_plan_and_scratch_over_shapes(jsg, capix):
    TR, TC = capix.DTW_TILE_ROWS, capix.DTW_TILE_COLS
    for pairs in (1, 3):
        for n in (1, 2, TR - 1, TR, TR + 1, 2 * TR + 1, 4096, 65536):
            for m in (1, 2, TC - 1, TC, TC + 1, 2 * TC + 2, 16384, 65536):
                ti, tj = -(-n // TR), -(-m // TC)
                assert jsg.rqa_plan(n, m, pairs) == ("rqa_tiles", TR, TC, ti + tj, capix.RQA_THREADS, capix.RQA_LDS_BYTES)
                assert jsg.rqa_plan(n, m, pairs, backtrack=False)[3] == ti + tj - 1
                a = capix.RqaArgs(sim=SIM, sim_pitch=m, sim_pair_pitch=n * m, pairs=pairs, n=n, m=m, knight=1, gap_onset=1.0, gap_extend=1.0, max_path=min(n, m),
                                  score=SCORE, score_pitch=m, score_pair_pitch=n * m, path_i=PATH_I, path_j=PATH_J, path_pitch=min(n, m), path_len=LEN)
                assert capix.lib().jsgx_rqa_scratch_bytes(C.byref(a)) == 8 * pairs * ti * tj + 8 * pairs * min(n, m)
    assert (capix.RQA_THREADS, capix.RQA_LDS_BYTES, capix.RQA_WINDOW) == (64, 17408, 32) and capix.RQA_LDS_BYTES <= 163840
    hdr = open(os.path.join(ROOT, "include", "jsgx.h")).read()
    for name, value in (("JSGX_RQA_THREADS", capix.RQA_THREADS), ("JSGX_RQA_LDS_BYTES", capix.RQA_LDS_BYTES), ("JSGX_RQA_WINDOW", capix.RQA_WINDOW), ("JSGX_ABI_VERSION", 1)):
        assert re.search(rf"#define {name} {value}\b", hdr), name
    for kernel in ("rqa_tiles", "rqa_backtrace"):
        assert f'"{kernel}"' in hdr


def test_struct_layout_matches_the_header(capix, tmp_path):
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler")
    struct, size = "jsgx_rqa_args", 152
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsgx.h")).read(), flags=re.S)
    body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", hdr, flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*(\[\d+\])?\s*$", decl).group(1) for decl in body.split(";") if decl.strip()]
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "jsgx.h"', "int main(void) {", f'    printf("%zu\\n", sizeof({struct}));']
    lines += [f'    printf("{f} %zu %zu\\n", offsetof({struct}, {f}), sizeof((({struct}*)0)->{f}));' for f in names]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)])
    out = subprocess.check_output([str(tmp_path / "layout")], text=True).split("\n")
    ctype = capix.RqaArgs
    assert out[0] == str(C.sizeof(ctype)) == str(size)
    assert [f for f, _ in ctype._fields_] == names
    offset = 0
    for (f, _), line in zip(ctype._fields_, out[1:]):
        assert line == f"{f} {getattr(ctype, f).offset} {getattr(ctype, f).size}"
        assert getattr(ctype, f).offset == offset, f"padding in front of {f}"
        offset += getattr(ctype, f).size


def test_python_names(jsg):
    outputs = ["d_step", "d_path_i", "d_path_j", "d_path_len", "d_end", "d_total"]
    want = {
        "rqa": ["sim", "gap_onset", "gap_extend", "knight_moves", "backtrack"],
        "rqa_launch": ["d_sim", "d_score", "gap_onset", "gap_extend", "knight_moves"] + outputs + ["d_scratch", "stream"],
        "rqa_scratch_bytes": ["d_sim", "d_score", "gap_onset", "gap_extend", "knight_moves"] + outputs,
        "rqa_plan": ["n", "m", "pairs", "backtrack"],
    }
    for name, params in want.items():
        assert callable(getattr(jsg, name)) and name in jsg.__all__
        assert list(inspect.signature(getattr(jsg, name)).parameters) == params, name
    assert [p.default for p in inspect.signature(jsg.rqa).parameters.values()][1:] == [1.0, 1.0, True, True]
    assert [p.default for p in inspect.signature(jsg.rqa_launch).parameters.values()][2:5] == [1.0, 1.0, True]
    for name in ("jsgx_rqa_scratch_bytes", "jsgx_rqa_launch", "jsgx_rqa_plan"):
        assert name in jsg.capix.SIGNATURES
    exported = subprocess.check_output(["nm", "-D", "--defined-only", jsg.capix.LIB_PATH], text=True) if shutil.which("nm") else None
    if exported is not None:
        assert {"jsgx_rqa_scratch_bytes", "jsgx_rqa_launch", "jsgx_rqa_plan"} <= {line.split()[-1] for line in exported.splitlines() if " T " in line}


def test_kernel_notes(capix, tmp_path):
    """The new object: its six kernels (the forward one with and without knight moves and a step plane, the backtrace with and without
    knight moves), no private segment (no scratch memory, no spills), the static LDS the header states and one wavefront a workgroup."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    obj = os.path.join(ROOT, "jadespectrogram_amd", "build", "jsgx_rqa.o")
    if not os.path.exists(obj):
        from jadespectrogram_amd import _build
        _build.build_lib()
    co = kernel_regs.code_object(obj, str(tmp_path))
    notes = subprocess.check_output([os.path.join(kernel_regs.LLVM, "llvm-readelf"), "--notes", co]).decode()
    found = {}
    for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
        g = lambda k: re.search(rf"\.{k}:\s+(\S+)", blk).group(1)
        name = subprocess.check_output(["c++filt", g("name")]).decode().strip()
        found[name.split("(")[0].replace("void ", "")] = (int(g("private_segment_fixed_size")), int(g("group_segment_fixed_size")), int(g("vgpr_spill_count")),
                                                         int(g("sgpr_spill_count")), int(g("max_flat_workgroup_size")))
    forward = (0, capix.RQA_LDS_BYTES, 0, 0, capix.RQA_THREADS)
    back = (0, 2 * 4 * capix.RQA_WINDOW ** 2 + 16, 0, 0, capix.RQA_THREADS)
    assert found == {"jsgx::rqa_kernel<true, true>": forward, "jsgx::rqa_kernel<true, false>": forward, "jsgx::rqa_kernel<false, true>": forward,
                     "jsgx::rqa_kernel<false, false>": forward, "jsgx::rqa_backtrace_kernel<true>": back, "jsgx::rqa_backtrace_kernel<false>": back}


def test_host_entry_points_under_asan_ubsan(capix):
    """tests/cpp/jsgx_rqa_host_test.cpp (its own main: the refusals in their order, the scratch size and the plan over shapes) built together
    with the host units it calls under the address and undefined-behaviour sanitizers and run as a child process; the same program against
    the shipped library, there with the refusals that only the launch decides, gives the same verdict."""
    d = tempfile.gettempdir()
    drv = os.path.join(ROOT, "tests", "cpp", "jsgx_rqa_host_test.cpp")
    hosts = [os.path.join(ROOT, "jadespectrogram_amd", "csrc", f) for f in ("jsgx_beat_host.cpp", "jsgx_rqa_host.cpp")]
    common = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]
    san = os.path.join(d, "jsgx_rqa_host_san")
    subprocess.check_call(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"] + hosts + [drv, "-o", san])
    libdir = os.path.dirname(capix.LIB_PATH)
    shipped = os.path.join(d, "jsgx_rqa_host_lib")
    subprocess.check_call(common + ["-DJSGX_RQA_TEST_LAUNCHES", drv, "-o", shipped, "-L", libdir, "-ljsgx", f"-Wl,-rpath,{libdir}"])
    for exe in (san, shipped):
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == "ok" and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr

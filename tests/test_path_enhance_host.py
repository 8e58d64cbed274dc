"""Sections 10 and 11 of the companion library, host side (include/jsgx.h): every refusal of the path enhancement and of the lag conversion
in its stated order (all decided without a device), the plan over reaches, the struct layouts against a C program, the header's constants,
the exported symbols, the Python names, the kernels' notes, and the host entry points and the filter-bank builder from a stand-alone C++
program under the address and undefined-behaviour sanitizers.  CPU only."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# never dereferenced: every call below is refused or planned
R, TAP_W, TAP_AT, FIRST, OUT = (i << 44 for i in range(1, 6))
BAD = -2


@pytest.fixture(scope="module")
def capix(jsg):
    if not os.path.exists(jsg.capix.LIB_PATH):
        from jadespectrogram_amd import _build
        _build.build_lib()
    jsg.capix.lib()
    return jsg.capix


def pe_args(capix, **kw):       # 3 pairs of 100 x 300, 7 filters of 3000 taps in all
    a = dict(r=R, r_pitch=300, r_pair_pitch=30000, tap_w=TAP_W, tap_at=TAP_AT, filter_first=FIRST, pairs=3, n=100, m=300, n_filters=7, n_taps=3000, reach_i=32,
             reach_j=30, clip=1, out=OUT, out_pitch=304, out_pair_pitch=30400)
    a.update(kw)
    return capix.PathEnhanceArgs(**a)


def lag_args(capix, **kw):      # 3 pairs of 100 x 100 to 200 x 100
    a = dict(in_=R, in_pitch=100, in_pair_pitch=10000, pairs=3, n=100, pad=1, axis=1, inverse=0, reserved0=0, out=OUT, out_pitch=104, out_pair_pitch=200 * 104)
    a.update(kw)
    return capix.LagArgs(**a)


OUT_SPAN = 2 * 30400 + 99 * 304 + 300
# in the order of the header: a call with two defects is refused for the earlier one
PE_REFUSED = [
    ("null r", dict(r=None), "null r"),
    ("null tap_w", dict(tap_w=None), "null tap_w"),
    ("null tap_at", dict(tap_at=None), "null tap_at"),
    ("null filter_first", dict(filter_first=None), "null filter_first"),
    ("null out", dict(out=None), "null out"),
    ("misaligned r", dict(r=R + 2), "pointers must be 4-byte aligned"),
    ("misaligned filter_first", dict(filter_first=FIRST + 1), "pointers must be 4-byte aligned"),
    ("no pairs", dict(pairs=0), "pairs must be in 1..65535"),
    ("65536 pairs", dict(pairs=65536), "pairs must be in 1..65535"),
    ("n 0", dict(n=0), "n must be in 1..65536"),
    ("n 65537", dict(n=65537), "n must be in 1..65536"),
    ("m 0", dict(m=0), "m must be in 1..65536"),
    ("m 65537", dict(m=65537), "m must be in 1..65536"),
    ("no filters", dict(n_filters=0), "n_filters must be in 1..32"),
    ("33 filters", dict(n_filters=33), "n_filters must be in 1..32"),
    ("no taps", dict(n_taps=0), "n_taps must be in 1..1048576"),
    ("too many taps", dict(n_taps=(1 << 20) + 1), "n_taps must be in 1..1048576"),
    ("reach_i 65", dict(reach_i=65), "reach_i must be in 0..64"),
    ("reach_i -1", dict(reach_i=-1), "reach_i must be in 0..64"),
    ("reach_j 65", dict(reach_j=65), "reach_j must be in 0..64"),
    ("clip 2", dict(clip=2), "clip must be 0 or 1"),
    ("r_pitch", dict(r_pitch=299), "r_pitch smaller than m"),
    ("r_pair_pitch", dict(r_pair_pitch=29999), "r_pair_pitch does not cover a plane"),
    ("out_pitch", dict(out_pitch=299), "out_pitch smaller than m"),
    ("out_pair_pitch", dict(out_pair_pitch=99 * 304 + 299), "out_pair_pitch does not cover a plane"),
    ("out ends in r", dict(out=R - 4 * OUT_SPAN + 4), "out overlaps r"),
    ("out inside tap_w", dict(out=TAP_W + 4 * 2999), "out overlaps tap_w"),
    ("out ends in tap_at", dict(out=TAP_AT - 4 * OUT_SPAN + 4), "out overlaps tap_at"),
    ("out inside filter_first", dict(out=FIRST + 4 * 7), "out overlaps filter_first"),
]
PE_CALLS = (("jsgx_path_enhance_launch", lambda lib, a: lib.jsgx_path_enhance_launch(C.byref(a), None)),
            ("jsgx_path_enhance_plan", lambda lib, a: lib.jsgx_path_enhance_plan(C.byref(a), None, 0, None, None, None, None)))
LAG_REFUSED = [
    ("null in", dict(in_=None), "null in"),
    ("null out", dict(out=None), "null out"),
    ("misaligned in", dict(in_=R + 1), "pointers must be 4-byte aligned"),
    ("misaligned out", dict(out=OUT + 2), "pointers must be 4-byte aligned"),
    ("no pairs", dict(pairs=0), "pairs must be in 1..65535"),
    ("n 0", dict(n=0), "n must be in 1..65536"),
    ("n 65537", dict(n=65537), "n must be in 1..65536"),
    ("pad 2", dict(pad=2), "pad must be 0 or 1"),
    ("axis 2", dict(axis=2), "axis must be 0 or 1"),
    ("axis -1", dict(axis=-1), "axis must be 0 or 1"),
    ("inverse 2", dict(inverse=2), "inverse must be 0 or 1"),
    ("reserved0", dict(reserved0=7), "reserved0 must be 0"),
    ("in_pitch", dict(in_pitch=99), "in_pitch smaller than the input's columns"),
    ("in_pair_pitch", dict(in_pair_pitch=9999), "in_pair_pitch does not cover a plane"),
    ("out_pitch", dict(out_pitch=99), "out_pitch smaller than the output's columns"),
    ("out_pair_pitch", dict(out_pair_pitch=199 * 104 + 99), "out_pair_pitch does not cover a plane"),
    ("out inside in", dict(out=R + 4 * 29999), "out overlaps in"),
]


@pytest.mark.parametrize("i", range(len(PE_REFUSED)), ids=[r[0] for r in PE_REFUSED])
def test_path_enhance_refusals_in_their_order(capix, i):
    lib = capix.lib()
    _, change, message = PE_REFUSED[i]
    a = pe_args(capix, **change)
    for who, call in PE_CALLS:
        assert call(lib, a) == BAD and lib.jsgx_last_error() == f"{who}: {message}".encode(), (who, PE_REFUSED[i][0], lib.jsgx_last_error())
    # with any later defect on top, the earlier one is still the one reported
    who, call = PE_CALLS[0]
    for _, later, later_message in PE_REFUSED[i + 1:]:
        if later_message == message or set(later) & set(change):
            continue
        assert call(lib, pe_args(capix, **dict(later, **change))) == BAD
        assert lib.jsgx_last_error() == f"{who}: {message}".encode(), (PE_REFUSED[i][0], later)


@pytest.mark.parametrize("i", range(len(LAG_REFUSED)), ids=[r[0] for r in LAG_REFUSED])
def test_lag_refusals_in_their_order(capix, i):
    lib = capix.lib()
    _, change, message = LAG_REFUSED[i]
    assert lib.jsgx_lag_launch(C.byref(lag_args(capix, **change)), None) == BAD and lib.jsgx_last_error() == f"jsgx_lag_launch: {message}".encode(), lib.jsgx_last_error()
    for _, later, later_message in LAG_REFUSED[i + 1:]:
        if later_message == message or set(later) & set(change):
            continue
        assert lib.jsgx_lag_launch(C.byref(lag_args(capix, **dict(later, **change))), None) == BAD
        assert lib.jsgx_last_error() == f"jsgx_lag_launch: {message}".encode(), (LAG_REFUSED[i][0], later)


def test_what_passes_and_the_shapes_of_the_lag_planes(capix):
    lib = capix.lib()
    plan = lambda **kw: lib.jsgx_path_enhance_plan(C.byref(pe_args(capix, **kw)), None, 0, None, None, None, None)
    assert plan() == 0
    # an output next to an input, not inside it; one pair: the pair pitches are not looked at; reaches of 0 and 64; the clip off
    assert plan(out=R - 4 * OUT_SPAN) == 0 and plan(out=TAP_W + 4 * 3000) == 0 and plan(out=FIRST + 4 * 8) == 0
    assert plan(pairs=1, r_pair_pitch=0, out_pair_pitch=0) == 0 and plan(reach_i=0, reach_j=64, clip=0) == 0 and plan(n_filters=32, n_taps=1 << 20) == 0
    for call in (lib.jsgx_path_enhance_launch(None, None), lib.jsgx_path_enhance_plan(None, None, 0, None, None, None, None), lib.jsgx_lag_launch(None, None)):
        assert call == BAD and lib.jsgx_last_error().endswith(b": null argument")
    assert lib.jsgx_path_enhance_plan(C.byref(pe_args(capix)), C.create_string_buffer(31), 31, None, None, None, None) == BAD
    assert lib.jsgx_last_error() == b"jsgx_path_enhance_plan: bad argument"
    import torch
    if torch.cuda.is_available():           # with a device the calls below would launch on pointers that are no memory
        return
    NO_DEVICE = capix.JSGX_ERR_NO_DEVICE
    assert lib.jsgx_path_enhance_launch(C.byref(pe_args(capix)), None) == NO_DEVICE and lib.jsgx_last_error() == b"jsgx_path_enhance_launch: no HIP device"
    lag = lambda **kw: lib.jsgx_lag_launch(C.byref(lag_args(capix, **kw)), None)
    assert lag() == NO_DEVICE and lib.jsgx_last_error() == b"jsgx_lag_launch: no HIP device"
    # the planes of every form: to lag the output has L rows (axis 1) or L columns (axis 0); from lag the input has
    assert lag(out=R + 4 * 30000) == NO_DEVICE and lag(pairs=1, in_pair_pitch=0, out_pair_pitch=0) == NO_DEVICE
    assert lag(pad=0, out_pair_pitch=99 * 104 + 100) == NO_DEVICE and lag(pad=0, out_pair_pitch=99 * 104 + 99) == BAD
    assert lag(axis=0, out_pitch=200, out_pair_pitch=100 * 200) == NO_DEVICE and lag(axis=0, out_pitch=199) == BAD
    assert lag(axis=0, pad=0, out_pitch=100, out_pair_pitch=10000) == NO_DEVICE
    assert lag(inverse=1, in_pair_pitch=200 * 100, out_pitch=100, out_pair_pitch=10000) == NO_DEVICE and lag(inverse=1, in_pair_pitch=199 * 100 + 99) == BAD
    assert lag(inverse=1, axis=0, in_pitch=200, in_pair_pitch=100 * 200, out_pitch=100, out_pair_pitch=10000) == NO_DEVICE and lag(inverse=1, axis=0, in_pitch=199) == BAD


def test_the_plan_over_reaches(jsg, capix):
    for ri in (0, 1, 25, 32, 64):
        for rj in (0, 1, 25, 32, 64):
            pitch = (64 + 2 * rj + 3) // 4 * 4 + 1
            want = ("path_enhance_tiles", capix.PE_TILE, capix.PE_TILE, capix.PE_THREADS, 4 * (64 + 2 * ri) * pitch)
            for n, m, pairs in ((1, 1, 1), (64, 64, 1), (65536, 65536, 3)):
                assert jsg.path_enhance_plan(ri, rj, n, m, pairs) == want and pitch % 4 == 1 and want[4] <= capix.PE_LDS_LIMIT
    assert jsg.path_enhance_plan(64, 64)[4] == 148224 and jsg.path_enhance_plan(32, 32)[4] == 66048 and 2 * 66048 <= capix.PE_LDS_LIMIT
    hdr = open(os.path.join(ROOT, "include", "jsgx.h")).read()
    for name, value in (("JSGX_PE_MAX_REACH", capix.PE_MAX_REACH), ("JSGX_PE_MAX_FILTERS", capix.PE_MAX_FILTERS), ("JSGX_PE_MAX_TAPS", capix.PE_MAX_TAPS),
                        ("JSGX_PE_TILE", capix.PE_TILE), ("JSGX_PE_THREADS", capix.PE_THREADS), ("JSGX_PE_LDS_LIMIT", capix.PE_LDS_LIMIT),
                        ("JSGX_PE_MIN_WINDOW", capix.PE_MIN_WINDOW), ("JSGX_PE_MAX_WINDOW", capix.PE_MAX_WINDOW), ("JSGX_LAG_THREADS", capix.LAG_THREADS),
                        ("JSGX_LAG_TILE", capix.LAG_TILE), ("JSGX_LAG_LDS_BYTES", capix.LAG_LDS_BYTES), ("JSGX_ABI_VERSION", 1)):
        assert re.search(rf"#define {name} {value}\b", hdr), name
    assert (capix.PE_MAX_REACH, capix.PE_MAX_FILTERS, capix.PE_MAX_TAPS, capix.PE_TILE, capix.PE_THREADS) == (64, 32, 1 << 20, 64, 256)
    assert capix.LAG_LDS_BYTES == (2 * capix.LAG_TILE - 1) * capix.LAG_TILE * 4
    for kernel in ("path_enhance_tiles", "lag_columns", "lag_rows"):
        assert f'"{kernel}"' in hdr
    assert capix.lib().jsgx_abi_version() == 1


@pytest.mark.parametrize("struct, size, ctype", [("jsgx_path_enhance_args", 104, "PathEnhanceArgs"), ("jsgx_lag_args", 72, "LagArgs")])
def test_struct_layout_matches_the_header(capix, tmp_path, struct, size, ctype):
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsgx.h")).read(), flags=re.S)
    body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", hdr, flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*(\[\d+\])?\s*$", decl).group(1) for decl in body.split(";") if decl.strip()]
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "jsgx.h"', "int main(void) {", f'    printf("%zu\\n", sizeof({struct}));']
    lines += [f'    printf("{f} %zu %zu\\n", offsetof({struct}, {f}), sizeof((({struct}*)0)->{f}));' for f in names]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)])
    out = subprocess.check_output([str(tmp_path / "layout")], text=True).split("\n")
    ctype = getattr(capix, ctype)
    assert out[0] == str(C.sizeof(ctype)) == str(size)
    assert [f.rstrip("_") for f, _ in ctype._fields_] == names          # `in` is a Python keyword: in_
    offset = 0
    for (f, _), line in zip(ctype._fields_, out[1:]):
        assert line == f"{f.rstrip('_')} {getattr(ctype, f).offset} {getattr(ctype, f).size}"
        assert getattr(ctype, f).offset == offset, f"padding in front of {f}"
        offset += getattr(ctype, f).size


def test_python_names(jsg):
    bank = ["window", "max_ratio", "min_ratio", "n_filters", "zero_mean", "drop_below"]
    want = {
        "diagonal_filter": ["window", "n", "slope", "zero_mean"],
        "path_enhance_filters": ["n"] + bank,
        "path_enhance": ["R", "n"] + bank + ["clip", "out"],
        "path_enhance_launch": ["d_r", "d_tap_w", "d_tap_at", "d_filter_first", "d_out", "reach_i", "reach_j", "clip", "stream"],
        "path_enhance_plan": ["reach_i", "reach_j", "n", "m", "pairs"],
        "recurrence_to_lag": ["R", "pad", "axis"],
        "lag_to_recurrence": ["lag", "axis"],
        "lag_launch": ["d_in", "d_out", "pad", "axis", "inverse", "stream"],
    }
    for name, params in want.items():
        assert callable(getattr(jsg, name)) and name in jsg.__all__
        assert list(inspect.signature(getattr(jsg, name)).parameters) == params, name
    assert [p.default for p in inspect.signature(jsg.path_enhance_filters).parameters.values()][1:] == ["hann", 2.0, None, 7, False, 0.0]
    assert [p.default for p in inspect.signature(jsg.path_enhance).parameters.values()][2:] == ["hann", 2.0, None, 7, False, 0.0, True, None]
    assert [p.default for p in inspect.signature(jsg.diagonal_filter).parameters.values()][2:] == [1.0, False]
    assert [p.default for p in inspect.signature(jsg.recurrence_to_lag).parameters.values()][1:] == [True, -1]
    assert inspect.signature(jsg.lag_to_recurrence).parameters["axis"].default == -1
    symbols = {"jsgx_path_enhance_launch", "jsgx_path_enhance_plan", "jsgx_diagonal_filter_build", "jsgx_diagonal_filter_table", "jsgx_lag_launch"}
    assert symbols <= set(jsg.capix.SIGNATURES)
    assert shutil.which("nm"), "nm (binutils) lists the exported symbols"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", jsg.capix.LIB_PATH], text=True)
    assert symbols <= {line.split()[-1] for line in exported.splitlines() if " T " in line}
    # the symmetric Hann window and the slope-1 table
    import numpy as np
    t = jsg.diagonal_filter("hann", 5)
    assert t.shape == (5, 5) and np.allclose(np.diag(t), np.array([0, 0.5, 1, 0.5, 0]) / 2.0) and t.sum() == 1.0 and np.count_nonzero(t) == 3


def test_kernel_notes(capix, tmp_path):
    """The new object: its five kernels, no private segment (no scratch memory, no spills), the LDS the header states (the enhancement's
    is dynamic: none is static) and 256 lanes a workgroup."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    obj = os.path.join(ROOT, "jadespectrogram_amd", "build", "jsgx_path_enhance.o")
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
        assert int(g("vgpr_count")) <= 128, name           # two workgroups of four wavefronts a compute unit and more keep their registers
    columns = (0, capix.LAG_LDS_BYTES, 0, 0, capix.LAG_THREADS)
    rows = (0, 0, 0, 0, capix.LAG_THREADS)
    assert found == {"jsgx::path_enhance_kernel": (0, 0, 0, 0, capix.PE_THREADS), "jsgx::lag_columns_kernel<true>": columns, "jsgx::lag_columns_kernel<false>": columns,
                     "jsgx::lag_rows_kernel<true>": rows, "jsgx::lag_rows_kernel<false>": rows}


def test_host_entry_points_under_asan_ubsan(capix):
    """tests/cpp/jsgx_path_enhance_host_test.cpp (its own main: the refusals in their order, the plan over reaches, the builder with guard
    bytes round its outputs) built together with the host units it calls under the address and undefined-behaviour sanitizers and run as a
    child process; the same program against the shipped library, there with the refusals of the launches, gives the same verdict."""
    d = tempfile.gettempdir()
    drv = os.path.join(ROOT, "tests", "cpp", "jsgx_path_enhance_host_test.cpp")
    hosts = [os.path.join(ROOT, "jadespectrogram_amd", "csrc", f) for f in ("jsgx_beat_host.cpp", "jsgx_path_enhance_host.cpp")]
    common = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]
    san = os.path.join(d, "jsgx_path_enhance_host_san")
    subprocess.check_call(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"] + hosts + [drv, "-o", san])
    libdir = os.path.dirname(capix.LIB_PATH)
    shipped = os.path.join(d, "jsgx_path_enhance_host_lib")
    subprocess.check_call(common + ["-DJSGX_PE_TEST_LAUNCHES", drv, "-o", shipped, "-L", libdir, "-ljsgx", f"-Wl,-rpath,{libdir}"])
    for exe in (san, shipped):
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == "ok" and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr

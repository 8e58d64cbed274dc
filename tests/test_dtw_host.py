"""Sections 2 and 3 of the companion library, host side (include/jsgx.h): every refusal of the cost and of the time warping in its stated
order (all decided without a device), the plans over shapes, the scratch size, the struct layouts against a C program, the Python names,
the kernels' notes, and the host entry points from a stand-alone C++ program under the address and undefined-behaviour sanitizers.  CPU
only."""
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
X, Y, COST, ACC, PATH_I, PATH_J, PATH_LEN, TOTAL, SCRATCH = (i << 44 for i in range(1, 10))
BAD = -2


@pytest.fixture(scope="module")
def capix(jsg):
    if not os.path.exists(jsg.capix.LIB_PATH):
        from jadespectrogram_amd import _build
        _build.build_lib()
    jsg.capix.lib()
    return jsg.capix


def cost_args(capix, **kw):
    a = dict(x=X, x_frame_pitch=20, x_pair_pitch=0, y=Y, y_frame_pitch=24, y_pair_pitch=300 * 24, pairs=3, n_features=20, n=100, m=300, metric=2, reserved0=0,
             cost=COST, cost_pitch=300, cost_pair_pitch=30000)
    a.update(kw)
    return capix.CdistArgs(**a)


def dtw_args(capix, **kw):
    a = dict(cost=COST, cost_pitch=300, cost_pair_pitch=30000, pairs=3, n=100, m=300, subseq=0, band=0, reserved0=0, weights_mul=(1.0, 1.0, 1.0),
             weights_add=(0.0, 0.0, 0.0), acc=ACC, acc_pitch=300, acc_pair_pitch=30000, path_i=PATH_I, path_j=PATH_J, path_pitch=399, max_path=399,
             path_len=PATH_LEN, total=TOTAL)
    a.update(kw)
    a["weights_mul"], a["weights_add"] = (C.c_float * 3)(*a["weights_mul"]), (C.c_float * 3)(*a["weights_add"])
    return capix.DtwArgs(**a)


# in the order of the header: a call with two defects is refused for the earlier one
COST_REFUSED = [
    ("null x", dict(x=None), "null x"),
    ("null y", dict(y=None), "null y"),
    ("null cost", dict(cost=None), "null cost"),
    ("misaligned x", dict(x=X + 1), "pointers must be 4-byte aligned"),
    ("misaligned cost", dict(cost=COST + 2), "pointers must be 4-byte aligned"),
    ("no pairs", dict(pairs=0), "pairs must be in 1..65535"),
    ("65536 pairs", dict(pairs=65536), "pairs must be in 1..65535"),
    ("no features", dict(n_features=0), "n_features must be in 1..1024"),
    ("1025 features", dict(n_features=1025, x_frame_pitch=1025, y_frame_pitch=1025, y_pair_pitch=300 * 1025), "n_features must be in 1..1024"),
    ("n 0", dict(n=0), "n must be in 1..65536"),
    ("n 65537", dict(n=65537, cost_pair_pitch=65537 * 300), "n must be in 1..65536"),
    ("m 0", dict(m=0), "m must be in 1..65536"),
    ("m 65537", dict(m=65537, cost_pitch=65537, cost_pair_pitch=65537 * 100, y_pair_pitch=65537 * 24), "m must be in 1..65536"),
    ("metric 3", dict(metric=3), "metric must be in 0..2"),
    ("metric -1", dict(metric=-1), "metric must be in 0..2"),
    ("reserved0", dict(reserved0=1), "reserved0 must be 0"),
    ("x_frame_pitch", dict(x_frame_pitch=19), "x_frame_pitch smaller than n_features"),
    ("y_frame_pitch", dict(y_frame_pitch=19), "y_frame_pitch smaller than n_features"),
    ("x_pair_pitch", dict(x_pair_pitch=99 * 20 + 19), "x_pair_pitch does not cover a sequence"),
    ("y_pair_pitch", dict(y_pair_pitch=299 * 24 + 19), "y_pair_pitch does not cover a sequence"),
    ("cost_pitch", dict(cost_pitch=299), "cost_pitch smaller than m"),
    ("cost_pair_pitch", dict(cost_pair_pitch=29999), "cost_pair_pitch does not cover a plane"),
    ("cost ends in x", dict(cost=X - 4 * 90000 + 4), "cost overlaps x"),
    ("cost inside y", dict(cost=Y + 4 * 1000), "cost overlaps y"),
]
DTW_REFUSED = [
    ("null cost", dict(cost=None), "null cost"),
    ("null acc", dict(acc=None), "null acc"),
    ("path_i alone", dict(path_j=None), "path_i and path_j go together"),
    ("path_j alone", dict(path_i=None), "path_i and path_j go together"),
    ("paths without path_len", dict(path_len=None), "null path_len with paths"),
    ("misaligned acc", dict(acc=ACC + 2), "pointers must be 4-byte aligned"),
    ("misaligned total", dict(total=TOTAL + 1), "pointers must be 4-byte aligned"),
    ("no pairs", dict(pairs=0), "pairs must be in 1..65535"),
    ("n 0", dict(n=0), "n must be in 1..65536"),
    ("n 65537", dict(n=65537, cost_pair_pitch=65537 * 300, acc_pair_pitch=65537 * 300, max_path=70000, path_pitch=70000), "n must be in 1..65536"),
    ("m 0", dict(m=0), "m must be in 1..65536"),
    ("subseq 2", dict(subseq=2), "subseq must be 0 or 1"),
    ("band -1", dict(band=-1), "band must be in 0..65536"),
    ("band 65537", dict(band=65537), "band must be in 0..65536"),
    ("weights_mul nan", dict(weights_mul=(1.0, float("nan"), 1.0)), "weights must be finite"),
    ("weights_add inf", dict(weights_add=(0.0, 0.0, float("inf"))), "weights must be finite"),
    ("reserved0", dict(reserved0=1), "reserved0 must be 0"),
    ("band with subseq", dict(band=2, subseq=1), "band and subseq exclude each other"),
    ("max_path", dict(max_path=398), "max_path smaller than n + m - 1"),
    ("cost_pitch", dict(cost_pitch=299), "cost_pitch smaller than m"),
    ("cost_pair_pitch", dict(cost_pair_pitch=29999), "cost_pair_pitch does not cover a plane"),
    ("acc_pitch", dict(acc_pitch=299), "acc_pitch smaller than m"),
    ("acc_pair_pitch", dict(acc_pair_pitch=29999), "acc_pair_pitch does not cover a plane"),
    ("path_pitch", dict(path_pitch=398), "path_pitch smaller than max_path"),
    ("acc ends in cost", dict(acc=COST - 4 * 90000 + 4), "acc overlaps cost"),
    ("path_len inside cost", dict(path_len=COST + 4 * 50000), "an output overlaps cost"),
    ("total inside acc", dict(total=ACC + 4 * 89999), "an output overlaps acc"),
]
COST_CALLS = (("jsgx_cdist_launch", lambda lib, a: lib.jsgx_cdist_launch(C.byref(a), None)),
              ("jsgx_cdist_plan", lambda lib, a: lib.jsgx_cdist_plan(C.byref(a), None, 0, None, None)))
DTW_CALLS = (("jsgx_dtw_launch", lambda lib, a: lib.jsgx_dtw_launch(C.byref(a), SCRATCH, 1 << 40, None)),
             ("jsgx_dtw_scratch_bytes", lambda lib, a: lib.jsgx_dtw_scratch_bytes(C.byref(a))),
             ("jsgx_dtw_plan", lambda lib, a: lib.jsgx_dtw_plan(C.byref(a), None, 0, None, None, None, None, None)))


def in_order(capix, refused, make, calls, i):
    lib = capix.lib()
    _, change, message = refused[i]
    a = make(capix, **change)
    for who, call in calls:
        assert call(lib, a) == BAD and lib.jsgx_last_error() == f"{who}: {message}".encode()
    # with any later defect on top, the earlier one is still the one reported
    who, call = calls[0]
    for _, later, later_message in refused[i + 1:]:
        if later_message == message or set(later) & set(change):
            continue
        assert call(lib, make(capix, **dict(later, **change))) == BAD
        assert lib.jsgx_last_error() == f"{who}: {message}".encode(), (refused[i][0], later)


@pytest.mark.parametrize("i", range(len(COST_REFUSED)), ids=[r[0] for r in COST_REFUSED])
def test_cost_refusals_in_their_order(capix, i):
    in_order(capix, COST_REFUSED, cost_args, COST_CALLS, i)


@pytest.mark.parametrize("i", range(len(DTW_REFUSED)), ids=[r[0] for r in DTW_REFUSED])
def test_dtw_refusals_in_their_order(capix, i):
    in_order(capix, DTW_REFUSED, dtw_args, DTW_CALLS, i)
    # ... also ahead of what only the launch refuses
    a = dtw_args(capix, **DTW_REFUSED[i][1])
    assert capix.lib().jsgx_dtw_launch(C.byref(a), None, 0, None) == BAD and capix.lib().jsgx_last_error() == f"jsgx_dtw_launch: {DTW_REFUSED[i][2]}".encode()


def test_what_only_the_launch_refuses_and_what_passes(capix):
    lib = capix.lib()
    a = dtw_args(capix)
    for scratch, size, message in ((None, 1 << 40, "null scratch"), (SCRATCH + 2, 1 << 40, "scratch must be 4-byte aligned"),
                                   (SCRATCH, 8 * 3 * 399 - 1, "scratch smaller than jsgx_dtw_scratch_bytes"), (None, 0, "null scratch"),
                                   (SCRATCH + 1, 0, "scratch must be 4-byte aligned")):
        assert lib.jsgx_dtw_launch(C.byref(a), scratch, size, None) == BAD and lib.jsgx_last_error() == f"jsgx_dtw_launch: {message}".encode()
    for call in (lib.jsgx_dtw_launch(None, SCRATCH, 1 << 40, None), lib.jsgx_dtw_scratch_bytes(None), lib.jsgx_dtw_plan(None, None, 0, None, None, None, None, None),
                 lib.jsgx_cdist_launch(None, None), lib.jsgx_cdist_plan(None, None, 0, None, None)):
        assert call == BAD and lib.jsgx_last_error().endswith(b": null argument")
    size = lambda **kw: lib.jsgx_dtw_scratch_bytes(C.byref(dtw_args(capix, **kw)))
    # one pair: the pair pitches are not looked at; the optional outputs may be missing; max_path matters with paths only
    assert size(pairs=1, cost_pair_pitch=0, acc_pair_pitch=0, path_pitch=0) == 8 * 399
    assert size(total=None) == 8 * 3 * 399 and size(path_i=None, path_j=None, max_path=0, path_pitch=0) == 0
    assert size(path_i=None, path_j=None, path_len=None, total=None, max_path=0) == 0
    assert size(subseq=1) > 0 and size(band=65536) > 0 and size(weights_mul=(0.0, -1.0, 1e30), weights_add=(-5.0, 0.0, 0.0)) > 0
    # an output next to an input, not inside it
    assert size(acc=COST - 4 * 90000) > 0 and size(acc=COST + 4 * 90000) > 0 and size(total=ACC + 4 * 90000) > 0
    plan = lambda **kw: lib.jsgx_cdist_plan(C.byref(cost_args(capix, **kw)), None, 0, None, None)
    assert plan() == 0 and plan(x_pair_pitch=2000, y_pair_pitch=0) == 0 and plan(pairs=1, cost_pair_pitch=0) == 0
    assert plan(cost=X - 4 * 90000) == 0 and plan(cost=X + 4 * 2000) == 0 and plan(cost=Y + 4 * (2 * 7200 + 299 * 24 + 20)) == 0


def test_no_device_comes_after_the_refusals(capix):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = capix.lib()
    assert lib.jsgx_cdist_launch(C.byref(cost_args(capix)), None) == capix.JSGX_ERR_NO_DEVICE
    assert lib.jsgx_last_error() == b"jsgx_cdist_launch: no HIP device"
    assert lib.jsgx_dtw_launch(C.byref(dtw_args(capix)), SCRATCH, 1 << 40, None) == capix.JSGX_ERR_NO_DEVICE
    assert lib.jsgx_last_error() == b"jsgx_dtw_launch: no HIP device"
    assert lib.jsgx_dtw_launch(C.byref(dtw_args(capix)), SCRATCH, 16, None) == BAD
    # without paths there is no scratch to refuse
    assert lib.jsgx_dtw_launch(C.byref(dtw_args(capix, path_i=None, path_j=None, max_path=0)), None, 0, None) == capix.JSGX_ERR_NO_DEVICE


def test_plans_and_scratch_over_shapes(jsg, capix):
    TR, TC = capix.DTW_TILE_ROWS, capix.DTW_TILE_COLS
    for n in (1, 2, TR - 1, TR, TR + 1, 2 * TR + 1, 4096, 65536):
        for m in (1, 2, TC - 1, TC, TC + 1, 3 * TC + 2, 16384, 65536):
            diagonals = -(-n // TR) + -(-m // TC) - 1
            assert jsg.dtw_plan(n, m) == ("dtw_tiles", TR, TC, diagonals + 1, capix.DTW_THREADS, capix.DTW_LDS_BYTES)
            assert jsg.dtw_plan(n, m, pairs=7, backtrack=False)[3] == diagonals
            for pairs in (1, 5):
                a = dtw_args(capix, pairs=pairs, n=n, m=m, cost_pitch=m, acc_pitch=m, cost_pair_pitch=n * m, acc_pair_pitch=n * m, max_path=n + m - 1, path_pitch=n + m)
                assert capix.lib().jsgx_dtw_scratch_bytes(C.byref(a)) == 8 * pairs * (n + m - 1)
    assert 0 < capix.DTW_LDS_BYTES <= 163840 and capix.DTW_LDS_BYTES == 4 * (TR * TC + TC + 4)
    for metric in ("sqeuclidean", "euclidean", "cosine"):
        for n, m, K in ((1, 1, 1), (63, 65, 12), (65536, 65536, 1024)):
            assert jsg.cdist_plan(n, m, K, pairs=2, metric=metric) == ("cdist_64x64", capix.CDIST_THREADS, capix.CDIST_LDS_BYTES)
    assert capix.CDIST_LDS_BYTES == 2 * 32 * (capix.CDIST_TILE + 4) * 4
    with pytest.raises(jsg.JsgError, match="metric must be one of"):
        jsg.cdist_plan(4, 4, 4, metric="manhattan")
    with pytest.raises(jsg.JsgError, match="n must be in"):
        jsg.dtw_plan(0, 5)
    hdr = open(os.path.join(ROOT, "include", "jsgx.h")).read()
    for name, value in (("JSGX_DTW_TILE_ROWS", TR), ("JSGX_DTW_TILE_COLS", TC), ("JSGX_DTW_THREADS", capix.DTW_THREADS), ("JSGX_DTW_LDS_BYTES", capix.DTW_LDS_BYTES),
                        ("JSGX_CDIST_TILE", capix.CDIST_TILE), ("JSGX_CDIST_THREADS", capix.CDIST_THREADS), ("JSGX_CDIST_LDS_BYTES", capix.CDIST_LDS_BYTES),
                        ("JSGX_CDIST_MAX_FEATURES", capix.CDIST_MAX_FEATURES), ("JSGX_DTW_MAX_LEN", capix.DTW_MAX_LEN), ("JSGX_METRIC_SQEUCLIDEAN", capix.METRIC_SQEUCLIDEAN),
                        ("JSGX_METRIC_EUCLIDEAN", capix.METRIC_EUCLIDEAN), ("JSGX_METRIC_COSINE", capix.METRIC_COSINE)):
        assert re.search(rf"#define {name} {value}\b", hdr), name
    assert "additions do not bump" in hdr or "grows by addition only" in hdr


def test_python_names(jsg):
    want = {
        "cdist": ["X", "Y", "metric"],
        "cdist_launch": ["d_x", "d_y", "d_cost", "metric", "stream"],
        "cdist_plan": ["n", "m", "n_features", "pairs", "metric"],
        "dtw": ["X", "Y", "C", "metric", "weights_mul", "weights_add", "subseq", "band", "backtrack"],
        "dtw_scratch_bytes": ["d_cost", "d_acc", "weights_mul", "weights_add", "subseq", "band", "d_path_i", "d_path_j", "d_path_len", "d_total"],
        "dtw_launch": ["d_cost", "d_acc", "weights_mul", "weights_add", "subseq", "band", "d_path_i", "d_path_j", "d_path_len", "d_total", "d_scratch", "stream"],
        "dtw_plan": ["n", "m", "pairs", "backtrack"],
    }
    for name, params in want.items():
        assert callable(getattr(jsg, name)) and name in jsg.__all__
        assert list(inspect.signature(getattr(jsg, name)).parameters) == params, name
    sig = inspect.signature(jsg.dtw)
    assert [p.default for p in sig.parameters.values()] == [None, None, None, "euclidean", None, None, False, 0, True]
    assert [p.kind for p in sig.parameters.values()][2:] == [inspect.Parameter.KEYWORD_ONLY] * 7
    assert inspect.signature(jsg.cdist).parameters["metric"].default == "euclidean"


@pytest.mark.parametrize("struct, binding", [("jsgx_cdist_args", "CdistArgs"), ("jsgx_dtw_args", "DtwArgs")])
def test_struct_layouts_match_the_header(capix, tmp_path, struct, binding):
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
    ctype = getattr(capix, binding)
    assert out[0] == str(C.sizeof(ctype))
    assert [f for f, _ in ctype._fields_] == names
    for (f, _), line in zip(ctype._fields_, out[1:]):
        assert line == f"{f} {getattr(ctype, f).offset} {getattr(ctype, f).size}"


def test_kernel_notes(capix, tmp_path):
    """The new objects: their kernels, no private segment (no scratch memory, no spills), and the static LDS the header and the plans state."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    found = {}
    for unit in ("jsgx_cdist.o", "jsgx_dtw.o"):
        obj = os.path.join(ROOT, "jadespectrogram_amd", "build", unit)
        if not os.path.exists(obj):
            from jadespectrogram_amd import _build
            _build.build_lib()
        co = kernel_regs.code_object(obj, str(tmp_path))
        notes = subprocess.check_output([os.path.join(kernel_regs.LLVM, "llvm-readelf"), "--notes", co]).decode()
        for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
            g = lambda k: re.search(rf"\.{k}:\s+(\S+)", blk).group(1)
            name = subprocess.check_output(["c++filt", g("name")]).decode().strip()
            found[(unit, name.split("(")[0].replace("void ", ""))] = (int(g("private_segment_fixed_size")), int(g("group_segment_fixed_size")), int(g("vgpr_spill_count")),
                                                                       int(g("sgpr_spill_count")), int(g("max_flat_workgroup_size")))
    cost = (0, capix.CDIST_LDS_BYTES, 0, 0, capix.CDIST_THREADS)
    assert found == {("jsgx_cdist.o", "jsgx::cdist_kernel<0>"): cost, ("jsgx_cdist.o", "jsgx::cdist_kernel<1>"): cost, ("jsgx_cdist.o", "jsgx::cdist_kernel<2>"): cost,
                     ("jsgx_dtw.o", "jsgx::dtw_kernel"): (0, capix.DTW_LDS_BYTES, 0, 0, capix.DTW_THREADS),
                     ("jsgx_dtw.o", "jsgx::dtw_backtrace_kernel"): (0, found[("jsgx_dtw.o", "jsgx::dtw_backtrace_kernel")][1], 0, 0, capix.DTW_THREADS)}
    assert found[("jsgx_dtw.o", "jsgx::dtw_backtrace_kernel")][1] <= 16384


def test_host_entry_points_under_asan_ubsan(capix):
    """tests/cpp/jsgx_dtw_host_test.cpp (its own main: the plans, the scratch size, the refusals) built together with both host units of the
    library under the address and undefined-behaviour sanitizers and run as a child process; the same program against the shipped library
    gives the same verdict."""
    d = tempfile.gettempdir()
    drv = os.path.join(ROOT, "tests", "cpp", "jsgx_dtw_host_test.cpp")
    hosts = [os.path.join(ROOT, "jadespectrogram_amd", "csrc", f) for f in ("jsgx_beat_host.cpp", "jsgx_dtw_host.cpp")]
    common = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]
    san = os.path.join(d, "jsgx_dtw_host_san")
    subprocess.check_call(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"] + hosts + [drv, "-o", san])
    libdir = os.path.dirname(capix.LIB_PATH)
    shipped = os.path.join(d, "jsgx_dtw_host_lib")
    subprocess.check_call(common + [drv, "-o", shipped, "-L", libdir, "-ljsgx", f"-Wl,-rpath,{libdir}"])
    for exe in (san, shipped):
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == "ok" and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr

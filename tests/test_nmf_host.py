"""Section 12 of the companion library, host side (include/jsgx.h): every refusal of the factorisation in its stated order (all decided
without a device), the plan and the scratch arithmetic, the struct layout against a C program, the header's constants, the exported
symbols, the Python names, the kernels' notes, and the host entry points from a stand-alone C++ program under the address and
undefined-behaviour sanitizers.  CPU only."""
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
V, A, CC, SCRATCH = (i << 44 for i in range(1, 5))
BAD = -2
NEED = 27552            # 4 * 3 * 7 * (7 * (2 + 2) + 1 * 300): two chunks of bins, one of frames
V_SPAN, A_SPAN, C_SPAN = 2 * 30000 + 99 * 300 + 300, 2 * 800 + 99 * 8 + 7, 2 * 2128 + 6 * 304 + 300


@pytest.fixture(scope="module")
def capix(jsg):
    if not os.path.exists(jsg.capix.LIB_PATH):
        from jadespectrogram_amd import _build
        _build.build_lib()
    jsg.capix.lib()
    return jsg.capix


def nmf_args(capix, **kw):       # 3 problems of 100 frames x 300 bins, 7 components
    a = dict(v=V, v_pitch=300, v_problem_pitch=30000, a=A, a_pitch=8, a_problem_pitch=800, c=CC, c_pitch=304, c_problem_pitch=2128, problems=3, n_frames=100,
             n_bins=300, n_components=7, n_iter=5, update_components=1, loss=0, reserved0=0)
    a.update(kw)
    return capix.NmfArgs(**a)


# in the order of the header: a call with two defects is refused for the earlier one.  "scratch" and "scratch_bytes" are the launch's own.
REFUSED = [
    ("null v", dict(v=None), "null v"),
    ("null a", dict(a=None), "null a"),
    ("null c", dict(c=None), "null c"),
    ("misaligned v", dict(v=V + 2), "pointers must be 4-byte aligned"),
    ("misaligned c", dict(c=CC + 1), "pointers must be 4-byte aligned"),
    ("no problems", dict(problems=0), "problems must be in 1..65535"),
    ("65536 problems", dict(problems=65536), "problems must be in 1..65535"),
    ("no frames", dict(n_frames=0), "n_frames must be in 1..16777216"),
    ("too many frames", dict(n_frames=(1 << 24) + 1), "n_frames must be in 1..16777216"),
    ("no bins", dict(n_bins=0), "n_bins must be in 1..16384"),
    ("16385 bins", dict(n_bins=16385), "n_bins must be in 1..16384"),
    ("no components", dict(n_components=0), "n_components must be in 1..64"),
    ("65 components", dict(n_components=65), "n_components must be in 1..64"),
    ("no iteration", dict(n_iter=0), "n_iter must be in 1..65536"),
    ("65537 iterations", dict(n_iter=65537), "n_iter must be in 1..65536"),
    ("update_components 2", dict(update_components=2), "update_components must be 0 or 1"),
    ("another loss", dict(loss=1), "loss must be JSGX_NMF_FROBENIUS"),
    ("reserved0", dict(reserved0=5), "reserved0 must be 0"),
    ("v_pitch", dict(v_pitch=299), "v_pitch smaller than n_bins"),
    ("v_problem_pitch", dict(v_problem_pitch=29999), "v_problem_pitch does not cover a plane"),
    ("a_pitch", dict(a_pitch=6), "a_pitch smaller than n_components"),
    ("a_problem_pitch", dict(a_problem_pitch=99 * 8 + 6), "a_problem_pitch does not cover a plane"),
    ("c_pitch", dict(c_pitch=299), "c_pitch smaller than n_bins"),
    ("c_problem_pitch", dict(c_problem_pitch=6 * 304 + 299), "c_problem_pitch does not cover a plane"),
    ("a ends in v", dict(a=V - 4 * A_SPAN + 4), "a overlaps v"),
    ("c inside v", dict(c=V + 4 * 1000), "c overlaps v"),
    ("a inside c", dict(a=CC + 4 * (C_SPAN - 1)), "a overlaps c"),
    ("null scratch", dict(scratch=None), "null scratch"),
    ("misaligned scratch", dict(scratch=SCRATCH + 2), "scratch must be 4-byte aligned"),
    ("small scratch", dict(scratch_bytes=NEED - 1), "scratch smaller than jsgx_nmf_scratch_bytes"),
    ("scratch ends in v", dict(scratch=V - NEED + 4), "scratch overlaps v"),
    ("scratch inside a", dict(scratch=A + 4 * (A_SPAN - 1)), "scratch overlaps a"),
    ("scratch inside c", dict(scratch=CC + 4 * 10), "scratch overlaps c"),
]


def launch(lib, capix, change):
    change = dict(change)
    scratch, scratch_bytes = change.pop("scratch", SCRATCH), change.pop("scratch_bytes", NEED)
    return lib.jsgx_nmf_launch(C.byref(nmf_args(capix, **change)), scratch, scratch_bytes, None)


@pytest.mark.parametrize("i", range(len(REFUSED)), ids=[r[0] for r in REFUSED])
def test_refusals_in_their_order(capix, i):
    lib = capix.lib()
    _, change, message = REFUSED[i]
    assert launch(lib, capix, change) == BAD and lib.jsgx_last_error() == f"jsgx_nmf_launch: {message}".encode(), lib.jsgx_last_error()
    if not set(change) & {"scratch", "scratch_bytes"}:          # what the launch refuses before it looks at the scratch, the other two calls refuse alike
        a = nmf_args(capix, **change)
        assert lib.jsgx_nmf_plan(C.byref(a), None, 0, None, None, None, None) == BAD and lib.jsgx_last_error() == f"jsgx_nmf_plan: {message}".encode()
        assert lib.jsgx_nmf_scratch_bytes(C.byref(a)) == BAD and lib.jsgx_last_error() == f"jsgx_nmf_scratch_bytes: {message}".encode()
    # with any later defect on top, the earlier one is still the one reported
    for _, later, later_message in REFUSED[i + 1:]:
        if later_message == message or set(later) & set(change):
            continue
        assert launch(lib, capix, dict(later, **change)) == BAD
        assert lib.jsgx_last_error() == f"jsgx_nmf_launch: {message}".encode(), (REFUSED[i][0], later)


def test_what_passes(capix):
    lib = capix.lib()
    size = lambda **kw: lib.jsgx_nmf_scratch_bytes(C.byref(nmf_args(capix, **kw)))
    assert size() == NEED
    # a plane next to another, not inside it; one problem: the problem pitches are not looked at; fixed components
    assert size(a=V - 4 * A_SPAN) == NEED and size(c=V + 4 * V_SPAN) == NEED and size(a=CC + 4 * C_SPAN) == NEED
    assert size(problems=1, v_problem_pitch=0, a_problem_pitch=0, c_problem_pitch=0) == NEED // 3
    assert size(update_components=0) == 4 * 3 * 7 * 7 * (2 + 2) and size(n_iter=65536) == NEED
    for call in (lib.jsgx_nmf_launch(None, SCRATCH, NEED, None), lib.jsgx_nmf_plan(None, None, 0, None, None, None, None), lib.jsgx_nmf_scratch_bytes(None)):
        assert call == BAD and lib.jsgx_last_error().endswith(b": null argument")
    assert lib.jsgx_nmf_plan(C.byref(nmf_args(capix)), C.create_string_buffer(15), 15, None, None, None, None) == BAD
    assert lib.jsgx_last_error() == b"jsgx_nmf_plan: bad argument"
    import torch
    if torch.cuda.is_available():           # with a device the calls below would launch on pointers that are no memory
        return
    NO_DEVICE = capix.JSGX_ERR_NO_DEVICE
    assert launch(lib, capix, {}) == NO_DEVICE and lib.jsgx_last_error() == b"jsgx_nmf_launch: no HIP device"
    # a larger scratch, and one that touches no plane
    assert launch(lib, capix, dict(scratch_bytes=NEED + 4096)) == NO_DEVICE and launch(lib, capix, dict(scratch=V - NEED)) == NO_DEVICE
    assert launch(lib, capix, dict(scratch=A + 4 * A_SPAN)) == NO_DEVICE


def test_the_plan_and_the_scratch_over_shapes(jsg, capix):
    lib = capix.lib()
    ck, ct = capix.NMF_CHUNK_K, capix.NMF_CHUNK_T
    assert ck % 4 == 0 and ct % 4 == 0
    for T in (1, 100, ct, ct + 1, 16384, 1 << 24):
        for K in (1, 300, ck, ck + 1, 16384):
            for r in (1, 7, 64):
                cK, cT = -(-K // ck), -(-T // ct)
                for update in (True, False):
                    assert jsg.nmf_plan(T, K, r, update_components=update) == ("nmf_update_a", capix.NMF_THREADS, capix.NMF_LDS_BYTES, 8 if update else 1, cT)
                    a = capix.NmfArgs(v=V, v_pitch=K, a=A, a_pitch=r, c=CC, c_pitch=K, problems=1, n_frames=T, n_bins=K, n_components=r, n_iter=1, update_components=int(update))
                    assert lib.jsgx_nmf_scratch_bytes(C.byref(a)) == (4 * r * (r * (2 + max(cK, cT)) + cT * K) if update else 4 * r * r * (2 + cK))
    hdr = open(os.path.join(ROOT, "include", "jsgx.h")).read()
    for name, value in (("JSGX_NMF_MAX_COMPONENTS", capix.NMF_MAX_COMPONENTS), ("JSGX_NMF_MAX_BINS", capix.NMF_MAX_BINS), ("JSGX_NMF_MAX_FRAMES", capix.NMF_MAX_FRAMES),
                        ("JSGX_NMF_MAX_ITER", capix.NMF_MAX_ITER), ("JSGX_NMF_CHUNK_K", capix.NMF_CHUNK_K), ("JSGX_NMF_CHUNK_T", capix.NMF_CHUNK_T),
                        ("JSGX_NMF_FROBENIUS", capix.NMF_FROBENIUS), ("JSGX_NMF_THREADS", capix.NMF_THREADS), ("JSGX_NMF_LDS_BYTES", capix.NMF_LDS_BYTES),
                        ("JSGX_ABI_VERSION", 1)):
        assert re.search(rf"#define {name} {value}\b", hdr), name
    assert float(re.search(r"#define JSGX_NMF_EPSILON (\S+?)f\b", hdr).group(1)) == capix.NMF_EPSILON == 2.0 ** -23
    assert (capix.NMF_MAX_COMPONENTS, capix.NMF_MAX_BINS, capix.NMF_MAX_FRAMES, capix.NMF_MAX_ITER) == (64, 16384, 1 << 24, 65536)
    for kernel in ("nmf_gram", "nmf_chunk_sum", "nmf_update_a", "nmf_partial_c", "nmf_update_c"):
        assert f'"{kernel}"' in hdr
    assert capix.lib().jsgx_abi_version() == 1


def test_struct_layout_matches_the_header(capix, tmp_path):
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler")
    struct, ctype = "jsgx_nmf_args", capix.NmfArgs
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsgx.h")).read(), flags=re.S)
    body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", hdr, flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*(\[\d+\])?\s*$", decl).group(1) for decl in body.split(";") if decl.strip()]
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "jsgx.h"', "int main(void) {", f'    printf("%zu\\n", sizeof({struct}));']
    lines += [f'    printf("{f} %zu %zu\\n", offsetof({struct}, {f}), sizeof((({struct}*)0)->{f}));' for f in names]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)])
    out = subprocess.check_output([str(tmp_path / "layout")], text=True).split("\n")
    assert out[0] == str(C.sizeof(ctype)) == "104"
    assert [f for f, _ in ctype._fields_] == names
    offset = 0
    for (f, _), line in zip(ctype._fields_, out[1:]):
        assert line == f"{f} {getattr(ctype, f).offset} {getattr(ctype, f).size}"
        assert getattr(ctype, f).offset == offset, f"padding in front of {f}"
        offset += getattr(ctype, f).size


def test_python_names(jsg):
    want = {
        "nmf_launch": ["d_v", "d_a", "d_c", "n_iter", "update_components", "d_scratch", "stream"],
        "nmf_scratch_bytes": ["d_v", "d_a", "d_c", "n_iter", "update_components"],
        "nmf_plan": ["n_frames", "n_bins", "n_components", "problems", "update_components"],
        "decompose": ["S", "n_components", "n_iter", "components", "activations", "fit", "sort", "seed"],
    }
    for name, params in want.items():
        assert callable(getattr(jsg, name)) and name in jsg.__all__
        assert list(inspect.signature(getattr(jsg, name)).parameters) == params, name
    assert [p.default for p in inspect.signature(jsg.decompose).parameters.values()][1:] == [None, 200, None, None, True, False, 0]
    assert [p.default for p in inspect.signature(jsg.nmf_plan).parameters.values()][3:] == [1, True]
    launch_params = inspect.signature(jsg.nmf_launch).parameters
    assert launch_params["n_iter"].default is inspect.Parameter.empty and launch_params["n_iter"].kind is inspect.Parameter.KEYWORD_ONLY
    assert launch_params["update_components"].default is True
    symbols = {"jsgx_nmf_launch", "jsgx_nmf_plan", "jsgx_nmf_scratch_bytes"}
    assert symbols <= set(jsg.capix.SIGNATURES)
    assert shutil.which("nm"), "nm (binutils) lists the exported symbols"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", jsg.capix.LIB_PATH], text=True)
    assert symbols <= {line.split()[-1] for line in exported.splitlines() if " T " in line}


def test_kernel_notes(capix, tmp_path):
    """The new object: its twenty-one kernels (those that hold accumulators come once per count of component tiles), no private segment
    (no scratch memory, no spills), the LDS the header states (one panel for the Gram kernel, none for the sum) and 256 lanes a workgroup."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    obj = os.path.join(ROOT, "jadespectrogram_amd", "build", "jsgx_nmf.o")
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
        assert int(g("vgpr_count")) <= 256, name           # a wavefront of each of two workgroups on a SIMD keeps its registers (512 a lane)
    two, one, none = ((0, lds, 0, 0, capix.NMF_THREADS) for lds in (capix.NMF_LDS_BYTES, capix.NMF_LDS_BYTES // 2, 0))
    want = {"nmf_chunk_sum_kernel": none}
    for tiles in (1, 2, 3, 4):
        want.update({f"nmf_gram_kernel<true, {tiles}>": one, f"nmf_gram_kernel<false, {tiles}>": one})
        want.update({f"nmf_update_a_kernel<{tiles}>": two, f"nmf_partial_c_kernel<{tiles}>": two, f"nmf_update_c_kernel<{tiles}>": two})
    assert found == want


def test_host_entry_points_under_asan_ubsan(capix):
    """tests/cpp/jsgx_nmf_host_test.cpp (its own main: the refusals in their order, the plan and the scratch over shapes up to the limits)
    built together with the host units it calls under the address and undefined-behaviour sanitizers and run as a child process; the same
    program against the shipped library, there with the refusals of the launch, gives the same verdict."""
    d = tempfile.gettempdir()
    drv = os.path.join(ROOT, "tests", "cpp", "jsgx_nmf_host_test.cpp")
    hosts = [os.path.join(ROOT, "jadespectrogram_amd", "csrc", f) for f in ("jsgx_beat_host.cpp", "jsgx_nmf_host.cpp")]
    common = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]
    san = os.path.join(d, "jsgx_nmf_host_san")
    subprocess.check_call(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"] + hosts + [drv, "-o", san])
    libdir = os.path.dirname(capix.LIB_PATH)
    shipped = os.path.join(d, "jsgx_nmf_host_lib")
    subprocess.check_call(common + ["-DJSGX_NMF_TEST_LAUNCHES", drv, "-o", shipped, "-L", libdir, "-ljsgx", f"-Wl,-rpath,{libdir}"])
    for exe in (san, shipped):
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == "ok" and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr

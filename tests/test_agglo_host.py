"""Section 17 of the companion library, host side (include/jsgx.h): every refusal of the agglomerative segmentation in its stated order
(all decided without a device), what passes up to the limits, the plan and the scratch size, the stretch lengths of the GPU test against
the header's threshold, the struct layout against a C program, the header's constants, the exported symbols, the Python names, the
kernels' notes, and the host entry points from a stand-alone C++ program under the address and undefined-behaviour sanitizers.  CPU
only."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import agglo_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, F, M, S, OUT = 1000, 65, 40, 41, 90
# never dereferenced: every call below is refused or planned
X, BOUNDS, N_BOUNDS, SEGMENTS, N_SEGMENTS, OUT_BOUNDS, N_OUT, ORDER, HEIGHT, SCRATCH = (i << 44 for i in range(1, 11))
BAD = -2
X_PAIR = N * (F + 3) + 7
X_SPAN, OUT_SPAN, B_SPAN, SEG_SPAN, TREE_SPAN = 2 * X_PAIR + (N - 1) * (F + 3) + F, 2 * (OUT + 1) + OUT, 2 * (M + 2) + M, 2 * (S + 3) + S + 1, 2 * (N + 5) + N
NEED = 4 * 3 * (N * F + N + (N + 63) // 64 + S + 1)


@pytest.fixture(scope="module")
def capix(jsg):
    if not os.path.exists(jsg.capix.LIB_PATH):
        from jadespectrogram_amd import _build
        _build.build_lib()
    jsg.capix.lib()
    return jsg.capix


def args(capix, **kw):       # 3 planes of 1000 frames of 65 features, 40 boundaries and the two ends, 90 results taken, the tree
    a = dict(x=X, x_frame_pitch=F + 3, x_pair_pitch=X_PAIR, bounds=BOUNDS, bounds_pitch=M + 2, n_bounds=N_BOUNDS, segments=SEGMENTS, segments_pitch=S + 3,
             n_segments=N_SEGMENTS, out_bounds=OUT_BOUNDS, out_pitch=OUT + 1, n_out=N_OUT, order=ORDER, height=HEIGHT, tree_pitch=N + 5, pairs=3, n_frames=N,
             n_features=F, max_bounds=M, bounds_all=0, max_segments=S, max_out=OUT, n_clusters=4, pad=1)
    a.update(kw)
    return capix.AgglomerativeArgs(**a)


# in the order of the header: a call with two defects is refused for the earlier one
REFUSED = [
    ("null x", dict(x=None), "null x"),
    ("null segments", dict(segments=None), "null segments"),
    ("null n_segments", dict(n_segments=None), "null n_segments"),
    ("null out_bounds", dict(out_bounds=None), "null out_bounds"),
    ("null n_out", dict(n_out=None), "null n_out"),
    ("null bounds", dict(bounds=None, max_bounds=M), "null bounds with max_bounds > 0"),
    ("order alone", dict(height=None), "order and height go together"),
    ("height alone", dict(order=None), "order and height go together"),
    ("misaligned x", dict(x=X + 2), "pointers must be 4-byte aligned"),
    ("misaligned n_bounds", dict(n_bounds=N_BOUNDS + 1), "pointers must be 4-byte aligned"),
    ("misaligned out_bounds", dict(out_bounds=OUT_BOUNDS + 3), "pointers must be 4-byte aligned"),
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
    ("no max_out", dict(max_out=0), "max_out must be in 1..16777216"),
    ("max_out", dict(max_out=(1 << 24) + 1), "max_out must be in 1..16777216"),
    ("no clusters", dict(n_clusters=0), "n_clusters must be at least 1"),
    ("negative clusters", dict(n_clusters=-3), "n_clusters must be at least 1"),
    ("pad", dict(pad=2), "pad must be 0 or 1"),
    ("reserved0", dict(reserved0=1), "reserved0 must be 0"),
    ("few segments", dict(max_segments=S - 1), "max_segments smaller than the stretches the list can give"),
    ("x_frame_pitch", dict(x_frame_pitch=F - 1), "x_frame_pitch smaller than n_features"),
    ("x_pair_pitch", dict(x_pair_pitch=X_PAIR - 11), "x_pair_pitch does not cover a plane"),
    ("bounds_pitch", dict(bounds_pitch=M - 1), "bounds_pitch neither 0 nor >= max_bounds"),
    ("segments_pitch", dict(segments_pitch=S), "segments_pitch smaller than max_segments + 1"),
    ("out_pitch", dict(out_pitch=OUT - 1), "out_pitch smaller than max_out"),
    ("tree_pitch", dict(tree_pitch=N - 1), "tree_pitch smaller than n_frames"),
    ("out_bounds ends in x", dict(out_bounds=X - 4 * OUT_SPAN + 4), "out_bounds overlaps x"),
    ("out_bounds inside bounds", dict(out_bounds=BOUNDS + 4 * (B_SPAN - 1)), "out_bounds overlaps bounds"),
    ("out_bounds ends in n_bounds", dict(out_bounds=N_BOUNDS - 4 * OUT_SPAN + 4 * 3), "out_bounds overlaps n_bounds"),
    ("n_out inside x", dict(n_out=X + 4 * 1000), "n_out overlaps x"),
    ("n_out is n_bounds", dict(n_out=N_BOUNDS), "n_out overlaps n_bounds"),
    ("segments inside x", dict(segments=X + 4 * (X_SPAN - 1)), "segments overlaps x"),
    ("segments ends in bounds", dict(segments=BOUNDS - 4 * SEG_SPAN + 4), "segments overlaps bounds"),
    ("n_segments ends in bounds", dict(n_segments=BOUNDS - 8), "n_segments overlaps bounds"),
    ("order ends in x", dict(order=X - 4 * TREE_SPAN + 4), "order overlaps x"),
    ("height inside n_bounds", dict(height=N_BOUNDS + 8), "height overlaps n_bounds"),
    ("n_out inside out_bounds", dict(n_out=OUT_BOUNDS + 4 * (OUT_SPAN - 1)), "out_bounds overlaps n_out"),
    ("segments inside out_bounds", dict(segments=OUT_BOUNDS + 4 * 7), "out_bounds overlaps segments"),
    ("height ends in out_bounds", dict(height=OUT_BOUNDS - 4 * TREE_SPAN + 4), "out_bounds overlaps height"),
    ("n_segments inside n_out", dict(n_segments=N_OUT + 8), "n_out overlaps n_segments"),
    ("n_segments inside segments", dict(n_segments=SEGMENTS + 4 * (SEG_SPAN - 1)), "segments overlaps n_segments"),
    ("order ends in segments", dict(order=SEGMENTS - 4 * TREE_SPAN + 4), "segments overlaps order"),
    ("height behind n_segments", dict(height=N_SEGMENTS + 4), "n_segments overlaps height"),
    ("height inside order", dict(height=ORDER + 4 * (TREE_SPAN - 1)), "order overlaps height"),
]
# the scratch, behind all of those: (scratch, scratch_bytes)
SCRATCH_REFUSED = [
    ("null scratch", (None, NEED), "null scratch"),
    ("misaligned scratch", (SCRATCH + 2, NEED), "scratch must be 4-byte aligned"),
    ("small scratch", (SCRATCH, NEED - 1), "scratch smaller than jsgx_agglomerative_scratch_bytes"),
    ("scratch inside x", (X + 4 * (X_SPAN - 1), NEED), "scratch overlaps x"),
    ("scratch ends in bounds", (BOUNDS - NEED + 4, NEED), "scratch overlaps bounds"),
    ("scratch ends in n_bounds", (N_BOUNDS - NEED + 12, NEED), "scratch overlaps n_bounds"),
    ("scratch inside out_bounds", (OUT_BOUNDS + 8, NEED), "scratch overlaps out_bounds"),
    ("scratch inside n_out", (N_OUT + 8, NEED), "scratch overlaps n_out"),
    ("scratch ends in segments", (SEGMENTS - NEED + 4, NEED), "scratch overlaps segments"),
    ("scratch is n_segments", (N_SEGMENTS, NEED), "scratch overlaps n_segments"),
    ("scratch ends in order", (ORDER - NEED + 4, NEED), "scratch overlaps order"),
    ("scratch inside height", (HEIGHT + 4 * (TREE_SPAN - 1), NEED), "scratch overlaps height"),
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
    in_order(lib, REFUSED, lambda change: lib.jsgx_agglomerative_launch(C.byref(args(capix, **change)), SCRATCH, NEED, None), "jsgx_agglomerative_launch", i)
    in_order(lib, REFUSED, lambda change: lib.jsgx_agglomerative_plan(C.byref(args(capix, **change)), None, 0, None, None, None), "jsgx_agglomerative_plan", i)
    in_order(lib, REFUSED, lambda change: lib.jsgx_agglomerative_scratch_bytes(C.byref(args(capix, **change))), "jsgx_agglomerative_scratch_bytes", i)
    # ... and every one of them comes before the scratch is looked at
    _, change, message = REFUSED[i]
    assert lib.jsgx_agglomerative_launch(C.byref(args(capix, **change)), None, 0, None) == BAD and lib.jsgx_last_error() == f"jsgx_agglomerative_launch: {message}".encode()


@pytest.mark.parametrize("i", range(len(SCRATCH_REFUSED)), ids=[r[0] for r in SCRATCH_REFUSED])
def test_scratch_refusals_in_their_order(capix, i):
    lib = capix.lib()
    _, (scratch, size), message = SCRATCH_REFUSED[i]
    assert lib.jsgx_agglomerative_launch(C.byref(args(capix)), scratch, size, None) == BAD
    assert lib.jsgx_last_error() == f"jsgx_agglomerative_launch: {message}".encode(), lib.jsgx_last_error()
    if i >= 3:          # a larger scratch is looked at for the bytes of the stated size only
        assert lib.jsgx_agglomerative_launch(C.byref(args(capix)), scratch, size + (1 << 40), None) == BAD and lib.jsgx_last_error().endswith(message.encode())


def test_the_long_plane_without_boundaries(capix):
    lib = capix.lib()
    long = dict(n_frames=ar.MAX_STRETCH + 1, x_pair_pitch=(ar.MAX_STRETCH + 1) * (F + 3), tree_pitch=ar.MAX_STRETCH + 1)
    plan = lambda **kw: lib.jsgx_agglomerative_plan(C.byref(args(capix, **dict(long, **kw))), None, 0, None, None, None)
    assert plan() == 0 and plan(bounds=None, n_bounds=None, max_bounds=0) == BAD
    assert lib.jsgx_last_error() == b"jsgx_agglomerative_plan: n_frames above 16384 without boundaries"
    assert plan(n_bounds=None, bounds_all=0) == BAD and plan(n_bounds=None, bounds_all=1) == 0 and plan(n_bounds=None, bounds_all=0, pad=0) == 0
    assert plan(n_bounds=None, bounds_all=0, max_segments=0) == BAD and lib.jsgx_last_error().endswith(b"max_segments must be in 1..1048577")          # the earlier one
    assert plan(n_bounds=None, bounds_all=0, x_frame_pitch=1) == BAD and lib.jsgx_last_error().endswith(b"n_frames above 16384 without boundaries")
    assert plan(n_bounds=None, bounds_all=0, n_frames=ar.MAX_STRETCH) == 0


def test_what_passes(capix):
    lib = capix.lib()
    ok = lambda **kw: lib.jsgx_agglomerative_plan(C.byref(args(capix, **kw)), None, 0, None, None, None)
    assert ok() == 0
    # a buffer next to another, not inside it
    assert ok(out_bounds=X - 4 * OUT_SPAN) == 0 and ok(out_bounds=X + 4 * X_SPAN) == 0 and ok(segments=BOUNDS + 4 * B_SPAN) == 0 and ok(n_segments=SEGMENTS + 4 * SEG_SPAN) == 0
    assert ok(n_out=N_BOUNDS + 12) == 0 and ok(n_out=N_BOUNDS - 12) == 0 and ok(height=ORDER + 4 * TREE_SPAN) == 0 and ok(order=X - 4 * TREE_SPAN) == 0
    # no tree; no boundaries at all; one list for every pair; the count on the host; bounds_all not looked at with n_bounds
    assert ok(order=None, height=None, tree_pitch=0) == 0 and ok(bounds=None, n_bounds=None, max_bounds=0) == 0 and ok(bounds_pitch=0) == 0
    assert ok(n_bounds=None, bounds_all=M) == 0 and ok(n_bounds=None, bounds_all=0, max_segments=1, segments_pitch=2) == 0 and ok(bounds_all=-5) == 0
    assert ok(n_bounds=None, bounds_all=3, max_segments=4) == 0 and ok(pad=0, max_segments=M - 1) == 0 and ok(pad=0, max_segments=M - 2) == BAD
    # one pair: no pair pitch is looked at; the ends of the ranges
    assert ok(pairs=1, x_pair_pitch=0, out_pitch=0, bounds_pitch=0, segments_pitch=0, tree_pitch=0) == 0
    assert ok(n_clusters=(1 << 31) - 1, max_out=1, out_pitch=1) == 0 and ok(max_out=1 << 24, out_pitch=1 << 24, out_bounds=1 << 58) == 0
    assert ok(max_bounds=1 << 20, bounds_pitch=1 << 20, max_segments=(1 << 20) + 1, segments_pitch=(1 << 20) + 2, segments=1 << 59) == 0
    for call in (lib.jsgx_agglomerative_launch(None, None, 0, None), lib.jsgx_agglomerative_plan(None, None, 0, None, None, None), lib.jsgx_agglomerative_scratch_bytes(None)):
        assert call == BAD and lib.jsgx_last_error().endswith(b": null argument")
    assert lib.jsgx_agglomerative_plan(C.byref(args(capix)), C.create_string_buffer(15), 15, None, None, None) == BAD
    assert lib.jsgx_last_error() == b"jsgx_agglomerative_plan: bad argument"
    assert lib.jsgx_agglomerative_scratch_bytes(C.byref(args(capix))) == NEED
    import torch
    if torch.cuda.is_available():           # with a device the calls below would launch on pointers that are no memory
        return
    NO_DEVICE = capix.JSGX_ERR_NO_DEVICE
    launch = lambda scratch=SCRATCH, size=NEED, **kw: lib.jsgx_agglomerative_launch(C.byref(args(capix, **kw)), scratch, size, None)
    assert launch() == NO_DEVICE and lib.jsgx_last_error() == b"jsgx_agglomerative_launch: no HIP device"
    assert launch(size=NEED + 4096) == NO_DEVICE and launch(scratch=X + 4 * X_SPAN) == NO_DEVICE and launch(scratch=X - NEED) == NO_DEVICE
    assert launch(bounds=None, n_bounds=None, max_bounds=0, pad=0) == NO_DEVICE


def test_the_plan_and_the_constants(jsg, capix):
    for frames in (1, 64, 65, 1025, 16384, 16385, 1 << 24):
        for feats in (1, 65, 65536):
            for P in (1, 3, 65535):
                for bounds in (0, 1, 700, 1 << 20):
                    for pad in (False, True):
                        if bounds == 0 and pad and frames > capix.AGGLO_MAX_STRETCH:
                            with pytest.raises(jsg.JsgError, match="n_frames above 16384 without boundaries"):
                                jsg.agglomerative_plan(frames, feats, P, bounds, pad)
                            continue
                        none = bounds + 2 * pad < 2
                        L = min(frames, capix.AGGLO_MAX_STRETCH)
                        want = ("agglo_wave", capix.AGGLO_THREADS, capix.AGGLO_LDS_BYTES, 2 if none else 4) if frames <= capix.AGGLO_SHORT else \
                            ("agglo_group", capix.AGGLO_GROUP_THREADS, 8 * L + 8 * ((L + 63) // 64), 2 if none else 5)
                        assert jsg.agglomerative_plan(frames, feats, P, bounds, pad) == want
    hdr = open(os.path.join(ROOT, "include", "jsgx.h")).read()
    for name, value in (("JSGX_AGGLO_MAX_STRETCH", capix.AGGLO_MAX_STRETCH), ("JSGX_AGGLO_SHORT", capix.AGGLO_SHORT), ("JSGX_AGGLO_THREADS", capix.AGGLO_THREADS),
                        ("JSGX_AGGLO_GROUP_THREADS", capix.AGGLO_GROUP_THREADS), ("JSGX_AGGLO_COPY_FRAMES", capix.AGGLO_COPY_FRAMES), ("JSGX_AGGLO_MAX_OUT", capix.AGGLO_MAX_OUT),
                        ("JSGX_AGGLO_LDS_BYTES", capix.AGGLO_LDS_BYTES), ("JSGX_AGGLO_LDS_LIMIT", capix.AGGLO_LDS_LIMIT), ("JSGX_ABI_VERSION", 1)):
        assert re.search(rf"#define {name} {value}\b", hdr), name
    assert (capix.AGGLO_MAX_STRETCH, capix.AGGLO_SHORT, capix.AGGLO_COPY_FRAMES) == (ar.MAX_STRETCH, ar.SHORT, ar.COPY_FRAMES) == (16384, 64, 64)
    assert capix.AGGLO_LDS_LIMIT == 8 * capix.AGGLO_MAX_STRETCH + 8 * (capix.AGGLO_MAX_STRETCH // 64) <= 163840 and capix.AGGLO_LDS_BYTES == 4 * 8 * capix.AGGLO_SHORT
    assert capix.AGGLO_MAX_STRETCH <= 65535          # the links are 16 bits
    for kernel in ("agglo_segments", "agglo_copy", "agglo_offsets", "agglo_wave", "agglo_group"):
        assert f'"{kernel}"' in hdr
    assert "Section 17 was added to version 1" in hdr and "160 bytes" in hdr
    assert capix.lib().jsgx_abi_version() == 1


def test_the_gpu_lengths_straddle_the_threshold(capix):
    """The kernel that serves a stretch depends on its length alone: the length at which "agglo_group" takes over is in the GPU test's list
    with its successor, next to each other inside one workgroup of four stretches, and so are the lengths the contract names."""
    assert set(ar.THRESHOLDS) == {capix.AGGLO_SHORT}
    for t in ar.THRESHOLDS:
        assert {t, t + 1} <= set(ar.LENGTHS) and {t, t + 1} <= set(ar.N_SET)
    groups = [set(ar.LENGTHS[i:i + 4]) for i in range(0, len(ar.LENGTHS), 4)]
    assert any(min(g) <= capix.AGGLO_SHORT < max(g) for g in groups) and any(max(g) <= capix.AGGLO_SHORT for g in groups)
    assert set(ar.N_SET) == {1, 2, 3, 63, 64, 65, 257, 1025} and set(ar.F_SET) == {1, 63, 64, 65, 130} and set(ar.PAIRS_SET) == {1, 3}
    assert max(ar.LENGTHS) > 4 * capix.AGGLO_SHORT          # more than four blocks of minima


def test_struct_layout_matches_the_header(capix, tmp_path):
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsgx.h")).read(), flags=re.S)
    struct, ctype, size = "jsgx_agglomerative_args", capix.AgglomerativeArgs, 160
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
    launch = ["d_x", "d_bounds", "d_n_bounds", "d_segments", "d_n_segments", "d_out_bounds", "d_n_out", "n_clusters", "pad", "bounds_all", "d_order", "d_height"]
    want = {
        "agglomerative_launch": launch + ["d_scratch", "stream"],
        "agglomerative_scratch_bytes": launch,
        "agglomerative_plan": ["n_frames", "n_features", "pairs", "max_bounds", "pad"],
        "agglomerative": ["data", "k", "return_tree"],
        "subsegment": ["data", "frames", "n_segments", "pad", "n_frames", "max_bounds"],
    }
    for name, params in want.items():
        assert callable(getattr(jsg, name)) and name in jsg.__all__
        assert list(inspect.signature(getattr(jsg, name)).parameters) == params, name
    assert [p.default for p in inspect.signature(jsg.agglomerative).parameters.values()][2:] == [False]
    assert [p.default for p in inspect.signature(jsg.subsegment).parameters.values()][2:] == [4, True, None, None]
    for fn in (jsg.agglomerative, jsg.subsegment):          # the deliberate differences are stated, and that librosa itself was not run
        doc = " ".join(fn.__doc__.split())
        assert "frame-major" in doc and "float32" in doc and "Agreement with librosa itself was not measured" in doc
        assert "lower frame" in doc and "sklearn's heap order decides" in doc
    doc = " ".join(jsg.subsegment.__doc__.split())
    assert "clipped" in doc and "non-decreasing" in doc and "librosa sorts" in doc and "it is not the number of frames of the plane" in doc
    with pytest.raises(jsg.JsgError, match="subsegment: frames must be non-decreasing"):          # the caller's own name in the text
        jsg.spectrogram._host_segments([5, 3], 10, True, "subsegment", "frames")
    with pytest.raises(jsg.JsgError, match="sync: idx must be non-decreasing"):
        jsg.spectrogram._host_segments([5, 3], 10, True)
    symbols = {"jsgx_agglomerative_launch", "jsgx_agglomerative_scratch_bytes", "jsgx_agglomerative_plan"}
    assert symbols <= set(jsg.capix.SIGNATURES)
    assert shutil.which("nm"), "nm (binutils) lists the exported symbols"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", jsg.capix.LIB_PATH], text=True)
    functions = {line.split()[-1] for line in exported.splitlines() if " T " in line}
    assert symbols <= functions and functions == set(jsg.capix.SIGNATURES)


def test_kernel_notes(capix, tmp_path):
    """The new object: its five kernels, no private segment (no scratch memory, no spills), the static LDS the header states (the keys and
    links of "agglo_group" are dynamic and not in the notes), the workgroups the header states, at most 128 VGPRs."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    obj = os.path.join(ROOT, "jadespectrogram_amd", "build", "jsgx_agglo.o")
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
    T = capix.AGGLO_THREADS
    assert found == {"agglo_segments_kernel": (0, 48, 0, 0, T), "agglo_copy_kernel": (0, 16, 0, 0, T), "agglo_offsets_kernel": (0, 48, 0, 0, T),
                     "agglo_wave_kernel": (0, capix.AGGLO_LDS_BYTES, 0, 0, T), "agglo_group_kernel": (0, 0, 0, 0, capix.AGGLO_GROUP_THREADS)}
    with open(os.path.join(ROOT, "tools", "kernel_regs.py")) as f:
        text = f.read()
    assert all(k in text for k in (*found, "jsgx_agglo.o"))


def test_one_copy_of_the_segment_rule():
    """Section 15's rule lives in one header that both units include."""
    csrc = os.path.join(ROOT, "jadespectrogram_amd", "csrc")
    texts = {f: open(os.path.join(csrc, f)).read() for f in ("jsgx_segments.h", "jsgx_sync.hip", "jsgx_agglo.hip")}
    assert "segments_of_pair(const SegmentsK& g" in texts["jsgx_segments.h"] and "unsigned key_of(float v)" in texts["jsgx_segments.h"]
    for unit in ("jsgx_sync.hip", "jsgx_agglo.hip"):
        assert '#include "jsgx_segments.h"' in texts[unit] and "segments_of_pair(" in texts[unit] and "key_of(float" not in texts[unit] and "entry(i - 1)" not in texts[unit]


def test_host_entry_points_under_asan_ubsan(capix):
    """tests/cpp/jsgx_agglo_host_test.cpp (its own main: the refusals in their order, the plan and the scratch size over shapes up to the
    limits, planes more than 2^31 elements apart) built together with the host units it calls under the address and undefined-behaviour
    sanitizers and run as a child process; the same program against the shipped library, there with the refusals of the launch and of
    its scratch, gives the same verdict."""
    d = tempfile.gettempdir()
    drv = os.path.join(ROOT, "tests", "cpp", "jsgx_agglo_host_test.cpp")
    hosts = [os.path.join(ROOT, "jadespectrogram_amd", "csrc", f) for f in ("jsgx_beat_host.cpp", "jsgx_agglo_host.cpp")]
    common = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]
    san = os.path.join(d, "jsgx_agglo_host_san")
    subprocess.check_call(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"] + hosts + [drv, "-o", san])
    libdir = os.path.dirname(capix.LIB_PATH)
    shipped = os.path.join(d, "jsgx_agglo_host_lib")
    subprocess.check_call(common + ["-DJSGX_AGGLO_TEST_LAUNCHES", drv, "-o", shipped, "-L", libdir, "-ljsgx", f"-Wl,-rpath,{libdir}"])
    for exe in (san, shipped):
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == "ok" and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr

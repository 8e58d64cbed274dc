"""Section 4 of the companion library, host side (include/jsgx.h): every refusal of the Viterbi decoder in its stated order (all decided
without a device), the scratch formula, the plans over shapes, the struct layout against a C program, the band transition builder against
numpy, the Python names, the kernels' notes, and the host entry points from a stand-alone C++ program under the address and
undefined-behaviour sanitizers.  CPU only."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# never dereferenced: every call below is refused, sized or planned
EMIT, INIT, TRANS, STATES, LOGP, VALUE, SCRATCH = (i << 44 for i in range(1, 8))
BAD = -2
FORMS = ("viterbi_dense_lds", "viterbi_dense_mem", "viterbi_band_lds", "viterbi_band_mem")


@pytest.fixture(scope="module")
def capix(jsg):
    if not os.path.exists(jsg.capix.LIB_PATH):
        from jadespectrogram_amd import _build
        _build.build_lib()
    jsg.capix.lib()
    return jsg.capix


def args(capix, **kw):
    a = dict(log_emit=EMIT, emit_frame_pitch=24, emit_seq_pitch=2400, log_init=INIT, trans=TRANS, trans_pitch=20, trans_form=0, band_half=0, seqs=3, n_states=20,
             n_frames=100, reserved0=0, states=STATES, states_pitch=100, logp=LOGP, value=VALUE, value_frame_pitch=20, value_seq_pitch=2000)
    a.update(kw)
    return capix.ViterbiArgs(**a)


def scratch_formula(capix, seqs, S, T):
    blocks = -(-T // capix.VITERBI_BLOCK)
    return -(-(4 * seqs * S + 4 * seqs * blocks + 2 * seqs * T * S + 2 * seqs * blocks * S) // 4) * 4


# in the order of the header: a call with two defects is refused for the earlier one
REFUSED = [
    ("null log_emit", dict(log_emit=None), "null log_emit"),
    ("null log_init", dict(log_init=None), "null log_init"),
    ("null trans", dict(trans=None), "null trans"),
    ("null states", dict(states=None), "null states"),
    ("misaligned log_emit", dict(log_emit=EMIT + 2), "pointers must be 4-byte aligned"),
    ("misaligned logp", dict(logp=LOGP + 1), "pointers must be 4-byte aligned"),
    ("misaligned value", dict(value=VALUE + 3), "pointers must be 4-byte aligned"),
    ("no seqs", dict(seqs=0), "seqs must be in 1..65535"),
    ("65536 seqs", dict(seqs=65536), "seqs must be in 1..65535"),
    ("no states", dict(n_states=0), "n_states must be in 1..2048"),
    ("2049 states", dict(n_states=2049, emit_frame_pitch=2049, trans_pitch=2049, value_frame_pitch=2049, emit_seq_pitch=204900, value_seq_pitch=204900), "n_states must be in 1..2048"),
    ("no frames", dict(n_frames=0), "n_frames must be in 1..2^20"),
    ("2^20 + 1 frames", dict(n_frames=(1 << 20) + 1, states_pitch=1 << 21, emit_seq_pitch=1 << 26, value_seq_pitch=1 << 26), "n_frames must be in 1..2^20"),
    ("trans_form 2", dict(trans_form=2), "trans_form must be 0 (dense) or 1 (band)"),
    ("trans_form -1", dict(trans_form=-1), "trans_form must be 0 (dense) or 1 (band)"),
    ("band_half with dense", dict(band_half=3), "band_half must be 0 with the dense form"),
    ("band_half 65", dict(trans_form=1, band_half=65), "band_half must be in 0..64"),
    ("band_half -1", dict(trans_form=1, band_half=-1), "band_half must be in 0..64"),
    ("reserved0", dict(reserved0=1), "reserved0 must be 0"),
    ("emit_frame_pitch", dict(emit_frame_pitch=19), "emit_frame_pitch smaller than n_states"),
    ("emit_seq_pitch", dict(emit_seq_pitch=99 * 24 + 19), "emit_seq_pitch does not cover a sequence"),
    ("trans_pitch", dict(trans_pitch=19), "trans_pitch smaller than n_states"),
    ("states_pitch", dict(states_pitch=99), "states_pitch smaller than n_frames"),
    ("value_frame_pitch", dict(value_frame_pitch=19), "value_frame_pitch smaller than n_states"),
    ("value_seq_pitch", dict(value_seq_pitch=1999), "value_seq_pitch does not cover a sequence"),
    ("states ends in log_emit", dict(states=EMIT - 4 * 300 + 4), "an output overlaps log_emit"),
    ("value inside log_emit", dict(value=EMIT + 4 * 1000), "an output overlaps log_emit"),
    ("logp inside log_init", dict(logp=INIT + 4 * 19), "an output overlaps log_init"),
    ("states inside trans", dict(states=TRANS + 4 * 399), "an output overlaps trans"),
    ("logp inside states", dict(logp=STATES + 4 * 299), "an output overlaps another output"),
    ("value ends in logp", dict(value=LOGP - 4 * 6000 + 4), "an output overlaps another output"),
]
CALLS = (("jsgx_viterbi_launch", lambda lib, a: lib.jsgx_viterbi_launch(C.byref(a), SCRATCH, 1 << 40, None)),
         ("jsgx_viterbi_scratch_bytes", lambda lib, a: lib.jsgx_viterbi_scratch_bytes(C.byref(a))),
         ("jsgx_viterbi_plan", lambda lib, a: lib.jsgx_viterbi_plan(C.byref(a), None, 0, None, None, None)))


@pytest.mark.parametrize("i", range(len(REFUSED)), ids=[r[0] for r in REFUSED])
def test_refusals_in_their_order(capix, i):
    lib = capix.lib()
    _, change, message = REFUSED[i]
    a = args(capix, **change)
    for who, call in CALLS:
        assert call(lib, a) == BAD and lib.jsgx_last_error() == f"{who}: {message}".encode()
    # with any later defect on top, the earlier one is still the one reported
    who, call = CALLS[0]
    for _, later, later_message in REFUSED[i + 1:]:
        if later_message == message or set(later) & set(change):
            continue
        assert call(lib, args(capix, **dict(later, **change))) == BAD
        assert lib.jsgx_last_error() == f"{who}: {message}".encode(), (REFUSED[i][0], later)
    # ... also ahead of what only the launch refuses
    assert lib.jsgx_viterbi_launch(C.byref(a), None, 0, None) == BAD and lib.jsgx_last_error() == f"jsgx_viterbi_launch: {message}".encode()


def test_what_only_the_launch_refuses_and_what_passes(capix):
    lib = capix.lib()
    a = args(capix)
    need = scratch_formula(capix, 3, 20, 100)
    for scratch, size, message in ((None, 1 << 40, "null scratch"), (SCRATCH + 2, 1 << 40, "scratch must be 4-byte aligned"),
                                   (SCRATCH, need - 1, "scratch smaller than jsgx_viterbi_scratch_bytes"), (None, 0, "null scratch"),
                                   (SCRATCH + 1, 0, "scratch must be 4-byte aligned")):
        assert lib.jsgx_viterbi_launch(C.byref(a), scratch, size, None) == BAD and lib.jsgx_last_error() == f"jsgx_viterbi_launch: {message}".encode()
    for call in (lib.jsgx_viterbi_launch(None, SCRATCH, 1 << 40, None), lib.jsgx_viterbi_scratch_bytes(None), lib.jsgx_viterbi_plan(None, None, 0, None, None, None)):
        assert call == BAD and lib.jsgx_last_error().endswith(b": null argument")
    assert lib.jsgx_viterbi_plan(C.byref(a), C.create_string_buffer(23), 23, None, None, None) == BAD and lib.jsgx_last_error() == b"jsgx_viterbi_plan: bad argument"
    size = lambda **kw: lib.jsgx_viterbi_scratch_bytes(C.byref(args(capix, **kw)))
    assert size() == need
    # one sequence: the sequence pitches are not looked at; the optional outputs may be missing, and then their pitches are not looked at
    assert size(seqs=1, emit_seq_pitch=0, states_pitch=0, value_seq_pitch=0) == scratch_formula(capix, 1, 20, 100)
    assert size(logp=None) == need and size(value=None, value_frame_pitch=0, value_seq_pitch=0) == need and size(logp=None, value=None) == need
    assert size(trans_form=1, band_half=0) == need and size(trans_form=1, band_half=64) == need
    # an output next to an input or to another output, not inside it
    assert size(states=EMIT - 4 * 300) == need and size(value=EMIT + 4 * (2 * 2400 + 99 * 24 + 20)) == need and size(logp=INIT + 4 * 20) == need
    assert size(states=TRANS + 4 * 400) == need and size(logp=STATES + 4 * 300) == need and size(value=LOGP - 4 * 6000) == need
    # the band table is 2W + 1 rows: what lies behind them is free
    assert size(trans_form=1, band_half=2, states=TRANS + 4 * 100) == need and size(trans_form=1, band_half=2, states=TRANS + 4 * 99) == BAD


def test_no_device_comes_after_the_refusals(capix):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = capix.lib()
    assert lib.jsgx_viterbi_launch(C.byref(args(capix)), SCRATCH, 1 << 40, None) == capix.JSGX_ERR_NO_DEVICE
    assert lib.jsgx_last_error() == b"jsgx_viterbi_launch: no HIP device"
    assert lib.jsgx_viterbi_launch(C.byref(args(capix)), SCRATCH, 16, None) == BAD


def test_plans_and_scratch_over_shapes(jsg, capix):
    B, LIMIT = capix.VITERBI_BLOCK, capix.VITERBI_LDS_LIMIT
    assert B in (64, 256, 1024) and LIMIT == 163840
    threads_of = {1: 64, 2: 128, 3: 192, 63: 1024, 64: 1024, 65: 576, 191: 768, 192: 768, 193: 832, 255: 1024, 256: 1024, 257: 576, 512: 1024, 513: 576, 1023: 1024,
                  1024: 1024, 1025: 1024, 2048: 1024}
    for S, threads in threads_of.items():
        for T in (1, B - 1, B, B + 1, 5 * B + 7, 1 << 20):
            lds = 4 * (S * S + 2 * S) if S <= 192 else 8 * S
            assert jsg.viterbi_plan(S, T) == ("viterbi_dense_lds" if S <= 192 else "viterbi_dense_mem", threads, lds, 3 if T <= B else 4), (S, T)
            assert lds <= LIMIT
            for seqs in (1, 5):
                a = args(capix, seqs=seqs, n_states=S, n_frames=T, emit_frame_pitch=S, emit_seq_pitch=S * T, trans_pitch=S, states_pitch=T, value_frame_pitch=S,
                         value_seq_pitch=S * T)
                assert capix.lib().jsgx_viterbi_scratch_bytes(C.byref(a)) == scratch_formula(capix, seqs, S, T)
    assert jsg.viterbi_plan(192, 10)[2] == 148992
    # band shapes on both sides of the LDS fit, 4 ((2W + 1) S + 2 S) <= 163840
    for S, W, in_lds in ((1, 0, True), (5, 0, True), (5, 4, True), (64, 3, True), (40, 64, True), (300, 25, True), (312, 64, True), (313, 64, False), (1200, 25, False),
                         (2048, 64, False), (2048, 8, True), (2048, 9, False), (772, 25, True), (773, 25, False)):
        lds = 4 * ((2 * W + 1) * S + 2 * S)
        assert (lds <= LIMIT) == in_lds
        name, threads, got, launches = jsg.viterbi_plan(S, B + 1, seqs=2, band_half=W)
        assert (name, got, launches) == (("viterbi_band_lds", lds, 4) if in_lds else ("viterbi_band_mem", 8 * S, 4)) and got <= LIMIT
        assert threads == jsg.viterbi_plan(S, 3)[1]
    with pytest.raises(jsg.JsgError, match="n_states must be in"):
        jsg.viterbi_plan(0, 5)
    with pytest.raises(jsg.JsgError, match="band_half must be in"):
        jsg.viterbi_plan(5, 5, band_half=65)
    hdr = open(os.path.join(ROOT, "include", "jsgx.h")).read()
    for name, value in (("JSGX_TRANS_DENSE", capix.TRANS_DENSE), ("JSGX_TRANS_BAND", capix.TRANS_BAND), ("JSGX_VITERBI_MAX_STATES", capix.VITERBI_MAX_STATES),
                        ("JSGX_VITERBI_MAX_FRAMES", capix.VITERBI_MAX_FRAMES), ("JSGX_VITERBI_MAX_BAND_HALF", capix.VITERBI_MAX_BAND_HALF),
                        ("JSGX_VITERBI_LDS_STATES", capix.VITERBI_LDS_STATES), ("JSGX_VITERBI_THREADS", capix.VITERBI_THREADS),
                        ("JSGX_VITERBI_LDS_LIMIT", capix.VITERBI_LDS_LIMIT), ("JSGX_VITERBI_BLOCK", capix.VITERBI_BLOCK), ("JSGX_ABI_VERSION", 1)):
        assert re.search(rf"#define {name} {value}\b", hdr), name
    for form in FORMS + ("viterbi_jump", "viterbi_ends", "viterbi_trace"):
        assert f'"{form}"' in hdr


def test_struct_layout_matches_the_header(capix, tmp_path):
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler")
    struct = "jsgx_viterbi_args"
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsgx.h")).read(), flags=re.S)
    body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", hdr, flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*(\[\d+\])?\s*$", decl).group(1) for decl in body.split(";") if decl.strip()]
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "jsgx.h"', "int main(void) {", f'    printf("%zu\\n", sizeof({struct}));']
    lines += [f'    printf("{f} %zu %zu\\n", offsetof({struct}, {f}), sizeof((({struct}*)0)->{f}));' for f in names]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)])
    out = subprocess.check_output([str(tmp_path / "layout")], text=True).split("\n")
    ctype = capix.ViterbiArgs
    assert out[0] == str(C.sizeof(ctype)) == "120"
    assert [f for f, _ in ctype._fields_] == names
    offset = 0
    for (f, _), line in zip(ctype._fields_, out[1:]):
        assert line == f"{f} {getattr(ctype, f).offset} {getattr(ctype, f).size}"
        assert getattr(ctype, f).offset == offset, f"padding in front of {f}"
        offset += getattr(ctype, f).size


def band_numpy(S, window):
    """The band transition as include/jsgx.h states it, in numpy: (table [2W+1][S], the probabilities of every source's row)."""
    w = np.asarray(window, np.float64)
    W = w.size // 2
    out = np.full((2 * W + 1, S), -np.inf, np.float32)
    rows = []
    for i in range(S):
        js = np.arange(max(0, i - W), min(S - 1, i + W) + 1)
        total = 0.0
        for j in js:
            total += w[j - i + W]
        with np.errstate(divide="ignore"):
            out[i - js + W, js] = np.log(w[js - i + W] / total).astype(np.float32)
        rows.append(out[i - js + W, js])
    return out, rows


def test_band_builder(jsg, capix):
    rng = np.random.default_rng(5)
    u = 2.0 ** -24
    for S, W in ((1, 0), (1, 3), (5, 0), (5, 4), (40, 64), (300, 25), (2048, 64)):
        window = rng.random(2 * W + 1) + 0.01
        if W >= 3:
            window[[0, W + 2]] = 0.0
        got = jsg.viterbi_band_transition(S, window)
        want, rows = band_numpy(S, window)
        assert got.dtype == np.float32 and got.shape == (2 * W + 1, S) and (got.view(np.uint32) == want.view(np.uint32)).all()
        for i, row in enumerate(rows):
            assert abs(np.exp(row.astype(np.float64)).sum() - 1.0) <= 4 * u, (S, W, i)
        src = np.arange(2 * W + 1)[:, None] - W + np.arange(S)[None, :]
        assert (got[(src < 0) | (src >= S)] == -np.inf).all() and (got[(src >= 0) & (src < S)] <= 0).all()
    # a triangular window is what librosa.sequence.transition_local builds from
    tri = jsg.viterbi_band_transition(6, [1, 2, 1])
    assert tri[1, 0] == np.float32(np.log(2 / 3)) and tri[1, 3] == np.float32(np.log(0.5)) and tri[0, 0] == -np.inf and tri[2, 5] == -np.inf
    # the pitch and the refusals, through the C entry point
    lib = capix.lib()
    out = np.full((3, 9), 777, np.float32)
    w = np.array([1.0, 2.0, 1.0])
    assert lib.jsgx_viterbi_band_build(6, 1, w.ctypes.data, out.ctypes.data, 9) == 0 and (out[:, :6] == tri).all() and (out[:, 6:] == 777).all()
    build = lambda S, W, win, o, pitch: lib.jsgx_viterbi_band_build(S, W, None if win is None else win.ctypes.data, None if o is None else o.ctypes.data, pitch)
    for call, message in ((lambda: build(6, 1, None, out, 9), "null window"), (lambda: build(6, 1, w, None, 9), "null out"),
                          (lambda: build(0, 1, w, out, 9), "n_states must be in 1..2048"), (lambda: build(2049, 1, w, out, 4096), "n_states must be in 1..2048"),
                          (lambda: build(6, -1, w, out, 9), "band_half must be in 0..64"), (lambda: build(6, 65, w, out, 9), "band_half must be in 0..64"),
                          (lambda: build(6, 1, np.array([1.0, 2.0, -1e-9]), out, 9), "window entries must be finite and >= 0"),
                          (lambda: build(6, 1, np.array([np.nan, 2.0, 1.0]), out, 9), "window entries must be finite and >= 0"),
                          (lambda: build(6, 1, np.array([1.0, 2.0, np.inf]), out, 9), "window entries must be finite and >= 0"),
                          (lambda: build(6, 1, np.array([1.0, 0.0, 1.0]), out, 9), "window[band_half] must be > 0"),
                          (lambda: build(6, 1, w, out, 5), "out_pitch smaller than n_states")):
        assert call() == BAD and lib.jsgx_last_error() == f"jsgx_viterbi_band_build: {message}".encode()
    # in their order: the earlier defect is the one reported
    assert build(0, 65, None, None, 0) == BAD and lib.jsgx_last_error().endswith(b"null window")
    assert build(0, 65, np.array([-1.0]), out, 0) == BAD and lib.jsgx_last_error().endswith(b"n_states must be in 1..2048")
    assert build(6, 1, np.array([-1.0, 0.0, 1.0]), out, 0) == BAD and lib.jsgx_last_error().endswith(b"window entries must be finite and >= 0")
    with pytest.raises(jsg.JsgError, match="2 \\* band_half \\+ 1"):
        jsg.viterbi_band_transition(6, [1.0, 1.0])


def test_python_names(jsg):
    want = {
        "viterbi": ["log_emit", "log_trans", "log_init", "band_half"],
        "viterbi_scratch_bytes": ["d_log_emit", "d_log_init", "d_log_trans", "d_states", "band_half", "d_logp", "d_value"],
        "viterbi_launch": ["d_log_emit", "d_log_init", "d_log_trans", "d_states", "band_half", "d_logp", "d_value", "d_scratch", "stream"],
        "viterbi_plan": ["n_states", "n_frames", "seqs", "band_half"],
        "viterbi_band_transition": ["n_states", "window"],
    }
    for name, params in want.items():
        assert callable(getattr(jsg, name)) and name in jsg.__all__
        assert list(inspect.signature(getattr(jsg, name)).parameters) == params, name
    sig = inspect.signature(jsg.viterbi)
    assert [p.default for p in sig.parameters.values()][2:] == [None, None] and sig.parameters["band_half"].kind == inspect.Parameter.KEYWORD_ONLY
    assert [p.default for p in inspect.signature(jsg.viterbi_plan).parameters.values()][2:] == [1, None]
    for name in ("jsgx_viterbi_scratch_bytes", "jsgx_viterbi_launch", "jsgx_viterbi_plan", "jsgx_viterbi_band_build"):
        assert name in jsg.capix.SIGNATURES


def test_kernel_notes(capix, tmp_path):
    """The new object: its seven kernels, no private segment (no scratch memory, no spills), no static LDS in the forward forms (all of
    it is dynamic, as the plan states it) and the workgroup sizes."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    obj = os.path.join(ROOT, "jadespectrogram_amd", "build", "jsgx_viterbi.o")
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
    forward = (0, 0, 0, 0, capix.VITERBI_THREADS)
    assert found == {"jsgx::viterbi_forward_kernel<false, false>": forward, "jsgx::viterbi_forward_kernel<false, true>": forward,
                     "jsgx::viterbi_forward_kernel<true, false>": forward, "jsgx::viterbi_forward_kernel<true, true>": forward,
                     "jsgx::viterbi_jump_kernel": (0, 0, 0, 0, 256), "jsgx::viterbi_ends_kernel": (0, 2048, 0, 0, 256), "jsgx::viterbi_trace_kernel": (0, 0, 0, 0, 64)}


def test_host_entry_points_under_asan_ubsan(capix):
    """tests/cpp/jsgx_viterbi_host_test.cpp (its own main: the refusals, the scratch size, the plans, the band builder on real host
    buffers) built together with the host units it calls under the address and undefined-behaviour sanitizers and run as a child process;
    the same program against the shipped library gives the same verdict."""
    d = tempfile.gettempdir()
    drv = os.path.join(ROOT, "tests", "cpp", "jsgx_viterbi_host_test.cpp")
    hosts = [os.path.join(ROOT, "jadespectrogram_amd", "csrc", f) for f in ("jsgx_beat_host.cpp", "jsgx_viterbi_host.cpp")]
    common = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]
    san = os.path.join(d, "jsgx_viterbi_host_san")
    subprocess.check_call(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"] + hosts + [drv, "-o", san])
    libdir = os.path.dirname(capix.LIB_PATH)
    shipped = os.path.join(d, "jsgx_viterbi_host_lib")
    subprocess.check_call(common + [drv, "-o", shipped, "-L", libdir, "-ljsgx", f"-Wl,-rpath,{libdir}"])
    for exe in (san, shipped):
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == "ok" and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr

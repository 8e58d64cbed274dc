"""Section 5 of the companion library, host side (include/jsgx.h): every refusal of the two pYIN launches in its stated order (all decided
without a device), plans and scratch size over the corners, the struct layouts against a C program, the four table builders against scipy
and numpy in double, the exported symbols and the header, the census of the decoder's lane splits against the lists of the GPU test, the
Python names, the kernels' notes, and the host entry points from a stand-alone C++ program under the address and undefined-behaviour
sanitizers.  CPU only."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import pyin_ref as pr
from test_jsgx_forms_host import census

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# never dereferenced: every call below is refused, sized or planned
A1, A2, A3, A4, A5, A6, A7, A8, SCRATCH = (i << 44 for i in range(1, 10))
BAD = -2


@pytest.fixture(scope="module")
def capix(jsg):
    if not os.path.exists(jsg.capix.LIB_PATH):
        from jadespectrogram_amd import _build
        _build.build_lib()
    jsg.capix.lib()
    return jsg.capix


def observe_args(capix, **kw):
    a = dict(cmnd=A1, cmnd_frame_pitch=344, cmnd_row_pitch=34400, rows=3, n_frames=100, tau_min=10, tau_max=338, prior=A2, decay=A3, norm=A4, edges=A5,
             n_thresholds=100, boltz_len=164, n_bins=601, no_trough_prob=0.01, log_emit=A6, emit_frame_pitch=1202, emit_row_pitch=120200, obs=A7,
             obs_frame_pitch=601, obs_row_pitch=60100, voiced_prob=A8, voiced_pitch=100)
    a.update(kw)
    return capix.PyinObserveArgs(**a)


def decode_args(capix, **kw):
    a = dict(log_emit=A1, emit_frame_pitch=1202, emit_seq_pitch=120200, log_init=A2, log_window=A3, src_offset=A4, log_switch=A5, n_bins=601, band_half=50, seqs=3,
             n_frames=100, states=A6, states_pitch=100, logp=A7, value=A8, value_frame_pitch=1202, value_seq_pitch=120200)
    a.update(kw)
    return capix.PyinDecodeArgs(**a)


def scratch_formula(capix, seqs, S, T):
    blocks = -(-T // capix.VITERBI_BLOCK)
    return -(-(4 * seqs * S + 4 * seqs * blocks + 2 * seqs * T * S + 2 * seqs * blocks * S) // 4) * 4


# in the order of the header: a call with two defects is refused for the earlier one
OBSERVE_REFUSED = [
    ("null cmnd", dict(cmnd=None), "null cmnd"),
    ("null prior", dict(prior=None), "null prior"),
    ("null decay", dict(decay=None), "null decay"),
    ("null norm", dict(norm=None), "null norm"),
    ("null edges", dict(edges=None), "null edges"),
    ("null log_emit", dict(log_emit=None), "null log_emit"),
    ("misaligned cmnd", dict(cmnd=A1 + 2), "pointers must be 4-byte aligned"),
    ("misaligned voiced_prob", dict(voiced_prob=A8 + 1), "pointers must be 4-byte aligned"),
    ("no rows", dict(rows=0), "rows must be in 1..65535"),
    ("65536 rows", dict(rows=65536), "rows must be in 1..65535"),
    ("no frames", dict(n_frames=0), "n_frames must be in 1..2^20"),
    ("tau_max 0", dict(tau_max=0), "tau_max must be in 1..4096"),
    ("tau_max 4097", dict(tau_max=4097, cmnd_frame_pitch=4100, cmnd_row_pitch=410000), "tau_max must be in 1..4096"),
    ("tau_min 0", dict(tau_min=0), "tau_min must be in 1..tau_max"),
    ("tau_min above tau_max", dict(tau_min=339), "tau_min must be in 1..tau_max"),
    ("no thresholds", dict(n_thresholds=0), "n_thresholds must be in 1..256"),
    ("257 thresholds", dict(n_thresholds=257), "n_thresholds must be in 1..256"),
    ("no bins", dict(n_bins=0), "n_bins must be in 1..1024"),
    ("1025 bins", dict(n_bins=1025, emit_frame_pitch=2050, emit_row_pitch=205000, obs_frame_pitch=1025, obs_row_pitch=102500), "n_bins must be in 1..1024"),
    ("boltz_len short", dict(boltz_len=163), "boltz_len must be in max(1, (tau_max - tau_min + 1) / 2)..4096"),
    ("boltz_len 4097", dict(boltz_len=4097), "boltz_len must be in max(1, (tau_max - tau_min + 1) / 2)..4096"),
    ("no_trough_prob 1.5", dict(no_trough_prob=1.5), "no_trough_prob must be in [0, 1]"),
    ("no_trough_prob NaN", dict(no_trough_prob=float("nan")), "no_trough_prob must be in [0, 1]"),
    ("cmnd_frame_pitch", dict(cmnd_frame_pitch=338), "cmnd_frame_pitch smaller than tau_max + 1"),
    ("cmnd_row_pitch", dict(cmnd_row_pitch=99 * 344 + 338), "cmnd_row_pitch does not cover a row"),
    ("emit_frame_pitch", dict(emit_frame_pitch=1201), "emit_frame_pitch smaller than 2 * n_bins"),
    ("emit_row_pitch", dict(emit_row_pitch=120199), "emit_row_pitch does not cover a row"),
    ("obs_frame_pitch", dict(obs_frame_pitch=600), "obs_frame_pitch smaller than n_bins"),
    ("obs_row_pitch", dict(obs_row_pitch=60099), "obs_row_pitch does not cover a row"),
    ("voiced_pitch", dict(voiced_pitch=99), "voiced_pitch smaller than n_frames"),
    ("voiced_prob inside cmnd", dict(voiced_prob=A1 + 4 * 1000), "an output overlaps cmnd"),
    ("obs ends in prior", dict(obs=A2 - 4 * (2 * 60100 + 99 * 601 + 601) + 4), "an output overlaps prior"),
    ("voiced_prob inside decay", dict(voiced_prob=A3 + 4 * 163), "an output overlaps decay"),
    ("voiced_prob inside norm", dict(voiced_prob=A4 + 4 * 164), "an output overlaps norm"),
    ("voiced_prob inside edges", dict(voiced_prob=A5 + 4 * 601), "an output overlaps edges"),
    ("voiced_prob inside log_emit", dict(voiced_prob=A6 + 4 * 5000), "an output overlaps another output"),
]
DECODE_REFUSED = [
    ("null log_emit", dict(log_emit=None), "null log_emit"),
    ("null log_init", dict(log_init=None), "null log_init"),
    ("null log_window", dict(log_window=None), "null log_window"),
    ("null src_offset", dict(src_offset=None), "null src_offset"),
    ("null log_switch", dict(log_switch=None), "null log_switch"),
    ("null states", dict(states=None), "null states"),
    ("misaligned log_window", dict(log_window=A3 + 2), "pointers must be 4-byte aligned"),
    ("misaligned value", dict(value=A8 + 3), "pointers must be 4-byte aligned"),
    ("no seqs", dict(seqs=0), "seqs must be in 1..65535"),
    ("65536 seqs", dict(seqs=65536), "seqs must be in 1..65535"),
    ("no bins", dict(n_bins=0), "n_bins must be in 1..1024"),
    ("1025 bins", dict(n_bins=1025, emit_frame_pitch=2050, emit_seq_pitch=205000, value_frame_pitch=2050, value_seq_pitch=205000), "n_bins must be in 1..1024"),
    ("band_half -1", dict(band_half=-1), "band_half must be in 0..128"),
    ("band_half 129", dict(band_half=129), "band_half must be in 0..128"),
    ("no frames", dict(n_frames=0), "n_frames must be in 1..2^20"),
    ("2^20 + 1 frames", dict(n_frames=(1 << 20) + 1, states_pitch=1 << 21, emit_seq_pitch=1 << 32, value_seq_pitch=1 << 32), "n_frames must be in 1..2^20"),
    ("emit_frame_pitch", dict(emit_frame_pitch=1201), "emit_frame_pitch smaller than 2 * n_bins"),
    ("emit_seq_pitch", dict(emit_seq_pitch=120199), "emit_seq_pitch does not cover a sequence"),
    ("states_pitch", dict(states_pitch=99), "states_pitch smaller than n_frames"),
    ("value_frame_pitch", dict(value_frame_pitch=1201), "value_frame_pitch smaller than 2 * n_bins"),
    ("value_seq_pitch", dict(value_seq_pitch=120199), "value_seq_pitch does not cover a sequence"),
    ("states ends in log_emit", dict(states=A1 - 4 * 300 + 4), "an output overlaps log_emit"),
    ("logp inside log_init", dict(logp=A2 + 4 * 1201), "an output overlaps log_init"),
    ("logp inside log_window", dict(logp=A3 + 4 * 100), "an output overlaps log_window"),
    ("logp inside src_offset", dict(logp=A4 + 4 * 600), "an output overlaps src_offset"),
    ("logp inside log_switch", dict(logp=A5 + 4 * 3), "an output overlaps log_switch"),
    ("logp inside states", dict(logp=A6 + 4 * 299), "an output overlaps another output"),
]
OBSERVE_CALLS = (("jsgx_pyin_observe_launch", lambda lib, a: lib.jsgx_pyin_observe_launch(C.byref(a), None)),
                 ("jsgx_pyin_observe_plan", lambda lib, a: lib.jsgx_pyin_observe_plan(C.byref(a), None, 0, None, None, None)))
DECODE_CALLS = (("jsgx_pyin_decode_launch", lambda lib, a: lib.jsgx_pyin_decode_launch(C.byref(a), SCRATCH, 1 << 40, None)),
                ("jsgx_pyin_decode_scratch_bytes", lambda lib, a: lib.jsgx_pyin_decode_scratch_bytes(C.byref(a))),
                ("jsgx_pyin_decode_plan", lambda lib, a: lib.jsgx_pyin_decode_plan(C.byref(a), None, 0, None, None, None, None)))


def in_order(capix, refused, calls, make, i):
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


@pytest.mark.parametrize("i", range(len(OBSERVE_REFUSED)), ids=[r[0] for r in OBSERVE_REFUSED])
def test_observe_refusals_in_their_order(capix, i):
    in_order(capix, OBSERVE_REFUSED, OBSERVE_CALLS, observe_args, i)


@pytest.mark.parametrize("i", range(len(DECODE_REFUSED)), ids=[r[0] for r in DECODE_REFUSED])
def test_decode_refusals_in_their_order(capix, i):
    in_order(capix, DECODE_REFUSED, DECODE_CALLS, decode_args, i)
    # ... also ahead of what only the launch refuses
    lib = capix.lib()
    a = decode_args(capix, **DECODE_REFUSED[i][1])
    assert lib.jsgx_pyin_decode_launch(C.byref(a), None, 0, None) == BAD and lib.jsgx_last_error() == f"jsgx_pyin_decode_launch: {DECODE_REFUSED[i][2]}".encode()


def test_what_only_the_launch_refuses_and_what_passes(capix):
    lib = capix.lib()
    a = decode_args(capix)
    need = scratch_formula(capix, 3, 1202, 100)
    for scratch, size, message in ((None, 1 << 40, "null scratch"), (SCRATCH + 2, 1 << 40, "scratch must be 4-byte aligned"),
                                   (SCRATCH, need - 1, "scratch smaller than jsgx_pyin_decode_scratch_bytes"), (None, 0, "null scratch")):
        assert lib.jsgx_pyin_decode_launch(C.byref(a), scratch, size, None) == BAD and lib.jsgx_last_error() == f"jsgx_pyin_decode_launch: {message}".encode()
    for call in (lib.jsgx_pyin_decode_launch(None, SCRATCH, 1 << 40, None), lib.jsgx_pyin_decode_scratch_bytes(None), lib.jsgx_pyin_decode_plan(None, None, 0, None, None, None, None),
                 lib.jsgx_pyin_observe_launch(None, None), lib.jsgx_pyin_observe_plan(None, None, 0, None, None, None)):
        assert call == BAD and lib.jsgx_last_error().endswith(b": null argument")
    buf = C.create_string_buffer(15)
    assert lib.jsgx_pyin_decode_plan(C.byref(a), buf, 15, None, None, None, None) == BAD and lib.jsgx_last_error() == b"jsgx_pyin_decode_plan: bad argument"
    assert lib.jsgx_pyin_observe_plan(C.byref(observe_args(capix)), buf, 15, None, None, None) == BAD and lib.jsgx_last_error() == b"jsgx_pyin_observe_plan: bad argument"
    size = lambda **kw: lib.jsgx_pyin_decode_scratch_bytes(C.byref(decode_args(capix, **kw)))
    assert size() == need
    # one sequence: the sequence pitches are not looked at; the optional outputs may be missing, and then their pitches are not looked at
    assert size(seqs=1, emit_seq_pitch=0, states_pitch=0, value_seq_pitch=0) == scratch_formula(capix, 1, 1202, 100)
    assert size(logp=None) == need and size(value=None, value_frame_pitch=0, value_seq_pitch=0) == need
    # an output next to an input, not inside it
    assert size(logp=A5 + 16) == need and size(logp=A3 + 4 * 101) == need and size(states=A1 - 4 * 300) == need and size(logp=A6 + 4 * 300) == need
    plan = lambda **kw: lib.jsgx_pyin_observe_plan(C.byref(observe_args(capix, **kw)), None, 0, None, None, None)
    assert plan() == 0 and plan(rows=1, cmnd_row_pitch=0, emit_row_pitch=0, obs_row_pitch=0, voiced_pitch=0) == 0
    assert plan(obs=None, obs_frame_pitch=0, obs_row_pitch=0, voiced_prob=None, voiced_pitch=0) == 0
    assert plan(voiced_prob=A5 + 4 * 602) == 0 and plan(voiced_prob=A4 + 4 * 165) == 0 and plan(voiced_prob=A3 + 4 * 164) == 0
    assert plan(no_trough_prob=0.0) == 0 and plan(no_trough_prob=1.0) == 0 and plan(tau_min=338, boltz_len=1) == 0 and plan(tau_min=337, boltz_len=1) == 0


def test_no_device_comes_after_the_refusals(capix):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = capix.lib()
    assert lib.jsgx_pyin_decode_launch(C.byref(decode_args(capix)), SCRATCH, 1 << 40, None) == capix.JSGX_ERR_NO_DEVICE
    assert lib.jsgx_last_error() == b"jsgx_pyin_decode_launch: no HIP device"
    assert lib.jsgx_pyin_observe_launch(C.byref(observe_args(capix)), None) == capix.JSGX_ERR_NO_DEVICE
    assert lib.jsgx_last_error() == b"jsgx_pyin_observe_launch: no HIP device"
    assert lib.jsgx_pyin_decode_launch(C.byref(decode_args(capix)), SCRATCH, 16, None) == BAD


def test_plans_and_scratch_over_the_corners(jsg, capix):
    B = capix.VITERBI_BLOCK
    for P in (1, 2, 16, 17, 601, 1024):
        for W in (0, 1, 50, 128):
            for T in (1, B, B + 1, 1 << 20):
                name, G, threads, lds, launches = jsg.pyin_decode_plan(P, W, T, seqs=2)
                assert (name, G, threads) == ("pyin_decode",) + pr.form(P, W) and lds == 4 * (4 * (P + 2 * W) + 2 * W + 1) <= 65536 and launches == (3 if T <= B else 4)
                a = decode_args(capix, seqs=2, n_bins=P, band_half=W, n_frames=T, emit_frame_pitch=2 * P, emit_seq_pitch=2 * P * T, states_pitch=T, value_frame_pitch=2 * P,
                                value_seq_pitch=2 * P * T, log_emit=100 << 44, value=200 << 44, states=300 << 44)
                assert capix.lib().jsgx_pyin_decode_scratch_bytes(C.byref(a)) == scratch_formula(capix, 2, 2 * P, T)
    assert jsg.pyin_decode_plan(601, 50, 4096) == ("pyin_decode", 1, 640, 4 * (4 * 701 + 101), 4)
    for tau_min, tau_max, P in ((1, 1, 1), (1, 2, 1), (10, 338, 601), (1, 4096, 1024), (4096, 4096, 7)):
        assert jsg.pyin_observe_plan(tau_min, tau_max, P) == ("pyin_observe", 64, 4 * (tau_max + 1 + 3 * ((tau_max - tau_min + 1) // 2 + 1) + P), 1)
    assert jsg.pyin_observe_plan(1, 4096, 1024)[2] <= 65536
    with pytest.raises(jsg.JsgError, match="n_bins must be in"):
        jsg.pyin_decode_plan(1025, 5, 5)
    with pytest.raises(jsg.JsgError, match="band_half must be in"):
        jsg.pyin_decode_plan(5, 129, 5)
    with pytest.raises(jsg.JsgError, match="tau_max must be in"):
        jsg.pyin_observe_plan(1, 4097, 5)
    hdr = open(os.path.join(ROOT, "include", "jsgx.h")).read()
    for name, value in (("JSGX_PYIN_MAX_BINS", capix.PYIN_MAX_BINS), ("JSGX_PYIN_MAX_BAND_HALF", capix.PYIN_MAX_BAND_HALF), ("JSGX_PYIN_MAX_THRESHOLDS", capix.PYIN_MAX_THRESHOLDS),
                        ("JSGX_PYIN_MAX_LAG", capix.PYIN_MAX_LAG), ("JSGX_PYIN_OBSERVE_THREADS", capix.PYIN_OBSERVE_THREADS), ("JSGX_PYIN_THREADS", capix.PYIN_THREADS),
                        ("JSGX_VITERBI_MAX_BAND_HALF", 64), ("JSGX_ABI_VERSION", 1)):
        assert re.search(rf"#define {name} {value}\b", hdr), name
    assert re.search(r"#define JSGX_LOG_ABS_BOUND 1\.0e-7\b", hdr) and capix.LOG_ABS_BOUND == 1.0e-7
    for form in ("pyin_observe", "pyin_decode"):
        assert f'"{form}"' in hdr


@pytest.mark.parametrize("struct, ctype_name, size", [("jsgx_pyin_observe_args", "PyinObserveArgs", 152), ("jsgx_pyin_decode_args", "PyinDecodeArgs", 120)])
def test_struct_layouts_match_the_header(capix, tmp_path, struct, ctype_name, size):
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
    ctype = getattr(capix, ctype_name)
    assert out[0] == str(C.sizeof(ctype)) == str(size)
    assert [f for f, _ in ctype._fields_] == names
    offset = 0
    for (f, _), line in zip(ctype._fields_, out[1:]):
        assert line == f"{f} {getattr(ctype, f).offset} {getattr(ctype, f).size}"
        assert getattr(ctype, f).offset == offset, f"padding in front of {f}"
        offset += getattr(ctype, f).size


def ulps_apart(a, b):
    """The distance in float32 steps between two float32 arrays of one sign pattern (and equal infinities)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert (np.isinf(a) == np.isinf(b)).all() and (a[np.isinf(a)] == b[np.isinf(b)]).all()
    fin = ~np.isinf(a)
    return np.abs(a[fin].view(np.int32).astype(np.int64) - b[fin].view(np.int32).astype(np.int64))


@pytest.mark.parametrize("ab, N", [((2, 18), 100), ((1, 1), 7), ((0.5, 0.5), 256), ((2, 18), 1)])
def test_prior_against_scipy(jsg, ab, N):
    """Both sides difference two doubles in [0, 1], and the tail bins of Beta(2, 18) are pure cancellation: one float32 ulp of the reference
    plus 2^-50."""
    from scipy import stats
    got = jsg.pyin_prior(N, ab)
    want = np.diff(stats.beta.cdf(np.linspace(0, 1, N + 1), *ab))
    assert got.dtype == np.float32 and got.shape == (N,)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want)
    print(f"prior {ab} N={N}: worst error {np.max(err / (ulp + 2.0 ** -50)):.3f} of the tolerance")
    assert (err <= ulp + 2.0 ** -50).all()
    assert abs(float(got.astype(np.float64).sum()) - 1.0) <= N * 2.0 ** -24


def test_boltzmann_bins_and_transition_builders_against_numpy(jsg, capix):
    """numpy in double, rounded once.  The builders and numpy call different exp, exp2 and log routines, which may differ in the last place of the
    double; that shows as 1 ulp of float32 in a rare entry at the most, so 1 ulp is what is asserted, and the count of differing entries is
    printed (with one C library and numpy build: none in any table)."""
    lib = capix.lib()
    differing = {}
    for lam, n in ((2.0, 1), (2.0, 164), (0.5, 4096), (7.25, 33)):
        decay, norm = np.full(n + 1, 777, np.float32), np.full(n + 2, 777, np.float32)
        assert lib.jsgx_pyin_boltzmann_build(lam, n, decay.ctypes.data, norm.ctypes.data) == 0 and decay[n] == 777 and norm[n + 1] == 777
        wd, wn = pr.boltzmann_tables(lam, n)
        for what, g, w in (("decay", decay[:n], wd), ("norm", norm[:n + 1], wn)):
            d = ulps_apart(g, w)
            assert d.max() <= 1, (what, lam, n)
            differing[what] = differing.get(what, 0) + int((d > 0).sum())
    for sr, fmin, bps, P in ((22050.0, 65.40639132514966, 10, 601), (48000.0, 30.0, 3, 1024), (100.0, 5.0, 1, 1), (8000.0, 55.0, 1024, 2)):
        edges, freqs = np.full(P + 2, 777, np.float32), np.full(P + 1, 777, np.float32)
        assert lib.jsgx_pyin_bins_build(sr, fmin, bps, P, edges.ctypes.data, freqs.ctypes.data) == 0 and edges[P + 1] == 777 and freqs[P] == 777
        we, wf = pr.bins_tables(sr, fmin, bps, P)
        for what, g, w in (("edges", edges[:P + 1], we), ("freqs", freqs[:P], wf)):
            d = ulps_apart(g, w)
            assert d.max() <= 1, (what, sr, P)
            differing[what] = differing.get(what, 0) + int((d > 0).sum())
        assert (np.diff(edges[:P + 1]) < 0).all() and (edges[:P] > sr / freqs[:P]).all() and (sr / freqs[:P] > edges[1:P + 1]).all()
    rng = np.random.default_rng(4)
    for P, W, sp in ((1, 0, 0.01), (1, 3, 0.5), (5, 4, 0.0), (601, 50, 0.01), (1024, 128, 1.0), (40, 64, 0.3)):
        window = rng.random(2 * W + 1) + 0.01
        if W >= 3:
            window[[0, W + 2]] = 0.0
        lw, off, sw = np.full(2 * W + 2, 777, np.float32), np.full(P + 1, 777, np.float32), np.full(5, 777, np.float32)
        assert lib.jsgx_pyin_transition_build(P, W, window.ctypes.data, sp, lw.ctypes.data, off.ctypes.data, sw.ctypes.data) == 0
        assert lw[2 * W + 1] == 777 and off[P] == 777 and sw[4] == 777
        wl, wo, ws = pr.transition_tables(P, window, sp)
        for what, g, w in (("log_window", lw[:-1], wl), ("src_offset", off[:P], wo), ("log_switch", sw[:4], ws)):
            d = ulps_apart(g, w)
            assert d.size == 0 or d.max() <= 1, (what, P, W)
            differing[what] = differing.get(what, 0) + int((d > 0).sum())
    print("entries that differ from numpy by 1 ulp:", differing)
    # the refusals in their order: the earlier defect is the one reported
    one = np.zeros(4, np.float32)
    w3 = np.array([1.0, 2.0, 1.0])
    last = lambda: lib.jsgx_last_error().split(b": ", 1)[1].decode()
    assert lib.jsgx_pyin_prior_build(0, -1.0, 1.0, None) == BAD and last() == "null out"
    assert lib.jsgx_pyin_prior_build(0, -1.0, 1.0, one.ctypes.data) == BAD and last() == "n_thresholds must be in 1..256"
    assert lib.jsgx_pyin_prior_build(257, 1.0, 1.0, one.ctypes.data) == BAD and last() == "n_thresholds must be in 1..256"
    assert lib.jsgx_pyin_prior_build(4, -1.0, 1.0, one.ctypes.data) == BAD and last() == "a and b must be finite and > 0"
    assert lib.jsgx_pyin_prior_build(4, 1.0, float("inf"), one.ctypes.data) == BAD and last() == "a and b must be finite and > 0"
    assert lib.jsgx_pyin_boltzmann_build(0.0, 0, None, None) == BAD and last() == "null decay"
    assert lib.jsgx_pyin_boltzmann_build(0.0, 0, one.ctypes.data, None) == BAD and last() == "null norm"
    assert lib.jsgx_pyin_boltzmann_build(0.0, 0, one.ctypes.data, one.ctypes.data) == BAD and last() == "lambda must be finite and > 0"
    assert lib.jsgx_pyin_boltzmann_build(2.0, 4097, one.ctypes.data, one.ctypes.data) == BAD and last() == "n must be in 1..4096"
    assert lib.jsgx_pyin_bins_build(0.0, 0.0, 0, 0, None, None) == BAD and last() == "null edges"
    assert lib.jsgx_pyin_bins_build(0.0, 0.0, 0, 0, one.ctypes.data, None) == BAD and last() == "null freqs"
    assert lib.jsgx_pyin_bins_build(0.0, 0.0, 0, 0, one.ctypes.data, one.ctypes.data) == BAD and last() == "sample_rate must be finite and > 0"
    assert lib.jsgx_pyin_bins_build(1.0, 0.0, 0, 0, one.ctypes.data, one.ctypes.data) == BAD and last() == "fmin must be finite and > 0"
    assert lib.jsgx_pyin_bins_build(1.0, 1.0, 0, 0, one.ctypes.data, one.ctypes.data) == BAD and last() == "bins_per_semitone must be in 1..1024"
    assert lib.jsgx_pyin_bins_build(1.0, 1.0, 1, 1025, one.ctypes.data, one.ctypes.data) == BAD and last() == "n_bins must be in 1..1024"
    build = lambda P, W, win, sp, a=one, b=one, c=one: lib.jsgx_pyin_transition_build(P, W, None if win is None else win.ctypes.data, sp, *(None if t is None else t.ctypes.data for t in (a, b, c)))
    for call, message in ((lambda: build(0, 129, None, 2.0, None, None, None), "null window"), (lambda: build(0, 129, w3, 2.0, None, None, None), "null log_window"),
                          (lambda: build(0, 129, w3, 2.0, one, None, None), "null src_offset"), (lambda: build(0, 129, w3, 2.0, one, one, None), "null log_switch"),
                          (lambda: build(0, 129, w3, 2.0), "n_bins must be in 1..1024"), (lambda: build(4, 129, w3, 2.0), "band_half must be in 0..128"),
                          (lambda: build(4, 1, np.array([-1.0, 0.0, 1.0]), 2.0), "window entries must be finite and >= 0"),
                          (lambda: build(4, 1, np.array([1.0, 0.0, np.inf]), 2.0), "window entries must be finite and >= 0"),
                          (lambda: build(4, 1, np.array([1.0, 0.0, 1.0]), 2.0), "window[band_half] must be > 0"), (lambda: build(4, 1, w3, 2.0), "switch_prob must be in [0, 1]"),
                          (lambda: build(4, 1, w3, -0.1), "switch_prob must be in [0, 1]"), (lambda: build(4, 1, w3, float("nan")), "switch_prob must be in [0, 1]")):
        assert call() == BAD and lib.jsgx_last_error() == f"jsgx_pyin_transition_build: {message}".encode()
    # the Python layer: pyin_tables holds what the builders give, and refuses what they refuse
    t = jsg.pyin_tables(22050.0, 65.40639132514966, 601, 10, 50, np.concatenate([np.arange(1, 52), np.arange(50, 0, -1)]), 10, 338)
    assert {k: v.shape for k, v in t.items()} == dict(prior=(100,), decay=(164,), norm=(165,), edges=(602,), freqs=(601,), log_window=(101,), src_offset=(601,),
                                                      log_switch=(4,), log_init=(1202,))
    assert all(v.dtype == np.float32 for v in t.values()) and np.isneginf(t["log_init"][:601]).all() and (t["log_init"][601:] == np.float32(np.log(1 / 601))).all()
    with pytest.raises(jsg.JsgError, match="2 \\* band_half \\+ 1"):
        jsg.pyin_tables(22050.0, 65.4, 601, 10, 50, [1.0, 1.0], 10, 338)
    with pytest.raises(jsg.JsgError, match="n_bins must be in"):
        jsg.pyin_tables(22050.0, 65.4, 1025, 10, 1, [1.0, 2.0, 1.0], 10, 338)
    with pytest.raises(jsg.JsgError, match="n_thresholds must be in"):
        jsg.pyin_prior(257)


def test_exported_symbols_and_the_header(capix):
    """libjsgx.so exports the nine new functions; the header declares them, and every jsgx_<name>( in it is exported."""
    new = {"jsgx_pyin_prior_build", "jsgx_pyin_boltzmann_build", "jsgx_pyin_bins_build", "jsgx_pyin_transition_build", "jsgx_pyin_observe_launch",
           "jsgx_pyin_observe_plan", "jsgx_pyin_decode_scratch_bytes", "jsgx_pyin_decode_launch", "jsgx_pyin_decode_plan"}
    assert new <= set(capix.SIGNATURES)
    out = subprocess.check_output(["nm", "-D", "--defined-only", capix.LIB_PATH], text=True)
    functions = {line.split()[-1] for line in out.splitlines() if len(line.split()) == 3 and line.split()[1] == "T"}
    assert new <= functions and functions == set(capix.SIGNATURES)
    hdr = open(os.path.join(ROOT, "include", "jsgx.h")).read()
    assert new <= set(re.findall(r"\b(jsgx_\w+)\(", hdr)) and set(re.findall(r"\b(jsgx_\w+)\(", hdr)) - {"jsgx_exp"} == set(capix.SIGNATURES)
    assert "#define JSGX_ABI_VERSION 1\n" in hdr and capix.lib().jsgx_abi_version() == 1


def test_decoder_shapes_cover_every_form_and_both_sides_of_every_boundary(jsg):
    """G over every (P, W): the restated rule equals the library's plan; every G is run by a listed shape; at every listed width both bin
    counts of every change of G along P are listed, and at P = 16 both widths of every change along W."""
    lib_form = lambda P, W: jsg.pyin_decode_plan(P, W, 3)[1:3]
    listed = {(P, W) for P in pr.FORM_BINS for W in pr.FORM_WIDTHS} | set(pr.FORM_PAIRS) | set(pr.FORM_WIDE)
    all_G = set()
    for W in range(0, jsg.capix.PYIN_MAX_BAND_HALF + 1):
        for P in (list(range(1, 70)) + [127, 128, 129, 255, 256, 257, 511, 512, 513, 601, 1023, 1024] if W not in pr.FORM_WIDTHS else range(1, jsg.capix.PYIN_MAX_BINS + 1)):
            assert lib_form(P, W) == pr.form(P, W), (P, W)      # ties the restated rule to the library
            all_G.add(pr.form(P, W)[0])
    assert all_G == {1, 2, 4, 8, 16, 32} == {pr.form(P, W)[0] for P, W in listed}
    for W in pr.FORM_WIDTHS:
        keys = {P: ("pyin_decode", pr.form(P, W)[0]) for P in range(1, jsg.capix.PYIN_MAX_BINS + 1)}
        changes = census(keys, pr.FORM_BINS, f"pyin decode, W = {W}")
        print(f"pyin decode, W = {W}: G changes at P =", changes)
        assert changes == {0: [], 1: [], 50: [65, 129, 257], 128: [17, 33, 65, 129, 257]}[W]
    keys = {W: ("pyin_decode", pr.form(16, W)[0]) for W in range(0, jsg.capix.PYIN_MAX_BAND_HALF + 1)}
    changes = census(keys, [W for P, W in listed if P == 16], "pyin decode, P = 16")
    assert changes == [8, 16, 32, 64, 128]
    # the issue's sizes
    assert {1, 2, 63, 64, 65, 601, 1024} <= set(pr.FORM_BINS) and {0, 1, 50, 128} <= set(pr.FORM_WIDTHS) and {1, 2, 255, 256, 257, 513} <= set(pr.FORM_FRAMES)
    assert any(W >= P for P, W in pr.FORM_WIDE) and all(P <= 1024 and W <= 128 for P, W in pr.FORM_WIDE + pr.FORM_PAIRS)
    # for every G a listed shape with fewer offsets than lanes would have; there is none by the rule: every lane has at least eight offsets
    assert all(2 * W + 1 >= 8 * pr.form(P, W)[0] or pr.form(P, W)[0] == 1 for P, W in listed)


def test_python_names(jsg):
    want = {
        "pyin_prior": ["n_thresholds", "beta_parameters"],
        "pyin_tables": ["sr", "fmin", "n_bins", "bins_per_semitone", "band_half", "window", "tau_min", "tau_max", "n_thresholds", "beta_parameters", "boltzmann_parameter",
                        "switch_prob"],
        "pyin_observe_launch": ["d_cmnd", "tau_min", "tau_max", "d_prior", "d_decay", "d_norm", "d_edges", "d_log_emit", "no_trough_prob", "d_obs", "d_voiced_prob", "stream"],
        "pyin_observe_plan": ["tau_min", "tau_max", "n_bins", "n_frames", "rows", "n_thresholds"],
        "pyin_decode_launch": ["d_log_emit", "d_log_init", "d_log_window", "d_src_offset", "d_log_switch", "d_states", "d_logp", "d_value", "d_scratch", "stream"],
        "pyin_decode_scratch_bytes": ["d_log_emit", "d_log_init", "d_log_window", "d_src_offset", "d_log_switch", "d_states", "d_logp", "d_value"],
        "pyin_decode_plan": ["n_bins", "band_half", "n_frames", "seqs"],
        "pyin_geometry": ["sr", "fmin", "fmax", "frame_length", "hop_length", "resolution", "max_transition_rate"],
        "pyin": ["x", "sr", "fmin", "fmax", "frame_length", "hop_length", "n_thresholds", "beta_parameters", "boltzmann_parameter", "resolution", "max_transition_rate",
                 "switch_prob", "no_trough_prob", "fill_na", "center"],
    }
    for name, params in want.items():
        assert callable(getattr(jsg, name)) and name in jsg.__all__
        assert list(inspect.signature(getattr(jsg, name)).parameters) == params, name
    defaults = [p.default for p in inspect.signature(jsg.pyin).parameters.values()][4:]
    assert defaults[:9] == [2048, None, 100, (2, 18), 2, 0.1, 35.92, 0.01, 0.01] and np.isnan(defaults[9]) and defaults[10] is True


def test_the_geometry_of_the_defaults_is_librosas(jsg):
    """librosa.pyin between C2 and C7 at 22 050 Hz: 10 bins per semitone, 601 pitch bins, max_semitones_per_frame = round(35.92 * 12 * 512 /
    22050) = 10 and transition_width = 10 * 10 + 1 = 101 points, so a half-width of 50; tau 10..338.  Other hops and resolutions by the
    same formulas, an odd product included (librosa's window then has an even number of points; the half-width is rounded down)."""
    C2, C7 = 65.40639132514966, 2093.004522404789
    assert jsg.pyin_geometry(22050, C2, C7) == (10, 601, 50, 10, 338)
    assert [p.default for p in inspect.signature(jsg.pyin_geometry).parameters.values()][3:] == [2048, None, 0.1, 35.92]
    assert jsg.pyin_geometry(22050, C2, C7, hop_length=256) == (10, 601, 25, 10, 338) and jsg.pyin_geometry(22050, C2, C7, frame_length=1024)[2] == 25
    assert jsg.pyin_geometry(22050, C2, C7, resolution=0.5) == (2, 121, 10, 10, 338) and jsg.pyin_geometry(22050, C2, C7, resolution=1.0)[:3] == (1, 61, 5)
    assert jsg.pyin_geometry(44100, 55.0, 880.0, 4096, 512, 1 / 3, 35.92) == (3, 145, 7, 50, 802)        # round(5.004) * 3 = 15 -> 7
    assert jsg.pyin_geometry(22050, C2, C7, 8192, 2048)[2] == 200                                          # beyond what the decoder serves: pyin refuses it
    # the tables of the defaults have the model's sizes, and the plan is the one the documents quote
    bps, P, W, tau_min, tau_max = jsg.pyin_geometry(22050, C2, C7)
    t = jsg.pyin_tables(22050, C2, P, bps, W, np.concatenate([np.arange(1, W + 2), np.arange(W, 0, -1)]), tau_min, tau_max)
    assert t["log_window"].shape == (101,) and t["log_init"].shape == (1202,) and t["decay"].shape == (164,)
    assert jsg.pyin_decode_plan(P, W, 4096, 8) == ("pyin_decode", 1, 640, 11620, 4)


def test_kernel_notes(capix, tmp_path):
    """The new object: its two kernels, no private segment (no scratch memory, no spills), no static LDS (all of it is dynamic, as the
    plans state it) and the workgroup sizes."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    obj = os.path.join(ROOT, "jadespectrogram_amd", "build", "jsgx_pyin.o")
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
    assert found == {"jsgx::pyin_observe_kernel": (0, 0, 0, 0, capix.PYIN_OBSERVE_THREADS), "jsgx::pyin_forward_kernel": (0, 0, 0, 0, capix.PYIN_THREADS)}


def test_host_entry_points_under_asan_ubsan(capix):
    """tests/cpp/jsgx_pyin_host_test.cpp (its own main: the builders on real host buffers with guards, the refusals, the plans, the scratch
    size) built together with the host units it calls under the address and undefined-behaviour sanitizers and run as a child process; the
    same program against the shipped library gives the same verdict."""
    d = tempfile.gettempdir()
    drv = os.path.join(ROOT, "tests", "cpp", "jsgx_pyin_host_test.cpp")
    hosts = [os.path.join(ROOT, "jadespectrogram_amd", "csrc", f) for f in ("jsgx_beat_host.cpp", "jsgx_viterbi_host.cpp", "jsgx_pyin_host.cpp")]
    common = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]
    san = os.path.join(d, "jsgx_pyin_host_san")
    subprocess.check_call(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"] + hosts + [drv, "-o", san])
    libdir = os.path.dirname(capix.LIB_PATH)
    shipped = os.path.join(d, "jsgx_pyin_host_lib")
    subprocess.check_call(common + [drv, "-o", shipped, "-L", libdir, "-ljsgx", f"-Wl,-rpath,{libdir}"])
    for exe in (san, shipped):
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == "ok" and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr

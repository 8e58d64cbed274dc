"""Constant-Q spectrograms, host side (include/jsg.h section 2h): the basis builder against tests/cqt_ref.py, its refusals, the plan swept
over the corners of the accepted range, the refusals of the launch (all decided without a device), the argument blocks of the Python
binding, the symbols and the resource use of the kernel.  CPU only."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import cqt_ref as cr
from test_binding_args import FakeTensor, expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# never dereferenced: every call below is refused before the basis or the data is looked at
CQ, IN, OUT = (i << 44 for i in range(1, 4))
L, HOP, K = 3000, 64, 9
T = cr.frames(L, HOP)
PATHS = {"cqt_span", "cqt_passes"}
LDS_MAX = 163840


def spec(jsg, **kw):
    a = dict(fs=22050.0, fmin=cr.C1, n_bins=24, bins_per_octave=12, filter_scale=1.0, gamma=0.0, scale=1)
    a.update(kw)
    return jsg.capi.CqtSpec(**a)


def valid_args(jsg, **kw):
    a = dict(in_=IN, in_pitch=L, rows=2, in_samples=L, hop=HOP, n_frames=T, out=OUT, out_frame_pitch=K, out_row_pitch=T * K, out_power=0, chunk_frames=0)
    a.update(kw)
    return jsg.capi.CqtArgs(**a)


def build(jsg, s):
    lib = jsg.capi.lib()
    total = C.c_int64(-1)
    assert lib.jsg_cqt_basis_build(C.byref(s), None, None, None, None, 0, C.byref(total)) == jsg.capi.JSG_OK          # count only
    half, off, hz = np.zeros(s.n_bins, np.int32), np.zeros(s.n_bins, np.int64), np.zeros(s.n_bins, np.float32)
    taps = np.zeros(total.value, np.complex64)
    n = C.c_int64(-1)
    assert lib.jsg_cqt_basis_build(C.byref(s), half.ctypes.data, off.ctypes.data, hz.ctypes.data, taps.ctypes.data, total.value, C.byref(n)) == jsg.capi.JSG_OK
    assert n.value == total.value
    return half, off, hz, taps


BASES = {"standard": dict(), "unscaled": dict(scale=0), "variable-Q": dict(gamma=24.7 * 0.1079), "84 bins": dict(n_bins=84),
         "36 per octave": dict(n_bins=60, bins_per_octave=36), "narrow": dict(filter_scale=0.5, fmin=1000.0, n_bins=36),
         "one tap": dict(fs=8.0, fmin=1.0, n_bins=1, bins_per_octave=1, filter_scale=0.05)}


@pytest.mark.parametrize("name", sorted(BASES))
def test_basis_builder_matches_numpy(jsg, name):
    s = spec(jsg, **BASES[name])
    half, off, hz, taps = build(jsg, s)
    w_half, w_off, w_f, w_len, w_taps = cr.basis(s.fs, s.fmin, s.n_bins, s.bins_per_octave, s.filter_scale, s.gamma, bool(s.scale))
    assert np.array_equal(half, w_half) and np.array_equal(off, w_off) and np.array_equal(hz, w_f.astype(np.float32))
    if name == "one tap":
        assert half[0] == 0 and taps.size == 1
    for k in range(s.n_bins):
        n = 2 * int(half[k]) + 1
        got, want = taps[off[k]:off[k] + n].astype(np.complex128), w_taps[off[k]:off[k] + n].astype(np.complex128)
        peak = np.abs(want).max()
        assert np.abs(got.real - want.real).max() <= 2.0 ** -23 * peak and np.abs(got.imag - want.imag).max() <= 2.0 ** -23 * peak, k
        l1 = np.abs(got).sum() / (np.sqrt(w_len[k]) if s.scale else 1.0)
        assert abs(l1 - 1.0) <= 1e-6, (k, l1)
    b = jsg.CqtBasis(s.fs, s.fmin, s.n_bins, s.bins_per_octave, s.filter_scale, s.gamma, bool(s.scale))
    assert np.array_equal(b.half_lengths, half) and np.array_equal(b.taps, taps) and np.array_equal(b.frequencies, hz) and b.n_bins == s.n_bins


BASIS_REFUSED = {
    "fs 0": (dict(fs=0.0), "fs must be finite and > 0"),
    "fs nan": (dict(fs=float("nan")), "fs must be finite and > 0"),
    "fmin negative": (dict(fmin=-1.0), "fmin must be finite and > 0"),
    "fmin inf": (dict(fmin=float("inf")), "fmin must be finite and > 0"),
    "no bins": (dict(n_bins=0), "n_bins must be in 1..4096"),
    "4097 bins": (dict(n_bins=4097), "n_bins must be in 1..4096"),
    "B 0": (dict(bins_per_octave=0), "bins_per_octave must be in 1..1200"),
    "B 1201": (dict(bins_per_octave=1201), "bins_per_octave must be in 1..1200"),
    "filter_scale 0": (dict(filter_scale=0.0), "filter_scale must be finite and > 0"),
    "filter_scale nan": (dict(filter_scale=float("nan")), "filter_scale must be finite and > 0"),
    "gamma negative": (dict(gamma=-1e-9), "gamma must be finite and >= 0"),
    "gamma inf": (dict(gamma=float("inf")), "gamma must be finite and >= 0"),
    "past Nyquist": (dict(n_bins=102), "the highest bin reaches past fs / 2"),
    "a bin too long": (dict(fmin=1.0, n_bins=12), "a bin is longer than 2 * 131072 + 1 taps"),
    "too many taps": (dict(fmin=25.0, n_bins=900, bins_per_octave=100, fs=44100.0), "the basis has more than 2^24 taps"),
}


@pytest.mark.parametrize("what", sorted(BASIS_REFUSED))
def test_basis_builder_refusals(jsg, what):
    lib, bad = jsg.capi.lib(), jsg.capi.JSG_ERR_INVALID
    change, message = BASIS_REFUSED[what]
    s = spec(jsg, **change)
    n = C.c_int64(-1)
    assert lib.jsg_cqt_basis_build(C.byref(s), None, None, None, None, 0, C.byref(n)) == bad and n.value == 0
    assert lib.jsg_last_error(None) == b"jsg_cqt_basis_build: " + message.encode()
    p = C.c_void_p()
    assert lib.jsg_cqt_create(C.byref(p), C.byref(s)) == bad and not p                 # before it looks for a device
    with pytest.raises(jsg.JsgError):
        jsg.CqtBasis(s.fs, s.fmin, s.n_bins, s.bins_per_octave, s.filter_scale, s.gamma, bool(s.scale))


def test_basis_builder_null_and_capacity(jsg):
    lib, bad = jsg.capi.lib(), jsg.capi.JSG_ERR_INVALID
    s, n = spec(jsg), C.c_int64()
    assert lib.jsg_cqt_basis_build(None, None, None, None, None, 0, C.byref(n)) == bad and lib.jsg_last_error(None) == b"jsg_cqt_basis_build: null argument"
    assert lib.jsg_cqt_basis_build(C.byref(s), None, None, None, None, 0, None) == bad
    taps = np.zeros(16, np.complex64)
    assert lib.jsg_cqt_basis_build(C.byref(s), None, None, None, taps.ctypes.data, 16, C.byref(n)) == bad and not taps.any()
    assert lib.jsg_last_error(None) == b"jsg_cqt_basis_build: taps_cap is smaller than the number of taps"
    # the edge of the Nyquist rule: 101 bins from C1 at 12 per octave reach 10548 Hz (x 1.029 < 11025), 102 do not
    assert lib.jsg_cqt_basis_build(C.byref(spec(jsg, n_bins=101)), None, None, None, None, 0, C.byref(n)) == jsg.capi.JSG_OK and n.value > 0


def test_create_refusals_and_no_device(jsg):
    lib, bad = jsg.capi.lib(), jsg.capi.JSG_ERR_INVALID
    err = lambda: lib.jsg_last_error(None)
    half, taps = cr.synthetic_basis()
    half, taps = np.array(half), np.array(taps)
    p = C.c_void_p()
    assert lib.jsg_cqt_create(None, C.byref(spec(jsg))) == bad and err() == b"jsg_cqt_create: null argument"
    assert lib.jsg_cqt_create_tables(None, K, half.ctypes.data, taps.ctypes.data) == bad and err() == b"jsg_cqt_create_tables: null argument"
    for n in (0, -1, 4097):
        assert lib.jsg_cqt_create_tables(C.byref(p), n, half.ctypes.data, taps.ctypes.data) == bad and err() == b"jsg_cqt_create_tables: n_bins must be in 1..4096"
    assert lib.jsg_cqt_create_tables(C.byref(p), K, None, taps.ctypes.data) == bad and err() == b"jsg_cqt_create_tables: null half_len"
    for v in (-1, 131073):
        h = half.copy()
        h[3] = v
        assert lib.jsg_cqt_create_tables(C.byref(p), K, h.ctypes.data, taps.ctypes.data) == bad and err() == b"jsg_cqt_create_tables: half_len must be in 0..131072"
    big = np.full(65, 131072, np.int32)                     # 65 x 262145 taps > 2^24
    assert lib.jsg_cqt_create_tables(C.byref(p), 65, big.ctypes.data, taps.ctypes.data) == bad and err() == b"jsg_cqt_create_tables: the basis has more than 2^24 taps"
    assert lib.jsg_cqt_create_tables(C.byref(p), K, half.ctypes.data, None) == bad and err() == b"jsg_cqt_create_tables: null taps" and not p
    assert lib.jsg_cqt_bins(None) == bad and lib.jsg_cqt_total_taps(None) == bad and lib.jsg_cqt_half_len(None, None) == bad
    assert lib.jsg_cqt_destroy(None) == jsg.capi.JSG_OK
    rc = lib.jsg_cqt_create_tables(C.byref(p), K, half.ctypes.data, taps.ctypes.data)
    if lib.jsg_device_count() > 0:
        got = np.zeros(K, np.int32)
        assert rc == jsg.capi.JSG_OK and lib.jsg_cqt_bins(p) == K and lib.jsg_cqt_total_taps(p) == taps.size
        assert lib.jsg_cqt_half_len(p, got.ctypes.data) == jsg.capi.JSG_OK and np.array_equal(got, half)
        lib.jsg_cqt_destroy(p)
        return
    assert rc == jsg.capi.JSG_ERR_NO_DEVICE and not p          # after the refusals above; nothing runs on the host
    assert lib.jsg_cqt_create(C.byref(p), C.byref(spec(jsg))) == jsg.capi.JSG_ERR_NO_DEVICE and not p


# refused before the basis is read, in this order
REFUSED = {
    "null in": (dict(in_=None), "null data pointer"),
    "null out": (dict(out=None), "null data pointer"),
    "out_power 2": (dict(out_power=2), "out_power must be 0 or 1"),
    "out_power negative": (dict(out_power=-1), "out_power must be 0 or 1"),
    "misaligned in": (dict(in_=IN + 2), "in must be 4-byte aligned"),
    "misaligned complex out": (dict(out=OUT + 4), "out must be 8-byte aligned (power: 4-byte)"),
    "misaligned power out": (dict(out=OUT + 2, out_power=1), "out must be 8-byte aligned (power: 4-byte)"),
    "rows 0": (dict(rows=0), "rows must be in 1..65535"),
    "rows 65536": (dict(rows=65536), "rows must be in 1..65535"),
    "no samples": (dict(in_samples=0), "in_samples must be in 1..2^31-1"),
    "2^31 samples": (dict(in_samples=1 << 31, rows=1), "in_samples must be in 1..2^31-1"),
    "hop 0": (dict(hop=0), "hop must be in 1..2^20"),
    "hop above 2^20": (dict(hop=(1 << 20) + 1), "hop must be in 1..2^20"),
    "no frames": (dict(n_frames=0), "n_frames must be in 1..2^31-1"),
    "2^31 frames": (dict(n_frames=1 << 31), "n_frames must be in 1..2^31-1"),
    "negative chunk": (dict(chunk_frames=-1), "chunk_frames must be 0 or in 1..65536"),
    "chunk too long": (dict(chunk_frames=65537), "chunk_frames must be 0 or in 1..65536"),
    "in_pitch": (dict(in_pitch=L - 1), "in_pitch smaller than in_samples"),
}
# refused once the number of bins is known
REFUSED_OUT = {
    "frame pitch": (dict(out_frame_pitch=K - 1), "out_frame_pitch smaller than the number of bins"),
    "row pitch": (dict(out_row_pitch=T * K - 1), "out_row_pitch smaller than (n_frames-1)*out_frame_pitch + bins"),
    "out is in": (dict(out=IN), "out overlaps in"),
    "out inside in": (dict(out=IN + 4 * (2 * L - 2)), "out overlaps in"),
    "out ends inside in": (dict(out=IN - 8 * (2 * T * K - 1)), "out overlaps in"),
}


def plan_of(jsg, half, a):
    """jsg_cqt_plan: (rc, name, [(class_max_taps, frames_per_item, taps_per_pass, lds_bytes)])."""
    half = np.ascontiguousarray(half, np.int32)
    name, n = C.create_string_buffer(32), C.c_int32(-1)
    cols = [np.full(jsg.capi.CQT_MAX_CLASSES, -1, np.int32) for _ in range(4)]
    rc = jsg.capi.lib().jsg_cqt_plan(half.size, half.ctypes.data, C.byref(a), name, 32, C.byref(n), *[c.ctypes.data for c in cols])
    return rc, name.value.decode(), [tuple(int(c[i]) for c in cols) for i in range(max(n.value, 0))]


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refusals_need_no_device_and_no_basis(jsg, what):
    lib, bad = jsg.capi.lib(), jsg.capi.JSG_ERR_INVALID
    change, message = REFUSED[what]
    a = valid_args(jsg, **change)
    assert lib.jsg_cqt_launch(C.c_void_p(CQ), C.byref(a), None) == bad, what
    assert lib.jsg_last_error(None) == b"jsg_cqt_launch: " + message.encode()
    buf = C.create_string_buffer(32)
    assert lib.jsg_cqt_kernel_name(C.c_void_p(CQ), C.byref(a), buf, 32) == bad, what
    assert lib.jsg_last_error(None) == b"jsg_cqt_kernel_name: " + message.encode()
    assert plan_of(jsg, cr.synthetic_basis()[0], a)[0] == bad
    assert lib.jsg_last_error(None) == b"jsg_cqt_plan: " + message.encode()


@pytest.mark.parametrize("what", sorted(REFUSED_OUT))
def test_refusals_that_need_the_bin_count(jsg, what):
    lib, bad = jsg.capi.lib(), jsg.capi.JSG_ERR_INVALID
    change, message = REFUSED_OUT[what]
    assert plan_of(jsg, cr.synthetic_basis()[0], valid_args(jsg, **change))[0] == bad, what
    assert lib.jsg_last_error(None) == b"jsg_cqt_plan: " + message.encode()


def test_documented_order_of_the_refusals(jsg):
    """An argument block with every fault at once is refused for the first of the list; mended one by one it walks down the list."""
    lib, bad = jsg.capi.lib(), jsg.capi.JSG_ERR_INVALID
    order = ["null in", "out_power 2", "misaligned in", "rows 0", "no samples", "hop 0", "no frames", "negative chunk"]
    faults = {}
    for name in order:
        faults.update(REFUSED[name][0])
    faults["in_"] = None
    good = {f[0]: getattr(valid_args(jsg), f[0]) for f in jsg.capi.CqtArgs._fields_}
    for name in order:
        assert lib.jsg_cqt_launch(C.c_void_p(CQ), C.byref(valid_args(jsg, **faults)), None) == bad
        assert lib.jsg_last_error(None) == b"jsg_cqt_launch: " + REFUSED[name][1].encode(), name
        for key in REFUSED[name][0]:
            faults[key] = good[key]
            if name == "null in":
                faults[key] = IN + 2            # the next fault of the same field
    a = valid_args(jsg)
    err = lambda: lib.jsg_last_error(None)
    assert lib.jsg_cqt_launch(C.c_void_p(CQ), None, None) == bad and err() == b"jsg_cqt_launch: null argument"
    assert lib.jsg_cqt_launch(None, C.byref(a), None) == bad and err() == b"jsg_cqt_launch: null basis"
    buf = C.create_string_buffer(32)
    assert lib.jsg_cqt_kernel_name(C.c_void_p(CQ), C.byref(a), None, 32) == bad and err() == b"jsg_cqt_kernel_name: bad argument"
    assert lib.jsg_cqt_kernel_name(C.c_void_p(CQ), C.byref(a), buf, 8) == bad
    assert lib.jsg_cqt_kernel_name(None, C.byref(a), buf, 32) == bad and err() == b"jsg_cqt_kernel_name: null basis"
    if lib.jsg_device_count() > 0:
        return      # with a device the call below would go on to read the made-up basis; tests/test_gpu_cqt.py launches for real
    # every argument check that needs no basis passed: the device is asked for before the basis is read
    assert lib.jsg_cqt_launch(C.c_void_p(CQ), C.byref(a), None) == jsg.capi.JSG_ERR_NO_DEVICE and err() == b"jsg_cqt_launch: no HIP device"
    for change in (dict(rows=1, in_pitch=0, out_row_pitch=-1), dict(chunk_frames=65536), dict(out_power=1, out=OUT + 4), dict(hop=1 << 20, n_frames=(1 << 31) - 1)):
        assert lib.jsg_cqt_launch(C.c_void_p(CQ), C.byref(valid_args(jsg, **change)), None) == jsg.capi.JSG_ERR_NO_DEVICE, change
    assert lib.jsg_cqt_launch(C.c_void_p(CQ), C.byref(valid_args(jsg, rows=0)), None) == bad


def test_cqt_frames(jsg):
    lib, bad = jsg.capi.lib(), jsg.capi.JSG_ERR_INVALID
    top = (1 << 31) - 1
    for n, hop in ((1, 1), (3000, 1), (3000, 7), (3000, 512), (3000, 3000), (3000, 5000), (top, 1), (top, 1 << 20), (1, 1 << 20)):
        assert lib.jsg_cqt_frames(n, hop) == 1 + n // hop == cr.frames(n, hop) == jsg.cqt_frames(n, hop)
    for n, hop, message in ((0, 1, "in_samples must be in 1..2^31-1"), (1 << 31, 1, "in_samples must be in 1..2^31-1"), (10, 0, "hop must be in 1..2^20"),
                            (10, (1 << 20) + 1, "hop must be in 1..2^20")):
        assert lib.jsg_cqt_frames(n, hop) == bad and lib.jsg_last_error(None) == b"jsg_cqt_frames: " + message.encode()
    with pytest.raises(jsg.JsgError):
        jsg.cqt_frames(10, 0)


HALF_CORNERS = [0, 1, 15, 16, 31, 32, 100, 5842, 6143, 6144, 40000, 131072]


@pytest.mark.parametrize("hop", [1, 7, 512, 5000, 12288, 1 << 20])
def test_every_accepted_call_has_a_pass_that_fits(jsg, hop):
    """Bases at the corners of the accepted sizes at every corner of (hop, T, chunk_frames): a pass takes at least one frame and one
    tap (a pass of none would never end on the device) and a workgroup asks for no more than the LDS a compute unit has."""
    bases = [[h] for h in HALF_CORNERS] + [HALF_CORNERS, [0] * 4096, [131072] * 63, list(cr.SYNTH_HALF)]
    for half in bases:
        Kb = len(half)
        longest = 2 * max(half) + 1
        for frames in (1, 2, 100, (1 << 31) - 1):
            for chunk in (0, 1, 3, 16, 17, 65536):
                a = valid_args(jsg, rows=1, hop=hop, n_frames=frames, chunk_frames=chunk, out_frame_pitch=Kb, in_samples=(1 << 31) - 1)
                rc, name, classes = plan_of(jsg, half, a)
                assert rc == jsg.capi.JSG_OK, (half[:4], frames, chunk, jsg.capi.lib().jsg_last_error(None))
                assert name in PATHS and (name == "cqt_passes") == (longest > 12288), (name, longest)
                assert 1 <= len(classes) <= 20 and [c[0] for c in classes] == sorted({c[0] for c in classes}, reverse=True)
                assert classes[0][0] == longest
                for n_max, F, P, lds in classes:
                    assert 1 <= F <= min(chunk or 4096, frames) and 1 <= P == min(n_max, 12288) and 0 < lds <= LDS_MAX, (n_max, F, P, lds)
                    assert lds >= 4 * ((F - 1) * min(hop, P) + P)              # the windows of F frames of a pass
                    if n_max > P:
                        assert F <= 16                                        # one sweep: the accumulators stay in registers


def test_plan_sizes_items_by_work(jsg):
    half = cr.basis(22050.0, cr.C1, 84)[0]
    a = valid_args(jsg, rows=8, in_samples=4096 * 512, in_pitch=4096 * 512, hop=512, n_frames=4096, out_frame_pitch=84, out_row_pitch=4096 * 84,
                   out=1 << 50)
    rc, name, classes = plan_of(jsg, half, a)
    assert rc == jsg.capi.JSG_OK and name == "cqt_span" and classes[0][0] == 11685 and classes[-1][0] <= 128
    frames = [c[1] for c in classes]
    assert frames == sorted(frames) and frames[0] == 16 and frames[-1] > 64           # long bins take few frames per item, short bins many
    lib, bad = jsg.capi.lib(), jsg.capi.JSG_ERR_INVALID
    assert lib.jsg_cqt_plan(84, half.ctypes.data, C.byref(a), None, 0, None, None, None, None, None) == jsg.capi.JSG_OK
    assert lib.jsg_cqt_plan(84, half.ctypes.data, C.byref(a), C.create_string_buffer(8), 8, None, None, None, None, None) == bad
    assert lib.jsg_cqt_plan(84, half.ctypes.data, None, None, 0, None, None, None, None, None) == bad and lib.jsg_last_error(None) == b"jsg_cqt_plan: null argument"
    assert lib.jsg_cqt_plan(0, half.ctypes.data, C.byref(a), None, 0, None, None, None, None, None) == bad
    assert lib.jsg_cqt_plan(84, None, C.byref(a), None, 0, None, None, None, None, None) == bad
    X, Y = FakeTensor((8, 4096 * 512), torch.float32), FakeTensor((8, 4096, 84), torch.complex64, ptr=1 << 50)
    b = jsg.CqtBasis(22050.0, cr.C1, 84)
    assert jsg.cqt_plan(b, X, 512, 4096, Y) == (name, classes)


def test_abi_stays_at_6_and_exports_the_section(jsg):
    lib = jsg.capi.lib()
    assert lib.jsg_abi_version() == 6
    for name in ("jsg_cqt_basis_build", "jsg_cqt_create", "jsg_cqt_create_tables", "jsg_cqt_destroy", "jsg_cqt_bins", "jsg_cqt_half_len", "jsg_cqt_total_taps",
                 "jsg_cqt_frames", "jsg_cqt_launch", "jsg_cqt_plan", "jsg_cqt_kernel_name"):
        assert hasattr(lib, name) and name in jsg.capi.SIGNATURES
    assert C.sizeof(jsg.capi.CqtArgs) == 80 and C.sizeof(jsg.capi.CqtSpec) == 48
    header = open(os.path.join(ROOT, "include", "jsg.h")).read()
    assert "#define JSG_ABI_VERSION 6 " in header and "#define JSG_CQT_MAX_HALF_LEN 131072" in header and "#define JSG_CQT_MAX_BINS 4096" in header
    for name in ("CqtBasis", "cqt_frames", "cqt_launch", "cqt_plan", "cqt_kernel_name", "cqt", "vqt", "cqt_frequencies", "cqt_db"):
        assert callable(getattr(jsg, name)) and name in jsg.__all__
    assert np.allclose(jsg.cqt_frequencies(3, None, 12), cr.C1 * 2.0 ** (np.arange(3) / 12), rtol=1e-15)
    assert np.array_equal(jsg.cqt_frequencies(24, cr.C1, 12), cr.standard_basis()[2])


def test_cqt_args(jsg):
    S = jsg.spectrogram
    half, taps = cr.synthetic_basis()
    b = jsg.CqtBasis.from_tables(half, taps)
    assert b.n_bins == K and np.array_equal(b.offsets, cr.offsets(half)) and b.frequencies is None and b._handles == {}
    X = FakeTensor((3, 3000), torch.float32, strides=(3072, 1), ptr=0x7F0000900000)
    Y = FakeTensor((3, T, 11), torch.complex64, strides=(T * 11 + 5, 11, 1), ptr=0x7F0000B00000)
    base = dict(in_=X.data_ptr(), in_pitch=3072, rows=3, in_samples=3000, hop=HOP, n_frames=T, out=Y.data_ptr(), out_frame_pitch=11, out_row_pitch=T * 11 + 5)
    expect(S._cqt_args(b, X, HOP, T, Y, False, 0), **base)
    P = FakeTensor((3, T, K), torch.float32, ptr=0x7F0000B00000)
    expect(S._cqt_args(b, X, HOP, T - 1, P, True, 3), **dict(base, n_frames=T - 1, out_frame_pitch=K, out_row_pitch=T * K, out_power=1, chunk_frames=3))
    # one row: a one-dimensional input with a two-dimensional output
    expect(S._cqt_args(b, X[1], HOP, T, Y[1], False, 0), **dict(base, in_=X.data_ptr() + 3072 * 4, out=Y.data_ptr() + (T * 11 + 5) * 8, rows=1, in_pitch=3000,
                                                                 out_row_pitch=T * 11))
    bad = [(FakeTensor((3, 3000), torch.float64), Y, False), (X, P, False), (X, Y, True), (X, FakeTensor((2, T, 11), torch.complex64), False),
           (X, FakeTensor((3, T - 1, 11), torch.complex64), False), (X, FakeTensor((3, T, K - 1), torch.complex64), False),
           (FakeTensor((3, 3000), torch.float32, is_cuda=False), Y, False), (X, FakeTensor((3, T, 11), torch.complex64, strides=(T * 11, 1, T)), False)]
    for d_in, d_out, power in bad:
        with pytest.raises(AssertionError):
            S._cqt_args(b, d_in, HOP, T, d_out, power, 0)
    with pytest.raises(AssertionError):
        jsg.CqtBasis.from_tables(half, taps[:-1])
    b.close()


def test_cqt_kernel_has_no_scratch_and_no_spills(jsg):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    obj = os.path.join(ROOT, "jadespectrogram_amd", "build", "jsg_cqt.o")
    if not os.path.exists(obj):
        from jadespectrogram_amd import _build
        _build.build_lib()
    with tempfile.TemporaryDirectory() as tmp:
        co = kernel_regs.code_object(obj, tmp)
        notes = subprocess.check_output([os.path.join(kernel_regs.LLVM, "llvm-readelf"), "--notes", co]).decode()
    blks = [b for b in re.split(r"\n\s+- \.agpr_count", notes)[1:] if "cqt_kernel" in b]
    assert len(blks) == 1
    for blk in blks:
        for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            assert re.search(rf"\.{key}:\s+(\S+)", blk).group(1) == "0", key

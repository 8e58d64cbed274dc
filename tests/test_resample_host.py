"""Band-limited resampling, host side (include/jsg.h sections 1 and 2g): the table builder against numpy, the refusals (all decided
before any device call) with their messages, the output length, the argument blocks of the Python binding, the symbols and the
resource use of the new kernels.  CPU only."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import resample_ref as rr
from test_binding_args import FakeTensor, expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# never dereferenced: every call below is refused before the plan or the data is looked at
RS, IN, OUT = (i << 44 for i in range(1, 4))
L, STEP = 3000, 147 / 160
T = rr.resample_length(L, STEP)


def valid_args(jsg, **kw):
    a = dict(in_=IN, in_pitch=L, rows=2, in_samples=L, step=STEP, out=OUT, out_pitch=T, out_samples=T, chunk_outputs=0)
    a.update(kw)
    return jsg.capi.ResampleArgs(**a)


@pytest.mark.parametrize("name", ["best", "fast"])
def test_table_builder_matches_numpy(jsg, name):
    Z, P, rolloff, beta = {"best": rr.BEST, "fast": rr.FAST}[name]
    assert jsg.spectrogram.SINC_TABLES[name] == (Z, P, rolloff, beta)
    got, want = jsg.sinc_table(Z, P, rolloff, beta), rr.table(name)[2]
    assert got.dtype == np.float32 and got.shape == (Z * P + 1,)
    assert got[0] == np.float32(rolloff)
    ulp = np.spacing(np.abs(want))
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
    # the two ends of the parameter ranges
    tiny = jsg.sinc_table(1, 1, 1.0, 0.0)                     # no window: (1, sinc(1))
    assert tiny.shape == (2,) and tiny[0] == 1.0 and abs(tiny[1]) < 1e-15
    assert jsg.sinc_table(64, 512, 0.5, 30.0).shape == (32769,)


TABLE_REFUSED = {
    "Z 0": ((0, 512, 0.9, 8.0), "num_zeros must be >= 1"),
    "Z negative": ((-1, 512, 0.9, 8.0), "num_zeros must be >= 1"),
    "P 0": ((16, 0, 0.9, 8.0), "per_zero must be >= 1"),
    "too long": ((64, 513, 0.9, 8.0), "num_zeros * per_zero must be <= 32768"),
    "overflowing product": ((1 << 20, 1 << 20, 0.9, 8.0), "num_zeros * per_zero must be <= 32768"),
    "rolloff 0": ((16, 512, 0.0, 8.0), "rolloff must be in (0, 1]"),
    "rolloff above 1": ((16, 512, 1.0000001, 8.0), "rolloff must be in (0, 1]"),
    "rolloff nan": ((16, 512, float("nan"), 8.0), "rolloff must be in (0, 1]"),
    "beta negative": ((16, 512, 0.9, -1e-9), "beta must be finite and >= 0"),
    "beta inf": ((16, 512, 0.9, float("inf")), "beta must be finite and >= 0"),
    "beta nan": ((16, 512, 0.9, float("nan")), "beta must be finite and >= 0"),
}


@pytest.mark.parametrize("what", sorted(TABLE_REFUSED))
def test_table_builder_refusals(jsg, what):
    lib = jsg.capi.lib()
    (Z, P, rolloff, beta), message = TABLE_REFUSED[what]
    out = np.zeros(8, np.float32)
    assert lib.jsg_sinc_table_build(Z, P, rolloff, beta, out.ctypes.data) == jsg.capi.JSG_ERR_INVALID
    assert lib.jsg_last_error(None) == b"jsg_sinc_table_build: " + message.encode()
    assert not out.any()
    # the plan refuses the same sizes, before it looks for a device
    if "zeros" in message or "per_zero" in message:
        p = C.c_void_p()
        assert lib.jsg_resampler_create(C.byref(p), Z, P, out.ctypes.data) == jsg.capi.JSG_ERR_INVALID and not p
        assert lib.jsg_last_error(None) == b"jsg_resampler_create: " + message.encode()


def test_table_builder_null_and_python_errors(jsg):
    lib = jsg.capi.lib()
    assert lib.jsg_sinc_table_build(16, 512, 0.9, 8.0, None) == jsg.capi.JSG_ERR_INVALID
    assert lib.jsg_last_error(None) == b"jsg_sinc_table_build: null output pointer"
    with pytest.raises(jsg.JsgError) as e:
        jsg.sinc_table(16, 512, 1.5, 8.0)
    assert e.value.code == jsg.capi.JSG_ERR_INVALID and "rolloff" in str(e.value)
    with pytest.raises(jsg.JsgError):
        jsg.Resampler("better")


def test_plan_refusals_and_no_device(jsg):
    lib, bad = jsg.capi.lib(), jsg.capi.JSG_ERR_INVALID
    t = np.array(rr.table("ramp")[2])
    p = C.c_void_p()
    assert lib.jsg_resampler_create(None, 1, 64, t.ctypes.data) == bad and lib.jsg_last_error(None) == b"jsg_resampler_create: null argument"
    assert lib.jsg_resampler_create(C.byref(p), 1, 64, None) == bad
    for v in (np.nan, np.inf, -np.inf):
        u = t.copy()
        u[64] = v
        assert lib.jsg_resampler_create(C.byref(p), 1, 64, u.ctypes.data) == bad and not p
        assert lib.jsg_last_error(None) == b"jsg_resampler_create: the table must be finite"
    assert lib.jsg_resampler_zeros(None) == bad and lib.jsg_resampler_per_zero(None) == bad
    assert lib.jsg_resampler_destroy(None) == jsg.capi.JSG_OK
    rc = lib.jsg_resampler_create(C.byref(p), 1, 64, t.ctypes.data)
    if lib.jsg_device_count() > 0:
        assert rc == jsg.capi.JSG_OK and lib.jsg_resampler_zeros(p) == 1 and lib.jsg_resampler_per_zero(p) == 64
        lib.jsg_resampler_destroy(p)
        return
    assert rc == jsg.capi.JSG_ERR_NO_DEVICE and not p       # after the refusals above; nothing runs on the host


REFUSED = {
    "null in": (dict(in_=None), "null data pointer"),
    "null out": (dict(out=None), "null data pointer"),
    "misaligned in": (dict(in_=IN + 2), "in and out must be 4-byte aligned"),
    "misaligned out": (dict(out=OUT + 1), "in and out must be 4-byte aligned"),
    "rows 0": (dict(rows=0), "rows must be in 1..65535"),
    "rows 65536": (dict(rows=65536), "rows must be in 1..65535"),
    "no samples": (dict(in_samples=0), "in_samples must be in 1..2^31-1"),
    "2^31 samples": (dict(in_samples=1 << 31, rows=1), "in_samples must be in 1..2^31-1"),
    "step nan": (dict(step=float("nan")), "step must be finite and in 1/64..64"),
    "step inf": (dict(step=float("inf")), "step must be finite and in 1/64..64"),
    "step 0": (dict(step=0.0), "step must be finite and in 1/64..64"),
    "step negative": (dict(step=-1.0), "step must be finite and in 1/64..64"),
    "step below 1/64": (dict(step=np.nextafter(1 / 64, 0)), "step must be finite and in 1/64..64"),
    "step above 64": (dict(step=np.nextafter(64.0, 65)), "step must be finite and in 1/64..64"),
    "one output short": (dict(out_samples=T - 1), "out_samples differs from jsg_resample_length(in_samples, step)"),
    "one output long": (dict(out_samples=T + 1, out_pitch=T + 1), "out_samples differs from jsg_resample_length(in_samples, step)"),
    "negative chunk": (dict(chunk_outputs=-1), "chunk_outputs must be 0 or in 1..65536"),
    "chunk too long": (dict(chunk_outputs=65537), "chunk_outputs must be 0 or in 1..65536"),
    "in_pitch": (dict(in_pitch=L - 1), "in_pitch smaller than in_samples"),
    "out_pitch": (dict(out_pitch=T - 1), "out_pitch smaller than out_samples"),
    "out is in": (dict(out=IN), "out overlaps in"),
    "out inside in": (dict(out=IN + 4 * (2 * L - 1)), "out overlaps in"),
    "out ends inside in": (dict(out=IN - 4 * (2 * T - 1)), "out overlaps in"),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refusals_need_no_device(jsg, what):
    lib, bad = jsg.capi.lib(), jsg.capi.JSG_ERR_INVALID
    change, message = REFUSED[what]
    a = valid_args(jsg, **change)
    assert lib.jsg_resample_launch(C.c_void_p(RS), C.byref(a), None) == bad, what
    assert lib.jsg_last_error(None) == b"jsg_resample_launch: " + message.encode()
    buf = C.create_string_buffer(32)
    assert lib.jsg_resample_kernel_name(C.c_void_p(RS), C.byref(a), buf, 32) == bad, what
    assert lib.jsg_last_error(None) == b"jsg_resample_kernel_name: " + message.encode()


def test_null_arguments_and_adjacent_buffers(jsg):
    lib, bad = jsg.capi.lib(), jsg.capi.JSG_ERR_INVALID
    err = lambda: lib.jsg_last_error(None)
    a = valid_args(jsg)
    assert lib.jsg_resample_launch(C.c_void_p(RS), None, None) == bad and err() == b"jsg_resample_launch: null argument"
    assert lib.jsg_resample_launch(None, C.byref(a), None) == bad and err() == b"jsg_resample_launch: null resampler"
    buf = C.create_string_buffer(32)
    assert lib.jsg_resample_kernel_name(C.c_void_p(RS), C.byref(a), None, 32) == bad and err() == b"jsg_resample_kernel_name: bad argument"
    assert lib.jsg_resample_kernel_name(C.c_void_p(RS), C.byref(a), buf, 8) == bad
    if lib.jsg_device_count() > 0:
        return      # with a device the calls below would go on to read the made-up plan; tests/test_gpu_resample.py launches for real
    ok = jsg.capi.JSG_ERR_NO_DEVICE     # every argument check passed
    assert lib.jsg_resample_launch(C.c_void_p(RS), C.byref(a), None) == ok and err() == b"jsg_resample_launch: no HIP device"
    # adjacent buffers do not overlap; one row: the pitches are not looked at
    assert lib.jsg_resample_launch(C.c_void_p(RS), C.byref(valid_args(jsg, out=IN + 4 * 2 * L)), None) == ok
    assert lib.jsg_resample_launch(C.c_void_p(RS), C.byref(valid_args(jsg, out=IN - 4 * 2 * T)), None) == ok
    assert lib.jsg_resample_launch(C.c_void_p(RS), C.byref(valid_args(jsg, rows=1, in_pitch=0, out_pitch=-1)), None) == ok
    assert lib.jsg_resample_launch(C.c_void_p(RS), C.byref(valid_args(jsg, in_=IN + 4, out=OUT + 12)), None) == ok
    for chunk in (1, 63, 65536):
        assert lib.jsg_resample_launch(C.c_void_p(RS), C.byref(valid_args(jsg, chunk_outputs=chunk)), None) == ok
    # ... and NO_DEVICE only after the argument checks
    assert lib.jsg_resample_launch(C.c_void_p(RS), C.byref(valid_args(jsg, rows=0)), None) == bad


def test_resample_length_at_the_ends_of_its_ranges(jsg):
    lib, bad = jsg.capi.lib(), jsg.capi.JSG_ERR_INVALID
    top = (1 << 31) - 1
    assert lib.jsg_resample_length(1, 1 / 64) == 64 and lib.jsg_resample_length(1, 64.0) == 1 and lib.jsg_resample_length(1, 1.0) == 1
    assert lib.jsg_resample_length(top, 1 / 64) == top * 64 and lib.jsg_resample_length(top, 64.0) == (top + 63) // 64
    assert lib.jsg_resample_length(top, 1.0) == top and lib.jsg_resample_length(65, 64.0) == 2 and lib.jsg_resample_length(64, 64.0) == 1
    for name, (orig, new) in rr.RATIONAL.items():
        for n in (1, 2, 146, 147, 148, 159, 160, 161, 3000, 44100, 1 << 22, top):
            assert lib.jsg_resample_length(n, rr.STEPS[name]) == -(-n * new // orig), (name, n)
    for name, step in rr.STEPS.items():
        for n in (1, 40, 3000, 32768):
            assert lib.jsg_resample_length(n, step) == rr.resample_length(n, step) == jsg.resample_length(n, step)
    for n, step, message in [(0, 1.0, "in_samples must be in 1..2^31-1"), (-5, 1.0, "in_samples must be in 1..2^31-1"),
                             (1 << 31, 1.0, "in_samples must be in 1..2^31-1"), (10, 0.0, "step must be finite and in 1/64..64"),
                             (10, float("nan"), "step must be finite and in 1/64..64"), (10, float("inf"), "step must be finite and in 1/64..64"),
                             (10, 64.5, "step must be finite and in 1/64..64"), (10, 0.015, "step must be finite and in 1/64..64")]:
        assert lib.jsg_resample_length(n, step) == bad and lib.jsg_last_error(None) == b"jsg_resample_length: " + message.encode()
    with pytest.raises(jsg.JsgError):
        jsg.resample_length(10, 65.0)


def test_abi_stays_at_6_and_exports_the_section(jsg):
    lib = jsg.capi.lib()
    assert lib.jsg_abi_version() == 6
    for name in ("jsg_sinc_table_build", "jsg_resampler_create", "jsg_resampler_destroy", "jsg_resampler_zeros", "jsg_resampler_per_zero",
                 "jsg_resample_length", "jsg_resample_launch", "jsg_resample_plan", "jsg_resample_kernel_name"):
        assert hasattr(lib, name) and name in jsg.capi.SIGNATURES
    assert C.sizeof(jsg.capi.ResampleArgs) == 72 and jsg.capi.RESAMPLE_MAX_TABLE == 32768
    header = open(os.path.join(ROOT, "include", "jsg.h")).read()
    assert "#define JSG_RESAMPLE_MAX_TABLE 32768" in header and "#define JSG_ABI_VERSION 6 " in header
    for name in ("sinc_table", "Resampler", "resample_length", "resample_launch", "resample_kernel_name", "resample_plan", "resample", "pitch_shift"):
        assert callable(getattr(jsg, name)) and name in jsg.__all__


def test_resample_args(jsg):
    S = jsg.spectrogram
    X = FakeTensor((3, 3000), torch.float32, strides=(3072, 1), ptr=0x7F0000900000)
    Y = FakeTensor((3, T), torch.float32, strides=(3400, 1), ptr=0x7F0000B00000)
    base = dict(in_=X.data_ptr(), in_pitch=3072, rows=3, in_samples=3000, step=STEP, out=Y.data_ptr(), out_pitch=3400, out_samples=T)
    expect(S._resample_args(X, STEP, Y, 0), **base)
    expect(S._resample_args(X, 2.0, Y, 64), **dict(base, step=2.0, chunk_outputs=64))          # the library, not the binding, checks the length
    # one row: one-dimensional tensors, or a row of a batch
    expect(S._resample_args(X[1], STEP, Y[1], 0), **dict(base, in_=X.data_ptr() + 3072 * 4, out=Y.data_ptr() + 3400 * 4, rows=1, in_pitch=3000, out_pitch=T))
    bad = [(FakeTensor((3, 3000), torch.float64), Y), (X, FakeTensor((3, T), torch.float64)), (X, FakeTensor((2, T), torch.float32)),
           (FakeTensor((3, 3000), torch.float32, is_cuda=False), Y), (FakeTensor((3, 3000), torch.float32, strides=(1, 3)), Y),
           (FakeTensor((2, 3, 3000), torch.float32), Y)]
    for d_in, d_out in bad:
        with pytest.raises(AssertionError):
            S._resample_args(d_in, STEP, d_out, 0)


def test_python_calls_take_float32_only(jsg):
    for dtype in (torch.float64, torch.float16):
        with pytest.raises(AssertionError):
            jsg.resample(FakeTensor((2, 3000), dtype), 44100, 48000)
        with pytest.raises(AssertionError):
            jsg.pitch_shift(FakeTensor((2, 3000), dtype), 4)
    with pytest.raises(AssertionError):
        jsg.resample(FakeTensor((2, 3000), torch.float32, is_cuda=False), 44100, 48000)


def plan_of(jsg, Z, P, n, step, chunk=0):
    """jsg_resample_plan of one row of n samples: (rc, name, outputs per pass, LDS bytes)."""
    a = valid_args(jsg, rows=1, in_samples=n, step=step, out_samples=rr.resample_length(n, step), chunk_outputs=chunk, out=3 << 44)
    name, sub, lds = C.create_string_buffer(32), C.c_int32(-1), C.c_int32(-1)
    rc = jsg.capi.lib().jsg_resample_plan(Z, P, C.byref(a), name, 32, C.byref(sub), C.byref(lds))
    return rc, name.value.decode(), sub.value, lds.value


TABLE_CORNERS = [(1, 1), (1, 64), (1, 32768), (32768, 1), (64, 512), (16, 512), (320, 64), (1024, 32), (512, 64), (181, 181), (2, 16384), (4096, 8)]
STEP_CORNERS = [1 / 64, 0.5, 1.0, 1.0 + 2.0 ** -30, 2.0, 3.7, 14.0, 20.0, 21.3, 21.5, 63.9, 64.0]


@pytest.mark.parametrize("ZP", TABLE_CORNERS, ids=str)
def test_every_accepted_call_has_a_pass_that_fits(jsg, ZP):
    """Every table the plan accepts at every step the launch accepts: a pass takes at least one output (a pass of none would never
    end on the device) and a workgroup asks for no more than the 160 KiB a compute unit has."""
    Z, P = ZP
    for step in STEP_CORNERS:
        hw = -(-(Z * P << 32) // int(np.rint((1 / step if step > 1 else 1.0) * P * 2.0 ** 32)))
        for n in (1, 3000, (1 << 31) - 1):
            T = rr.resample_length(n, step)
            for chunk in (0, 1, 64, 4096, 65536):
                rc, name, sub, lds = plan_of(jsg, Z, P, n, step, chunk)
                assert rc == jsg.capi.JSG_OK, (step, n, chunk, jsg.capi.lib().jsg_last_error(None))
                assert 1 <= sub <= min(chunk or 4096, T) and 0 < lds <= 160 * 1024, (step, n, chunk, name, sub, lds)
                table_bytes = 4 * ((Z * P + 4) // 4 * 4)
                if name == "resample_direct":       # nothing but the table is staged, a chunk is one pass
                    assert lds == table_bytes and sub == min(chunk or 4096, T) and 2 * hw + 6 + 255 * step > 40960 - 256
                else:                               # the span of a pass: its outputs' reach plus both wings
                    assert name in ("resample_lds", "resample_l2")
                    span = lds // 4 - (table_bytes // 4 if name == "resample_lds" else 0)
                    assert span >= int((sub - 1) * step) + 2 * hw + 2, (step, n, chunk, name, sub, lds)


def test_plan_paths_and_refusals(jsg):
    lib, bad = jsg.capi.lib(), jsg.capi.JSG_ERR_INVALID
    # tables with many zero crossings at a large step: the wings alone exceed the LDS
    assert plan_of(jsg, 320, 64, 3000, 64.0)[1] == plan_of(jsg, 1024, 32, 3000, 20.0)[1] == plan_of(jsg, 512, 64, 3000, 64.0)[1] == "resample_direct"
    assert plan_of(jsg, 32768, 1, (1 << 31) - 1, 64.0)[1:] == ("resample_direct", 4096, 4 * 32772)
    assert plan_of(jsg, 64, 512, 3000, 64.0)[1] == "resample_l2" and plan_of(jsg, 64, 512, 3000, 21.3)[1] == "resample_lds"
    assert plan_of(jsg, 64, 512, 100000, 21.5)[1] == "resample_l2" and plan_of(jsg, 16, 512, 3000, 64.0)[1] == "resample_lds"
    assert plan_of(jsg, 64, 512, 10000, 2.0)[1:3] == ("resample_lds", 3964)         # a default chunk of 4096 outputs takes two passes
    a = valid_args(jsg)
    assert lib.jsg_resample_plan(64, 512, C.byref(a), None, 0, None, None) == jsg.capi.JSG_OK
    for Z, P in ((0, 512), (64, 0), (64, 513), (-1, -1), (1 << 20, 1 << 20)):
        assert lib.jsg_resample_plan(Z, P, C.byref(a), None, 0, None, None) == bad
        assert lib.jsg_last_error(None) == b"jsg_resample_plan: num_zeros and per_zero must be >= 1, their product <= 32768"
    assert lib.jsg_resample_plan(64, 512, C.byref(a), C.create_string_buffer(8), 8, None, None) == bad
    assert lib.jsg_resample_plan(64, 512, None, None, 0, None, None) == bad and lib.jsg_last_error(None) == b"jsg_resample_plan: null argument"
    for what in sorted(REFUSED):
        change, message = REFUSED[what]
        assert lib.jsg_resample_plan(64, 512, C.byref(valid_args(jsg, **change)), None, 0, None, None) == bad, what
        assert lib.jsg_last_error(None) == b"jsg_resample_plan: " + message.encode()
    X, Y = FakeTensor((3, 3000), torch.float32), FakeTensor((3, T), torch.float32, ptr=0x7F0000B00000)
    assert jsg.resample_plan(jsg.Resampler("fast"), X, STEP, Y) == plan_of(jsg, 16, 512, 3000, STEP)[1:]


def test_resampler_descriptions(jsg):
    best, fast = jsg.Resampler(), jsg.Resampler("fast")
    assert (best.num_zeros, best.per_zero, best.table.shape) == (64, 512, (32769,)) and (fast.num_zeros, fast.per_zero) == (16, 512)
    Z, P, t = rr.table("ramp")
    r = jsg.Resampler.from_table(t, Z, P)
    assert np.array_equal(r.table, t) and r.table.dtype == np.float32 and r._handles == {}
    with pytest.raises(AssertionError):
        jsg.Resampler.from_table(t[:-1], Z, P)
    best.close(), fast.close(), r.close()


def test_resample_kernels_have_no_scratch_and_no_spills(jsg):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    obj = os.path.join(ROOT, "jadespectrogram_amd", "build", "jsg_resample.o")
    if not os.path.exists(obj):
        from jadespectrogram_amd import _build
        _build.build_lib()
    with tempfile.TemporaryDirectory() as tmp:
        co = kernel_regs.code_object(obj, tmp)
        notes = subprocess.check_output([os.path.join(kernel_regs.LLVM, "llvm-readelf"), "--notes", co]).decode()
    blks = [b for b in re.split(r"\n\s+- \.agpr_count", notes)[1:] if "resample_kernel" in b]
    assert len(blks) == 3      # table and span in LDS, the table through L2, the input through L2
    for blk in blks:
        for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            assert re.search(rf"\.{key}:\s+(\S+)", blk).group(1) == "0", key

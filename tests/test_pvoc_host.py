"""Phase vocoder, host side (include/jsg.h section 2e): the frame count against the definition, the refusals (all decided before
anything is enqueued, so they need no device), the symbols and the resource use of the new kernels.  CPU only."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

import pvoc_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN, OUT, SCRATCH = 0x10000000, 0x40000000, 0x70000000     # never dereferenced: every call below is refused or asks for a size only


def valid_args(jsg, **kw):
    n, T, rate = 1024, 300, 0.8
    K = n // 2 + 1
    a = dict(in_=IN, in_frame_pitch=K, in_row_pitch=T * K, rows=2, n=n, hop=256, n_frames_in=T, rate=rate, out=OUT,
             out_frame_pitch=K, out_row_pitch=pr.n_frames_out(T, rate) * K, n_frames_out=pr.n_frames_out(T, rate), chunk_frames=0)
    a.update(kw)
    return jsg.capi.PvocArgs(**a)


@pytest.mark.parametrize("rate", [0.5, 0.8, 1.0, 1 / 0.9, 1.3, 2.0, 1000.0])
def test_frames_match_the_definition(jsg, rate):
    for T in (1, 2, 63, 64, 65, 4097):
        want = sum(1 for i in range(2 * T + 2) if float(i) * rate < T)      # the definition, counted
        assert jsg.pvoc_frames(T, rate) == want == pr.n_frames_out(T, rate), (T, rate)


def test_frames_refusals(jsg):
    lib, bad = jsg.capi.lib(), jsg.capi.JSG_ERR_INVALID
    for T, rate in ((0, 1.0), (-5, 1.0), (1 << 31, 1.0), (10, 0.0), (10, -1.0), (10, float("nan")), (10, float("inf")),
                    (1 << 30, 0.4), (5, 1e-300)):
        assert lib.jsg_pvoc_frames(T, rate) == bad, (T, rate)
    assert lib.jsg_pvoc_frames((1 << 31) - 1, 1.0) == (1 << 31) - 1
    assert lib.jsg_pvoc_frames((1 << 30), 0.5) == bad                       # exactly 2^31 frames
    assert lib.jsg_pvoc_frames((1 << 30) - 1, 0.5) == (1 << 31) - 2


def test_valid_call_has_a_scratch_size_without_a_device(jsg):
    lib = jsg.capi.lib()
    a = valid_args(jsg)
    need = lib.jsg_pvoc_scratch_bytes(C.byref(a))
    assert need > 0 and need % 16 == 0
    for chunk in (1, 7, 64, 65536):
        a = valid_args(jsg, chunk_frames=chunk)
        chunks = -(-a.n_frames_out // chunk)
        assert lib.jsg_pvoc_scratch_bytes(C.byref(a)) == -(-(2 * chunks * 513 * 4) // 16) * 16
    # one row: the row pitches are not looked at
    assert lib.jsg_pvoc_scratch_bytes(C.byref(valid_args(jsg, rows=1, in_row_pitch=0, out_row_pitch=-1))) > 0
    # every even n in range, with any hop up to n: no transform is done here
    for n, hop in ((2, 1), (2, 2), (400, 100), (1000, 999), (65536, 65536)):
        K = n // 2 + 1
        a = valid_args(jsg, n=n, hop=hop, in_frame_pitch=K, out_frame_pitch=K, in_row_pitch=300 * K, out_row_pitch=375 * K)
        assert lib.jsg_pvoc_scratch_bytes(C.byref(a)) > 0, (n, hop)


REFUSED = {
    "null in": dict(in_=None),
    "null out": dict(out=None),
    "misaligned in": dict(in_=IN + 4),
    "misaligned out": dict(out=OUT + 4),
    "odd n": dict(n=1023),
    "n too small": dict(n=0),
    "n too large": dict(n=65538),
    "hop 0": dict(hop=0),
    "hop above n": dict(hop=1025),
    "rows 0": dict(rows=0),
    "rows 65536": dict(rows=65536),
    "rate 0": dict(rate=0.0),
    "rate negative": dict(rate=-0.8),
    "rate nan": dict(rate=float("nan")),
    "rate inf": dict(rate=float("inf")),
    "no input frames": dict(n_frames_in=0),
    "2^31 input frames": dict(n_frames_in=1 << 31),
    "too many output frames": dict(n_frames_in=1 << 30, rate=0.4, rows=1),
    "wrong n_frames_out": dict(n_frames_out=374),
    "n_frames_out one more": dict(n_frames_out=376),
    "in_frame_pitch": dict(in_frame_pitch=512),
    "out_frame_pitch": dict(out_frame_pitch=512),
    "in_row_pitch": dict(in_row_pitch=300 * 513 - 1),
    "out_row_pitch": dict(out_row_pitch=375 * 513 - 1),
    "negative chunk": dict(chunk_frames=-1),
    "chunk too long": dict(chunk_frames=65537),
    "out inside in": dict(out=IN + 8 * 513),
    "out ends inside in": dict(out=IN - 8 * 513),
    "out is in": dict(out=IN),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refusals_need_no_device(jsg, what):
    lib, bad = jsg.capi.lib(), jsg.capi.JSG_ERR_INVALID
    a = valid_args(jsg, **REFUSED[what])
    assert lib.jsg_pvoc_scratch_bytes(C.byref(a)) == bad, what
    assert lib.jsg_pvoc_launch(C.byref(a), C.c_void_p(SCRATCH), 1 << 40, None) == bad, what
    assert lib.jsg_last_error(None).startswith(b"jsg_pvoc_launch: ")


def test_scratch_refusals_and_null_arguments(jsg):
    lib, bad = jsg.capi.lib(), jsg.capi.JSG_ERR_INVALID
    a = valid_args(jsg)
    need = lib.jsg_pvoc_scratch_bytes(C.byref(a))
    assert lib.jsg_pvoc_launch(C.byref(a), None, need, None) == bad
    assert lib.jsg_pvoc_launch(C.byref(a), C.c_void_p(SCRATCH + 8), need, None) == bad
    assert b"16-byte" in lib.jsg_last_error(None)
    assert lib.jsg_pvoc_launch(C.byref(a), C.c_void_p(SCRATCH), need - 1, None) == bad
    assert lib.jsg_pvoc_launch(C.byref(a), C.c_void_p(SCRATCH), -1, None) == bad
    assert lib.jsg_pvoc_launch(None, C.c_void_p(SCRATCH), need, None) == bad
    assert lib.jsg_pvoc_scratch_bytes(None) == bad
    # adjacent buffers do not overlap
    end_of_in = IN + 8 * (300 * 513 + 299 * 513 + 513)
    assert lib.jsg_pvoc_scratch_bytes(C.byref(valid_args(jsg, out=end_of_in))) == need
    assert lib.jsg_pvoc_scratch_bytes(C.byref(valid_args(jsg, out=end_of_in - 8))) == bad


def test_no_device_no_fallback(jsg):
    lib = jsg.capi.lib()
    if lib.jsg_device_count() > 0:
        return      # with a device the launch would run on the made-up pointers; tests/test_gpu_pvoc.py launches for real
    a = valid_args(jsg)
    need = lib.jsg_pvoc_scratch_bytes(C.byref(a))
    assert lib.jsg_pvoc_launch(C.byref(a), C.c_void_p(SCRATCH), need, None) == jsg.capi.JSG_ERR_NO_DEVICE


def test_abi_stays_at_6_and_exports_the_section(jsg):
    lib = jsg.capi.lib()
    assert lib.jsg_abi_version() == 6
    for name in ("jsg_pvoc_frames", "jsg_pvoc_scratch_bytes", "jsg_pvoc_launch"):
        assert hasattr(lib, name) and name in jsg.capi.SIGNATURES
    assert C.sizeof(jsg.capi.PvocArgs) == 96
    for name in ("pvoc_frames", "phase_vocoder_launch", "phase_vocoder", "time_stretch"):
        assert callable(getattr(jsg, name))


def test_pvoc_kernels_have_no_scratch_and_no_spills(jsg):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    obj = os.path.join(ROOT, "jadespectrogram_amd", "build", "jsg_pvoc.o")
    if not os.path.exists(obj):
        from jadespectrogram_amd import _build
        _build.build_lib()
    with tempfile.TemporaryDirectory() as tmp:
        co = kernel_regs.code_object(obj, tmp)
        notes = subprocess.check_output([os.path.join(kernel_regs.LLVM, "llvm-readelf"), "--notes", co]).decode()
    blks = [b for b in re.split(r"\n\s+- \.agpr_count", notes)[1:] if any(k in b for k in ("pvoc_walk_kernel", "pvoc_scan_kernel"))]
    assert len(blks) == 3      # chunk sums, prefixes, output
    for blk in blks:
        for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            assert re.search(rf"\.{key}:\s+(\S+)", blk).group(1) == "0", key

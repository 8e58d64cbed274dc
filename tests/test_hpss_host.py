"""Harmonic-percussive separation, host side (include/jsg.h section 2f): the refusals (all decided before anything is enqueued, so
they need no device) with their messages, the scratch size, the argument blocks of the Python binding, the symbols and the resource
use of the new kernels.  CPU only."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest
import torch

from test_binding_args import FakeTensor, expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# never dereferenced: every call below is refused or asks for a size only
IN, OUT_H, OUT_P, MASK_H, MASK_P, SCRATCH = (i << 44 for i in range(1, 7))      # far enough apart for the largest call below
T, K = 300, 513


def valid_args(jsg, **kw):
    a = dict(in_=IN, in_complex=1, in_frame_pitch=K, in_row_pitch=T * K, rows=2, n_bins=K, n_frames=T, win_time=31, win_freq=31, margin_h=1.0,
             margin_p=1.0, out_h=OUT_H, out_p=OUT_P, out_frame_pitch=K, out_row_pitch=T * K, mask_h=MASK_H, mask_p=MASK_P, mask_frame_pitch=K,
             mask_row_pitch=T * K, chunk_frames=0)
    a.update(kw)
    return jsg.capi.HpssArgs(**a)


def test_valid_call_has_a_scratch_size_without_a_device(jsg):
    lib = jsg.capi.lib()
    need = lib.jsg_hpss_scratch_bytes(C.byref(valid_args(jsg)))
    assert need >= 0 and need % 16 == 0
    for chunk in (1, 7, 64, 65536):                 # never changes the result; the scratch may depend on it
        assert lib.jsg_hpss_scratch_bytes(C.byref(valid_args(jsg, chunk_frames=chunk))) >= 0
    # one row: the row pitches are not looked at
    assert lib.jsg_hpss_scratch_bytes(C.byref(valid_args(jsg, rows=1, in_row_pitch=0, out_row_pitch=-1, mask_row_pitch=-1))) >= 0
    # every odd window in range, real input, any subset of the outputs; the pitches of absent outputs are not looked at
    for w in range(1, 64, 2):
        assert lib.jsg_hpss_scratch_bytes(C.byref(valid_args(jsg, win_time=w, win_freq=64 - w))) >= 0
    assert lib.jsg_hpss_scratch_bytes(C.byref(valid_args(jsg, in_complex=0, in_=IN + 4, out_h=OUT_H + 4))) >= 0
    assert lib.jsg_hpss_scratch_bytes(C.byref(valid_args(jsg, out_h=None, out_p=None, out_frame_pitch=0, out_row_pitch=0))) >= 0
    assert lib.jsg_hpss_scratch_bytes(C.byref(valid_args(jsg, mask_h=None, mask_p=None, mask_frame_pitch=0, mask_row_pitch=0))) >= 0
    assert lib.jsg_hpss_scratch_bytes(C.byref(valid_args(jsg, out_h=None, mask_h=None, mask_p=None))) >= 0
    # the extremes of every range
    big = dict(rows=1, out_h=None, out_p=None, mask_p=None)
    assert lib.jsg_hpss_scratch_bytes(C.byref(valid_args(jsg, n_frames=(1 << 31) - 1, n_bins=1, in_frame_pitch=1, mask_frame_pitch=1, **big))) >= 0
    assert lib.jsg_hpss_scratch_bytes(C.byref(valid_args(jsg, n_frames=1, n_bins=32769, in_frame_pitch=32769, mask_frame_pitch=32769, **big))) >= 0
    assert lib.jsg_hpss_scratch_bytes(C.byref(valid_args(jsg, margin_h=1e18, margin_p=3.5))) >= 0


def test_scratch_is_monotone_in_rows_and_frames(jsg):
    lib = jsg.capi.lib()
    size = lambda rows, frames: lib.jsg_hpss_scratch_bytes(C.byref(valid_args(
        jsg, rows=rows, n_frames=frames, in_row_pitch=frames * K, out_row_pitch=frames * K, mask_row_pitch=frames * K)))
    for rows in (1, 2, 3, 8, 100):
        sizes = [size(rows, f) for f in (1, 2, 31, 63, 64, 65, 300, 4096, 100000)]
        assert all(s >= 0 for s in sizes) and sizes == sorted(sizes)
    for frames in (1, 64, 300, 4096):
        sizes = [size(r, frames) for r in (1, 2, 3, 8, 100, 65535)]
        assert all(s >= 0 for s in sizes) and sizes == sorted(sizes)


REFUSED = {
    "all four outputs null": (dict(out_h=None, out_p=None, mask_h=None, mask_p=None), "all four outputs are null"),
    "null in": (dict(in_=None), "null input pointer"),
    "even win_time": (dict(win_time=30), "win_time must be odd and in 1..63"),
    "win_time 0": (dict(win_time=0), "win_time must be odd and in 1..63"),
    "win_time negative": (dict(win_time=-31), "win_time must be odd and in 1..63"),
    "win_time 65": (dict(win_time=65), "win_time must be odd and in 1..63"),
    "even win_freq": (dict(win_freq=2), "win_freq must be odd and in 1..63"),
    "win_freq 0": (dict(win_freq=0), "win_freq must be odd and in 1..63"),
    "win_freq 65": (dict(win_freq=65), "win_freq must be odd and in 1..63"),
    "rows 0": (dict(rows=0), "rows must be in 1..65535"),
    "rows 65536": (dict(rows=65536), "rows must be in 1..65535"),
    "no bins": (dict(n_bins=0), "n_bins must be in 1..32769"),
    "32770 bins": (dict(n_bins=32770, in_frame_pitch=32770, out_frame_pitch=32770, mask_frame_pitch=32770, rows=1), "n_bins must be in 1..32769"),
    "no frames": (dict(n_frames=0), "n_frames must be in 1..2^31-1"),
    "2^31 frames": (dict(n_frames=1 << 31, rows=1), "n_frames must be in 1..2^31-1"),
    "negative chunk": (dict(chunk_frames=-1), "chunk_frames must be 0 or in 1..65536"),
    "chunk too long": (dict(chunk_frames=65537), "chunk_frames must be 0 or in 1..65536"),
    "margin_h below 1": (dict(margin_h=0.999), "margin_h must be finite and >= 1"),
    "margin_h nan": (dict(margin_h=float("nan")), "margin_h must be finite and >= 1"),
    "margin_h inf": (dict(margin_h=float("inf")), "margin_h must be finite and >= 1"),
    "margin_p below 1": (dict(margin_p=0.0), "margin_p must be finite and >= 1"),
    "margin_p negative": (dict(margin_p=-2.0), "margin_p must be finite and >= 1"),
    "margin_p nan": (dict(margin_p=float("nan")), "margin_p must be finite and >= 1"),
    "in_complex 2": (dict(in_complex=2), "in_complex must be 0 or 1"),
    "in_frame_pitch": (dict(in_frame_pitch=K - 1), "in_frame_pitch smaller than n_bins"),
    "out_frame_pitch": (dict(out_frame_pitch=K - 1), "out_frame_pitch smaller than n_bins"),
    "mask_frame_pitch": (dict(mask_frame_pitch=K - 1), "mask_frame_pitch smaller than n_bins"),
    "in_row_pitch": (dict(in_row_pitch=T * K - 1), "in_row_pitch smaller than one row of frames"),
    "out_row_pitch": (dict(out_row_pitch=T * K - 1), "out_row_pitch smaller than one row of frames"),
    "mask_row_pitch": (dict(mask_row_pitch=T * K - 1), "mask_row_pitch smaller than one row of frames"),
    "misaligned in": (dict(in_=IN + 4), "in, out_h and out_p must be 8-byte aligned (complex float pairs)"),
    "misaligned out_h": (dict(out_h=OUT_H + 4), "in, out_h and out_p must be 8-byte aligned (complex float pairs)"),
    "misaligned out_p": (dict(out_p=OUT_P + 4), "in, out_h and out_p must be 8-byte aligned (complex float pairs)"),
    "misaligned real in": (dict(in_complex=0, in_=IN + 2), "in, out_h and out_p must be 4-byte aligned"),
    "misaligned mask_h": (dict(mask_h=MASK_H + 2), "mask_h and mask_p must be 4-byte aligned"),
    "misaligned mask_p": (dict(mask_p=MASK_P + 1), "mask_h and mask_p must be 4-byte aligned"),
    "out_h is in": (dict(out_h=IN), "out_h overlaps in"),
    "out_h inside in": (dict(out_h=IN + 8 * K), "out_h overlaps in"),
    "out_p ends inside in": (dict(out_p=IN - 8 * K), "out_p overlaps in"),
    "mask_h inside in": (dict(mask_h=IN + 4 * 2 * T * K * 2 - 4), "mask_h overlaps in"),
    "mask_p is in": (dict(mask_p=IN), "mask_p overlaps in"),
    "out_p is out_h": (dict(out_p=OUT_H), "out_p overlaps out_h"),
    "mask_h inside out_p": (dict(mask_h=OUT_P + 8), "mask_h overlaps out_p"),
    "mask_p is mask_h": (dict(mask_p=MASK_H), "mask_p overlaps mask_h"),
    "mask_p ends inside mask_h": (dict(mask_p=MASK_H - 4), "mask_p overlaps mask_h"),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refusals_need_no_device(jsg, what):
    lib, bad = jsg.capi.lib(), jsg.capi.JSG_ERR_INVALID
    change, message = REFUSED[what]
    a = valid_args(jsg, **change)
    assert lib.jsg_hpss_scratch_bytes(C.byref(a)) == bad, what
    assert lib.jsg_last_error(None) == b"jsg_hpss_scratch_bytes: " + message.encode()
    assert lib.jsg_hpss_launch(C.byref(a), C.c_void_p(SCRATCH), 1 << 40, None) == bad, what
    assert lib.jsg_last_error(None) == b"jsg_hpss_launch: " + message.encode()


def test_scratch_refusals_and_null_arguments(jsg):
    lib, bad = jsg.capi.lib(), jsg.capi.JSG_ERR_INVALID
    a = valid_args(jsg)
    need = lib.jsg_hpss_scratch_bytes(C.byref(a))
    err = lambda: lib.jsg_last_error(None)
    if need > 0:
        assert lib.jsg_hpss_launch(C.byref(a), None, need, None) == bad and err() == b"jsg_hpss_launch: null scratch"
        assert lib.jsg_hpss_launch(C.byref(a), C.c_void_p(SCRATCH), need - 1, None) == bad
        assert err() == b"jsg_hpss_launch: scratch smaller than jsg_hpss_scratch_bytes"
        assert lib.jsg_hpss_launch(C.byref(a), C.c_void_p(SCRATCH), -1, None) == bad
    assert lib.jsg_hpss_launch(C.byref(a), C.c_void_p(SCRATCH + 8), need, None) == bad
    assert err() == b"jsg_hpss_launch: scratch must be 16-byte aligned"
    assert lib.jsg_hpss_launch(None, C.c_void_p(SCRATCH), need, None) == bad and err() == b"jsg_hpss_launch: null argument"
    assert lib.jsg_hpss_scratch_bytes(None) == bad and err() == b"jsg_hpss_scratch_bytes: null argument"
    # adjacent buffers do not overlap
    end_of_in = IN + 8 * 2 * T * K
    assert lib.jsg_hpss_scratch_bytes(C.byref(valid_args(jsg, out_h=end_of_in))) == need
    assert lib.jsg_hpss_scratch_bytes(C.byref(valid_args(jsg, out_h=end_of_in - 8))) == bad
    assert lib.jsg_hpss_scratch_bytes(C.byref(valid_args(jsg, mask_p=MASK_H + 4 * 2 * T * K))) == need
    # a real input spans half the bytes
    assert lib.jsg_hpss_scratch_bytes(C.byref(valid_args(jsg, in_complex=0, out_h=IN + 4 * 2 * T * K))) == need
    assert lib.jsg_hpss_scratch_bytes(C.byref(valid_args(jsg, in_complex=0, out_h=IN + 4 * 2 * T * K - 4))) == bad


def test_no_device_no_fallback(jsg):
    lib = jsg.capi.lib()
    if lib.jsg_device_count() > 0:
        return      # with a device the launch would run on the made-up pointers; tests/test_gpu_hpss.py launches for real
    a = valid_args(jsg)
    need = lib.jsg_hpss_scratch_bytes(C.byref(a))
    assert lib.jsg_hpss_launch(C.byref(a), C.c_void_p(SCRATCH), need, None) == jsg.capi.JSG_ERR_NO_DEVICE
    # ... and only after the argument checks
    assert lib.jsg_hpss_launch(C.byref(valid_args(jsg, win_time=30)), C.c_void_p(SCRATCH), need, None) == jsg.capi.JSG_ERR_INVALID


def test_abi_stays_at_6_and_exports_the_section(jsg):
    lib = jsg.capi.lib()
    assert lib.jsg_abi_version() == 6
    for name in ("jsg_hpss_scratch_bytes", "jsg_hpss_launch"):
        assert hasattr(lib, name) and name in jsg.capi.SIGNATURES
    assert C.sizeof(jsg.capi.HpssArgs) == 136 and jsg.capi.HPSS_MAX_WINDOW == 63
    header = open(os.path.join(ROOT, "include", "jsg.h")).read()
    assert "#define JSG_HPSS_MAX_WINDOW 63" in header and "#define JSG_ABI_VERSION 6 " in header
    for name in ("hpss_scratch_bytes", "hpss_launch", "hpss", "hpss_audio"):
        assert callable(getattr(jsg, name)) and name in jsg.__all__


def test_hpss_args(jsg):
    S = jsg.spectrogram
    X = FakeTensor((3, 14, 513), torch.complex64, strides=(14 * 520, 520, 1), ptr=0x7F0000900000)
    Hm = FakeTensor((3, 14, 513), torch.complex64, strides=(14 * 576, 576, 1), ptr=0x7F0000B00000)
    Pc = FakeTensor((3, 14, 513), torch.complex64, strides=(14 * 576, 576, 1), ptr=0x7F0000C00000)
    Mh = FakeTensor((3, 14, 513), torch.float32, strides=(14 * 640, 640, 1), ptr=0x7F0000D00000)
    Mp = FakeTensor((3, 14, 513), torch.float32, strides=(14 * 640, 640, 1), ptr=0x7F0000E00000)
    base = dict(in_=X.data_ptr(), in_complex=1, in_frame_pitch=520, in_row_pitch=14 * 520, rows=3, n_bins=513, n_frames=14, win_time=31, win_freq=31,
                margin_h=1.0, margin_p=1.0)
    outs = dict(out_h=Hm.data_ptr(), out_p=Pc.data_ptr(), out_frame_pitch=576, out_row_pitch=14 * 576)
    masks = dict(mask_h=Mh.data_ptr(), mask_p=Mp.data_ptr(), mask_frame_pitch=640, mask_row_pitch=14 * 640)
    expect(S._hpss_args(X, Hm, Pc, Mh, Mp, 31, 1.0, 0), **base, **outs, **masks)
    # pairs are (harmonic / time, percussive / frequency); absent outputs are null with pitches of zero
    expect(S._hpss_args(X, Hm, None, None, Mp, (17, 9), (2.0, 3.5), 64),
           **dict(base, win_time=17, win_freq=9, margin_h=2.0, margin_p=3.5, chunk_frames=64, out_h=Hm.data_ptr(), out_frame_pitch=576,
                  out_row_pitch=14 * 576, mask_p=Mp.data_ptr(), mask_frame_pitch=640, mask_row_pitch=14 * 640))
    expect(S._hpss_args(X, None, Pc, None, None, 5, 1.0, 0), **dict(base, win_time=5, win_freq=5, out_p=Pc.data_ptr(), out_frame_pitch=576,
                                                                 out_row_pitch=14 * 576))
    # one row: two-dimensional tensors
    expect(S._hpss_args(X[2], None, None, Mh[2], None, 31, 1.0, 0),
           **dict(base, in_=X.data_ptr() + 2 * 14 * 520 * 8, rows=1, mask_h=Mh.data_ptr() + 2 * 14 * 640 * 4, mask_frame_pitch=640, mask_row_pitch=14 * 640))
    # float32 input is power: real outputs
    Pw = FakeTensor((3, 14, 513), torch.float32, strides=(14 * 520, 520, 1), ptr=0x7F0000900000)
    Ho = FakeTensor((3, 14, 513), torch.float32, ptr=0x7F0000B00000)
    expect(S._hpss_args(Pw, Ho, None, Mh, Mp, 31, 1.0, 0),
           **dict(base, in_complex=0, out_h=Ho.data_ptr(), out_frame_pitch=513, out_row_pitch=14 * 513), **masks)
    bad = [(X, Ho, None, None, None),                                                  # the outputs have the input's kind
           (Pw, Hm, None, None, None),
           (X, None, None, Hm, None),                                                  # masks are float32
           (X, FakeTensor((3, 13, 513), torch.complex64), None, None, None),          # and the input's shape
           (X, FakeTensor((2, 14, 513), torch.complex64), None, None, None),
           (X, Hm, FakeTensor((3, 14, 513), torch.complex64), None, None),            # the two outputs share their pitches
           (X, None, None, Mh, FakeTensor((3, 14, 513), torch.float32)),
           (X, FakeTensor((3, 14, 513), torch.complex64, strides=(1, 3, 42)), None, None, None),
           (FakeTensor((3, 14, 513), torch.float64), None, None, Mh, None),
           (FakeTensor((3, 14, 513), torch.complex64, is_cuda=False), None, None, Mh, None),
           (X[0][0], None, None, Mh, None)]
    for d_in, h, p, mh, mp in bad:
        with pytest.raises(AssertionError):
            S._hpss_args(d_in, h, p, mh, mp, 31, 1.0, 0)
    with pytest.raises(AssertionError):
        S._hpss_args(X, Hm, None, None, None, (31, 31, 31), 1.0, 0)


def test_hpss_scratch_bytes_through_the_binding(jsg):
    X = FakeTensor((3, 14, 513), torch.complex64, ptr=0x7F0000900000)
    Mh = FakeTensor((3, 14, 513), torch.float32, ptr=0x7F0000D00000)
    a = jsg.spectrogram._hpss_args(X, None, None, Mh, None, 31, 1.0, 0)
    assert jsg.hpss_scratch_bytes(X, d_mask_h=Mh) == jsg.capi.lib().jsg_hpss_scratch_bytes(C.byref(a)) >= 0
    with pytest.raises(jsg.JsgError) as e:
        jsg.hpss_scratch_bytes(X, d_mask_h=Mh, kernel_size=(31, 30))
    assert e.value.code == jsg.capi.JSG_ERR_INVALID and "win_freq must be odd" in str(e.value)
    with pytest.raises(jsg.JsgError):
        jsg.hpss_scratch_bytes(X)


def test_hpss_kernels_have_no_scratch_and_no_spills(jsg):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    obj = os.path.join(ROOT, "jadespectrogram_amd", "build", "jsg_hpss.o")
    if not os.path.exists(obj):
        from jadespectrogram_amd import _build
        _build.build_lib()
    with tempfile.TemporaryDirectory() as tmp:
        co = kernel_regs.code_object(obj, tmp)
        notes = subprocess.check_output([os.path.join(kernel_regs.LLVM, "llvm-readelf"), "--notes", co]).decode()
    blks = [b for b in re.split(r"\n\s+- \.agpr_count", notes)[1:] if any(k in b for k in ("hpss_freq_kernel", "hpss_time_kernel"))]
    assert len(blks) == 8      # two passes x (any window, 31) x (complex, real power)
    for blk in blks:
        for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            assert re.search(rf"\.{key}:\s+(\S+)", blk).group(1) == "0", key

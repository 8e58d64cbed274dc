"""Complex STFT / inverse STFT, host side (include/jsg.h section 2d): the NOLA check against a float64 numpy envelope, the refusals
that need no device, the symbols and the resource use of the new kernels (no spills, no scratch).  CPU only."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def interior_min(w, hop):
    w2 = w.astype(np.float64) ** 2
    return min(float(w2[rho::hop].sum()) for rho in range(hop))


def test_nola_known_cases(jsg):
    hann = jsg.window(jsg.capi.WIN_HANN, 1024)
    ok, mn = jsg.istft_nola(1024, 512, hann)
    assert ok and mn > 0.1
    ok, mn = jsg.istft_nola(1024, 1024, np.ones(1024, np.float32))
    assert ok and mn == 1.0
    ok, mn = jsg.istft_nola(1024, 1024, hann)       # the periodic Hann window starts at 0: residue 0 has no weight at hop n
    assert not ok and mn == 0.0
    v = C.c_float()
    assert jsg.capi.lib().jsg_istft_nola(1024, 1024, hann.ctypes.data, C.byref(v)) == jsg.capi.JSG_ERR_INVALID


@pytest.mark.parametrize("n", [512, 1024, 2048, 4096, 8192])
@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4, 5])
def test_nola_minimum_matches_float64(jsg, n, kind):
    w = jsg.window(kind, n)
    for hop in (1, 7, n // 4, 441, 480, n // 2, n - 1, n):
        if hop > n:
            continue
        ok, mn = jsg.istft_nola(n, hop, w)
        want = interior_min(w, hop)
        assert mn == np.float32(want), (n, kind, hop, mn, want)
        assert ok == (want > 1e-11)


def test_nola_refuses_bad_arguments(jsg):
    lib, v = jsg.capi.lib(), C.c_float()
    w = np.ones(1024, np.float32)
    assert lib.jsg_istft_nola(1024, 0, w.ctypes.data, C.byref(v)) == jsg.capi.JSG_ERR_INVALID
    assert lib.jsg_istft_nola(1024, 1025, w.ctypes.data, C.byref(v)) == jsg.capi.JSG_ERR_INVALID
    assert lib.jsg_istft_nola(1000, 250, w.ctypes.data, C.byref(v)) == jsg.capi.JSG_ERR_UNSUPPORTED
    assert lib.jsg_istft_nola(16384, 250, np.ones(16384, np.float32).ctypes.data, C.byref(v)) == jsg.capi.JSG_ERR_UNSUPPORTED
    assert lib.jsg_istft_nola(1024, 256, None, C.byref(v)) == jsg.capi.JSG_ERR_INVALID
    bad = w.copy()
    bad[3] = np.nan
    assert lib.jsg_istft_nola(1024, 256, bad.ctypes.data, C.byref(v)) == jsg.capi.JSG_ERR_INVALID


def test_plan_refusals_before_any_device(jsg):
    lib, p = jsg.capi.lib(), C.c_void_p()
    w = np.ones(8192 * 2, np.float32)
    for n in (256, 1000, 16384):
        assert lib.jsg_cstft_create(C.byref(p), n, w.ctypes.data) == jsg.capi.JSG_ERR_UNSUPPORTED
        assert not p
    assert lib.jsg_cstft_create(C.byref(p), 1024, None) == jsg.capi.JSG_ERR_INVALID
    bad = np.ones(1024, np.float32)
    bad[100] = np.inf
    assert lib.jsg_cstft_create(C.byref(p), 1024, bad.ctypes.data) == jsg.capi.JSG_ERR_INVALID
    assert lib.jsg_cstft_create(None, 1024, w.ctypes.data) == jsg.capi.JSG_ERR_INVALID
    # null plans / arguments are refused by every entry point
    a = jsg.capi.CstftArgs()
    assert lib.jsg_cstft_launch(None, C.byref(a), None) == jsg.capi.JSG_ERR_INVALID
    ia = jsg.capi.IstftArgs()
    assert lib.jsg_istft_launch(None, C.byref(ia), None, 0, None) == jsg.capi.JSG_ERR_INVALID
    assert lib.jsg_istft_scratch_floats(None, C.byref(ia)) == jsg.capi.JSG_ERR_INVALID
    assert lib.jsg_cstft_fft_size(None) == jsg.capi.JSG_ERR_INVALID
    assert lib.jsg_cstft_destroy(None) == jsg.capi.JSG_OK
    assert b"null" in lib.jsg_last_error(None)


def test_no_device_no_fallback(jsg):
    """Without a GPU the plan (and so every compute entry point) is refused with JSG_ERR_NO_DEVICE: nothing runs on the host."""
    lib, p = jsg.capi.lib(), C.c_void_p()
    w = jsg.window(jsg.capi.WIN_HANN, 1024)
    rc = lib.jsg_cstft_create(C.byref(p), 1024, w.ctypes.data)
    if lib.jsg_device_count() > 0:
        assert rc == jsg.capi.JSG_OK and p and lib.jsg_cstft_fft_size(p) == 1024
        lib.jsg_cstft_destroy(p)
        return
    assert rc == jsg.capi.JSG_ERR_NO_DEVICE and not p
    with pytest.raises(jsg.JsgError) as ei:
        jsg.CStftPlan(1024, w)
    assert ei.value.code == jsg.capi.JSG_ERR_NO_DEVICE


def test_abi_stays_at_6_and_exports_the_section(jsg):
    lib = jsg.capi.lib()
    assert lib.jsg_abi_version() == 6
    for name in ("jsg_cstft_create", "jsg_cstft_destroy", "jsg_cstft_fft_size", "jsg_cstft_launch", "jsg_istft_nola", "jsg_istft_launch",
                 "jsg_istft_scratch_floats"):
        assert hasattr(lib, name)
    assert C.sizeof(jsg.capi.CstftArgs) == 64 and C.sizeof(jsg.capi.IstftArgs) == 64


def test_cstft_kernels_have_no_scratch_and_no_spills(jsg):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    obj = os.path.join(ROOT, "jadespectrogram_amd", "build", "jsg_cstft.o")
    if not os.path.exists(obj):
        from jadespectrogram_amd import _build
        _build.build_lib()
    with tempfile.TemporaryDirectory() as tmp:
        co = kernel_regs.code_object(obj, tmp)
        notes = subprocess.check_output([os.path.join(kernel_regs.LLVM, "llvm-readelf"), "--notes", co]).decode()
    blks = [b for b in re.split(r"\n\s+- \.agpr_count", notes)[1:]
            if any(k in b for k in ("cstft_fwd_kernel", "istft_c2r_kernel", "istft_ola_kernel"))]
    assert len(blks) == 11     # forward and c2r for five sizes, one overlap-add kernel
    for blk in blks:
        for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            assert re.search(rf"\.{key}:\s+(\S+)", blk).group(1) == "0", key

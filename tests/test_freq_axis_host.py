"""Display frequency axes on the host (include/jsg.h, section 2c): jsg_freq_axis_build against an independent float64 computation, the
partition of the bin axis, the identity axis, the geometric centres of a LOG axis, every refusal, and the C++ drop-in's new methods."""
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f32(x):
    return float(np.float32(x))


def _slaney_mel(f):
    step = math.log(6.4) / 27.0
    return f / (200.0 / 3.0) if f < 1000.0 else 15.0 + math.log(f / 1000.0) / step


def _slaney_hz(m):
    step = math.log(6.4) / 27.0
    return (200.0 / 3.0) * m if m < 15.0 else 1000.0 * math.exp(step * (m - 15.0))


def model_rows(n, fs, scale, H, fmin, fmax):
    """The row table of section 2c in float64, written from the contract; also returns the bounds b_j (in bins)."""
    from jadespectrogram_amd import capi
    fs, fmin, fmax = _f32(fs), _f32(fmin), _f32(fmax)
    w, wi = {capi.AXIS_LINEAR: (lambda f: f, lambda u: u), capi.AXIS_LOG: (math.log, math.exp),
             capi.AXIS_MEL: (_slaney_mel, _slaney_hz)}[scale]
    u0 = w(fmin)
    du = (w(fmax) - u0) / (H - 1)
    b = np.array([wi(u0 + (j - 0.5) * du) * n / fs for j in range(H + 1)])
    first, count, t, centre = (np.zeros(H, np.int64), np.zeros(H, np.int64), np.zeros(H, np.float32), np.zeros(H, np.float32))
    for r in range(H):
        c = wi(u0 + r * du)
        centre[r] = c
        ks = [k for k in range(max(0, math.ceil(b[r])), min(n // 2, math.ceil(b[r + 1])) + 1) if b[r] <= k < b[r + 1]]
        if ks:
            first[r], count[r] = ks[0], len(ks)
        else:
            x = c * n / fs
            k = min(math.floor(x), n // 2 - 1)
            first[r], t[r] = k, np.float32(x - k)
    return first, count, t, centre, b


SPECS = []
for _n in (512, 1024, 2048, 4096, 8192):
    for _scale, _lo, _hi in ((1, 0.0, 24000.0), (1, 0.0, 4000.0), (1, 1234.5, 1800.0), (2, 20.0, 20000.0), (2, 1.0, 24000.0),
                             (3, 0.0, 24000.0), (3, 300.0, 8000.0)):
        for _H in (2, 37, 256, 1080, _n // 2 + 1):
            SPECS.append((_n, 48000.0, _scale, _H, _lo, _hi))
SPECS += [(4096, 44100.0, 2, 4 * 2049, 30.0, 22050.0), (1024, 96000.0, 3, 700, 50.0, 47000.0), (2048, 22050.0, 1, 16384, 100.0, 200.0)]


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: "n%d-fs%g-s%d-H%d-%g-%g" % s)
def test_table_matches_float64_model(jsg, spec):
    n, fs, scale, H, lo, hi = spec
    ax = jsg.FreqAxis(n, fs, H, lo, hi, scale)
    first, count, t, centre = ax.rows()
    mf, mc, mt, mcen, b = model_rows(n, fs, scale, H, lo, hi)
    near = np.abs(b - np.round(b)) < 1e-9                     # a bound within 1e-9 of an integer may land on either side
    free = near[:-1] | near[1:]
    ok = ~free
    assert (first[ok] == mf[ok]).all() and (count[ok] == mc[ok]).all()
    assert (t[ok] == mt[ok]).all()
    assert np.array_equal(centre, mcen)
    # interpolated rows: t in [0, 1], k and k+1 inside the spectrum
    z = count == 0
    assert ((t[z] >= 0) & (t[z] <= 1)).all() and (first[z] >= 0).all() and (first[z] + 1 <= n // 2).all()
    assert (t[~z] == 0).all()


@pytest.mark.parametrize("spec", SPECS[::3], ids=lambda s: "n%d-fs%g-s%d-H%d-%g-%g" % s)
def test_rows_partition_the_bins_in_order(jsg, spec):
    n, fs, scale, H, lo, hi = spec
    first, count, t, centre = jsg.FreqAxis(n, fs, H, lo, hi, scale).rows()
    red = count > 0
    starts, ends = first[red], first[red] + count[red]
    assert (starts[1:] == ends[:-1]).all(), "the reduced rows must follow each other without gap or overlap"
    assert (ends <= n // 2 + 1).all() and (starts >= 0).all()
    if lo == 0.0 and hi == fs / 2:
        assert starts[0] == 0 and ends[-1] == n // 2 + 1, "a full-range axis covers every bin"
    # interpolated rows sit between the reduced rows around them
    assert (np.diff(centre.astype(np.float64)) > 0).all()


@pytest.mark.parametrize("n", [512, 1024, 2048, 4096, 8192])
@pytest.mark.parametrize("fs", [44100.0, 48000.0, 96000.0])
def test_identity_axis_is_one_bin_per_row(jsg, n, fs):
    first, count, t, centre = jsg.FreqAxis(n, fs, n // 2 + 1, 0.0, fs / 2, jsg.capi.AXIS_LINEAR).rows()
    assert (first == np.arange(n // 2 + 1)).all() and (count == 1).all() and (t == 0).all()
    assert np.allclose(centre, np.arange(n // 2 + 1) * fs / n, rtol=1e-6)


@pytest.mark.parametrize("H", [2, 37, 1080, 4097])
def test_log_centres_are_geometric_and_inside_the_range(jsg, H):
    lo, hi = 20.0, 20000.0
    c = jsg.FreqAxis(4096, 48000.0, H, lo, hi, jsg.capi.AXIS_LOG).rows()[3].astype(np.float64)
    assert c[0] == np.float32(lo) and c[-1] == np.float32(hi)
    ratio = (hi / lo) ** (1.0 / (H - 1))
    assert np.allclose(c[1:] / c[:-1], ratio, rtol=2e-6)
    for scale in (jsg.capi.AXIS_LINEAR, jsg.capi.AXIS_MEL):
        c = jsg.FreqAxis(4096, 48000.0, H, lo, hi, scale).rows()[3]
        assert (c >= np.float32(lo)).all() and (c <= np.float32(hi)).all()


def test_mel_centres_follow_slaney(jsg):
    c = jsg.FreqAxis(2048, 48000.0, 128, 0.0, 8000.0, jsg.capi.AXIS_MEL).rows()[3].astype(np.float64)
    m = np.array([_slaney_mel(f) for f in c])
    assert np.allclose(np.diff(m), (_slaney_mel(8000.0)) / 127, rtol=1e-5)


REFUSED = [
    (256, 48000.0, 1, 100, 0.0, 1000.0), (16384, 48000.0, 1, 100, 0.0, 1000.0), (1000, 48000.0, 1, 100, 0.0, 1000.0),
    (1024, 0.0, 1, 100, 0.0, 1000.0), (1024, -48000.0, 1, 100, 0.0, 1000.0), (1024, float("nan"), 1, 100, 0.0, 1000.0),
    (1024, float("inf"), 1, 100, 0.0, 1000.0),
    (1024, 48000.0, 0, 100, 0.0, 1000.0), (1024, 48000.0, 4, 100, 0.0, 1000.0), (1024, 48000.0, -1, 100, 0.0, 1000.0),
    (1024, 48000.0, 1, 1, 0.0, 1000.0), (1024, 48000.0, 1, 0, 0.0, 1000.0), (1024, 48000.0, 1, 16385, 0.0, 1000.0),
    (1024, 48000.0, 1, 100, -1.0, 1000.0), (1024, 48000.0, 1, 100, 0.0, 24000.5), (1024, 48000.0, 1, 100, 1000.0, 1000.0),
    (1024, 48000.0, 1, 100, 2000.0, 1000.0), (1024, 48000.0, 2, 100, 0.0, 1000.0), (1024, 48000.0, 1, 100, float("nan"), 1000.0),
    (1024, 48000.0, 1, 100, 0.0, float("nan")), (1024, 48000.0, 3, 100, 0.0, float("inf")),
]


@pytest.mark.parametrize("spec", REFUSED, ids=lambda s: "n%d-fs%g-s%d-H%d-%g-%g" % s)
def test_refusals(jsg, spec):
    with pytest.raises(jsg.JsgError) as e:
        jsg.FreqAxis(*spec[:2], spec[3], spec[4], spec[5], spec[2])
    assert e.value.code == jsg.capi.JSG_ERR_INVALID


def test_default_axis_is_valid(jsg):
    first, count, t, centre = jsg.FreqAxis(1024, 48000.0, 300).rows()
    assert centre[0] == 0.0 and centre[-1] == 24000.0 and count.sum() == 513


def test_axis_kernel_has_no_scratch_and_no_spills(jsg):
    import re
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    obj = os.path.join(ROOT, "jadespectrogram_amd", "build", "jsg_display_axis.o")
    if not os.path.exists(obj):
        from jadespectrogram_amd import _build
        _build.build_lib()
    with tempfile.TemporaryDirectory() as tmp:
        co = kernel_regs.code_object(obj, tmp)
        notes = subprocess.check_output([os.path.join(kernel_regs.LLVM, "llvm-readelf"), "--notes", co]).decode()
    blk = [b for b in re.split(r"\n\s+- \.agpr_count", notes)[1:] if "colormap_axis_kernel" in b]
    assert len(blk) == 1
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        assert re.search(rf"\.{key}:\s+(\S+)", blk[0]).group(1) == "0", key


def test_edges_are_accepted(jsg):
    jsg.FreqAxis(512, 48000.0, 2, 0.0, 24000.0, jsg.capi.AXIS_LINEAR)
    jsg.FreqAxis(8192, 48000.0, 16384, 1e-3, 24000.0, jsg.capi.AXIS_LOG)


def test_null_outputs_are_refused(jsg):
    import ctypes as C
    s = jsg.capi.AxisSpec(1024, 48000.0, jsg.capi.AXIS_LOG, 100, 20.0, 20000.0)
    a = np.zeros(100, np.int32)
    rc = jsg.capi.lib().jsg_freq_axis_build(C.byref(s), None, a.ctypes.data, a.ctypes.data, a.ctypes.data)
    assert rc == jsg.capi.JSG_ERR_INVALID
    assert jsg.capi.lib().jsg_freq_axis_build(None, a.ctypes.data, a.ctypes.data, a.ctypes.data, a.ctypes.data) == jsg.capi.JSG_ERR_INVALID


def build_cpp_driver(jsg):
    exe = os.path.join(tempfile.gettempdir(), "jsg_display_axis_test")
    src = os.path.join(ROOT, "tests", "cpp", "display_axis_test.cpp")
    libdir = os.path.dirname(jsg.capi.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
           "-L", libdir, "-ljsg", f"-Wl,-rpath,{libdir}"]
    subprocess.check_call(cmd)
    return exe


def test_cpp_display_axis_methods_compile_and_link(jsg):
    exe = build_cpp_driver(jsg)
    assert subprocess.call([exe]) == 2   # without arguments: usage code, no GPU touched

"""libjsg.so's host-side precompute (windows, geometry, colour tables) and the C-ABI surface.  CPU only:
nothing here touches a GPU; the compute entry points must refuse to run without one."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol(jsg):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "jsg.h")).read()
    declared = set(re.findall(r"\b(jsg_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 45
    lib = jsg.capi.lib()
    for name in sorted(declared):
        assert hasattr(lib, name), f"libjsg.so does not export {name}"
    assert declared == set(jsg.capi.SIGNATURES), declared ^ set(jsg.capi.SIGNATURES)
    assert lib.jsg_abi_version() == 6


STRUCTS = ("jsg_stft_args", "jsg_colormap_args", "jsg_stft_image_args", "jsg_fb_spec", "jsg_axis_spec", "jsg_cstft_args", "jsg_istft_args",
           "jsg_pvoc_args")


def test_ctypes_structs_match_the_header_layout(jsg, tmp_path):
    """capi.py restates the argument structs of include/jsg.h by hand: same fields, in the same order, at the same offsets, of the same
    sizes as the host C compiler lays them out (`in` is `in_` in Python, where `in` is a keyword)."""
    import ctypes
    import shutil
    import subprocess
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsg.h")).read(), flags=re.S)
    declared = {}
    for name in STRUCTS:
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, flags=re.S).group(1)
        declared[name] = [re.search(r"(\w+)\s*$", piece).group(1) for decl in body.split(";") if decl.strip() for piece in decl.split(",")]
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "jsg.h"', "int main(void) {"]
    for name, names in declared.items():
        lines.append(f'    printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'    printf("{f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));' for f in names]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)])
    out = iter(subprocess.check_output([str(tmp_path / "layout")], text=True).split("\n"))
    for name, names in declared.items():
        cls = getattr(jsg.capi, "".join(part.capitalize() for part in name.split("_")[1:]))      # jsg_stft_image_args -> StftImageArgs
        assert next(out) == f"{name} {ctypes.sizeof(cls)}"
        assert [f for f, _ in cls._fields_] == ["in_" if f == "in" else f for f in names], name
        for (f, _), c_name in zip(cls._fields_, names):
            assert next(out) == f"{c_name} {getattr(cls, f).offset} {getattr(cls, f).size}", (name, f)


def test_windows_bit_exact_vs_oracle(jsg, oracle):
    for kind in range(6):
        for n in (512, 1024, 2048, 4096, 8192):
            a, b = jsg.window(kind, n), oracle.window(kind, n)
            assert (a.view(np.uint32) == b.view(np.uint32)).all(), (kind, n)


def test_geometry_vs_oracle_and_kats(jsg, oracle, golden):
    for n, d in golden["kats"]["geometry_fs48000_mem10"].items():
        for pct, (hop, fb, W) in d.items():
            assert jsg.feed_samples(float(pct), int(n)) == hop
            assert jsg.memsize_blocks(10.0, 48000.0, hop) == W
    rng = np.random.default_rng(1)
    for _ in range(200):
        pct = float(rng.choice([100.0, 50.0, 25.0, 12.5, 10.0, 6.25]))
        n = int(rng.choice([512, 1024, 2048, 4096, 8192]))
        fs = float(rng.choice([44100.0, 48000.0, 96000.0, 192000.0]))
        mem = float(rng.uniform(0.05, 20.0))
        hop = jsg.feed_samples(pct, n)
        assert hop == oracle.feed_samples(pct, n)
        assert jsg.memsize_blocks(mem, fs, hop) == oracle.memsize_blocks(mem, fs, hop)
    for ms in (1.0, 5.0, 10.0, 21.3, 42.0, 100.0):
        assert jsg.next_power_of_2(ms, 48000.0) == oracle.next_power_of_2(ms, 48000.0)


def test_colormap_tables_bit_exact_vs_reference_golden(jsg, golden):
    g = golden["colormap"]
    for scheme in range(7):
        assert (jsg.colormap_lut(256, scheme) == np.array(g["lut256"][str(scheme)], dtype=np.int32)).all()
        for n in (2, 7, 64, 100, 1000):
            ref = np.array(g["lut_other"][f"{scheme}:{n}"], dtype=np.int32)
            assert (jsg.colormap_lut(n, scheme) == ref).all(), (scheme, n)


def test_colormap_range_bit_exact_vs_reference_golden(jsg, golden):
    for case in golden["colormap"]["map_cases"]:
        st = np.array(case["state_hex"], dtype=np.uint32)
        got = np.array(jsg.colormap_range(case["n_colors"], case["lo"], case["hi"]), dtype=np.float32).view(np.uint32)
        assert (got == st).all(), case["lo"]


def test_ccolorpalette_mirror(jsg, golden):
    p = jsg.CColorPalette(256, jsg.CColorPalette.kJade)
    p.setValueRange(-50.0, 50.0)
    assert abs(float(p.m_AccessMult) - golden["kats"]["colormap_range_m50_p50"]["access_mult"]) < 1e-7
    p.setColorSceme(4)
    assert (p.m_Color == np.array(golden["colormap"]["switch_scheme"]["6->4"], dtype=np.int32)).all()


def test_bad_arguments_are_rejected(jsg):
    lib = jsg.capi.lib()
    assert lib.jsg_window_build(9, 1024, np.zeros(1024, np.float32).ctypes.data) == jsg.capi.JSG_ERR_INVALID
    assert lib.jsg_colormap_build(256, 7, np.zeros(256, np.int32).ctypes.data) == jsg.capi.JSG_ERR_INVALID
    assert lib.jsg_feed_samples(50.0, 0) == jsg.capi.JSG_ERR_INVALID
    # the round-3 entry points refuse null / malformed arguments with a code (nothing fatal crosses the C boundary, no GPU needed)
    import ctypes as C
    cap = jsg.capi
    a = cap.StftArgs()
    buf = C.create_string_buffer(32)
    assert lib.jsg_stft_kernel_name(None, C.byref(a), buf, 32) == cap.JSG_ERR_INVALID
    assert lib.jsg_stft_db_launch_batches(None, C.byref(a), 2, None) == cap.JSG_ERR_INVALID
    assert lib.jsg_stft_db_launch_batches(None, None, 0, None) == cap.JSG_ERR_INVALID      # a plan is required even for an empty list
    assert lib.jsg_stft_db_launch_many_threads(None, C.byref(a), 1, None, 0, 2) == cap.JSG_ERR_INVALID
    ia = cap.StftImageArgs()
    assert lib.jsg_stft_image_needs_scratch(None, C.byref(ia)) == cap.JSG_ERR_INVALID
    assert lib.jsg_stft_image_launch(None, C.byref(ia), None) == cap.JSG_ERR_INVALID
    assert lib.jsg_stft_image_strided_needs_scratch(None, C.byref(ia), 2) == cap.JSG_ERR_INVALID
    assert lib.jsg_stft_image_launch_strided(None, C.byref(ia), 2, 0, 0, None) == cap.JSG_ERR_INVALID
    msg = lib.jsg_last_error(None)
    assert msg and b"null" in msg
    # round 4
    assert lib.jsg_stft_db_launch_strided(None, C.byref(a), 2, 0, 0, None) == cap.JSG_ERR_INVALID
    assert lib.jsg_stft_db_strided_kernel_name(None, C.byref(a), 2, 0, buf, 32) == cap.JSG_ERR_INVALID
    assert lib.jsg_calib_copy_launch(None, None, 16, None) == cap.JSG_ERR_INVALID
    assert lib.jsg_calib_copy_launch(C.c_void_p(16), C.c_void_p(32), 24, None) == cap.JSG_ERR_INVALID     # not a multiple of 16 bytes
    assert lib.jsg_process_block_n(None, None, 2, 1024) == cap.JSG_ERR_INVALID
    assert lib.jsg_get_dropped_blocks(None) == cap.JSG_ERR_INVALID
    # colour loop: an image pitch of 0, negative, or smaller than the image width would be out-of-bounds device writes
    ca = cap.ColormapArgs()
    ca.db, ca.lut, ca.argb_out = 256, 256, 256                      # (non-null dummies: the checks come before anything is dereferenced)
    ca.height, ca.ring_width, ca.n_cols, ca.x_wrap, ca.n_colors = 513, 100, 10, 100, 256
    for pitch in (0, -8, 99):
        ca.argb_pitch = pitch
        assert lib.jsg_colormap_launch(C.byref(ca), None) == cap.JSG_ERR_INVALID, pitch


def test_only_the_c_abi_is_exported(jsg):
    """libjsg.so is built with -fvisibility=hidden: every exported FUNCTION is a jsg_* entry point of include/jsg.h (VERDICT r3, weak 8:
    jsg::launch_Cfg*, jsg::touch_module_* used to be visible)."""
    import shutil, subprocess
    if not shutil.which("nm"):
        import pytest
        pytest.skip("nm not available")
    out = subprocess.check_output(["nm", "-D", "--defined-only", jsg.capi.LIB_PATH]).decode()
    funcs = [l.split()[-1] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T"]
    assert funcs and all(f.startswith("jsg_") for f in funcs), [f for f in funcs if not f.startswith("jsg_")][:5]
    assert set(funcs) == set(jsg.capi.SIGNATURES)
    assert "launch_Cfg" not in out and "touch_module" not in out


def test_no_cpu_fallback(jsg):
    """Without a GPU the engine must refuse loudly, not compute on the host."""
    import pytest
    if jsg.capi.lib().jsg_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(jsg.JsgError) as ei:
        jsg.Spectrogram(2)
    assert ei.value.code == jsg.capi.JSG_ERR_NO_DEVICE
    with pytest.raises(jsg.JsgError):
        jsg.Plan(1024, jsg.window(1, 1024))


def test_display_freq_rows_vs_oracle(jsg, oracle):
    from jadespectrogram_amd.spectrogram import display_freq_rows
    rng = np.random.default_rng(5)
    cases = [(48000.0, 1025, 1.0, 20000.0), (48000.0, 1025, 0.0, 24000.0), (44100.0, 513, 30000.0, 40000.0),
             (96000.0, 2049, 5000.0, 100.0), (48000.0, 1025, 1000.0, 1000.0)]
    for _ in range(300):
        cases.append((float(rng.choice([44100.0, 48000.0, 96000.0])), int(rng.choice([257, 513, 1025, 2049, 4097])),
                      float(np.exp(rng.uniform(0.0, np.log(10000.0)))), float(np.exp(rng.uniform(np.log(500.0), np.log(20000.0))))))
    for c in cases:
        assert display_freq_rows(*c) == oracle.display_freq_rows(*c), c
    # the plugin's defaults: full band at 48 kHz, H = 1025 -> rows [0, 854): everything up to 20 kHz
    assert display_freq_rows(48000.0, 1025, 1.0, 20000.0) == (0, 854, 854, 171)


def test_colormap_range_fuzz_vs_oracle(jsg, oracle):
    """setValueRange (CColorpalette.cpp:39-54) for arbitrary slider positions: swapped, equal, tiny and huge ranges.
    The oracle's arithmetic is pinned by the reference-built golden cases above; here the library follows it bit for bit."""
    from hypothesis import given, settings, strategies as st
    finite = st.floats(min_value=-1e6, max_value=1e6, allow_nan=False, allow_infinity=False, width=32)

    @settings(max_examples=300, deadline=None)
    @given(lo=finite, hi=finite, n=st.integers(min_value=2, max_value=4096), same=st.booleans())
    def check(lo, hi, n, same):
        if same:
            hi = lo
        if lo == hi == 0.0:
            return   # Min = 0.99*Max = Max: the reference divides by zero here (undefined), not part of the contract
        p = oracle.OracleColorPalette(n, oracle.CM_JADE)
        p.set_value_range(lo, hi)
        want = np.array([p.vmin, p.vmax, p.mult], dtype=np.float32).view(np.uint32)
        got = np.array(jsg.colormap_range(n, lo, hi), dtype=np.float32).view(np.uint32)
        assert (got == want).all(), (lo, hi, n)

    check()


def test_geometry_fuzz_vs_oracle(jsg, oracle):
    """hop, ring width and fft-size-from-milliseconds for arbitrary (not only the GUI's) parameter values."""
    from hypothesis import given, settings, strategies as st

    @settings(max_examples=300, deadline=None)
    @given(pct=st.floats(min_value=1.0, max_value=100.0), n=st.sampled_from([512, 1024, 2048, 4096, 8192]),
           fs=st.floats(min_value=8000.0, max_value=384000.0), mem=st.floats(min_value=0.01, max_value=60.0),
           ms=st.floats(min_value=0.5, max_value=200.0))
    def check(pct, n, fs, mem, ms):
        pct, fs, mem, ms = (float(np.float32(v)) for v in (pct, fs, mem, ms))   # the C-ABI takes floats
        hop = jsg.feed_samples(pct, n)
        assert hop == oracle.feed_samples(pct, n)
        if hop > 0:
            assert jsg.memsize_blocks(mem, fs, hop) == oracle.memsize_blocks(mem, fs, hop)
        assert jsg.next_power_of_2(ms, fs) == oracle.next_power_of_2(ms, fs)

    check()


def test_colormap_tables_against_the_reference_build_itself(jsg):
    """The product's tables against the reference's CColorpalette.cpp compiled as it lies (oracle/Makefile target `ref`):
    its tables are recorded in tests/golden/colormap_ref_tables.json (oracle/gen_golden.py), and where build() has made
    oracle/_ref the library is also called live.  This is the check of the two perceptual schemes at 256 colours that does
    not lean on tests/golden/colormap_ref.json, from which their embedded table (csrc/jsg_colormap_tables.inc) was
    generated.  Reference: CColorpalette.cpp:106-339 (Viridis :254-271, Plasma :272-289)."""
    import ctypes
    import json
    sizes = (256, 2, 3, 7, 64, 100, 255, 257, 512, 1000)
    with open(os.path.join(ROOT, "tests", "golden", "colormap_ref_tables.json")) as fh:
        recorded = json.load(fh)["lut"]
    so = os.path.join(ROOT, "oracle", "_ref", "libjade_colorpalette_ref.so")
    ref = None
    if os.path.exists(so):
        ref = ctypes.CDLL(so)
        ref.ref_cp_lut.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    for scheme in range(7):
        for n in sizes:
            want = np.array(recorded[f"{scheme}:{n}"], dtype=np.int32)
            assert want.shape == (n,), (scheme, n)
            assert (jsg.colormap_lut(n, scheme) == want).all(), (scheme, n)
            if ref is not None:
                live = np.zeros(n, dtype=np.int32)
                ref.ref_cp_lut(n, scheme, live.ctypes.data)
                assert (live == want).all(), (scheme, n)


def test_colormap_tables_match_the_survey_hashes(jsg, oracle, golden):
    """A second record that is independent of colormap_ref.json: the FNV-1a-32 hashes of the seven 256-colour tables that the
    survey took from its own run of the reference build (tests/golden/survey_kats.json)."""
    for scheme, h in golden["kats"]["colormap_fnv1a32_lut256"].items():
        lut = jsg.colormap_lut(256, int(scheme))
        assert "%08x" % oracle.fnv1a32(lut.astype("<i4").tobytes()) == h, scheme

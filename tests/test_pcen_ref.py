"""The numpy restatement of include/jsgx.h section 13 (tests/pcen_ref.py) on its own: the float32 definition against the float64 route
through scipy.signal.lfilter and numpy powers that shares none of its code, over planes at three scales with a silent stretch and three
parameter sets; E against section 1's routine (bits) and against exp in double, L against log in double, on samples of their full ranges
(every float32: tools/pcen_accuracy.cpp, profiles/pcen_accuracy.md); the known answers: a silent frame, b = 1, a constant plane; the split of
a plane into two calls, at a multiple of the chunk (bits) and elsewhere (the bound); the shipped routines of csrc/jsgx_internal.h against
the restatement, bit for bit, from a small C++ program; and the table and the coefficient.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

import pcen_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
T, B = 1000, 40


def errors(M, params, state=None):
    o32, S32, _ = pr.pcen32(M, state=state, **params)
    o64, S64, _ = pr.pcen64(M, state=state, **params)
    den = o64 + float(F32(params["bias"])) ** float(F32(params["power"]))
    assert (S64 >= 0).all() and np.isfinite(o32).all()
    assert (o32[den == 0] == 0).all() and (S32[S64 == 0] == 0).all()          # silent without bias, or b = 1: 0 / 0 is not an error
    live, smooth = den > 0, S64 > 0
    return float(np.max(np.abs(S32 - S64)[smooth] / S64[smooth])), float(np.max(np.abs(o32[live] - o64[live]) / den[live]))


@pytest.mark.parametrize("which", range(len(pr.PARAMS)), ids=[p[0] for p in pr.PARAMS])
@pytest.mark.parametrize("scale", pr.SCALES, ids=["1", "2^31", "1e-6"])
def test_the_definition_against_float64(scale, which):
    """Seeds the accuracy tool did not use."""
    name, params = pr.PARAMS[which]
    for seed in (101, 102):
        M = pr.plane(T, B, seed, scale)
        assert (M[T // 2:T // 2 + T // 5] == 0).all() and (M[:T // 2] > 0).any()
        s, o = errors(M, params)
        print(f"scale {scale:g}, {name}, seed {seed}: S {s:.3g} (bound {pr.S_BOUND:.3g}), out {o:.3g} (bound {pr.OUT_BOUND:.3g})")
        assert s <= pr.S_BOUND and o <= pr.OUT_BOUND


def test_the_bounds_are_the_measurements():
    text = open(os.path.join(ROOT, "profiles", "pcen_accuracy.md")).read()
    assert f"Worst over everything: S {pr.S_MEASURED:.2e}, out {pr.OUT_MEASURED:.2e}." in text
    assert pr.S_BOUND == 4 * pr.S_MEASURED and pr.OUT_BOUND == 4 * pr.OUT_MEASURED


def strided(lo, hi, n):
    """n float32 values across [lo, hi] (one sign), evenly spaced in their bit patterns, both ends included."""
    a, b = sorted((int(F32(lo).view(np.uint32)), int(F32(hi).view(np.uint32))))
    return np.unique(np.linspace(a, b, n).astype(np.uint64)).astype(np.uint32).view(F32)


def test_the_exponential(jsg):
    x = np.concatenate([strided(-87.0, -0.0, 200001), F32([-87.0, -86.99999, -1.0, -1e-45, -0.0])])
    assert pr.same_bits(pr.exp_any32(x), pr.exp32(x)), "E against section 1's routine on [-87, 0]"
    full = np.concatenate([x, strided(0.0, 88.72, 200001), F32([0.0, 1e-45, 1.0, 88.0, 88.72])])
    got, want = pr.exp_any32(full).astype(np.float64), np.exp(full.astype(np.float64))
    worst = float(np.max(np.abs(got - want) / want))
    print(f"E: worst relative error {worst:.3g} over {full.size} values")
    assert worst <= jsg.capix.EXP_REL_BOUND and np.isfinite(got).all()
    edges = pr.exp_any32(F32([np.nan, -np.inf, np.nextafter(F32(-87.0), F32(-100.0)), np.nextafter(F32(88.72), F32(100.0)), 100.0, np.inf]))
    assert np.isnan(edges[0]) and (edges[1:3].view(np.uint32) == 0).all() and np.isposinf(edges[3:]).all()
    assert pr.exp_any32(F32([88.72]))[0] == F32(3.3931806e38)


def test_the_logarithm(jsg):
    x = np.concatenate([strided(1e-45, 3.4028235e38, 400001), F32([1e-45, 1.1754942e-38, 1.1754944e-38, 0.5, 1.0, 2.0, 3.4028235e38])])
    got, want = pr.log32(x).astype(np.float64), np.log(x.astype(np.float64))
    worst = float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))
    print(f"L: worst error {worst:.3g} of max(1, |ln x|) over {x.size} values")
    assert worst <= jsg.capix.LOG_ABS_BOUND
    assert pr.log32(F32([1.0]))[0].view(np.uint32) == 0 and np.isneginf(pr.log32(F32([0.0]))[0]) and np.isposinf(pr.log32(F32([np.inf]))[0])


def test_a_silent_frame_gives_plus_zero():
    for name, params in pr.PARAMS:
        for scale in pr.SCALES:
            M = pr.plane(300, 7, 5, scale)
            out, S, _ = pr.pcen32(M, **params)
            silent = M == 0
            assert silent.any() and (out[silent].view(np.uint32) == 0).all(), (name, scale)
            assert (out[~silent] >= 0).all() and (out > 0).any() and (S > 0).all()


def test_b_of_one():
    M = pr.plane(300, 7, 6)
    params = dict(pr.PARAMS[0][1], b=1.0)
    out, S, s = pr.pcen32(M, **params)
    assert pr.same_bits(S, M) and pr.same_bits(s, M[-1]) and (pr.decay(1.0) == 0).all()
    assert errors(M, params)[1] <= pr.OUT_BOUND


def test_two_calls():
    name, params = pr.PARAMS[0]
    M = pr.plane(T, B, 7)
    whole = pr.pcen32(M, **params)
    for cut in (256, 512, 768):
        first = pr.pcen32(M[:cut], **params)
        second = pr.pcen32(M[cut:], state=first[2], **params)
        for k in range(2):
            assert pr.same_bits(np.concatenate([first[k], second[k]]), whole[k]), (cut, k)
        assert pr.same_bits(second[2], whole[2])
    # elsewhere: another association of the same sum, within the bound against float64 (whose answer does not depend on the cut)
    first = pr.pcen32(M[:500], **params)
    second = pr.pcen32(M[500:], state=first[2], **params)
    S = np.concatenate([first[1], second[1]])
    out = np.concatenate([first[0], second[0]])
    assert not pr.same_bits(S, whole[1])
    o64, S64, _ = pr.pcen64(M, **params)
    s_err = float(np.max(np.abs(S - S64) / S64))
    o_err = float(np.max(np.abs(out - o64) / (o64 + 2.0 ** 0.5)))
    print(f"split at 500: S {s_err:.3g}, out {o_err:.3g}")
    assert s_err <= pr.S_BOUND and o_err <= pr.OUT_BOUND
    # the float64 route in two calls: the state is the smoothed value, zi = a * state
    h = pr.pcen64(M[:500], **params)
    t = pr.pcen64(M[500:], state=h[2].astype(F32), **params)
    assert np.max(np.abs(np.concatenate([h[1], t[1]]) - S64) / S64) < 1e-6


def test_a_constant_plane():
    """M = c: S = c at every frame (a c + b c = c), out = (c (eps + c)^-gain + bias)^power - bias^power, in double."""
    for name, params in pr.PARAMS:
        for c in (0.37, 1.0, 4000.0):
            M = np.full((600, 3), c, F32)
            out, S, s = pr.pcen32(M, **params)
            c64, p = float(F32(c)), {k: float(F32(v)) for k, v in params.items()}
            want = (c64 * (p["eps"] + c64) ** -p["gain"] + p["bias"]) ** p["power"] - p["bias"] ** p["power"]
            assert np.max(np.abs(S - c64) / c64) <= pr.S_BOUND, (name, c)
            assert np.max(np.abs(out - want) / (want + p["bias"] ** p["power"])) <= pr.OUT_BOUND, (name, c)


def test_the_table_and_the_coefficient(jsg):
    for b in (pr.default_b(), 0.025, 1.0, 0.5, 1e-4):
        assert pr.same_bits(jsg.pcen_decay(b), pr.decay(b)), b
    assert jsg.pcen_coefficient(0.4, 22050, 512) == pr.default_b()
    Tc = 0.06 * 44100 / 256
    assert abs(jsg.pcen_coefficient(0.06, 44100, 256) - (np.sqrt(1 + 4 * Tc * Tc) - 1) / (2 * Tc * Tc)) < 1e-15
    for bad in (0.0, -0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(jsg.JsgError):
            jsg.pcen_decay(bad)


def test_the_shipped_routines_equal_the_restatement(tmp_path):
    """exp_any and log_pos of csrc/jsgx_internal.h (what the kernels compile) on the host, bit for bit against exp_any32 and log32."""
    src = tmp_path / "routines.cpp"
    src.write_text('#include <cstdio>\n#include "jsgx_internal.h"\nint main() {\n    unsigned b;\n    while (std::scanf("%x", &b) == 1)\n'
                   '        std::printf("%08x %08x\\n", jsgx::bits_of_float(jsgx::exp_any(jsgx::float_of_bits(b))), jsgx::bits_of_float(jsgx::log_pos(jsgx::float_of_bits(b))));\n'
                   "    return 0;\n}\n")
    exe = tmp_path / "routines"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "jadespectrogram_amd", "csrc"),
                           str(src), "-o", str(exe)])
    x = np.concatenate([strided(-100.0, -0.0, 5001), strided(0.0, 3.4028235e38, 20001), strided(80.0, 90.0, 2001),
                        F32([np.nan, np.inf, -np.inf, -87.0, 88.72, 0.0, 1e-45, 1.1754942e-38, 1.0])])
    out = subprocess.run([str(exe)], input="\n".join(f"{v:08x}" for v in x.view(np.uint32)), capture_output=True, text=True, check=True).stdout.split()
    got = np.array([int(v, 16) for v in out], np.uint32).reshape(-1, 2)
    assert pr.same_bits(got[:, 0].copy().view(F32), pr.exp_any32(x)) and pr.same_bits(got[:, 1].copy().view(F32), pr.log32(x))

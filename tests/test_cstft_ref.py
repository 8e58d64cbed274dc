"""The helpers of tests/cstft_ref.py, shown to bite before the GPU tests trust them.  CPU only, a few seconds.

* the float64 reference agrees with the closed forms (an impulse, a tone on a bin);
* a float32 CPU FFT passes every bound at M = 1, so the reference alone never fails a test;
* a numpy float32 restatement of cstft_fwd_kernel's arithmetic (radix-4 Stockham passes, a radix-2 pass last where log2 N is odd,
  twiddles rounded once from double, the real split as written; no contraction -- test code, it pins no bits) passes at M = 2 and
  fails the bound with any one of four faults switched on;
* the per-sample inverse bound fails when one bin of one frame is turned by one twiddle step.
"""
import numpy as np
import pytest

import cstft_ref as R

CPU_SIZES = (512, 2048, 8192)


# ------------------------------------------------------------------------------------------------ the restated forward kernel
def restated_forward(fr, fault=None):
    """fr [F][n] float32 windowed frames (consecutive frames share a tile as in the kernel: max(1, 2048 / n) per tile) ->
    [F][n/2+1] complex64.  fault: None, 'split', 'pass', 'nyquist' or 'frame'."""
    f32 = np.float32
    F, n = fr.shape
    N = n // 2
    ang = -2.0 * np.pi * np.arange(N) / n
    twr, twi = np.cos(ang).astype(f32), np.sin(ang).astype(f32)

    def tw(m):      # W_n^m, m < n, from the half table
        s = np.where(m < N, f32(1), f32(-1))
        return s * twr[m % N], s * twi[m % N]

    def mul(ar, ai, br, bi):
        return ar * br - ai * bi, ar * bi + ai * br

    zr, zi = fr[:, 0::2].astype(f32), fr[:, 1::2].astype(f32)
    NS = 1
    while NS < N:
        Rx = 4 if NS * 4 <= N else 2
        Q = N // Rx
        j = np.arange(Q)
        k = j % NS
        step = 2 * N // (Rx * NS)
        a = [[zr[:, j + r * Q].copy(), zi[:, j + r * Q].copy()] for r in range(Rx)]
        if fault == "frame" and NS == 1:        # frames 1.. of a tile read input 1 of butterfly Q/3 from the frame before
            fpb = max(1, 1024 // N)
            f = np.arange(F)[np.arange(F) % fpb != 0]
            a[1][0][f, Q // 3], a[1][1][f, Q // 3] = zr[f - 1, Q // 3 + Q], zi[f - 1, Q // 3 + Q]
        if NS > 1:
            for r in range(1, Rx):
                m = r * k * step
                if fault == "pass" and NS * Rx == N and r == 1:
                    m[Q // 3] += 1              # one twiddle of the last pass, one table entry further
                a[r] = list(mul(a[r][0], a[r][1], *tw(m)))
        if Rx == 2:
            y = [(a[0][0] + a[1][0], a[0][1] + a[1][1]), (a[0][0] - a[1][0], a[0][1] - a[1][1])]
        else:
            t0 = (a[0][0] + a[2][0], a[0][1] + a[2][1])
            t1 = (a[0][0] - a[2][0], a[0][1] - a[2][1])
            t2 = (a[1][0] + a[3][0], a[1][1] + a[3][1])
            d = (a[1][0] - a[3][0], a[1][1] - a[3][1])
            t3 = (d[1], -d[0])
            y = [(t0[0] + t2[0], t0[1] + t2[1]), (t1[0] + t3[0], t1[1] + t3[1]), (t0[0] - t2[0], t0[1] - t2[1]), (t1[0] - t3[0], t1[1] - t3[1])]
        dst = (j // NS) * NS * Rx + k
        zr, zi = np.empty_like(zr), np.empty_like(zi)
        for r in range(Rx):
            zr[:, dst + r * NS], zi[:, dst + r * NS] = y[r]
        NS *= Rx
    k = np.arange(N + 1)
    ik, im = k & (N - 1), (N - k) & (N - 1)
    if fault == "nyquist":
        ik[N] = 1
    kt = k.copy()
    if fault == "split":
        kt[3 * N // 4] += 1
    Er, Ei = (zr[:, ik] + zr[:, im]) * f32(0.5), (zi[:, ik] - zi[:, im]) * f32(0.5)
    Or, Oi = (zi[:, ik] + zi[:, im]) * f32(0.5), (zr[:, im] - zr[:, ik]) * f32(0.5)
    pr, pi = mul(*tw(kt), Or, Oi)
    assert pr.dtype == f32 and Er.dtype == f32
    return ((Er + pr) + 1j * (Ei + pi)).astype(np.complex64)


def run_frames(fn, x, n, hop, F, w):
    fr = R.frames_f32(x, n, hop, 0, F, w)
    return np.stack([fn(np.ascontiguousarray(row)) for row in fr])


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("n", [512, 8192])
def test_reference_matches_the_closed_forms(n):
    for kind in ("rect", "ramp"):
        w = R.window(kind, n)
        x, hop, F = R.impulse(n)
        frames = np.unique(np.concatenate([np.arange(4), np.arange(n - 4, n), np.arange(5, n, 97)]))
        ref = np.fft.rfft(R.frames_f32(x, n, hop, 0, F, w)[0, frames].astype(np.float64), axis=-1)
        assert np.abs(ref - R.impulse_closed_form(n, w, frames)).max() <= 1e-12
    x = R.tones(n, n, 1)
    ref = R.forward_f64(x, n, n, 1, R.window("rect", n))[:, 0]
    k = np.arange(n // 2 + 1)
    amp = np.abs(ref[k, k])
    assert (amp[1:-1] >= 0.5 * n - 1e-2).all() and (amp[1:-1] <= 0.5 * n + 1e-2).all()     # float32 samples: 6e-8 each
    off = np.abs(ref)
    off[k, k] = 0
    assert off.max() <= 1e-6 * n        # the float32 rounding of the samples, spread over the other bins


def test_frame_metric_sees_one_weak_bin():
    n = 2048
    x, hop, F, w = R.forward_class("noise_hann", n)
    ref = R.forward_f64(x, n, hop, F, w)
    X = ref.astype(np.complex64)
    good = R.forward_figures(X, x, n, hop, w)
    assert good.ratio <= 1.0        # rounding the reference to complex64 is better than any float32 FFT
    weak = int(np.argmin(np.abs(ref[1, 7])))
    X[1, 7, weak] += 2 * np.pi / n * X[1, 7, weak + 1 if weak < n // 2 else weak - 1]
    bad = R.forward_figures(X, x, n, hop, w)
    assert (bad.row, bad.frame, bad.bin) == (1, 7, weak) and bad.e > R.M * bad.Y
    l2 = np.linalg.norm(X[1, 7] - ref[1, 7]) / np.linalg.norm(ref[1, 7])
    assert l2 < 1e-3       # for scale: what a per-frame L2 figure makes of the same fault


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("n", CPU_SIZES)
@pytest.mark.parametrize("cls", R.FORWARD_CLASSES)
def test_float32_cpu_fft_passes_forward_at_m1(cls, n):
    x, hop, F, w = R.forward_class(cls, n, small=True)
    X = R.rfft32(R.frames_f32(x, n, hop, 0, F, w))
    g = R.assert_forward(X, x, n, hop, w, f"scipy {cls} n={n}", m=1.0)
    assert 2e-8 < g.Y < 1e-6        # a single-precision FFT: the yardstick is neither exact nor broken


@pytest.mark.parametrize("n", CPU_SIZES)
@pytest.mark.parametrize("cls", R.FORWARD_CLASSES)
def test_restated_kernel_passes_at_m2(cls, n):
    x, hop, F, w = R.forward_class(cls, n, small=True)
    X = run_frames(restated_forward, x, n, hop, F, w)
    R.assert_forward(X, x, n, hop, w, f"restated {cls} n={n}")
    if F > 1 or cls != "tones":
        assert (X[:, :, 0].imag == 0).all() and (X[:, :, -1].imag == 0).all()


# the class of input that is named for each fault must catch it (others may too)
FAULTS = [("split", "tones", CPU_SIZES), ("pass", "noise_rect", CPU_SIZES), ("nyquist", "impulses", CPU_SIZES),
          ("frame", "noise_hann", (512, 1024))]      # tiles hold more than one frame below 2048 points only


@pytest.mark.parametrize("fault,cls,n", [(f, c, n) for f, c, sizes in FAULTS for n in sizes])
def test_injected_fault_is_caught(fault, cls, n):
    x, hop, F, w = R.forward_class(cls, n, small=True)
    X = run_frames(lambda fr: restated_forward(fr, fault), x, n, hop, F, w)
    clean = run_frames(restated_forward, x, n, hop, F, w)
    assert (X != clean).any()
    g = R.forward_figures(X, x, n, hop, w)
    assert g.e > R.M * g.Y, f"{fault} not caught by {cls} at n={n}: e={g.e:.3g}, Y={g.Y:.3g}"
    assert g.e > 100 * g.Y or fault in ("split", "pass"), (fault, g)
    with pytest.raises(AssertionError):
        R.assert_forward(X, x, n, hop, w, "faulty")


# ------------------------------------------------------------------------------------------------ inverse
def inverse_f32_pipeline(X, n, hop, w, T):
    """A float32 CPU stand-in for the GPU: float32 irfft, times w, float32 ascending sum, times float32(1 / env64)."""
    rows, F = X.shape[0], X.shape[1]
    span = (F - 1) * hop + n
    fr = R.irfft32(X, n).astype(np.float32) * w.astype(np.float32)
    acc, env = np.zeros((rows, span), np.float32), np.zeros(span)
    w2 = w.astype(np.float64) ** 2
    for j in range(F):
        acc[:, j * hop:j * hop + n] += fr[:, j]
        env[j * hop:j * hop + n] += w2
    live = env > R.ENV_EPS
    rec = (1.0 / np.where(live, env, 1.0)).astype(np.float32)
    return np.where(live, acc * rec, np.float32(0))[:, :T]


@pytest.mark.parametrize("n", CPU_SIZES)
def test_float32_cpu_pipeline_passes_inverse_at_m1(n):
    worst = 0.0
    for wk, hop, F in R.inverse_cases(n):
        w = R.window(wk, n)
        X = R.random_bins(3, F, n, seed=n + hop)
        T = (F - 1) * hop + n
        ref = R.inverse_f64(X, n, hop, w, T)
        y = inverse_f32_pipeline(X, n, hop, w, T)
        g = R.assert_inverse(y, ref, R.inverse_yardstick(X, n), f"{wk} hop={hop}", n, hop, m=1.0, dead_cap=T // 1000)
        assert g.dead == int((ref.env <= R.ENV_EPS).sum()) and (y[:, ref.env <= R.ENV_EPS] == 0).all()
        worst = max(worst, g.ratio)
    assert worst > 0.05       # the bound is a bound, not a blanket


def test_basis_and_unread_imaginary_parts():
    n = 512
    X = R.basis_bins(n)
    w = R.window("rect", n)
    T = X.shape[1] * n
    ref = R.inverse_f64(X, n, n, w, T)
    m = np.arange(n)
    fr = ref.y.reshape(-1, n)
    assert np.abs(fr[5] - 2.0 / n * np.cos(2 * np.pi * 5 * m / n)).max() <= 1e-15
    assert np.abs(fr[n // 2 + 1 + 5] + 2.0 / n * np.sin(2 * np.pi * 5 * m / n)).max() <= 1e-15
    assert np.abs(fr[0] - 1.0 / n).max() <= 1e-15 and np.abs(fr[n // 2] - (1.0 / n) * (-1.0) ** m).max() <= 1e-15
    assert (fr[n // 2 + 1] == 0).all() and (fr[n + 1] == 0).all()       # a unit in the imaginary part of bin 0, of bin n/2
    y = inverse_f32_pipeline(X, n, n, w, T)
    R.assert_inverse(y, ref, R.inverse_yardstick(X, n), "basis", n, n, m=1.0)


@pytest.mark.parametrize("n", CPU_SIZES)
def test_inverse_bound_bites(n):
    hop, F = n // 4, 12
    w = R.window("hann", n)
    X = R.random_bins(2, F, n, seed=n)
    T = (F - 1) * hop + n
    ref = R.inverse_f64(X, n, hop, w, T)
    Y = R.inverse_yardstick(X, n)
    strong = int(np.argmax(np.abs(X[1, 5])))      # the strongest bin of one frame, turned by one twiddle step
    bad = X.copy()
    bad[1, 5, strong] *= np.complex64(np.exp(2j * np.pi / n))
    g = R.inverse_figures(inverse_f32_pipeline(bad, n, hop, w, T), ref, Y)
    assert g.ratio > 1.0 and g.row == 1 and 5 * hop <= g.t < 5 * hop + n
    y = inverse_f32_pipeline(X, n, hop, w, T)
    y[0, T // 2] = np.nan
    assert R.inverse_figures(y, ref, Y).ratio == np.inf
    y = inverse_f32_pipeline(X, n, hop, w, T)
    dead = np.flatnonzero(ref.env <= R.ENV_EPS)
    assert dead.size >= 1
    y[0, dead[0]] = 1e-30
    assert R.inverse_figures(y, ref, Y).ratio == np.inf

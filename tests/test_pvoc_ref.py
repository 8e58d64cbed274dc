"""Phase vocoder, the yardsticks themselves (tests/pvoc_ref.py): the float32 restatement of the library's arithmetic against the
float64 reference of the definition, within the bound the GPU tests build on.  CPU only."""
import numpy as np
import pytest

import pvoc_ref as pr

RATES = list(pr.RATES)


@pytest.mark.parametrize("n,hop", [(512, 128), (512, 100), (1024, 256), (2048, 512), (2048, 100)])
def test_restatement_stays_within_its_bound(n, hop):
    for rate in RATES:
        X = pr.make_input(n, hop, pr.frames_for(rate))
        R = pr.reference(X, rate, hop, n)
        S = pr.restatement(X, rate, hop, n)
        assert S.shape == R.shape == (pr.n_frames_out(X.shape[0], rate), n // 2 + 1)
        err = pr.rel_error(S, R)
        ratio = float((err / pr.bound_restatement(R.shape[0])[:, None]).max())
        print(f"n {n} hop {hop} rate {rate:.4f}: worst relative error {err.max():.3e}, worst ratio to the bound {ratio:.3f}")
        assert ratio <= 1.0, (n, hop, rate, ratio)
        both_zero = (np.abs(R) == 0)
        assert both_zero.any() and (S[both_zero] == 0).all()


def test_restatement_long_input():
    """4000 output frames: the bound grows with the frame index, the error must not outgrow it."""
    n, hop, rate = 1024, 256, 0.8
    X = pr.make_input(n, hop, pr.frames_for(rate, 4000))
    R, S = pr.reference(X, rate, hop, n), pr.restatement(X, rate, hop, n)
    assert R.shape[0] == 4000
    assert (pr.rel_error(S, R) <= pr.bound_restatement(4000)[:, None]).all()


@pytest.mark.parametrize("n,hop", [(512, 128), (2048, 100)])
def test_reference_rate_one_is_the_identity(n, hop):
    """At rate 1 alpha is 0 and the phase telescopes to arg X[i].  In float64 every step rounds five times at a size of up to
    A_k + 2 pi (the angle difference, minus A_k, 2 pi times the rounded quotient, its subtraction, plus A_k), and the float64 2 pi is
    off by 0.35 * 2^-53 relative: at most 6 * 2^-53 (A_k + 2 pi) per step.  The running sum rounds each partial sum of size up to
    m (A_k + pi) to half an ulp: at most 2^-54 (i+1)^2 (A_k + pi) up to frame i.  2^-48 covers the angles, the magnitude, sine and
    cosine."""
    X = pr.make_input(n, hop, 300)
    R = pr.reference(X, 1.0, hop, n)
    i = np.arange(300, dtype=np.float64)[:, None]
    A = 2 * np.pi * hop * np.arange(n // 2 + 1)[None, :] / n
    bound = 2.0 ** -48 + 6 * 2.0 ** -53 * (i + 1) * (A + 2 * np.pi) + 2.0 ** -54 * (i + 1) ** 2 * (A + np.pi)
    assert (pr.rel_error(R, X.astype(np.complex128)) <= bound).all()


def test_one_frame_and_rate_beyond_the_input():
    X = pr.make_input(512, 128, 1)
    for rate in RATES:
        R, S = pr.reference(X, rate, 128, 512), pr.restatement(X, rate, 128, 512)
        assert R.shape[0] == pr.n_frames_out(1, rate) == (2 if rate < 1 else 1)
        assert (pr.rel_error(S, R) <= pr.bound_restatement(R.shape[0])[:, None]).all()
    X = pr.make_input(512, 100, 3)
    R = pr.reference(X, 3.5, 100, 512)
    assert R.shape[0] == 1 and (pr.rel_error(pr.restatement(X, 3.5, 100, 512), R) <= pr.bound_restatement(1)[:, None]).all()


@pytest.mark.parametrize("case", pr.edge_cases(), ids=pr.edge_id)
def test_restatement_on_the_edge_cases(case):
    """Tiny, tile-sized and the largest n, hops 1 and n, rates from 0.1 to 3.5 and next to 1, Hann noise and the special values: the
    yardstick of the GPU tests is itself within its bound there, finite, and exactly zero where the reference is."""
    n, hop, rate, T, kind = case
    X = pr.edge_input(case)
    R, S = pr.reference(X, rate, hop, n), pr.restatement(X, rate, hop, n)
    assert S.shape == R.shape == (pr.n_frames_out(T, rate), n // 2 + 1)
    assert np.isfinite(R.real).all() and np.isfinite(R.imag).all() and np.isfinite(S.real).all() and np.isfinite(S.imag).all()
    err = pr.rel_error(S, R)
    ratio = float((err / pr.bound_restatement(R.shape[0])[:, None]).max())
    print(f"{pr.edge_id(case)}: worst relative error {err.max():.3e}, worst ratio to the bound {ratio:.3f}")
    assert ratio <= 1.0
    both_zero = (np.abs(R) == 0)
    assert both_zero.any() and not both_zero.all() and (S[both_zero] == 0).all()


def test_special_input_holds_what_it_promises():
    X = pr.special_input(512, 400)
    assert X.dtype == np.complex64 and X.shape == (400, 257) and not X.flags.writeable
    re, im = X.real, X.imag
    mod = np.abs(X.astype(np.complex128))
    assert np.isfinite(mod).all() and mod[mod > 0].min() >= 2.0 ** -91 and mod.max() < 2.0 ** 126.5
    with np.errstate(over="ignore", under="ignore"):
        naive = re * re + im * im
    assert np.isinf(naive).any() and ((naive == 0) & (mod > 0)).any()          # x * x leaves float32 at both ends
    zero = (re == 0) & (im == 0)
    assert 0.10 < zero.mean() < 0.20
    for sr in (False, True):
        for si in (False, True):
            assert (zero & (np.signbit(re) == sr) & (np.signbit(im) == si)).sum() > 0.02 * X.size, (sr, si)
    ang = np.arctan2(im.astype(np.float64), re.astype(np.float64))
    on_dir = ~zero & ((re == 0) | (im == 0) | (np.abs(re) == np.abs(im)))
    assert 0.15 < on_dir.mean() < 0.30
    for q in range(-4, 5):                                                      # every multiple of pi / 4, -pi and +pi among them
        assert (on_dir & (ang == q * (np.pi / 4))).any(), q


@pytest.mark.parametrize("rate", [0.38, 1.0, 1.3, 2.5])
@pytest.mark.parametrize("n,hop", [(512, 128), (2048, 100)])
def test_reference_continues_a_stationary_phase(n, hop, rate):
    """X[j][k] = m_k exp(i (theta_k + j w_k)) in complex128: every pair has the moduli m_k and the angle difference w_k, so as long
    as a1 is inside the input (floor(i rate) + 1 <= T - 1) the definition gives m_k exp(i (theta_k + i w_k)) whatever the rate.
    The bound is that of test_reference_rate_one_is_the_identity (five roundings a step at a size of up to A_k + 2 pi and the
    float64 2 pi: 6 * 2^-53 (A_k + 2 pi) per step; the running sum: 2^-54 (i+1)^2 (A_k + pi); 2^-48 for the angles, the modulus,
    sine and cosine) plus what the input itself carries: theta_k + j w_k is rounded at a size of up to (T + 1) pi, so the angle of
    X[j] is off by up to 2^-53 (T + 1) pi; away from rate 1 these do not telescope, each step takes two of them, and the expected
    value rounds theta_k + i w_k the same way: at most 2^-52 (i+1) (T + 2) pi."""
    T, K = 200, n // 2 + 1
    rng = np.random.default_rng(n + hop)
    m, theta, w = rng.uniform(0.1, 10.0, K), rng.uniform(-np.pi, np.pi, K), rng.uniform(-np.pi, np.pi, K)
    X = m[None, :] * np.exp(1j * (theta[None, :] + np.arange(T)[:, None] * w[None, :]))
    R = pr.reference(X, rate, hop, n)
    assert R.shape[0] == pr.n_frames_out(T, rate)
    i = np.arange(R.shape[0], dtype=np.float64)[:, None]
    inside = np.floor(i[:, 0] * rate) + 1 <= T - 1
    assert inside.sum() >= R.shape[0] - 3 and inside.sum() > 70
    want = m[None, :] * np.exp(1j * (theta[None, :] + i * w[None, :]))
    A = 2 * np.pi * hop * np.arange(K)[None, :] / n
    bound = (2.0 ** -48 + 6 * 2.0 ** -53 * (i + 1) * (A + 2 * np.pi) + 2.0 ** -54 * (i + 1) ** 2 * (A + np.pi)
             + 2.0 ** -52 * (i + 1) * (T + 2) * np.pi)
    err = pr.rel_error(R, want)
    print(f"n {n} hop {hop} rate {rate}: worst error / bound {float((err / bound)[inside].max()):.3f}")
    assert (err[inside] <= bound[inside]).all()


def _naive_hypot(z):
    """A float32 sqrt(x x + y y) in place of hypotf: the squares overflow above 2^64 and vanish below 2^-75."""
    with np.errstate(over="ignore", under="ignore"):
        return np.sqrt((z.real * z.real).astype(np.float32) + (z.imag * z.imag).astype(np.float32))


def _atan2_without_signed_zeros(z):
    """atan2f fed x + 0.0f: -0 becomes +0, so arg(-0 + 0j) is 0 instead of pi and arg(-1 - 0j) is pi instead of -pi."""
    return np.arctan2(z.imag + np.float32(0), z.real + np.float32(0))


@pytest.mark.parametrize("fault", [dict(modulus=_naive_hypot), dict(angle=_atan2_without_signed_zeros)], ids=["naive-hypot", "atan2-drops-zero-signs"])
def test_special_input_catches_what_hann_noise_lets_through(fault):
    """Two plausible defects of a kernel, injected into the restatement.  On Hann-windowed noise each stays within the device's cap
    at the worst ratio of the sound restatement (to three figures); on special_input each breaks the cap.  If this fails after a
    change to special_input, the class has lost what it is for."""
    n, hop, rate, T = 512, 128, 0.8, 400
    cap = pr.bound_cap(pr.n_frames_out(T, rate))[:, None]

    def worst(X, **kw):
        with np.errstate(invalid="ignore", over="ignore"):
            return float(np.nan_to_num(pr.rel_error(pr.restatement(X, rate, hop, n, **kw), pr.reference(X, rate, hop, n)) / cap, nan=np.inf).max())

    X = pr.make_input(n, hop, T)
    sound, faulty = worst(X), worst(X, **fault)
    print(f"Hann noise: sound {sound:.4f} of the cap, faulty {faulty:.4f}")
    assert sound <= 1.0 and faulty <= 1.0 and round(faulty, 3) == round(sound, 3)
    X = pr.special_input(n, T)
    sound, faulty = worst(X), worst(X, **fault)
    print(f"special values: sound {sound:.4f} of the cap, faulty {faulty:.3e}")
    assert sound <= 1.0 and not faulty <= 1.0

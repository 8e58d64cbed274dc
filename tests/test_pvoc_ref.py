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

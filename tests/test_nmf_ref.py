"""The numpy restatement of include/jsgx.h section 12 (tests/nmf_ref.py) on its own: its float64 form against scikit-learn's
multiplicative-update solver, one float32 update of either factor against float64 inside the bound the header's sums give, the known
answers, the loss over 50 iterations, and that the probe input of the GPU test tells the order of a sum.  CPU only; needs no library."""
import warnings

import numpy as np
import pytest

import nmf_ref as nr

SHAPES = [(64, 1025, 32), (96, 300, 7), (33, 2049, 64)]


def sklearn_factors(V, A0, C0, n_iter, update_components=True):
    nmf = pytest.importorskip("sklearn.decomposition")
    V, A0, C0 = (np.array(x, np.float64) for x in (V, A0, C0))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        W, H, _ = nmf.non_negative_factorization(V, W=A0 if update_components else None, H=C0, n_components=C0.shape[0], init="custom", update_H=update_components,
                                                 solver="mu", beta_loss="frobenius", tol=0, max_iter=n_iter)
    return W, H


@pytest.mark.parametrize("n_iter", [1, 3, 25])
def test_the_float64_form_is_scikit_learns(n_iter):
    V, A0, C0 = nr.problem(70, 33, 5)
    W, H = sklearn_factors(V, A0, C0, n_iter)
    A, C = nr.nmf64(V, A0, C0, n_iter)
    for got, want in ((A, W), (C, H)):
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"n_iter {n_iter}: relative difference {err:.3e}")
        assert err <= 1e-12


def test_fixed_components_are_scikit_learns_transform():
    """With update_H=False scikit-learn ignores the caller's W and starts from the constant sqrt(mean(V) / r)."""
    V, _, C0 = nr.problem(70, 33, 5)
    W, H = sklearn_factors(V, None, C0, 25, update_components=False)
    A, C = nr.nmf64(V, np.full((70, 5), nr.constant_start(V, 5)), C0, 25, update_components=False)
    assert np.array_equal(C, np.array(C0, np.float64)) and np.array_equal(H, C)
    err = np.abs(A - W).max() / np.abs(W).max()
    print(f"relative difference {err:.3e}")
    assert err <= 1e-12


@pytest.mark.parametrize("T, K, r", SHAPES)
def test_one_float32_update_against_float64(T, K, r):
    V, A0, C0 = nr.problem(T, K, r)
    V64, A64, C64 = (np.array(x, np.float64) for x in (V, A0, C0))
    A1 = nr.update_a32(V, A0, C0)
    bound = nr.update_bound(K, nr.CHUNK_K, r)
    err = np.abs(A1 - nr.update_a64(V64, A64, C64)) / nr.update_a64(V64, A64, C64)
    print(f"A: {err.max() / nr.U:.1f} u, bound {bound / nr.U:.0f} u")
    assert err.max() <= bound
    # the components from the float32 activations, both forms
    C1 = nr.update_c32(V, A1, C0)
    want = nr.update_c64(V64, np.array(A1, np.float64), C64)
    bound = nr.update_bound(T, nr.CHUNK_T, r)
    err = np.abs(C1 - want) / want
    print(f"C: {err.max() / nr.U:.1f} u, bound {bound / nr.U:.0f} u")
    assert err.max() <= bound


def integers(T, K, r, seed=3):
    rng = np.random.default_rng(seed)
    A = rng.integers(0, 4, (T, r)).astype(np.float32)
    C = rng.integers(0, 4, (r, K)).astype(np.float32)
    A[:, 0] += 1                                      # no empty frame
    C[0] += 1                                         # no empty bin
    return (A.astype(np.float64) @ C.astype(np.float64)).astype(np.float32), A, C


def test_an_exact_factorisation_is_a_fixed_point():
    """V = A C from small integers: every sum is exact, N = D and N2 = D2, every ratio is exactly 1."""
    V, A, C = integers(40, 70, 6)
    assert (V > 0).all() and V.max() < 2 ** 10        # every D and D2 is positive: a zero would take the 2^-23 rule, not the ratio
    A3, C3 = nr.nmf32(V, A, C, 3)
    assert nr.same_bits(A3, A) and nr.same_bits(C3, C)


def test_zero_frames_bins_and_rows():
    V, A0, C0 = (np.array(x) for x in nr.problem(40, 70, 6))
    V[7] = 0                                          # an all-zero frame zeroes its row of A
    V[:, 11] = 0                                      # an all-zero bin zeroes its column of C
    A0[20] = 0                                        # an all-zero row of A takes the 2^-23 rule and stays zero
    A, C = nr.nmf32(V, A0, C0, 2)
    assert not A[7].any() and not C[:, 11].any() and not A[20].any()
    keep = np.ones(40, bool)
    keep[[7, 20]] = False
    assert (A[keep] > 0).all() and (np.delete(C, 11, axis=1) > 0).all() and np.isfinite(A).all() and np.isfinite(C).all()


def test_the_probe_input_tells_the_order():
    """The shape of the first GPU test: with k descending inside every chunk the bits differ, so equal bits there mean the stated order."""
    V, A0, C0 = nr.problem(32, 258, 32)
    up, down = nr.update_a32(V, A0, C0), nr.update_a32(V, A0, C0, reverse=True)
    differ = int((up.view(np.uint32) != down.view(np.uint32)).sum())
    print(f"{differ} of {up.size} activations differ")
    assert differ >= up.size // 4
    assert np.abs(up - down).max() <= 64 * nr.U * np.abs(up).max()          # and yet the same numbers to rounding


def test_the_loss_falls():
    V, A0, C0 = nr.problem(70, 33, 5)
    for form in (nr.nmf64, None):
        if form is not None:
            losses = []
            form(V, A0, C0, 50, losses=losses)
        else:
            losses, A, C = [], np.array(A0), np.array(C0)
            for _ in range(50):
                A, C = nr.nmf32(V, A, C, 1)
                losses.append(float(np.linalg.norm(V.astype(np.float64) - A.astype(np.float64) @ C.astype(np.float64))))
        assert losses[49] < losses[0]

"""The references of the band-kernel tests (tests/fb_band_ref.py) checked on their own: band_f32 against a scalar float32 loop, the CSR and
the dense form bit for bit, and |band_f32 - band_f64| <= band_cap for every bank tests/test_gpu_fb_band.py runs -- so the bound the GPU is
held to is known to be satisfiable by a correct float32 sum before a GPU sees it.  CPU only."""
import numpy as np
import pytest

import fb_band_ref as R


def scalar_band(P, fb):
    out = np.zeros((P.shape[0], fb.n_bands), np.float32)
    for j in range(P.shape[0]):
        for b in range(fb.n_bands):
            acc = np.float32(0.0)
            for k in range(int(fb.n_bins[b])):
                prod = np.float32(fb.weights[fb.offset[b] + k]) * np.float32(P[j, fb.first_bin[b] + k])
                acc = np.float32(acc + prod)
            out[j, b] = acc
    return out


def test_band_f32_equals_a_scalar_loop(jsg):
    n = 512
    P = R.power_plane(3, n)
    for fb in (R.edge_bank(jsg, n, "edge"), R.edge_bank(jsg, n, "narrow257"), jsg.Filterbank(n, R.FS, 10, 0.0, R.FS / 2)):
        got = R.band_f32(P, fb)
        assert got.dtype == np.float32 and (got.view(np.uint32) == scalar_band(P, fb).view(np.uint32)).all()


@pytest.mark.parametrize("n", [512, 4096])
def test_csr_and_dense_forms_agree(jsg, n):
    P = R.power_plane(5, n, seed=1)
    for W in (R.edge_matrix(n), R.narrow_matrix(n, 255), R.wide_matrix(n)):
        fb = jsg.Filterbank.from_matrix(W)
        assert (fb.matrix().view(np.uint32) == W.view(np.uint32)).all()
        assert (R.band_f32(P, fb).view(np.uint32) == R.band_dense(P, W).view(np.uint32)).all()
    fb = jsg.Filterbank(n, R.FS, 48, 0.0, R.FS / 2)
    assert (R.band_f32(P, fb).view(np.uint32) == R.band_dense(P, fb.matrix()).view(np.uint32)).all()


def test_the_seeded_banks_have_the_shapes_they_claim(jsg):
    for n in (1024, 4096, 8192):
        H = n // 2 + 1
        fb = R.edge_bank(jsg, n, "edge")
        E = R.EDGE_ROWS
        assert fb.n_bins[E["empty"]] == 0
        assert (fb.first_bin[E["bin0"]], fb.n_bins[E["bin0"]]) == (0, 1)
        assert (fb.first_bin[E["nyquist"]], fb.n_bins[E["nyquist"]]) == (H - 1, 1)
        assert fb.first_bin[E["ends_at_nyquist"]] + fb.n_bins[E["ends_at_nyquist"]] == H and fb.n_bins[E["ends_at_nyquist"]] > 1
        assert fb.n_bins[E["full"]] == H and fb.n_bins[E["full_zeros_inside"]] == H
        W = fb.matrix()
        assert (W[E["full"]] > 0).all() and np.count_nonzero(W[E["full_zeros_inside"]]) == 2
        neg = W[E["negative"], fb.first_bin[E["negative"]]:fb.first_bin[E["negative"]] + fb.n_bins[E["negative"]]]
        assert (neg < 0).sum() == 1 and (neg == 0).sum() == 4
        for B in R.NARROW_BANDS:
            nb = R.edge_bank(jsg, n, f"narrow{B}")
            assert nb.n_bands == B and nb.n_bins.min() >= 1 and nb.n_bins.max() <= 12 and (nb.weights > 0).all()
            assert nb.first_bin[0] == 0 and (B == 1 or nb.first_bin[-1] + nb.n_bins[-1] == H)
        assert R.edge_bank(jsg, n, "mel1").n_bands == 1
    assert R.wide_matrix(2048).shape == (24, 1025) and (R.wide_matrix(2048) > 0).all()


def test_split_columns():
    for n_cols in (32777, 16393, 6149, 8197, 3075, 4099, 9, 2 * 8 * 2048 + 9):
        k, c, f = R.split_columns(n_cols)
        assert k * c * f == n_cols and k >= 1 and 1 <= c <= 16 and f >= 1
    assert R.split_columns(3075) == (5, 3, 205) and R.split_columns(4099) == (1, 1, 4099) and R.split_columns(32777) == (73, 1, 449)


def _banks(jsg):
    for n, name, _ in R.FULL_CASES:
        yield n, name, R.full_bank(jsg, n, name)
    for n in R.TILE_N.values():
        for name in R.EDGE_BANKS:
            yield n, name, R.edge_bank(jsg, n, name)


def test_the_float64_bound_holds_for_the_reference_alone(jsg):
    """|band_f32 - band_f64| <= band_cap on positive random power planes, for every bank of the GPU tests."""
    worst = {}
    for n, name, fb in _banks(jsg):
        for seed in (0, 1):
            P = R.power_plane(24, n, seed=seed)
            assert (P > 0).all()
            err = np.abs(R.band_f32(P, fb).astype(np.float64) - R.band_f64(P, fb))
            cap = R.band_cap(P, fb)
            assert err.shape == cap.shape == (24, fb.n_bands)
            assert (err <= cap).all(), (n, name, float(np.max(err / np.maximum(cap, 1e-300))))
            live = cap > 0
            worst[(n, name)] = float(np.max(err[live] / cap[live])) if live.any() else 0.0
        assert (R.band_cap(P, fb)[:, fb.n_bins == 0] == 0).all()          # an empty band is exactly zero
    print("\n  worst |f32 - f64| / cap per bank:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) > 0.01          # the bound is not vacuous: the float32 sums do use a visible share of it

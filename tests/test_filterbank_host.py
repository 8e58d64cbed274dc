"""Filterbank construction (jsg_filterbank_build, host only): the scales at pinned values, every weight against a float64 restatement of
include/jsg.h section 2b (librosa's construction written out here), the LINEAR identity, LOG interpolation rows, UNIT_SUM rows, empty
bands, refusals, and the dense-matrix round trip.  CPU only."""
import math

import numpy as np
import pytest

SLANEY_LOGSTEP = math.log(6.4) / 27.0


def hz_to_mel(f, htk):
    f = np.asarray(f, np.float64)
    if htk:
        return 2595.0 * np.log10(1.0 + f / 700.0)
    return np.where(f < 1000.0, f / (200.0 / 3.0), 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / SLANEY_LOGSTEP)


def mel_to_hz(m, htk):
    m = np.asarray(m, np.float64)
    if htk:
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m < 15.0, (200.0 / 3.0) * m, 1000.0 * np.exp(SLANEY_LOGSTEP * (m - 15.0)))


def ref_bank(n, fs, B, fmin, fmax, scale, norm):
    """float64 dense [B][n/2+1] bank (before the float32 rounding), the spec of include/jsg.h 2b."""
    H = n // 2 + 1
    k = np.arange(H, dtype=np.float64)
    bins = lambda hz: np.asarray(hz, np.float64) * n / fs
    if scale in (0, 1):
        htk = scale == 1
        m = np.linspace(hz_to_mel(fmin, htk), hz_to_mel(fmax, htk), B + 2)
        hz = mel_to_hz(m, htk)
        lo, c, hi = bins(hz[:-2]), bins(hz[1:-1]), bins(hz[2:])
        slaney = 2.0 / (hz[2:] - hz[:-2])
    else:
        b = np.arange(-1, B + 1, dtype=np.float64)
        if scale == 2:
            r = (fmax / fmin) ** (1.0 / (B - 1))
            cen = fmin * r ** b
        else:
            cen = fmin + b * ((fmax - fmin) / (B - 1))
        x = bins(cen)
        c = x[1:-1]
        lo, hi = np.minimum(x[:-2], c - 1.0), np.maximum(x[2:], c + 1.0)
        slaney = 2.0 / ((hi - lo) * fs / n)
    up = (k[None, :] - lo[:, None]) / (c - lo)[:, None]
    down = (hi[:, None] - k[None, :]) / (hi - c)[:, None]
    W = np.maximum(0.0, np.minimum(up, down))
    if norm == 1:
        W = W * slaney[:, None]
    elif norm == 2:
        s = W.sum(axis=1, keepdims=True)
        W = np.where(s > 0, W / np.where(s > 0, s, 1.0), W)
    return W


def ulp_diff(a, b):
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def test_scale_formulas_at_pinned_values():
    assert hz_to_mel(1000.0, False) == pytest.approx(15.0, abs=1e-12)
    assert hz_to_mel(6400.0, False) == pytest.approx(42.0, abs=1e-12)
    assert hz_to_mel(700.0, True) == pytest.approx(2595.0 * math.log10(2.0), abs=1e-12)
    assert mel_to_hz(42.0, False) == pytest.approx(6400.0, rel=1e-14)


def test_centres_follow_the_scales(jsg):
    fb = jsg.Filterbank(2048, 48000.0, 40, 0.0, 24000.0, scale=jsg.capi.FB_MEL_SLANEY)
    want = mel_to_hz(np.linspace(0.0, hz_to_mel(24000.0, False), 42)[1:-1], False)
    assert np.allclose(fb.centres_hz, want, rtol=1e-6)
    lg = jsg.Filterbank(2048, 48000.0, 64, 20.0, 20000.0, scale=jsg.capi.FB_LOG)
    assert lg.centres_hz[0] == pytest.approx(20.0, rel=1e-6) and lg.centres_hz[-1] == pytest.approx(20000.0, rel=1e-6)
    assert np.allclose(np.diff(np.log(lg.centres_hz.astype(np.float64))), math.log(1000.0) / 63, rtol=1e-5)


@pytest.mark.parametrize("n", [512, 2048, 8192])
@pytest.mark.parametrize("fs", [44100.0, 48000.0, 96000.0])
@pytest.mark.parametrize("scale", [0, 1, 2, 3])
def test_weights_match_float64_restatement(jsg, n, fs, scale):
    H = n // 2 + 1
    for B in (1, 40, 128, H):
        for norm in (0, 1, 2):
            fmin = 30.0 if scale == 2 else (0.0 if scale != 3 else 100.0)
            fmax = fs / 2.0 if scale in (0, 1) else min(fs / 2.0, 16000.0)
            if scale in (2, 3) and B < 2:
                with pytest.raises(jsg.JsgError) as e:
                    jsg.Filterbank(n, fs, B, fmin, fmax, scale=scale, norm=norm)
                assert e.value.code == jsg.capi.JSG_ERR_INVALID
                continue
            fb = jsg.Filterbank(n, fs, B, fmin, fmax, scale=scale, norm=norm)
            got = fb.matrix()
            ref = ref_bank(n, fs, B, fmin, fmax, scale, norm)
            ref32 = ref.astype(np.float32)
            d = ulp_diff(got, ref32)
            assert d.max() <= 1, (B, norm, int(d.max()), np.unravel_index(int(d.argmax()), d.shape))
            # the CSR is the trimmed support of the dense bank: no zero weight at either end of a band
            for b in range(B):
                if fb.n_bins[b]:
                    w = fb.weights[fb.offset[b]:fb.offset[b] + fb.n_bins[b]]
                    assert w[0] != 0 and w[-1] != 0
                    assert fb.first_bin[b] >= 0 and fb.first_bin[b] + fb.n_bins[b] <= H
            assert (fb.offset == np.concatenate([[0], np.cumsum(fb.n_bins)[:-1]])).all()


@pytest.mark.parametrize("n,fs", [(512, 44100.0), (1024, 48000.0), (4096, 96000.0), (8192, 48000.0)])
def test_linear_full_range_is_the_identity(jsg, n, fs):
    H = n // 2 + 1
    fb = jsg.Filterbank(n, fs, H, 0.0, fs / 2.0, scale=jsg.capi.FB_LINEAR, norm=jsg.capi.FB_NORM_UNIT_SUM)
    assert (fb.first_bin == np.arange(H)).all() and (fb.n_bins == 1).all()
    assert (fb.weights.view(np.uint32) == np.float32(1.0).view(np.uint32)).all()


def test_log_row_narrower_than_a_bin_interpolates(jsg):
    n, fs, B = 1024, 48000.0, 400
    fb = jsg.Filterbank(n, fs, B, 20.0, 500.0, scale=jsg.capi.FB_LOG, norm=jsg.capi.FB_NORM_NONE)
    checked = 0
    for b in range(1, B - 1):
        c = fb.centres_hz[b] * np.float64(n) / fs
        r = (500.0 / 20.0) ** (1.0 / (B - 1))
        cen = 20.0 * r ** np.array([b - 1, b, b + 1], np.float64) * n / fs
        if cen[2] - cen[1] < 1.0 and cen[1] - cen[0] < 1.0 and cen[1] != math.floor(cen[1]):
            k = math.floor(cen[1])
            frac = cen[1] - k
            assert fb.n_bins[b] == 2 and fb.first_bin[b] == k, b
            w = fb.weights[fb.offset[b]:fb.offset[b] + 2]
            assert w[0] == np.float32(1.0 - frac) and w[1] == np.float32(frac), (b, w, frac)
            checked += 1
    assert checked > 100


@pytest.mark.parametrize("scale", [2, 3, 0])
def test_unit_sum_rows(jsg, scale):
    for n in (512, 2048, 8192):
        fb = jsg.Filterbank(n, 48000.0, 96, 40.0, 20000.0, scale=scale, norm=jsg.capi.FB_NORM_UNIT_SUM)
        W = fb.matrix()
        s = W.sum(axis=1, dtype=np.float32)
        nonempty = fb.n_bins > 0
        assert np.abs(s[nonempty].astype(np.float64) - 1.0).max() <= 2.0 ** -22


def test_empty_mel_bands_are_reported(jsg):
    fb = jsg.Filterbank(512, 48000.0, 128, 0.0, 24000.0, scale=jsg.capi.FB_MEL_SLANEY)
    empty = fb.n_bins == 0
    assert empty.any() and (fb.matrix()[empty] == 0).all()
    assert fb.weights.size == int(fb.n_bins.sum())


def test_invalid_specs_are_refused(jsg):
    C = jsg.capi
    good = dict(n=1024, fs=48000.0, n_bands=40, fmin=0.0, fmax=24000.0, scale=C.FB_MEL_SLANEY, norm=C.FB_NORM_SLANEY)
    bad = [dict(n=256), dict(n=16384), dict(n=1000), dict(fmin=-1.0), dict(fmax=24001.0), dict(fmin=500.0, fmax=500.0),
           dict(fmin=600.0, fmax=500.0), dict(n_bands=0), dict(n_bands=C.FB_MAX_BANDS + 1), dict(fs=0.0), dict(fmin=float("nan")),
           dict(scale=4), dict(norm=3), dict(scale=C.FB_LOG, fmin=0.0), dict(scale=C.FB_LOG, n_bands=1), dict(scale=C.FB_LINEAR, n_bands=1)]
    for change in bad:
        spec = dict(good, **change)
        with pytest.raises(jsg.JsgError) as e:
            jsg.Filterbank(spec["n"], spec["fs"], spec["n_bands"], spec["fmin"], spec["fmax"], scale=spec["scale"], norm=spec["norm"])
        assert e.value.code == C.JSG_ERR_INVALID, change
    # the C entry point itself: too small a weight buffer is a size mismatch, with nnz reported
    import ctypes
    s = C.FbSpec(1024, 48000.0, 40, 0.0, 24000.0, 0, 1)
    nnz = ctypes.c_int64()
    arrs = [np.zeros(40, np.int32) for _ in range(3)] + [np.zeros(40, np.float32)]
    w = np.zeros(4, np.float32)
    rc = C.lib().jsg_filterbank_build(ctypes.byref(s), *[a.ctypes.data for a in arrs], w.ctypes.data, w.size, ctypes.byref(nnz))
    assert rc == C.JSG_ERR_SIZE_MISMATCH and nnz.value > 4


def test_from_matrix_round_trips(jsg):
    rng = np.random.default_rng(3)
    H = 513
    W = np.zeros((20, H), np.float32)
    for b in range(20):
        a = int(rng.integers(0, H - 40))
        W[b, a:a + 30] = rng.random(30).astype(np.float32) + 0.1
        W[b, a + 10] = 0.0              # interior zero
        W[b, a + 11] = -0.25            # negative weight
    W[5] = 0.0                          # empty row
    W[6, 0] = 1e-30                     # tiny weights at both ends
    W[6, H - 1] = 3.0
    fb = jsg.Filterbank.from_matrix(W)
    assert (fb.matrix().view(np.uint32) == W.view(np.uint32)).all()
    assert fb.n_bins[5] == 0 and fb.n_bins[6] == H


def test_create_matrix_refuses_before_touching_a_device(jsg):
    """jsg_filterbank_create_matrix checks its arguments before it looks for a device: these refusals hold on any machine."""
    import ctypes
    C = jsg.capi
    lib = C.lib()
    H = 513
    h = ctypes.c_void_p()
    for bad in (np.nan, np.inf, -np.inf):
        W = np.zeros((4, H), np.float32)
        W[1, 10:20] = 1.0
        W[2, 300] = bad
        assert lib.jsg_filterbank_create_matrix(ctypes.byref(h), 1024, 4, W.ctypes.data) == C.JSG_ERR_INVALID, bad
        assert not h.value
    W = np.ones((4, H), np.float32)
    assert lib.jsg_filterbank_create_matrix(ctypes.byref(h), 1000, 4, W.ctypes.data) == C.JSG_ERR_INVALID
    assert lib.jsg_filterbank_create_matrix(ctypes.byref(h), 1024, 0, W.ctypes.data) == C.JSG_ERR_INVALID
    assert lib.jsg_filterbank_create_matrix(ctypes.byref(h), 1024, 4, None) == C.JSG_ERR_INVALID


@pytest.mark.parametrize("n_fft,hop", [(512, 160), (2048, 441), (1024, 2048), (1024, 0)])
def test_mel_spectrogram_refuses_hops_that_do_not_divide_n_fft(jsg, n_fft, hop):
    import torch
    with pytest.raises(jsg.JsgError) as e:
        jsg.mel_spectrogram_db(torch.zeros(48000), 48000.0, n_fft, hop, 64)
    assert e.value.code == jsg.capi.JSG_ERR_INVALID and "divide" in str(e.value)

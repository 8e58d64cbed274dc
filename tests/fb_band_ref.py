"""Host references and seeded banks of the band-kernel tests (fb_band_kernel, csrc/jsg_filterbank.hip; include/jsg.h section 2b).  A helper:
no tests in here.

band_f32 / band_dense restate the kernel's sum (bins ascending from +0.0f, every product and every sum rounded on its own), band_f64 is the
same sum in float64, band_cap the float32 summation bound between the two.  The banks are the ones tests/test_gpu_fb_band.py runs;
tests/test_fb_band_ref.py checks references and bound on the CPU for every one of them."""
import numpy as np

FS = 48000.0
TILE_N = {8: 1024, 4: 4096, 2: 8192}          # the FFT size the edge tests use for a tile of T columns
NARROW_BANDS = (1, 255, 256, 257, 513)      # one band; one short of, exactly and one past the band loop's stride of 256 threads; a third pass


def band_f32(P, fb):
    """P [F][n/2+1] float32 -> [F][B] float32: the bank in the specified order."""
    P = np.asarray(P, np.float32)
    out = np.zeros((P.shape[0], fb.n_bands), np.float32)
    for b in range(fb.n_bands):
        acc = np.zeros(P.shape[0], np.float32)
        f, o = int(fb.first_bin[b]), int(fb.offset[b])
        for k in range(int(fb.n_bins[b])):
            acc = acc + fb.weights[o + k] * P[:, f + k]      # float32 * float32 -> rounded product; + -> rounded sum
        out[:, b] = acc
    return out


def band_dense(P, W):
    """P [F][n/2+1] -> [F][B] straight from a dense bank: bins from the first to the last nonzero of every row, ascending, float32."""
    P = np.asarray(P, np.float32)
    out = np.zeros((P.shape[0], W.shape[0]), np.float32)
    for b in range(W.shape[0]):
        nz = np.flatnonzero(W[b])
        acc = np.zeros(P.shape[0], np.float32)
        for k in range(nz[0], nz[-1] + 1) if nz.size else ():
            acc = acc + W[b, k] * P[:, k]
        out[:, b] = acc
    return out


def _band_f64(P, fb, weight):
    P = np.asarray(P, np.float32).astype(np.float64)
    out = np.zeros((P.shape[0], fb.n_bands), np.float64)
    for b in range(fb.n_bands):
        f, o, nb = int(fb.first_bin[b]), int(fb.offset[b]), int(fb.n_bins[b])
        out[:, b] = P[:, f:f + nb] @ weight(fb.weights[o:o + nb].astype(np.float64))
    return out


def band_f64(P, fb):
    """The same sums in float64 (weights and power as the float32 values they are)."""
    return _band_f64(P, fb, lambda w: w)


def band_cap(P, fb):
    """(n_bins + 1) * 2^-24 * (|W| . P), [F][B] float64: what float32 rounding of every product and every sum can move a band away from
    band_f64 of the SAME float32 power plane (the summation term of test_hardware_log_and_float64_bound; no FFT term: reference and kernel
    start from the same plane)."""
    return (fb.n_bins[None, :].astype(np.float64) + 1.0) * 2.0 ** -24 * _band_f64(np.abs(P), fb, np.abs)


def narrow_matrix(n, B, seed=0):
    """B narrow bands (1..12 bins, positive weights) anywhere on the axis; the first starts at bin 0, the last ends at bin n/2."""
    H = n // 2 + 1
    rng = np.random.default_rng(1000 * B + n + seed)
    W = np.zeros((B, H), np.float32)
    for b in range(B):
        width = int(rng.integers(1, 13))
        a = int(rng.integers(0, H - width + 1))
        if b == 0:
            a = 0
        if b == B - 1 and B > 1:
            a = H - width
        W[b, a:a + width] = rng.random(width).astype(np.float32) + 0.05
    return W


def wide_matrix(n, seed=0):
    """24 full-width rows: 24 (n/2 + 1) weights, past the 28 KB a bank may take in LDS at every FFT size."""
    H = n // 2 + 1
    return np.random.default_rng(24 + n + seed).random((24, H)).astype(np.float32) + 0.01


EDGE_ROWS = dict(empty=0, bin0=1, nyquist=2, ends_at_nyquist=3, full=4, full_zeros_inside=5, negative=6)


def edge_matrix(n, seed=0):
    """12 rows: an empty row, a one-bin band at bin 0, one at bin n/2, a band whose last bin is n/2, a full-width band, a full-width band of
    zeros between its two end weights, a band with interior zeros and a negative weight, five narrow positive bands."""
    H = n // 2 + 1
    rng = np.random.default_rng(12 + n + seed)
    W = np.zeros((12, H), np.float32)
    W[1, 0] = 1.5
    W[2, H - 1] = 0.75
    W[3, H - 20:] = rng.random(20).astype(np.float32) + 0.05
    W[4] = rng.random(H).astype(np.float32) + 0.01
    W[5, 0] = 2.0
    W[5, H - 1] = 1e-30
    a = H // 3
    W[6, a:a + 50] = rng.random(50).astype(np.float32) + 0.05
    W[6, a + 7] = 0.0
    W[6, a + 20:a + 23] = 0.0
    W[6, a + 30] = -0.5
    for b in range(7, 12):
        s = int(rng.integers(0, H - 40))
        W[b, s:s + 33] = rng.random(33).astype(np.float32) + 0.05
    return W


# the six banks of the full cases: (n, name, bank staged in LDS)
FULL_CASES = [(512, "mel40", True), (2048, "wide24", False), (4096, "mel48", True), (4096, "linear_identity", False),
              (8192, "linear48", True), (8192, "mel128", False)]


def full_bank(jsg, n, name):
    C = jsg.capi
    if name == "mel40":
        return jsg.Filterbank(n, FS, 40, 0.0, FS / 2)
    if name == "wide24":
        return jsg.Filterbank.from_matrix(wide_matrix(n))
    if name == "mel48":
        return jsg.Filterbank(n, FS, 48, 0.0, FS / 2)
    if name == "linear_identity":
        return jsg.Filterbank(n, FS, n // 2 + 1, 0.0, FS / 2, scale=C.FB_LINEAR, norm=C.FB_NORM_UNIT_SUM)
    if name == "linear48":
        return jsg.Filterbank(n, FS, 48, 100.0, 12000.0, scale=C.FB_LINEAR)
    if name == "mel128":
        return jsg.Filterbank(n, FS, 128, 0.0, FS / 2)
    raise KeyError(name)


# the banks of the band-count and band-shape edges, per tile size
EDGE_BANKS = [f"narrow{B}" for B in NARROW_BANDS] + ["edge", "mel1"]


def edge_bank(jsg, n, name):
    if name.startswith("narrow"):
        return jsg.Filterbank.from_matrix(narrow_matrix(n, int(name[6:])))
    if name == "edge":
        return jsg.Filterbank.from_matrix(edge_matrix(n))
    if name == "mel1":
        return jsg.Filterbank(n, FS, 1, 0.0, FS / 2)
    raise KeyError(name)


def power_plane(F, n, seed=0):
    """A positive random power plane [F][n/2+1] float32: the power of complex Gaussian bins under a random envelope over 60 dB."""
    H = n // 2 + 1
    rng = np.random.default_rng(77 + n + seed)
    g = rng.standard_normal((2, F, H))
    env = 10.0 ** (-6.0 * rng.random(H))
    return ((g[0] ** 2 + g[1] ** 2) * env[None, :] * n).astype(np.float32)


def prime_factors(x):
    out, d = [], 2
    while d * d <= x:
        while x % d == 0:
            out.append(d)
            x //= d
        d += 1
    if x > 1:
        out.append(x)
    return out


def split_columns(n_cols):
    """n_cols = batches * channels * frames for a per-channel call: the smallest prime factor (where it is at most 16 and not the only one)
    becomes the channels, the next the batches, the rest the frames of a row.  A prime n_cols is one row."""
    f = prime_factors(n_cols)
    channels = f.pop(0) if len(f) > 1 and f[0] <= 16 else 1
    batches = f.pop(0) if len(f) > 1 else 1
    return batches, channels, int(np.prod(f, dtype=np.int64))

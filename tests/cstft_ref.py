"""References, yardsticks and bounds for the complex STFT / inverse STFT (include/jsg.h section 2d).  Plain numpy (scipy's pocketfft
for the single-precision yardstick, torch.fft on the CPU where scipy is missing); importable without a GPU.

Forward.  Reference: float64 rfft of the *float32* windowed frames (the kernel rounds x * w to float32 once, so does the reference).
Metric, per frame: e = max_k |X[k] - X_ref[k]| / max_k |X_ref[k]| -- every bin has the same weight, a wrong weak bin shows.
Yardstick Y: the same metric for a single-precision CPU FFT on the same float32 frames, the largest over the frames of the call; it
is measured when the test runs, never a constant.  Bound: e <= M * Y.

Inverse.  Reference: float64 irfft (imaginary parts of bins 0 and n/2 dropped), times w, overlap-added, divided by the float64
envelope, 0 where the envelope is <= 1e-11.  Bound, per output sample t with a live envelope:

    |y[t] - y_ref[t]| <= (M * Y_inv * B[t] + (c[t] + 3) * 2^-24 * A[t]) / env[t]

B[t] = sum_j peak_j |w[t - j hop]| (peak_j = largest |sample| of frame j's float64 irfft), A[t] = sum_j |frame_j[t - j hop] w|, c[t] =
the number of covering frames, Y_inv = the yardstick's max_t |frame32 - frame64| / peak over the call's frames.  The first term is
each covering frame's transform error, the second the float32 roundings of * 1/n, * w, the ascending sum and the final product.

M = 2.  A numpy float32 restatement of the forward kernel (tests/test_cstft_ref.py) sits at e / Y = 1.00 .. 1.36 over all sizes and
input classes; the GPU, which contracts multiply-adds, is measured by tools/cstft_accuracy.py (profiles/cstft_accuracy.md): the rule
is M = 2 while the worst measured ratio is at most 1.6, and never more than 3.  An off-by-one twiddle is at 2 pi / n, three orders of
magnitude above either.
"""
from collections import namedtuple

import numpy as np

M = 2.0
SIZES = (512, 1024, 2048, 4096, 8192)
ENV_EPS = 1e-11
U24 = 2.0 ** -24

try:
    import scipy.fft as _sfft

    def rfft32(frames32):
        return _sfft.rfft(np.ascontiguousarray(frames32, np.float32), axis=-1)

    def irfft32(X64c, n):
        return _sfft.irfft(np.ascontiguousarray(X64c, np.complex64), n, axis=-1)
except ImportError:   # the same pocketfft family through torch on the CPU
    import torch as _torch

    def rfft32(frames32):
        return _torch.fft.rfft(_torch.from_numpy(np.ascontiguousarray(frames32, np.float32)), dim=-1).numpy()

    def irfft32(X64c, n):
        return _torch.fft.irfft(_torch.from_numpy(np.ascontiguousarray(X64c, np.complex64)), n, dim=-1).numpy()


# ------------------------------------------------------------------------------------------------ windows and input classes
def window(kind, n):
    m = np.arange(n, dtype=np.float64)
    if kind == "rect":
        w = np.ones(n)
    elif kind == "hann":
        w = 0.5 - 0.5 * np.cos(2 * np.pi * m / n)
    elif kind == "blackman":
        w = 0.42 - 0.5 * np.cos(2 * np.pi * m / n) + 0.08 * np.cos(4 * np.pi * m / n)
    elif kind == "ramp":      # asymmetric, no zeros
        w = 0.25 + 0.75 * m / n
    else:
        raise ValueError(kind)
    return w.astype(np.float32)


def noise(rows, L, seed):
    return np.random.default_rng(seed).standard_normal((rows, L)).astype(np.float32)


def impulse(n):
    """One impulse, hop 1, n frames: frame j sees it at position n - 1 - j.  Returns (x [1][2n-1], hop, F)."""
    x = np.zeros((1, 2 * n - 1), np.float32)
    x[0, n - 1] = 1.0
    return x, 1, n


def tones(n, L, seed):
    """Row k: cos(2 pi k t / n + phase_k), k = 0..n/2, the angle reduced exactly before the cosine."""
    ph = np.random.default_rng(seed).uniform(0, 2 * np.pi, n // 2 + 1)
    kt = (np.arange(n // 2 + 1, dtype=np.int64)[:, None] * np.arange(L, dtype=np.int64)[None, :]) % n
    return np.cos(2 * np.pi * kt / n + ph[:, None]).astype(np.float32)


def impulse_closed_form(n, w, frames):
    """X[j][k] = w[m] W_n^(k m), m = n - 1 - j, in float64 with the angle reduced exactly."""
    m = n - 1 - np.asarray(frames, dtype=np.int64)
    km = (m[:, None] * np.arange(n // 2 + 1, dtype=np.int64)[None, :]) % n
    return w.astype(np.float64)[m][:, None] * np.exp(-2j * np.pi * km / n)


FORWARD_CLASSES = ("noise_rect", "noise_hann", "impulses", "impulses_ramp", "tones")


def forward_class(cls, n, small=False):
    """(x [rows][L], hop, F, w) of an input class.  small: a thinned version for the CPU (impulses at 256 positions with both ends,
    one per row in place of one per frame; every 16th tone with both ends), the full one otherwise."""
    if cls == "noise_rect":
        hop, F = n // 4, 24
        return noise(3, (F - 1) * hop + n, n + 1), hop, F, window("rect", n)
    if cls == "noise_hann":
        hop, F = 441, 24
        return noise(3, (F - 1) * hop + n, n + 2), hop, F, window("hann", n)
    if cls in ("impulses", "impulses_ramp"):
        w = window("rect" if cls == "impulses" else "ramp", n)
        if not small:
            return impulse(n) + (w,)
        pos = np.unique(np.concatenate([np.arange(8), np.arange(n - 8, n), np.random.default_rng(n).integers(0, n, 240)]))
        x = np.zeros((pos.size, n), np.float32)
        x[np.arange(pos.size), pos] = 1.0
        return x, n, 1, w
    if cls == "tones":
        hop, F = 441, 2
        x = tones(n, (F - 1) * hop + n, n + 3)
        if small:
            x = x[np.unique(np.concatenate([np.arange(0, n // 2 + 1, 16), [1, n // 2 - 1, n // 2]]))]
        return x, hop, F, window("rect", n)
    raise ValueError(cls)


# ------------------------------------------------------------------------------------------------ forward
def frames_f32(x, n, hop, f0, f1, w):
    """The float32 windowed frames f0..f1-1 of every row: [rows][f1-f0][n]."""
    v = np.lib.stride_tricks.sliding_window_view(x, n, axis=1)[:, f0 * hop:(f1 - 1) * hop + 1:hop]
    return v * w.astype(np.float32)[None, None, :]


def forward_f64(x, n, hop, F, w, f0=0):
    """float64 rfft of the float32 windowed frames f0..F-1: [rows][F-f0][n/2+1] complex128."""
    return np.fft.rfft(frames_f32(x, n, hop, f0, F, w).astype(np.float64), axis=-1)


def frame_metric(X, ref):
    """(e [rows][frames], worst bin [rows][frames]): e = max_k |X - ref| / max_k |ref|; a zero reference frame gives 0 if X is
    zero too, else inf."""
    d = np.abs(X.astype(np.complex128) - ref)
    top = np.abs(ref).max(axis=-1)
    worst = d.max(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(top > 0, worst / top, np.where(worst > 0, np.inf, 0.0))
    e = np.where(np.isnan(worst), np.inf, e)
    return e, d.argmax(axis=-1)


ForwardFigures = namedtuple("ForwardFigures", "e Y ratio row frame bin")


def forward_figures(X, x, n, hop, w, frames=None, slice_frames=None):
    """e (the largest over the frames looked at), the yardstick Y over the same frames, e / Y and where e sits.  X: [rows][F][n/2+1]
    from the code under test.  frames: the frame indices to look at (default all); the work goes in slices of slice_frames frames
    so that the host holds about 0.25 GB of float64 at a time."""
    rows, F = X.shape[0], X.shape[1]
    if slice_frames is None:
        slice_frames = max(1, (1 << 24) // (rows * n))
    keep = None if frames is None else np.zeros(F, bool)
    if keep is not None:
        keep[np.asarray(frames)] = True
    best = (-1.0, 0, 0, 0)
    Y = 0.0
    for f0 in range(0, F, slice_frames):
        f1 = min(F, f0 + slice_frames)
        sel = slice(None) if keep is None else keep[f0:f1]
        if keep is not None and not keep[f0:f1].any():
            continue
        fr = frames_f32(x, n, hop, f0, f1, w)[:, sel]
        ref = np.fft.rfft(fr.astype(np.float64), axis=-1)
        e, kb = frame_metric(X[:, f0:f1][:, sel], ref)
        Y = max(Y, float(frame_metric(rfft32(fr), ref)[0].max()))
        r, j = np.unravel_index(int(np.argmax(e)), e.shape)
        if e[r, j] > best[0]:
            fidx = np.arange(f0, f1)[sel][j]
            best = (float(e[r, j]), int(r), int(fidx), int(kb[r, j]))
    return ForwardFigures(best[0], Y, best[0] / Y if Y > 0 else (0.0 if best[0] == 0 else np.inf), best[1], best[2], best[3])


def assert_forward(X, x, n, hop, w, what, frames=None, m=None):
    m = M if m is None else m
    g = forward_figures(X, x, n, hop, w, frames)
    print(f"{what}: e={g.e:.3g} Y={g.Y:.3g} ratio={g.ratio:.3f}")
    assert g.e <= m * g.Y, (f"{what}: e = {g.e:.3g} > {m} * Y = {m * g.Y:.3g} at row {g.row}, frame {g.frame}, bin {g.bin} "
                            f"(n={n}, hop={hop})")
    return g


# ------------------------------------------------------------------------------------------------ inverse
InverseRef = namedtuple("InverseRef", "y env B A c")


def drop_unread_imag(X):
    X = np.array(X, dtype=np.complex128)
    X[..., 0] = X[..., 0].real
    X[..., -1] = X[..., -1].real
    return X


def inverse_f64(X, n, hop, w, T):
    """X [rows][F][n/2+1] -> InverseRef of [rows][T] arrays (env, c: [T]); T <= (F-1) hop + n."""
    rows, F = X.shape[0], X.shape[1]
    span = (F - 1) * hop + n
    assert 1 <= T <= span
    w64 = w.astype(np.float64)
    fr = np.fft.irfft(drop_unread_imag(X), n, axis=-1)
    peak = np.abs(fr).max(axis=-1)
    fr *= w64
    y, B, A = np.zeros((rows, span)), np.zeros((rows, span)), np.zeros((rows, span))
    env, c = np.zeros(span), np.zeros(span)
    aw, w2 = np.abs(w64), w64 * w64
    for j in range(F):
        s = slice(j * hop, j * hop + n)
        y[:, s] += fr[:, j]
        A[:, s] += np.abs(fr[:, j])
        B[:, s] += peak[:, j, None] * aw
        env[s] += w2
        c[s] += 1
    live = env > ENV_EPS
    y = np.where(live, y / np.where(live, env, 1.0), 0.0)
    return InverseRef(y[:, :T], env[:T], B[:, :T], A[:, :T], c[:T])


def slice_ref(ref, lo, hi):
    return InverseRef(ref.y[:, lo:hi], ref.env[lo:hi], ref.B[:, lo:hi], ref.A[:, lo:hi], ref.c[lo:hi])


def inverse_yardstick(X, n):
    """Y_inv: max_t |frame32 - frame64| / peak over the frames of X (frames whose float64 irfft is zero do not count)."""
    f64 = np.fft.irfft(drop_unread_imag(X), n, axis=-1)
    f32 = irfft32(X, n).astype(np.float64)
    peak = np.abs(f64).max(axis=-1)
    d = np.abs(f32 - f64).max(axis=-1)
    ok = peak > 0
    return float((d[ok] / peak[ok]).max()) if ok.any() else 0.0


def small_odd_hop(n):
    return 7 if n == 512 else 61


def inverse_cases(n):
    """(window, hop, F) of the overlap-add cases: F = 40 frames, or 40 more than the floor((n-1)/hop) + 1 that cover one sample
    where the hop is small, so that a call with the smallest scratch runs in 40 chunks."""
    so = small_odd_hop(n)
    return [("hann", n // 4, 40), ("blackman", n // 4, 40), ("hann", n // 2, 40), ("rect", n // 2, 40), ("hann", 441, 40),
            ("rect", 441, 40), ("rect", n - 1, 40), ("rect", n, 40), ("hann", so, (n - 1) // so + 1 + 40), ("rect", so, (n - 1) // so + 1 + 40)]


def random_bins(rows, F, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, F, n // 2 + 1)) + 1j * rng.standard_normal((rows, F, n // 2 + 1))).astype(np.complex64)


def basis_bins(n):
    """[1][2 (n/2+1)][n/2+1]: frame k a unit in the real part of bin k, frame n/2+1+k a unit in its imaginary part."""
    B = n // 2 + 1
    X = np.zeros((1, 2 * B, B), np.complex64)
    X[0, np.arange(B), np.arange(B)] = 1.0
    X[0, B + np.arange(B), np.arange(B)] = 1.0j
    return X


InverseFigures = namedtuple("InverseFigures", "ratio row t err tol dead")


def inverse_figures(y, ref, Y_inv, m=None):
    """The worst err / tol over every sample with a live envelope, where it sits, and the number of dead samples per row (which must
    be exactly 0 in y: a dead sample that is not 0 gives ratio inf)."""
    m = M if m is None else m
    live = ref.env > ENV_EPS
    y = y.astype(np.float64)
    err = np.abs(y - ref.y)
    err = np.where(np.isnan(err), np.inf, err)
    tol = (m * Y_inv * ref.B + (ref.c + 3) * U24 * ref.A) / np.where(live, ref.env, 1.0)
    q = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))   # tol 0: an all-zero frame set
    q = np.where(live[None, :], q, np.where(y == 0.0, 0.0, np.inf))
    r, t = np.unravel_index(int(np.argmax(q)), q.shape)
    return InverseFigures(float(q[r, t]), int(r), int(t), float(err[r, t]), float(tol[r, t]), int((~live).sum()))


def assert_inverse(y, ref, Y_inv, what, n, hop, m=None, dead_cap=None):
    g = inverse_figures(y, ref, Y_inv, m)
    print(f"{what}: err/tol={g.ratio:.3f} Y_inv={Y_inv:.3g} dead={g.dead}")
    assert g.ratio <= 1.0, (f"{what}: |y - ref| = {g.err:.3g} > tol = {g.tol:.3g} at row {g.row}, sample {g.t} (frames "
                            f"{max(0, -(-(g.t - n + 1) // hop))}..{g.t // hop}, offset {g.t % hop} past a hop; env {ref.env[g.t]:.3g}; n={n}, hop={hop})")
    if dead_cap is not None:
        assert g.dead <= dead_cap, f"{what}: {g.dead} samples with a dead envelope, more than {dead_cap}"
    return g

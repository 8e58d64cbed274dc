"""Phase vocoder (include/jsg.h section 2e): the float64 reference of the definition, a float32 numpy restatement of the library's
arithmetic, the bounds, and the seeded inputs the tests share.  A helper, no tests."""
import functools

import numpy as np

TWO_PI = 2.0 * np.pi


def n_frames_out(T: int, rate: float) -> int:
    """#{i >= 0 : float(i) * rate < T}, by the definition (one IEEE multiply per i), without the library."""
    rate = float(rate)
    g = max(0, int(np.ceil(T / rate)) - 3)
    while g > 0 and float(g - 1) * rate >= T:
        g -= 1
    while float(g) * rate < T:
        g += 1
    return g


def _grid(T: int, rate: float):
    """j = floor(t_i) and alpha = float32(t_i - j) for every output frame."""
    t = np.arange(n_frames_out(T, rate), dtype=np.float64) * np.float64(rate)
    j = np.floor(t).astype(np.int64)
    return j, (t - j).astype(np.float32)


def reference(X: np.ndarray, rate: float, hop: int, n: int) -> np.ndarray:
    """The definition in float64 with the unreduced A_k = 2 pi hop k / n: X [T][K] complex -> [T_out][K] complex128."""
    X = np.asarray(X).astype(np.complex128)
    T, K = X.shape
    assert K == n // 2 + 1
    j, alpha = _grid(T, rate)
    Xp = np.concatenate([X, np.zeros((2, K), np.complex128)])
    a0, a1 = Xp[j], Xp[j + 1]
    al = alpha.astype(np.float64)[:, None]
    mag = al * np.abs(a1) + (1.0 - al) * np.abs(a0)
    A = TWO_PI * hop * np.arange(K, dtype=np.float64) / n
    x = np.angle(a1) - np.angle(a0) - A
    d = x - TWO_PI * np.round(x / TWO_PI) + A
    phi = np.angle(X[0])[None, :] + np.concatenate([np.zeros((1, K)), np.cumsum(d[:-1], axis=0)])
    return mag * (np.cos(phi) + 1j * np.sin(phi))


def _angle(z: np.ndarray) -> np.ndarray:
    return np.arctan2(z.imag, z.real)


def restatement(X: np.ndarray, rate: float, hop: int, n: int, *, angle=_angle, modulus=np.abs) -> np.ndarray:
    """The library's arithmetic in numpy: float32 arctan2, the phase in uint32 fixed point (2^32 units per turn), float32 cos / sin.
    X [T][K] complex64 -> [T_out][K] complex64.  Not bit-exact with the device (atan2f and sincosf are the device library's).
    `angle` and `modulus` (complex64 array -> float32 array) stand for atan2f and hypotf: the tests put faulty ones in their place."""
    X = np.asarray(X).astype(np.complex64)
    T, K = X.shape
    assert K == n // 2 + 1
    f32 = np.float32
    j, alpha = _grid(T, rate)
    Xp = np.concatenate([X, np.zeros((2, K), np.complex64)])
    ang = angle(Xp).astype(f32)
    mod = modulus(Xp).astype(f32)
    al = alpha[:, None]
    mag = (al * mod[j + 1]).astype(f32) + ((f32(1) - al) * mod[j]).astype(f32)
    inv = f32(1.0 / TWO_PI)
    adv = ((hop * np.arange(K, dtype=np.int64)) % n).astype(np.float64) / np.float64(n)
    u = ((ang[j + 1] - ang[j]).astype(f32) * inv).astype(f32).astype(np.float64)
    u = u - adv
    u = u - np.round(u)
    u = u + adv
    mask = np.int64(0xFFFFFFFF)
    inc = np.rint(u * 4294967296.0).astype(np.int64) & mask
    phi0 = np.rint((ang[0] * inv).astype(f32).astype(np.float64) * 4294967296.0).astype(np.int64) & mask
    acc = (phi0[None, :] + np.concatenate([np.zeros((1, K), np.int64), np.cumsum(inc[:-1], axis=0)])) & mask
    ph = acc.astype(np.uint32).view(np.int32).astype(f32) * f32(TWO_PI / 4294967296.0)
    return ((mag * np.cos(ph).astype(f32)).astype(f32) + 1j * (mag * np.sin(ph).astype(f32)).astype(f32)).astype(np.complex64)


def bound_restatement(T_out: int) -> np.ndarray:
    """What the restatement keeps against float64, relative per element, for output frame i: 2^-21 + (i+1) 2^-20."""
    return 2.0 ** -21 + (np.arange(T_out, dtype=np.float64) + 1.0) * 2.0 ** -20


# Bound (a): the device's worst relative error on a case may be this many times the restatement's worst on the same case.  Chosen as 4
# before any run; the first runs on an MI355X gave at most 1.47 on the cases of profiles/pvoc_accuracy.md and 1.54 on the other inputs
# of the GPU tests, and 1.25 times that, rounded up to the next half, is 2.
YARDSTICKS = 2.0


def bound_cap(T_out: int) -> np.ndarray:
    """The analytic cap for the device, output frame i: 2^-20 + (i+1) 3 2^-20 (two angles at up to 4 ulp of pi each per step, plus
    the subtraction and the scaling; 2^-20 for the magnitude and sincosf)."""
    return 2.0 ** -20 + (np.arange(T_out, dtype=np.float64) + 1.0) * 3.0 * 2.0 ** -20


def rel_error(Y: np.ndarray, R: np.ndarray) -> np.ndarray:
    """|Y - R| / max(|R|, 2^-100) per element."""
    return np.abs(np.asarray(Y).astype(np.complex128) - R) / np.maximum(np.abs(R), 2.0 ** -100)


@functools.lru_cache(maxsize=8)
def make_input(n: int, hop: int, T: int, seed: int = 0) -> np.ndarray:
    """The complex64 STFT (periodic Hann window, T frames at `hop`) of seeded noise plus a tone, with exact zeros: bins 3 and K-2 of
    every frame (where K >= 5, so that n = 2 and 4 keep bins that are not zero), a scattering of single bins, and one whole frame
    (where T > 4).  Read-only: the tests share it."""
    rng = np.random.default_rng(seed + 1000003 * n + 7919 * hop + T)
    L = (T - 1) * hop + n
    s = np.arange(L, dtype=np.float64)
    x = (0.3 * rng.standard_normal(L) + np.sin(TWO_PI * 0.0617 * s + 0.3)).astype(np.float32)
    w = (0.5 - 0.5 * np.cos(TWO_PI * np.arange(n) / n)).astype(np.float32)
    idx = (np.arange(T) * hop)[:, None] + np.arange(n)[None, :]
    X = np.fft.rfft((x[idx] * w[None, :]).astype(np.float64), axis=1).astype(np.complex64)
    K = n // 2 + 1
    if K >= 5:
        X[:, 3] = 0
        X[:, K - 2] = 0
    X[rng.integers(0, T, 4 * T), rng.integers(0, K, 4 * T)] = 0
    if T > 4:
        X[T // 3] = 0
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=8)
def special_input(n: int, T: int, seed: int = 0) -> np.ndarray:
    """complex64 [T][K] of the values where atan2f and hypotf go wrong, read-only and shared like make_input: random phases at
    magnitudes 2^e U(0.5, 1) with e uniform in -90..126 (x * x underflows or overflows at either end, every modulus is finite); about
    a quarter of the elements on the eight directions 1, i, -1, -i, +-1 +- i times 2^-40..2^40 (angles that are exact multiples of
    pi / 4, +-pi among them, so differences sit on the ties of the wrap; a zero part of such an element has either sign); about
    15 % zeros with all four combinations of signs (arg(-0 + 0j) = pi, arg(-0 - 0j) = -pi), written through the float32 view."""
    rng = np.random.default_rng(seed + 1000003 * n + 7919 * T + 104729)
    K = n // 2 + 1
    mag = np.ldexp(rng.uniform(0.5, 1.0, (T, K)), rng.integers(-90, 127, (T, K)))
    X = (mag * np.exp(1j * rng.uniform(-np.pi, np.pi, (T, K)))).astype(np.complex64)
    v = X.view(np.float32).reshape(T, K, 2)

    def signed(shape):
        return np.where(rng.integers(0, 2, shape) == 1, np.float32(-1), np.float32(1))

    dirs = np.array([[1, 0], [0, 1], [-1, 0], [0, -1], [1, 1], [1, -1], [-1, 1], [-1, -1]], np.float32)
    on = rng.random((T, K)) < 0.25
    d = dirs[rng.integers(0, 8, int(on.sum()))]
    d = np.where(d == 0, np.float32(0) * signed(d.shape), d)
    v[on] = np.ldexp(d, rng.integers(-40, 41, (d.shape[0], 1))).astype(np.float32)
    zero = rng.random((T, K)) < 0.15
    v[zero] = np.float32(0) * signed((int(zero.sum()), 2))
    X.setflags(write=False)
    return X


def frames_for(rate: float, about: int = 2000) -> int:
    """T such that T_out is about `about`."""
    return max(1, int(round(about * rate)))


RATES = (0.5, 0.8, 1.0, 1 / 0.9, 1.3, 2.0)


def accuracy_cases():
    """(n, hop, rate, T) of the GPU accuracy check: K = 257 / 1025 (every 64-bin tile ends ragged), hops n/4 and 100, about 2000
    output frames; then one input frame, and a rate beyond the input (one output frame)."""
    cases = [(n, hop, rate, frames_for(rate)) for n in (512, 2048) for hop in (n // 4, 100) for rate in RATES]
    cases += [(512, 128, rate, 1) for rate in RATES]
    cases += [(2048, 100, 3.5, 3), (512, 100, 1000.0, 7)]
    return cases


def case_id(case) -> str:
    n, hop, rate, T = case
    return f"n{n}-hop{hop}-rate{rate:.4g}-T{T}"


def edge_cases():
    """(n, hop, rate, T, kind), kind "noise" (make_input) or "special" (special_input): K = 2, 3, 64, 65, 66 (one partial tile, a
    full last tile, one live lane in the last tile) at hops n/4, n and 1 with about 300 output frames; the largest n (K = 32769, 513
    tiles) at hop n - 1; rates far below 0.5 (many outputs share a pair), above 2 (pairs are skipped, some steps still move by
    one) and within 2^-30 of 1, about 1000 output frames."""
    kinds = ("noise", "special")
    small = [(n, max(1, n // 4)) for n in (2, 4, 126, 128, 130)] + [(126, 126), (126, 1)]
    cases = [(n, hop, rate, frames_for(rate, 300), kind) for n, hop in small for rate in (0.8, 1.0, 1.3) for kind in kinds]
    cases += [(65536, 65535, rate, 6, kind) for rate in (0.38, 2.0) for kind in kinds]
    cases += [(512, 128, rate, frames_for(rate, 1000), kind) for rate in (0.1, 1 / 3, 2.5, 3.5, 1 - 2.0 ** -30, 1 + 2.0 ** -30) for kind in kinds]
    return cases


def edge_id(case) -> str:
    n, hop, rate, T, kind = case
    return f"{kind}-n{n}-hop{hop}-rate{rate:.10g}-T{T}"


def edge_input(case, seed: int = 0) -> np.ndarray:
    n, hop, rate, T, kind = case
    return special_input(n, T, seed) if kind == "special" else make_input(n, hop, T, seed)


def accuracy_figures(X, Y, rate, hop, n):
    """Against the float64 reference R: the restatement's worst relative error (the yardstick of bound (a)), the device result's
    worst relative error, its worst ratio to the per-frame cap (b), and whether every element with R = 0 is exactly zero."""
    R = reference(X, rate, hop, n)
    yard = float(rel_error(restatement(X, rate, hop, n), R).max())
    err = rel_error(Y, R)
    zeros_exact = bool((np.asarray(Y)[np.abs(R) == 0] == 0).all())
    return dict(yardstick=yard, worst=float(err.max()), cap_ratio=float((err / bound_cap(R.shape[0])[:, None]).max()),
                zeros_exact=zeros_exact, n_zero=int((np.abs(R) == 0).sum()), n_nonzero=int((np.abs(R) > 0).sum()))

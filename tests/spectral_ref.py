"""Spectral shape descriptors (include/jsg.h section 2l): the definitions evaluated in float64, the float32 restatement in the library's
stated orders, the stated bounds, the shared planes.  numpy only (the logarithm is oracle/mirror's exact_db: the library's own source
line by line); tests/test_spectral_ref.py checks this module on the CPU, tests/test_gpu_spectral.py compares the GPU against it.

The restatement: the lane sum of section 2j (lane l of W takes k = l, l + W, ... ascending, then a halving tree) for E, N1 (fmaf), L
and M2 (fmaf); mx by "v > mx or v is NaN" from +0; the prefix sum in chunks of W bins, an inclusive scan by steps 1, 2, 4, ... within a
chunk and a chain of bases across chunks; k* the lowest k with cum[k] >= fl(p * cum[K-1]).  The float32 fmaf is the exact emulation of
tests/rhythm_ref.py.
"""
import functools

import numpy as np

from rhythm_ref import U, fma32

FLOATS = ("energy", "centroid", "spread", "rolloff", "flatness_db", "crest")
OUTPUTS = ("energy", "centroid", "spread", "rolloff", "rolloff_bin", "flatness_db", "crest")
# K <= 64 * this: the register path of that name (jsg_spectral_shape_plan); above the last, "spectral_stream"
REGS = (1, 2, 4, 9, 17, 33, 65)
IN_FLIGHT = {1: 8, 2: 8, 4: 4, 9: 2, 17: 2, 33: 1, 65: 1}


def lanes(K):
    return 64 if K > 32 else 1 << max(0, (K - 1).bit_length())


def plan(K):
    """(path, lanes per frame, frames a group has in flight) that jsg_spectral_shape_plan must name for K bins."""
    W = lanes(K)
    nc = -(-K // W)
    for n in REGS:
        if nc <= n:
            return f"spectral_regs{n}", W, IN_FLIGHT[n]
    return "spectral_stream", W, 1


@functools.lru_cache(maxsize=None)
def _mirror():
    from oracle import mirror
    return mirror.load()


def exact_db(p):
    p = np.asarray(p, np.float32)
    return _mirror().exact_db(p).reshape(p.shape)


def _chunked(a, W):
    """[..., K] -> [..., nc, W], bins past K as +0."""
    K = a.shape[-1]
    nc = -(-K // W)
    out = np.zeros(a.shape[:-1] + (nc * W,), a.dtype)
    out[..., :K] = a
    return out.reshape(a.shape[:-1] + (nc, W))


def _tree(acc, op=lambda a, b: a + b):
    s = acc.shape[-1] // 2
    while s >= 1:
        acc = op(acc[..., :s], acc[..., s:2 * s])
        s //= 2
    return acc[..., 0]


def _keep_nan_max(a, b):
    return np.where((b > a) | np.isnan(b), b, a)


def shape32(S, f, roll=0.85):
    """The float32 restatement: S [..., T, K] float32, f [K] float32 -> dict of [..., T] arrays (rolloff_bin int32; N1, which the
    library does not return, for its bound)."""
    S, f = np.asarray(S, np.float32), np.asarray(f, np.float32)
    K = S.shape[-1]
    W = lanes(K)
    x, fc = _chunked(S, W), _chunked(f, W)
    nc = x.shape[-2]
    ok = (np.arange(nc * W) < K).reshape(nc, W)
    Kf = np.float32(K)
    zero = np.zeros(x.shape[:-2] + (W,), np.float32)
    with np.errstate(all="ignore"):
        E, N1, mx, L = zero.copy(), zero.copy(), zero.copy(), zero.copy()
        for j in range(nc):
            v = x[..., j, :]
            E = np.where(ok[j], E + v, E)
            N1 = np.where(ok[j], fma32(fc[j], v, N1), N1)
            mx = np.where(ok[j], _keep_nan_max(mx, v), mx)
            L = np.where(ok[j], L + exact_db(v), L)
        E, N1, L, mx = _tree(E), _tree(N1), _tree(L), _tree(mx, _keep_nan_max)
        none = E == 0
        c = np.where(none, np.float32(0), N1 / E).astype(np.float32)
        M2 = zero.copy()
        for j in range(nc):
            d = fc[j] - c[..., None]
            M2 = np.where(ok[j], fma32(d * d, x[..., j, :], M2), M2)
        M2 = _tree(M2)
        spread = np.where(none, np.float32(0), np.sqrt(M2 / E)).astype(np.float32)
        crest = np.where(none, np.float32(0), mx / (E / Kf)).astype(np.float32)
        flat = (L / Kf - exact_db(E / Kf)).astype(np.float32)
        # the prefix sum
        sc = x.copy()
        s = 1
        while s < W:
            nxt = sc.copy()
            nxt[..., s:] = sc[..., s:] + sc[..., :-s]
            sc = nxt
            s *= 2
        cum = np.empty_like(sc)
        base = np.zeros(x.shape[:-2], np.float32)
        for j in range(nc):
            cum[..., j, :] = base[..., None] + sc[..., j, :]
            base = base + sc[..., j, W - 1]
        cum = cum.reshape(cum.shape[:-2] + (nc * W,))[..., :K]
        thr = (np.float32(roll) * cum[..., K - 1]).astype(np.float32)
        ge = cum >= thr[..., None]
        k = np.where(ge.any(axis=-1), ge.argmax(axis=-1), K - 1)
        nan = np.isnan(thr)
        rolloff = np.where(nan, np.float32(np.nan), f[k]).astype(np.float32)
        k = np.where(nan, -1, k).astype(np.int32)
    return dict(energy=E, centroid=c, spread=spread, rolloff=rolloff, rolloff_bin=k, flatness_db=flat, crest=crest, N1=N1)


def shape64(S, f, roll=0.85):
    """The plain formulas in float64 on the float32 inputs (finite, non-negative S): dict as shape32, plus N1."""
    S, f = np.asarray(S, np.float32).astype(np.float64), np.asarray(f, np.float32).astype(np.float64)
    K = S.shape[-1]
    with np.errstate(all="ignore"):
        E = S.sum(axis=-1)
        N1 = (S * f).sum(axis=-1)
        none = E == 0
        c = np.where(none, 0.0, N1 / E)
        spread = np.where(none, 0.0, np.sqrt((S * (f - c[..., None]) ** 2).sum(axis=-1) / E))
        crest = np.where(none, 0.0, S.max(axis=-1) / (E / K))
        flat = (10 * np.log10(S + 1e-11)).mean(axis=-1) - 10 * np.log10(E / K + 1e-11)
        cum = np.cumsum(S, axis=-1)
        k = (cum >= (np.float64(np.float32(roll)) * cum[..., -1])[..., None]).argmax(axis=-1)
    return dict(energy=E, N1=N1, centroid=c, spread=spread, rolloff=f[k], rolloff_bin=k.astype(np.int32), flatness_db=flat, crest=crest)


def bounds(K):
    """The relative bounds of section 2l on E, N1 and the centroid (f >= 0): n = ceil(K / W) + log2 W roundings of non-negative terms."""
    W = lanes(K)
    n = -(-K // W) + (W.bit_length() - 1)
    return dict(energy=(n + 1) * U, N1=(n + 1) * U, centroid=(2 * n + 4) * U)


def freqs(K, step=None):
    """float32 [K]: k * step, the FFT bins of 22 050 Hz where step is None.  Read-only."""
    step = 11025.0 / max(K - 1, 1) if step is None else step
    f = (np.arange(K, dtype=np.float64) * step).astype(np.float32)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def planes(R=3, T=70, K=257, seed=0):
    """[R][T][K] float32 power-like planes: exponentially distributed values under a spectral tilt, a few exact zeros, row 1 with a
    moving peak 40 dB above the rest, row 2 scaled down by 1e-6.  Read-only."""
    rng = np.random.default_rng(20261020 + seed + 1000 * K + T)
    S = rng.exponential(1.0, (R, T, K)) * np.exp(-3.0 * np.arange(K) / K)
    S[rng.random((R, T, K)) < 0.02] = 0.0
    if R > 1:
        S[1, np.arange(T), (np.arange(T) * 7) % K] += 1e4
    if R > 2:
        S[2] *= 1e-6
    S = S.astype(np.float32)
    S.setflags(write=False)
    return S


def raw(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(raw(a), raw(b))


def same_but_nan(a, b):
    """same(), with a NaN of any sign and payload equal to any other NaN."""
    if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    return same(np.where(np.isnan(a), np.float32(0), a), np.where(np.isnan(b), np.float32(0), b))


def same_outputs(got, want, names=OUTPUTS):
    """The names whose bits differ (NaN of any payload equal), empty where all agree."""
    return [n for n in names if not (np.array_equal(got[n], want[n]) and got[n].dtype == want[n].dtype if n == "rolloff_bin" else same_but_nan(got[n], want[n]))]

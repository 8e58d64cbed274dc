"""Constant-Q / variable-Q spectrograms by direct evaluation (include/jsg.h section 2h): the standard basis in double, the definition
evaluated in float64, the float32 restatement in the library's stated order, the per-element cap, the shared inputs and the case list.
numpy only; tests/test_cqt_ref.py checks this module on the CPU, tests/test_gpu_cqt.py compares the GPU against it.

The restatement: with W = 64 where a bin has more than 32 taps, else the smallest power of two >= its taps, lane l of W takes the live
taps i = l, l + W, ... in ascending order with a fused multiply-add into its own accumulator (re and im apart), then a halving tree
W/2, ..., 1.  A float32 fmaf is emulated as a float64 multiply-add rounded to float32; the rare double rounding is why the restatement
is a yardstick and not a bit mirror.
"""
import functools

import numpy as np

# bound (a) of tests/test_gpu_cqt.py: GPU error <= YARDSTICKS x the restatement's error on the same case, both relative to the row's
# peak.  4 before any GPU run; afterwards 1.25 x the worst measured ratio, rounded up to the next half (the rule of
# profiles/stft_power_accuracy.md).  Measured on an MI355X: the worst ratio over the cases of tools/cqt_accuracy.py is 1.000 (the GPU's
# bits equal the restatement's in every component; profiles/cqt_accuracy.md), so 1.25 x 1.000 rounded up to the next half.
YARDSTICKS = 1.5

C1 = 32.70319566257483
L = 3000
SYNTH_HALF = (0, 1, 31, 32, 33, 63, 64, 100, 1000)
HOPS = (1, 7, 64, 512, 5000)
STANDARD = dict(fs=22050.0, fmin=C1, n_bins=24, bins_per_octave=12, filter_scale=1.0, gamma=0.0, scale=True)
STANDARD_L, STANDARD_HOP = 30000, 512


def frames(n, hop):
    return 1 + n // hop


def lane_width(N):
    W = 1
    while W < 64 and W < N:
        W *= 2
    return W


def basis(fs, fmin, n_bins, bins_per_octave=12, filter_scale=1.0, gamma=0.0, scale=True):
    """(half_len int32 [K], offset int64 [K], centre_hz float64 [K], length float64 [K], taps complex64 [sum N_k]) of the standard
    basis: all arithmetic in double, each component rounded to float32 once."""
    B = float(bins_per_octave)
    r = 2.0 ** (1.0 / B)
    alpha = (r * r - 1.0) / (r * r + 1.0)
    Q = filter_scale / alpha
    f = fmin * 2.0 ** (np.arange(n_bins, dtype=np.float64) / B)
    if f[-1] * (1.0 + alpha / 2.0) > fs / 2.0:
        raise ValueError("the highest bin reaches past fs / 2")
    length = Q * fs / (f + gamma / alpha)
    half = np.floor(length / 2.0).astype(np.int32)
    n = 2 * half.astype(np.int64) + 1
    offset = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
    taps = np.zeros(int(n.sum()), np.complex64)
    for k in range(n_bins):
        m = np.arange(-int(half[k]), int(half[k]) + 1, dtype=np.float64)
        g = 0.5 + 0.5 * np.cos(np.pi * m / (half[k] + 1.0))
        g = g / g.sum() * (np.sqrt(length[k]) if scale else 1.0)
        u = f[k] * m / fs
        phi = 2.0 * np.pi * (u - np.floor(u))
        taps[offset[k]:offset[k] + n[k]] = (g * np.cos(phi)).astype(np.float32) + 1j * (-(g * np.sin(phi))).astype(np.float32)
    return half, offset, f, length, taps


@functools.lru_cache(maxsize=None)
def standard_basis(scale=True):
    out = basis(**dict(STANDARD, scale=scale))
    for v in out:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def synthetic_basis(halves=SYNTH_HALF, seed=20261019):
    """(half_len, taps): seeded complex taps of about unit L1 norm per bin (no structure: every tap position matters)."""
    rng = np.random.default_rng(seed)
    half = np.array(halves, np.int32)
    parts = []
    for h in half:
        N = 2 * int(h) + 1
        parts.append(((rng.standard_normal(N) + 1j * rng.standard_normal(N)) / N).astype(np.complex64))
    taps = np.concatenate(parts)
    half.setflags(write=False)
    taps.setflags(write=False)
    return half, taps


def offsets(half):
    n = 2 * np.asarray(half, np.int64) + 1
    return np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)


def impulse_at(n):
    return n // 2 + 1


@functools.lru_cache(maxsize=None)
def inputs(n=L):
    """[3][n] float32: seeded noise, a tone at 0.05 cycles per sample, one impulse at impulse_at(n).  Read-only."""
    rng = np.random.default_rng(20261019 + n)
    x = np.zeros((3, n), np.float32)
    x[0] = rng.standard_normal(n).astype(np.float32)
    x[1] = np.sin(2 * np.pi * 0.05 * np.arange(n)).astype(np.float32)
    x[2, impulse_at(n)] = 1.0
    x.setflags(write=False)
    return x


def evaluate(x, half, taps, hop, T, restate=True):
    """x [rows][n] float32 -> dict: C64 complex128 [rows][T][K] (the float64 evaluation on the float32 taps), C32 complex64 (the float32
    restatement), cap_re / cap_im (the per-element cap (b): (N_live + 4) 2^-24 sum |c x| per component), n_live int64 [T][K]."""
    x = np.atleast_2d(x)
    R, n = x.shape
    K = len(half)
    off = offsets(half)
    x64 = x.astype(np.float64)
    C64 = np.zeros((R, T, K), np.complex128)
    C32 = np.zeros((R, T, K), np.complex64)
    cap_re, cap_im = np.zeros((R, T, K)), np.zeros((R, T, K))
    n_live = np.zeros((T, K), np.int64)
    centre = np.arange(T, dtype=np.int64) * hop
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            h = int(half[k])
            N = 2 * h + 1
            W = lane_width(N)
            c = taps[off[k]:off[k] + N]
            cr, ci = c.real.astype(np.float64), c.imag.astype(np.float64)
            acc_re, acc_im = np.zeros((R, T, W), np.float32), np.zeros((R, T, W), np.float32)
            s_re, s_im, a_re, a_im = (np.zeros((R, T)) for _ in range(4))
            for i0 in range(0, N, W):
                i = np.arange(i0, min(N, i0 + W))
                m = centre[:, None] - h + i[None, :]                # [T][w]
                live = (m >= 0) & (m < n)
                if not live.any():
                    continue
                xm = x64[:, np.clip(m, 0, n - 1)]                  # [R][T][w]
                pr, pi = xm * cr[i], xm * ci[i]
                s_re += np.where(live, pr, 0.0).sum(axis=2)
                s_im += np.where(live, pi, 0.0).sum(axis=2)
                a_re += np.where(live, np.abs(pr), 0.0).sum(axis=2)
                a_im += np.where(live, np.abs(pi), 0.0).sum(axis=2)
                n_live[:, k] += live.sum(axis=1)
                if restate:
                    w = i.size
                    fr = (pr + acc_re[:, :, :w].astype(np.float64)).astype(np.float32)
                    fi = (pi + acc_im[:, :, :w].astype(np.float64)).astype(np.float32)
                    acc_re[:, :, :w] = np.where(live, fr, acc_re[:, :, :w])
                    acc_im[:, :, :w] = np.where(live, fi, acc_im[:, :, :w])
            C64[:, :, k] = s_re + 1j * s_im
            cap_re[:, :, k] = (n_live[:, k] + 4) * 2.0 ** -24 * a_re
            cap_im[:, :, k] = (n_live[:, k] + 4) * 2.0 ** -24 * a_im
            if restate:
                s = W // 2
                while s >= 1:
                    acc_re = acc_re[:, :, :s] + acc_re[:, :, s:2 * s]
                    acc_im = acc_im[:, :, :s] + acc_im[:, :, s:2 * s]
                    s //= 2
                C32[:, :, k] = acc_re[:, :, 0] + 1j * acc_im[:, :, 0]
    return dict(C64=C64, C32=C32, cap_re=cap_re, cap_im=cap_im, n_live=n_live)


def restatement_cap(half, ref):
    """Cap (b) of the restatement's own order: (ceil(N / 64) + 10) 2^-24 sum |c x| per component (a chain of ceil(N / W) fused
    multiply-adds and a tree of at most 6 additions), as (cap_re, cap_im)."""
    N = 2 * np.asarray(half, np.int64) + 1
    depth = (-(-N // 64) + 10).astype(np.float64)
    live = np.maximum(ref["n_live"] + 4, 1).astype(np.float64)
    return ref["cap_re"] / live * depth, ref["cap_im"] / live * depth


def impulse_response(half, taps, hop, T, m0):
    """C of a unit impulse at m0: c_k[m0 - t hop] where |m0 - t hop| <= h_k, 0 elsewhere; complex64 [T][K]."""
    K = len(half)
    off = offsets(half)
    out = np.zeros((T, K), np.complex64)
    m = m0 - np.arange(T, dtype=np.int64) * hop
    for k in range(K):
        h = int(half[k])
        hit = np.abs(m) <= h
        out[hit, k] = taps[off[k] + h + m[hit]]
    return out


def touched(half, hop, T, m0):
    """bool [T][K]: the (t, k) with a live tap on sample m0."""
    m = np.abs(m0 - np.arange(T, dtype=np.int64) * hop)
    return m[:, None] <= np.asarray(half, np.int64)[None, :]


def interior(half, hop, T, n):
    """bool [T][K]: the (t, k) whose every tap is live."""
    t = np.arange(T, dtype=np.int64)[:, None] * hop
    h = np.asarray(half, np.int64)[None, :]
    return (t - h >= 0) & (t + h < n)


@functools.lru_cache(maxsize=None)
def case(hop):
    """evaluate() of the shared inputs on the synthetic basis for one hop, computed once.  Read-only."""
    half, taps = synthetic_basis()
    out = evaluate(inputs(L), half, taps, hop, frames(L, hop))
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def standard_inputs(k_tone=12, amplitude=0.5):
    """[2][STANDARD_L] float32: seeded noise, a tone of `amplitude` at the centre of bin k_tone of the standard basis."""
    f = standard_basis()[2][k_tone]
    rng = np.random.default_rng(7)
    x = np.zeros((2, STANDARD_L), np.float32)
    x[0] = rng.standard_normal(STANDARD_L).astype(np.float32)
    x[1] = (amplitude * np.cos(2 * np.pi * f / STANDARD["fs"] * np.arange(STANDARD_L))).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def standard_case(scale=True):
    half, _, _, _, taps = standard_basis(scale)
    out = evaluate(standard_inputs(), half, taps, STANDARD_HOP, frames(STANDARD_L, STANDARD_HOP))
    for v in out.values():
        v.setflags(write=False)
    return out


def peak_error(C, C64):
    """max |C - C64| per row over frames and bins (the larger of the two components), relative to the row's peak of |component| of
    C64 (0 for a row that is zero everywhere)."""
    d = C.astype(np.complex128) - C64
    err = np.maximum(np.abs(d.real), np.abs(d.imag)).reshape(C.shape[0], -1).max(axis=1)
    peak = np.maximum(np.abs(C64.real), np.abs(C64.imag)).reshape(C.shape[0], -1).max(axis=1)
    return np.where(peak > 0, err / np.where(peak > 0, peak, 1.0), err)

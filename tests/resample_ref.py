"""Band-limited resampling (include/jsg.h section 2g): the definition evaluated in float64, the float32 restatement, the per-sample
cap, the shared inputs and the case list.  numpy only; tests/test_resample_ref.py checks this module on the CPU, tests/test_gpu_resample.py
compares the GPU against it.

The restatement sums each wing in ascending tap index with a fused multiply-add into an accumulator of its own, adds the two once and
scales once, which is the order the library states.  A float32 fmaf is emulated as a float64 multiply-add rounded to float32; the
rare double rounding is why the restatement is a yardstick and not a bit mirror.
"""
import functools
import math

import numpy as np

# bound (a) of tests/test_gpu_resample.py: GPU error <= YARDSTICKS x the restatement's error on the same case, both relative to the
# case's peak.  4 before any GPU run; afterwards 1.25 x the worst measured ratio, rounded up to the next half (the rule of
# profiles/stft_power_accuracy.md).  Measured on an MI355X: the worst ratio over the case list is 1.000 (the GPU's bits equal the
# restatement's on all 268 362 outputs; profiles/resample_accuracy.md), so 1.25 x 1.000 rounded up to the next half.
YARDSTICKS = 1.5

BEST = (64, 512, 0.9475937167399596, 14.769656459379492)
FAST = (16, 512, 0.85, 8.555504641634386)


def kaiser_table(Z, P, rolloff, beta):
    """The table of jsg_sinc_table_build by numpy (np.sinc, np.i0) in double, rounded to float32 once."""
    j = np.arange(Z * P + 1, dtype=np.float64)
    u = j / (Z * P)
    return (rolloff * np.sinc(rolloff * (j / P)) * np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - u * u))) / np.i0(beta)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def table(name):
    """(Z, P, win) of "best", "fast" or "ramp" (win[j] = 1 - j/64, one zero crossing: linear interpolation for steps <= 1)."""
    if name == "ramp":
        t = (1.0 - np.arange(65, dtype=np.float64) / 64.0).astype(np.float32)
        Z, P = 1, 64
    else:
        Z, P, rolloff, beta = {"best": BEST, "fast": FAST}[name]
        t = kaiser_table(Z, P, rolloff, beta)
    t.setflags(write=False)
    return Z, P, t


TABLES = ("best", "fast", "ramp")
STEPS = {"147/160": 147 / 160, "160/147": 160 / 147, "2": 2.0, "0.5": 0.5, "2^(4/12)": 2.0 ** (4 / 12), "2^(-7/12)": 2.0 ** (-7 / 12), "1": 1.0,
         "3.7": 3.7, "1+2^-30": 1.0 + 2.0 ** -30, "1/64": 1 / 64, "64": 64.0}
RATIONAL = {"147/160": (147, 160), "160/147": (160, 147), "2": (2, 1), "0.5": (1, 2), "1": (1, 1), "1/64": (1, 64), "64": (64, 1)}   # step = orig / new
CASES = [(t, s) for t in TABLES for s in STEPS]


def case_id(c):
    return f"{c[0]}-{c[1]}"


def case_length(step_name):
    return 40 if step_name == "1/64" else 3000


def resample_length(L, step):
    """#{i >= 0 : float(i) * step < L}."""
    g = int(math.ceil(L / step))
    while g > 0 and float(g - 1) * step >= L:
        g -= 1
    while float(g) * step < L:
        g += 1
    return g


@functools.lru_cache(maxsize=None)
def inputs(L):
    """[3][L] float32: seeded noise, a tone at 0.05 cycles per sample, one impulse at impulse_at(L).  Read-only."""
    rng = np.random.default_rng(20261018 + L)
    x = np.zeros((3, L), np.float32)
    x[0] = rng.standard_normal(L).astype(np.float32)
    x[1] = np.sin(2 * np.pi * 0.05 * np.arange(L)).astype(np.float32)
    x[2, impulse_at(L)] = 1.0
    x.setflags(write=False)
    return x


def impulse_at(L):
    return L // 2 + 1


class Geometry:
    """The integers of the definition for every output of one (L, step, Z, P)."""

    def __init__(self, L, step, Z, P):
        self.L, self.step, self.Z, self.P = L, float(step), Z, P
        self.scale = 1.0 / self.step if self.step > 1.0 else 1.0
        self.S = int(np.rint(self.scale * P * 4294967296.0))
        self.lim = (Z * P) << 32
        self.T = resample_length(L, self.step)
        t = np.arange(self.T, dtype=np.float64) * self.step
        fl = np.floor(t)
        self.n = fl.astype(np.int64)
        self.F_L = np.rint((t - fl) * float(self.S)).astype(np.int64)
        self.F_R = self.S - self.F_L
        self.max_taps = -(-self.lim // self.S)          # per wing

    def wings(self):
        """(wing, k, m, pos, live) for k = 0, 1, ...: the arrays over the outputs of tap k of the left (0) and the right (1) wing."""
        for k in range(self.max_taps):
            for wing in (0, 1):
                m = self.n - k if wing == 0 else self.n + 1 + k
                pos = (self.F_L if wing == 0 else self.F_R) + k * self.S
                live = (pos < self.lim) & (m >= 0) & (m < self.L)
                if live.any():
                    yield wing, k, m, pos, live


def weights(win, pos, live):
    """(w as float32 by the emulated fmaf, w in float64) at the positions `pos` (where live; elsewhere position 0 is read and unused)."""
    pos = np.where(live, pos, 0)
    o = pos >> 32
    eta = ((pos & 0xFFFFFFFF) >> 8).astype(np.float32) * np.float32(2.0 ** -24)
    delta = win[o + 1] - win[o]                          # float32 subtraction: part of the definition
    w64 = eta.astype(np.float64) * delta.astype(np.float64) + win[o].astype(np.float64)
    return w64.astype(np.float32), w64


def evaluate(x, step, Z, P, win):
    """x [rows][L] float32 -> dict: y64 (the float64 evaluation), y32 (the float32 restatement), cap (the per-sample cap (b)),
    first / last (the lowest and highest input index with a live tap, per output; first > last where there is none)."""
    x = np.atleast_2d(x)
    R, L = x.shape
    g = Geometry(L, step, Z, P)
    x64 = x.astype(np.float64)
    sum64 = np.zeros((R, g.T))
    sumabs = np.zeros((R, g.T))
    acc = [np.zeros((R, g.T), np.float32), np.zeros((R, g.T), np.float32)]
    count = [np.zeros(g.T, np.int64), np.zeros(g.T, np.int64)]
    first, last = g.n + 1, g.n.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for wing, k, m, pos, live in g.wings():
            w32, w64 = weights(win, pos, live)
            mm = np.clip(m, 0, L - 1)
            xm = x64[:, mm]
            prod = np.where(live, w64 * xm, 0.0)
            sum64 += prod
            sumabs += np.abs(prod)
            fused = (w32.astype(np.float64) * xm + acc[wing].astype(np.float64)).astype(np.float32)
            acc[wing] = np.where(live, fused, acc[wing])
            count[wing] += live
            if wing == 0:
                first = np.where(live, np.minimum(first, m), first)
            else:
                last = np.where(live, np.maximum(last, m), last)
        sf = np.float32(g.scale)
        y32 = sf * (acc[0] + acc[1])
        y64 = np.float64(sf) * sum64
        N = np.maximum(count[0], count[1])
        cap = (N + 4) * 2.0 ** -24 * g.scale * sumabs
    return dict(y64=y64, y32=y32.astype(np.float32), cap=cap, first=first, last=last, T=g.T, geometry=g)


def impulse_response(L, step, Z, P, win, m0):
    """y of a unit impulse at m0 to the bit: fl((float)scale * w_i) where output i has a live tap at m0, +0 elsewhere."""
    g = Geometry(L, step, Z, P)
    left = m0 <= g.n
    k = np.where(left, g.n - m0, m0 - g.n - 1)
    pos = np.where(left, g.F_L, g.F_R) + k * g.S
    live = pos < g.lim
    w32, _ = weights(win, pos, live)
    return np.where(live, np.float32(g.scale) * w32, np.float32(0.0)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(table_name, step_name):
    """evaluate() of the shared inputs for one case, computed once.  Read-only."""
    Z, P, win = table(table_name)
    out = evaluate(inputs(case_length(step_name)), STEPS[step_name], Z, P, win)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def peak_error(y, y64):
    """max |y - y64| per row, relative to the row's peak of |y64| (0 for a row that is zero everywhere)."""
    peak = np.abs(y64).max(axis=1)
    err = np.abs(y.astype(np.float64) - y64).max(axis=1)
    return np.where(peak > 0, err / np.where(peak > 0, peak, 1.0), err)

"""numpy restatement of include/jsgx.h section 13 (per-channel energy normalisation): the float32 definition operation by operation (E and
L on beat_ref.fma32 and pyin_ref.log32, the chunked smoother, the compression with every product and sum rounded on its own), a float64
route through scipy.signal.lfilter and numpy powers that shares none of it, the planes and parameter sets of the tests, and the shape
list of the GPU test.  tests/test_pcen_ref.py checks this module on the CPU; tests/test_gpu_pcen.py compares the GPU against it bit for
bit."""
import numpy as np

from beat_ref import exp32, fma32  # noqa: F401
from pyin_ref import log32

F32 = np.float32
CHUNK = 256                   # JSGX_PCEN_CHUNK of include/jsgx.h
EXP_LOW, EXP_HIGH = F32(-87.0), F32(88.72)


def F(v):
    return np.float32(v)


def same_bits(a, b):
    """Equal shapes and equal bits, NaN matching NaN of any payload."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# ---------------------------------------------------------------------------------------------------- E
def exp_any32(x):
    """E(x) of the header on a float32 array: the exponential of section 1 carried to the whole line."""
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        nan, low, high = np.isnan(x), x < EXP_LOW, x > EXP_HIGH
        v = np.where(nan | low | high, F(0), x).astype(F32)
        n = np.floor(fma32(v, F(1.44269502162933349609375), F(0.5)))
        r = fma32(n, F(-0.693145751953125), v)
        r = fma32(n, F(-1.42860676533018704503775e-06), r)
        p = np.full(v.shape, 1.984127011382952332496643e-04, F32)
        for c in (1.388888922519981861114502e-03, 8.333333767950534820556641e-03, 4.166666790843009948730469e-02, 1.666666716337203979492188e-01,
                  0.5, 1.0, 1.0):
            p = fma32(p, r, F(c))
        ni = n.astype(np.int32)
        half = ni >> 1                                                            # floor(n / 2)
        first = ((half + 127) << 23).astype(np.uint32).view(F32)
        second = ((ni - half + 127) << 23).astype(np.uint32).view(F32)
        out = ((p * first).astype(F32) * second).astype(F32)
    out = np.where(low, F(0), out)
    out = np.where(high, F(np.inf), out)
    return np.where(nan, F(np.nan), out).astype(F32)


# ---------------------------------------------------------------------------------------------------- the float32 definition
def decay(b):
    """q[j] = (float)(a^(j+1)), a = fl(1.0f - b): pow in double of the float a, rounded once."""
    a = F(1.0) - F(b)
    return np.power(np.float64(a), np.arange(1, CHUNK + 1, dtype=np.float64)).astype(F32)


def smooth32(M, b, state=None):
    """M float32 [..., T, B] -> (S of the same shape, the state behind the last frame [..., B])."""
    M = np.asarray(M, F32)
    T = M.shape[-2]
    b = F(b)
    a, q = F(1.0) - b, decay(b)
    s = np.array(M[..., 0, :] if state is None else state, F32)
    S = np.empty(M.shape, F32)
    with np.errstate(all="ignore"):
        for t0 in range(0, T, CHUNK):
            p = np.zeros(s.shape, F32)
            for j in range(min(CHUNK, T - t0)):
                p = fma32(a, p, (b * M[..., t0 + j, :]).astype(F32))
                S[..., t0 + j, :] = fma32(q[j], s, p)
            s = S[..., min(T, t0 + CHUNK) - 1, :].copy()
    return S, s


def compress32(M, S, gain, bias, power, eps):
    M, S = np.asarray(M, F32), np.asarray(S, F32)
    gain, bias, power, eps = F(gain), F(bias), F(power), F(eps)
    with np.errstate(all="ignore"):
        g = exp_any32(-gain * log32(eps + S))
        y = bias + M * g
        d = exp_any32(power * log32(np.array([bias], F32)))[0]
        return (exp_any32(power * log32(y)) - d).astype(F32)


def pcen32(M, b, gain=0.98, bias=2.0, power=0.5, eps=1e-6, state=None):
    """The definition: (out, S, state_out), float32."""
    S, s = smooth32(M, b, state)
    return compress32(M, S, gain, bias, power, eps), S, s


# ---------------------------------------------------------------------------------------------------- the float64 route
def pcen64(M, b, gain=0.98, bias=2.0, power=0.5, eps=1e-6, state=None):
    """scipy.signal.lfilter and numpy powers in double on the float32 data and scalars: (out, S, state_out).  a = 1 - b in double."""
    from scipy.signal import lfilter
    M = np.asarray(M, F32).astype(np.float64)
    b, gain, bias, power, eps = (float(F(v)) for v in (b, gain, bias, power, eps))
    a = 1.0 - b
    s = M[..., 0, :] if state is None else np.asarray(state, F32).astype(np.float64)
    S, _ = lfilter([b], [1.0, -a], M, axis=-2, zi=(a * s)[..., None, :])
    with np.errstate(all="ignore"):
        out = (M * (eps + S) ** -gain + bias) ** power - bias ** power
    return out, S, S[..., -1, :]


def default_b():
    T = 0.4 * 22050 / 512
    return (np.sqrt(1.0 + 4.0 * T * T) - 1.0) / (2.0 * T * T)


# (name, dict of b, gain, bias, power, eps): librosa's defaults, a second set, and no bias
PARAMS = (("defaults", dict(b=default_b(), gain=0.98, bias=2.0, power=0.5, eps=1e-6)),
          ("second", dict(b=0.025, gain=0.8, bias=10.0, power=0.25, eps=1e-6)),
          ("no bias", dict(b=default_b(), gain=0.98, bias=0.0, power=0.5, eps=1e-6)))
SCALES = (1.0, 2.0 ** 31, 1e-6)
# The definition in float32 against the float64 route over these scales and sets, 16 seeds each (tools/pcen_accuracy.py, profiles/pcen_accuracy.md):
# the relative error of S at most 6.24e-6, |out32 - out64| / (out64 + bias^power) at most 1.51e-6.  The asserted bounds are four times
# these: the error of a recurrence varies with the signal by about that much from seed to seed.
S_MEASURED, OUT_MEASURED = 6.24e-6, 1.51e-6
S_BOUND, OUT_BOUND = 4 * S_MEASURED, 4 * OUT_MEASURED


def plane(T, B, seed=0, scale=1.0, rows=None, silent=True):
    """A mel-like non-negative plane float32 [T][B] (or [rows][T][B]): a band profile times a slowly varying level times squared noise,
    with a silent stretch over the fifth of the frames behind the middle."""
    rng = np.random.default_rng([seed, T, B])
    shape = (T, B) if rows is None else (rows, T, B)
    level = 1.0 + 0.9 * np.sin(np.arange(T) / 37.0)[:, None]
    profile = 1.0 / (1.0 + np.arange(B) / 8.0)[None, :]
    M = (rng.standard_normal(shape) ** 2) * level * profile * scale
    if silent and T >= 10:
        M[..., T // 2:T // 2 + T // 5, :] = 0.0
    return M.astype(F32)


# The shapes of the GPU test, (rows, T, B).  Frames: one, two, both sides of a chunk (255 | 256 | 257: "pcen_single" ends at 256), two chunks
# and a frame, three chunks and a tail; and, since four lanes share a chain in "pcen_apply" with 64 frames each, both sides of a part (64 |
# 65), two parts and two frames, three parts and one.  Bands: one, two, counts below a wavefront that do not divide it (31, 40, 63), the
# wavefront and its neighbours, two wavefronts, and 200.  Every value appears, the corners of (T, B) appear, and with fewer than 64 bands and
# several rows, chunks or parts a wavefront holds lanes of several of them.  tests/test_pcen_host.py derives the forms from the plan over
# every band count and fails where this list misses one.
T_SET = (1, 2, 64, 65, 130, 193, 255, 256, 257, 513, 1000)
B_SET = (1, 2, 31, 40, 63, 64, 65, 128, 200)
ROWS_SET = (1, 3)
SHAPES = [(1, 1, 1), (3, 1, 200), (3, 1000, 1), (1, 1000, 200), (3, 2, 2), (1, 255, 31), (3, 256, 40), (1, 257, 63), (3, 513, 64), (1, 256, 65),
          (3, 257, 128), (1, 513, 40), (3, 255, 65), (1, 2, 128), (3, 1000, 31), (1, 257, 2), (3, 513, 63), (1, 64, 40), (3, 65, 63), (1, 130, 2),
          (3, 193, 31), (1, 65, 128)]

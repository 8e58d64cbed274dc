"""The numpy restatement of include/jsgx.h section 5 (pYIN), operation by operation in float32: L, the observation of one frame (troughs,
thresholds, lane sums, parabola, bins, emissions) and the factored decoder (V, psi, states, logp); an independent float64 reading of the
observation from scipy's beta and Boltzmann distributions; the lane split of the forward kernel with the shapes that run every form of
it; input makers; and the tables in numpy."""
import numpy as np

from viterbi_ref import NEG_INF, same_bits  # noqa: F401

F32 = np.float32
THREADS = 1024                # JSGX_PYIN_THREADS of include/jsgx.h
LANES = 64


def F(v):
    return np.float32(v)


def form(P, W):
    """(G, threads) of include/jsgx.h 5c: G the largest power of two <= 64 with 8 G <= 2 W + 1 and P * G <= 512 (1 where there is none),
    P * G lanes rounded up to whole wavefronts."""
    G = 1
    while G < 64 and 8 * (2 * G) <= 2 * W + 1 and P * 2 * G <= 512:
        G *= 2
    return G, -(-P * G // 64) * 64


# The shapes of the GPU test, FORM_BINS x FORM_WIDTHS and FORM_PAIRS.  The bin counts: both counts wherever the limit P * G <= 512 changes
# G at some width (16 | 17, 32 | 33, 64 | 65, 128 | 129, 256 | 257), the smallest, 512 | 513, librosa's 601 and the largest.  The widths:
# none, one, librosa's 50, the largest.  FORM_PAIRS: at P = 16, where the width alone decides, both widths wherever 8 G <= 2 W + 1 changes
# G (7 | 8, 15 | 16, 31 | 32, 63 | 64, 127 | 128 with 128 among the widths); (P, W) pairs with W >= P are in FORM_WIDE.  tests/test_pyin_host.py checks the lists against
# form() over every (P, W).
FORM_BINS = (1, 2, 16, 17, 32, 33, 63, 64, 65, 128, 129, 256, 257, 512, 513, 601, 1024)
FORM_WIDTHS = (0, 1, 50, 128)
FORM_PAIRS = ((16, 7), (16, 8), (16, 15), (16, 16), (16, 31), (16, 32), (16, 63), (16, 64), (16, 127))
FORM_WIDE = ((1, 1), (2, 50), (17, 17), (63, 128))
FORM_FRAMES = (1, 2, 255, 256, 257, 513)


# ------------------------------------------------------------------------------------------------ L
def log32(x):
    """L(x) of the header on a float32 array."""
    x = np.asarray(x, F32)
    shape = x.shape
    x = x.reshape(-1).copy()
    out = np.empty(x.shape, F32)
    with np.errstate(all="ignore"):
        special = ~(x > 0) | np.isinf(x)
        out[x == 0] = -np.inf
        out[(x < 0) | np.isnan(x)] = np.nan
        out[x == np.inf] = np.inf
        v = np.where(special, F(1), x).astype(F32)
        tiny = v < F(1.1754943508222875e-38)
        v = np.where(tiny, v * F(16777216.0), v).astype(F32)
        k = np.where(tiny, -24, 0).astype(np.int64)
        i = v.view(np.uint32).astype(np.int64) + (0x3f800000 - 0x3f3504f3)
        k = k + (i >> 23) - 127
        m = ((i & 0x007fffff) + 0x3f3504f3).astype(np.uint32).view(F32)
        f = m - F(1)
        s = f / (F(2) + f)
        z = s * s
        w = z * z
        t1 = w * (F(float.fromhex("0xccce13p-25")) + w * F(float.fromhex("0xf89e26p-26")))
        t2 = z * (F(float.fromhex("0xaaaaaap-24")) + w * F(float.fromhex("0x91e9eep-25")))
        r = t2 + t1
        hfsq = (F(0.5) * f) * f
        dk = k.astype(F32)
        res = (((s * (hfsq + r) + dk * F(9.0580006145e-06)) - hfsq) + f) + dk * F(6.9313812256e-01)
    out[~special] = res[~special]
    return out.reshape(shape)


# ------------------------------------------------------------------------------------------------ tables in numpy (double, rounded once)
def boltzmann_tables(lam, n):
    i = np.arange(n, dtype=np.float64)
    m = np.arange(1, n + 1, dtype=np.float64)
    return np.exp(-lam * i).astype(F32), np.concatenate([[0.0], (1.0 - np.exp(-lam)) / (1.0 - np.exp(-lam * m))]).astype(F32)


def bins_tables(sr, fmin, bps, P):
    b = np.arange(P + 1, dtype=np.float64)
    return (sr / (fmin * np.exp2((b - 0.5) / (12.0 * bps)))).astype(F32), (fmin * np.exp2(b[:P] / (12.0 * bps))).astype(F32)


def transition_tables(P, window, switch_prob):
    w = np.asarray(window, np.float64)
    W = w.size // 2
    with np.errstate(divide="ignore"):
        log_window = np.log(w).astype(F32)
        off = np.empty(P, F32)
        for p in range(P):
            total = 0.0
            for d in range(max(0, p - W), min(P - 1, p + W) + 1):
                total += w[d - p + W]
            off[p] = F(-np.log(total))
        sw = np.log(np.array([1 - switch_prob, switch_prob, switch_prob, 1 - switch_prob], np.float64)).astype(F32)
    return log_window, off, sw


def max_troughs(tau_min, tau_max):
    return (tau_max - tau_min + 1) // 2


# ------------------------------------------------------------------------------------------------ the observation
def lane_sum(terms):
    """terms float32 [n] in the order of their index (k or b): lane l adds l, l + 64, ... ascending from +0, then the halving tree."""
    acc = np.zeros(LANES, F32)
    for i, v in enumerate(np.asarray(terms, F32)):
        acc[i % LANES] = acc[i % LANES] + v
    m = 32
    while m >= 1:
        acc[:m] = acc[:m] + acc[m:2 * m]
        m //= 2
    return acc[0]


def troughs_of(h, tau_min, tau_max):
    out = []
    for tau in range(tau_min, tau_max):
        if (h[tau] < h[tau + 1]) if tau == tau_min else (h[tau - 1] > h[tau] and h[tau] <= h[tau + 1]):
            out.append(tau)
    return out


def period32(h, tau):
    with np.errstate(invalid="ignore"):
        a, b, c = F(h[tau - 1]), F(h[tau]), F(h[tau + 1])
        den = F(F(a - b) + F(c - b))
        s = F(0)
        if den > 0:
            s = F(F(F(0.5) * F(a - c)) / den)
            if not abs(s) <= 1:
                s = F(0)
    return F(F(tau) + s)


def bin_of(period, edges, P):
    return int(sum(1 for b in range(1, P) if period <= edges[b]))


def observe32(h, tau_min, tau_max, prior, decay, norm, edges, no_trough_prob):
    """One frame h float32 [>= tau_max + 1] -> (log_emit float32 [2P], obs float32 [P], voiced float32) as include/jsgx.h 5b states it."""
    h = np.asarray(h, F32)
    prior, decay, norm, edges = (np.asarray(a, F32) for a in (prior, decay, norm, edges))
    N, P = prior.size, edges.size - 1
    obs = np.zeros(P, F32)
    emit = np.empty(2 * P, F32)
    if np.isnan(h[tau_min:tau_max + 1]).any():
        emit[:P] = -np.inf
        emit[P:] = log32(F(1) / F(P))
        return emit, obs, F(np.nan)
    th = ((np.arange(N) + 1) / float(N)).astype(F32)
    lags = troughs_of(h, tau_min, tau_max)
    below = np.array([[h[tau] < th[k] for k in range(N)] for tau in lags], bool).reshape(len(lags), N)
    n_k = below.sum(axis=0)
    rank = np.zeros(N, np.int64)
    prob = []
    for j in range(len(lags)):
        terms = np.zeros(N, F32)
        for k in np.flatnonzero(below[j]):
            terms[k] = F(prior[k] * F(norm[n_k[k]] * decay[rank[k]]))
        rank += below[j]
        prob.append(lane_sum(terms))
    if lags:
        g = min(range(len(lags)), key=lambda j: (h[lags[j]], j))
        q = lane_sum(np.where(below[g], F(0), prior))
        prob[g] = F(prob[g] + F(F(no_trough_prob) * q))
    for j, tau in enumerate(lags):
        b = bin_of(period32(h, tau), edges, P)
        obs[b] = obs[b] + prob[j]
    total = lane_sum(obs)
    voiced = F(1) if total > 1 else total
    emit[:P] = log32(obs)
    emit[P:] = log32(F(F(1) - voiced) / F(P))
    return emit, obs, voiced


def observe64(h, tau_min, tau_max, N, beta_ab, lam, sr, fmin, bps, P, no_trough_prob):
    """An independent reading of the observation of one frame in float64, written from the algorithm and sharing nothing with the float32
    restatement above: the troughs from the signs of the first differences of d', the parabola in float64, the thresholds' prior from
    scipy.stats.beta, the position pmf from scipy.stats.boltzmann, the bins from logarithms -> (obs float64 [P], voiced float64, the bins of
    the troughs, their lags)."""
    from scipy import stats
    h64 = np.asarray(h, np.float64)
    th = np.asarray(((np.arange(N) + 1) / float(N)).astype(F32), np.float64)      # the thresholds are the float32 ones: they decide, they are not rounded
    prior = np.diff(stats.beta.cdf(np.linspace(0, 1, N + 1), *beta_ab))
    # a local minimum: d' falls into the lag (strictly) and does not fall out of it; at tau_min it has only to rise out of it (strictly)
    step = np.sign(np.diff(h64))                        # step[tau] is the way from tau to tau + 1
    lags = [int(tau) for tau in np.arange(tau_min + 1, tau_max) if step[tau - 1] < 0 and step[tau] >= 0]
    if tau_max > tau_min and step[tau_min] > 0:
        lags.insert(0, tau_min)
    obs = np.zeros(P)
    bins = []
    probs = np.zeros(len(lags))
    for k in range(N):
        under = [j for j, tau in enumerate(lags) if h64[tau] < th[k]]
        for pos, j in enumerate(under):
            probs[j] += prior[k] * stats.boltzmann.pmf(pos, lam, len(under))
    if lags:
        g = int(np.argmin([h64[tau] for tau in lags]))
        probs[g] += no_trough_prob * sum(prior[k] for k in range(N) if not h64[lags[g]] < th[k])
    for j, tau in enumerate(lags):
        a, b, c = h64[tau - 1], h64[tau], h64[tau + 1]
        curve = a - 2.0 * b + c
        shift = 0.5 * (a - c) / curve if curve > 0 else 0.0
        period = tau + (shift if abs(shift) <= 1 else 0.0)
        b = int(np.clip(np.round(12 * bps * np.log2(sr / period / fmin)), 0, P - 1))
        bins.append(b)
        obs[b] += probs[j]
    return obs, min(1.0, obs.sum()), bins, lags


def frame_of(rng, tau_max, n_dips, depth):
    """A d'-like frame: 1 with n_dips smooth dips at distinct places, plus small noise."""
    h = np.ones(tau_max + 1) + 0.02 * rng.random(tau_max + 1)
    tau = np.arange(tau_max + 1)
    for c in rng.choice(np.arange(8, tau_max - 4), n_dips, replace=False):
        h -= depth * rng.random() * np.exp(-0.5 * ((tau - c) / 1.5) ** 2)
    return np.maximum(h, 1e-4).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the decoder
def _nan_to_neg_inf(v):
    return np.where(np.isnan(v), NEG_INF, v)


def decode32(log_emit, log_init, log_window, src_offset, log_switch):
    """log_emit [T][2P], log_init [2P], log_window [2W+1], src_offset [P], log_switch [4] -> (V float32 [T][2P], psi int32 [T][2P] with row 0
    zero, states int32 [T], logp float32) as include/jsgx.h 5c states it."""
    b = np.ascontiguousarray(log_emit, dtype=F32)
    p0, lw, off, sw = (np.ascontiguousarray(a, dtype=F32) for a in (log_init, log_window, src_offset, log_switch))
    T, S = b.shape
    P, W = S // 2, lw.size // 2
    pd = np.arange(P)
    src = np.arange(2 * W + 1)[:, None] - W + pd[None, :]         # row k holds the source p = p' - W + k; log_window index 2W - k
    valid = (src >= 0) & (src < P)
    src_c = np.clip(src, 0, P - 1)
    lw_rows = lw[::-1][:, None]
    V = np.empty((T, S), F32)
    psi = np.zeros((T, S), np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        V[0] = p0 + b[0]
        for t in range(1, T):
            m, at = [], []
            for u in range(2):
                U = V[t - 1][u * P:(u + 1) * P] + off
                w = _nan_to_neg_inf(U[src_c] + lw_rows)
                top = np.where(valid, w, NEG_INF).max(axis=0)
                r = np.argmax(valid & (w == top[None, :]), axis=0)          # the first, so the lowest p
                m.append(w[r, pd])
                at.append(src_c[r, pd])
            for v in range(2):
                c0 = _nan_to_neg_inf(m[0] + sw[v])
                c1 = _nan_to_neg_inf(m[1] + sw[2 + v])
                second = c1 > c0
                V[t][v * P:(v + 1) * P] = np.where(second, c1, c0) + b[t][v * P:(v + 1) * P]
                psi[t][v * P:(v + 1) * P] = np.where(second, P + at[1], at[0])
    w_end = _nan_to_neg_inf(V[T - 1])
    e = int(np.argmax(w_end == w_end.max()))
    states = np.empty(T, np.int32)
    states[T - 1] = e
    for t in range(T - 1, 0, -1):
        states[t - 1] = psi[t][states[t]]
    return V, psi, states, F(w_end[e])


def decode64(log_emit, log_init, log_window, src_offset, log_switch):
    """The best log-probability of the same model in float64, by the dense recurrence."""
    b, p0, lw, off, sw = (np.asarray(a, np.float64) for a in (log_emit, log_init, log_window, src_offset, log_switch))
    A = dense_of(lw, off, sw, dtype=np.float64)
    V = p0 + b[0]
    for t in range(1, b.shape[0]):
        V = (V[:, None] + A).max(axis=0) + b[t]
    return V.max()


def dense_of(log_window, src_offset, log_switch, dtype=F32):
    """The [2P][2P] matrix A((u, p), (u', p')) = src_offset[p] + log_window[p' - p + W] + log_switch[2u + u'], -inf outside the pitch band."""
    lw, off, sw = (np.asarray(a, dtype) for a in (log_window, src_offset, log_switch))
    P, W = off.size, lw.size // 2
    A = np.full((2 * P, 2 * P), -np.inf, dtype)
    for u in range(2):
        for v in range(2):
            for p in range(P):
                for d in range(max(0, p - W), min(P - 1, p + W) + 1):
                    A[u * P + p, v * P + d] = (off[p] + lw[d - p + W]) + sw[2 * u + v]
    return A


def eighths(shape, seed, dead=0.0):
    """Multiples of 1/8 in [-3, 0], a share `dead` of the entries -inf: every sum is exact and ties are frequent."""
    rng = np.random.default_rng(seed)
    x = (-rng.integers(0, 25, size=shape) / 8.0).astype(F32)
    if dead:
        x[rng.random(size=shape) < dead] = NEG_INF
    return x


def floats(shape, seed, dead=0.0):
    rng = np.random.default_rng(seed)
    return (-4.0 * rng.random(size=shape)).astype(F32)


MAKERS = {"eighths": eighths, "floats": floats}


def decode_inputs(kind, T, P, W, seed, dead=0.0):
    """(log_emit [T][2P], log_init [2P], log_window [2W+1], src_offset [P], log_switch [4]); only the emissions may hold -inf."""
    make = MAKERS[kind]
    return (make((T, 2 * P), 5 * seed, dead), make((2 * P,), 5 * seed + 1), make((2 * W + 1,), 5 * seed + 2), make((P,), 5 * seed + 3),
            make((4,), 5 * seed + 4))

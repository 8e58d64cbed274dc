"""The numpy restatement of include/jsgx.h section 4 (Viterbi decoding), operation by operation in float32: both transition forms, V, psi,
the states and logp; the lane split of the forward kernel and the shapes that run every form of it; the input makers of the tests; and
the bit comparison."""
import numpy as np

NEG_INF = np.float32(-np.inf)
THREADS = 1024                # JSGX_VITERBI_THREADS of include/jsgx.h


def form(S):
    """(G, threads) of include/jsgx.h, "The kernels": G the largest power of two <= 64 with S * G <= 1024 (1 where there is none),
    S * G lanes rounded up to whole wavefronts, 1024 at the most."""
    G = 64
    while G > 1 and S * G > THREADS:
        G //= 2
    return G, min(THREADS, -(-S * G // 64) * 64)


# The state counts of the dense GPU test (tests/test_gpu_viterbi.py): every (plan name, G) that a state count in 1..2048 gives and both
# counts wherever one of them changes (17, 33, 65, 129, 193, 257, 513); 1025 and 2048 give a lane its second destination.
FORM_STATES = (1, 2, 3, 16, 17, 24, 32, 33, 63, 64, 65, 128, 129, 191, 192, 193, 255, 256, 257, 512, 513, 1023, 1024, 1025, 2048)

# (S, W) of the band GPU test: for every G a band with fewer sources per destination than G lanes (2W + 1 < G; none for G = 1), one next
# to G (2W + 1 = G - 1 or G + 1; 1 for G = 1) and one with more (2W + 1 > G); W = 0, a band as wide as the matrix and one wider; and
# both sides of the LDS limit of the band table at W = 64 (312 | 313).  tests/test_jsgx_forms_host.py checks the list against form().
FORM_BANDS = ((1, 0), (5, 0), (5, 4), (16, 31), (16, 32),                  # G = 64
              (24, 3), (24, 15), (32, 16), (17, 40),                         # G = 32
              (64, 3), (40, 7), (33, 8), (40, 64),                           # G = 16
              (70, 1), (100, 3), (128, 4), (65, 30),                         # G = 8
              (129, 0), (200, 1), (256, 2), (192, 10),                       # G = 4
              (257, 0), (512, 1), (300, 25), (312, 64), (313, 64),           # G = 2
              (513, 0), (1200, 25), (2048, 64))                              # G = 1


def same_bits(a, b) -> bool:
    """NaN positions equal, all other bits equal."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.uint32)[~na] == b.view(np.uint32)[~nb]).all())


def _select(w, i_of_row, valid):
    """The pair rule over axis 0: w [R][S] float32 without NaN, i_of_row [R][S] the source of each entry ascending along axis 0, valid
    [R][S] -> (best [S] with the bits of the chosen w, i* [S])."""
    top = np.where(valid, w, NEG_INF).max(axis=0)
    r = np.argmax(valid & (w == top[None, :]), axis=0)          # the first, so the lowest source; +0 == -0
    cols = np.arange(w.shape[1])
    return w[r, cols], i_of_row[r, cols]


def viterbi32(log_emit, log_init, trans, band_half=None):
    """log_emit [T][S], log_init [S], trans [S][S] (dense; band_half None) or [2W+1][S] (band) -> (V float32 [T][S], psi int32 [T][S] with
    row 0 zero, states int32 [T], logp float32)."""
    b = np.ascontiguousarray(log_emit, dtype=np.float32)
    p0 = np.ascontiguousarray(log_init, dtype=np.float32)
    A = np.ascontiguousarray(trans, dtype=np.float32)
    T, S = b.shape
    j = np.arange(S)
    if band_half is None:
        assert A.shape == (S, S)
        src = np.broadcast_to(np.arange(S)[:, None], (S, S))
        valid = np.ones((S, S), bool)
        table = A
    else:
        W = int(band_half)
        assert A.shape == (2 * W + 1, S)
        src = np.arange(2 * W + 1)[:, None] - W + j[None, :]    # row r holds the source i = j + r - W
        valid = (src >= 0) & (src < S)
        table = np.where(valid, A, np.float32(0))               # an entry outside the matrix is never read
    src_c = np.clip(src, 0, S - 1)
    V = np.empty((T, S), np.float32)
    psi = np.zeros((T, S), np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        V[0] = p0 + b[0]
        for t in range(1, T):
            v = V[t - 1][src_c] + table                          # fl(V[t-1][i] + A(i, j))
            w = np.where(np.isnan(v), NEG_INF, v)
            best, psi[t] = _select(w, src_c, valid)
            V[t] = best + b[t]
    w_end = np.where(np.isnan(V[T - 1]), NEG_INF, V[T - 1])
    e = int(np.argmax(w_end == w_end.max()))
    states = np.empty(T, np.int32)
    states[T - 1] = e
    for t in range(T - 1, 0, -1):
        states[t - 1] = psi[t][states[t]]
    return V, psi, states, np.float32(w_end[e])


def band_as_dense(trans, band_half, fill=NEG_INF):
    """The [S][S] matrix of a band table, `fill` outside the band."""
    A = np.asarray(trans, dtype=np.float32)
    W, S = int(band_half), A.shape[1]
    D = np.full((S, S), fill, np.float32)
    for r in range(2 * W + 1):
        for j in range(S):
            i = j + r - W
            if 0 <= i < S:
                D[i, j] = A[r, j]
    return D


def poison_band(trans, band_half, value=np.float32(1e30)):
    """The band table with the never-read entries (a source outside 0..S-1) set to `value`."""
    A = np.array(trans, dtype=np.float32)
    W, S = int(band_half), A.shape[1]
    src = np.arange(2 * W + 1)[:, None] - W + np.arange(S)[None, :]
    A[(src < 0) | (src >= S)] = value
    return A


def eighths(shape, seed):
    """Multiples of 1/8 in [-3, 0] with a quarter of the entries -inf: every sum is exact and ties are frequent."""
    rng = np.random.default_rng(seed)
    x = (-rng.integers(0, 25, size=shape) / 8.0).astype(np.float32)
    x[rng.random(size=shape) < 0.25] = NEG_INF
    return x


def floats(shape, seed):
    """Random non-positive floats in (-4, 0): no ties."""
    rng = np.random.default_rng(seed)
    return (-4.0 * rng.random(size=shape)).astype(np.float32)


MAKERS = {"eighths": eighths, "floats": floats}


def inputs(kind, T, S, seed, band_half=None):
    """(log_emit [T][S], log_init [S], trans) of one kind; the band table has its never-read entries poisoned."""
    make = MAKERS[kind]
    b, p0 = make((T, S), 3 * seed), make((S,), 3 * seed + 1)
    if band_half is None:
        return b, p0, make((S, S), 3 * seed + 2)
    return b, p0, poison_band(make((2 * band_half + 1, S), 3 * seed + 2), band_half)

"""The power-STFT plans on impulses, impulse pairs, tones, a comb and noise, per bin, without a GPU (tests/stft_basis.py: classes, metric,
yardstick, bound).

1. The float64 reference agrees with the closed forms of an impulse, a pair and an on-bin tone to 1e-12 of the peak.
2. The kernel mirror (oracle/jsg_mirror.c, which the GPU equals bit for bit: tests/test_gpu_mirror.py, tests/test_gpu_stft_basis.py)
   holds e <= M * Y for every plan of oracle.mirror.PLANS on every class and window; a frame with an all-zero reference is +0.0 in
   every bin and there is at most one per call.  Thinned as stft_basis says (thin=True): impulses at every position of every size (the
   lead-ins 1..3 of n <= 2048 are left to the GPU test), pairs at every (n // 128 + 1)-th frame with both ends.
3. The bound bites: five faults injected into a float32 radix-2 FFT with a real-split post pass (written here, no kernel restated)
   each fail e <= M * Y on a structured class; fault_verdicts() also says whether the old gate -- parity_util.assert_power_close on 12
   frames of oracle.synth_audio, as tests/test_oracle_golden.py holds the mirror to float64 -- would have seen them
   (profiles/stft_power_accuracy.md has the table).
"""
import numpy as np
import pytest

import stft_basis as B

SIZES = list(B.SIZES)


@pytest.fixture(scope="module")
def mirror():
    from oracle import mirror as m
    return m.load()


def _sliced(call, step=512):
    for f0 in range(0, call.F, step):
        yield f0, min(call.F, f0 + step)


# ------------------------------------------------------------------------------------------------ 1. the reference and closed forms
@pytest.mark.parametrize("wname", ["rect", "hann", "ramp"])
@pytest.mark.parametrize("n", SIZES)
def test_reference_of_an_impulse_is_the_squared_window_entry_in_every_bin(n, wname):
    w64 = B.window(wname, n).astype(np.float64)
    seen = np.zeros(n, bool)
    for i, call in enumerate(B.calls("impulses", n, wname, thin=True)):
        m = B.impulse_positions(n, i, thin=True)
        assert m.size == call.F
        seen[m] = True
        for f0, f1 in _sliced(call):
            ref = B.power_f64(call, f0, f1)
            want = (w64[m[f0:f1]] ** 2)[:, None]
            assert np.abs(ref - want).max() <= 1e-12 * want.max()
            assert (np.abs(ref - want).max(axis=1) <= 1e-12 * want[:, 0]).all(), "per frame, against its own peak"
    assert seen.all(), "the impulses calls must put the impulse at every position of the frame"
    if n >= 4096:
        assert all(call.F <= 2731 for call in B.calls("impulses", n, wname, thin=True))


@pytest.mark.parametrize("wname", ["rect", "hann", "ramp"])
@pytest.mark.parametrize("n", SIZES)
def test_reference_of_a_pair_carries_the_cosine_of_its_distance(n, wname):
    w = B.window(wname, n)
    k = np.arange(n // 2 + 1, dtype=np.int64)
    for thin in (True, False) if n <= 1024 else (True,):
        cl = B.calls("pairs", n, wname, thin=thin)
        assert sorted({int(c.name.split(" d=")[1].split()[0]) for c in cl}) == sorted(B.pair_distances(n))
        for call in cl:
            d = int(call.name.split(" d=")[1].split()[0])
            lead = int(call.name.split("lead=")[1])
            pa = n - 1 - lead - call.hop * np.arange(call.F)
            pb = pa - d
            assert pb.min() >= 0
            a = (np.float32(B.PAIR_AMPS[0]) * w[pa]).astype(np.float64)[:, None]       # the float32 windowed samples
            b = (np.float32(B.PAIR_AMPS[1]) * w[pb]).astype(np.float64)[:, None]
            want = a * a + b * b + 2 * a * b * np.cos(2 * np.pi * ((k * d) % n) / n)[None, :]
            ref = B.power_f64(call)
            assert (np.abs(ref - want).max(axis=1) <= 1e-12 * want.max(axis=1) + 1e-300).all(), call.name
        if thin:      # both ends of every distance: the first frame that sees both impulses and the last
            for d in B.pair_distances(n):
                sub = [c for c in cl if f" d={d} " in c.name]
                tops = {n - 1 - int(c.name.split("lead=")[1]) for c in sub}
                lows = {n - 1 - int(c.name.split("lead=")[1]) - c.hop * (c.F - 1) - d for c in sub}
                assert n - 1 in tops and 0 in lows, (d, tops, lows)
                if sum(c.F for c in sub) >= 64:
                    res = np.concatenate([(n - 1 - int(c.name.split("lead=")[1]) - c.hop * np.arange(c.F)) % 64 for c in sub])
                    assert np.unique(res).size == 64


@pytest.mark.parametrize("n", SIZES)
def test_reference_of_an_on_bin_tone(n):
    """The float64 tone itself (the class rounds it to float32, which alone moves the peak bin by 1e-9 of itself): (n/2)^2 at bin k,
    n^2 cos^2(phi) at k = 0 and n/2, 0 elsewhere."""
    ph = B.tone_phases(n)
    assert ph[0] == ph[-1] == 0.3
    ks = np.unique(np.concatenate([np.arange(0, n // 2 + 1, max(1, n // 256)), [1, n // 2 - 1, n // 2]]))
    kt = (ks[:, None].astype(np.int64) * np.arange(n, dtype=np.int64)[None, :]) % n
    P = B.power_of_frames(np.cos(2 * np.pi * kt / n + ph[ks][:, None])[None])
    want = np.zeros_like(P)
    want[np.arange(ks.size), ks] = np.where((ks == 0) | (ks == n // 2), (n * np.cos(ph[ks])) ** 2, (n / 2) ** 2)
    assert (np.abs(P - want).max(axis=1) <= 1e-12 * want.max(axis=1)).all()
    call, = B.calls("tones", n, "rect")
    assert call.F == n // 2 + 1 and call.hop == n and call.x.shape == (1, n * (n // 2 + 1))
    got = B.power_f64(call, 0, 3)       # the class holds these tones, rounded to float32
    assert abs(got[0, 0] - want[0, 0]) <= 1e-6 * want[0, 0] and abs(got[1, 1] - (n / 2) ** 2) <= 1e-6 * (n / 2) ** 2


def test_zero_reference_frames_are_counted_and_must_be_plus_zero():
    n = 512
    call, = B.calls("impulses", n, "hann", thin=True)
    ref = B.power_f64(call)
    assert (ref.max(axis=1) == 0).sum() == 1 and ref[n - 1].max() == 0        # the impulse on w[0] = 0
    P = ref.astype(np.float32)
    assert B.figures({0: P}, call)[0].zero_frames == 1
    B.assert_power_basis(P, call, "float64 rounded once")
    for bad in (np.float32(-0.0), np.float32(1e-30), np.float32("nan")):
        Q = P.copy()
        Q[n - 1, 7] = bad
        with pytest.raises(AssertionError):
            B.assert_power_basis(Q, call, "a zero-reference frame that is not +0.0")
    silent = call._replace(x=np.concatenate([call.x, np.zeros((1, 2), np.float32)], axis=1), F=call.F + 2)     # two silent frames more
    with pytest.raises(AssertionError, match="all-zero reference"):
        B.assert_power_basis(np.concatenate([P, np.zeros((2, n // 2 + 1), np.float32)]), silent, "lost frames")


# ------------------------------------------------------------------------------------------------ 2. the mirror
@pytest.mark.parametrize("cls", B.CLASSES)
@pytest.mark.parametrize("n", SIZES)
def test_mirror_holds_the_bound_on_every_plan_class_and_window(mirror, n, cls):
    from oracle import mirror as mirror_mod
    plans = mirror_mod.PLANS[n]
    for wname in B.CLASS_WINDOWS[cls]:
        for pair in sorted({B.plan_is_pair(p) for p in plans}):
            mine = [p for p in plans if B.plan_is_pair(p) == pair]
            zero_frames = 0
            for call in B.calls(cls, n, wname, pair=pair, thin=True):
                assert call.x.shape[0] == (2 if pair else 1)
                figs = B.figures({p: B.mirror_columns(mirror, p, call) for p in mine}, call)
                for p in mine:
                    B.check(figs[p], call, p)
                zero_frames += figs[mine[0]].zero_frames
            if cls == "impulses" and wname == "hann":
                assert zero_frames == 1, "exactly one frame puts the impulse on w[0] = 0: the +0.0 rule must have been exercised"
            else:
                assert zero_frames == 0


# ------------------------------------------------------------------------------------------------ 3. the bound bites
FAULTS = ("window entry from its neighbour", "window read reversed", "twiddle entry replaced by the next", "mirror pair one bin off",
          "bin n/2 with the wrong sign")


def model_power(x, w, fault=None):
    """|rfft|^2 of the frames x [F][n] (raw samples) times w, in float32: n/2-point radix-2 decimation-in-time complex FFT of the packed
    frame, then the real-split post pass X[k] = (S + T) / 2, X[n/2 - k] = conj(S - T) / 2 with S = Z[k] + conj Z[n/2 - k],
    T = -i W_n^k (Z[k] - conj Z[n/2 - k]).  fault: one of FAULTS."""
    assert fault is None or fault in FAULTS
    n = w.size
    Mh = n // 2
    wu = w.astype(np.float32).copy()
    if fault == FAULTS[0]:
        wu[n // 2 + 3] = w[n // 2 + 4]
    if fault == FAULTS[1]:
        wu = wu[::-1].copy()
    f = (x.astype(np.float32) * wu[None, :]).astype(np.float32)
    z = np.empty((f.shape[0], Mh), np.complex64)
    z.real, z.imag = f[:, 0::2], f[:, 1::2]
    bits = Mh.bit_length() - 1
    rev = np.array([int(format(i, f"0{bits}b")[::-1], 2) for i in range(Mh)])
    z = z[:, rev]
    tw = np.exp(-2j * np.pi * np.arange(Mh // 2) / Mh).astype(np.complex64)
    if fault == FAULTS[2]:
        tw[Mh // 4 + 3] = tw[Mh // 4 + 4]        # an odd entry: read by the last stage only
    size = 2
    while size <= Mh:
        half = size // 2
        zz = z.reshape(-1, Mh // size, size)
        a, b = zz[:, :, :half], zz[:, :, half:] * tw[::Mh // size][None, None, :]
        z = np.concatenate([a + b, a - b], axis=2).reshape(-1, Mh)
        size *= 2
    assert z.dtype == np.complex64
    k = np.arange(Mh // 2 + 1)
    q = (Mh - k) % Mh
    if fault == FAULTS[3]:
        q[Mh // 4 + 5] -= 1
    zk, zq = z[:, k], np.conj(z[:, q])
    wp = (-1j * np.exp(-2j * np.pi * k / n)).astype(np.complex64)
    S, T = zk + zq, (zk - zq) * wp[None, :]
    lo, hi = np.complex64(0.5) * (S + T), np.conj(np.complex64(0.5) * (S - T))
    if fault == FAULTS[4]:
        hi[:, 0] = lo[:, 0]
    X = np.empty((f.shape[0], Mh + 1), np.complex64)
    X[:, Mh - k] = hi
    X[:, k] = lo
    return (X.real * X.real + X.imag * X.imag).astype(np.float32)


def model_on_call(call, fault=None):
    raw = np.lib.stride_tricks.sliding_window_view(call.x[0], call.w.size)[:(call.F - 1) * call.hop + 1:call.hop]
    return np.concatenate([model_power(raw[f0:f1], call.w, fault) for f0, f1 in _sliced(call, 1024)])


STRUCTURED = sorted(((c, wn) for c in ("pairs", "impulses", "tones", "comb") for wn in B.CLASS_WINDOWS[c]),
                    key=lambda cw: (cw[1] != "ramp", cw[0] != "tones"))      # the asymmetric window first, then the tones, then the rest


def old_gate(n, fault):
    """parity_util.assert_power_close on 12 frames of synth_audio, Hann, hop n/2: "passes", or what it said."""
    from oracle import jsg_oracle as oracle
    from parity_util import assert_power_close
    hop, F = n // 2, 12
    x = oracle.synth_audio(1, (F - 1) * hop + n, seed=n + 1)
    w = oracle.window(oracle.WIN_HANN, n)
    raw = np.lib.stride_tricks.sliding_window_view(x[0], n)[::hop][:F]
    ref = oracle.power_spectrum_f64((raw * w[None, :]).astype(np.float32))
    try:
        assert_power_close(model_power(raw, w, fault), ref, "model")
    except AssertionError as err:
        return "fails (" + str(err).replace("model: ", "") + ")"
    return "passes"


def fault_verdicts(n, fault, stop_at_first=False):
    """({"class window": worst e / Y of the faulty model over the thinned calls}, the old gate's verdict)."""
    new = {}
    for cls, wname in STRUCTURED:
        worst = 0.0
        for call in B.calls(cls, n, wname, thin=True):
            worst = max(worst, B.figures({0: model_on_call(call, fault)}, call)[0].ratio)
        new[f"{cls} {wname}"] = worst
        if stop_at_first and worst > B.M:
            break
    return new, old_gate(n, fault)


@pytest.mark.parametrize("n", [1024, 4096])
def test_the_model_without_a_fault_holds_the_bound_and_the_old_gate(n):
    for cls in B.CLASSES:
        for wname in B.CLASS_WINDOWS[cls] if n == 1024 else B.CLASS_WINDOWS[cls][-1:]:
            for call in B.calls(cls, n, wname, thin=True):
                B.assert_power_basis(model_on_call(call), call, "radix-2 model")
    assert old_gate(n, None) == "passes"


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("n", [1024, 4096])
def test_every_injected_fault_fails_the_bound_on_a_structured_class(n, fault):
    new, old = fault_verdicts(n, fault, stop_at_first=True)
    print(f"n={n} {fault}: " + ", ".join(f"{k} {v:.3g}" for k, v in new.items()) + f"; old gate {old}")
    assert max(new.values()) > B.M, f"n={n}: '{fault}' passes e <= M * Y on every structured class: {new}"

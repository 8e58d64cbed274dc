"""Structured inputs, the float64 reference, the yardstick and the bound for the power-STFT plans (Cfg512 .. Cfg8192, the pair plan and
the runs form of Cfg1024).  Plain numpy, importable without a GPU; tests/test_stft_basis_ref.py runs the kernel mirror through it,
tests/test_gpu_stft_basis.py the device, tools/stft_power_accuracy.py prints the table (profiles/stft_power_accuracy.md).

Reference: float64 rfft of the *float32* windowed frames, power taken in float64 (two channels: the mean of the two float64 powers).
Metric, per frame: e = max_k |P - P_ref| / max_k P_ref -- every bin has the weight of the frame peak, so a wrong weak bin shows and a
flat-spectrum frame (an impulse) is judged at 1e-6 in every bin, not at the 1e-5 * P of parity_util.  The figure of a call is the
largest e over its frames.  Yardstick Y: the same figure for a single-precision pocketfft (cstft_ref.rfft32) on the same float32 frames,
measured when the test runs, never a constant.  Bound: e <= M * Y.

A frame whose reference is zero in every bin is not skipped: every bin of it must be exactly +0.0 (linear power), and a call may hold
at most one such frame (on the classes below: the Hann window's w[0] = 0 meeting a lone impulse).

M = 2.5.  The rule: the mirror's worst e / Y over every plan, class and window (tools/stft_power_accuracy.py), times 1.25, rounded up
to the next half, and never above 3.  Measured: 1.98 (Cfg2048, pairs, Hann, d = n - 1), on the mirror and, bit for bit the same, on an
MI355X; 1.98 * 1.25 = 2.48.  The whole table is in profiles/stft_power_accuracy.md.

Input classes (a Call is a float32 stream [channels][samples] plus hop, frame count, feedblocks and the window; frame j starts at
sample j * hop):

impulses  one unit sample.  n <= 2048: hop 1, lead-ins 0..3: with `lead` zero samples fewer in front of it, frame j sees the impulse at
          position n - 1 - lead - j, so a position meets every frame slot of a four-frame workgroup.  n >= 4096: hop 3, lead-ins 0, 1, 2,
          which together give every position and every position residue modulo 64 in at most 2731 frames per call.  The frame count is
          the number of frames that see the impulse, (n - 1 - lead) // hop + 1 (at most ceil(n / hop)): no frame is silent.
pairs     two impulses, 1.0 and 0.75, d = 1, 37, n/2, n - 1 apart, same hops, lead-in 0, every frame that sees both.  The power of
          one impulse does not depend on a twiddle's phase; the pair's 2 a b w_a w_b cos(2 pi k d / n) does.
tones     one frame per bin k = 0 .. n/2, hop n: cos(2 pi k t / n + phi_k), phi_k seeded, 0.3 at k = 0 and n/2.
comb      an impulse every 577 samples, amplitudes 1, -0.5, 1, ..., hop n/2, feedblocks 2 (the geometry of the runs form).  At 512 points
          a frame fits between two impulses 577 apart and would be silent, so the spacing there is 283.
noise     standard normal, 64 frames, hop n/4: the anchor to what the broadband tests see.

Windows: rect, hann (the project's RMS-normalised Hann, oracle.window), ramp (0.25 + 0.75 m / n: asymmetric, no zeros -- the one that
shows a reversed or shifted window index).  The pair plan takes two channels: channel 1 is channel 0 reversed in time, times 0.5.

thin=True (the CPU suite, where the mirror costs 0.03 .. 0.8 ms per frame): impulses drop lead-ins 1..3 at n <= 2048 (every position
stays; all three thirds stay at 4096 and 8192); pairs take every (n // 128 + 1)-th frame of the same stream (an odd step: every residue
modulo 64) at two lead-ins, so that both the first and the last frame that sees both impulses are there.
"""
import os
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import cstft_ref as R

M = 2.5
SIZES = (512, 1024, 2048, 4096, 8192)
PAIR_AMPS = (1.0, 0.75)
COMB_SPACING = 577
CLASSES = ("impulses", "pairs", "tones", "comb", "noise")
CLASS_WINDOWS = {"impulses": ("rect", "hann", "ramp"), "pairs": ("rect", "hann", "ramp"), "tones": ("rect", "hann"),
                 "comb": ("rect", "hann", "ramp"), "noise": ("rect", "hann")}
MIX_ABSMEAN = 0

Call = namedtuple("Call", "name x hop F fb w")


def window(kind, n):
    if kind == "hann":
        from oracle import jsg_oracle
        return jsg_oracle.window(jsg_oracle.WIN_HANN, n)
    return R.window(kind, n)


def pair_distances(n):
    return (1, 37, n // 2, n - 1)


def comb_spacing(n):
    return COMB_SPACING if n >= 1024 else 283


def _channels(x0, pair):
    """[1][L], or for the pair plan [2][L]: channel 1 = channel 0 reversed in time, times 0.5."""
    return np.stack([x0, np.float32(0.5) * x0[::-1]]) if pair else x0[None, :]


def taps_call(name, n, w, hop, lead, taps, pair=False):
    """Impulses of amplitude a at distance d behind the first one, taps = [(d, a), ...] with d = 0 first.  Frame j sees the first at
    position n - 1 - lead - j * hop and the others d below it; the call holds every frame that sees them all."""
    dmax = max(d for d, _ in taps)
    F = (n - 1 - lead - dmax) // hop + 1
    assert F >= 1
    x0 = np.zeros((F - 1) * hop + n, np.float32)
    for d, a in taps:
        x0[n - 1 - lead - d] = a
    return Call(name, _channels(x0, pair), hop, F, max(F, n // hop + 1), w)


def impulse_positions(n, call_index, thin=False):
    """The position at which frame j of the call_index-th impulses call sees the impulse."""
    hop, leads = _impulse_plan(n, thin)
    lead = leads[call_index]
    return n - 1 - lead - hop * np.arange((n - 1 - lead) // hop + 1)


def _impulse_plan(n, thin):
    if n <= 2048:
        return 1, ((0,) if thin else (0, 1, 2, 3))
    return 3, (0, 1, 2)


def tone_phases(n):
    ph = np.random.default_rng(n).uniform(0, 2 * np.pi, n // 2 + 1)
    ph[0] = ph[-1] = 0.3
    return ph


def calls(cls, n, wname, pair=False, thin=False):
    """The calls of a class at one size and window."""
    w = window(wname, n)
    tag = f"{cls} {wname} n={n}"
    if cls == "impulses":
        hop, leads = _impulse_plan(n, thin)
        return [taps_call(f"{tag} hop={hop} lead={lead}", n, w, hop, lead, [(0, 1.0)], pair) for lead in leads]
    if cls == "pairs":
        out = []
        for d in pair_distances(n):
            taps = [(0, PAIR_AMPS[0]), (d, PAIR_AMPS[1])]
            if thin:
                hop = n // 128 + 1
                leads = sorted({0, (n - 1 - d) % hop})
            else:
                hop, leads = (1 if n <= 2048 else 3), (0,)
            out += [taps_call(f"{tag} d={d} hop={hop} lead={lead}", n, w, hop, lead, taps, pair) for lead in leads]
        return out
    if cls == "tones":
        k = np.arange(n // 2 + 1, dtype=np.int64)
        kt = (k[:, None] * np.arange(n, dtype=np.int64)[None, :]) % n      # the angle reduced exactly before the cosine
        x0 = np.cos(2 * np.pi * kt / n + tone_phases(n)[:, None]).astype(np.float32).reshape(-1)
        return [Call(tag, _channels(x0, pair), n, n // 2 + 1, 1, w)]
    if cls == "comb":
        return [comb_call(n, w, 0, 130, pair, tag)]
    if cls == "noise":
        hop, F = n // 4, 64
        x0 = np.random.default_rng(n + 7).standard_normal((F - 1) * hop + n).astype(np.float32)
        return [Call(tag, _channels(x0, pair), hop, F, 4, w)]
    raise ValueError(cls)


def comb_call(n, w, lead, F, pair=False, tag="comb"):
    """hop n/2, feedblocks 2; the first impulse (amplitude 1) at sample `lead`."""
    hop, s = n // 2, comb_spacing(n)
    x0 = np.zeros((F - 1) * hop + n, np.float32)
    at = np.arange(lead, x0.size, s)
    x0[at] = np.where(np.arange(at.size) % 2 == 0, 1.0, -0.5)
    return Call(f"{tag} lead={lead} F={F}", _channels(x0, pair), hop, F, 2, w)


# ------------------------------------------------------------------------------------------------ reference, metric, bound
def frames_f32(call, f0, f1):
    """The float32 windowed frames f0..f1-1 of every channel: [channels][f1-f0][n]."""
    return R.frames_f32(call.x, call.w.size, call.hop, f0, f1, call.w)


def power_of_frames(fr):
    """[channels][frames][n] -> [frames][n/2+1] float64: the mean over the channels of |rfft(float64(frame))|^2."""
    X = np.fft.rfft(np.asarray(fr, dtype=np.float64), axis=-1)
    return (X.real * X.real + X.imag * X.imag).mean(axis=0)


def power_f64(call, f0=0, f1=None):
    """The reference of the frames f0..f1-1 of a call: power_of_frames of its float32 windowed frames."""
    return power_of_frames(frames_f32(call, f0, call.F if f1 is None else f1))


def _power_f32fft(fr):
    X = R.rfft32(fr)
    re, im = X.real.astype(np.float64), X.imag.astype(np.float64)
    return (re * re + im * im).mean(axis=0)


def frame_metric(P, ref):
    """(e [frames], worst bin [frames], zero [frames]): e = max_k |P - ref| / max_k ref.  A frame whose reference is zero in every bin
    has e = 0 if every bin of P is exactly +0.0, else inf.  NaN in P gives inf."""
    d = np.abs(P.astype(np.float64) - ref)
    top = ref.max(axis=-1)
    worst = np.where(np.isnan(d).any(axis=-1), np.inf, np.nan_to_num(d, nan=0.0).max(axis=-1))
    zero = top == 0
    plus_zero = (np.ascontiguousarray(P, np.float32).view(np.uint32) == 0).all(axis=-1)
    e = np.where(zero, np.where(plus_zero, 0.0, np.inf), worst / np.where(zero, 1.0, top))
    return e, d.argmax(axis=-1), zero


Figures = namedtuple("Figures", "e Y ratio frame bin zero_frames")


def figures(outputs, call, slice_frames=None):
    """{key: Figures} for {key: P [F][n/2+1]} of one call: the reference and the yardstick are computed once, in slices of frames so
    that the host holds about 0.25 GB of float64 at a time."""
    n, C = call.w.size, call.x.shape[0]
    if slice_frames is None:
        slice_frames = max(1, (1 << 23) // (C * n))
    best = {k: (-1.0, 0, 0) for k in outputs}
    Y, zeros = 0.0, 0
    for f0 in range(0, call.F, slice_frames):
        f1 = min(call.F, f0 + slice_frames)
        fr = frames_f32(call, f0, f1)
        ref = power_of_frames(fr)
        y, _, zero = frame_metric(_power_f32fft(fr), ref)
        Y = max(Y, float(y[~zero].max()) if (~zero).any() else 0.0)
        zeros += int(zero.sum())
        for k, P in outputs.items():
            assert P.shape == (call.F, n // 2 + 1), (P.shape, call.F, n)
            e, kb, _ = frame_metric(P[f0:f1], ref)
            j = int(np.argmax(e))
            if e[j] > best[k][0]:
                best[k] = (float(e[j]), f0 + j, int(kb[j]))
    return {k: Figures(b[0], Y, b[0] / Y if Y > 0 else (0.0 if b[0] == 0 else np.inf), b[1], b[2], zeros) for k, b in best.items()}


def check(g, call, what, m=None):
    """Print the figures, then assert the cap on zero-reference frames and e <= m * Y."""
    m = M if m is None else m
    print(f"{what} | {call.name}: e={g.e:.3g} Y={g.Y:.3g} ratio={g.ratio:.3f} zero-reference frames={g.zero_frames}")
    assert g.zero_frames <= 1, f"{what} | {call.name}: {g.zero_frames} frames with an all-zero reference, at most 1 may go unjudged by e"
    assert np.isfinite(g.e), (f"{what} | {call.name}: frame {g.frame} is NaN, or its reference is zero in every bin and bin {g.bin} is not "
                              f"exactly +0.0")
    assert g.e <= m * g.Y, (f"{what} | {call.name}: e = {g.e:.3g} > {m} * Y = {m * g.Y:.3g} at frame {g.frame}, bin {g.bin} "
                            f"(hop={call.hop}, F={call.F})")
    return g


def assert_power_basis(P, call, what, m=None):
    return check(figures({0: P}, call)[0], call, what, m)


# ------------------------------------------------------------------------------------------------ the mirror, on several cores
def mirror_columns(mirror, plan, call, exact_db=False, workers=None):
    """oracle.mirror's columns of a call; the frames are independent, so they are spread over threads (ctypes drops the GIL)."""
    workers = min(16, os.cpu_count() or 1) if workers is None else workers
    step = max(64, -(-call.F // workers))
    spans = [(f0, min(call.F, f0 + step)) for f0 in range(0, call.F, step)]

    def run(span):
        return mirror.columns(plan, call.x, call.hop, span[1] - span[0], call.w, feedblocks=call.fb, mix=MIX_ABSMEAN, first_frame=span[0],
                              exact_db=exact_db)
    if len(spans) == 1:
        return run(spans[0])
    with ThreadPoolExecutor(len(spans)) as pool:
        return np.concatenate(list(pool.map(run, spans)))


def plan_is_pair(plan):
    return plan.endswith("P")


# ------------------------------------------------------------------------------------------------ the device
PINS = ((512, 0, "Cfg512"), (1024, 1, "Cfg1024"), (1024, 2, "Cfg1024B"), (2048, 1, "Cfg2048"), (2048, 2, "Cfg2048B"), (2048, 3, "Cfg2048P"),
        (4096, 1, "Cfg4096"), (4096, 2, "Cfg4096B"), (8192, 0, "Cfg8192"))      # (n, plan_select, the kernel it must name)


def gpu_columns(jsg, torch, call, sel, kernel, linear_out=True, exact_log=False):
    """[F][n/2+1] float32 of jsg.stft_db on the device, launched over a NaN-filled buffer; asserts the kernel's name first."""
    n = call.w.size
    plan = jsg.Plan(n, call.w)
    d_x = torch.from_numpy(call.x).cuda()
    d_out = torch.full((call.F, (n // 2 + 1 + 31) // 32 * 32), float("nan"), device="cuda")
    kw = dict(feedblocks=call.fb, mix_mode=MIX_ABSMEAN, plan_select=sel)
    name = jsg.stft_kernel_name(plan, d_x, call.hop, call.F, d_out, **kw)
    assert name == kernel, f"{call.name}: plan_select={sel} names {name}, not {kernel}"
    jsg.stft_db(plan, d_x, call.hop, call.F, d_out, linear_out=linear_out, exact_log=exact_log, **kw)
    torch.cuda.synchronize()
    return d_out[:, :n // 2 + 1].cpu().numpy()

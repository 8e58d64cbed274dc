"""Complex STFT / inverse STFT (csrc/jsg_cstft.hip) at the size it is run at, per bin, in pitched buffers.

tests/test_gpu_cstft.py never gives a workgroup a second tile, judges a frame in L2 and uses torch's contiguous buffers only.  Here:

1. walked tiles: more than three rounds of tiles per workgroup, ragged last tile, three rows; every frame against float64, and bit
   for bit against the same frames launched from another tile slot, workgroup and round;
2. every bin and every position: impulses (hop 1), a tone on every bin, noise; bins 0 and n/2 real; zeros give zeros;
3. pitched, padded and odd-offset buffers, forward and inverse: same bits, padding untouched;
4. one NaN in, exactly its frames (forward) or its samples (inverse) NaN out, everything else bit-equal;
5. istft_c2r_kernel alone (rectangular window, hop n): random bins and the basis, per sample;
6. the overlap-add on every sample with a live envelope, small odd hops chunked;
7. the automatic 64 MiB chunking: the size rule, three scratch sizes bit-equal, the seams, a shifted call;
8. the round trip of jsg.stft / jsg.istft at that size, and the wrappers' corners.

References, metrics and bounds: tests/cstft_ref.py.  Forward: per frame e = max_k |X - X_ref| / max_k |X_ref| <= M * Y, Y the same
figure of a float32 CPU FFT on the same frames; inverse: the per-sample bound.  M = 2.

Measured on an MI355X (tools/cstft_accuracy.py, profiles/cstft_accuracy.md), worst e_gpu / Y per class, and the size it is at:
walked tiles hop n/4 1.19 (8192), hop 441 1.14 (4096); noise, rectangular 1.22 (4096); noise, Hann 1.28 (1024); impulses 1.14 (4096);
impulses, ramp window 1.04 (4096); tones 1.26 (4096).  Per size the worst class is at 1.11 / 1.28 / 1.20 / 1.26 / 1.25 (512 .. 8192):
no growth with n.  All at most 1.6, so M = 2 stands.  Inverse, worst err / tol at
M = 2 (M = 1): c2r alone on random bins 0.41 (0.75), on the basis 0.50 (0.99, at 8192), overlap-add 0.42 (0.82).

The file takes 22 s on an MI355X machine where tests/test_gpu_cstft.py takes 3.6 s (six times; the float64 comparison of item 1
looks at every frame).
"""
import warnings

import numpy as np
import pytest

import cstft_ref as R

pytestmark = pytest.mark.gpu

SIZES = list(R.SIZES)
SENT_C = complex(7.0, 7.0)
SENT_F = 3.0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def bits(torch, t):
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().view(torch.int32)


def same_bits(torch, a, b):
    return a.shape == b.shape and torch.equal(bits(torch, a), bits(torch, b))


def first_difference(torch, a, b):
    d = (bits(torch, a) != bits(torch, b)).nonzero()
    return "equal" if d.numel() == 0 else f"{d.shape[0]} differing words, first at index {tuple(int(v) for v in d[0])}"


def gpu_forward(jsg, torch, plan, x, hop, F):
    """[rows][F][n/2+1] complex64 on the device, launched over the sentinel; a finite input gives exactly real bins 0 and n/2."""
    d_in = x if torch.is_tensor(x) else torch.from_numpy(x).cuda()
    out = torch.full((d_in.shape[0], F, plan.n // 2 + 1), SENT_C, dtype=torch.complex64, device="cuda")
    jsg.cstft(plan, d_in, hop, F, out)
    torch.cuda.synchronize()
    for k in (0, plan.n // 2):
        bad = (out[..., k].imag != 0).nonzero()
        assert bad.numel() == 0, (f"bin {k} has a non-zero imaginary part at (row, frame) {tuple(int(v) for v in bad[0])}: the real "
                                  f"split yields 0 + 0 there for every finite input (n={plan.n}, hop={hop})")
    return out


def gpu_inverse(jsg, torch, plan, X, hop, T=None, d_scratch=None):
    d_X = X if torch.is_tensor(X) else torch.from_numpy(X).cuda()
    F = d_X.shape[1]
    T = (F - 1) * hop + plan.n if T is None else T
    y = torch.full((d_X.shape[0], T), SENT_F, device="cuda")
    jsg.istft_launch(plan, d_X, hop, F, y, d_scratch=d_scratch)
    torch.cuda.synchronize()
    return y


def walked_frames(torch, n, ragged):
    """Frames per row of a 3-row call with 3 * (8 * CUs + 1) tiles: every workgroup of the largest grid (8 per CU) takes at least
    three tiles and the last round is ragged; the last tile of a row holds `ragged` frames where a tile holds several."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    fpb = max(1, 2048 // n)
    tiles_per_row = 8 * cus + 1
    assert (3 * tiles_per_row - 3 * 8 * cus) % 2 == 1
    return (tiles_per_row - 1) * fpb + max(1, min(ragged, fpb))


def mix(rows, L, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(L, dtype=np.float64)
    out = np.zeros((rows, L), np.float32)
    for r in range(rows):
        out[r] = 0.5 * np.sin(2 * np.pi * (0.013 + 0.007 * r) * t) + 0.2 * np.sin(2 * np.pi * 0.21 * t + r) + 0.1 * rng.uniform(-1, 1, L)
    return out


# ------------------------------------------------------------------------------------------------ 1. walked tiles, forward
@pytest.mark.parametrize("hop_kind", ["quarter", 441])
@pytest.mark.parametrize("n", SIZES)
def test_walked_tiles_forward(jsg, torch_cuda, n, hop_kind):
    torch = torch_cuda
    hop = n // 4 if hop_kind == "quarter" else 441
    fpb = max(1, 2048 // n)
    F = walked_frames(torch, n, 1 if hop == 441 else fpb - 1)
    assert fpb == 1 or F % fpb != 0
    w = R.window("hann", n)
    plan = jsg.CStftPlan(n, w)
    x = R.noise(3, (F - 1) * hop + n, seed=n + hop)
    d_x = torch.from_numpy(x).cuda()
    X = gpu_forward(jsg, torch, plan, d_x, hop, F)
    # no reference: a frame's bins may not depend on its tile slot, its workgroup or the round
    Xs = gpu_forward(jsg, torch, plan, d_x[:, hop:], hop, F - 1)
    assert same_bits(torch, Xs, X[:, 1:]), f"launched one frame later (n={n}, hop={hop}, F={F}): [row, frame - 1, bin, re/im] " + first_difference(torch, Xs, X[:, 1:])
    del Xs
    for r in range(3):
        Xr = gpu_forward(jsg, torch, plan, d_x[r:r + 1], hop, F)
        assert same_bits(torch, Xr, X[r:r + 1]), f"row {r} launched alone (n={n}, hop={hop}, F={F}): " + first_difference(torch, Xr, X[r:r + 1])
        del Xr
    g = R.assert_forward(X.cpu().numpy(), x, n, hop, w, f"walked tiles n={n} hop={hop} F={F} (tile = frame // {fpb})")
    assert g.Y < 1e-6


# ------------------------------------------------------------------------------------------------ 2. every bin, every position
@pytest.mark.parametrize("cls", R.FORWARD_CLASSES)
@pytest.mark.parametrize("n", SIZES)
def test_every_bin_every_position(jsg, torch_cuda, n, cls):
    torch = torch_cuda
    x, hop, F, w = R.forward_class(cls, n)
    plan = jsg.CStftPlan(n, w)
    X = gpu_forward(jsg, torch, plan, x, hop, F).cpu().numpy()
    g = R.assert_forward(X, x, n, hop, w, f"{cls} n={n}")
    assert g.Y < 1e-6
    if cls.startswith("impulses"):      # the closed form X[j][k] = w[m] W_n^(k m), m = n - 1 - j, on a spread of positions
        frames = np.unique(np.concatenate([np.arange(8), np.arange(n - 8, n), np.arange(11, n, 37)]))
        cf = R.impulse_closed_form(n, w, frames)
        e, kb = R.frame_metric(X[0, frames], cf)
        j = int(np.argmax(e))
        assert e[j] <= R.M * g.Y, f"{cls} n={n}: e = {e[j]:.3g} against the closed form at frame {frames[j]} (position {n - 1 - frames[j]}), bin {kb[j]}"


@pytest.mark.parametrize("n", SIZES)
def test_zero_input_gives_zero_bins(jsg, torch_cuda, n):
    torch = torch_cuda
    plan = jsg.CStftPlan(n, R.window("ramp", n))
    F, hop = 4 * max(1, 2048 // n) + 1, 441
    X = gpu_forward(jsg, torch, plan, torch.zeros((2, (F - 1) * hop + n), device="cuda"), hop, F)
    assert bool((torch.view_as_real(X) == 0).all()), "an all-zero input must overwrite the sentinel with zero in every bin"
    y = gpu_inverse(jsg, torch, plan, torch.zeros((2, F, n // 2 + 1), dtype=torch.complex64, device="cuda"), hop)
    assert not (y != 0).any()


# ------------------------------------------------------------------------------------------------ 3. pitched and offset buffers
@pytest.mark.parametrize("n", SIZES)
def test_pitched_and_offset_buffers_forward(jsg, torch_cuda, n):
    torch = torch_cuda
    B = n // 2 + 1
    rows, F = 3, 3 * max(1, 2048 // n) + 2
    w = R.window("hann", n)
    plan = jsg.CStftPlan(n, w)
    for hop in (441, 1, n - 1):
        L = (F - 1) * hop + n
        x = R.noise(rows, L, seed=n + hop)
        want = gpu_forward(jsg, torch, plan, x, hop, F)
        wide = torch.full((rows, L + 6), 1e30, device="cuda")       # anything read outside the view would blow the bins up
        wide[:, 1:1 + L] = torch.from_numpy(x).cuda()
        d_in = wide[:, 1:1 + L]                                       # starts at an odd float, in_pitch > in_samples
        assert d_in.data_ptr() % 8 == 4 and d_in.stride(0) == L + 6
        fp = B + 3
        rp = F * fp + 5
        flat = torch.full((rows * rp + 11,), SENT_C, dtype=torch.complex64, device="cuda")
        out = torch.as_strided(flat, (rows, F, B), (rp, fp, 1))
        jsg.cstft(plan, d_in, hop, F, out)
        torch.cuda.synchronize()
        assert same_bits(torch, out, want), f"n={n} hop={hop}: pitched against contiguous, [row, frame, bin, re/im] " + first_difference(torch, out, want)
        pad = torch.ones(flat.shape, dtype=torch.bool, device="cuda")
        torch.as_strided(pad, (rows, F, B), (rp, fp, 1)).fill_(False)
        assert int(pad.sum()) == flat.numel() - rows * F * B
        sent = torch.full((int(pad.sum()),), SENT_C, dtype=torch.complex64, device="cuda")
        assert same_bits(torch, flat[pad], sent), f"n={n} hop={hop}: the forward launch wrote into the padding of the output"


@pytest.mark.parametrize("n", SIZES)
def test_pitched_and_offset_buffers_inverse(jsg, torch_cuda, n):
    torch = torch_cuda
    B = n // 2 + 1
    rows, F = 3, 3 * max(1, 2048 // n) + 2
    w = R.window("hann", n)
    plan = jsg.CStftPlan(n, w)
    for hop in (441, n // 4):
        span = (F - 1) * hop + n
        Xn = R.random_bins(rows, F, n, seed=n + hop)
        full = gpu_inverse(jsg, torch, plan, Xn, hop)
        T = span - 37                                     # short of the span, the frame count is not
        assert (T - 1) // hop + 1 >= F
        want = gpu_inverse(jsg, torch, plan, Xn, hop, T=T)
        assert same_bits(torch, want, full[:, :T])
        fp, op = B + 3, T + 7
        rp = F * fp + 5
        Xflat = torch.full((rows * rp + 11,), complex(1e30, -1e30), dtype=torch.complex64, device="cuda")
        Xp = torch.as_strided(Xflat, (rows, F, B), (rp, fp, 1))
        Xp.copy_(torch.from_numpy(Xn).cuda())
        yflat = torch.full((1 + rows * op + 9,), SENT_F, device="cuda")
        y = torch.as_strided(yflat, (rows, T), (op, 1), 1)            # starts at an odd float
        assert y.data_ptr() % 8 == 4
        jsg.istft_launch(plan, Xp, hop, F, y)
        torch.cuda.synchronize()
        assert same_bits(torch, y, want), f"n={n} hop={hop}: pitched against contiguous, [row, sample] " + first_difference(torch, y, want)
        pad = torch.ones(yflat.shape, dtype=torch.bool, device="cuda")
        torch.as_strided(pad, (rows, T), (op, 1), 1).fill_(False)
        assert bool((yflat[pad] == SENT_F).all()), f"n={n} hop={hop}: the inverse launch wrote outside [row][0, out_samples)"
        # a short out_samples with fewer frames reaching it: the frames past it are not needed and change nothing
        T2 = (F - 3) * hop + 5
        y2 = torch.full((rows, T2 + 4), SENT_F, device="cuda")
        jsg.istft_launch(plan, Xp, hop, F, y2, T2)
        torch.cuda.synchronize()
        assert same_bits(torch, y2[:, :T2], full[:, :T2]) and bool((y2[:, T2:] == SENT_F).all()), (n, hop)


# ------------------------------------------------------------------------------------------------ 4. NaN containment
@pytest.mark.parametrize("n", [512, 1024, 4096])
def test_nan_containment_forward(jsg, torch_cuda, n):
    torch = torch_cuda
    fpb = max(1, 2048 // n)
    rows, hop, F = 2, n // 4, 2 * max(fpb, 2) + 3
    plan = jsg.CStftPlan(n, R.window("hann", n))      # w[0] = 0: NaN * 0 is NaN all the same
    L = (F - 1) * hop + n
    x = R.noise(rows, L, seed=n)
    clean = gpu_forward(jsg, torch, plan, x, hop, F)
    j = max(fpb, 2)                                    # frames j, j + 1 share a tile where a tile holds several
    spots = {"first sample of a frame": j * hop, "last sample of a frame": j * hop + n - 1, "shared by two frames of one tile": (j + 1) * hop + 5,
             "random": int(np.random.default_rng(n).integers(0, L)), "first sample": 0, "last sample": L - 1}
    for what, s in spots.items():
        xn = x.copy()
        xn[1, s] = np.nan
        out = torch.full((rows, F, n // 2 + 1), SENT_C, dtype=torch.complex64, device="cuda")
        jsg.cstft(plan, torch.from_numpy(xn).cuda(), hop, F, out)
        torch.cuda.synchronize()
        reads = np.array([f * hop <= s < f * hop + n for f in range(F)])
        assert reads.any()
        hit = torch.from_numpy(reads).cuda()
        assert same_bits(torch, out[0], clean[0]), f"n={n}, NaN at row 1 sample {s} ({what}): row 0 changed"
        assert same_bits(torch, out[1][~hit], clean[1][~hit]), (f"n={n}, NaN at sample {s} ({what}): a frame that does not read it changed, [frame, bin, re/im] "
                                                                 + first_difference(torch, out[1][~hit], clean[1][~hit]))
        v = torch.view_as_real(out[1][hit])
        finite = torch.isfinite(v).all(dim=-1).nonzero()
        assert finite.numel() == 0, f"n={n}, NaN at sample {s} ({what}): frame {np.flatnonzero(reads)[int(finite[0][0])]} reads it, bin {int(finite[0][1])} is finite"


@pytest.mark.parametrize("n", [512, 1024, 4096])
def test_nan_containment_inverse(jsg, torch_cuda, n):
    torch = torch_cuda
    fpb = max(1, 2048 // n)
    rows, hop, F = 2, n // 4, 2 * max(fpb, 2) + 3
    w = R.window("hann", n)
    plan = jsg.CStftPlan(n, w)
    Xn = R.random_bins(rows, F, n, seed=n)
    T = (F - 1) * hop + n
    clean = gpu_inverse(jsg, torch, plan, Xn, hop)
    live = R.inverse_f64(Xn[:1], n, hop, w, T).env > R.ENV_EPS
    rng = np.random.default_rng(n)
    for j, k, part in [(0, 0, "re"), (F - 1, n // 2, "re"), (fpb, 1, "im"), (fpb + 1, int(rng.integers(1, n // 2)), "re"), (F // 2, n // 4, "im")]:
        Xb = Xn.copy()
        Xb[1, j, k] = complex(np.nan, Xb[1, j, k].imag) if part == "re" else complex(Xb[1, j, k].real, np.nan)
        y = gpu_inverse(jsg, torch, plan, Xb, hop)
        hit = np.zeros(T, bool)
        hit[j * hop:j * hop + n] = True
        hit &= live
        h = torch.from_numpy(hit).cuda()
        assert same_bits(torch, y[0], clean[0]), f"n={n}, NaN in row 1 frame {j} bin {k}: row 0 changed"
        clean_ones = np.flatnonzero(hit)[(~torch.isnan(y[1][h])).cpu().numpy()]
        assert clean_ones.size == 0, f"n={n}, NaN in frame {j} bin {k} ({part}): sample {clean_ones[:1]} of [{j * hop}, {j * hop + n}) is not NaN"
        assert same_bits(torch, y[1][~h], clean[1][~h]), f"n={n}, NaN in frame {j} bin {k} ({part}): outside [j hop, j hop + n), [sample] " + first_difference(torch, y[1][~h], clean[1][~h])
    for j, k in [(0, 0), (fpb + 1, n // 2), (F - 1, 0)]:      # the imaginary parts of bins 0 and n/2 are not read
        Xb = Xn.copy()
        Xb[1, j, k] = complex(Xb[1, j, k].real, np.nan)
        y = gpu_inverse(jsg, torch, plan, Xb, hop)
        assert same_bits(torch, y, clean), f"n={n}: a NaN in the imaginary part of bin {k} of frame {j} changed the output, " + first_difference(torch, y, clean)


# ------------------------------------------------------------------------------------------------ 5. the c2r kernel alone
def check_frames_alone(jsg, torch, plan, Xn, what, slice_frames=1024):
    """Rectangular window, hop n: the overlap-add is the identity, the output is irfft of each frame (env = 1)."""
    n = plan.n
    w = R.window("rect", n)
    y = gpu_inverse(jsg, torch, plan, Xn, n).cpu().numpy()
    Y_inv = R.inverse_yardstick(Xn, n) if Xn.shape[1] <= slice_frames else max(
        R.inverse_yardstick(Xn[:, f:f + slice_frames], n) for f in range(0, Xn.shape[1], slice_frames))
    worst = 0.0
    for f0 in range(0, Xn.shape[1], slice_frames):
        Xs = Xn[:, f0:f0 + slice_frames]
        ref = R.inverse_f64(Xs, n, n, w, Xs.shape[1] * n)
        assert (ref.env == 1).all()
        g = R.inverse_figures(y[:, f0 * n:(f0 + Xs.shape[1]) * n], ref, Y_inv)
        assert g.ratio <= 1.0, (f"{what} n={n}: |y - ref| = {g.err:.3g} > tol = {g.tol:.3g} at row {g.row}, frame {f0 + g.t // n}, "
                                f"sample {g.t % n} of the frame (Y_inv = {Y_inv:.3g})")
        worst = max(worst, g.ratio)
    print(f"{what} n={n}: err/tol={worst:.3f} Y_inv={Y_inv:.3g}")
    return y


@pytest.mark.parametrize("n", SIZES)
def test_c2r_alone_random_bins(jsg, torch_cuda, n):
    torch = torch_cuda
    plan = jsg.CStftPlan(n, R.window("rect", n))
    Xn = R.random_bins(3, 4 * max(1, 2048 // n) + 3, n, seed=n)
    y = check_frames_alone(jsg, torch, plan, Xn, "random bins")
    Xi = Xn.copy()
    Xi[..., 0] += 5j
    Xi[..., -1] -= 3j
    y2 = gpu_inverse(jsg, torch, plan, Xi, n)
    assert same_bits(torch, y2, torch.from_numpy(y).cuda()), f"n={n}: imaginary parts in bins 0 and n/2 changed the output, [row, sample] " + first_difference(torch, y2, torch.from_numpy(y).cuda())


@pytest.mark.parametrize("n", SIZES)
def test_c2r_alone_basis(jsg, torch_cuda, n):
    torch = torch_cuda
    plan = jsg.CStftPlan(n, R.window("rect", n))
    y = check_frames_alone(jsg, torch, plan, R.basis_bins(n), "basis").reshape(-1, n)
    B = n // 2 + 1
    assert not y[B].any() and not y[2 * B - 1].any(), "a unit in the imaginary part of bin 0 or n/2 must give an all-zero frame"
    m = np.arange(n)
    for k in (0, 1, n // 4 + 1, n // 2 - 1, n // 2):       # the closed forms, for scale 1e-6 of the amplitude
        amp = (1.0 if k in (0, n // 2) else 2.0) / n
        assert np.abs(y[k] - amp * np.cos(2 * np.pi * ((k * m) % n) / n)).max() <= 1e-6 * amp, k
        if 0 < k < n // 2:
            assert np.abs(y[B + k] + amp * np.sin(2 * np.pi * ((k * m) % n) / n)).max() <= 1e-6 * amp, k


# ------------------------------------------------------------------------------------------------ 6. overlap-add, all samples
@pytest.mark.parametrize("n", SIZES)
def test_overlap_add_every_sample(jsg, torch_cuda, n):
    torch = torch_cuda
    rows = 3
    for wk, hop, F in R.inverse_cases(n):
        w = R.window(wk, n)
        plan = jsg.CStftPlan(n, w)
        Xn = R.random_bins(rows, F, n, seed=n + hop)
        T = (F - 1) * hop + n
        K = (n - 1) // hop
        y = gpu_inverse(jsg, torch, plan, Xn, hop)
        if F > K + 1:       # the same call in chunks: the smallest scratch (one new frame per chunk) and a few frames more
            for per_row in (K + 1, K + 4):
                yc = gpu_inverse(jsg, torch, plan, Xn, hop, d_scratch=torch.empty(rows * n * per_row, device="cuda"))
                assert same_bits(torch, yc, y), f"{wk} n={n} hop={hop} F={F}: {per_row} scratch frames per row, [row, sample] " + first_difference(torch, yc, y)
        ref = R.inverse_f64(Xn, n, hop, w, T)
        R.assert_inverse(y.cpu().numpy(), ref, R.inverse_yardstick(Xn, n), f"overlap-add {wk} n={n} hop={hop} F={F}", n, hop, dead_cap=T // 1000)


# ------------------------------------------------------------------------------------------------ 7. the 64 MiB path
def scratch_rule(n, rows, hop, F_reaching):
    """include/jsg.h: the whole call up to 16 Mi floats, else whole frames of all rows within the cap, at least the minimum."""
    frame, cap = rows * n, 16 << 20
    whole, minimum = F_reaching * frame, min(F_reaching, (n - 1) // hop + 1) * frame
    return whole if whole <= cap else max(minimum, cap // frame * frame)


def test_automatic_chunking_above_64_mib(jsg, torch_cuda):
    torch = torch_cuda
    n, rows, F, hop = 2048, 4, 6200, 512
    w = R.window("hann", n)
    plan = jsg.CStftPlan(n, w)
    Xn = R.random_bins(rows, F, n, seed=7)
    X = torch.from_numpy(Xn).cuda()
    T = (F - 1) * hop + n
    K = (n - 1) // hop
    y = torch.full((rows, T), SENT_F, device="cuda")
    rec = jsg.istft_scratch_floats(plan, X, hop, F, y)
    assert rec == scratch_rule(n, rows, hop, F) == 16 << 20 and rec < rows * n * F
    # the rule below the cap, with out_samples short of the last frames, and where the minimum is above the cap
    assert jsg.istft_scratch_floats(plan, X, hop, 2048, y, out_samples=2047 * hop + n) == scratch_rule(n, rows, hop, 2048) == rows * n * 2048 == 16 << 20
    assert jsg.istft_scratch_floats(plan, X, hop, 2049, y, out_samples=2048 * hop + n) == scratch_rule(n, rows, hop, 2049) == 16 << 20
    assert jsg.istft_scratch_floats(plan, X, hop, F, y, out_samples=100 * hop) == scratch_rule(n, rows, hop, 100) == rows * n * 100
    p512 = jsg.CStftPlan(512, R.window("rect", 512))
    Xq = torch.empty((65, 600, 257), dtype=torch.complex64, device="cuda")
    yq = torch.empty((65, 599 + 512), device="cuda")
    assert jsg.istft_scratch_floats(p512, Xq, 1, 600, yq) == scratch_rule(512, 65, 1, 600) == 65 * 512 * 512 > 16 << 20
    del Xq, yq
    jsg.istft_launch(plan, X, hop, F, y)                     # d_scratch=None: 64 MiB, chunks of 2048 - K new frames
    whole = gpu_inverse(jsg, torch, plan, X, hop, d_scratch=torch.empty(rows * n * F, device="cuda"))
    assert same_bits(torch, y, whole), "automatic chunks against whole-call scratch, [row, sample] " + first_difference(torch, y, whole)
    del whole
    least = gpu_inverse(jsg, torch, plan, X, hop, d_scratch=torch.empty(rows * n * (K + 1), device="cuda"))
    assert same_bits(torch, y, least), "automatic chunks against the smallest scratch, [row, sample] " + first_difference(torch, y, least)
    del least
    # frames 1..F-1 alone: every sample that frame 0 does not cover has the same frames in the same order
    shifted = gpu_inverse(jsg, torch, plan, X[:, 1:], hop)
    assert same_bits(torch, shifted[:, n - hop:], y[:, n:]), "frames 1..F-1 against the full call, [row, sample - n] " + first_difference(torch, shifted[:, n - hop:], y[:, n:])
    del shifted
    step = rec // (rows * n) - K
    seams = [i * step * hop for i in (1, 2, 3)]
    assert seams[2] < T - n, "the call must run in at least four automatic chunks"
    yh = y.cpu().numpy()
    Y_inv = max(R.inverse_yardstick(Xn[r:r + 1], n) for r in range(rows))
    for r in range(rows):                                    # row by row: the host holds one row's float64 frames at a time
        ref = R.inverse_f64(Xn[r:r + 1], n, hop, w, T)
        for s in seams + [hop, 2 * hop, 3 * hop]:            # ... and the first seams of the smallest scratch
            lo = max(0, s - n)
            g = R.inverse_figures(yh[r:r + 1, lo:s + n], R.slice_ref(ref, lo, s + n), Y_inv)
            assert g.ratio <= 1.0, f"row {r}, seam at sample {s}: |y - ref| = {g.err:.3g} > tol = {g.tol:.3g} at sample {lo + g.t}"
        R.assert_inverse(yh[r:r + 1], ref, Y_inv, f"64 MiB path row {r}", n, hop, dead_cap=T // 1000)      # all samples, not a 1 % draw


# ------------------------------------------------------------------------------------------------ 8. round trip at that size
@pytest.mark.parametrize("hop_kind", ["quarter", 441])
@pytest.mark.parametrize("n", SIZES)
def test_round_trip_full_size(jsg, torch_cuda, n, hop_kind):
    torch = torch_cuda
    hop = n // 4 if hop_kind == "quarter" else 441
    frames = walked_frames(torch, n, 1)
    L = (frames - 1) * hop             # a multiple of hop, as in test_gpu_cstft.test_round_trip; centred: 1 + L / hop frames
    win = torch.from_numpy(R.window("hann", n))
    xn = mix(3, L, seed=n)
    x = torch.from_numpy(xn).cuda()
    X = jsg.stft(x, n, hop, window=win)
    assert X.shape == (3, n // 2 + 1, frames)
    y = jsg.istft(X, n, hop, window=win)
    assert y.shape == x.shape
    worst = float((y - x).abs().max())
    assert worst <= 1e-5 * float(x.abs().max()), f"n={n} hop={hop}: round trip off by {worst:.3g} at [row, sample] {tuple(int(v) for v in ((y - x).abs() == worst).nonzero()[0])}"
    Xh = X.transpose(-1, -2).cpu().numpy()
    yh = y.cpu().numpy()
    w = win.numpy()
    Y_inv = max(R.inverse_yardstick(Xh[r:r + 1], n) for r in range(3))
    for r in range(3):
        ref = R.inverse_f64(Xh[r:r + 1], n, hop, w, n // 2 + L)
        cut = R.slice_ref(ref, n // 2, n // 2 + L)
        assert (cut.env > R.ENV_EPS).all()
        R.assert_inverse(yh[r:r + 1], cut, Y_inv, f"round trip n={n} hop={hop} row {r} (sample + n/2 of the span)", n, hop, dead_cap=0)


def test_wrapper_corners(jsg, torch_cuda):
    torch = torch_cuda
    n, hop = 1024, 256
    win = torch.hann_window(n)
    L = 40 * hop
    x = torch.from_numpy(mix(6, L, seed=3)).cuda()
    X = jsg.stft(x, n, hop, window=win)                                  # [6][bins][frames], a transposed view
    y = jsg.istft(X, n, hop, window=win)
    # a [2, 3, L] batch is its six rows
    Xb = jsg.stft(x.reshape(2, 3, L), n, hop, window=win)
    assert Xb.shape == (2, 3, n // 2 + 1, 41) and same_bits(torch, Xb.reshape(6, n // 2 + 1, 41), X)
    yb = jsg.istft(Xb, n, hop, window=win)
    assert yb.shape == (2, 3, L) and same_bits(torch, yb.reshape(6, L), y)
    # a length longer than the span: zeros behind it, like torch.istft
    span_len = 40 * hop + n - n // 2
    yl = jsg.istft(X, n, hop, window=win, length=span_len + 100)
    assert yl.shape == (6, span_len + 100) and same_bits(torch, yl[:, :L], y) and not yl[:, span_len:].any()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)       # torch says that it pads
        ref = torch.istft(X.cpu().to(torch.complex128), n, hop, window=win.double(), length=span_len + 100)
    assert ref.shape == yl.shape and not ref[:, span_len:].any()
    assert float((yl.cpu().double() - ref)[:, :L].abs().max()) <= 1e-5 * float(ref.abs().max())
    Xh = X.transpose(-1, -2).cpu().numpy()      # ... and to the last sample of the span, where the envelope is w[n-1]^2, per sample
    full = R.inverse_f64(Xh, n, hop, win.numpy(), 40 * hop + n)
    R.assert_inverse(yl[:, :span_len].cpu().numpy(), R.slice_ref(full, n // 2, 40 * hop + n), R.inverse_yardstick(Xh, n), "length past the span", n, hop, dead_cap=0)
    # a non-contiguous X: bins-major memory, a strided slice of frames
    Xc = X.contiguous()
    assert Xc.stride(-1) == 1 and X.stride(-1) != 1
    assert same_bits(torch, jsg.istft(Xc, n, hop, window=win), y)
    Xw = torch.zeros((6, n // 2 + 1, 82), dtype=torch.complex64, device="cuda")
    Xw[..., ::2] = X
    assert same_bits(torch, jsg.istft(Xw[..., ::2], n, hop, window=win), y)

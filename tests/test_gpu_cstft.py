"""Complex STFT and inverse STFT on the GPU (jsg_cstft_launch, jsg_istft_launch; include/jsg.h section 2d): forward bins against a
float64 rfft (per-frame L2 and the power bound of parity_util), agreement with the dB path's linear power, torch.stft / torch.istft in
float64, round trips, bit-identical results across scratch sizes, rows and graph replay, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from parity_util import assert_power_close

pytestmark = pytest.mark.gpu

SIZES = [512, 1024, 2048, 4096, 8192]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def signals(kind, rows, L, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(L, dtype=np.float64)
    out = np.zeros((rows, L), np.float32)
    for r in range(rows):
        if kind == "mix":
            f = 0.013 + 0.007 * r
            out[r] = 0.5 * np.sin(2 * np.pi * f * t) + 0.2 * np.sin(2 * np.pi * 0.21 * t + r) + 0.1 * rng.uniform(-1, 1, L)
        elif kind == "sine":
            out[r] = np.sin(2 * np.pi * (0.0371 + 0.001 * r) * t)
        else:   # chirp
            out[r] = 0.9 * np.sin(2 * np.pi * (0.001 + 0.45 * t / (2 * L)) * t + r)
    return out


def frames_f64(x, n, hop, F, w):
    idx = np.arange(F)[:, None] * hop + np.arange(n)[None, :]
    return np.fft.rfft(x.astype(np.float64)[:, idx] * w.astype(np.float64)[None, None, :], axis=-1)


def run_cstft(jsg, torch, plan, x, hop, F):
    n = plan.n
    d_in = torch.from_numpy(x).cuda()
    out = torch.full((x.shape[0], F, n // 2 + 1), complex(7.0, 7.0), dtype=torch.complex64, device="cuda")
    jsg.cstft(plan, d_in, hop, F, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("win", [0, 1, 3, 4])
def test_forward_against_float64(jsg, torch_cuda, n, win):
    w = jsg.window(win, n)
    plan = jsg.CStftPlan(n, w)
    for hop in (n // 4, n // 2, 441, 1, n):
        for rows in (1, 8):
            F = 9 if hop == 1 else (12 if rows == 8 else 20)
            kind = ["mix", "sine", "chirp"][(hop + rows) % 3]
            x = signals(kind, rows, (F - 1) * hop + n, seed=n + hop + rows)
            got = run_cstft(jsg, torch_cuda, plan, x, hop, F)
            ref = frames_f64(x, n, hop, F, w)
            err = np.linalg.norm(got.astype(np.complex128) - ref, axis=-1)
            nrm = np.linalg.norm(ref, axis=-1)
            assert (err <= 1e-6 * nrm).all(), f"n={n} win={win} hop={hop} rows={rows}: worst {np.max(err / nrm):.3g}"
            assert_power_close(np.abs(got.astype(np.complex128)) ** 2, np.abs(ref) ** 2, f"n={n} win={win} hop={hop} rows={rows}")


@pytest.mark.parametrize("n", SIZES)
def test_power_agrees_with_the_db_path(jsg, torch_cuda, n):
    torch = torch_cuda
    w = jsg.window(1, n)
    hop, F = n // 4, 16
    x = signals("mix", 1, (F - 1) * hop + n, seed=3)
    X = run_cstft(jsg, torch, jsg.CStftPlan(n, w), x, hop, F)[0]
    pitch = (n // 2 + 1 + 31) // 32 * 32
    d_p = torch.zeros((F, pitch), device="cuda")
    jsg.stft_db(jsg.Plan(n, w, 1.0), torch.from_numpy(x).cuda(), hop, F, d_p, feedblocks=n // hop, linear_out=True)
    torch.cuda.synchronize()
    p64 = np.abs(frames_f64(x, n, hop, F, w)[0]) ** 2
    assert_power_close(np.abs(X.astype(np.complex128)) ** 2, p64, "cstft")
    assert_power_close(d_p[:, :n // 2 + 1].cpu().numpy(), p64, "stft_db")


@pytest.mark.parametrize("n", [512, 1024, 4096])
@pytest.mark.parametrize("hop_kind", ["q", "h", 441])
def test_round_trip(jsg, torch_cuda, n, hop_kind):
    torch = torch_cuda
    hop = {"q": n // 4, "h": n // 2}.get(hop_kind, 441)
    win = torch.hann_window(n)
    L = (20 + 3 * n // hop) * hop      # a multiple of hop: the last returned sample sits mid-frame, away from the window's tail
    x = torch.from_numpy(signals("mix", 3, L, seed=n)).cuda()
    X = jsg.stft(x, n, hop, window=win)
    tol = 1e-5 * float(x.abs().max())
    y = jsg.istft(X, n, hop, window=win)
    assert y.shape == x.shape and float((y - x).abs().max()) <= tol
    y2 = jsg.istft(X, n, hop, window=win, length=L - 123)
    assert y2.shape == (3, L - 123) and torch.equal(y2, y[:, :L - 123])


@pytest.mark.parametrize("n", SIZES)
def test_forward_against_torch(jsg, torch_cuda, n):
    torch = torch_cuda
    x = torch.from_numpy(signals("chirp", 2, 6 * n + 333, seed=1))
    for center in (True, False):
        for wl, hop in ((n, n // 4), (3 * n // 4, 480)):
            win = torch.hann_window(wl, dtype=torch.float64)
            ref = torch.stft(x.double(), n, hop, wl, window=win, center=center, return_complex=True)
            got = jsg.stft(x.cuda(), n, hop, wl, window=win.float(), center=center)
            assert got.shape == ref.shape and got.dtype == torch.complex64
            g = got.cpu().to(torch.complex128)
            err = torch.linalg.vector_norm(g - ref, dim=-2)
            nrm = torch.linalg.vector_norm(ref, dim=-2)
            assert bool((err <= 1e-6 * nrm).all()), (center, wl, hop, float((err / nrm).max()))
    # a jsg window id and the rectangular default
    ref = torch.stft(x.double(), n, n // 2, window=torch.ones(n, dtype=torch.float64), return_complex=True)
    assert torch.allclose(jsg.stft(x.cuda(), n, n // 2).cpu().to(torch.complex128), ref, rtol=0, atol=1e-6 * float(ref.abs().max()))
    idw = torch.from_numpy(jsg.window(3, n).astype(np.float64))
    ref = torch.stft(x.double(), n, n // 4, window=idw, return_complex=True)
    assert torch.allclose(jsg.stft(x.cuda(), n, window=3).cpu().to(torch.complex128), ref, rtol=0, atol=1e-6 * float(ref.abs().max()))


@pytest.mark.parametrize("n", SIZES)
def test_inverse_against_torch_on_arbitrary_bins(jsg, torch_cuda, n):
    torch = torch_cuda
    rng = np.random.default_rng(n)
    for hop, wl, center in ((n // 4, n, True), (441, n, True), (n // 2, n, False), (n // 4, n // 2, True)):
        F = 11
        Xn = (rng.standard_normal((2, n // 2 + 1, F)) + 1j * rng.standard_normal((2, n // 2 + 1, F)))
        X64 = torch.from_numpy(Xn)
        win = torch.hann_window(wl, dtype=torch.float64) if not (hop == n // 2 and not center) else torch.ones(wl, dtype=torch.float64)
        ref = torch.istft(X64, n, hop, wl, window=win, center=center)
        got = jsg.istft(X64.to(torch.complex64).cuda(), n, hop, wl, window=win.float(), center=center).cpu().double()
        assert got.shape == ref.shape
        assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max()), (hop, wl, center)


def test_inverse_edges_and_torch_refusal(jsg, torch_cuda):
    torch = torch_cuda
    n, hop, F = 1024, 256, 9
    w = torch.hann_window(n)
    rng = np.random.default_rng(5)
    X = torch.from_numpy((rng.standard_normal((1, F, n // 2 + 1)) + 1j * rng.standard_normal((1, F, n // 2 + 1))).astype(np.complex64)).cuda()
    plan = jsg.CStftPlan(n, w.numpy())
    T = (F - 1) * hop + n
    y = torch.full((1, T), 5.0, device="cuda")
    jsg.istft_launch(plan, X, hop, F, y)
    torch.cuda.synchronize()
    y = y.cpu().double()[0]
    assert float(y[0]) == 0.0        # w[0] = 0: the envelope of the first sample is zero
    Xt = X.cpu().to(torch.complex128).transpose(1, 2)
    frames = torch.fft.irfft(Xt, n, dim=1) * w.double()[None, :, None]
    ola = torch.zeros(T, dtype=torch.float64)
    env = torch.zeros(T, dtype=torch.float64)
    for j in range(F):
        ola[j * hop:j * hop + n] += frames[0, :, j]
        env[j * hop:j * hop + n] += w.double() ** 2
    assert bool((y[env <= 1e-11] == 0).all()) and int((env <= 1e-11).sum()) >= 1
    ok = env > 1e-3                  # where the quotient is well conditioned (the very edges divide by w^2 ~ 1e-10)
    want = ola / env
    assert float((y[ok] - want[ok]).abs().max()) <= 1e-5 * float(want[ok].abs().max())
    with pytest.raises(RuntimeError):
        torch.istft(Xt, n, hop, window=w.double(), center=False)
    with pytest.raises(jsg.JsgError):
        jsg.istft(X.transpose(1, 2), n, hop, window=w, center=False)
    jsg.istft(X.transpose(1, 2), n, hop, window=w, center=True)            # ... and neither raises with centring
    torch.istft(Xt, n, hop, window=w.double(), center=True)


def test_determinism_scratch_rows_and_repeat(jsg, torch_cuda):
    torch = torch_cuda
    for n, hop in ((1024, 441), (2048, 512), (512, 1)):
        w = jsg.window(1, n)
        plan = jsg.CStftPlan(n, w)
        rows, F = 4, (40 if hop > 1 else 12)
        x = torch.from_numpy(signals("mix", rows, (F - 1) * hop + n, seed=9)).cuda()
        X = torch.empty((rows, F, n // 2 + 1), dtype=torch.complex64, device="cuda")
        jsg.cstft(plan, x, hop, F, X)
        X2 = torch.empty_like(X)
        jsg.cstft(plan, x, hop, F, X2)
        Xr = torch.empty_like(X)
        for r in range(rows):
            jsg.cstft(plan, x[r:r + 1], hop, F, Xr[r:r + 1])
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(X), torch.view_as_real(X2)) and torch.equal(torch.view_as_real(X), torch.view_as_real(Xr))
        T = (F - 1) * hop + n
        K = (n - 1) // hop
        outs = []
        for per_row in (F, min(F, K + 1), min(F, K + 2), min(F, K + 7), max(F - 1, min(F, K + 1))):   # the smallest accepted size .. the whole call
            y = torch.full((rows, T), 3.0, device="cuda")
            sc = torch.empty(rows * n * per_row + 3, dtype=torch.float32, device="cuda")
            jsg.istft_launch(plan, X, hop, F, y, d_scratch=sc)
            outs.append(y)
        yr = torch.full((rows, T), 3.0, device="cuda")
        for r in range(rows):
            jsg.istft_launch(plan, X[r:r + 1], hop, F, yr[r:r + 1])
        y_again = torch.full((rows, T), 3.0, device="cuda")
        jsg.istft_launch(plan, X, hop, F, y_again)
        torch.cuda.synchronize()
        for y in outs[1:] + [yr, y_again]:
            assert torch.equal(y, outs[0]), (n, hop)


def test_refusals(jsg, torch_cuda):
    torch = torch_cuda
    lib = jsg.capi.lib()
    n, hop, F, rows = 1024, 256, 8, 2
    w = jsg.window(1, n)
    plan = jsg.CStftPlan(n, w)
    x = torch.zeros((rows, (F - 1) * hop + n), device="cuda")
    X = torch.full((rows, F, n // 2 + 1), complex(9, 9), dtype=torch.complex64, device="cuda")
    good = jsg.spectrogram._cstft_args(plan, x, hop, F, X, None)

    def fwd(**kw):
        a = jsg.capi.CstftArgs.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.jsg_cstft_launch(plan._p, C.byref(a), None)

    E = jsg.capi.JSG_ERR_INVALID
    for kw in (dict(in_=None), dict(out=None), dict(hop=0), dict(hop=n + 1), dict(out_frame_pitch=n // 2), dict(out_row_pitch=100),
               dict(in_samples=x.shape[1] - 1), dict(rows=0), dict(n_frames=-1), dict(in_pitch=-1), dict(out=X.data_ptr() + 4)):
        assert fwd(**kw) == E, kw
        assert lib.jsg_last_error(None)
    torch.cuda.synchronize()
    assert bool((torch.view_as_real(X) == 9).all())
    assert fwd() == 0
    # inverse: a refused call, chunked or not, leaves the output untouched
    y = torch.full((rows, (F - 1) * hop + n), 4.0, device="cuda")
    gi = jsg.spectrogram._istft_args(plan, X, hop, F, y, None)
    sc = torch.empty(rows * n * F, device="cuda")

    def inv(scratch=sc.data_ptr(), floats=sc.numel(), p=plan._p, **kw):
        a = jsg.capi.IstftArgs.from_buffer_copy(gi)
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.jsg_istft_launch(p, C.byref(a), scratch, floats, None)

    small = rows * n * ((n - 1) // hop + 1)
    for kw in (dict(in_=None), dict(out=None), dict(hop=0), dict(hop=n + 1), dict(hop=n), dict(in_frame_pitch=n // 2),
               dict(in_row_pitch=10), dict(out_pitch=10), dict(out_samples=0), dict(out_samples=(F - 1) * hop + n + 1),
               dict(scratch=None), dict(floats=small - 1), dict(floats=small - 1, out_pitch=10), dict(scratch=sc.data_ptr() + 4),
               dict(n_frames=0), dict(rows=0), dict(p=None), dict(in_=X.data_ptr() + 4)):
        assert inv(**kw) == E, kw
    torch.cuda.synchronize()
    assert bool((y == 4.0).all())
    assert inv(floats=small) == 0
    # a plan made on another device is refused
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1):
            assert fwd() == E
            assert inv() == E
    # Python: torch's refusal (NOLA in the span)
    with pytest.raises(jsg.JsgError):
        jsg.istft(X.transpose(1, 2), n, n, window=torch.hann_window(n), center=True)


def test_graph_capture_matches_eager(jsg, torch_cuda):
    torch = torch_cuda
    n, hop, F, rows = 2048, 480, 30, 2
    w = jsg.window(1, n)
    plan = jsg.CStftPlan(n, w)
    L = (F - 1) * hop + n
    x = torch.zeros((rows, L), device="cuda")
    X = torch.empty((rows, F, n // 2 + 1), dtype=torch.complex64, device="cuda")
    y = torch.empty((rows, L), device="cuda")
    sc = torch.empty(rows * n * 8, device="cuda")        # several chunks
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        jsg.cstft(plan, x, hop, F, X, stream=s.cuda_stream)          # warm-up outside capture
        jsg.istft_launch(plan, X, hop, F, y, d_scratch=sc, stream=s.cuda_stream)
    s.synchronize()
    with torch.cuda.graph(g, stream=s):
        jsg.cstft(plan, x, hop, F, X, stream=s.cuda_stream)
        jsg.istft_launch(plan, X, hop, F, y, d_scratch=sc, stream=s.cuda_stream)
    for seed in (1, 2):
        x.copy_(torch.from_numpy(signals("mix", rows, L, seed=seed)))
        g.replay()
        torch.cuda.synchronize()
        Xe = torch.empty_like(X)
        ye = torch.empty_like(y)
        jsg.cstft(plan, x, hop, F, Xe)
        jsg.istft_launch(plan, Xe, hop, F, ye, d_scratch=torch.empty(rows * n * 8, device="cuda"))
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(X), torch.view_as_real(Xe)) and torch.equal(y, ye)

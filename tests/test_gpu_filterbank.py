"""Filterbank spectrograms on the GPU (jsg_stft_fb_launch(_strided), include/jsg.h section 2b).

The bit-exact chain: the STFT kernel's linear power is reproduced by the CPU mirror of the kernel (oracle/jsg_mirror.c, plan named by
jsg_stft_fb_kernel_name), the bank by a float32 numpy loop in the specified order (bins ascending from +0.0f, every product and every sum
rounded on its own), the logarithm by the shared float32 routine (exact_log).  Beside it: the LINEAR identity bank against stft_db, the
hardware logarithm, a float64 bound, chunking, strided calls and ring wrap, NaN containment, refusals, graph capture, colour, torch.
The band kernel on its own -- every tile size and bank path, second tiles, partial tiles, band-count edges -- is in tests/test_gpu_fb_band.py
(references: tests/fb_band_ref.py)."""
import ctypes

import numpy as np
import pytest

from fb_band_ref import band_dense, band_f32
from parity_util import DB_SLACK, FLOOR_BY_N, LOG_FLOOR
from test_gpu_fullsize import _b_rule

pytestmark = pytest.mark.gpu

MIX = {"absmean2": (0, 2), "absmean3": (0, 3), "max": (1, 2), "min": (2, 2), "left": (3, 2), "right": (4, 2), "sum": (101, 2),
       "perch": (100, 2)}
PINS = [(512, 0), (1024, 1), (1024, 2), (2048, 1), (2048, 2), (2048, 3), (4096, 1), (4096, 2), (8192, 0)]
FS = 48000.0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def mir():
    from oracle import mirror
    return mirror.load()


def bank_for(jsg, n, scale, B=48):
    C = jsg.capi
    if scale == C.FB_LOG:
        return jsg.Filterbank(n, FS, B, 40.0, 20000.0, scale=scale)
    if scale == C.FB_LINEAR:
        return jsg.Filterbank(n, FS, B, 100.0, 12000.0, scale=scale)
    return jsg.Filterbank(n, FS, B, 0.0, FS / 2, scale=scale)


def run_fb(jsg, torch, plan, fb, x, hop, F, *, mix=0, pin=0, exact=True, linear=False, W=None, pos=0, scratch=None, feedblocks=None,
           first_frame=0):
    d_in = torch.from_numpy(x).cuda()
    W = W or F
    shape = (x.shape[0], W, fb.n_bands + 3) if mix == 100 else (W, fb.n_bands + 3)
    d_out = torch.full(shape, -7.0, dtype=torch.float32, device="cuda")
    kw = dict(mix_mode=mix, plan_select=pin, exact_log=exact, linear_out=linear, ring_pos=pos, feedblocks=feedblocks, first_frame=first_frame)
    name = jsg.stft_fb_kernel_name(plan, fb, d_in, hop, F, d_out, **kw)
    d_sc = None if scratch is None else torch.empty(scratch, dtype=torch.float32, device="cuda")
    jsg.stft_fb_db(plan, fb, d_in, hop, F, d_out, d_scratch=d_sc, **kw)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), name


def mirror_bands(mir, name, x, hop, F, win, fb, mix, feedblocks=None, first_frame=0):
    if mix == 100:
        return np.stack([band_f32(mir.columns(name, x[c:c + 1], hop, F, win, feedblocks=feedblocks, mix=3, first_frame=first_frame), fb)
                         for c in range(x.shape[0])])
    return band_f32(mir.columns(name, x, hop, F, win, feedblocks=feedblocks, mix=mix, first_frame=first_frame), fb)


@pytest.mark.parametrize("n,pin", PINS)
def test_bit_exact_chain(jsg, oracle, mir, torch_cuda, n, pin):
    torch = torch_cuda
    C = jsg.capi
    win = oracle.window(oracle.WIN_HANN, n)
    plan = jsg.Plan(n, win)
    F = 24
    for i, (mname, (mix, ch)) in enumerate(MIX.items()):
        if pin == 3 and mname not in ("absmean2", "sum"):
            continue
        scale = i % 4
        fb = bank_for(jsg, n, scale)
        irregular = mname == "absmean3"      # the reference's perc10 hop: 10 frames per block, hop int(0.1 n + 0.5)
        hop, fbk = (int(0.1 * n + 0.5), 10) if irregular else (n // 2, None)
        L = (F // 10 + 2) * n if irregular else (F - 1) * hop + n
        x = oracle.synth_audio(ch, L, seed=n + i)
        got, name = run_fb(jsg, torch, plan, fb, x, hop, F, mix=mix, pin=pin, feedblocks=fbk)
        if pin == 2:
            assert name == f"Cfg{n}B" or (n == 1024 and mix in (1, 2)), (name, mname)
        if pin == 3:
            assert name == "Cfg2048P", name
        want = mir.exact_db(mirror_bands(mir, name, x, hop, F, win, fb, mix, feedblocks=fbk))
        g = got[..., :fb.n_bands]
        assert (g.view(np.uint32) == want.view(np.uint32)).all(), (name, mname, scale, int((g != want).sum()))
        assert (got[..., fb.n_bands:] == -7.0).all()          # nothing written past the bands
        lin, _ = run_fb(jsg, torch, plan, fb, x, hop, F, mix=mix, pin=pin, linear=True, feedblocks=fbk)
        wl = mirror_bands(mir, name, x, hop, F, win, fb, mix, feedblocks=fbk)
        assert (lin[..., :fb.n_bands].view(np.uint32) == wl.view(np.uint32)).all(), (name, mname, "linear")


@pytest.mark.parametrize("n,pin", PINS)
def test_linear_identity_equals_stft_db(jsg, oracle, torch_cuda, n, pin):
    torch = torch_cuda
    H = n // 2 + 1
    win = oracle.window(oracle.WIN_HANN, n)
    plan = jsg.Plan(n, win)
    fb = jsg.Filterbank(n, FS, H, 0.0, FS / 2, scale=jsg.capi.FB_LINEAR, norm=jsg.capi.FB_NORM_UNIT_SUM)
    ch, F = (2, 64)
    x = oracle.synth_audio(ch, (F - 1) * (n // 2) + n, seed=7 * n)
    d_in = torch.from_numpy(x).cuda()
    for exact in (False, True):
        got, name = run_fb(jsg, torch, plan, fb, x, n // 2, F, pin=pin, exact=exact)
        sel = {"": 1, "B": 2, "P": 3}[name[len(f"Cfg{n}"):]] if n in (1024, 2048, 4096) else 0
        d_ref = torch.zeros((F, H), dtype=torch.float32, device="cuda")
        jsg.stft_db(plan, d_in, n // 2, F, d_ref, plan_select=sel, exact_log=exact)
        assert jsg.stft_kernel_name(plan, d_in, n // 2, F, d_ref, plan_select=sel) == name
        ref = d_ref.cpu().numpy()
        assert (got[:, :H].view(np.uint32) == ref.view(np.uint32)).all(), (name, exact, int((got[:, :H] != ref).sum()))


@pytest.mark.parametrize("n", [1024, 4096])
def test_hardware_log_and_float64_bound(jsg, oracle, torch_cuda, n):
    """Hardware log within DB_SLACK of the exact one.  Against float64 (DFT power in float64, the bank in float64):
        |band_gpu - band_64| <= sum_k w_k (1e-5 P_k + FLOOR(n) P_peak) + (n_bins + 1) * 2^-24 * sum_k |w_k| P_k
    -- the power bound of parity_util per bin carried through the weights, plus the float32 summation term (one rounding per product and
    per sum)."""
    torch = torch_cuda
    win = oracle.window(oracle.WIN_HANN, n)
    plan = jsg.Plan(n, win)
    fb = jsg.Filterbank(n, FS, 128, 0.0, FS / 2)
    F, hop, ch = 40, n // 4, 2
    x = oracle.synth_audio(ch, (F - 1) * hop + n, seed=n)
    hw, name = run_fb(jsg, torch, plan, fb, x, hop, F, exact=False)
    ex, _ = run_fb(jsg, torch, plan, fb, x, hop, F, exact=True)
    B = fb.n_bands
    assert np.abs(hw[:, :B].astype(np.float64) - ex[:, :B]).max() <= DB_SLACK
    lin, _ = run_fb(jsg, torch, plan, fb, x, hop, F, linear=True)
    idx = (np.arange(F) * hop)[:, None] + np.arange(n)[None, :]
    frames = x[:, idx].astype(np.float64) * win.astype(np.float64)[None, None, :]
    P = (np.abs(np.fft.rfft(frames, axis=-1)) ** 2).mean(axis=0)            # AbsMean of 2 channels, float64
    Wd = fb.matrix().astype(np.float64)
    band64 = P @ Wd.T
    peak = P.max(axis=1, keepdims=True)
    tol = (1e-5 * P + FLOOR_BY_N[n] * peak) @ Wd.T + (fb.n_bins[None, :] + 1) * 2.0 ** -24 * (P @ np.abs(Wd).T)
    err = np.abs(lin[:, :B].astype(np.float64) - band64)
    assert (err <= tol).all(), f"{name}: worst ratio {np.max(err / np.maximum(tol, 1e-300)):.3g}"


def test_chunking_does_not_change_bits_and_keeps_one_plan(jsg, oracle, mir, torch_cuda):
    torch = torch_cuda
    n, ch = 1024, 4
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    w = 1
    while not _b_rule(w * 32, 32, n_cu):
        w += 1
    F = w * 32 + 5                       # the whole call fills the rounds of Cfg1024B; a chunk of 32 columns alone would not
    assert _b_rule(F, 32, n_cu) and not _b_rule(32, 32, n_cu)
    win = oracle.window(oracle.WIN_HANN, n)
    plan = jsg.Plan(n, win)
    fb = jsg.Filterbank(n, FS, 64, 0.0, FS / 2)
    x = oracle.synth_audio(ch, (F - 1) * 512 + n, seed=11)
    pitch = 544                           # floats per power column in scratch (n/2+1 rounded up to whole 128-byte lines)
    outs = []
    for cols in (32, 33, 96, 1000, None):
        got, name = run_fb(jsg, torch, plan, fb, x, 512, F, scratch=None if cols is None else cols * pitch)
        assert name == "Cfg1024B", name
        outs.append(got)
    for o in outs[1:]:
        assert (o.view(np.uint32) == outs[0].view(np.uint32)).all()
    want = mir.exact_db(mirror_bands(mir, "Cfg1024B", x, 512, F, win, fb, 0))
    assert (outs[0][:, :64].view(np.uint32) == want.view(np.uint32)).all()
    other, name1 = run_fb(jsg, torch, plan, fb, x, 512, F, pin=1, scratch=32 * pitch)
    assert name1 == "Cfg1024" and (other.view(np.uint32) != outs[0].view(np.uint32)).any()   # the two plans differ on this input
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.zeros((F, 64), dtype=torch.float32, device="cuda")
    with pytest.raises(jsg.JsgError) as e:                                  # less than one workgroup step of Cfg1024B
        jsg.stft_fb_db(plan, fb, d_in, 512, F, d_out, d_scratch=torch.empty(31 * pitch, device="cuda"))
    assert e.value.code == jsg.capi.JSG_ERR_INVALID


def test_strided_equals_single_calls_and_ring_wraps(jsg, oracle, torch_cuda):
    torch = torch_cuda
    n, ch, F, K, W = 2048, 2, 50, 5, 64
    win = oracle.window(oracle.WIN_HANN, n)
    plan = jsg.Plan(n, win)
    fb = jsg.Filterbank(n, FS, 80, 30.0, 20000.0, scale=jsg.capi.FB_LOG)
    for mix in (0, 100):
        xs = np.stack([oracle.synth_audio(ch, (F - 1) * 1024 + n, seed=20 + k) for k in range(K)])
        d_in = torch.from_numpy(xs).cuda()
        shape = (K, ch, W, 96) if mix == 100 else (K, W, 96)
        d_out = torch.full(shape, -7.0, dtype=torch.float32, device="cuda")
        kw = dict(mix_mode=mix, exact_log=True, ring_pos=W - 7)
        name = jsg.stft_fb_kernel_name(plan, fb, d_in, 1024, F, d_out, strided=True, **kw)
        sel = {"": 1, "B": 2, "P": 3}[name[len(f"Cfg{n}"):]]
        jsg.stft_fb_db_strided(plan, fb, d_in, 1024, F, d_out, d_scratch=torch.empty(3 * 1056 * F * ch, device="cuda"), **kw)
        for k in range(K):
            got1, n1 = run_fb(jsg, torch, plan, fb, xs[k], 1024, F, mix=mix, pin=sel, W=W, pos=W - 7)
            assert n1 == name
            got = d_out[k].cpu().numpy()
            assert (got[..., :80].view(np.uint32) == got1[..., :80].view(np.uint32)).all(), (mix, k)
        cols = (np.arange(F) + W - 7) % W
        untouched = np.setdiff1d(np.arange(W), cols)
        assert (d_out.cpu().numpy()[..., untouched, :] == -7.0).all()


def test_nan_sample_reaches_exactly_its_columns(jsg, oracle, torch_cuda):
    torch = torch_cuda
    n, hop, F = 1024, 256, 40
    win = oracle.window(oracle.WIN_HANN, n)
    plan = jsg.Plan(n, win)
    fb = jsg.Filterbank(n, FS, 64, 0.0, FS / 2)
    x = oracle.synth_audio(2, (F - 1) * hop + n, seed=5)
    s = 9000
    x[1, s] = np.nan
    got, _ = run_fb(jsg, torch, plan, fb, x, hop, F)
    hit = np.array([j * hop <= s < j * hop + n for j in range(F)])
    nan = np.isnan(got[:, :64])
    assert nan[hit].all() and not nan[~hit].any()


def test_empty_bands_read_minus_110_db(jsg, oracle, mir, torch_cuda):
    torch = torch_cuda
    n = 512
    plan = jsg.Plan(n, oracle.window(oracle.WIN_HANN, n))
    fb = jsg.Filterbank(n, FS, 128, 0.0, FS / 2)
    empty = fb.n_bins == 0
    assert empty.any()
    x = oracle.synth_audio(1, 15 * 256 + n, seed=1)
    for exact in (True, False):
        got, _ = run_fb(jsg, torch, plan, fb, x, 256, 16, exact=exact)
        e = got[:, :128][:, empty]
        floor_db = mir.exact_db(np.zeros(1, np.float32))[0]
        assert abs(floor_db + 110.0) < 1e-4
        assert (e == floor_db).all() if exact else np.abs(e - floor_db).max() <= DB_SLACK


def test_refusals(jsg, oracle, torch_cuda):
    torch = torch_cuda
    C = jsg.capi
    lib = C.lib()
    n, F = 1024, 16
    plan = jsg.Plan(n, oracle.window(oracle.WIN_HANN, n))
    fb = jsg.Filterbank(n, FS, 40, 0.0, FS / 2)
    fb2 = jsg.Filterbank(2048, FS, 40, 0.0, FS / 2)
    x = torch.from_numpy(oracle.synth_audio(1, (F - 1) * 512 + n, seed=2)).cuda()
    out = torch.zeros((F, 40), dtype=torch.float32, device="cuda")
    sc = torch.empty(1 << 20, dtype=torch.float32, device="cuda")
    a = jsg.spectrogram._stft_args(plan, x, 512, F, out, col_height=40)
    h = fb.handle()

    def call(p=plan._p, f=h, args=a, s=sc.data_ptr(), sf=sc.numel()):
        return lib.jsg_stft_fb_launch(p, f, ctypes.byref(args) if args is not None else None, s, sf, None)

    assert call() == C.JSG_OK
    assert call(f=fb2.handle()) == C.JSG_ERR_INVALID                  # another FFT size
    assert call(p=None) == C.JSG_ERR_INVALID and call(f=None) == C.JSG_ERR_INVALID and call(args=None) == C.JSG_ERR_INVALID
    assert call(s=None) == C.JSG_ERR_INVALID
    assert call(sf=4 * 544 - 1) == C.JSG_ERR_INVALID                    # less than one workgroup step (4 columns of Cfg1024)
    assert call(s=sc.data_ptr() + 4) == C.JSG_ERR_INVALID               # not 16-byte aligned
    b = C.StftArgs.from_buffer_copy(a); b.out_pitch = 39
    assert call(args=b) == C.JSG_ERR_INVALID                            # out_pitch < n_bands
    b = C.StftArgs.from_buffer_copy(a); b.out_tail = out.data_ptr()
    assert call(args=b) == C.JSG_ERR_INVALID                            # out_tail set
    b = C.StftArgs.from_buffer_copy(a); b.out_db = None
    assert call(args=b) == C.JSG_ERR_INVALID
    b = C.StftArgs.from_buffer_copy(a); b.ring_width = F - 1
    assert call(args=b) == C.JSG_ERR_INVALID                            # n_frames > ring_width
    b = C.StftArgs.from_buffer_copy(a); b.n_frames = F + 1
    assert call(args=b) == C.JSG_ERR_INVALID                            # reads past in_samples (and more frames than ring columns)
    buf = ctypes.create_string_buffer(32)
    assert lib.jsg_stft_fb_kernel_name(plan._p, fb2.handle(), ctypes.byref(a), 1, buf, 32) == C.JSG_ERR_INVALID
    torch.cuda.synchronize()


def test_refuses_a_bank_or_plan_of_another_device(jsg, oracle, torch_cuda):
    torch = torch_cuda
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs in the process: a bank or plan created on device 1, launched on device 0")
    C = jsg.capi
    n, F = 1024, 16
    plan = jsg.Plan(n, oracle.window(oracle.WIN_HANN, n))
    fb = jsg.Filterbank(n, FS, 40, 0.0, FS / 2)
    with torch.cuda.device(1):
        plan1 = jsg.Plan(n, oracle.window(oracle.WIN_HANN, n))
        h1 = fb.handle(1)
    x = torch.from_numpy(oracle.synth_audio(1, (F - 1) * 512 + n, seed=2)).cuda()
    out = torch.zeros((F, 40), dtype=torch.float32, device="cuda")
    sc = torch.empty(1 << 20, dtype=torch.float32, device="cuda")
    a = jsg.spectrogram._stft_args(plan, x, 512, F, out, col_height=40)
    lib = C.lib()
    assert lib.jsg_stft_fb_launch(plan._p, h1, ctypes.byref(a), sc.data_ptr(), sc.numel(), None) == C.JSG_ERR_INVALID
    assert lib.jsg_stft_fb_launch(plan1._p, fb.handle(0), ctypes.byref(a), sc.data_ptr(), sc.numel(), None) == C.JSG_ERR_INVALID
    torch.cuda.synchronize()


def test_refused_call_enqueues_nothing(jsg, oracle, torch_cuda):
    """A strided call cut into one-batch chunks (small scratch): every refusal is decided for the whole call before the first chunk."""
    torch = torch_cuda
    C = jsg.capi
    lib = C.lib()
    n, ch, F, K = 1024, 2, 64, 4
    plan = jsg.Plan(n, oracle.window(oracle.WIN_HANN, n))
    fb = jsg.Filterbank(n, FS, 40, 0.0, FS / 2)
    xs = torch.from_numpy(np.stack([oracle.synth_audio(ch, (F - 1) * 512 + n, seed=30 + k) for k in range(K)])).cuda()
    out = torch.full((K, F, 40), -7.0, dtype=torch.float32, device="cuda")
    sc = torch.empty(16 * 544, dtype=torch.float32, device="cuda")        # 16 columns: four chunks per batch
    a = jsg.spectrogram._stft_args(plan, xs[0], 512, F, out[0], col_height=40)

    def call(args):
        rc = lib.jsg_stft_fb_launch_strided(plan._p, fb.handle(), ctypes.byref(args), K, xs.stride(0), out.stride(0), sc.data_ptr(),
                                            sc.numel(), None)
        torch.cuda.synchronize()
        return rc

    for change in (dict(in_pitch=a.in_samples - 1), dict(n_frames=F + 1), dict(mix_mode=7), dict(hop=0),
                   dict(first_frame=(1 << 31) - F)):
        b = C.StftArgs.from_buffer_copy(a)
        for k, v in change.items():
            setattr(b, k, v)
        assert call(b) < 0, change
        assert (out == -7.0).all(), change
    assert call(a) == C.JSG_OK and not (out == -7.0).any()


def test_dense_caller_bank(jsg, oracle, mir, torch_cuda):
    """jsg_filterbank_create_matrix / jsg_filterbank_weights through the C path, and one launch with that bank."""
    torch = torch_cuda
    C = jsg.capi
    n, F, hop = 2048, 32, 512
    H = n // 2 + 1
    rng = np.random.default_rng(8)
    W = np.zeros((24, H), np.float32)
    for b in range(20):
        a = int(rng.integers(0, H - 60))
        W[b, a:a + 50] = rng.random(50).astype(np.float32) + 0.05
        W[b, a + 7] = 0.0                  # interior zeros
        W[b, a + 20:a + 23] = 0.0
        W[b, a + 30] = -0.5                # a negative weight
    W[20] = 0.0                            # an empty row
    W[21] = rng.random(H).astype(np.float32) + 0.01          # full width, nonzero at both ends
    W[22, 0] = 2.0                         # full width, zeros inside
    W[22, H - 1] = 1e-30
    W[23, H - 1] = 1.0                     # only the last bin
    fb = jsg.Filterbank.from_matrix(W)
    got_w = fb.device_weights()
    assert (got_w.view(np.uint32) == W.view(np.uint32)).all()
    win = oracle.window(oracle.WIN_HANN, n)
    plan = jsg.Plan(n, win)
    x = oracle.synth_audio(2, (F - 1) * hop + n, seed=12)
    got, name = run_fb(jsg, torch, plan, fb, x, hop, F, linear=True)
    P = mir.columns(name, x, hop, F, win)
    want = band_dense(P, W)
    assert (got[:, :24].view(np.uint32) == want.view(np.uint32)).all(), int((got[:, :24] != want).sum())
    got_db, _ = run_fb(jsg, torch, plan, fb, x, hop, F, exact=True)
    want_db = mir.exact_db(np.maximum(want, 0.0))
    ok = want >= 0                                           # (a negative band power is outside the logarithm's contract)
    assert ok.mean() > 0.9 and (got_db[:, :24].view(np.uint32)[ok] == want_db.view(np.uint32)[ok]).all()
    for bad in (np.nan, np.inf):
        Wb = W.copy()
        Wb[3, 500] = bad
        with pytest.raises(jsg.JsgError) as e:
            jsg.Filterbank.from_matrix(Wb).handle()
        assert e.value.code == C.JSG_ERR_INVALID


def test_graph_capture_replays_to_the_same_bits(jsg, oracle, torch_cuda):
    torch = torch_cuda
    n, F = 2048, 300
    plan = jsg.Plan(n, oracle.window(oracle.WIN_HANN, n))
    fb = jsg.Filterbank(n, FS, 128, 0.0, FS / 2)
    x = torch.from_numpy(oracle.synth_audio(2, (F - 1) * 512 + n, seed=9)).cuda()
    ref = torch.zeros((F, 128), dtype=torch.float32, device="cuda")
    out = torch.zeros_like(ref)
    sc = torch.empty(64 * 1056, dtype=torch.float32, device="cuda")       # several chunks
    jsg.stft_fb_db(plan, fb, x, 512, F, ref, d_scratch=sc, exact_log=True)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            jsg.stft_fb_db(plan, fb, x, 512, F, out, d_scratch=sc, exact_log=True, stream=st.cuda_stream)
    torch.cuda.synchronize()
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == ref.cpu().numpy().view(np.uint32)).all()


def test_colormap_over_band_columns(jsg, oracle, mir, torch_cuda):
    torch = torch_cuda
    n, F, B = 4096, 48, 200
    win = oracle.window(oracle.WIN_HANN, n)
    plan = jsg.Plan(n, win)
    fb = jsg.Filterbank(n, FS, B, 20.0, 20000.0, scale=jsg.capi.FB_LOG)
    x = oracle.synth_audio(2, (F - 1) * 1024 + n, seed=3)
    d_in = torch.from_numpy(x).cuda()
    d_db = torch.zeros((F, B), dtype=torch.float32, device="cuda")
    jsg.stft_fb_db(plan, fb, d_in, 1024, F, d_db, exact_log=True)
    name = jsg.stft_fb_kernel_name(plan, fb, d_in, 1024, F, d_db, exact_log=True)
    d_lut = torch.from_numpy(jsg.colormap_lut(256, jsg.capi.CM_JADE)).cuda()
    d_img = torch.zeros((B, F), dtype=torch.int32, device="cuda")
    jsg.colormap(d_db, d_lut, -80.0, 20.0, d_argb=d_img, height=B)
    torch.cuda.synchronize()
    bands = mir.exact_db(mirror_bands(mir, name, x, 1024, F, win, fb, 0))
    pal = oracle.OracleColorPalette(256, oracle.CM_JADE)
    pal.set_value_range(-80.0, 20.0)
    lut = jsg.colormap_lut(256, jsg.capi.CM_JADE).astype(np.uint32) | np.uint32(0xFF000000)
    want = lut[pal.index(bands).astype(np.int64)]                              # [F][B]
    got = d_img.cpu().numpy().view(np.uint32)[::-1, :].T                     # image row height-1-b holds band b
    assert int((got != want).sum()) == 0


def test_mel_spectrogram_db_equals_the_raw_launch(jsg, oracle, torch_cuda):
    torch = torch_cuda
    n, hop, M = 2048, 512, 128
    x = torch.from_numpy(oracle.synth_audio(2, 48000, seed=4)).cuda()
    got = jsg.mel_spectrogram_db(x, 44100.0, n, hop, M, fmin=20.0, fmax=16000.0, exact_log=True)
    F = 1 + (48000 - n) // hop
    assert tuple(got.shape) == (F, M) and got.device == x.device
    plan = jsg.Plan(n, jsg.window(jsg.capi.WIN_HANN, n))
    fb = jsg.Filterbank(n, 44100.0, M, 20.0, 16000.0)
    ref = torch.zeros((F, M), dtype=torch.float32, device="cuda")
    jsg.stft_fb_db(plan, fb, x, hop, F, ref, exact_log=True)
    torch.cuda.synchronize()
    assert (got.cpu().numpy().view(np.uint32) == ref.cpu().numpy().view(np.uint32)).all()
    again = jsg.mel_spectrogram_db(x[0], 44100.0, n, hop, M, fmin=20.0, fmax=16000.0)   # mono, cached plan and bank
    assert tuple(again.shape) == (F, M) and torch.isfinite(again).all()

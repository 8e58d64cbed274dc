"""The launches that work through scratch memory, called without a scratch tensor AND with a stream that is not torch's current one:
the binding then allocates the scratch for the call and records it on the caller's stream, so that the caching allocator cannot hand
the block out again under the running kernels.  Bit for bit the result of the same call with the caller's own scratch on the current
stream."""
import ctypes

import numpy as np
import pytest

import pvoc_ref as pr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def side_stream(torch):
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())       # the inputs were written on the current stream
    assert st.cuda_stream != torch.cuda.current_stream().cuda_stream
    return st


def bits(torch, t):
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)


def test_stft_fb_db(jsg, oracle, torch_cuda):
    torch = torch_cuda
    n, hop, F, bands = 512, 128, 16, 40
    plan = jsg.Plan(n, oracle.window(oracle.WIN_HANN, n))
    fb = jsg.Filterbank(n, 48000.0, bands)
    x = torch.from_numpy(oracle.synth_audio(1, (F - 1) * hop + n, seed=5)).cuda()
    want = torch.zeros((F, bands), dtype=torch.float32, device="cuda")
    sc = torch.empty(jsg.stft_fb_scratch_floats(plan, fb, x, hop, F, want, exact_log=True), dtype=torch.float32, device="cuda")
    jsg.stft_fb_db(plan, fb, x, hop, F, want, d_scratch=sc, exact_log=True)
    got = torch.zeros_like(want)
    st = side_stream(torch)
    jsg.stft_fb_db(plan, fb, x, hop, F, got, exact_log=True, stream=st.cuda_stream)
    torch.cuda.synchronize()
    assert torch.isfinite(want).all() and torch.equal(bits(torch, got), bits(torch, want))


def test_istft_launch(jsg, torch_cuda):
    torch = torch_cuda
    n, hop, F = 512, 128, 9
    plan = jsg.CStftPlan(n, jsg.window(jsg.capi.WIN_HANN, n))
    T = (F - 1) * hop + n
    rng = np.random.default_rng(11)
    X = torch.from_numpy((rng.standard_normal((1, F, n // 2 + 1)) + 1j * rng.standard_normal((1, F, n // 2 + 1))).astype(np.complex64)).cuda()
    want = torch.zeros((1, T), dtype=torch.float32, device="cuda")
    sc = torch.empty(n * 5, dtype=torch.float32, device="cuda")          # the three overlapping frames and two new ones per chunk
    jsg.istft_launch(plan, X, hop, F, want, d_scratch=sc)
    got = torch.zeros_like(want)
    st = side_stream(torch)
    jsg.istft_launch(plan, X, hop, F, got, stream=st.cuda_stream)
    torch.cuda.synchronize()
    assert want.abs().max() > 0 and torch.equal(bits(torch, got), bits(torch, want))


def test_phase_vocoder_launch(jsg, torch_cuda):
    torch = torch_cuda
    n, hop, T, rate, chunk = 512, 128, 9, 1.3, 4
    X = torch.from_numpy(np.array(pr.make_input(n, hop, T))).cuda()[None]
    want = torch.zeros((1, jsg.pvoc_frames(T, rate), n // 2 + 1), dtype=torch.complex64, device="cuda")
    assert want.shape[1] > chunk                                         # more than one chunk
    a = jsg.spectrogram._pvoc_args(X, rate, hop, n, want, chunk)
    sc = torch.empty(jsg.capi.lib().jsg_pvoc_scratch_bytes(ctypes.byref(a)) // 4, dtype=torch.int32, device="cuda")
    jsg.phase_vocoder_launch(X, rate, hop, n, want, chunk_frames=chunk, d_scratch=sc)
    got = torch.zeros_like(want)
    st = side_stream(torch)
    jsg.phase_vocoder_launch(X, rate, hop, n, got, chunk_frames=chunk, stream=st.cuda_stream)
    torch.cuda.synchronize()
    assert want.abs().max() > 0 and torch.equal(bits(torch, got), bits(torch, want))

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


def both_ways(jsg, torch, name):
    """A case of tests/test_gpu_scratch_contents.py (its shapes, inputs, sentinel-filled outputs and reference) launched with the caller's
    own scratch on the current stream and without a scratch tensor on a side stream: the same bytes in every output, and the reference's."""
    import test_gpu_scratch_contents as sc
    work, _ = sc.built(jsg, torch, name)
    want, got = work.alloc(), work.alloc()
    args, kw = work.bind(want)
    work.launch(*args, d_scratch=torch.empty(work.need, dtype=torch.uint8, device="cuda"), **kw)
    st = side_stream(torch)
    args, kw = work.bind(got)
    work.launch(*args, stream=st.cuda_stream, **kw)
    torch.cuda.synchronize()
    work.check(tuple(t.cpu().numpy() for t in want))
    for g, w in zip(got, want):
        assert g.cpu().numpy().tobytes() == w.cpu().numpy().tobytes()


def test_hpss_launch(jsg, torch_cuda):
    both_ways(jsg, torch_cuda, "hpss-K65-complex-windows1x63")


def test_beat_launch(jsg, torch_cuda):
    both_ways(jsg, torch_cuda, "beat-period33-smooth1")


def test_dtw_launch(jsg, torch_cuda):
    both_ways(jsg, torch_cuda, "dtw-subseq")


def test_viterbi_launch(jsg, torch_cuda):
    both_ways(jsg, torch_cuda, "viterbi-band-65-states-half-30")


def test_pyin_decode_launch(jsg, torch_cuda):
    both_ways(jsg, torch_cuda, "pyin_decode-129-bins-half-50")


def test_knn_launch(jsg, torch_cuda):
    both_ways(jsg, torch_cuda, "knn-k65-split3-width2")


def test_rqa_launch(jsg, torch_cuda):
    both_ways(jsg, torch_cuda, "rqa-knight-moves")


def test_nmf_launch(jsg, torch_cuda):
    both_ways(jsg, torch_cuda, "nmf-257-frames-257-bins-5-components")


def test_pcen_launch(jsg, torch_cuda):
    both_ways(jsg, torch_cuda, "pcen-513-frames-state-in")


def test_peak_launch(jsg, torch_cuda):
    both_ways(jsg, torch_cuda, "peak-two-blocks-and-five-frames-long-wait-backtracking")

"""The time-lag conversion of libjsgx.so on the GPU (include/jsgx.h section 11) against tests/path_enhance_ref.py: a pure permutation, so
the bits of planes of distinct values are equal; sizes around the 64 x 64 tile, both pad values, both axes, both directions; three pairs
in pitched buffers whose guards stay; the round trip; graph capture."""
import numpy as np
import pytest

import path_enhance_ref as pr

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25e11)
SIZES = [1, 2, 63, 64, 65, 130]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def guarded(torch, planes, rows, cols, pad, sentinel, offset):
    pitch, size = cols + pad, rows * (cols + pad) + 3 * pad
    flat = torch.full((planes * size + offset + 5,), sentinel, dtype=torch.float32, device="cuda")
    return flat, torch.as_strided(flat, (planes, rows, cols), (size, pitch, 1), storage_offset=offset)


def untouched(flat, view, sentinel, offset):
    got = flat.cpu().numpy()
    inside = np.zeros(got.size, bool)
    P, R, W = view.shape
    inside[(offset + np.arange(P)[:, None, None] * view.stride(0) + np.arange(R)[None, :, None] * view.stride(1) + np.arange(W)[None, None, :]).ravel()] = True
    return bool((got[~inside] == sentinel).all() if sentinel == sentinel else np.isnan(got[~inside]).all())


def run(jsg, torch, planes, out_shape, *, pad, axis, inverse, guard=0):
    P = len(planes)
    fi, d_in = guarded(torch, P, *planes[0].shape, guard, float("nan"), 3)
    d_in.copy_(torch.from_numpy(np.stack(planes)))
    fo, d_out = guarded(torch, P, *out_shape, 2 * guard, float(SENTINEL), 1)
    jsg.lag_launch(d_in, d_out, pad=pad, axis=axis, inverse=inverse)
    torch.cuda.synchronize()
    assert untouched(fo, d_out, SENTINEL, 1), "a guard element was written"
    assert untouched(fi, d_in, float("nan"), 3) and pr.same_bits(d_in.cpu().numpy(), np.stack(planes)), "the input was written"
    return d_out.cpu().numpy()


@pytest.mark.parametrize("N", SIZES)
def test_both_directions_pads_and_axes(jsg, torch_cuda, N):
    R = pr.distinct_plane(N, N, N)
    for pad in (False, True):
        for axis in (1, 0):
            want = pr.to_lag(R, pad, axis)
            got = run(jsg, torch_cuda, [R], want.shape, pad=pad, axis=axis, inverse=False)[0]
            assert pr.same_bits(got, want), (N, pad, axis, "to lag", np.argwhere(got != want)[:4])
            assert not np.signbit(got[got == 0]).any()
            # from lag, on a lag plane whose padding holds values too: every element of the input counts
            lag = pr.distinct_plane(*want.shape, N + 1)
            back = run(jsg, torch_cuda, [lag], (N, N), pad=pad, axis=axis, inverse=True)[0]
            assert pr.same_bits(back, pr.from_lag(lag, axis)), (N, pad, axis, "from lag")
            # the round trip, in bits
            assert pr.same_bits(run(jsg, torch_cuda, [got], (N, N), pad=pad, axis=axis, inverse=True)[0], R), (N, pad, axis, "round trip")


@pytest.mark.parametrize("axis", [1, 0])
def test_three_pairs_in_padded_buffers(jsg, torch_cuda, axis):
    N = 67
    planes = [pr.distinct_plane(N, N, seed) for seed in (1, 2, 3)]
    planes[1][5, 7], planes[1][66, 0], planes[2][0, 66] = np.nan, -0.0, np.inf
    for pad in (False, True):
        wants = [pr.to_lag(R, pad, axis) for R in planes]
        got = run(jsg, torch_cuda, planes, wants[0].shape, pad=pad, axis=axis, inverse=False, guard=7)
        back = run(jsg, torch_cuda, wants, (N, N), pad=pad, axis=axis, inverse=True, guard=5)
        for p in range(3):
            assert pr.same_bits(got[p], wants[p]) and pr.same_bits(back[p], planes[p]), (p, pad, axis)


def test_the_python_layer_and_graph_capture(jsg, torch_cuda):
    torch = torch_cuda
    N = 70
    R = pr.distinct_plane(N, N, 9)
    d_R = torch.from_numpy(R).cuda()
    for axis, ax in ((-1, 1), (1, 1), (0, 0), (-2, 0)):
        for pad in (True, False):
            lag = jsg.recurrence_to_lag(d_R, pad=pad, axis=axis)
            assert pr.same_bits(lag.cpu().numpy(), pr.to_lag(R, pad, ax))
            assert pr.same_bits(jsg.lag_to_recurrence(lag, axis=axis).cpu().numpy(), R)
    batch = torch.stack([d_R, d_R.T.contiguous()])
    lag = jsg.recurrence_to_lag(batch)
    assert tuple(lag.shape) == (2, 2 * N, N) and pr.same_bits(lag[1].cpu().numpy(), pr.to_lag(R.T, True, 1))
    assert pr.same_bits(jsg.lag_to_recurrence(lag).cpu().numpy(), batch.cpu().numpy())
    with pytest.raises(jsg.JsgError, match="axis must be"):
        jsg.recurrence_to_lag(d_R, axis=2)
    with pytest.raises(jsg.JsgError, match="out overlaps in"):
        jsg.lag_launch(d_R, d_R, pad=False)
    # a captured first launch of each kernel form, replayed once
    d_in = torch.zeros((2, N, N), dtype=torch.float32, device="cuda")
    d_lag1 = torch.full((2, 2 * N, N), float(SENTINEL), dtype=torch.float32, device="cuda")
    d_lag0 = torch.full((2, N, 2 * N), float(SENTINEL), dtype=torch.float32, device="cuda")
    d_back1, d_back0 = (torch.full((2, N, N), float(SENTINEL), dtype=torch.float32, device="cuda") for _ in range(2))
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            s = side.cuda_stream
            jsg.lag_launch(d_in, d_lag1, axis=1, stream=s)
            jsg.lag_launch(d_lag1, d_back1, axis=1, inverse=True, stream=s)
            jsg.lag_launch(d_in, d_lag0, axis=0, stream=s)
            jsg.lag_launch(d_lag0, d_back0, axis=0, inverse=True, stream=s)
    torch.cuda.synchronize()
    assert (d_back1.cpu().numpy() == SENTINEL).all() and (d_lag0.cpu().numpy() == SENTINEL).all()          # captured, not run
    planes = [pr.distinct_plane(N, N, seed) for seed in (21, 22)]
    d_in.copy_(torch.from_numpy(np.stack(planes)))
    g.replay()
    torch.cuda.synchronize()
    for p, Rp in enumerate(planes):
        assert pr.same_bits(d_lag1[p].cpu().numpy(), pr.to_lag(Rp, True, 1)) and pr.same_bits(d_lag0[p].cpu().numpy(), pr.to_lag(Rp, True, 0))
        assert pr.same_bits(d_back1[p].cpu().numpy(), Rp) and pr.same_bits(d_back0[p].cpu().numpy(), Rp)

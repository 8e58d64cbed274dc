"""Strided launches of the 1024-point "runs" kernel as two populations of workgroups (csrc/jsg_runs_grid.h, DESIGN.md section 6 "Two
populations"): from a threshold of workgroup steps on, a launch whose grid is the library's choice (blocks_per_cu = 0) runs one resident
generation of long-lived workgroups and short-lived ones behind them.  Only WHICH workgroup transforms a super-group changes, so not a bit
may: every case runs the smallest launches that take the form -- the threshold itself and one step on either side of it -- with
blocks_per_cu = 0 into a sentinel-filled buffer and compares the WHOLE buffer, padding included, with the same call on the uniform grid
(blocks_per_cu = 32), and its first, middle and last batch with single launches."""
import os
import re

import pytest

pytestmark = pytest.mark.gpu

N, HOP, H = 1024, 512, 513
SENTINEL = -7.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def plan(jsg, oracle):
    return jsg.Plan(N, oracle.window(oracle.WIN_HANN, N))


@pytest.fixture(scope="module")
def threshold(torch_cuda):
    """workgroup steps (super-groups of 8 columns) from which a launch takes the two-population form on this device: runs_two_pop_threshold"""
    src = open(os.path.join(ROOT, "jadespectrogram_amd", "csrc", "jsg_runs_grid.h")).read()
    gen = int(re.search(r"constexpr int kRunsPopMinGenerations = (\d+);", src).group(1))
    per_cu = int(re.search(r"constexpr int kRunsResidentPerCu = (\d+);", src).group(1))
    n_cu = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    t = ((per_cu * n_cu) & ~255) * gen
    assert t > 0, f"{n_cu} CUs: no launch takes the two-population form"
    return t


def _rows_for(steps, F, C=1):
    """batches so that batches * C rows of ceil(F / 8) super-groups are at least `steps` steps"""
    per_batch = C * ((F + 7) // 8)
    return (steps + per_batch - 1) // per_batch


def _buffers(torch, K, rows, W, pitch, tail):
    shape = (K, rows, W, pitch) if rows > 1 else (K, W, pitch)
    return torch.full(shape, SENTINEL, device="cuda"), (torch.full((K, rows, W), SENTINEL, device="cuda") if tail else None)


def _case(jsg, torch, plan, *, F, K, C=1, W=None, pos=0, linear=False, exact=False, tail=False, seed=1):
    cap = jsg.capi
    per_ch = C > 1
    W = W or F
    pitch = 512 if tail else 544
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    d_in = torch.empty((K, C, (F - 1) * HOP + N), device="cuda").uniform_(-1.0, 1.0, generator=g)
    kw = dict(feedblocks=2, mix_mode=cap.MIX_PER_CHANNEL if per_ch else cap.MIX_ABSMEAN, ring_pos=pos, linear_out=linear, exact_log=exact, plan_select=1)
    got, t_got = _buffers(torch, K, C, W, pitch, tail)
    uni, t_uni = _buffers(torch, K, C, W, pitch, tail)
    assert jsg.stft_db_strided_kernel_name(plan, d_in, HOP, F, got, d_tail=t_got, **kw) == "Cfg1024"
    jsg.stft_db_strided(plan, d_in, HOP, F, got, d_tail=t_got, blocks_per_cu=0, **kw)
    jsg.stft_db_strided(plan, d_in, HOP, F, uni, d_tail=t_uni, blocks_per_cu=32, **kw)
    torch.cuda.synchronize()
    cols = sorted({(pos + i) % W for i in range(F)})
    assert bool((uni[..., cols, :H - (1 if tail else 0)] != SENTINEL).all()), "the uniform grid did not write its columns"
    assert torch.equal(got, uni), "blocks_per_cu = 0 and = 32 differ (columns, padding or unused ring columns)"
    if tail:
        assert torch.equal(t_got, t_uni), "tail planes differ"
    for b in sorted({0, K // 2, K - 1}):
        one, t_one = _buffers(torch, 1, C, W, pitch, tail)
        if per_ch:
            jsg.stft_db_strided(plan, d_in[b:b + 1], HOP, F, one, d_tail=t_one, blocks_per_cu=32, **kw)   # (one batch: far below the threshold)
        else:
            jsg.stft_db(plan, d_in[b], HOP, F, one[0], d_tail=(t_one[0] if tail else None), **kw)
        torch.cuda.synchronize()
        assert torch.equal(got[b], one[0]), f"batch {b} differs from its single launch"
        if tail:
            assert torch.equal(t_got[b], t_one[0]), f"tail plane of batch {b} differs from its single launch"
    return d_in, got, t_got


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_threshold_and_one_step_on_either_side(jsg, torch_cuda, plan, threshold, delta):
    """rows of 7 frames: one super-group each (not a multiple of 8 columns, the row ends inside the run of columns 6, 7)"""
    _case(jsg, torch_cuda, plan, F=7, K=threshold + delta, W=8, pos=3, seed=30 + delta)


@pytest.mark.parametrize("tail", [False, True])
def test_rows_of_several_super_groups_with_a_ring_wrap(jsg, torch_cuda, plan, threshold, tail):
    """61 frames = 8 super-groups per row, the last one ends inside a run; column 26 sits at W - 1: the ring wraps between the columns of a run"""
    _case(jsg, torch_cuda, plan, F=61, K=_rows_for(threshold + 3, 61), W=64, pos=37, tail=tail, seed=33)


@pytest.mark.parametrize("tail", [False, True])
def test_per_channel_rows(jsg, torch_cuda, plan, threshold, tail):
    """8 channels, one row per (batch, channel), 3 super-groups per row"""
    _case(jsg, torch_cuda, plan, F=21, K=_rows_for(threshold + 1, 21, C=8), C=8, W=24, pos=19, tail=tail, seed=34)


@pytest.mark.parametrize("kw", [dict(exact=True), dict(exact=True, tail=True), dict(linear=True), dict(linear=True, tail=True)],
                         ids=lambda k: "-".join(k))
def test_exact_logarithm_and_linear_output(jsg, torch_cuda, plan, threshold, kw):
    _case(jsg, torch_cuda, plan, F=19, K=_rows_for(threshold + 2, 19), W=20, pos=13, seed=35, **kw)


def test_capture_into_a_graph_replayed_twice(jsg, torch_cuda, plan, threshold):
    torch = torch_cuda
    F, W, pos = 13, 16, 9
    K = _rows_for(threshold + 1, F)
    d_in, eager, t_eager = _case(jsg, torch, plan, F=F, K=K, W=W, pos=pos, tail=True, seed=36)
    kw = dict(feedblocks=2, ring_pos=pos, plan_select=1)
    st = torch.cuda.Stream()
    cap, t_cap = _buffers(torch, K, 1, W, 512, True)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        jsg.stft_db_strided(plan, d_in, HOP, F, cap, d_tail=t_cap, stream=st.cuda_stream, **kw)   # (warm-up: nothing is set up inside the capture)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=st):
            jsg.stft_db_strided(plan, d_in, HOP, F, cap, d_tail=t_cap, stream=st.cuda_stream, **kw)
        for _ in range(2):
            cap.fill_(SENTINEL); t_cap.fill_(SENTINEL)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(cap, eager) and torch.equal(t_cap, t_eager)

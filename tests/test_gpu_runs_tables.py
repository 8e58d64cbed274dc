"""The table and load side of the 1024-point "runs" kernel (stft_db_kernel STREAM == 2; DESIGN.md section 6, "Runs tables"): window values of
the lower frame half held in registers for a wave's life, the stage-1 and post-pass tables read straight from global memory with a smaller LDS
table block behind them, the read-once hop loaded with a cache hint.  None of that may change a bit or a byte.  Every case sends a strided
call through the launcher's AUTOMATIC rule (1024 points, hop 512, one channel per column: the runs form from two batches on) into a buffer
pre-filled with a sentinel and compares the WHOLE buffer, padding included, with single launches of the same batches -- which take the plain
one-batch kernel, whose tables all come from LDS.  The shapes are the smallest at which a run can go wrong: a row shorter than a run, rows that
end inside a run, one super-group of eight columns plus one column, several super-groups.  One case runs with a window of distinct values per
sample (a ramp): a window pair taken from the wrong register then moves whole bins, not only roundings."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, HOP, H = 1024, 512, 513
SENTINEL = -7.0


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
def ramp_plan(jsg):
    """w[i] = (i + 1) / 1024: 1024 distinct values, no symmetry between the frame halves or inside a pair"""
    return jsg.Plan(N, (np.arange(1, N + 1, dtype=np.float64) / N).astype(np.float32))


def _input(torch, K, C, n_samples, seed, lead):
    """[K][C][n_samples] float32, a view that starts `lead` floats into its (256-byte aligned) allocation; n_samples is a multiple of 512, so
    every row starts 4 * lead bytes off a 16-byte boundary"""
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    flat = torch.empty(K * C * n_samples + lead + 64, device="cuda").uniform_(-1.0, 1.0, generator=g)
    assert flat.data_ptr() % 16 == 0
    return flat[lead:lead + K * C * n_samples].view(K, C, n_samples)


def _outputs(torch, K, rows, W, pitch, per_ch):
    per_batch = rows * W * pitch
    flat = torch.full((K * per_batch,), SENTINEL, device="cuda")
    view = flat.view(K, rows, W, pitch) if per_ch else flat.view(K, W, pitch)
    return flat, view


def _case(jsg, torch, plan, *, F, K, C=1, mix="absmean", W=None, pos=0, lead=0, linear=False, exact=False, tail=False, seed=1):
    cap = jsg.capi
    m = {"absmean": cap.MIX_ABSMEAN, "per_channel": cap.MIX_PER_CHANNEL}[mix]
    per_ch = mix == "per_channel"
    rows = C if per_ch else 1
    W = W or F
    pitch = 544                                  # 513 floats of a column (512 with the tail plane) + padding
    used = H - 1 if tail else H
    d_in = _input(torch, K, C, (F - 1) * HOP + N, seed, lead)
    assert d_in.data_ptr() % 16 == (4 * lead) % 16
    g_flat, got = _outputs(torch, K, rows, W, pitch, per_ch)
    r_flat, ref = _outputs(torch, K, rows, W, pitch, per_ch)
    t_got = torch.full((K, rows, W), SENTINEL, device="cuda") if tail else None
    t_ref = torch.full((K, rows, W), SENTINEL, device="cuda") if tail else None
    kw = dict(feedblocks=2, mix_mode=m, ring_pos=pos, linear_out=linear, exact_log=exact)
    # the automatic rule: no plan_select.  (One channel per column never takes the two-stage plan; the runs form reports the plan's name.)
    assert jsg.stft_db_strided_kernel_name(plan, d_in, HOP, F, got, d_tail=t_got, **kw) == "Cfg1024"
    jsg.stft_db_strided(plan, d_in, HOP, F, got, d_tail=t_got, **kw)
    for b in range(K):
        jsg.stft_db(plan, d_in[b], HOP, F, ref[b], d_tail=(t_ref[b] if tail else None), plan_select=1, **kw)
    torch.cuda.synchronize()
    cols = sorted({(pos + i) % W for i in range(F)})
    assert bool((ref[..., cols, :used] != SENTINEL).all()), "the single launches did not write their columns"
    assert bool((got[..., used:] == SENTINEL).all()), "padding behind bin n/2 was written"
    assert torch.equal(g_flat, r_flat), "columns differ from single launches, or padding / unused ring columns were written"
    if tail:
        assert torch.equal(t_got, t_ref), "tail plane differs from single launches"


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("F", [1, 2, 3, 7, 8, 9, 33])
def test_row_lengths_and_batch_counts(jsg, torch_cuda, plan, F, K):
    """1: a row shorter than a run; 2: exactly a run; 3, 7, 9: rows ending inside a run; 8: one super-group; 9, 33: whole super-groups plus one
    column.  One batch is a single launch by the library's rule, three take the runs form."""
    _case(jsg, torch_cuda, plan, F=F, K=K, W=F + 2, pos=1, seed=100 + 10 * F + K)


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("kw", [
    dict(W=10, pos=3),                       # the ring wraps inside a run: column 6 sits at W - 1, column 7 at 0
    dict(tail=True),
    dict(tail=True, W=10, pos=3),
    dict(C=3, mix="per_channel"),
    dict(C=3, mix="per_channel", tail=True),
    dict(exact=True),
    dict(linear=True),
    dict(lead=1),                            # the input rows start 4 bytes off a 16-byte boundary
    dict(lead=1, tail=True, exact=True, W=10, pos=3),
], ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_variants(jsg, torch_cuda, plan, kw, K):
    _case(jsg, torch_cuda, plan, F=9, K=K, seed=7, **kw)


@pytest.mark.parametrize("kw", [dict(), dict(tail=True), dict(C=3, mix="per_channel", linear=True)],
                         ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()) or "plain")
def test_window_of_distinct_values(jsg, torch_cuda, ramp_plan, kw):
    _case(jsg, torch_cuda, ramp_plan, F=33, K=3, W=35, pos=30, seed=9, **kw)
    _case(jsg, torch_cuda, ramp_plan, F=7, K=3, seed=10, **kw)

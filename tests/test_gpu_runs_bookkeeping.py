"""The store side of the 1024-point "runs" kernel (stft_db_kernel STREAM == 2): since the bookkeeping trim ("Runs
bookkeeping") the later columns of a run take their ring column, their column address and their tail-plane row from the run's first column by
increment (one add, one wrap compare), every column store is scalar base + a per-wave lane offset + an immediate, lane 0's exceptions are
selected instead of branched, and bin n/2 is computed on lane 0 alone.  None of that may change a bit or a byte: every case runs a strided
dispatch (one channel per column, exactly 50 % overlap -- the launches the runs form serves) into a buffer pre-filled with a sentinel and
compares the WHOLE buffer, padding included, with single launches of the same batches, which take the plain one-batch kernel.  The cases sit
where the increment and the flags can go wrong: run-length edges, a ring wrap between the two columns of a run / at a run boundary / at the
first column, every address term, both layouts and output modes, per-channel rows, surplus steps, graph replay."""
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


def _input(torch, K, C, n_samples, seed, lead):
    """[K][C][n_samples] float32, a view that starts `lead` floats into its allocation"""
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    flat = torch.empty(K * C * n_samples + lead + 64, device="cuda").uniform_(-1.0, 1.0, generator=g)
    return flat[lead:lead + K * C * n_samples].view(K, C, n_samples)


def _outputs(torch, K, rows, W, pitch, batch_pad, per_ch):
    """a sentinel-filled backing buffer and its [K][W][pitch] (per-channel: [K][rows][W][pitch]) view; batches `batch_pad` floats apart on top"""
    per_batch = rows * W * pitch + batch_pad
    flat = torch.full((K * per_batch,), SENTINEL, device="cuda")
    if per_ch:
        view = flat.as_strided((K, rows, W, pitch), (per_batch, W * pitch, pitch, 1))
    else:
        view = flat.as_strided((K, W, pitch), (per_batch, pitch, 1))
    return flat, view


def _case(jsg, torch, plan, *, F, K, C=1, mix="absmean", W=None, pos=0, first=0, lead=0, bpc=0, linear=False, exact=False, tail=False,
          pitch=None, batch_pad=0, seed=1, stream=None):
    cap = jsg.capi
    m = {"absmean": cap.MIX_ABSMEAN, "left": cap.MIX_LEFT, "right": cap.MIX_RIGHT, "per_channel": cap.MIX_PER_CHANNEL}[mix]
    per_ch = mix == "per_channel"
    rows = C if per_ch else 1
    W = W or F
    pitch = pitch or (512 if tail else 544)
    d_in = _input(torch, K, C, (first + F - 1) * HOP + N, seed, lead)
    g_flat, got = _outputs(torch, K, rows, W, pitch, batch_pad, per_ch)
    r_flat, ref = _outputs(torch, K, rows, W, pitch, batch_pad, per_ch)
    t_got = torch.full((K, rows, W), SENTINEL, device="cuda") if tail else None
    t_ref = torch.full((K, rows, W), SENTINEL, device="cuda") if tail else None
    kw = dict(feedblocks=2, mix_mode=m, ring_pos=pos, first_frame=first, linear_out=linear, exact_log=exact)
    assert jsg.stft_db_strided_kernel_name(plan, d_in, HOP, F, got, d_tail=t_got, plan_select=1, **kw) == "Cfg1024"
    skw = {} if stream is None else dict(stream=stream)
    jsg.stft_db_strided(plan, d_in, HOP, F, got, d_tail=t_got, plan_select=1, blocks_per_cu=bpc, **skw, **kw)
    for b in range(K):
        jsg.stft_db(plan, d_in[b], HOP, F, ref[b], d_tail=(t_ref[b] if tail else None), plan_select=1, **skw, **kw)
    torch.cuda.synchronize()
    cols = sorted({(pos + i) % W for i in range(F)})
    assert bool((ref[..., cols, :H - (1 if tail else 0)] != SENTINEL).all()), "the single launches did not write their columns"
    assert torch.equal(g_flat, r_flat), "columns differ from single launches, or padding / unused ring columns were written"
    if tail:
        assert torch.equal(t_got, t_ref), "tail plane differs from single launches"
    return g_flat, t_got


@pytest.mark.parametrize("F", [1, 2, 3, 9])
def test_rows_shorter_than_a_run_exactly_a_run_and_ending_inside_one(jsg, torch_cuda, plan, F):
    _case(jsg, torch_cuda, plan, F=F, K=3, W=F + 2, pos=1, seed=10 + F)
    _case(jsg, torch_cuda, plan, F=F, K=3, W=F, pos=0, tail=True, seed=20 + F)


@pytest.mark.parametrize("W,pos,F,what", [
    (12, 5, 10, "between the two columns of a run: column 6 sits at W - 1, column 7 at 0"),
    (12, 4, 10, "at a run boundary: column 7 sits at W - 1, column 8 at 0"),
    (10, 9, 10, "behind the first column: column 0 sits at W - 1"),
    (10, 0, 10, "none: the row fills the ring exactly"),
    (9, 8, 9, "behind the first column, the row ends inside a run"),
    (64, 37, 61, "between the columns of a run of a later wave (column 26 at W - 1), several super-groups per row"),
])
@pytest.mark.parametrize("tail", [False, True])
def test_ring_wrap_positions(jsg, torch_cuda, plan, W, pos, F, what, tail):
    """A run's first column is even; the later one is derived from it.  With the tail plane its address wraps with the column."""
    _case(jsg, torch_cuda, plan, F=F, K=4, W=W, pos=pos, tail=tail, seed=W + pos)


@pytest.mark.parametrize("kw", [
    dict(first=5), dict(lead=1), dict(lead=3), dict(pitch=576), dict(batch_pad=40), dict(first=3, lead=1, pitch=640, batch_pad=8, tail=True),
], ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_address_terms(jsg, torch_cuda, plan, kw):
    """first_frame, an input base that is 4-byte aligned only, a column pitch above the minimum, batches that are not a whole number of
    columns apart."""
    _case(jsg, torch_cuda, plan, F=21, K=3, W=24, pos=19, seed=5, **kw)


@pytest.mark.parametrize("kw", [
    dict(linear=True), dict(linear=True, tail=True), dict(exact=True), dict(exact=True, tail=True), dict(C=2, mix="left"),
    dict(C=2, mix="right", tail=True),
], ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_layouts_and_output_modes(jsg, torch_cuda, plan, kw):
    _case(jsg, torch_cuda, plan, F=19, K=3, W=20, pos=13, seed=6, **kw)


@pytest.mark.parametrize("tail", [False, True])
def test_per_channel_rows_end_inside_a_super_group(jsg, torch_cuda, plan, tail):
    """3 channels x 2 batches = 6 rows of 5 frames: every row is one super-group of 8 columns whose last three are not stored."""
    _case(jsg, torch_cuda, plan, F=5, K=2, C=3, mix="per_channel", W=6, pos=4, tail=tail, seed=7)


def test_surplus_steps_are_stored_twice_with_the_same_bits(jsg, torch_cuda, plan):
    """blocks_per_cu = 1: 37 rows x 8 super-groups = 296 steps on a grid of one workgroup per CU -- the second round's surplus workgroups
    start over with the first groups.  And a launch with fewer super-groups than workgroups."""
    _case(jsg, torch_cuda, plan, F=60, K=37, W=64, pos=50, bpc=1, tail=True, seed=8)
    _case(jsg, torch_cuda, plan, F=60, K=37, W=60, pos=0, bpc=1, seed=9)
    _case(jsg, torch_cuda, plan, F=9, K=3, W=9, pos=2, bpc=1, seed=11)


def test_one_capture_and_replay_on_one_stream(jsg, torch_cuda, plan):
    torch = torch_cuda
    F, K, W, pos = 27, 4, 32, 29
    d_in = _input(torch, K, 1, (F - 1) * HOP + N, 12, 0)
    eager = torch.full((K, W, 512), SENTINEL, device="cuda")
    t_eager = torch.full((K, 1, W), SENTINEL, device="cuda")
    for b in range(K):
        jsg.stft_db(plan, d_in[b], HOP, F, eager[b], d_tail=t_eager[b], feedblocks=2, ring_pos=pos, plan_select=1)
    st = torch.cuda.Stream()
    cap = torch.full((K, W, 512), SENTINEL, device="cuda")
    t_cap = torch.full((K, 1, W), SENTINEL, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        jsg.stft_db_strided(plan, d_in, HOP, F, cap, d_tail=t_cap, feedblocks=2, ring_pos=pos, plan_select=1, stream=st.cuda_stream)   # (warm-up: nothing is set up inside the capture)
        torch.cuda.synchronize()
        cap.fill_(SENTINEL); t_cap.fill_(SENTINEL)
        with torch.cuda.graph(g, stream=st):
            jsg.stft_db_strided(plan, d_in, HOP, F, cap, d_tail=t_cap, feedblocks=2, ring_pos=pos, plan_select=1, stream=st.cuda_stream)
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap, eager) and torch.equal(t_cap, t_eager)

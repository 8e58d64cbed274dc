"""NaN containment of the stateless launches: one NaN sample in one batch, channel and position must turn exactly the columns whose frame
reads it into NaN (in every bin) and leave every other column bit for bit as on the clean input.  Plans that share state between frames
-- four frames per wavefront (Cfg1024B), two (Cfg2048), the "runs" kernel that keeps half a raw frame in registers, the pair plan that
packs two channels into one complex transform -- would show a leak here that no tolerance can blur.  Every plan, pinned by plan_select
and confirmed by the kernel-name query; single, strided and per-channel launches; dB under both logarithms and linear power."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# plan -> (n, plan_select)
PLANS = {"Cfg512": (512, 1), "Cfg1024": (1024, 1), "Cfg1024B": (1024, 2), "Cfg2048": (2048, 1), "Cfg2048B": (2048, 2),
         "Cfg2048P": (2048, 3), "Cfg4096": (4096, 1), "Cfg4096B": (4096, 2), "Cfg8192": (8192, 1)}
F = 24          # frames per batch (several wavefront groups of every plan)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def _nan_positions(n, hop, rng):
    """The first and the last sample frame 5 reads, a sample two frames share, and one at random."""
    j = 5
    return [j * hop, j * hop + n - 1, (j + 1) * hop + 3, int(rng.integers(0, (F - 1) * hop + n))]


def _expected(n, hop, pos):
    starts = np.arange(F) * hop
    return (starts <= pos) & (pos < starts + n)


@pytest.mark.parametrize("form", ["single", "strided", "per_channel", "runs"])
@pytest.mark.parametrize("plan_name", list(PLANS))
def test_one_nan_sample_reaches_exactly_its_frames(jsg, oracle, torch_cuda, plan_name, form):
    torch = torch_cuda
    n, sel = PLANS[plan_name]
    if form == "runs" and plan_name != "Cfg1024":
        pytest.skip("the runs geometry is a 1024-point strided launch of one channel")
    if form == "per_channel" and plan_name == "Cfg2048P":
        pytest.skip("the pair plan mixes a channel pair into one column (sum-type mixes only)")
    hop = n // 2
    K = 1 if form in ("single", "per_channel") else 3
    Cn = 1 if form == "runs" else 2
    mix = jsg.capi.MIX_PER_CHANNEL if form == "per_channel" else jsg.capi.MIX_ABSMEAN
    S = (F - 1) * hop + n
    H, pitch = n // 2 + 1, (n // 2 + 1 + 31) // 32 * 32
    rng = np.random.default_rng(sum(map(ord, plan_name + form)))
    clean = torch.from_numpy((0.5 * rng.standard_normal((K, Cn, S))).astype(np.float32)).cuda()
    plan = jsg.Plan(n, oracle.window(oracle.WIN_HANN, n))
    planes = Cn if form == "per_channel" else 1
    shape = (K, planes, F, pitch)

    def launch(x, linear, exact):
        out = torch.full(shape, -7.0, device="cuda")
        kw = dict(feedblocks=2, mix_mode=mix, linear_out=linear, exact_log=exact, plan_select=sel)
        if K == 1:
            o = out[0] if planes > 1 else out[0, 0]
            name = jsg.stft_kernel_name(plan, x[0], hop, F, o, **kw)
            jsg.stft_db(plan, x[0], hop, F, o, **kw)
        else:
            o = out if planes > 1 else out[:, 0]
            name = jsg.stft_db_strided_kernel_name(plan, x, hop, F, o, **kw)
            jsg.stft_db_strided(plan, x, hop, F, o, **kw)
        assert name == plan_name, (name, plan_name)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    cases = [(False, False), (False, True), (True, False)]        # dB hardware log, dB exact log, linear power
    ref = {c: launch(clean, *c) for c in cases}
    for pos in _nan_positions(n, hop, rng):
        b, c = int(rng.integers(0, K)), int(rng.integers(0, Cn))
        x = clean.clone()
        x[b, c, pos] = float("nan")
        want = np.zeros((K, planes, F), bool)
        want[b, c if planes > 1 else 0] = _expected(n, hop, pos)
        assert want.any()
        for case in cases:
            got = launch(x, *case)
            what = f"{plan_name} {form} NaN at batch {b} channel {c} sample {pos} linear={case[0]} exact={case[1]}"
            bad = ~np.isfinite(got[..., :H])
            cols = bad.any(axis=-1)
            assert (cols == want).all(), f"{what}: non-finite columns {np.argwhere(cols).tolist()} vs expected {np.argwhere(want).tolist()}"
            assert np.isnan(got[..., :H][want]).all(), f"{what}: a column whose frame reads the NaN is not NaN in every bin"
            keep = ~want
            assert (got[keep].view(np.uint32) == ref[case][keep].view(np.uint32)).all(), f"{what}: a column that does not read the NaN changed"
            assert (got[..., H:] == -7.0).all(), f"{what}: wrote outside the columns"

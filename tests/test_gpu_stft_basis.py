"""Every power-STFT plan per bin on impulses, impulse pairs, tones, a comb and noise (tests/stft_basis.py: classes, float64 reference,
metric, yardstick, bound; tests/test_stft_basis_ref.py holds the kernel mirror to the same bound without a GPU).

a. linear power of every pinned plan on every class and window: equal to the mirror (oracle/jsg_mirror.c) bit for bit, and
   e = max_k |P - P_ref| / max_k P_ref <= M * Y per frame against float64.  Impulse streams send exact zeros through every butterfly:
   a multiply-add contracted on one side only shows there.
b. exact_log dB columns equal the mirror's bit for bit on rect tones (most bins at or near zero power) and Hann impulses, whose
   zero-reference frame reads the shared routine's floor, -110 dB, in every bin.
c. the runs form (stft_db_strided, 1024 points, one channel, hop 512): six batches of the comb at six lead-ins, rows of 130 columns and
   of 129, where a row ends inside a run.
d. a pitched buffer with an odd ring position: padding and unwritten ring columns keep their sentinel, the written ones are those of (a).

Measured on an MI355X (profiles/stft_power_accuracy.md): every call equals the mirror, the worst e / Y is 1.98 (Cfg2048, pairs, Hann,
d = n - 1) against M = 2.5.  The file takes 22 s there, where tests/test_gpu_mirror.py takes 4.8 s and tests/test_gpu_round6.py 2.9 s;
most of it is the mirror and the float64 reference on the host (the slowest case, the impulses of Cfg8192, takes 3.3 s).
"""
import numpy as np
import pytest

import stft_basis as B

pytestmark = pytest.mark.gpu

SENT = -7.0
DB_FLOOR = np.float32(10.0 * np.log10(np.float64(np.float32(1e-11))))      # 10 log10(0 + 1e-11f): -110 dB


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def mirror():
    from oracle import mirror as m
    return m.load()


def assert_same_bits(got, ref, what):
    bad = got.view(np.uint32) != ref.view(np.uint32)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} values differ from the mirror; first at (frame, bin) "
                           f"{tuple(int(v) for v in np.argwhere(bad)[0])}: {got[bad][0]!r} vs {ref[bad][0]!r}")


# ------------------------------------------------------------------------------------------------ a. linear power
@pytest.mark.parametrize("cls", B.CLASSES)
@pytest.mark.parametrize("n,sel,kernel", B.PINS)
def test_linear_power_equals_the_mirror_and_holds_the_bound(jsg, mirror, torch_cuda, n, sel, kernel, cls):
    for wname in B.CLASS_WINDOWS[cls]:
        zero_frames = 0
        for call in B.calls(cls, n, wname, pair=B.plan_is_pair(kernel)):
            P = B.gpu_columns(jsg, torch_cuda, call, sel, kernel)
            assert_same_bits(P, B.mirror_columns(mirror, kernel, call), f"{kernel} | {call.name}")
            zero_frames += B.assert_power_basis(P, call, kernel).zero_frames
        hann_zero = cls == "impulses" and wname == "hann"      # w[0] = 0 under the lone impulse, once per position sweep
        # (hop 1: every lead-in reaches position 0; the pair plan's second channel, reversed in time, is there too at lead-in 0 only)
        assert zero_frames == ((4 if n <= 2048 and not B.plan_is_pair(kernel) else 1) if hann_zero else 0)


# ------------------------------------------------------------------------------------------------ b. exact dB
@pytest.mark.parametrize("n,sel,kernel", B.PINS)
def test_exact_db_equals_the_mirror_on_tones_and_hann_impulses(jsg, mirror, torch_cuda, n, sel, kernel):
    pair = B.plan_is_pair(kernel)
    floored = 0
    for call in B.calls("tones", n, "rect", pair=pair) + B.calls("impulses", n, "hann", pair=pair):
        db = B.gpu_columns(jsg, torch_cuda, call, sel, kernel, linear_out=False, exact_log=True)
        assert_same_bits(db, B.mirror_columns(mirror, kernel, call, exact_db=True), f"{kernel} exact dB | {call.name}")
        if B.power_f64(call, call.F - 1, call.F).max() == 0:      # the last frame of an impulses call: the impulse on w[0] = 0
            assert (db[-1].view(np.uint32) == DB_FLOOR.view(np.uint32)).all(), f"{kernel} | {call.name}: a zero-reference frame must read -110 dB"
            floored += 1
    assert floored == (4 if n <= 2048 and not pair else 1) and DB_FLOOR == np.float32(-110.0)


# ------------------------------------------------------------------------------------------------ c. the runs form
@pytest.mark.parametrize("F", [130, 129])
def test_runs_form_on_the_comb(jsg, mirror, torch_cuda, F):
    torch = torch_cuda
    n, hop, W, pitch = 1024, 512, 130, 544
    leads = (0, 1, 63, 288, 511, 576)
    for wname in B.CLASS_WINDOWS["comb"]:
        w = B.window(wname, n)
        batches = [B.comb_call(n, w, lead, F, tag=f"comb {wname} n={n}") for lead in leads]
        plan = jsg.Plan(n, w)
        d_in = torch.from_numpy(np.stack([c.x for c in batches])).cuda()
        d_out = torch.full((len(leads), W, pitch), SENT, device="cuda")
        kw = dict(feedblocks=2, mix_mode=B.MIX_ABSMEAN, plan_select=1)
        assert d_in.shape == (6, 1, (F - 1) * hop + n) and 2 * hop == n       # with one channel per column: what the runs form needs
        assert jsg.stft_db_strided_kernel_name(plan, d_in, hop, F, d_out, **kw) == "Cfg1024"
        jsg.stft_db_strided(plan, d_in, hop, F, d_out, linear_out=True, **kw)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert (got[:, F:] == SENT).all() and (got[:, :, n // 2 + 1:] == SENT).all()
        for b, call in enumerate(batches):
            P = np.ascontiguousarray(got[b, :F, :n // 2 + 1])
            assert_same_bits(P, B.mirror_columns(mirror, "Cfg1024", call), f"runs, batch {b} | {call.name}")
            assert B.assert_power_basis(P, call, f"runs, batch {b}").zero_frames == 0


# ------------------------------------------------------------------------------------------------ d. pitch, ring, padding
@pytest.mark.parametrize("n,sel,kernel", B.PINS)
def test_pitched_buffer_with_an_odd_ring_position(jsg, torch_cuda, n, sel, kernel):
    torch = torch_cuda
    call = B.calls("impulses", n, "ramp", pair=B.plan_is_pair(kernel))[0]
    H, F = n // 2 + 1, call.F
    want = B.gpu_columns(jsg, torch, call, sel, kernel)
    pitch = (H + 31) // 32 * 32 + 32
    W = F + 7
    pos = W - 4 if (W - 4) % 2 else W - 3       # odd, and the columns wrap round the end of the ring
    assert pos % 2 == 1 and pos + F > W
    flat = torch.full((W * pitch + 9,), SENT, device="cuda")
    ring = flat[:W * pitch].view(W, pitch)
    plan = jsg.Plan(n, call.w)
    d_x = torch.from_numpy(call.x).cuda()
    kw = dict(feedblocks=call.fb, mix_mode=B.MIX_ABSMEAN, plan_select=sel, ring_pos=pos)
    assert jsg.stft_kernel_name(plan, d_x, call.hop, F, ring, **kw) == kernel
    jsg.stft_db(plan, d_x, call.hop, F, ring, linear_out=True, **kw)
    torch.cuda.synchronize()
    got = ring.cpu().numpy()
    cols = (pos + np.arange(F)) % W
    assert (got[cols, :H].view(np.uint32) == want.view(np.uint32)).all(), f"{kernel}: pitched ring columns differ from the contiguous launch"
    untouched = np.setdiff1d(np.arange(W), cols)
    assert untouched.size == 7 and (got[untouched] == SENT).all(), f"{kernel}: a ring column outside the launch was written"
    assert (got[:, H:] == SENT).all(), f"{kernel}: the padding behind bin n/2 was written"
    assert bool((flat[W * pitch:] == SENT).all())

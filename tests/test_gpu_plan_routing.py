"""Plan routing where the launcher's automatic rule flips.  1024, 2048 and 4096 points have two kernels each, which round differently in
the last bits; the launcher picks one per launch (csrc/jsg_kernels.hip: resolve_variant) from the channels per column, the
mix, the frame count and the CU count of the device.  Several entry points promise bit-identity relative to a PINNED plan (include/jsg.h:
strided dB launches, the fused display path, jsg_stft_db_strided_kernel_name); these tests check those promises on both sides of the rule,
and check the kernels the benchmark times against a float64 DFT directly.

Every size that depends on the rule is derived from the CU count of the device with the launcher's own fill rule (_b_rule), and every
test that claims a given plan ran also shows that the two plans give different bits on the same input."""
import os
import sys

import numpy as np
import pytest

from parity_util import FLOOR_BY_N, REL, STRONG_REL, assert_db_close, floor_for
from test_gpu_fullsize import _b_rule, _stream
from test_gpu_strided import _batches, _run_case

pytestmark = pytest.mark.gpu

# columns per workgroup step (Cfg::TPB in csrc/jsg_stft_kernel.h)
TPB = {"Cfg1024": 4, "Cfg1024B": 32, "Cfg2048": 4, "Cfg2048B": 16, "Cfg4096": 2, "Cfg4096B": 8}
STEP_LIMIT = 1 << 20           # workgroup steps of one strided launch (jsg_stft_db_launch_strided cuts longer jobs)
HOP = 512
SENT = -7.0                    # what the output buffers hold before a launch: a value no column of these inputs takes


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(autouse=True)
def _memory_report(torch_cuda):
    """Peak allocation of every test (the split-job tests allocate up to ~17 GB); printed with -s."""
    torch = torch_cuda
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    print(f"  [peak allocation {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB]")
    torch.cuda.empty_cache()


def _n_cu(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _f_hi(tpb, n_cu):
    """The smallest frame count whose launch fills its (first) round of "B" workgroups."""
    w = 1
    while not _b_rule(w * tpb, tpb, n_cu):
        w += 1
    f = (w - 1) * tpb + 1
    assert _b_rule(f, tpb, n_cu) and not _b_rule(f - 1, tpb, n_cu)
    return f


def _power_f64(torch, x, n, hop, F, win32, mix_sum=False):
    """Float64 DFT (torch.fft.rfft: a checker only, never on the product path) of the float32 windowed frames j * hop of x [C][samples],
    the per-channel powers rounded to float32 and summed in channel order in float32 like the reference (Spectrogram.cpp:68-76);
    AbsMean divides the sum by the channel count in float32.  Returns float32 [F][n/2+1]."""
    acc = None
    for ch in range(x.shape[0]):
        fr = (x[ch].unfold(0, n, hop)[:F] * win32).to(torch.float64)      # float32 product, then exact in float64
        X = torch.fft.rfft(fr, dim=-1)
        p = (X.real * X.real + X.imag * X.imag).to(torch.float32)
        acc = p if acc is None else acc + p
        del fr, X
    return acc if mix_sum else acc / np.float32(x.shape[0])


def _check_power(torch, got, ref, C, what):
    """Every bin of every column against the float64 reference, with the bound of test_full_launch_every_bin_against_float64_fft
    (tests/parity_util.py, plus the C + 1 float32 roundings of the reference's own mix).  Returns the worst error relative to the
    frame peak."""
    H = ref.shape[-1]
    ref = ref.to(torch.float64)
    got = got[..., :H].to(torch.float64)
    peak = ref.max(dim=-1, keepdim=True).values
    err = (got - ref).abs()
    tol = REL * ref + (floor_for(H) + (C + 1) * 6e-8) * peak
    assert bool((err <= tol).all()), f"{what}: worst ratio to the bound {float((err / tol).max()):.3g}"
    strong = ref > 1e-2 * peak
    assert float((err[strong] / ref[strong]).max()) <= STRONG_REL + (C + 1) * 6e-8, what
    return float((err / peak).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# T1: the automatic 1024-point rule at its boundary (round 6: Cfg1024B from four mixed channels on, for launches that fill their rounds)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,mix,side", [(8, "absmean", "fills"), (4, "absmean", "fills"), (5, "sum", "fills"),
                                        (3, "absmean", "fills"), (8, "absmean", "one_workgroup_short")])
def test_1024_rule_at_its_boundary(jsg, oracle, torch_cuda, C, mix, side):
    """At F_hi (the smallest launch that fills its round of 32-column workgroups) four or more mixed channels take Cfg1024B -- named so,
    equal to plan_select = 2 bit for bit -- and three channels, or one workgroup fewer, take Cfg1024 (= plan_select = 1).  Both sides
    against the float64 DFT, every bin of every column."""
    torch = torch_cuda
    n, n_cu = 1024, _n_cu(torch)
    F = _f_hi(TPB["Cfg1024B"], n_cu) - (1 if side == "one_workgroup_short" else 0)
    takes_b = C >= 4 and _b_rule(F, TPB["Cfg1024B"], n_cu)
    assert takes_b == (side == "fills" and C >= 4)                       # the side of the rule this case is on
    m = jsg.capi.MIX_SUM if mix == "sum" else jsg.capi.MIX_ABSMEAN
    win = oracle.window(oracle.WIN_HANN, n)
    plan = jsg.Plan(n, win)
    x = _stream(torch, C, (F - 1) * HOP + n, seed=1000 + 10 * C)
    H, pitch = n // 2 + 1, 544
    out = {sel: torch.full((F, pitch), SENT, device="cuda") for sel in (0, 1, 2)}
    kw = dict(feedblocks=2, mix_mode=m, linear_out=True)
    name = jsg.stft_kernel_name(plan, x, HOP, F, out[0], **kw)
    assert name == ("Cfg1024B" if takes_b else "Cfg1024"), (name, F, n_cu)
    for sel in (0, 1, 2):
        jsg.stft_db(plan, x, HOP, F, out[sel], plan_select=sel, **kw)
    torch.cuda.synchronize()
    assert not torch.equal(out[1][:, :H], out[2][:, :H]), "the two plans give the same bits on this input: the test cannot tell them apart"
    assert torch.equal(out[0], out[2 if takes_b else 1]), f"{name}: automatic selection differs from the pinned plan"
    ref = _power_f64(torch, x, n, HOP, F, torch.from_numpy(win).cuda(), mix_sum=(mix == "sum"))
    worst = _check_power(torch, out[0], ref, C, f"{name} {C} ch {mix} F={F}")
    print(f"\n  T1 {name} {C} ch {mix} F={F} ({n_cu} CUs): worst error / frame peak {worst:.2e} (FLOOR_BY_N[1024] = {FLOOR_BY_N[1024]:.1e})")


# ---------------------------------------------------------------------------------------------------------------------------------
# T2: strided jobs longer than 2^20 workgroup steps go out as several launches -- all of them on the plan of the whole call
# ---------------------------------------------------------------------------------------------------------------------------------
def _split_case(case, n_cu):
    """(n, C, mix, F, W, ring_pos, tail, expected kernel).  F of (a) / (b): one batch is half a round of "B" workgroups (4096 / 2048
    columns on 256 CUs), so a lone batch does not fill its round while the whole call does."""
    if case == "a_1024_absmean_4ch":
        F = TPB["Cfg1024B"] * (n_cu // 2)
        return 1024, 4, "absmean", F, F, 0, False, "Cfg1024B"
    if case == "b_2048_absmean_2ch":
        F = TPB["Cfg2048B"] * (n_cu // 2)
        return 2048, 2, "absmean", F, F, 0, False, "Cfg2048B"
    return 1024, 8, "per_channel", 1001, 1100, 700, True, "Cfg1024"      # (c): a wrapping ring and the tail plane


def _run_split_job(jsg, oracle, torch, n, C, m, per_ch, F, W, pos, use_tail, K):
    """One strided call of K batches (one input batch repeated: in_batch_stride = 0, out_pitch = n/2 + 1, an untouched gap behind every
    ring) and the single launches of batch 0 pinned to plan 1 and plan 2.  Returns the verdicts only: the ~8-17 GB of buffers are gone
    when it returns, whatever the verdicts are."""
    H = n // 2 + 1
    P = H                                                                # out_pitch = n/2 + 1: no padding behind a column
    rows = C if per_ch else 1
    plan = jsg.Plan(n, oracle.window(oracle.WIN_HANN, n))
    ns = ((F - 1) * HOP + n + 3) // 4 * 4
    d_in = _batches(torch, 1, C, ns, seed=n + F).expand(K, C, ns)       # in_batch_stride = 0
    ring = rows * W * P
    G = 64                                                               # untouched floats behind every ring
    flat = torch.full((K * (ring + G),), SENT, device="cuda")
    shape, strides = ((K, C, W, P), (ring + G, W * P, P, 1)) if per_ch else ((K, W, P), (ring + G, P, 1))
    out = flat.as_strided(shape, strides)
    tail = torch.full((K, rows, W), SENT, device="cuda") if use_tail else None
    kw = dict(feedblocks=n // HOP, mix_mode=m, ring_pos=pos)
    name = jsg.stft_db_strided_kernel_name(plan, d_in, HOP, F, out, d_tail=tail, **kw)
    jsg.stft_db_strided(plan, d_in, HOP, F, out, d_tail=tail, **kw)
    refs = {}
    for sel in (1, 2):
        r = torch.full(shape[1:], SENT, device="cuda")
        rt = torch.full((rows, W), SENT, device="cuda") if use_tail else None
        jsg.stft_db(plan, d_in[0], HOP, F, r, plan_select=sel, d_tail=rt, **kw)
        refs[sel] = (r, rt)
    torch.cuda.synchronize()
    v = {"name": name, "distinct": not torch.equal(refs[1][0], refs[2][0]), "first_bad_ring": None}
    ref, ref_tail = refs[2 if name.endswith("B") else 1]
    v["ring0"] = torch.equal(out[0], ref) and (not use_tail or torch.equal(tail[0], ref_tail))
    S = 32                                                               # batches per comparison (bounded temporaries)
    for b0 in range(1, K, S):
        b1 = min(K, b0 + S)
        same = (out[b0:b1] == out[0]).flatten(1).all(1)
        if use_tail:
            same &= (tail[b0:b1] == tail[0]).flatten(1).all(1)
        if not bool(same.all()):
            v["first_bad_ring"] = b0 + int((~same).nonzero()[0, 0])
            break
    v["gaps_untouched"] = bool((flat.view(K, ring + G)[:, ring:] == SENT).all())
    v["gb"] = flat.numel() * 4 / 1e9
    del d_in, flat, out, tail, refs, ref, ref_tail, same
    torch.cuda.empty_cache()
    return v


@pytest.mark.parametrize("case", ["a_1024_absmean_4ch", "b_2048_absmean_2ch", "c_1024_per_channel_tail"])
def test_split_strided_job_takes_one_plan(jsg, oracle, torch_cuda, case):
    """A job one batch longer than one launch addresses: the launcher issues a launch of the first batches and a single launch of the
    last one.  Every ring must equal ring 0 bit for bit, ring 0 must equal ONE single launch pinned to the plan
    jsg_stft_db_strided_kernel_name reports, and nothing outside the columns (the gap behind every ring, the ring columns the launch does
    not own, the float behind a column of the tail layout) is written.  The input is one batch repeated (in_batch_stride = 0)."""
    torch = torch_cuda
    cap = jsg.capi
    n_cu = _n_cu(torch)
    n, C, mix, F, W, pos, use_tail, expect = _split_case(case, n_cu)
    per_ch = mix == "per_channel"
    rows = C if per_ch else 1
    # steps as the launcher counts them (jsg_stft_db_launch_strided: the smallest workgroup step of the plan's kernels, 4 columns)
    steps = rows * -(-F // TPB[f"Cfg{n}"])
    K = STEP_LIMIT // steps + 1
    assert (K - 1) * steps <= STEP_LIMIT < K * steps                    # exactly one batch more than one launch takes
    if expect.endswith("B"):
        assert _b_rule(K * F, TPB[expect], n_cu) and not _b_rule(F, TPB[expect], n_cu)   # the whole call fills, one batch alone does not
    v = _run_split_job(jsg, oracle, torch, n, C, cap.MIX_PER_CHANNEL if per_ch else cap.MIX_ABSMEAN, per_ch, F, W, pos, use_tail, K)
    name = v["name"]
    print(f"\n  T2 {case}: {K} batches x {rows} row(s) x {F} columns = {K * steps} steps, {name} ({n_cu} CUs), output {v['gb']:.1f} GB")
    assert name == expect, (name, expect, K, n_cu)
    assert v["distinct"], "the two plans give the same bits on this input: the test cannot tell them apart"
    assert v["ring0"], f"{name}: ring 0 differs from a single launch pinned to the reported plan"
    assert v["first_bad_ring"] is None, \
        f"{name}: ring {v['first_bad_ring']} of {K} differs from ring 0 (one launch takes {STEP_LIMIT // steps} batches)"
    assert v["gaps_untouched"], f"{name}: something behind a ring was written"


# ---------------------------------------------------------------------------------------------------------------------------------
# T3: Max / Min strided at 2048 / 4096 points -- launched batch by batch, so ONE batch decides the plan
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,C,mix", [(2048, 8, "max"), (4096, 2, "min")])
def test_max_min_strided_report_the_plan_of_one_batch(jsg, oracle, torch_cuda, n, C, mix):
    """Max / Min have no strided kernel: every batch is its own launch.  With a call that fills its rounds while one batch does not, the
    name query must report what one batch takes (the small-workgroup kernel) and the columns must be those of single launches pinned to
    it (test_gpu_strided._run_case pins them to the reported plan)."""
    torch = torch_cuda
    cap = jsg.capi
    n_cu = _n_cu(torch)
    tpb_b = TPB[f"Cfg{n}B"]
    F, K = tpb_b * (n_cu // 4), 4
    assert _b_rule(K * F, tpb_b, n_cu) and not _b_rule(F, tpb_b, n_cu)     # the whole call fills, one batch does not
    m = cap.MIX_MAX if mix == "max" else cap.MIX_MIN
    name = _run_case(jsg, oracle, torch, n, C, F, K, HOP, mix=m, W=F + 13, ring_pos=F // 2)
    assert name == f"Cfg{n}", (name, F, K, n_cu)
    # the plans are told apart on this input: _run_case's batch 0 (same generator, same seed), single launches pinned to 1 and 2
    fb = n // HOP
    last = F - 1
    ns = ((last // fb) * n + (last % fb) * HOP + n + 3) // 4 * 4
    x0 = _batches(torch, K, C, ns, seed=n + 7 * F + K)[0]
    plan = jsg.Plan(n, oracle.window(oracle.WIN_HANN, n))
    pitch = (n // 2 + 1 + 31) // 32 * 32
    o = {sel: torch.full((F, pitch), SENT, device="cuda") for sel in (1, 2)}
    for sel in (1, 2):
        jsg.stft_db(plan, x0, HOP, F, o[sel], feedblocks=fb, mix_mode=m, plan_select=sel)
    torch.cuda.synchronize()
    assert not torch.equal(o[1], o[2]), "the two plans give the same bits on this input: the test cannot tell them apart"
    print(f"\n  T3 {mix} {n} points {C} ch: {K} x {F} columns ({n_cu} CUs) -> {name}")


# ---------------------------------------------------------------------------------------------------------------------------------
# T4: the display contract at 1024 points -- the display launches always take the three-stage arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------
def test_1024_display_image_is_that_of_the_three_stage_plan(jsg, oracle, torch_cuda):
    """8 channels AbsMean at F_hi, where stft_db takes Cfg1024B by itself: stft_image (one kernel) and stft_image_strided (4 images, one
    kernel) with plan_select 0, 1 and 2 give the pixels of stft_db(plan_select = 1) + colormap.  256 colours over +-2 dB around the
    median dB of the input make the image sensitive to the last bits: stft_db(1) + colormap and stft_db(2) + colormap must differ."""
    torch = torch_cuda
    n, C, K = 1024, 8, 4
    n_cu = _n_cu(torch)
    F = _f_hi(TPB["Cfg1024B"], n_cu)
    assert _b_rule(F, TPB["Cfg1024B"], n_cu)
    H = n // 2 + 1
    plan = jsg.Plan(n, oracle.window(oracle.WIN_HANN, n))
    ns = (F - 1) * HOP + n
    d_in = torch.stack([_stream(torch, C, ns, seed=4000 + k) for k in range(K)]).contiguous()       # [K][C][samples]
    d_lut = torch.from_numpy(jsg.colormap_lut(256, jsg.capi.CM_JADE)).cuda()
    db = {sel: torch.empty((K, F, 544), device="cuda") for sel in (1, 2)}
    assert jsg.stft_kernel_name(plan, d_in[0], HOP, F, db[1][0], feedblocks=2) == "Cfg1024B"
    for sel in (1, 2):
        for k in range(K):
            jsg.stft_db(plan, d_in[k], HOP, F, db[sel][k], feedblocks=2, plan_select=sel)
    torch.cuda.synchronize()
    med = float(db[1][0, :, :H].median())
    lo, hi = med - 2.0, med + 2.0
    two = {}
    for sel in (1, 2):
        two[sel] = torch.zeros((K, H, F), dtype=torch.int32, device="cuda")
        for k in range(K):
            jsg.colormap(db[sel][k], d_lut, lo, hi, d_argb=two[sel][k], n_cols=F, height=H)
    torch.cuda.synchronize()
    flips = int((two[1] != two[2]).sum())      # measured on an MI355X (256 CUs, F = 7105): 867 of 14 579 460 pixels
    print(f"\n  T4 F={F} ({n_cu} CUs), colours over {lo:.2f}..{hi:.2f} dB: {flips} of {two[1].numel()} pixels differ between the plans")
    assert flips > 0, "the colour range does not expose the last bits: the test cannot tell the plans apart"
    kw = dict(feedblocks=2, ring_width=F, x_first=0)
    for sel in (0, 1, 2):
        one = torch.full((K, H, F), 0x12345678, dtype=torch.int32, device="cuda")
        for k in range(K):
            assert not jsg.stft_image_needs_scratch(plan, d_in[k], HOP, F, d_lut, lo, hi, one[k], None, plan_select=sel, **kw)
            jsg.stft_image(plan, d_in[k], HOP, F, d_lut, lo, hi, one[k], None, plan_select=sel, **kw)
        strided = torch.full((K, H, F), 0x12345678, dtype=torch.int32, device="cuda")
        assert not jsg.stft_image_strided_needs_scratch(plan, d_in, HOP, F, d_lut, lo, hi, strided, None, plan_select=sel, **kw)
        jsg.stft_image_strided(plan, d_in, HOP, F, d_lut, lo, hi, strided, None, plan_select=sel, **kw)
        torch.cuda.synchronize()
        assert torch.equal(one, two[1]), f"plan_select = {sel}: stft_image differs from stft_db(plan_select = 1) + colormap"
        assert torch.equal(strided, two[1]), f"plan_select = {sel}: stft_image_strided differs from stft_db(plan_select = 1) + colormap"


# ---------------------------------------------------------------------------------------------------------------------------------
# T5: the kernels bench.py times, next to the float64 DFT
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["c2", "c4"])
def test_timed_strided_dispatch_every_bin_against_float64(jsg, oracle, torch_cuda, cfg):
    """The strided dispatch of bench.py's C2 line (64 mono batches of 4096 columns, hop 512) and of one GPU's C4 shard (8 batches x 8
    channels, one column per channel), a different seeded bench.synth_audio input per batch: every bin of every column of every batch
    against the float64 DFT, one batch at a time, and the dB columns of >= 512 columns spread over all batches.  Both geometries take the
    "runs" kernel -- csrc/jsg_kernels.hip, resolve_variant: k1024Runs = a strided launch at 1024 points, not the "B" plan, no display, one
    channel per column (mixop 3), regular frames with 2 * hop == n -- which no query reports; the conditions are asserted here."""
    torch = torch_cuda
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    c = bench.CONFIGS[cfg]
    n, hop, C, F = c["n"], c["hop"], c["channels"], c["frames"]
    per_ch = bool(c.get("per_channel"))
    K = 64 if cfg == "c2" else 8
    assert n == 1024 and 2 * hop == n and (C == 1 or per_ch)           # the "runs" conditions that depend on the geometry
    H, pitch = n // 2 + 1, 544
    win = jsg.window(jsg.capi.WIN_HANN, n)
    plan = jsg.Plan(n, win)
    ns = (F * hop + (n - hop) + 3) // 4 * 4
    d_in = torch.empty((K, C, ns), device="cuda")
    for b in range(K):
        d_in[b].copy_(torch.from_numpy(bench.synth_audio(C, ns, fs=c["fs"], seed=5000 + 97 * b)))
    m = jsg.capi.MIX_PER_CHANNEL if per_ch else jsg.capi.MIX_ABSMEAN
    shape = (K, C, F, pitch) if per_ch else (K, F, pitch)
    d_pow = torch.empty(shape, device="cuda")
    d_db = torch.empty(shape, device="cuda")
    kw = dict(feedblocks=n // hop, mix_mode=m)
    assert jsg.stft_db_strided_kernel_name(plan, d_in, hop, F, d_db, **kw) == "Cfg1024"
    jsg.stft_db_strided(plan, d_in, hop, F, d_pow, linear_out=True, **kw)
    jsg.stft_db_strided(plan, d_in, hop, F, d_db, **kw)
    w32 = torch.from_numpy(win).cuda()
    rng = np.random.default_rng(20261015)
    per_row = 16 if cfg == "c2" else 8                                   # dB columns per row: 1024 (C2) / 512 (C4) in all
    worst = 0.0
    db_cols = 0
    for b in range(K):
        for ch in range(C if per_ch else 1):
            x = d_in[b, ch:ch + 1]
            got_p = d_pow[b, ch] if per_ch else d_pow[b]
            got_db = d_db[b, ch] if per_ch else d_db[b]
            ref = _power_f64(torch, x, n, hop, F, w32)                    # [F][H] float32 (one channel: no mix)
            worst = max(worst, _check_power(torch, got_p, ref, 1, f"{cfg} batch {b} channel {ch}"))
            cols = np.sort(rng.choice(F, per_row, replace=False))
            p32 = ref[torch.from_numpy(cols).cuda()].cpu().numpy()
            assert_db_close(got_db[torch.from_numpy(cols).cuda(), :H].cpu().numpy(), oracle.to_db(p32), p32.astype(np.float64),
                            f"{cfg} batch {b} channel {ch} dB")
            db_cols += len(cols)
    assert db_cols >= 512
    print(f"\n  T5 {cfg}: {K} batches x {C if per_ch else 1} row(s) x {F} columns, every bin against float64: worst error / frame peak "
          f"{worst:.2e} (FLOOR_BY_N[1024] = {FLOOR_BY_N[1024]:.1e}); {db_cols} dB columns checked")

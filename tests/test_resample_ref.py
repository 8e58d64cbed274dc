"""The reference of band-limited resampling checked against itself on the CPU (tests/resample_ref.py): the float32 restatement within
half of the per-sample cap, the tables good enough to carry a tone, the analytic cases to the bit, and the output length."""
import numpy as np
import pytest

import resample_ref as rr

# The tone at 0.05 cycles per input sample lies in the passband while 0.05 * step < rolloff / 2, and the middle half of the output
# sees whole wings while L / 4 >= Z * step: every step of the list but 64 (the tone is filtered out) and 1/64 (L = 40 is shorter than a wing).
TONE_STEPS = [s for s in rr.STEPS if s not in ("64", "1/64")]


@pytest.mark.parametrize("c", rr.CASES, ids=rr.case_id)
def test_restatement_within_half_the_cap(c):
    r = rr.case(*c)
    err = np.abs(r["y32"].astype(np.float64) - r["y64"])
    assert np.isfinite(err).all() and (err <= 0.5 * r["cap"]).all(), float((err / np.maximum(r["cap"], 1e-300)).max())


@pytest.mark.parametrize("name,bound", [("best", 2e-6), ("fast", 5e-5)])
def test_interior_tone_error(name, bound):
    worst = 0.0
    for s in TONE_STEPS:
        r, step = rr.case(name, s), rr.STEPS[s]
        T = r["T"]
        i = np.arange(T // 4, 3 * T // 4)
        want = np.sin(2 * np.pi * 0.05 * (i * step))
        worst = max(worst, float(np.abs(r["y64"][1, i] - want).max()))
    print(f"{name}: worst interior tone error {worst:.3g}")
    assert worst <= bound


def test_ramp_at_step_1_is_the_identity():
    Z, P, win = rr.table("ramp")
    x = rr.inputs(3000)
    r = rr.evaluate(x, 1.0, Z, P, win)
    assert r["T"] == 3000 and np.array_equal(r["y32"].view(np.uint32), x.view(np.uint32))


def test_ramp_at_step_half_is_linear_interpolation():
    Z, P, win = rr.table("ramp")
    x = rr.inputs(3000)
    y = rr.evaluate(x, 0.5, Z, P, win)["y32"]
    assert y.shape == (3, 6000)
    assert np.array_equal(y[:, 0::2].view(np.uint32), x.view(np.uint32))
    nxt = np.concatenate([x[:, 1:], np.zeros((3, 1), np.float32)], axis=1)     # past the end there is no live tap
    want = np.float32(0.5) * x + np.float32(0.5) * nxt                          # both products exact: fl(0.5 (x[q] + x[q+1]))
    assert np.array_equal(y[:, 1::2].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(want[:, :-1], (np.float32(0.5) * (x[:, :-1] + x[:, 1:])).astype(np.float32))


@pytest.mark.parametrize("c", rr.CASES, ids=rr.case_id)
def test_impulse_is_one_product_chain(c):
    Z, P, win = rr.table(c[0])
    L = rr.case_length(c[1])
    want = rr.impulse_response(L, rr.STEPS[c[1]], Z, P, win, rr.impulse_at(L))
    got = rr.case(*c)["y32"][2]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.count_nonzero(want) > 0


def test_live_range_matches_the_sum():
    """first / last bracket exactly the inputs an output depends on: a NaN just outside changes nothing, one just inside does."""
    Z, P, win = rr.table("fast")
    x = np.array(rr.inputs(3000)[:1])
    clean = rr.evaluate(x, 3.7, Z, P, win)
    for m0 in (0, 1499, 2999):
        bad = x.copy()
        bad[0, m0] = np.nan
        r = rr.evaluate(bad, 3.7, Z, P, win)
        hit = (clean["first"] <= m0) & (m0 <= clean["last"])
        assert hit.any() and np.isnan(r["y32"][0][hit]).all() and np.isnan(r["y64"][0][hit]).all()
        assert np.array_equal(r["y32"][0][~hit].view(np.uint32), clean["y32"][0][~hit].view(np.uint32))


@pytest.mark.parametrize("name", sorted(rr.RATIONAL))
def test_length_is_torchaudios_for_rational_steps(name):
    orig, new = rr.RATIONAL[name]
    step = rr.STEPS[name]
    for L in range(1, 2001):
        assert rr.resample_length(L, step) == -(-L * new // orig), L

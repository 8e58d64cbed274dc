"""tests/cqt_ref.py checked on the CPU: the tone identity of the standard basis, the impulse identity, the restatement inside its cap and
the hop-delay identity on interior frames."""
import numpy as np

import cqt_ref as cr


def raw(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_basis_sizes_of_the_issue():
    half, offset, f, length, taps = cr.basis(22050.0, cr.C1, 84)
    n = 2 * half.astype(np.int64) + 1
    assert n[0] == 11685 and n[-1] == 97 and int(n.sum()) == 206580 == taps.size
    assert np.array_equal(offset, cr.offsets(half)) and abs(f[12] - 2 * cr.C1) < 1e-9
    # L1 norm: 1, times sqrt(l_k) with the scale
    for k in (0, 40, 83):
        assert abs(np.abs(taps[offset[k]:offset[k] + n[k]].astype(np.complex128)).sum() / np.sqrt(length[k]) - 1.0) < 1e-6


def test_tone_at_a_bin_centre_gives_half_its_amplitude():
    half, offset, f, length, taps = cr.standard_basis(False)
    ref = cr.standard_case(False)
    C = ref["C64"][1]                                      # the tone of amplitude 0.5 at bin 12
    inside = cr.interior(half, cr.STANDARD_HOP, C.shape[0], cr.STANDARD_L)
    frames = np.flatnonzero(inside.all(axis=1))
    assert frames.size >= 10
    mag = np.abs(C[frames])
    print("tone: |C| at the bin", mag[:, 12].min(), mag[:, 12].max(), "neighbours", mag[:, 11].max(), mag[:, 13].max())
    assert (np.abs(mag[:, 12] / 0.25 - 1.0) <= 1e-4).all()
    assert (mag.argmax(axis=1) == 12).all()


def test_impulse_identity():
    half, taps = cr.synthetic_basis()
    m0 = cr.impulse_at(cr.L)
    for hop in cr.HOPS:
        ref = cr.case(hop)
        T = cr.frames(cr.L, hop)
        want = cr.impulse_response(half, taps, hop, T, m0)
        hit = cr.touched(half, hop, T, m0)
        assert (hit.any() or hop > cr.L) and not hit.all()        # hop 5000: one frame, which the impulse does not reach
        assert (ref["C32"][2] == want).all() and (ref["C64"][2] == want.astype(np.complex128)).all()
        assert np.array_equal(raw(ref["C32"][2][hit]), raw(want[hit]))


def test_restatement_stays_inside_its_cap():
    half, taps = cr.synthetic_basis()
    worst = 0.0
    for hop in cr.HOPS:
        ref = cr.case(hop)
        cap_re, cap_im = cr.restatement_cap(half, ref)
        d = ref["C32"].astype(np.complex128) - ref["C64"]
        for err, cap in ((np.abs(d.real), cap_re), (np.abs(d.imag), cap_im)):
            assert (err <= cap).all()
            worst = max(worst, float((err / np.maximum(cap, 1e-300)).max()))
    half, _, _, _, taps = cr.standard_basis()
    ref = cr.standard_case()
    cap_re, cap_im = cr.restatement_cap(half, ref)
    d = ref["C32"].astype(np.complex128) - ref["C64"]
    assert (np.abs(d.real) <= cap_re).all() and (np.abs(d.imag) <= cap_im).all()
    worst = max(worst, float((np.abs(d.real) / np.maximum(cap_re, 1e-300)).max()))
    print("restatement: worst error over its cap", worst)
    # ... and inside cap (b), which holds for any order
    assert (np.abs(d.real) <= ref["cap_re"]).all() and (np.abs(d.imag) <= ref["cap_im"]).all()


def test_hop_delay_identity_on_interior_frames():
    half, taps = cr.synthetic_basis()
    x = np.array(cr.inputs(cr.L)[:2])
    for hop in (7, 64, 512):
        T = cr.frames(cr.L, hop)
        delayed = np.zeros_like(x)
        delayed[:, hop:] = x[:, :-hop]
        a = cr.evaluate(x, half, taps, hop, T)["C32"]
        b = cr.evaluate(delayed, half, taps, hop, T)["C32"]
        inside = cr.interior(half, hop, T, cr.L)
        both = inside[1:] & inside[:-1]
        assert both.any()
        for r in range(2):
            assert np.array_equal(raw(b[r, 1:][both]), raw(a[r, :-1][both]))

"""A census of the lane-split forms of the beat and Viterbi kernels of libjsgx.so (include/jsgx.h sections 1 and 4) against the shape lists
that drive their GPU tests (beat_ref.FORM_PERIODS, viterbi_ref.FORM_STATES, viterbi_ref.FORM_BANDS).  The forms are derived here from the
restated rules (beat_ref.form, viterbi_ref.form) and from the library's own plan calls over every period and state count, not copied: a
new form, or a boundary that moves, leaves a form or one side of a boundary outside the lists and fails here, before a GPU test that
no longer runs it passes.  CPU only: the plan calls need no device."""
import beat_ref as br
import viterbi_ref as vr


def census(keys, listed, what):
    """keys: {size: form key} over a contiguous range of sizes.  Every distinct key has a listed size, and wherever the key changes between
    size - 1 and size both are listed.  Returns the sizes at which the key changes."""
    listed = set(listed)
    assert listed <= set(keys), (what, "a listed size outside the range", sorted(listed - set(keys)))
    missing = {key for key in set(keys.values()) if not any(keys[size] == key for size in listed)}
    assert not missing, (what, "forms that no listed size runs", sorted(missing))
    changes = [size for size in sorted(keys) if size - 1 in keys and keys[size - 1] != keys[size]]
    one_sided = [size for size in changes if size - 1 not in listed or size not in listed]
    assert not one_sided, (what, "boundaries (the first size of the new form) without both sides listed", one_sided)
    return changes


def test_beat_periods_cover_every_form_and_both_sides_of_every_boundary(jsg):
    keys = {}
    for P in range(1, br.MAX_PERIOD + 1):
        a, G, F = br.form(P)
        name = jsg.beat_plan(P)[0]
        assert name == ("beat_frames" if G == 1 else "beat_split"), (P, name, G)      # the restated rule and the library agree on the one thing the plan tells
        keys[P] = (G, F, name)
    changes = census(keys, br.FORM_PERIODS, "beat")
    print("beat: the form changes at", changes, "forms:", sorted(set(keys.values())))
    assert len(changes) >= 2 and len(set(keys.values())) == len(changes) + 1        # a form is one run of periods


def test_viterbi_state_counts_cover_every_form_and_both_sides_of_every_boundary(jsg):
    keys = {}
    for S in range(1, 2049):
        G, threads = vr.form(S)
        name, plan_threads = jsg.viterbi_plan(S, 3)[:2]
        assert plan_threads == threads, (S, plan_threads, threads)      # ties the restated rule to the library
        keys[S] = (name, G)
    changes = census(keys, vr.FORM_STATES, "viterbi dense")
    print("viterbi: the form changes at", changes, "forms:", sorted(set(keys.values())))
    assert len(changes) >= 2 and len(set(keys.values())) == len(changes) + 1


def test_viterbi_bands_on_every_side_of_every_lane_split(jsg):
    """For every G that a state count gives: a listed band with fewer sources per destination than G lanes (2W + 1 < G; G = 1 has none), one
    next to G (the nearest odd numbers: G - 1 or G + 1, and 1 for G = 1) and one with more."""
    groups = {vr.form(S)[0] for S in range(1, 2049)}
    widths = {G: {2 * W + 1 for S, W in vr.FORM_BANDS if vr.form(S)[0] == G} for G in groups}
    for S, W in vr.FORM_BANDS:
        assert 1 <= S <= 2048 and 0 <= W <= jsg.capix.VITERBI_MAX_BAND_HALF, (S, W)
    for G in sorted(groups):
        near = {1} if G == 1 else {G - 1, G + 1}
        assert G == 1 or any(w < G for w in widths[G]), (G, "no band narrower than the lane split", sorted(widths[G]))
        assert widths[G] & near, (G, "no band next to the lane split", sorted(widths[G]))
        assert any(w > G for w in widths[G]), (G, "no band wider than the lane split", sorted(widths[G]))


def test_viterbi_bands_on_both_sides_of_the_lds_limit(jsg):
    """At W = 64 the table and the two rows of V fill the LDS up to S = 312; the list holds that and the first S that does not fit.  The limit
    is found from the plan, over every S."""
    W = jsg.capix.VITERBI_MAX_BAND_HALF
    names = {S: jsg.viterbi_plan(S, 3, band_half=W)[0] for S in range(1, 2049)}
    last = max(S for S, name in names.items() if name == "viterbi_band_lds")
    assert all(name == ("viterbi_band_lds" if S <= last else "viterbi_band_mem") for S, name in names.items())
    assert (last, W) in vr.FORM_BANDS and (last + 1, W) in vr.FORM_BANDS, last
    assert jsg.viterbi_plan(312, 3, band_half=64)[::2] == ("viterbi_band_lds", 163488) and names[313] == "viterbi_band_mem"
    assert 163488 <= jsg.capix.VITERBI_LDS_LIMIT < 4 * (129 * 313 + 2 * 313)
    # the plan's name over the whole list, as the GPU test expects it: the header's rule on the bytes of the table and two rows of V
    for S, Wb in vr.FORM_BANDS:
        fits = 4 * ((2 * Wb + 1) * S + 2 * S) <= jsg.capix.VITERBI_LDS_LIMIT
        assert jsg.viterbi_plan(S, 3, band_half=Wb)[0] == ("viterbi_band_lds" if fits else "viterbi_band_mem"), (S, Wb)

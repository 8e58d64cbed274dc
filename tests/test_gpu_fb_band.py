"""The band kernel of the filterbank spectrograms (fb_band_kernel, csrc/jsg_filterbank.hip) on its own: all six instantiations (8, 4 or 2
power columns per LDS tile x the bank staged in LDS or read through the caches), workgroups that take a second and a third tile, partial
last tiles, tiles that straddle rows and batches and hold the ring wrap, band counts around the band loop's stride of 256 threads, band
shapes at both ends of the axis, NaN and Inf containment inside a tile, and the same bits for every chunking.

Reference of every case: the power plane the band kernel read, fetched with stft_db_strided(linear_out=True) pinned to the STFT variant
jsg_stft_fb_kernel_name reported (the two kernel names are asserted equal), then the bank on the host in the specified order
(fb_band_ref.band_f32).  Bit for bit in linear and exact-log mode; the hardware logarithm within DB_SLACK of the exact one.

Every test asserts, through jsg_fb_band_plan, the (tile_cols, bank_in_lds) it claims to cover, passes scratch for one chunk (the whole
call is then ONE band launch of the stated column count), and fills the output with a sentinel that everything outside the written band
columns must still hold: past n_bands up to out_pitch, the unvisited ring columns, the padding between channel planes and batches."""
import numpy as np
import pytest

import fb_band_ref as R
from parity_util import DB_SLACK

pytestmark = pytest.mark.gpu

SENT = -7.0
PER_CHANNEL = 100
PAD_COLS, PAD_FLOATS = 2, 3                  # ring columns between channel planes, floats of a column past the bands
STEP = {"Cfg512": 16, "Cfg1024": 4, "Cfg1024B": 32, "Cfg2048": 4, "Cfg2048B": 16, "Cfg2048P": 16, "Cfg4096": 2, "Cfg4096B": 8,
        "Cfg8192": 1}                        # columns per workgroup step of the STFT variants (Cfg::TPB in csrc/jsg_stft_kernel.h)
MODES = ("linear", "exact", "hw")


class Ctx:
    def __init__(self, jsg, oracle, torch, mir):
        self.jsg, self.oracle, self.torch, self.mir = jsg, oracle, torch, mir
        self.n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        self._plans, self._cache = {}, {}

    def plan(self, n):
        if n not in self._plans:
            self._plans[n] = self.jsg.Plan(n, self.oracle.window(self.oracle.WIN_HANN, n))
        return self._plans[n]

    def cached(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def audio(self, k, ch, L, seed):
        return self.oracle.synth_audio(k * ch, L, seed=seed).reshape(k, ch, L)


@pytest.fixture(scope="module")
def ctx(jsg, oracle):
    import torch
    from oracle import mirror
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return Ctx(jsg, oracle, torch, mirror.load())


def band_plan(ctx, n, fb, n_cols):
    return ctx.jsg.fb_band_plan(n, fb.n_bands, fb.weights.size, n_cols, ctx.n_cu)


def claim(ctx, n, fb, n_cols, T, lds):
    """The instantiation this call reaches, asserted: fb_band_kernel<T, lds>."""
    p = band_plan(ctx, n, fb, n_cols)
    assert (p["tile_cols"], p["bank_in_lds"]) == (T, lds), (n, fb.n_bands, fb.weights.size, p)
    assert lds == (3 * fb.n_bands + fb.weights.size <= 7168)
    return p


def run_band(ctx, n, fb, xs, hop, F, *, mix, mode, W=None, pos=0, scratch_cols=None):
    """One strided filterbank call on xs [k][ch][L].  Returns (the whole output allocation [k][rows+1][W+PAD_COLS][B+PAD_FLOATS] or, mixed
    down, [k][W+PAD_COLS][B+PAD_FLOATS], the STFT kernel name).  scratch_cols None: scratch for the whole call (one band launch)."""
    jsg, torch = ctx.jsg, ctx.torch
    plan = ctx.plan(n)
    k, ch, _ = xs.shape
    rows = ch if mix == PER_CHANNEL else 1
    W = W or F
    d_in = torch.from_numpy(xs).cuda()
    shape = (k, rows + 1, W + PAD_COLS, fb.n_bands + PAD_FLOATS) if mix == PER_CHANNEL else (k, W + PAD_COLS, fb.n_bands + PAD_FLOATS)
    base = torch.full(shape, SENT, dtype=torch.float32, device="cuda")
    d_out = base[:, :rows, :W] if mix == PER_CHANNEL else base[:, :W]
    kw = dict(mix_mode=mix, ring_pos=pos, linear_out=mode == "linear", exact_log=mode == "exact")
    name = jsg.stft_fb_kernel_name(plan, fb, d_in, hop, F, d_out, strided=True, **kw)
    pitch = band_plan(ctx, n, fb, 1)["pw_pitch"]
    cols = max(k * rows * F, 64) if scratch_cols is None else scratch_cols
    d_sc = torch.empty(cols * pitch, dtype=torch.float32, device="cuda")
    jsg.stft_fb_db_strided(plan, fb, d_in, hop, F, d_out, d_scratch=d_sc, **kw)
    torch.cuda.synchronize()
    return base.cpu().numpy(), name


def power_plane(ctx, n, xs, hop, F, mix, name):
    """The power columns the band kernel read, [k * rows * F][n/2+1] in its column order: stft_db_strided pinned to the variant `name`."""
    jsg, torch = ctx.jsg, ctx.torch
    plan = ctx.plan(n)
    k, ch, _ = xs.shape
    rows = ch if mix == PER_CHANNEL else 1
    H = n // 2 + 1
    sel = {"": 1, "B": 2, "P": 3}[name[len(f"Cfg{n}"):]] if n in (1024, 2048, 4096) else 0
    d_in = torch.from_numpy(xs).cuda()
    d_pw = torch.zeros((k, rows, F, H) if mix == PER_CHANNEL else (k, F, H), dtype=torch.float32, device="cuda")
    kw = dict(mix_mode=mix, linear_out=True, plan_select=sel)
    assert jsg.stft_db_strided_kernel_name(plan, d_in, hop, F, d_pw, **kw) == name
    jsg.stft_db_strided(plan, d_in, hop, F, d_pw, **kw)
    torch.cuda.synchronize()
    return d_pw.cpu().numpy().reshape(-1, H)


def split_output(base, fb, F, W, pos, mix):
    """(band columns [k * rows * F][B] in the kernel's column order, True where everything else still holds the sentinel)."""
    B = fb.n_bands
    ring = (pos + np.arange(F)) % W
    written = np.zeros(base.shape, bool)
    if mix == PER_CHANNEL:
        written[:, :-1, ring, :B] = True
        got = base[:, :-1][:, :, ring, :B]
    else:
        written[:, ring, :B] = True
        got = base[:, ring, :B]
    return np.ascontiguousarray(got).reshape(-1, B), bool((base[~written] == SENT).all())


def reference(ctx, P, fb):
    """(band power, exact dB of it, where the band power is >= 0: inside the logarithm's contract)."""
    with np.errstate(all="ignore"):
        lin = R.band_f32(np.asfortranarray(P), fb)
        return lin, ctx.mir.exact_db(np.maximum(lin, 0.0)), lin >= 0


def check_modes(ctx, n, fb, xs, hop, F, *, mix, W, pos, float64_bound=False):
    """Run the call in the three output modes against the host reference; returns the STFT kernel name."""
    P = name = None
    got = {}
    for mode in MODES:
        base, nm = run_band(ctx, n, fb, xs, hop, F, mix=mix, mode=mode, W=W, pos=pos)
        if P is None:
            name = nm
            P = power_plane(ctx, n, xs, hop, F, mix, name)
        assert nm == name
        got[mode], clean = split_output(base, fb, F, W, pos, mix)
        assert clean, f"{name} {mode}: written outside the band columns"
    lin, db, ok = reference(ctx, P, fb)
    assert ok.mean() > 0.9
    bits = lambda a: a.view(np.uint32)
    assert (bits(got["linear"]) == bits(lin)).all(), (name, "linear", int((bits(got["linear"]) != bits(lin)).sum()), lin.size)
    assert (bits(got["exact"])[ok] == bits(db)[ok]).all(), (name, "exact", int((bits(got["exact"]) != bits(db))[ok].sum()), lin.size)
    assert np.abs(got["hw"].astype(np.float64) - got["exact"])[ok].max() <= DB_SLACK, name
    if float64_bound:
        err, cap = np.abs(got["linear"].astype(np.float64) - R.band_f64(P, fb)), R.band_cap(P, fb)
        assert (err <= cap).all(), f"{name}: worst ratio {np.max(err / np.maximum(cap, 1e-300)):.3g}"
    return name


# ---------------------------------------------------------------------------------------------------------------------------------
# a. every instantiation, with second and third tiles
# ---------------------------------------------------------------------------------------------------------------------------------
def full_case(ctx, n, bank):
    """Bank, geometry and input of the full case: n_cols = 2 T G + T + 1 columns for the grid G of this device, made up of batches x
    channels x frames in per-channel mode, ring_width = frames + 3, ring_pos = ring_width - 5."""
    def make():
        fb = R.full_bank(ctx.jsg, n, bank)
        p = band_plan(ctx, n, fb, 1 << 28)
        T, G = p["tile_cols"], p["grid"]
        n_cols = 2 * T * G + T + 1
        k, ch, F = R.split_columns(n_cols)
        hop = n // 8
        xs = ctx.audio(k, ch, (F - 1) * hop + n, seed=n + len(bank))
        return dict(fb=fb, T=T, G=G, n_cols=n_cols, k=k, ch=ch, F=F, hop=hop, xs=xs, W=F + 3, pos=F + 3 - 5)
    return ctx.cached(("full", n, bank), make)


@pytest.mark.parametrize("n,bank,lds", R.FULL_CASES)
def test_every_instantiation_with_second_and_third_tiles(ctx, n, bank, lds):
    c = full_case(ctx, n, bank)
    fb, T, G, n_cols, k, ch, F = (c[x] for x in ("fb", "T", "G", "n_cols", "k", "ch", "F"))
    p = claim(ctx, n, fb, n_cols, {512: 8, 2048: 8, 4096: 4, 8192: 2}[n], lds)
    assert k * ch * F == n_cols and p["grid"] == G
    n_tiles = -(-n_cols // T)
    assert n_tiles == 2 * G + 2 and n_cols - (n_tiles - 1) * T == 1      # every workgroup two tiles, 0 and 1 a third, the last tile one column
    rows = k * ch                                                          # rows of F columns in the chunk
    assert F % T != 0
    if rows > 1:                                                           # (a prime n_cols is one row: 8192 points, bank through L2, 256 CUs)
        assert any((r * F) % T for r in range(1, rows)), "no tile straddles two rows"
    if k > 1:
        assert any((b * ch * F) % T for b in range(1, k)), "no tile straddles two batches"
    # ring: frame j goes to column (pos + j) % W: the wrap sits between j = 4 and j = 5
    assert (c["pos"] + 4) % c["W"] == c["W"] - 1 and (c["pos"] + 5) % c["W"] == 0
    assert any((r * F + 4) // T == (r * F + 5) // T for r in range(rows)), "no tile holds the ring wrap"
    name = check_modes(ctx, n, fb, c["xs"], c["hop"], F, mix=PER_CHANNEL, W=c["W"], pos=c["pos"], float64_bound=True)
    print(f"\n  fb_band_kernel<{T}, {str(lds).lower()}> after {name}: grid {G}, {n_cols} columns = {k} batches x {ch} channels x {F} frames, "
          f"{n_tiles} tiles, {fb.n_bands} bands, {fb.weights.size} weights")


def test_the_full_cases_straddle_rows_and_batches_at_every_tile_size(ctx):
    """On this device's grid the column counts of the six cases factor into several rows (and batches) for T = 8, 4 and 2."""
    seen = {}
    for n, bank, _ in R.FULL_CASES:
        c = full_case(ctx, n, bank)
        s = seen.setdefault(c["T"], [False, False])
        s[0] |= c["k"] * c["ch"] > 1
        s[1] |= c["k"] > 1
    assert seen == {8: [True, True], 4: [True, True], 2: [True, True]}, seen


# ---------------------------------------------------------------------------------------------------------------------------------
# b. column-count edges
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,n_cols", [(T, c) for T in (8, 4, 2) for c in sorted({1, T - 1, T, T + 1})])
def test_column_count_edges(ctx, T, n_cols):
    n = R.TILE_N[T]
    fb = ctx.cached(("linear40", n), lambda: ctx.jsg.Filterbank(n, R.FS, 40, 100.0, 12000.0, scale=ctx.jsg.capi.FB_LINEAR))
    claim(ctx, n, fb, n_cols, T, True)
    hop, F = n // 4, n_cols                               # mixed down, one batch: one row of n_cols columns
    xs = ctx.audio(1, 2, (F - 1) * hop + n, seed=3 * n + n_cols)
    check_modes(ctx, n, fb, xs, hop, F, mix=0, W=F + 2, pos=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# c. band-count and band-shape edges
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [8, 4, 2])
@pytest.mark.parametrize("bank", R.EDGE_BANKS)
def test_band_count_and_band_shape_edges(ctx, T, bank):
    n = R.TILE_N[T]
    fb = ctx.cached((bank, n), lambda: R.edge_bank(ctx.jsg, n, bank))
    F, hop = 37, n // 4                                    # a few dozen columns, no multiple of T: a partial last tile
    lds = not (bank == "edge" and n == 8192)                # (two full-width rows of 4097 weights: past 28 KB)
    claim(ctx, n, fb, F, T, lds)
    assert F % T != 0
    xs = ctx.cached(("edge audio", n), lambda: ctx.audio(1, 1, (F - 1) * hop + n, seed=5 * n))
    check_modes(ctx, n, fb, xs, hop, F, mix=0, W=F + 2, pos=F + 2 - 3, float64_bound=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# d. containment inside a tile
# ---------------------------------------------------------------------------------------------------------------------------------
def _contained(ctx, T):
    n = R.TILE_N[T]
    fb = ctx.cached(("edge", n), lambda: R.edge_bank(ctx.jsg, n, "edge"))
    F, hop = 21, n // 4
    claim(ctx, n, fb, F, T, n != 8192)
    xs = ctx.audio(1, 1, (F - 1) * hop + n, seed=7 * n)
    s = 8 * hop + 17                                        # in the frames 5 .. 8: they share tiles with the clean columns 4 and 9 (.. 11)
    hit = np.array([j * hop <= s < j * hop + n for j in range(F)])
    assert hit.nonzero()[0].tolist() == [5, 6, 7, 8] and 4 // T == 5 // T and 8 // T == 9 // T
    return n, fb, F, hop, xs, s, hit


@pytest.mark.parametrize("T", [4, 2])
def test_a_nan_sample_stays_in_its_columns_of_a_tile(ctx, T):
    n, fb, F, hop, xs, s, hit = _contained(ctx, T)
    bad = xs.copy()
    bad[0, 0, s] = np.nan
    live = fb.n_bins > 0
    assert live.any() and not live.all()
    for mode in ("linear", "exact"):
        clean, _ = run_band(ctx, n, fb, xs, hop, F, mix=0, mode=mode)
        base, _ = run_band(ctx, n, fb, bad, hop, F, mix=0, mode=mode)
        c, ok_c = split_output(clean, fb, F, F, 0, 0)
        g, ok_g = split_output(base, fb, F, F, 0, 0)
        assert ok_c and ok_g
        nan = np.isnan(g)
        assert nan[hit][:, live].all() and not nan[~hit].any() and not nan[:, ~live].any(), (mode, nan.sum(axis=1))
        assert not np.isnan(c).any()
        same = ~nan
        assert (g.view(np.uint32)[same] == c.view(np.uint32)[same]).all(), mode       # the tile neighbours 4 and 9 .. included: bit for bit


@pytest.mark.parametrize("T", [4, 2])
def test_an_infinite_power_column_follows_ieee_per_band(ctx, T):
    n, fb, F, hop, xs, s, hit = _contained(ctx, T)
    big = xs.copy()
    big[0, 0, s] = 1e25                                      # power ~ 1e50 w^2: +Inf in float32 wherever the window is not tiny
    clean, name = run_band(ctx, n, fb, xs, hop, F, mix=0, mode="linear")
    base, name2 = run_band(ctx, n, fb, big, hop, F, mix=0, mode="linear")
    assert name == name2
    c, ok_c = split_output(clean, fb, F, F, 0, 0)
    g, ok_g = split_output(base, fb, F, F, 0, 0)
    assert ok_c and ok_g
    P = power_plane(ctx, n, big, hop, F, 0, name)
    inf = np.isinf(P)
    assert not np.isnan(P).any() and inf[hit].any(axis=1).all() and not inf[~hit].any()
    want, _, _ = reference(ctx, P, fb)
    assert (np.isnan(g) == np.isnan(want)).all()
    fine = ~np.isnan(want)
    assert (g.view(np.uint32)[fine] == want.view(np.uint32)[fine]).all()
    # ... and said band by band: a zero weight over an Inf bin gives NaN, positive weights +Inf, bands away from the Inf bins do not move
    Wd = fb.matrix()
    k = np.arange(n // 2 + 1)[None, :]
    span = (k >= fb.first_bin[:, None]) & (k < (fb.first_bin + fb.n_bins)[:, None])               # [B][H]
    zero_over_inf = (inf.astype(np.float32) @ (span & (Wd == 0)).astype(np.float32).T) > 0         # [F][B]
    reaches = (inf.astype(np.float32) @ span.astype(np.float32).T) > 0
    positive = ((Wd > 0) | ~span).all(axis=1) & (fb.n_bins > 0)
    assert zero_over_inf.any() and (reaches & positive[None, :]).any() and (~reaches[hit]).any()
    assert np.isnan(g[zero_over_inf]).all()
    assert (g[reaches & positive[None, :]] == np.inf).all()
    assert (g.view(np.uint32)[~reaches] == c.view(np.uint32)[~reaches]).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# e. the same bits for every chunking
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,bank,lds", [c for c in R.FULL_CASES if c[0] >= 4096])
def test_chunking_does_not_change_bits(ctx, n, bank, lds):
    c = full_case(ctx, n, bank)
    fb, F, ch = c["fb"], c["F"], c["ch"]
    claim(ctx, n, fb, c["n_cols"], {4096: 4, 8192: 2}[n], lds)
    kw = dict(mix=PER_CHANNEL, mode="exact", W=c["W"], pos=c["pos"])
    whole, name = run_band(ctx, n, fb, c["xs"], c["hop"], F, **kw)
    assert split_output(whole, fb, F, c["W"], c["pos"], PER_CHANNEL)[1]
    for steps in (1, 33):                                    # scratch for one workgroup step of the STFT variant, and for 33
        cap = steps * STEP[name]                             # columns per row the scratch holds
        assert cap < c["k"] * F                              # not the whole call
        base, nm = run_band(ctx, n, fb, c["xs"], c["hop"], F, scratch_cols=ch * cap, **kw)
        assert nm == name
        assert (base.view(np.uint32) == whole.view(np.uint32)).all(), (name, steps)

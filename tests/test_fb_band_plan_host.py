"""jsg_fb_band_plan (include/jsg.h section 2b): how the band kernel of a filterbank chunk is launched -- tile columns, bank path, scratch pitch,
LDS bytes and grid, as the launcher itself takes them.  Host arithmetic only: CPU only."""
import ctypes

import pytest

SIZES = (512, 1024, 2048, 4096, 8192)
PITCH = {512: 288, 1024: 544, 2048: 1056, 4096: 2080, 8192: 4128}
TILE = {512: 8, 1024: 8, 2048: 8, 4096: 4, 8192: 2}
BANK_WORDS = 7168                 # 28 KB: the largest bank (3 words per band + the weights) staged in LDS
LDS_PER_CU = 160 * 1024


def want_grid(n_cols, T, n_cu, lds):
    return max(1, min(-(-n_cols // T), n_cu * min(8, LDS_PER_CU // lds)))


@pytest.mark.parametrize("n", SIZES)
def test_pitch_and_tile_columns(jsg, n):
    p = jsg.fb_band_plan(n, 40, 500, 100, 256)
    assert p["pw_pitch"] == PITCH[n] and p["tile_cols"] == TILE[n]
    assert p["pw_pitch"] >= n // 2 + 1 and p["pw_pitch"] % 32 == 0 and p["pw_pitch"] - 32 < n // 2 + 1     # whole 128-byte lines, no more
    assert set(p) == {"tile_cols", "bank_in_lds", "pw_pitch", "lds_bytes", "grid"}


@pytest.mark.parametrize("n", SIZES)
def test_bank_path_flips_between_7168_and_7169_words(jsg, n):
    for B in (1, 40, 128, 2048):
        for words, lds in ((BANK_WORDS, True), (BANK_WORDS + 1, False)):
            nnz = words - 3 * B
            p = jsg.fb_band_plan(n, B, nnz, 1000, 256)
            assert p["bank_in_lds"] is lds, (n, B, nnz)
            assert p["lds_bytes"] == 4 * TILE[n] * PITCH[n] + (4 * words if lds else 0)
    # the band descriptors alone past the limit: never in LDS, whatever the weights
    assert jsg.fb_band_plan(n, 2390, 0, 1000, 256)["bank_in_lds"] is False
    assert jsg.fb_band_plan(n, 2389, 1, 1000, 256)["bank_in_lds"] is True
    assert jsg.fb_band_plan(n, 1, (1 << 31) - 1, 1000, 256)["bank_in_lds"] is False


def test_lds_bytes_and_grid_over_a_sweep(jsg):
    seen = set()
    for n in SIZES:
        for B in (1, 2, 40, 128, 255, 256, 257, 1000, 2389, 2390, 4097, 8192):
            for nnz in (0, 1, 486, 4000, 7165 - 3 * min(B, 2000), 7168, 24600, 1 << 20):
                words = 3 * B + nnz
                lds = 4 * TILE[n] * PITCH[n] + (4 * words if words <= BANK_WORDS else 0)
                assert lds <= 64 * 1024
                for n_cols in (1, TILE[n] - 1, TILE[n], TILE[n] + 1, 1000, 7000, 40000, 1 << 28):
                    if n_cols < 1:
                        continue
                    for n_cu in (1, 64, 256, 304):
                        p = jsg.fb_band_plan(n, B, nnz, n_cols, n_cu)
                        assert p["lds_bytes"] == lds and p["bank_in_lds"] is (words <= BANK_WORDS)
                        assert p["grid"] == want_grid(n_cols, TILE[n], n_cu, lds), (n, B, nnz, n_cols, n_cu)
                        seen.add((p["tile_cols"], p["bank_in_lds"]))
    assert seen == {(T, lds) for T in (8, 4, 2) for lds in (True, False)}          # the six instantiations of the kernel


def test_grid_on_256_compute_units(jsg):
    """The device the suite runs on: a workgroup takes a second tile only past 1024 .. 2048 workgroups' worth of columns."""
    assert jsg.fb_band_plan(512, 40, 486, 1 << 28, 256)["grid"] == 2048          # 11.6 KB of LDS: eight workgroups per CU
    assert jsg.fb_band_plan(2048, 24, 24600, 1 << 28, 256)["grid"] == 1024       # a tile of 33 KB: four
    assert jsg.fb_band_plan(4096, 48, 3920, 1 << 28, 256)["grid"] == 768         # tile and bank, 49.5 KB: three
    assert jsg.fb_band_plan(1024, 64, 2000, 7000, 256)["grid"] == 875            # fewer tiles than the grid could hold: one tile each


def test_refusals(jsg):
    C = jsg.capi
    ok = dict(n=1024, n_bands=40, nnz=500, n_cols=100, n_cu=256)
    jsg.fb_band_plan(**ok)
    bad = [dict(n=0), dict(n=256), dict(n=1000), dict(n=1536), dict(n=16384), dict(n=-1024),
           dict(n_bands=0), dict(n_bands=-1), dict(n_bands=8193),
           dict(nnz=-1), dict(nnz=1 << 31),
           dict(n_cols=0), dict(n_cols=-5), dict(n_cols=(1 << 28) + 1),
           dict(n_cu=0), dict(n_cu=-1)]
    for change in bad:
        with pytest.raises(jsg.JsgError) as e:
            jsg.fb_band_plan(**{**ok, **change})
        assert e.value.code == C.JSG_ERR_INVALID, change
    for edge in (dict(n_bands=1), dict(n_bands=8192), dict(nnz=0), dict(nnz=(1 << 31) - 1), dict(n_cols=1), dict(n_cols=1 << 28), dict(n_cu=1)):
        jsg.fb_band_plan(**{**ok, **edge})


def test_null_outputs_and_declaration(jsg):
    C = jsg.capi
    lib = C.lib()
    assert "jsg_fb_band_plan" in C.SIGNATURES
    assert lib.jsg_fb_band_plan(2048, 128, 4000, 5000, 256, None, None, None, None, None) == C.JSG_OK
    grid = ctypes.c_int32(-1)
    assert lib.jsg_fb_band_plan(2048, 128, 4000, 5000, 256, None, None, None, None, ctypes.byref(grid)) == C.JSG_OK and grid.value == 625
    assert lib.jsg_fb_band_plan(2048, 128, 4000, 0, 256, None, None, None, None, ctypes.byref(grid)) == C.JSG_ERR_INVALID and grid.value == 625
    assert lib.jsg_abi_version() == 6

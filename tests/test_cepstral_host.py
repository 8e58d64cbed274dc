"""Cepstral coefficients and delta features, host side (include/jsg.h section 2k): every refusal of the two launches and the two
builders in its stated order (all decided without a device), the projection's plan swept over the corners of the accepted range, the
tables and weights against the float64 formulas, the symbols, the exports, the struct layouts and the kernels' notes.  CPU only."""
import ctypes as C
import inspect
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import cepstral_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# never dereferenced: every call below is refused, or only planned
IN, TABLE, OUT, WEIGHTS = (i << 44 for i in range(1, 5))
LDS_MAX = 163840
BAD = -2


def mfcc_args(jsg, **kw):
    a = dict(in_=IN, frame_pitch=128, row_pitch=40 * 128, rows=2, n_in=128, n_frames=40, table=TABLE, n_out=20, out=OUT, out_frame_pitch=20,
             out_row_pitch=40 * 20, chunk_frames=0)
    a.update(kw)
    return jsg.capi.MfccArgs(**a)


def delta_args(jsg, **kw):
    a = dict(in_=IN, frame_pitch=20, row_pitch=40 * 20, rows=2, n_coeffs=20, n_frames=40, weights=WEIGHTS, width=9, mode=0, out=OUT,
             out_frame_pitch=20, out_row_pitch=40 * 20)
    a.update(kw)
    return jsg.capi.DeltaArgs(**a)


def plan(jsg, a):
    name, frames, lds = C.create_string_buffer(32), C.c_int32(-1), C.c_int32(-1)
    rc = jsg.capi.lib().jsg_mfcc_plan(C.byref(a), name, 32, C.byref(frames), C.byref(lds))
    return rc, name.value.decode(), frames.value, lds.value


# in the order of the header: a call with two defects is refused for the earlier one
MFCC_REFUSED = [
    ("null in", dict(in_=None), "null in"),
    ("null table", dict(table=None), "null table"),
    ("null out", dict(out=None), "null out"),
    ("misaligned in", dict(in_=IN + 2), "pointers must be 4-byte aligned"),
    ("misaligned table", dict(table=TABLE + 1), "pointers must be 4-byte aligned"),
    ("misaligned out", dict(out=OUT + 3), "pointers must be 4-byte aligned"),
    ("no rows", dict(rows=0), "rows must be in 1..65535"),
    ("65536 rows", dict(rows=65536), "rows must be in 1..65535"),
    ("n_in 0", dict(n_in=0), "n_in must be in 1..4096"),
    ("n_in 4097", dict(n_in=4097, frame_pitch=4097, row_pitch=40 * 4097, n_out=1), "n_in must be in 1..4096"),
    ("n_out 0", dict(n_out=0), "n_out must be in 1..4096"),
    ("n_out 4097", dict(n_out=4097, n_in=1, out_frame_pitch=4097, out_row_pitch=40 * 4097), "n_out must be in 1..4096"),
    ("table of 32769", dict(n_out=257, out_frame_pitch=257, out_row_pitch=40 * 257), "n_in*n_out must be at most 32768"),
    ("no frames", dict(n_frames=0), "n_frames must be in 1..2^31-1"),
    ("2^31 frames", dict(n_frames=2 ** 31, row_pitch=2 ** 40, out_row_pitch=2 ** 40), "n_frames must be in 1..2^31-1"),
    ("chunk -1", dict(chunk_frames=-1), "chunk_frames must be 0 or in 1..65536"),
    ("chunk 65537", dict(chunk_frames=65537), "chunk_frames must be 0 or in 1..65536"),
    ("frame_pitch", dict(frame_pitch=127), "frame_pitch smaller than n_in"),
    ("row_pitch", dict(row_pitch=40 * 128 - 1), "row_pitch smaller than (n_frames-1)*frame_pitch + n_in"),
    ("out_frame_pitch", dict(out_frame_pitch=19), "out_frame_pitch smaller than n_out"),
    ("out_row_pitch", dict(out_row_pitch=40 * 20 - 1), "out_row_pitch smaller than (n_frames-1)*out_frame_pitch + n_out"),
    ("out inside in", dict(out=IN + 4 * 100), "out overlaps in"),
    ("out ends in in", dict(out=IN - 4 * 2 * 40 * 20 + 4), "out overlaps in"),
    ("out ends in the table", dict(out=TABLE - 4 * 2 * 40 * 20 + 4), "out overlaps table"),
    ("out starts in the table", dict(out=TABLE + 4 * (128 * 20 - 1)), "out overlaps table"),
]
DELTA_REFUSED = [
    ("null in", dict(in_=None), "null in"),
    ("null weights", dict(weights=None), "null weights"),
    ("null out", dict(out=None), "null out"),
    ("misaligned weights", dict(weights=WEIGHTS + 2), "pointers must be 4-byte aligned"),
    ("misaligned out", dict(out=OUT + 1), "pointers must be 4-byte aligned"),
    ("no rows", dict(rows=0), "rows must be in 1..65535"),
    ("65536 rows", dict(rows=65536), "rows must be in 1..65535"),
    ("no coefficients", dict(n_coeffs=0), "n_coeffs must be in 1..65536"),
    ("65537 coefficients", dict(n_coeffs=65537, frame_pitch=65537, row_pitch=40 * 65537, out_frame_pitch=65537, out_row_pitch=40 * 65537), "n_coeffs must be in 1..65536"),
    ("no frames", dict(n_frames=0), "n_frames must be in 1..2^31-1"),
    ("2^31 frames", dict(n_frames=2 ** 31, row_pitch=2 ** 40, out_row_pitch=2 ** 40), "n_frames must be in 1..2^31-1"),
    ("width 1", dict(width=1), "width must be odd and in 3..255"),
    ("width 8", dict(width=8), "width must be odd and in 3..255"),
    ("width 257", dict(width=257, n_frames=300, row_pitch=300 * 20, out_row_pitch=300 * 20), "width must be odd and in 3..255"),
    ("mode 2", dict(mode=2), "mode must be 0 (interp) or 1 (nearest)"),
    ("mode -1", dict(mode=-1), "mode must be 0 (interp) or 1 (nearest)"),
    ("too few frames to interpolate", dict(n_frames=8, row_pitch=8 * 20, out_row_pitch=8 * 20), "n_frames smaller than width (interp)"),
    ("frame_pitch", dict(frame_pitch=19), "frame_pitch smaller than n_coeffs"),
    ("row_pitch", dict(row_pitch=40 * 20 - 1), "row_pitch smaller than (n_frames-1)*frame_pitch + n_coeffs"),
    ("out_frame_pitch", dict(out_frame_pitch=19), "out_frame_pitch smaller than n_coeffs"),
    ("out_row_pitch", dict(out_row_pitch=40 * 20 - 1), "out_row_pitch smaller than (n_frames-1)*out_frame_pitch + n_coeffs"),
    ("out inside in", dict(out=IN + 4 * 100), "out overlaps in"),
    ("out ends in the weights", dict(out=WEIGHTS - 4 * 2 * 40 * 20 + 4), "out overlaps weights"),
]
FAMILIES = {
    "mfcc": (MFCC_REFUSED, mfcc_args, (("jsg_mfcc_launch", lambda lib, a, buf: lib.jsg_mfcc_launch(C.byref(a), None)),
                                       ("jsg_mfcc_plan", lambda lib, a, buf: lib.jsg_mfcc_plan(C.byref(a), None, 0, None, None)),
                                       ("jsg_mfcc_kernel_name", lambda lib, a, buf: lib.jsg_mfcc_kernel_name(C.byref(a), buf, 32)))),
    "delta": (DELTA_REFUSED, delta_args, (("jsg_delta_launch", lambda lib, a, buf: lib.jsg_delta_launch(C.byref(a), None)),)),
}
CASES = [(family, i) for family, (refused, _, _) in FAMILIES.items() for i in range(len(refused))]


@pytest.mark.parametrize("family,i", CASES, ids=[f"{family}: {FAMILIES[family][0][i][0]}" for family, i in CASES])
def test_refusals_in_their_order(jsg, family, i):
    lib = jsg.capi.lib()
    refused, make, calls = FAMILIES[family]
    _, change, message = refused[i]
    a = make(jsg, **change)
    buf = C.create_string_buffer(32)
    for who, call in calls:
        assert call(lib, a, buf) == BAD and lib.jsg_last_error(None) == f"{who}: {message}".encode()
    # with any later defect on top, the earlier one is still the one reported
    who, call = calls[0]
    for _, later, later_message in refused[i + 1:]:
        if later_message == message or set(later) & set(change):
            continue
        both = make(jsg, **dict(later, **change))
        assert call(lib, both, buf) == BAD
        assert lib.jsg_last_error(None) == f"{who}: {message}".encode(), (refused[i][0], later)


def test_null_arguments_and_what_one_row_ignores(jsg):
    lib = jsg.capi.lib()
    assert lib.jsg_mfcc_launch(None, None) == BAD and lib.jsg_last_error(None) == b"jsg_mfcc_launch: null argument"
    assert lib.jsg_delta_launch(None, None) == BAD and lib.jsg_last_error(None) == b"jsg_delta_launch: null argument"
    assert lib.jsg_mfcc_plan(None, None, 0, None, None) == BAD
    buf = C.create_string_buffer(32)
    a = mfcc_args(jsg)
    assert lib.jsg_mfcc_kernel_name(C.byref(a), None, 32) == BAD and lib.jsg_mfcc_kernel_name(C.byref(a), buf, 23) == BAD
    assert lib.jsg_mfcc_plan(C.byref(a), buf, 23, None, None) == BAD
    # one row: the row pitches are not looked at
    assert plan(jsg, mfcc_args(jsg, rows=1, row_pitch=0, out_row_pitch=0))[0] == 0
    # an output next to an input, not inside it
    assert plan(jsg, mfcc_args(jsg, out=IN + 4 * 2 * 40 * 128))[0] == 0
    assert plan(jsg, mfcc_args(jsg, out=TABLE - 4 * 2 * 40 * 20))[0] == 0
    assert plan(jsg, mfcc_args(jsg, out=TABLE + 4 * 128 * 20))[0] == 0
    # the table limit itself, and both ranges at their ends
    assert plan(jsg, mfcc_args(jsg, n_out=256, out_frame_pitch=256, out_row_pitch=40 * 256))[0] == 0
    assert plan(jsg, mfcc_args(jsg, n_in=4096, frame_pitch=4096, row_pitch=40 * 4096, n_out=8))[0] == 0
    assert plan(jsg, mfcc_args(jsg, n_in=8, frame_pitch=8, row_pitch=40 * 8, n_out=4096, out_frame_pitch=4096, out_row_pitch=40 * 4096))[0] == 0


def test_no_device_comes_after_the_refusals(jsg):
    lib = jsg.capi.lib()
    if lib.jsg_device_count() > 0:
        pytest.skip("a GPU is present")
    for make, call in ((mfcc_args, lib.jsg_mfcc_launch), (delta_args, lib.jsg_delta_launch)):
        assert call(C.byref(make(jsg)), None) == jsg.capi.JSG_ERR_NO_DEVICE
        assert call(C.byref(make(jsg, rows=0)), None) == BAD
    assert lib.jsg_delta_launch(C.byref(delta_args(jsg, mode=1, n_frames=1, rows=1)), None) == jsg.capi.JSG_ERR_NO_DEVICE


def block_of(M):
    return next((mb for mb in (4, 5, 8, 10, 16) if 4 * mb >= M), 16)


CORNERS = (1, 2, 3, 4, 5, 13, 16, 17, 20, 21, 32, 33, 40, 41, 64, 128, 256, 257, 4096)


def test_plan_over_the_corners(jsg):
    seen, fewer = set(), 0
    for B, M in itertools.product(CORNERS, CORNERS):
        if B * M > 32768:
            continue
        for chunk, frames in itertools.product((0, 1, 3, 64, 65536), (1, 2, 63, 64, 65, 2 ** 31 - 1)):
            a = mfcc_args(jsg, rows=1, n_in=B, n_out=M, frame_pitch=B, out_frame_pitch=M, n_frames=frames, chunk_frames=chunk)
            rc, name, F, lds = plan(jsg, a)
            assert rc == 0, (B, M, chunk, frames)
            seen.add(name)
            assert name == f"mfcc_block{block_of(M)}"
            per = (B | 1) + (M | 1)
            want = max(1, min(64, frames, chunk or 64, (LDS_MAX // 4 - B * M) // per))
            assert F == want and lds == 4 * (B * M + F * per) and 0 < lds <= LDS_MAX, (B, M, chunk, frames, F, lds)
            fewer += want < min(64, frames, chunk or 64)
            assert plan(jsg, a) == (rc, name, F, lds)              # stable
    assert seen == {"mfcc_block4", "mfcc_block5", "mfcc_block8", "mfcc_block10", "mfcc_block16"} and fewer > 0
    # the default at the usual size: 20 coefficients are four blocks of 5, one per wave; 64 frames of 128 bands and the table are 48 KB
    assert plan(jsg, mfcc_args(jsg, n_frames=4096, row_pitch=4096 * 128, out_row_pitch=4096 * 20))[1:] == ("mfcc_block5", 64, 4 * (2560 + 64 * 150))
    # 128 x 256 at the table limit: the 160 KiB hold 21 frames next to the table
    assert plan(jsg, mfcc_args(jsg, n_out=256, out_frame_pitch=256, out_row_pitch=40 * 256))[1:] == ("mfcc_block16", 21, 4 * (32768 + 21 * 386))
    assert jsg.capi.MFCC_MAX_TABLE == 32768


TABLES = [(128, 20), (128, 128), (40, 13), (1, 1), (2, 2), (257, 20), (4096, 8), (181, 181)]


@pytest.mark.parametrize("B,M", TABLES)
def test_tables_against_the_formula(jsg, B, M):
    for norm, lifter, inverse in itertools.product(("ortho", "none"), (0.0, 22.0), (False, True)):
        got = jsg.mfcc_table(B, M, norm, lifter, inverse)
        want = cr.dct_table64(B, M, norm, lifter, inverse)
        assert got.dtype == np.float32 and got.shape == ((B, M) if inverse else (M, B))
        # the double result is far inside half a float32 ulp of the exact value: only a rounding-boundary flip of one ulp can differ
        assert np.abs(got.astype(np.float64) - want.astype(np.float32).astype(np.float64)).max() <= 2.0 ** -23 * np.abs(want).max(), (norm, lifter, inverse)
    assert np.array_equal(jsg.mfcc_table(B, M, None), jsg.mfcc_table(B, M, "none"))
    # cos(pi/2) is an exact zero of the formula: coefficient m, band b with m (2b + 1) = B (mod 2B)
    D = jsg.mfcc_table(B, M)
    m, b = np.arange(M)[:, None], np.arange(B)[None, :]
    zero = (m * (2 * b + 1)) % (2 * B) == B
    assert (D[zero] == 0).all() and (D[~zero] != 0).all()


def test_forward_times_inverse_is_the_identity(jsg):
    for B in (1, 2, 13, 128):
        fwd, inv = jsg.mfcc_table(B, B).astype(np.float64), jsg.mfcc_table(B, B, inverse=True).astype(np.float64)
        # both tables carry one rounding per element (u relative); a product element sums B such terms
        bound = (B + 2) * cr.U * (np.abs(inv) @ np.abs(fwd))
        assert (np.abs(inv @ fwd - np.eye(B)) <= 2 * bound).all()


def test_table_refusals(jsg):
    lib = jsg.capi.lib()
    out = np.zeros(64, np.float32)
    who = b"jsg_mfcc_table_build: "
    for args, message in (((0, 1, 1, 0.0, 0), "n_bands must be in 1..4096"), ((4097, 1, 1, 0.0, 0), "n_bands must be in 1..4096"),
                          ((8, 0, 1, 0.0, 0), "n_coeffs must be in 1..4096"), ((8, 4097, 1, 0.0, 0), "n_coeffs must be in 1..4096"),
                          ((8, 9, 1, 0.0, 0), "n_coeffs must be at most n_bands"), ((257, 128, 1, 0.0, 0), "n_bands*n_coeffs must be at most 32768"),
                          ((8, 4, 2, 0.0, 0), "norm must be 0 (none) or 1 (ortho)"), ((8, 4, -1, 0.0, 0), "norm must be 0 (none) or 1 (ortho)"),
                          ((8, 4, 1, 0.0, 2), "inverse must be 0 or 1"), ((8, 4, 1, -1.0, 0), "lifter must be finite and >= 0"),
                          ((8, 4, 1, float("nan"), 0), "lifter must be finite and >= 0"), ((8, 4, 1, float("inf"), 1), "lifter must be finite and >= 0"),
                          ((8, 4, 1, 2.0, 1), "the lifter is zero at a coefficient: no inverse"),        # 1 + sin(3 pi / 2) at m = 2
                          # in the stated order: the earlier defect is the one reported
                          ((0, 0, 7, -1.0, 7), "n_bands must be in 1..4096"), ((8, 9, 7, -1.0, 7), "n_coeffs must be at most n_bands"),
                          ((8, 4, 7, -1.0, 7), "norm must be 0 (none) or 1 (ortho)"), ((8, 4, 1, -1.0, 7), "inverse must be 0 or 1")):
        assert lib.jsg_mfcc_table_build(*args, out.ctypes.data) == BAD and lib.jsg_last_error(None) == who + message.encode(), args
    assert lib.jsg_mfcc_table_build(8, 4, 1, 0.0, 0, None) == BAD and lib.jsg_last_error(None) == who + b"null out"
    assert lib.jsg_mfcc_table_build(8, 4, 1, 2.0, 0, out.ctypes.data) == 0          # forward: a zero lifter value is fine
    with pytest.raises(jsg.JsgError):
        jsg.mfcc_table(8, 4, "slaney")


@pytest.mark.parametrize("width,order", [(3, 1), (3, 2), (5, 2), (9, 1), (9, 2), (9, 3), (9, 4), (255, 1), (255, 2), (255, 3), (255, 4)])
def test_weights_against_the_formula(jsg, width, order):
    got = jsg.delta_weights(width, order)
    want = cr.delta_weights64(width, order)
    assert got.dtype == np.float32 and got.shape == (width,)
    assert np.abs(got.astype(np.float64) - want.astype(np.float32).astype(np.float64)).max() <= 2.0 ** -23 * np.abs(want).max()
    assert cr.same(got, (np.float32((-1) ** order) * got[::-1]) + np.float32(0))    # exactly (anti)symmetric
    if order % 2:
        assert got[width // 2] == 0 and not np.signbit(got[width // 2])             # the centre weight of an odd order: an exact +0
    else:
        assert got[width // 2] != 0
    if (width, order) == (9, 1):
        assert cr.same(got, ((np.arange(9) - 4) / 60.0).astype(np.float32))


def test_weight_refusals(jsg):
    lib = jsg.capi.lib()
    out = np.zeros(256, np.float32)
    who = b"jsg_delta_weights_build: "
    for args, message in (((1, 1), "width must be odd and in 3..255"), ((4, 1), "width must be odd and in 3..255"), ((257, 1), "width must be odd and in 3..255"),
                          ((9, 0), "order must be in 1..4 and below width"), ((9, 5), "order must be in 1..4 and below width"),
                          ((3, 3), "order must be in 1..4 and below width"), ((4, 0), "width must be odd and in 3..255")):
        assert lib.jsg_delta_weights_build(*args, out.ctypes.data) == BAD and lib.jsg_last_error(None) == who + message.encode(), args
    assert lib.jsg_delta_weights_build(9, 1, None) == BAD and lib.jsg_last_error(None) == who + b"null out"
    with pytest.raises(jsg.JsgError):
        jsg.delta_weights(8)


def test_symbols_and_exports(jsg):
    lib = jsg.capi.lib()
    for name in ("jsg_mfcc_launch", "jsg_mfcc_plan", "jsg_mfcc_kernel_name", "jsg_mfcc_table_build", "jsg_delta_weights_build", "jsg_delta_launch"):
        assert hasattr(lib, name) and name in jsg.capi.SIGNATURES
    for name in ("mfcc_table", "mfcc_launch", "mfcc_plan", "mfcc_kernel_name", "delta_weights", "delta_launch", "mfcc", "mfcc_to_mel_db", "delta", "mfcc_audio"):
        assert callable(getattr(jsg, name)) and name in jsg.__all__
    hdr = open(os.path.join(ROOT, "include", "jsg.h")).read()
    assert "2k. Cepstral coefficients and delta features" in hdr and "section 2k" in hdr
    assert "#define JSG_ABI_VERSION 6 " in hdr and lib.jsg_abi_version() == 6
    for define, value in (("JSG_MFCC_MAX_BANDS", jsg.capi.MFCC_MAX_BANDS), ("JSG_MFCC_MAX_COEFFS", jsg.capi.MFCC_MAX_COEFFS), ("JSG_MFCC_MAX_TABLE", jsg.capi.MFCC_MAX_TABLE),
                          ("JSG_DCT_NORM_NONE", jsg.capi.DCT_NORM_NONE), ("JSG_DCT_NORM_ORTHO", jsg.capi.DCT_NORM_ORTHO),
                          ("JSG_DELTA_MAX_WIDTH", jsg.capi.DELTA_MAX_WIDTH), ("JSG_DELTA_MAX_ORDER", jsg.capi.DELTA_MAX_ORDER),
                          ("JSG_DELTA_MAX_COEFFS", jsg.capi.DELTA_MAX_COEFFS), ("JSG_DELTA_EDGE_INTERP", jsg.capi.DELTA_EDGE_INTERP),
                          ("JSG_DELTA_EDGE_NEAREST", jsg.capi.DELTA_EDGE_NEAREST)):
        assert re.search(rf"#define {define} {value}\b", hdr), define
    assert (jsg.capi.MFCC_MAX_BANDS, jsg.capi.MFCC_MAX_COEFFS, jsg.capi.MFCC_MAX_TABLE, jsg.capi.DELTA_MAX_WIDTH, jsg.capi.DELTA_MAX_ORDER) == (4096, 4096, 32768, 255, 4)
    sig = inspect.signature(jsg.mfcc)
    assert list(sig.parameters) == ["S", "n_mfcc", "norm", "lifter"] and [p.default for p in list(sig.parameters.values())[1:]] == [20, "ortho", 0.0]
    sig = inspect.signature(jsg.delta)
    assert list(sig.parameters) == ["X", "width", "order", "mode"] and [p.default for p in list(sig.parameters.values())[1:]] == [9, 1, "interp"]
    sig = inspect.signature(jsg.mfcc_audio)
    assert list(sig.parameters) == ["x", "sr", "n_mfcc", "n_fft", "hop", "n_mels", "fmin", "fmax", "lifter"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [20, 2048, 512, 128, 0.0, None, 0.0]
    sig = inspect.signature(jsg.mfcc_to_mel_db)
    assert list(sig.parameters) == ["C", "n_mels", "norm", "lifter"] and [p.default for p in list(sig.parameters.values())[1:]] == [128, "ortho", 0.0]
    sig = inspect.signature(jsg.mfcc_table)
    assert list(sig.parameters) == ["n_bands", "n_coeffs", "norm", "lifter", "inverse"] and [p.default for p in list(sig.parameters.values())[1:]] == [20, "ortho", 0.0, False]
    assert [p.default for p in inspect.signature(jsg.delta_weights).parameters.values()] == [9, 1]
    for text in (jsg.mfcc.__doc__, jsg.delta.__doc__, jsg.mfcc_audio.__doc__, jsg.mfcc_to_mel_db.__doc__):
        text = " ".join(text.split())
        assert "axis -2" in text and "not measured" in text


@pytest.mark.parametrize("struct,cls", [("jsg_mfcc_args", "MfccArgs"), ("jsg_delta_args", "DeltaArgs")])
def test_struct_layout_matches_the_header(jsg, tmp_path, struct, cls):
    import shutil
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsg.h")).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*$", piece).group(1) for decl in body.split(";") if decl.strip() for piece in decl.split(",")]
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "jsg.h"', "int main(void) {", f'    printf("%zu\\n", sizeof({struct}));']
    lines += [f'    printf("{f} %zu %zu\\n", offsetof({struct}, {f}), sizeof((({struct}*)0)->{f}));' for f in names]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)])
    out = subprocess.check_output([str(tmp_path / "layout")], text=True).split("\n")
    cls = getattr(jsg.capi, cls)
    assert out[0] == str(C.sizeof(cls))
    assert [f for f, _ in cls._fields_] == ["in_" if f == "in" else f for f in names]
    for (f, _), c_name, line in zip(cls._fields_, names, out[1:]):
        assert line == f"{c_name} {getattr(cls, f).offset} {getattr(cls, f).size}"


def test_kernel_notes(jsg, tmp_path):
    """No private segment (no scratch, no spills) in any kernel of the unit; the projection's LDS is all dynamic (what jsg_mfcc_plan
    states), the delta kernel holds its 256 weight slots statically; the unit's kernels are the five the plan names and the delta one."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    obj = os.path.join(ROOT, "jadespectrogram_amd", "build", "jsg_cepstral.o")
    if not os.path.exists(obj):
        from jadespectrogram_amd import _build
        _build.build_lib()
    co = kernel_regs.code_object(obj, str(tmp_path))
    notes = subprocess.check_output([os.path.join(kernel_regs.LLVM, "llvm-readelf"), "--notes", co]).decode()
    found = {}
    for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
        g = lambda k: re.search(rf"\.{k}:\s+(\S+)", blk).group(1)
        found[g("name")] = (int(g("private_segment_fixed_size")), int(g("group_segment_fixed_size")), int(g("vgpr_spill_count")), int(g("sgpr_spill_count")))
    assert len(found) == 6 and sum("mfcc_kernel" in k for k in found) == 5 and sum("delta_kernel" in k for k in found) == 1
    for name, (private, lds, vspill, sspill) in found.items():
        assert private == 0 and vspill == 0 and sspill == 0, name
        assert lds == (1024 if "delta_kernel" in name else 0), name

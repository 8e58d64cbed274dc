"""Sections 6 to 8 of the companion library, host side (include/jsgx.h): every refusal of the neighbour search, of the recurrence plane and
of nn_filter in its stated order (all decided without a device), the scratch formula and the plan on both sides of every boundary (the
strip rows, the automatic split against the compute units, k = 256 | 257, the LDS limit), the struct layouts against a C program, the
Python names, the kernels' notes, and the host entry points from a stand-alone C++ program under the address and undefined-behaviour
sanitizers.  CPU only."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# never dereferenced: every call below is refused, sized or planned
X, Y, INDEX, DIST, BW, OUT, WEIGHTS, SCRATCH = (i << 44 for i in range(1, 9))
BAD = -2


@pytest.fixture(scope="module")
def capix(jsg):
    if not os.path.exists(jsg.capix.LIB_PATH):
        from jadespectrogram_amd import _build
        _build.build_lib()
    jsg.capix.lib()
    return jsg.capix


def knn_args(capix, **kw):      # 3 pairs of 100 x 300 frames of 20 features, k = 10
    a = dict(x=X, x_frame_pitch=24, x_pair_pitch=2400, y=Y, y_frame_pitch=20, y_pair_pitch=6000, pairs=3, n_features=20, n=100, m=300, metric=1, k=10, width=1,
             split=0, nn_index=INDEX, index_pitch=12, index_pair_pitch=1200, nn_dist=DIST, dist_pitch=10, dist_pair_pitch=1000)
    a.update(kw)
    return capix.KnnArgs(**a)


def rec_args(capix, **kw):
    a = dict(nn_index=INDEX, index_pitch=12, index_pair_pitch=1200, nn_dist=DIST, dist_pitch=10, dist_pair_pitch=1000, bandwidth=BW, pairs=3, n=100, m=100, k=10,
             mode=2, sym=1, diag=1, reserved0=0, out=OUT, out_pitch=104, out_pair_pitch=10400)
    a.update(kw)
    return capix.RecurrenceArgs(**a)


def nnf_args(capix, **kw):
    a = dict(s=X, s_frame_pitch=24, s_pair_pitch=2400, nn_index=INDEX, index_pitch=12, index_pair_pitch=1200, weights=WEIGHTS, weights_pitch=10,
             weights_pair_pitch=1000, pairs=3, n=100, n_features=20, k=10, out=OUT, out_frame_pitch=20, out_pair_pitch=2000)
    a.update(kw)
    return capix.NnFilterArgs(**a)


# in the order of the header: a call with two defects is refused for the earlier one
KNN_REFUSED = [
    ("null x", dict(x=None), "null x"),
    ("null y", dict(y=None), "null y"),
    ("null nn_index", dict(nn_index=None), "null nn_index"),
    ("null nn_dist", dict(nn_dist=None), "null nn_dist"),
    ("misaligned x", dict(x=X + 2), "pointers must be 4-byte aligned"),
    ("misaligned nn_dist", dict(nn_dist=DIST + 1), "pointers must be 4-byte aligned"),
    ("no pairs", dict(pairs=0), "pairs must be in 1..65535"),
    ("65536 pairs", dict(pairs=65536), "pairs must be in 1..65535"),
    ("no features", dict(n_features=0), "n_features must be in 1..1024"),
    ("1025 features", dict(n_features=1025, x_frame_pitch=1025, y_frame_pitch=1025, x_pair_pitch=0, y_pair_pitch=0), "n_features must be in 1..1024"),
    ("n 0", dict(n=0), "n must be in 1..65536"),
    ("n 65537", dict(n=65537, x_pair_pitch=0, index_pair_pitch=1 << 30, dist_pair_pitch=1 << 30), "n must be in 1..65536"),
    ("m 0", dict(m=0), "m must be in 1..65536"),
    ("m 65537", dict(m=65537, y_pair_pitch=0), "m must be in 1..65536"),
    ("metric 3", dict(metric=3), "metric must be in 0..2"),
    ("metric -1", dict(metric=-1), "metric must be in 0..2"),
    ("k 0", dict(k=0), "k must be in 1..256"),
    ("k 257", dict(k=257, index_pitch=257, dist_pitch=257, index_pair_pitch=25700, dist_pair_pitch=25700), "k must be in 1..256"),
    ("width -1", dict(width=-1), "width must be >= 0"),
    ("split -1", dict(split=-1), "split must be in 0..16"),
    ("split 17", dict(split=17), "split must be in 0..16"),
    ("x_frame_pitch", dict(x_frame_pitch=19), "x_frame_pitch smaller than n_features"),
    ("y_frame_pitch", dict(y_frame_pitch=19), "y_frame_pitch smaller than n_features"),
    ("x_pair_pitch", dict(x_pair_pitch=99 * 24 + 19), "x_pair_pitch does not cover a sequence"),
    ("y_pair_pitch", dict(y_pair_pitch=299 * 20 + 19), "y_pair_pitch does not cover a sequence"),
    ("index_pitch", dict(index_pitch=9), "index_pitch smaller than k"),
    ("index_pair_pitch", dict(index_pair_pitch=99 * 12 + 9), "index_pair_pitch does not cover a plane"),
    ("dist_pitch", dict(dist_pitch=9), "dist_pitch smaller than k"),
    ("dist_pair_pitch", dict(dist_pair_pitch=999), "dist_pair_pitch does not cover a plane"),
    ("nn_index ends in x", dict(nn_index=X - 4 * (2 * 1200 + 99 * 12 + 10) + 4), "an output overlaps x"),
    ("nn_dist inside x", dict(nn_dist=X + 4 * 1000), "an output overlaps x"),
    ("nn_index inside y", dict(nn_index=Y + 4 * (2 * 6000 + 299 * 20 + 19)), "an output overlaps y"),
    ("nn_dist ends in nn_index", dict(nn_dist=INDEX - 4 * 3000 + 4), "nn_index overlaps nn_dist"),
]
KNN_CALLS = (("jsgx_knn_launch", lambda lib, a: lib.jsgx_knn_launch(C.byref(a), SCRATCH, 1 << 50, None)),
             ("jsgx_knn_scratch_bytes", lambda lib, a: lib.jsgx_knn_scratch_bytes(C.byref(a))),
             ("jsgx_knn_plan", lambda lib, a: lib.jsgx_knn_plan(C.byref(a), 256, None, 0, None, None, None, None)))

REC_REFUSED = [
    ("null nn_index", dict(nn_index=None), "null nn_index"),
    ("null out", dict(out=None), "null out"),
    ("misaligned bandwidth", dict(bandwidth=BW + 2), "pointers must be 4-byte aligned"),
    ("no pairs", dict(pairs=0), "pairs must be in 1..65535"),
    ("n 65537", dict(n=65537, m=65537, out_pitch=1 << 17, out_pair_pitch=1 << 40, index_pair_pitch=1 << 30, dist_pair_pitch=1 << 30), "n must be in 1..65536"),
    ("m 0", dict(m=0), "m must be in 1..65536"),
    ("k 257", dict(k=257, index_pitch=257, dist_pitch=257, index_pair_pitch=25700, dist_pair_pitch=25700), "k must be in 1..256"),
    ("mode 3", dict(mode=3), "mode must be in 0..2"),
    ("sym 2", dict(sym=2), "sym must be 0 or 1"),
    ("diag -1", dict(diag=-1), "diag must be 0 or 1"),
    ("reserved0", dict(reserved0=7), "reserved0 must be 0"),
    ("sym with n != m", dict(m=101), "sym needs n == m"),
    ("null nn_dist", dict(nn_dist=None), "null nn_dist"),
    ("null bandwidth", dict(bandwidth=None), "null bandwidth"),
    ("index_pitch", dict(index_pitch=9), "index_pitch smaller than k"),
    ("index_pair_pitch", dict(index_pair_pitch=99 * 12 + 9), "index_pair_pitch does not cover a plane"),
    ("dist_pitch", dict(dist_pitch=9), "dist_pitch smaller than k"),
    ("dist_pair_pitch", dict(dist_pair_pitch=999), "dist_pair_pitch does not cover a plane"),
    ("out_pitch", dict(out_pitch=99), "out_pitch smaller than m"),
    ("out_pair_pitch", dict(out_pair_pitch=99 * 104 + 99), "out_pair_pitch does not cover a plane"),
    ("out ends in nn_index", dict(out=INDEX - 4 * (2 * 10400 + 99 * 104 + 100) + 4), "out overlaps nn_index"),
    ("out inside nn_dist", dict(out=DIST + 4 * 2999), "out overlaps nn_dist"),
    ("out ends in bandwidth", dict(out=BW - 4 * (2 * 10400 + 99 * 104 + 100) + 4 * 3), "out overlaps bandwidth"),
]
NNF_REFUSED = [
    ("null s", dict(s=None), "null s"),
    ("null nn_index", dict(nn_index=None), "null nn_index"),
    ("null out", dict(out=None), "null out"),
    ("misaligned weights", dict(weights=WEIGHTS + 1), "pointers must be 4-byte aligned"),
    ("65536 pairs", dict(pairs=65536), "pairs must be in 1..65535"),
    ("n 0", dict(n=0), "n must be in 1..65536"),
    ("65537 features", dict(n_features=65537, s_frame_pitch=1 << 17, out_frame_pitch=1 << 17, s_pair_pitch=1 << 30, out_pair_pitch=1 << 30), "n_features must be in 1..65536"),
    ("k 0", dict(k=0), "k must be in 1..256"),
    ("s_frame_pitch", dict(s_frame_pitch=19), "s_frame_pitch smaller than n_features"),
    ("s_pair_pitch", dict(s_pair_pitch=99 * 24 + 19), "s_pair_pitch does not cover a plane"),
    ("index_pitch", dict(index_pitch=9), "index_pitch smaller than k"),
    ("index_pair_pitch", dict(index_pair_pitch=99 * 12 + 9), "index_pair_pitch does not cover a plane"),
    ("weights_pitch", dict(weights_pitch=9), "weights_pitch smaller than k"),
    ("weights_pair_pitch", dict(weights_pair_pitch=999), "weights_pair_pitch does not cover a plane"),
    ("out_frame_pitch", dict(out_frame_pitch=19), "out_frame_pitch smaller than n_features"),
    ("out_pair_pitch", dict(out_pair_pitch=1999), "out_pair_pitch does not cover a plane"),
    ("out inside s", dict(out=X + 4 * (2 * 2400 + 99 * 24 + 19)), "out overlaps s"),
    ("out ends in nn_index", dict(out=INDEX - 4 * 6000 + 4), "out overlaps nn_index"),
    ("out inside weights", dict(out=WEIGHTS + 4 * 2999), "out overlaps weights"),
]


def in_order(lib, make, refused, i, calls):
    _, change, message = refused[i]
    a = make(**change)
    for who, call in calls:
        assert call(lib, a) == BAD and lib.jsgx_last_error() == f"{who}: {message}".encode(), (who, refused[i][0], lib.jsgx_last_error())
    # with any later defect on top, the earlier one is still the one reported
    who, call = calls[0]
    for _, later, later_message in refused[i + 1:]:
        if later_message == message or set(later) & set(change):
            continue
        assert call(lib, make(**dict(later, **change))) == BAD
        assert lib.jsgx_last_error() == f"{who}: {message}".encode(), (refused[i][0], later)


@pytest.mark.parametrize("i", range(len(KNN_REFUSED)), ids=[r[0] for r in KNN_REFUSED])
def test_knn_refusals_in_their_order(capix, i):
    lib = capix.lib()
    in_order(lib, lambda **kw: knn_args(capix, **kw), KNN_REFUSED, i, KNN_CALLS)
    # ... also ahead of what only the launch refuses
    a = knn_args(capix, **KNN_REFUSED[i][1])
    assert lib.jsgx_knn_launch(C.byref(a), None, 0, None) == BAD and lib.jsgx_last_error() == f"jsgx_knn_launch: {KNN_REFUSED[i][2]}".encode()


@pytest.mark.parametrize("i", range(len(REC_REFUSED)), ids=[r[0] for r in REC_REFUSED])
def test_recurrence_refusals_in_their_order(capix, i):
    in_order(capix.lib(), lambda **kw: rec_args(capix, **kw), REC_REFUSED, i, (("jsgx_recurrence_launch", lambda lib, a: lib.jsgx_recurrence_launch(C.byref(a), None)),))


@pytest.mark.parametrize("i", range(len(NNF_REFUSED)), ids=[r[0] for r in NNF_REFUSED])
def test_nn_filter_refusals_in_their_order(capix, i):
    in_order(capix.lib(), lambda **kw: nnf_args(capix, **kw), NNF_REFUSED, i, (("jsgx_nn_filter_launch", lambda lib, a: lib.jsgx_nn_filter_launch(C.byref(a), None)),))


def test_what_only_the_launch_refuses_and_what_passes(capix):
    lib = capix.lib()
    a = knn_args(capix)
    need = 8 * 3 * 100 * 10 * 4          # 300 columns are five tiles: the automatic rule gives four workgroups a strip at the most
    for scratch, size, message in ((None, 1 << 40, "null scratch"), (SCRATCH + 2, 1 << 40, "scratch must be 4-byte aligned"),
                                   (SCRATCH, need - 1, "scratch smaller than jsgx_knn_scratch_bytes"), (None, 0, "null scratch")):
        assert lib.jsgx_knn_launch(C.byref(a), scratch, size, None) == BAD and lib.jsgx_last_error() == f"jsgx_knn_launch: {message}".encode()
    for call in (lib.jsgx_knn_launch(None, SCRATCH, 1 << 40, None), lib.jsgx_knn_scratch_bytes(None), lib.jsgx_knn_plan(None, 256, None, 0, None, None, None, None),
                 lib.jsgx_recurrence_launch(None, None), lib.jsgx_nn_filter_launch(None, None)):
        assert call == BAD and lib.jsgx_last_error().endswith(b": null argument")
    assert lib.jsgx_knn_plan(C.byref(a), 256, C.create_string_buffer(15), 15, None, None, None, None) == BAD and lib.jsgx_last_error() == b"jsgx_knn_plan: bad argument"
    assert lib.jsgx_knn_plan(C.byref(a), 0, None, 0, None, None, None, None) == BAD and lib.jsgx_last_error() == b"jsgx_knn_plan: n_cu must be >= 1"
    size = lambda **kw: lib.jsgx_knn_scratch_bytes(C.byref(knn_args(capix, **kw)))
    assert size() == need
    # one workgroup a strip needs no scratch, and then the launch does not look at it
    assert size(split=1) == 0 and size(m=64, y_pair_pitch=0) == 0 and size(split=3) == need // 4 * 3 and size(split=16) == need // 4 * 5
    # one pair: the pair pitches of the outputs are not looked at; a pair pitch of 0 on an input is a shared sequence
    assert size(pairs=1, index_pair_pitch=0, dist_pair_pitch=0) == need // 3 and size(x_pair_pitch=0, y_pair_pitch=0) == need
    # an output next to an input or to the other output, not inside it
    assert size(nn_index=X - 4 * (2 * 1200 + 99 * 12 + 10)) == need and size(nn_dist=Y + 4 * (2 * 6000 + 299 * 20 + 20)) == need and size(nn_dist=INDEX - 4 * 3000) == need
    assert size(k=256, index_pitch=256, dist_pitch=256, index_pair_pitch=25600, dist_pair_pitch=25600) == 8 * 3 * 100 * 256 * 4
    assert size(width=1 << 30) == need
    ok = lambda a, call: call(C.byref(a), None) in (0, capix.JSGX_ERR_NO_DEVICE)
    # the plane: connectivity needs neither distances nor a bandwidth; distance no bandwidth; their pitches are then not looked at
    rec = lambda **kw: rec_args(capix, **kw)
    import torch
    if not torch.cuda.is_available():           # with a device these calls would launch on pointers that are no memory
        assert ok(rec(), lib.jsgx_recurrence_launch) and ok(rec(mode=0, nn_dist=None, bandwidth=None, dist_pitch=0, dist_pair_pitch=0), lib.jsgx_recurrence_launch)
        assert ok(rec(mode=1, bandwidth=None), lib.jsgx_recurrence_launch) and ok(rec(sym=0, m=101), lib.jsgx_recurrence_launch)
        assert ok(rec(mode=1, out=BW - 4 * (2 * 10400 + 99 * 104 + 100) + 4 * 3), lib.jsgx_recurrence_launch)        # the bandwidth is not read in distance mode
        assert ok(rec(out=INDEX - 4 * (2 * 10400 + 99 * 104 + 100)), lib.jsgx_recurrence_launch) and ok(rec(pairs=1, index_pair_pitch=0, dist_pair_pitch=0, out_pair_pitch=0), lib.jsgx_recurrence_launch)
        nnf = lambda **kw: nnf_args(capix, **kw)
        assert ok(nnf(), lib.jsgx_nn_filter_launch) and ok(nnf(weights=None, weights_pitch=0, weights_pair_pitch=0), lib.jsgx_nn_filter_launch)
        assert ok(nnf(out=X + 4 * (2 * 2400 + 99 * 24 + 20)), lib.jsgx_nn_filter_launch) and ok(nnf(n_features=65536, s_frame_pitch=65536, out_frame_pitch=65536, s_pair_pitch=1 << 23, out_pair_pitch=1 << 23, s=9 << 44, out=10 << 44), lib.jsgx_nn_filter_launch)
        assert lib.jsgx_knn_launch(C.byref(a), SCRATCH, need, None) == capix.JSGX_ERR_NO_DEVICE and lib.jsgx_last_error() == b"jsgx_knn_launch: no HIP device"
        assert lib.jsgx_knn_launch(C.byref(knn_args(capix, split=1)), None, 0, None) == capix.JSGX_ERR_NO_DEVICE


def test_plans_and_scratch_over_shapes(jsg, capix):
    STRIP, TILE, LIMIT = capix.KNN_STRIP, capix.KNN_TILE, capix.KNN_LDS_LIMIT
    assert (STRIP, TILE, LIMIT, capix.KNN_THREADS, capix.KNN_MAX_K) == (64, 64, 163840, 256, 256)

    def auto(pairs, n, m, n_cu):
        strips, tiles, S = pairs * -(-n // STRIP), -(-m // TILE), 1
        while S < 16 and strips * S < n_cu and 2 * S <= tiles:
            S *= 2
        return S

    for pairs in (1, 3):
        for n in (1, STRIP - 1, STRIP, STRIP + 1, 2 * STRIP, 2 * STRIP + 1, 4096, 16384, 65536):          # a row more is a strip more
            for m in (1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, 15 * TILE, 16 * TILE, 16 * TILE + 1, 65536):
                for n_cu in (1, 2, 64, 255, 256, 257, 304):
                    for k in (1, 256):
                        name, strip, S, threads, lds = jsg.knn_plan(n, m, 20, k, pairs=pairs, n_cu=n_cu)
                        assert (name, strip, threads, lds) == ("knn_64", STRIP, 256, capix.KNN_LDS_STATIC + 6 * STRIP * k) and lds <= LIMIT
                        assert S == auto(pairs, n, m, n_cu) and S in (1, 2, 4, 8, 16) and S <= -(-m // TILE), (pairs, n, m, n_cu, S)
                for split in range(1, 17):
                    assert jsg.knn_plan(n, m, 20, 5, pairs=pairs, split=split)[2] == min(split, -(-m // TILE))
    # the automatic split on both sides of a workgroup per compute unit: 256 strips fill 256 compute units, 255 do not
    assert jsg.knn_plan(16384, 16384, 20, 256, n_cu=256)[2] == 1 and jsg.knn_plan(16384 - 64, 16384, 20, 256, n_cu=256)[2] == 2
    assert jsg.knn_plan(4096, 4096, 20, 130, n_cu=256)[2] == 4 and jsg.knn_plan(4096, 4096, 20, 130, n_cu=257)[2] == 8 and jsg.knn_plan(4096, 4096, 20, 130, n_cu=304)[2] == 8
    # k = 256 | 257 and the LDS limit: the largest list fits with room to spare, and no served k comes near the limit
    assert jsg.knn_plan(100, 100, 20, 256)[4] == capix.KNN_LDS_STATIC + 98304 == 142080 <= LIMIT
    with pytest.raises(jsg.JsgError, match="k must be in 1..256"):
        jsg.knn_plan(100, 100, 20, 257)
    with pytest.raises(jsg.JsgError, match="k must be in 1..256"):
        jsg.knn_plan(100, 100, 20, 0)
    with pytest.raises(jsg.JsgError, match="metric must be one of"):
        jsg.knn_plan(100, 100, 20, 5, metric="manhattan")
    assert [jsg.knn_default_k(n, w) for n, w in ((1, 0), (2, 0), (3, 1), (4, 0), (5, 0), (100, 1), (16384, 1), (16385, 0), (10 ** 6, 0), (3, 2), (10, 6))] == \
        [4, 4, 4, 6, 6, 20, 256, 256, 256, 1, 1]
    hdr = open(os.path.join(ROOT, "include", "jsgx.h")).read()
    for name, value in (("JSGX_KNN_MAX_K", capix.KNN_MAX_K), ("JSGX_KNN_MAX_SPLIT", capix.KNN_MAX_SPLIT), ("JSGX_KNN_STRIP", STRIP), ("JSGX_KNN_TILE", TILE),
                        ("JSGX_KNN_THREADS", capix.KNN_THREADS), ("JSGX_KNN_LDS_STATIC", capix.KNN_LDS_STATIC), ("JSGX_KNN_LDS_LIMIT", LIMIT),
                        ("JSGX_KNN_MERGE_THREADS", capix.KNN_MERGE_THREADS), ("JSGX_REC_CONNECTIVITY", capix.REC_CONNECTIVITY), ("JSGX_REC_DISTANCE", capix.REC_DISTANCE),
                        ("JSGX_REC_AFFINITY", capix.REC_AFFINITY), ("JSGX_REC_THREADS", capix.REC_THREADS), ("JSGX_REC_CHUNK", capix.REC_CHUNK),
                        ("JSGX_REC_LDS_BYTES", capix.REC_LDS_BYTES), ("JSGX_NNF_MAX_FEATURES", capix.NNF_MAX_FEATURES), ("JSGX_NNF_THREADS", capix.NNF_THREADS),
                        ("JSGX_ABI_VERSION", 1)):
        assert re.search(rf"#define {name} {value}\b", hdr), name
    for kernel in ("knn_64", "knn_merge", "recurrence_rows", "nn_filter_rows"):
        assert f'"{kernel}"' in hdr


@pytest.mark.parametrize("struct, ctype, size", [("jsgx_knn_args", "KnnArgs", 128), ("jsgx_recurrence_args", "RecurrenceArgs", 112), ("jsgx_nn_filter_args", "NnFilterArgs", 112)])
def test_struct_layouts_match_the_header(capix, tmp_path, struct, ctype, size):
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsgx.h")).read(), flags=re.S)
    body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", hdr, flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*(\[\d+\])?\s*$", decl).group(1) for decl in body.split(";") if decl.strip()]
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "jsgx.h"', "int main(void) {", f'    printf("%zu\\n", sizeof({struct}));']
    lines += [f'    printf("{f} %zu %zu\\n", offsetof({struct}, {f}), sizeof((({struct}*)0)->{f}));' for f in names]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)])
    out = subprocess.check_output([str(tmp_path / "layout")], text=True).split("\n")
    ctype = getattr(capix, ctype)
    assert out[0] == str(C.sizeof(ctype)) == str(size)
    assert [f for f, _ in ctype._fields_] == names
    offset = 0
    for (f, _), line in zip(ctype._fields_, out[1:]):
        assert line == f"{f} {getattr(ctype, f).offset} {getattr(ctype, f).size}"
        assert getattr(ctype, f).offset == offset, f"padding in front of {f}"
        offset += getattr(ctype, f).size


def test_python_names(jsg):
    want = {
        "knn": ["x", "y", "k", "width", "metric", "split"],
        "knn_launch": ["d_x", "d_y", "d_index", "d_dist", "width", "metric", "split", "d_scratch", "stream"],
        "knn_scratch_bytes": ["d_x", "d_y", "d_index", "d_dist", "width", "metric", "split"],
        "knn_plan": ["n", "m", "n_features", "k", "pairs", "metric", "split", "n_cu"],
        "knn_default_k": ["n", "width"],
        "recurrence_matrix": ["data", "k", "width", "metric", "sym", "mode", "bandwidth", "self"],
        "cross_similarity": ["data", "data_ref", "k", "metric", "mode", "bandwidth"],
        "recurrence_launch": ["d_index", "d_dist", "d_out", "mode", "sym", "diag", "d_bandwidth", "stream"],
        "nn_filter": ["S", "index", "weights"],
        "nn_filter_launch": ["d_s", "d_index", "d_out", "d_weights", "stream"],
    }
    for name, params in want.items():
        assert callable(getattr(jsg, name)) and name in jsg.__all__
        assert list(inspect.signature(getattr(jsg, name)).parameters) == params, name
    sig = inspect.signature(jsg.knn)
    assert [p.default for p in sig.parameters.values()][1:] == [None, None, 0, "euclidean", 0] and sig.parameters["width"].kind == inspect.Parameter.KEYWORD_ONLY
    assert [p.default for p in inspect.signature(jsg.recurrence_matrix).parameters.values()][1:] == [None, 1, "euclidean", False, "connectivity", None, False]
    assert [p.default for p in inspect.signature(jsg.cross_similarity).parameters.values()][2:] == [None, "euclidean", "connectivity", None]
    assert inspect.signature(jsg.nn_filter).parameters["weights"].default is None
    for name in ("jsgx_knn_scratch_bytes", "jsgx_knn_launch", "jsgx_knn_plan", "jsgx_recurrence_launch", "jsgx_nn_filter_launch"):
        assert name in jsg.capix.SIGNATURES
    assert "med_k_scalar" in jsg.recurrence_matrix.__doc__ and "v[(c-1)//2] + v[c//2]" in jsg.recurrence_matrix.__doc__


def test_kernel_notes(capix, tmp_path):
    """The new object: its six kernels, no private segment (no scratch memory, no spills), the static LDS the header states (the lists of
    the search are dynamic, as the plan states them) and the workgroup sizes."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    obj = os.path.join(ROOT, "jadespectrogram_amd", "build", "jsgx_knn.o")
    if not os.path.exists(obj):
        from jadespectrogram_amd import _build
        _build.build_lib()
    co = kernel_regs.code_object(obj, str(tmp_path))
    notes = subprocess.check_output([os.path.join(kernel_regs.LLVM, "llvm-readelf"), "--notes", co]).decode()
    found = {}
    for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
        g = lambda k: re.search(rf"\.{k}:\s+(\S+)", blk).group(1)
        name = subprocess.check_output(["c++filt", g("name")]).decode().strip()
        found[name.split("(")[0].replace("void ", "")] = (int(g("private_segment_fixed_size")), int(g("group_segment_fixed_size")), int(g("vgpr_spill_count")),
                                                         int(g("sgpr_spill_count")), int(g("max_flat_workgroup_size")))
    forward = (0, capix.KNN_LDS_STATIC, 0, 0, capix.KNN_THREADS)
    assert found == {"jsgx::knn_kernel<0>": forward, "jsgx::knn_kernel<1>": forward, "jsgx::knn_kernel<2>": forward,
                     "jsgx::knn_merge_kernel": (0, 1024, 0, 0, capix.KNN_MERGE_THREADS), "jsgx::recurrence_kernel": (0, capix.REC_LDS_BYTES, 0, 0, capix.REC_THREADS),
                     "jsgx::nn_filter_kernel": (0, 0, 0, 0, capix.NNF_THREADS)}


def test_host_entry_points_under_asan_ubsan(capix):
    """tests/cpp/jsgx_knn_host_test.cpp (its own main: the refusals, the scratch size and the plans over shapes) built together with the
    host units it calls under the address and undefined-behaviour sanitizers and run as a child process; the same program against the
    shipped library, there with the refusals that only the launches decide, gives the same verdict."""
    d = tempfile.gettempdir()
    drv = os.path.join(ROOT, "tests", "cpp", "jsgx_knn_host_test.cpp")
    hosts = [os.path.join(ROOT, "jadespectrogram_amd", "csrc", f) for f in ("jsgx_beat_host.cpp", "jsgx_knn_host.cpp")]
    common = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]
    san = os.path.join(d, "jsgx_knn_host_san")
    subprocess.check_call(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"] + hosts + [drv, "-o", san])
    libdir = os.path.dirname(capix.LIB_PATH)
    shipped = os.path.join(d, "jsgx_knn_host_lib")
    subprocess.check_call(common + ["-DJSGX_KNN_TEST_LAUNCHES", drv, "-o", shipped, "-L", libdir, "-ljsgx", f"-Wl,-rpath,{libdir}"])
    for exe in (san, shipped):
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == "ok" and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr

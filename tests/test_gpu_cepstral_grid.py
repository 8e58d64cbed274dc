"""The projection kernel of section 2k where a workgroup takes a second work item on each of its staging paths.  mfcc_kernel is
persistent (`item += gridDim.x`) and stages a tile in one of three ways: through registers one item ahead ("pre"), with 16-byte
loads straight to LDS ("vec"), or with 4-byte loads ("scalar").  tests/test_gpu_cepstral.py gives only the scalar path more items
than the grid has workgroups.  Here every path gets more than three grids of items with a ragged last round and a number of chunks
per row that does not divide the grid, so a workgroup's successive items differ in row, in position and in frame count (full chunks,
then the single last frame).  The bits are those of cr.project32 inside its float64 bound, those of one-row launches (six or so items:
no second round), and the same with the 16-byte loads turned off by the view's offset and pitches."""
import os
import re
import time

import numpy as np
import pytest

import cepstral_ref as cr
from cepstral_ref import raw, same
from test_gpu_cepstral import check_projection, run_mfcc, strides_of, torch_cuda  # noqa: F401  (torch_cuda is a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jadespectrogram_amd", "csrc")
DISTINCT = 7            # the rows repeat this many distinct planes


def constants():
    """kMfccPre, kMfccThreads, kMfccLdsOne and the cap on workgroups per compute unit, read from the sources so that a retune is seen."""
    unit, shared = open(os.path.join(CSRC, "jsg_cepstral.hip")).read(), open(os.path.join(CSRC, "jsg_internal.h")).read()
    pre = re.search(r"constexpr int kMfccPre = (\d+);", unit)
    threads = re.search(r"constexpr int kMfccThreads = (\d+);", shared)
    lds_one = re.search(r"constexpr int kMfccLdsOne = (\d+);", shared)
    cap = re.search(r"by_lds = std::min<long long>\((\d+), kMfccLdsOne / p\.lds_floats\);", unit)
    assert pre and threads and lds_one and cap, "the constants of mfcc_kernel's grid and staging rule are no longer where this test reads them"
    return tuple(int(m.group(1)) for m in (pre, threads, lds_one, cap))


# B, M, chunk_frames, the frames per item F that gives, T (full chunks and a single last frame), the path of a 16-byte aligned view.
# The product shape takes seven chunks per row (T = 385), not six (T = 321): by_lds is 3 there, and on 256 compute units six divides
# 768, so every workgroup would keep the kind of item it started with; seven and nine divide no multiple of 256 up to 8 x 256.
CASES = {
    "pre-product": dict(B=128, M=20, chunk=0, F=64, T=385, path="pre"),        # eight pieces per thread: all the registers
    "pre-small": dict(B=32, M=13, chunk=0, F=64, T=513, path="pre"),           # two pieces per thread
    "pre-chunk8": dict(B=128, M=20, chunk=8, F=8, T=65, path="pre"),           # one piece per thread, frames past F in the others
    "vec": dict(B=256, M=20, chunk=0, F=64, T=321, path="vec"),                # sixteen pieces per thread: no registers
}
# an offset and pitches that turn the 16-byte loads off: a base that is 4-byte aligned only, pitches that are no multiple of four
UNALIGNED = dict(offset=1, pad_frame=3, pad_row=5)


def staging_path(shape, B, F, offset=0, pad_frame=0, pad_row=0):
    """The rule of mfcc_kernel's header: vec where B % 4 == 0, the base is 16-byte aligned (the allocation is) and both pitches are
    multiples of four; pre where a thread's share of a tile is then at most kMfccPre pieces of 16 bytes."""
    n_pre, threads, _, _ = constants()
    row_pitch, frame_pitch, _ = strides_of(shape, (pad_row, pad_frame))
    vec = B % 4 == 0 and offset % 4 == 0 and frame_pitch % 4 == 0 and row_pitch % 4 == 0
    if not vec:
        return "scalar"
    return "pre" if -(-F * (B // 4) // threads) <= n_pre else "vec"


_prepared = {}


def prepared(jsg, torch, name):
    """Per case, once: the sizes, the input of `rows` rows that repeat DISTINCT planes, the table, the restatement of the distinct
    planes, and (filled in by the first test that runs) the result of the aligned launch."""
    if name in _prepared:
        return _prepared[name]
    c = dict(CASES[name])
    B, M, T, F = c["B"], c["M"], c["T"], c["F"]
    _, _, lds_one, cap = constants()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    distinct = np.array(cr.planes(DISTINCT, 513, 256)[:, :T, :B])
    D = np.array(jsg.mfcc_table(B, M) if name == "pre-product" else cr.tables(M, B))
    d_one, d_D = torch.from_numpy(distinct[:1]).cuda(), torch.from_numpy(D).cuda()
    _, F_plan, lds_bytes = jsg.mfcc_plan(d_one, d_D, torch.empty((1, T, M), dtype=torch.float32, device="cuda"), chunk_frames=c["chunk"])
    assert F_plan == F and lds_bytes % 4 == 0, (F_plan, lds_bytes)
    by_lds = min(cap, lds_one // (lds_bytes // 4))
    assert by_lds >= 1
    chunks = -(-T // F)
    assert T % F == 1 and chunks >= 5                   # full chunks, then a single frame
    # the grid is cus * min(by_lds, what the registers allow), and the registers' share is not visible here: three rounds of the
    # largest it can be, and the other two premises for every size it can have
    bound = cus * by_lds
    grids = [cus * k for k in range(1, by_lds + 1)]
    rows = -(-(3 * bound + 1) // chunks)
    while any(rows * chunks % g == 0 for g in grids):
        rows += 1
    items = rows * chunks
    assert items >= 3 * bound, (items, bound)
    for g in grids:
        assert items % g != 0, ("no ragged last round", items, g)
        assert g % chunks != 0, ("a workgroup's items are all of one kind", chunks, g)
    idx = np.arange(rows) % DISTINCT
    c.update(D=D, S=distinct[idx], idx=idx, want=cr.project32(distinct, D), rows=rows, chunks=chunks, items=items, bound=bound, grids=grids, got=None)
    _prepared[name] = c
    return c


def aligned_run(jsg, torch, c):
    if c["got"] is None:
        c["got"] = run_mfcc(jsg, torch, c["S"], c["D"], chunk_frames=c["chunk"], pad_out=3, pad_out_row=2)
    return c["got"]


def sample_rows(c):
    """The first row, the last, and the two rows that straddle each multiple of grid // chunks (the row where a workgroup's round
    ends), for every size the grid can have."""
    rows = {0, c["rows"] - 1}
    for g in c["grids"]:
        step = g // c["chunks"]
        rows |= {r for m in range(step, c["rows"], step) for r in (m - 1, m)}
    return sorted(rows)


@pytest.mark.parametrize("name", CASES)
def test_vector_paths_take_more_items_than_the_grid(jsg, torch_cuda, name):
    torch = torch_cuda
    c = prepared(jsg, torch, name)
    assert staging_path(c["S"].shape, c["B"], c["F"]) == c["path"]
    t = time.perf_counter()
    got = aligned_run(jsg, torch, c)            # the sentinels around the view are checked inside
    elapsed = time.perf_counter() - t
    want = c["want"][c["idx"]]
    assert same(got, want), (name, "elements that differ from the restatement", int((raw(got) != raw(want)).sum()), got.size)
    check_projection(got[:DISTINCT], c["S"][:DISTINCT], c["D"], name)
    sample = sample_rows(c)
    for r in sample:
        assert same(run_mfcc(jsg, torch, c["S"][r], c["D"], chunk_frames=c["chunk"]), got[r:r + 1]), (name, "row together differs from row alone", r)
    print(f"mfcc {name} ({c['path']}): {c['rows']} rows x {c['chunks']} chunks = {c['items']} items, grid at most {c['bound']}, {elapsed:.2f} s, "
          f"{len(sample)} rows alone, {time.perf_counter() - t:.2f} s in all")


@pytest.mark.parametrize("name", CASES)
def test_same_bits_with_the_vector_loads_turned_off(jsg, torch_cuda, name):
    """The same values through a view whose offset and pitches turn the 16-byte loads off: the scalar path, with the same items and
    the same grid, gives the bits of the vector path."""
    torch = torch_cuda
    c = prepared(jsg, torch, name)
    assert staging_path(c["S"].shape, c["B"], c["F"], **UNALIGNED) == "scalar"
    base = aligned_run(jsg, torch, c)
    t = time.perf_counter()
    got = run_mfcc(jsg, torch, c["S"], c["D"], chunk_frames=c["chunk"], out_offset=2, pad_out=1, **UNALIGNED)
    assert same(got, base), (name, "elements that differ from the vector path", int((raw(got) != raw(base)).sum()), got.size)
    print(f"mfcc {name} (scalar): {c['items']} items, grid at most {c['bound']}, {time.perf_counter() - t:.2f} s")

"""Band-limited resampling and pitch shift on the GPU (include/jsg.h section 2g) against tests/resample_ref.py: accuracy on the case
list under both bounds, the analytic cases and the impulse to the bit, identical bits over chunk lengths, row counts, pitches, the
default chunk's edges, a launch of many items and every kernel path, the edges of short inputs, NaN containment, the Python layer
(resample, pitch_shift) and graph capture."""
import numpy as np
import pytest

import resample_ref as rr

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25e11)
DEFAULT_CHUNK = 4096        # outputs per work item where chunk_outputs = 0 (RS_DEFAULT_CHUNK of csrc/jsg_resample.hip)
PATHS = {"resample_lds", "resample_l2"}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


_plans = {}


def plan(jsg, name):
    """The Resampler over the numpy-built table of tests/resample_ref.py (so that GPU and reference read the same bits)."""
    if name not in _plans:
        Z, P, win = rr.table(name)
        _plans[name] = jsg.Resampler.from_table(win, Z, P)
    return _plans[name]


def raw(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(raw(a), raw(b))


def run(jsg, torch, name, x, step, *, chunk_outputs=0, pad_in=0, pad_out=0, offset=0, whole=False, query=False):
    """x numpy [rows][L] -> y numpy [rows][T] of one launch.  Rows lie pad_in / pad_out floats apart beyond their length and both
    buffers start `offset` floats into their allocation; the output buffer is filled with a sentinel first.  whole: also the
    output rows with their padding.  query: the kernel name instead."""
    x = np.atleast_2d(x)
    R, L = x.shape
    T = rr.resample_length(L, step)
    b_in = torch.zeros(offset + R * (L + pad_in), dtype=torch.float32, device="cuda")
    d_in = b_in[offset:].view(R, L + pad_in)[:, :L]
    d_in.copy_(torch.from_numpy(np.array(x)))
    b_out = torch.full((offset + R * (T + pad_out),), float(SENTINEL), dtype=torch.float32, device="cuda")
    d_full = b_out[offset:].view(R, T + pad_out)
    d_out = d_full[:, :T]
    if query:
        return jsg.resample_kernel_name(plan(jsg, name), d_in, step, d_out, chunk_outputs=chunk_outputs)
    jsg.resample_launch(plan(jsg, name), d_in, step, d_out, chunk_outputs=chunk_outputs)
    torch.cuda.synchronize()
    full = d_full.cpu().numpy()
    return (full[:, :T].copy(), full) if whole else full[:, :T].copy()


_tight = {}


def tight(jsg, torch, name, step_name):
    """The GPU's result of a case in tight buffers with the default chunk, computed once."""
    if (name, step_name) not in _tight:
        _tight[name, step_name] = run(jsg, torch, name, rr.inputs(rr.case_length(step_name)), rr.STEPS[step_name])
    return _tight[name, step_name]


def check_bounds(y, ref, what=""):
    """Bound (b) on every sample, then bound (a) per row; prints the figures first."""
    err = np.abs(y.astype(np.float64) - ref["y64"])
    over = float((err / np.maximum(ref["cap"], 1e-300)).max()) if err.size else 0.0
    e_gpu, e_ref = rr.peak_error(y, ref["y64"]), rr.peak_error(ref["y32"], ref["y64"])
    print(f"{what}: error over cap {over:.3f}; error / 2^-24 of the peak, GPU {e_gpu / 2.0 ** -24}, restatement {e_ref / 2.0 ** -24}")
    assert np.isfinite(y).all() and (err <= ref["cap"]).all(), over
    assert (e_gpu <= rr.YARDSTICKS * e_ref).all(), (e_gpu, e_ref)


@pytest.mark.parametrize("c", rr.CASES, ids=rr.case_id)
def test_accuracy_pitched_rows_at_an_odd_offset(jsg, torch_cuda, c):
    name, step_name = c
    L, step = rr.case_length(step_name), rr.STEPS[step_name]
    ref = rr.case(name, step_name)
    y, full = run(jsg, torch_cuda, name, rr.inputs(L), step, pad_in=5, pad_out=3, offset=1, whole=True)
    assert y.shape == (3, ref["T"])
    check_bounds(y, ref, rr.case_id(c))
    assert (full[:, ref["T"]:] == SENTINEL).all()                                   # between out_samples and the pitch: not written
    Z, P, win = rr.table(name)
    assert same(y[2], rr.impulse_response(L, step, Z, P, win, rr.impulse_at(L)))    # every tap position of the case to the bit
    assert same(y, tight(jsg, torch_cuda, name, step_name))                        # tight and padded pitches, two alignments


def test_every_path_is_taken(jsg, torch_cuda):
    taken = {c: run(jsg, torch_cuda, c[0], rr.inputs(rr.case_length(c[1])), rr.STEPS[c[1]], query=True) for c in rr.CASES}
    assert set(taken.values()) == PATHS, taken
    assert taken[("best", "64")] == "resample_l2" and taken[("best", "147/160")] == "resample_lds" and taken[("fast", "64")] == "resample_lds"


def test_ramp_at_step_1_is_the_identity(jsg, torch_cuda):
    x = rr.inputs(3000)
    assert same(tight(jsg, torch_cuda, "ramp", "1"), np.array(x))


def test_ramp_at_step_half_is_linear_interpolation(jsg, torch_cuda):
    x = rr.inputs(3000)
    y = tight(jsg, torch_cuda, "ramp", "0.5")
    nxt = np.concatenate([x[:, 1:], np.zeros((3, 1), np.float32)], axis=1)
    assert same(y[:, 0::2], np.array(x)) and same(y[:, 1::2], (np.float32(0.5) * (x + nxt)).astype(np.float32))


CHUNK_CASES = [("fast", "147/160"), ("best", "3.7"), ("best", "64"), ("ramp", "1/64")]       # the third takes the L2 path


@pytest.mark.parametrize("chunk", [0, 1, 63, 64, 65, 1000])
@pytest.mark.parametrize("c", CHUNK_CASES, ids=rr.case_id)
def test_bits_do_not_depend_on_the_chunk(jsg, torch_cuda, c, chunk):
    name, step_name = c
    y = run(jsg, torch_cuda, name, rr.inputs(rr.case_length(step_name)), rr.STEPS[step_name], chunk_outputs=chunk, pad_in=chunk % 7, pad_out=chunk % 5)
    assert same(y, tight(jsg, torch_cuda, name, step_name))


# chunks that take more than one pass: the span is staged again between the passes.  (table, step, L, outputs per pass at chunk 0)
PASS_CASES = [("best", 2.0, 10000, 3964), ("best", 3.7, 20000, 2084), ("best", 64.0, 38400 + 77, 512), ("fast", 40.0, 170000, 787)]


@pytest.mark.parametrize("c", PASS_CASES, ids=lambda c: f"{c[0]}-{c[1]:g}")
def test_chunks_of_several_passes(jsg, torch_cuda, c):
    name, step, L, sub0 = c
    x = np.random.default_rng(L).standard_normal((2, L)).astype(np.float32)
    T = rr.resample_length(L, step)
    d = torch_cuda.empty((2, L), dtype=torch_cuda.float32, device="cuda"), torch_cuda.empty((2, T), dtype=torch_cuda.float32, device="cuda")
    passes = lambda chunk: -(-min(chunk or DEFAULT_CHUNK, T) // jsg.resample_plan(plan(jsg, name), d[0], step, d[1], chunk_outputs=chunk)[1])
    assert jsg.resample_plan(plan(jsg, name), d[0], step, d[1])[1] == sub0 < T and passes(64) == 1
    one_pass = run(jsg, torch_cuda, name, x, step, chunk_outputs=64)
    for chunk in (0, DEFAULT_CHUNK, 65536, sub0 + 1):
        assert passes(chunk) >= 2, chunk
        assert same(run(jsg, torch_cuda, name, x, step, chunk_outputs=chunk, pad_in=3, pad_out=1), one_pass), chunk
    if step <= 4:
        Z, P, win = rr.table(name)
        check_bounds(one_pass, rr.evaluate(x, step, Z, P, win), f"{name} step {step:g} L = {L}")


# tables of many zero crossings at a large step: the wings alone exceed the LDS, the input is read through L2
DIRECT_CASES = [(320, 64, 64.0, 3000), (1024, 32, 20.0, 3000), (512, 64, 64.0, 5000)]


@pytest.mark.parametrize("c", DIRECT_CASES, ids=str)
def test_direct_path(jsg, torch_cuda, c):
    Z, P, step, L = c
    win = rr.kaiser_table(Z, P, 0.9, 10.0)
    _plans[c] = jsg.Resampler.from_table(win, Z, P)
    x = np.random.default_rng(Z).standard_normal((2, L)).astype(np.float32)
    assert run(jsg, torch_cuda, c, x, step, query=True) == "resample_direct"
    y, full = run(jsg, torch_cuda, c, x, step, pad_in=2, pad_out=3, offset=1, whole=True)
    ref = rr.evaluate(x, step, Z, P, win)
    check_bounds(y, ref, f"direct {c}")
    assert (full[:, ref["T"]:] == SENTINEL).all()
    for chunk in (1, 7, 65536):
        assert same(run(jsg, torch_cuda, c, x, step, chunk_outputs=chunk), y)
    _plans.pop(c).close()


@pytest.mark.parametrize("c", [("fast", "147/160"), ("best", "64")], ids=rr.case_id)
def test_bits_do_not_depend_on_the_row_count(jsg, torch_cuda, c):
    name, step_name = c
    step = rr.STEPS[step_name]
    base = np.array(rr.inputs(3000)[:, 1000:1064])                       # L = 64: noise, tone, zeros
    base[2, 33] = 1.0
    three = run(jsg, torch_cuda, name, base, step)
    Z, P, win = rr.table(name)
    check_bounds(three, rr.evaluate(base, step, Z, P, win), "L = 64")
    for r in range(3):
        assert same(run(jsg, torch_cuda, name, base[r], step), three[r:r + 1])
    many = run(jsg, torch_cuda, name, np.tile(base, (21845, 1)), step, pad_in=1)
    assert many.shape[0] == 65535 and same(many, np.tile(three, (21845, 1)))


@pytest.mark.parametrize("L", [3762, 3763, 3764])
def test_default_chunk_edges(jsg, torch_cuda, L):
    """T one less than, exactly and one more than the default chunk (step 147/160: T = ceil(L 160 / 147))."""
    step = rr.STEPS["147/160"]
    T = rr.resample_length(L, step)
    assert T == DEFAULT_CHUNK + (L - 3763)
    x = np.random.default_rng(L).standard_normal((2, L)).astype(np.float32)
    y = run(jsg, torch_cuda, "fast", x, step)
    Z, P, win = rr.table("fast")
    check_bounds(y, rr.evaluate(x, step, Z, P, win), f"T = {T}")
    assert same(y, run(jsg, torch_cuda, "fast", x, step, chunk_outputs=DEFAULT_CHUNK - 1))
    assert same(y, run(jsg, torch_cuda, "fast", x, step, chunk_outputs=64))


def test_many_items_in_one_launch(jsg, torch_cuda):
    """2^22 outputs at chunk_outputs = 64: 65 536 work items, several times the grid."""
    L = 1 << 21
    x = np.random.default_rng(22).standard_normal((1, L)).astype(np.float32)
    y = run(jsg, torch_cuda, "fast", x, 0.5, chunk_outputs=64)
    assert y.shape == (1, 1 << 22) and same(y, run(jsg, torch_cuda, "fast", x, 0.5))
    Z, P, win = rr.table("fast")
    head = rr.evaluate(x[:, :4096], 0.5, Z, P, win)                       # outputs that see nothing past sample 4096 - Z
    keep = 2 * (4096 - Z) - 2
    err = np.abs(y[:, :keep].astype(np.float64) - head["y64"][:, :keep])
    assert (err <= head["cap"][:, :keep]).all()


@pytest.mark.parametrize("name", rr.TABLES)
@pytest.mark.parametrize("L", [1, 10])
def test_short_inputs(jsg, torch_cuda, name, L):
    """L = 1 and an input shorter than one wing: every output is an edge."""
    Z, P, win = rr.table(name)
    x = np.random.default_rng(L).standard_normal((2, L)).astype(np.float32)
    for step_name in ("147/160", "160/147", "3.7", "1/64", "64", "1"):
        step = rr.STEPS[step_name]
        y = run(jsg, torch_cuda, name, x, step, pad_out=2)
        ref = rr.evaluate(x, step, Z, P, win)
        assert y.shape == (2, ref["T"])
        check_bounds(y, ref, f"{name} L = {L} step {step_name}")


@pytest.mark.parametrize("c", [("fast", "147/160"), ("best", "3.7")], ids=rr.case_id)
def test_nan_is_contained(jsg, torch_cuda, c):
    name, step_name = c
    step = rr.STEPS[step_name]
    ref = rr.case(name, step_name)
    clean = tight(jsg, torch_cuda, name, step_name)
    for m0, value in ((0, np.nan), (1499, np.inf), (2999, np.nan)):
        x = np.array(rr.inputs(3000))
        x[1, m0] = value
        y = run(jsg, torch_cuda, name, x, step)
        hit = (ref["first"] <= m0) & (m0 <= ref["last"])
        assert hit.any() and not hit.all()
        assert same(y[0], clean[0]) and same(y[2], clean[2])
        assert same(y[1][~hit], clean[1][~hit])
        assert (np.isnan(y[1][hit]) if np.isnan(value) else ~np.isfinite(y[1][hit])).all()


def test_python_resample_batches(jsg, torch_cuda):
    torch = torch_cuda
    x = torch.from_numpy(np.random.default_rng(7).standard_normal((2, 3, 2205)).astype(np.float32)).cuda()
    y = jsg.resample(x, 44100, 48000)
    T = rr.resample_length(2205, 44100 / 48000)
    assert y.shape == (2, 3, T) == (2, 3, 2400) and y.dtype == torch.float32
    want = torch.empty((6, T), dtype=torch.float32, device="cuda")
    rs = jsg.Resampler("best")
    jsg.resample_launch(rs, x.reshape(6, -1), 44100 / 48000, want)
    assert torch.equal(y.reshape(6, T), want)
    assert torch.equal(jsg.resample(x[1, 2], 44100, 48000), y[1, 2]) and jsg.resample(x[0], 44100, 48000).shape == (3, T)
    fast = jsg.Resampler("fast")
    yf = jsg.resample(x, 48000, 16000, resampler=fast)
    assert yf.shape == (2, 3, 735) and not torch.equal(yf, jsg.resample(x, 48000, 16000))
    Z, P, win = 64, 512, rs.table
    check_bounds(y.reshape(6, T).cpu().numpy(), rr.evaluate(x.reshape(6, -1).cpu().numpy(), 44100 / 48000, Z, P, win), "resample 44100 -> 48000")


@pytest.mark.parametrize("n_steps", [4, -7])
def test_pitch_shift(jsg, torch_cuda, n_steps):
    torch = torch_cuda
    sr, L = 22050, 32768
    x = torch.from_numpy(np.sin(2 * np.pi * 440.0 / sr * np.arange(L)).astype(np.float32)[None]).cuda()
    y = jsg.pitch_shift(x, n_steps)
    assert y.shape == (1, L) and y.dtype == torch.float32
    # the composition of the public calls, bit for bit
    rate = 2.0 ** (-n_steps / 12)
    z = jsg.time_stretch(x, rate)
    w = torch.empty((1, jsg.resample_length(z.shape[-1], 1.0 / rate)), dtype=torch.float32, device="cuda")
    jsg.resample_launch(jsg.Resampler("best"), z, 1.0 / rate, w)
    w = w[:, :L] if w.shape[1] >= L else torch.nn.functional.pad(w, (0, L - w.shape[1]))
    assert torch.equal(y, w)
    peak = int(np.argmax(np.abs(np.fft.rfft(y[0].cpu().numpy().astype(np.float64)))))
    want = 440.0 * 2.0 ** (n_steps / 12) * L / sr
    print(f"pitch_shift {n_steps:+d}: peak at bin {peak}, expected {want:.2f}")
    assert abs(peak - want) <= 1.0
    assert torch.equal(jsg.pitch_shift(x[0], n_steps), y[0])              # one-dimensional input


def test_graph_capture(jsg, torch_cuda):
    """A captured graph on one stream that holds the launch, replayed twice, equals eager."""
    torch = torch_cuda
    name, step_name = "best", "2^(4/12)"
    step = rr.STEPS[step_name]
    d_in = torch.from_numpy(np.array(rr.inputs(3000))).cuda()
    d_out = torch.zeros((3, rr.resample_length(3000, step)), dtype=torch.float32, device="cuda")
    rs = plan(jsg, name)
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):      # warm-up outside capture (uploads the table on first use)
        jsg.resample_launch(rs, d_in, step, d_out, stream=s.cuda_stream)
    s.synchronize()
    with torch.cuda.graph(graph, stream=s):
        jsg.resample_launch(rs, d_in, step, d_out, stream=s.cuda_stream)
    for _ in range(2):
        d_out.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert same(d_out.cpu().numpy(), tight(jsg, torch_cuda, name, step_name))

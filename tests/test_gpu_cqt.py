"""Constant-Q and variable-Q spectrograms on the GPU (include/jsg.h section 2h) against tests/cqt_ref.py: accuracy under both bounds in
pitched buffers with sentinels, the impulse to the bit, identical bits over chunk lengths, row counts, pitches, a launch of many items
and both paths, the hop-delay identity, the power plane and its dB / colour chain, NaN containment, frames beyond the signal, graph
capture of a first launch, and the Python layer.  Bases come from CqtBasis.from_tables, so that GPU and reference read the same bits."""
import numpy as np
import pytest

import cqt_ref as cr

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25e11)
PATHS = {"cqt_span", "cqt_passes"}          # what jsg_cqt_plan can return


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


_bases = {}


def basis(jsg, name="synthetic"):
    if name not in _bases:
        if name == "synthetic":
            half, taps = cr.synthetic_basis()
        elif name == "long":                 # one bin of 80 001 taps: the taps take several passes
            half, taps = cr.synthetic_basis((40000,), 5)
        elif name == "sixteen":              # 16 bins over the lane widths and one tap count above 64
            half, taps = cr.synthetic_basis((0, 0, 1, 2, 3, 5, 7, 8, 12, 15, 16, 20, 31, 32, 40, 70), 6)
        else:
            half, _, _, _, taps = cr.standard_basis(name == "standard")
        _bases[name] = jsg.CqtBasis.from_tables(half, taps)
    return _bases[name]


def raw(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(raw(a), raw(b))


def run(jsg, torch, b, x, hop, T, *, power=False, chunk_frames=0, pad_in=0, pad_frame=0, pad_row=0, offset=0, query=False):
    """x numpy [rows][n] -> C numpy [rows][T][K] of one launch (complex64, or float32 power).  Input rows lie pad_in floats apart beyond
    their length, frames pad_frame and rows pad_row output elements apart beyond theirs; the input starts `offset` floats and the output
    `offset` elements into its allocation.  The input allocation holds NaN outside the rows (a tap that is not live is not read and
    multiplied by zero).  The output allocation is filled with a sentinel first, and every element of it that the
    launch must not write is checked to hold it still.  query: the kernel name instead."""
    x = np.atleast_2d(x)
    R, n = x.shape
    K = b.n_bins
    b_in = torch.full((offset + R * (n + pad_in),), float("nan"), dtype=torch.float32, device="cuda")    # NaN around the rows: never read
    d_in = b_in[offset:].view(R, n + pad_in)[:, :n]
    d_in.copy_(torch.from_numpy(np.array(x)))
    fp = K + pad_frame
    rp = T * fp + pad_row
    total = offset + R * rp + 3
    width = 1 if power else 2
    flat = torch.full((total * width,), float(SENTINEL), dtype=torch.float32, device="cuda")
    elems = flat if power else torch.view_as_complex(flat.view(-1, 2))
    d_out = torch.as_strided(elems, (R, T, K), (rp, fp, 1), storage_offset=offset)
    if query:
        return jsg.cqt_kernel_name(b, d_in, hop, T, d_out, power=power, chunk_frames=chunk_frames)
    jsg.cqt_launch(b, d_in, hop, T, d_out, power=power, chunk_frames=chunk_frames)
    torch.cuda.synchronize()
    got = flat.cpu().numpy().reshape(total, width)
    written = np.zeros(total, bool)
    at = offset + (np.arange(R)[:, None, None] * rp + np.arange(T)[None, :, None] * fp + np.arange(K)[None, None, :])
    written[at.ravel()] = True
    assert (got[~written] == SENTINEL).all()            # before the buffer, between K and the pitches, after the last row
    out = got[at.ravel()].reshape(R, T, K, width)
    return out[..., 0].copy() if power else out.copy().view(np.complex64)[..., 0]


_tight = {}


def tight(jsg, torch, hop):
    """The GPU's result of the shared inputs on the synthetic basis in tight buffers with the default chunk, computed once."""
    if hop not in _tight:
        _tight[hop] = run(jsg, torch, basis(jsg), cr.inputs(cr.L), hop, cr.frames(cr.L, hop))
    return _tight[hop]


def check_bounds(C, ref, what=""):
    """Bound (b) on every element and component, then bound (a) per row; prints the figures first."""
    d = C.astype(np.complex128) - ref["C64"]
    over = max(float((np.abs(d.real) / np.maximum(ref["cap_re"], 1e-300)).max()), float((np.abs(d.imag) / np.maximum(ref["cap_im"], 1e-300)).max()))
    e_gpu, e_ref = cr.peak_error(C, ref["C64"]), cr.peak_error(ref["C32"], ref["C64"])
    ratio = float(np.max(np.where(e_ref > 0, e_gpu / np.where(e_ref > 0, e_ref, 1.0), 0.0)))
    print(f"{what}: error over cap {over:.3f}; error / 2^-24 of the peak, GPU {e_gpu / 2.0 ** -24}, restatement {e_ref / 2.0 ** -24}; worst ratio {ratio:.3f}")
    assert np.isfinite(C.real).all() and np.isfinite(C.imag).all()
    assert (np.abs(d.real) <= ref["cap_re"]).all() and (np.abs(d.imag) <= ref["cap_im"]).all(), over
    assert (e_gpu <= cr.YARDSTICKS * e_ref).all(), (e_gpu, e_ref)


@pytest.mark.parametrize("hop", cr.HOPS)
def test_accuracy_pitched_rows_at_an_odd_offset(jsg, torch_cuda, hop):
    ref = cr.case(hop)
    T = cr.frames(cr.L, hop)
    C = run(jsg, torch_cuda, basis(jsg), cr.inputs(cr.L), hop, T, pad_in=5, pad_frame=3, pad_row=7, offset=1)
    assert C.shape == (3, T, len(cr.SYNTH_HALF))
    check_bounds(C, ref, f"hop {hop}")
    # the impulse: every tap of every bin it reaches, to the bit; zero elsewhere (by value: a zero's sign may differ)
    half, taps = cr.synthetic_basis()
    want = cr.impulse_response(half, taps, hop, T, cr.impulse_at(cr.L))
    hit = cr.touched(half, hop, T, cr.impulse_at(cr.L))
    assert (C[2] == want).all() and same(C[2][hit], want[hit])
    assert same(C, tight(jsg, torch_cuda, hop))                                     # tight and padded pitches, two alignments


def test_standard_basis_bounds_and_tone(jsg, torch_cuda):
    x = cr.standard_inputs()
    T = cr.frames(cr.STANDARD_L, cr.STANDARD_HOP)
    C = run(jsg, torch_cuda, basis(jsg, "standard"), x, cr.STANDARD_HOP, T, pad_frame=1)
    check_bounds(C, cr.standard_case(True), "standard basis")
    U = run(jsg, torch_cuda, basis(jsg, "unscaled"), x, cr.STANDARD_HOP, T)
    check_bounds(U, cr.standard_case(False), "standard basis, no scale")
    half = cr.standard_basis(False)[0]
    frames = np.flatnonzero(cr.interior(half, cr.STANDARD_HOP, T, cr.STANDARD_L).all(axis=1))
    mag = np.abs(U[1][frames].astype(np.complex128))
    print("tone of amplitude 0.5 at bin 12: |C|", mag[:, 12].min(), mag[:, 12].max())
    assert frames.size >= 10 and (np.abs(mag[:, 12] / 0.25 - 1.0) <= 1e-4).all() and (mag.argmax(axis=1) == 12).all()


@pytest.mark.parametrize("hop", [7, 512])
def test_bits_do_not_depend_on_the_chunk_or_the_pitches(jsg, torch_cuda, hop):
    T = cr.frames(cr.L, hop)
    for chunk in (1, 2, 3, 17, T + 5, 65536):
        C = run(jsg, torch_cuda, basis(jsg), cr.inputs(cr.L), hop, T, chunk_frames=chunk, pad_in=chunk % 7, pad_frame=chunk % 5, pad_row=chunk % 3, offset=chunk % 2)
        assert same(C, tight(jsg, torch_cuda, hop)), chunk


def test_bits_do_not_depend_on_the_row_count(jsg, torch_cuda):
    hop = 7
    base = np.array(cr.inputs(cr.L)[:, 1000:1016])                       # L = 16: noise, tone, zeros
    base[2, 9] = 1.0
    half, taps = cr.synthetic_basis()
    T = cr.frames(16, hop)
    three = run(jsg, torch_cuda, basis(jsg), base, hop, T)
    check_bounds(three, cr.evaluate(base, half, taps, hop, T), "L = 16")
    for r in range(3):
        assert same(run(jsg, torch_cuda, basis(jsg), base[r], hop, T), three[r:r + 1])
    many = run(jsg, torch_cuda, basis(jsg), np.tile(base, (21845, 1)), hop, T, pad_in=1)
    assert many.shape[0] == 65535 and same(many, np.tile(three, (21845, 1, 1)))


def test_many_items_in_one_launch(jsg, torch_cuda):
    """8 rows x 16 bins x 100 frames at chunk_frames = 1: 12 800 work items, several times the grid."""
    b = basis(jsg, "sixteen")
    hop, n = 5, 499
    T = cr.frames(n, hop)
    assert T == 100
    x = np.random.default_rng(8).standard_normal((8, n)).astype(np.float32)
    props = torch_cuda.cuda.get_device_properties(0)
    assert 8 * 16 * T >= 3 * 8 * props.multi_processor_count
    C = run(jsg, torch_cuda, b, x, hop, T, chunk_frames=1)
    assert same(C, run(jsg, torch_cuda, b, x, hop, T, pad_frame=2))
    check_bounds(C, cr.evaluate(x, b.half_lengths, b.taps, hop, T), "16 bins, chunk 1")


def test_every_path_is_taken(jsg, torch_cuda):
    """One bin of 80 001 taps over 4 frames walks its taps in passes; the accumulators live across them, so the bits are the chunk's."""
    b = basis(jsg, "long")
    hop, n = 20000, 60001
    T = cr.frames(n, hop)
    assert T == 4
    x = np.random.default_rng(4).standard_normal((2, n)).astype(np.float32)
    names = {run(jsg, torch_cuda, b, x, hop, T, query=True), run(jsg, torch_cuda, basis(jsg), cr.inputs(cr.L), 512, cr.frames(cr.L, 512), query=True)}
    assert names == PATHS
    assert run(jsg, torch_cuda, b, x, hop, T, query=True) == "cqt_passes"
    C = run(jsg, torch_cuda, b, x, hop, T, pad_frame=1, offset=1)
    check_bounds(C, cr.evaluate(x, b.half_lengths, b.taps, hop, T), "80 001 taps")
    for chunk in (1, 3):
        assert same(run(jsg, torch_cuda, b, x, hop, T, chunk_frames=chunk), C)
    # a longer signal at a small hop: the windows of a pass overlap in LDS, and frames 14..20 have every tap live
    x2 = np.random.default_rng(5).standard_normal((2, 100001)).astype(np.float32)
    T2 = cr.frames(100001, 3000)
    assert T2 == 34 and cr.interior(b.half_lengths, 3000, T2, 100001).sum() == 7
    C2 = run(jsg, torch_cuda, b, x2, 3000, T2)
    check_bounds(C2, cr.evaluate(x2, b.half_lengths, b.taps, 3000, T2), "80 001 taps, hop 3000")
    assert same(run(jsg, torch_cuda, b, x2, 3000, T2, chunk_frames=2), C2)


@pytest.mark.parametrize("hop", [7, 64, 512])
def test_hop_delay_identity(jsg, torch_cuda, hop):
    half, _ = cr.synthetic_basis()
    x = np.array(cr.inputs(cr.L)[:2])
    delayed = np.zeros_like(x)
    delayed[:, hop:] = x[:, :-hop]
    T = cr.frames(cr.L, hop)
    a = tight(jsg, torch_cuda, hop)[:2]
    d = run(jsg, torch_cuda, basis(jsg), delayed, hop, T)
    inside = cr.interior(half, hop, T, cr.L)
    both = inside[1:] & inside[:-1]
    assert both.any()
    for r in range(2):
        assert same(d[r, 1:][both], a[r, :-1][both])


def test_power_plane_and_its_colour_chain(jsg, torch_cuda):
    torch = torch_cuda
    hop = 64
    T = cr.frames(cr.L, hop)
    C = tight(jsg, torch, hop)
    P = run(jsg, torch, basis(jsg), cr.inputs(cr.L), hop, T, power=True, pad_frame=2, pad_row=1, offset=1)
    re, im = C.real.astype(np.float32), C.imag.astype(np.float32)
    assert P.dtype == np.float32 and same(P, re * re + im * im)
    # cqt_db then colormap equals the same chain fed from numpy's power of the complex output
    x = torch.from_numpy(np.array(cr.standard_inputs()[1])).cuda()
    kw = dict(hop_length=512, n_bins=24)
    db = jsg.cqt_db(x, 22050.0, **kw)
    Cx = jsg.cqt(x, 22050.0, **kw).transpose(-1, -2).cpu().numpy()
    power = (Cx.real * Cx.real + Cx.imag * Cx.imag).astype(np.float32)
    d_db = torch.empty((power.shape[0], 24), dtype=torch.float32, device="cuda")
    jsg.spectrogram.db_from_power(torch.from_numpy(power).cuda(), d_db)
    assert db.shape == (24, power.shape[0]) and torch.equal(db.transpose(-1, -2), d_db)
    d_lut = torch.from_numpy(jsg.colormap_lut(256, 6)).cuda()
    images = []
    for plane in (db.transpose(-1, -2).contiguous(), d_db):
        img = torch.zeros((24, power.shape[0]), dtype=torch.int32, device="cuda")
        jsg.colormap(plane, d_lut, -80.0, 0.0, d_argb=img)
        torch.cuda.synchronize()
        images.append(img.cpu().numpy())
    assert np.array_equal(images[0], images[1]) and len(np.unique(images[0])) > 8


@pytest.mark.parametrize("hop", [7, 512])
def test_nan_is_contained(jsg, torch_cuda, hop):
    half, _ = cr.synthetic_basis()
    T = cr.frames(cr.L, hop)
    clean = tight(jsg, torch_cuda, hop)
    for m0, value in ((0, np.nan), (1499, np.inf), (2999, np.nan)):
        x = np.array(cr.inputs(cr.L))
        x[1, m0] = value
        C = run(jsg, torch_cuda, basis(jsg), x, hop, T)
        hit = cr.touched(half, hop, T, m0)
        assert hit.any() and not hit.all()
        assert same(C[0], clean[0]) and same(C[2], clean[2])
        assert same(C[1][~hit], clean[1][~hit])
        bad = C[1][hit]
        assert (np.isnan(bad.real) & np.isnan(bad.imag) if np.isnan(value) else ~np.isfinite(bad.real) | ~np.isfinite(bad.imag)).all()


def test_frames_beyond_the_signal_are_plus_zero(jsg, torch_cuda):
    hop = 512
    T = cr.frames(cr.L, hop) + 9             # the last 7 frames lie more than 1000 samples past the end
    C = run(jsg, torch_cuda, basis(jsg), cr.inputs(cr.L), hop, T, pad_frame=1)
    assert same(C[:, :cr.frames(cr.L, hop)], tight(jsg, torch_cuda, hop))
    half, _ = cr.synthetic_basis()
    empty = np.arange(T)[:, None] * hop - np.asarray(half, np.int64)[None, :] >= cr.L
    assert empty[-7:].all() and empty.sum() > 7 * 9
    assert (raw(C[:, empty]) == 0).all()                                  # +0 in both components
    Pw = run(jsg, torch_cuda, basis(jsg), cr.inputs(cr.L), hop, T, power=True)
    assert (raw(Pw[:, empty]) == 0).all()


def test_graph_capture_of_a_first_launch(jsg, torch_cuda):
    """A new basis: created (uploaded) outside the capture, its first launch inside it; replayed twice, equals eager."""
    torch = torch_cuda
    hop = 64
    T = cr.frames(cr.L, hop)
    half, taps = cr.synthetic_basis()
    b = jsg.CqtBasis.from_tables(half, taps)
    b.handle(0)
    d_in = torch.from_numpy(np.array(cr.inputs(cr.L))).cuda()
    d_out = torch.zeros((3, T, b.n_bins), dtype=torch.complex64, device="cuda")
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=s):
        jsg.cqt_launch(b, d_in, hop, T, d_out, stream=s.cuda_stream)
    for _ in range(2):
        d_out.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert same(d_out.cpu().numpy(), tight(jsg, torch_cuda, hop))
    b.close()


def test_python_layer(jsg, torch_cuda):
    torch = torch_cuda
    x = np.array(cr.standard_inputs())
    half, _, f, _, taps = cr.standard_basis(True)
    ref = cr.standard_case(True)
    kw = dict(hop_length=cr.STANDARD_HOP, n_bins=24)
    C = jsg.cqt(x, 22050.0, **kw)                                       # numpy in, numpy out
    T = cr.frames(cr.STANDARD_L, cr.STANDARD_HOP)
    assert isinstance(C, np.ndarray) and C.dtype == np.complex64 and C.shape == (2, 24, T)
    assert np.array_equal(jsg.cqt_frequencies(24), f)
    b = jsg.spectrogram._cqt_basis(22050.0, None, 24, 12, 1.0, 0.0, True)
    assert np.array_equal(b.half_lengths, half)
    # the library's own basis differs from numpy's by an ulp of a tap here and there: the reference is evaluated on the library's taps
    own = ref if np.array_equal(b.taps, taps) else cr.evaluate(x, b.half_lengths, b.taps, cr.STANDARD_HOP, T)
    check_bounds(np.ascontiguousarray(C.transpose(0, 2, 1)), own, "cqt()")
    d = np.abs(C.transpose(0, 2, 1).astype(np.complex128) - ref["C64"])
    assert d.max() <= 1e-5 * np.abs(ref["C64"]).max()                   # ... and numpy's basis gives the same transform
    xt = torch.from_numpy(x).cuda()
    Ct = jsg.cqt(xt, 22050.0, **kw)
    assert Ct.is_cuda and Ct.shape == (2, 24, T) and same(Ct.cpu().numpy(), C)
    assert same(jsg.vqt(xt, 22050.0, gamma=0.0, **kw).cpu().numpy(), C)                 # gamma = 0: the bits of cqt
    assert same(jsg.cqt(xt[1], 22050.0, **kw).cpu().numpy(), C[1])                      # one-dimensional input
    V = jsg.vqt(xt, 22050.0, gamma=6.0, **kw)
    vb = jsg.spectrogram._cqt_basis(22050.0, None, 24, 12, 1.0, 6.0, True)
    assert (vb.half_lengths < half).all() and V.shape == (2, 24, T)
    check_bounds(np.ascontiguousarray(V.cpu().numpy().transpose(0, 2, 1)), cr.evaluate(x, vb.half_lengths, vb.taps, cr.STANDARD_HOP, T), "vqt(gamma = 6)")
    assert np.array_equal(vb.half_lengths, cr.basis(22050.0, cr.C1, 24, gamma=6.0)[0])

"""Non-negative matrix factorisation of libjsgx.so on the GPU (include/jsgx.h section 12) against tests/nmf_ref.py, bit for bit, in pitched
buffers full of sentinels that must come back untouched.  The first test is the pipe probe: one activation update whose sums, on data
where the order of a sum shows in its bits, equal the k-ascending fmaf chain; every other test rests on it.  Then the graph capture of a
first launch, every component count, bin count and frame count at which a kernel takes another path (crossed sparsely: every value
appears, and so does every pair of extremes), one to three iterations and once 25, fixed components, three problems, the known answers,
two scratch sizes, a plane more than 2^31 elements behind the first, and the Python layer: decompose behind stft_fb on two tones, fit=False,
sort=True."""
import functools

import numpy as np
import pytest

import nmf_ref as nr

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25e11)
CK, CT = nr.CHUNK_K, nr.CHUNK_T
R_SET = (1, 5, 16, 17, 32, 33, 64)
K_SET = (1, 2, 3, 31, 33, CK - 1, CK, CK + 1, 2 * CK + 3)
T_SET = (1, 2, 31, 33, 64, 65, CT, CT + 1, 2 * CT + 5)
# (T, K, r): the eight corners, then every other value once or more
SHAPES = [(T, K, r) for T in (T_SET[0], T_SET[-1]) for K in (K_SET[0], K_SET[-1]) for r in (R_SET[0], R_SET[-1])] + [
    (2, 2, 5), (31, 3, 16), (33, 31, 17), (64, 33, 32), (65, CK - 1, 33), (CT, CK, 5), (CT + 1, CK + 1, 16), (64, CK + 1, 17), (33, CK, 32), (2, CK - 1, 33)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def test_the_sets_are_covered():
    assert {s[0] for s in SHAPES} == set(T_SET) and {s[1] for s in SHAPES} == set(K_SET) and {s[2] for s in SHAPES} == set(R_SET)


def guarded(torch, planes, rows, cols, pad, sentinel, offset):
    """A flat buffer full of `sentinel` and the view [planes][rows][cols] inside it with `pad` extra elements per row and 3 * pad per plane."""
    pitch, size = cols + pad, rows * (cols + pad) + 3 * pad
    flat = torch.full((planes * size + offset + 5,), sentinel, dtype=torch.float32, device="cuda")
    return flat, torch.as_strided(flat, (planes, rows, cols), (size, pitch, 1), storage_offset=offset)


def untouched(flat, view, sentinel, offset):
    got = flat.cpu().numpy()
    inside = np.zeros(got.size, bool)
    P, R, W = view.shape
    inside[(offset + np.arange(P)[:, None, None] * view.stride(0) + np.arange(R)[None, :, None] * view.stride(1) + np.arange(W)[None, None, :]).ravel()] = True
    return bool((got[~inside] == sentinel).all() if sentinel == sentinel else np.isnan(got[~inside]).all())


def run(jsg, torch, problems, n_iter, *, update=True, pad=3, extra_scratch=0):
    """One launch over `problems` (a list of (V, A0, C0) of equal shapes) -> (A [P][T][r], C [P][r][K]) as numpy, after checking that
    nothing outside A and C was written: not the padding, not V, not the scratch's guard."""
    P, (T, K), r = len(problems), problems[0][0].shape, problems[0][2].shape[0]
    fv, d_v = guarded(torch, P, T, K, pad, float("nan"), 3)
    fa, d_a = guarded(torch, P, T, r, 2 * pad, float(SENTINEL), 1)
    fc, d_c = guarded(torch, P, r, K, pad, float(SENTINEL), 2)
    for d, i in ((d_v, 0), (d_a, 1), (d_c, 2)):
        d.copy_(torch.from_numpy(np.stack([p[i] for p in problems])))
    need = jsg.nmf_scratch_bytes(d_v, d_a, d_c, n_iter=n_iter, update_components=update)
    assert need % 4 == 0 and need > 0
    d_scratch = torch.full((need // 4 + extra_scratch + 4,), float(SENTINEL), dtype=torch.float32, device="cuda")
    jsg.nmf_launch(d_v, d_a, d_c, n_iter=n_iter, update_components=update, d_scratch=d_scratch[:need // 4 + extra_scratch])
    torch.cuda.synchronize()
    assert untouched(fa, d_a, SENTINEL, 1) and untouched(fc, d_c, SENTINEL, 2), "a guard element was written"
    assert untouched(fv, d_v, float("nan"), 3) and nr.same_bits(d_v.cpu().numpy(), np.stack([p[0] for p in problems])), "the plane was written"
    assert (d_scratch[need // 4 + extra_scratch:].cpu().numpy() == SENTINEL).all(), "the scratch's guard was written"
    return d_a.cpu().numpy(), d_c.cpu().numpy()


def check(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert nr.same_bits(got, want), (what, np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want)))[:4])


@functools.lru_cache(maxsize=None)
def reference(T, K, r, n_iter, update=True, seed=0):
    V, A0, C0 = nr.problem(T, K, r, seed)
    A, C = nr.nmf32(V, A0, C0, n_iter, update)
    A.setflags(write=False), C.setflags(write=False)
    return A, C


def test_the_pipe_probe(jsg, torch_cuda):
    """T = 32, K = 258, r = 32, one iteration, fixed components, on the input that tests/test_nmf_ref.py shows to tell the order of a sum:
    the matrix pipe's sums are the header's chains (N over two chunks of bins, G, D), or nothing below can hold."""
    T, K, r = 32, 258, 32
    V, A0, C0 = nr.problem(T, K, r)
    A, C = run(jsg, torch_cuda, [(V, A0, C0)], 1, update=False)
    check(C[0], C0, "fixed components")
    want = nr.update_a32(V, A0, C0)
    differ = int((A[0].view(np.uint32) != want.view(np.uint32)).sum())
    down = nr.update_a32(V, A0, C0, reverse=True)
    print(f"pipe probe: {differ} of {want.size} activations differ from the ascending chain; {int((A[0].view(np.uint32) != down.view(np.uint32)).sum())} from the descending one")
    check(A[0], want, "the ascending chain")


def test_graph_capture_of_a_first_launch(jsg, torch_cuda):
    """r = 40 is the one count between 33 and 48 in this file in front of the shapes below: the kernels of three component tiles, and every
    kernel of the component update, are launched here for the first time in the process, under capture."""
    torch = torch_cuda
    T, K, r = 70, 130, 40
    V, A0, C0 = nr.problem(T, K, r)
    d_v = torch.zeros((T, K), dtype=torch.float32, device="cuda")
    d_a, d_c = torch.from_numpy(np.array(A0)).cuda(), torch.from_numpy(np.array(C0)).cuda()
    d_scratch = torch.empty(jsg.nmf_scratch_bytes(d_v, d_a, d_c) // 4, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            jsg.nmf_launch(d_v, d_a, d_c, n_iter=2, d_scratch=d_scratch, stream=side.cuda_stream)
    torch.cuda.synchronize()
    assert nr.same_bits(d_a.cpu().numpy(), A0) and nr.same_bits(d_c.cpu().numpy(), C0)          # captured, not run
    d_v.copy_(torch.from_numpy(np.array(V)))
    g.replay()
    torch.cuda.synchronize()
    A, C = reference(T, K, r, 2)
    check(d_a.cpu().numpy(), A, "replayed A")
    check(d_c.cpu().numpy(), C, "replayed C")


@pytest.mark.parametrize("T, K, r", SHAPES)
def test_shapes(jsg, torch_cuda, T, K, r):
    assert jsg.nmf_plan(T, K, r) == ("nmf_update_a", 256, 40960, 8, -(-T // CT))
    n_iter = 1 if T * K * r > 1 << 20 else 2
    A, C = run(jsg, torch_cuda, [nr.problem(T, K, r)], n_iter)
    wa, wc = reference(T, K, r, n_iter)
    check(A[0], wa, "A")
    check(C[0], wc, "C")


@pytest.mark.parametrize("n_iter, shape", [(1, (65, 257, 17)), (2, (65, 257, 17)), (3, (65, 257, 17)), (25, (70, 33, 5))])
def test_iterations(jsg, torch_cuda, n_iter, shape):
    A, C = run(jsg, torch_cuda, [nr.problem(*shape)], n_iter, pad=0)
    wa, wc = reference(*shape, n_iter)
    check(A[0], wa, "A")
    check(C[0], wc, "C")


def test_fixed_components(jsg, torch_cuda):
    T, K, r = 65, CK + 1, 17
    assert jsg.nmf_plan(T, K, r, update_components=False)[3] == 1
    V, A0, C0 = nr.problem(T, K, r)
    A, C = run(jsg, torch_cuda, [(V, A0, C0)], 3, update=False)
    check(C[0], C0, "C stays")
    check(A[0], reference(T, K, r, 3, False)[0], "A")


def test_three_problems(jsg, torch_cuda):
    T, K, r = 70, 130, 7
    problems = [nr.problem(T, K, r, seed) for seed in (0, 5, 6)]
    A, C = run(jsg, torch_cuda, problems, 2)
    for p, seed in enumerate((0, 5, 6)):
        wa, wc = reference(T, K, r, 2, True, seed)
        check(A[p], wa, ("A", p))
        check(C[p], wc, ("C", p))


def test_a_problem_pitch_beyond_2_to_31(jsg, torch_cuda):
    """The second problem's plane lies more than 2^31 elements behind the first (one allocation of 8.6 GB, not filled): the kernels'
    offsets into V are 64-bit."""
    torch = torch_cuda
    T, K, r = 33, 70, 5
    pitch = (1 << 31) + 64
    flat = torch.empty(pitch + T * (K + 1) + 8, dtype=torch.float32, device="cuda")
    d_v = torch.as_strided(flat, (2, T, K), (pitch, K + 1, 1), storage_offset=3)
    problems = [nr.problem(T, K, r, seed) for seed in (0, 7)]
    d_v.copy_(torch.from_numpy(np.stack([p[0] for p in problems])))
    d_a, d_c = (torch.from_numpy(np.stack([p[i] for p in problems])).cuda() for i in (1, 2))
    jsg.nmf_launch(d_v, d_a, d_c, n_iter=2)
    torch.cuda.synchronize()
    for p, seed in enumerate((0, 7)):
        wa, wc = reference(T, K, r, 2, True, seed)
        check(d_a[p].cpu().numpy(), wa, ("A", p))
        check(d_c[p].cpu().numpy(), wc, ("C", p))
    del flat, d_v
    torch.cuda.empty_cache()


def test_two_scratch_sizes(jsg, torch_cuda):
    T, K, r = CT + 1, 70, 5
    first = run(jsg, torch_cuda, [nr.problem(T, K, r)], 2)
    second = run(jsg, torch_cuda, [nr.problem(T, K, r)], 2, extra_scratch=12345)
    check(first[0], second[0], "A")
    check(first[1], second[1], "C")
    check(first[0][0], reference(T, K, r, 2)[0], "A against the restatement")


def test_known_answers(jsg, torch_cuda):
    """Without the restatement: an exact factorisation of small integers is a fixed point, bit for bit; an all-zero frame zeroes its row of
    A, an all-zero bin its column of C, and an all-zero row of A stays zero."""
    rng = np.random.default_rng(3)
    T, K, r = 70, 130, 6
    A0, C0 = rng.integers(0, 4, (T, r)).astype(np.float32), rng.integers(0, 4, (r, K)).astype(np.float32)
    A0[:, 0] += 1
    C0[0] += 1
    V = (A0.astype(np.float64) @ C0.astype(np.float64)).astype(np.float32)
    A, C = run(jsg, torch_cuda, [(V, A0, C0)], 3)
    check(A[0], A0, "the fixed point's A")
    check(C[0], C0, "the fixed point's C")
    V, A0, C0 = (np.array(x) for x in nr.problem(T, K, r))
    V[7] = 0
    V[:, 11] = 0
    A0[20] = 0
    A, C = run(jsg, torch_cuda, [(V, A0, C0)], 2)
    assert not A[0][7].any() and not C[0][:, 11].any() and not A[0][20].any()
    keep = np.ones(T, bool)
    keep[[7, 20]] = False
    assert (A[0][keep] > 0).all() and (np.delete(C[0], 11, axis=1) > 0).all()


# ---------------------------------------------------------------------------------------------------- the Python layer
def two_tones(jsg, torch):
    """Band power [frames][bands] of a signal that holds one tone in its first half and another in its second, from stft_fb on the GPU."""
    fs, n, hop, bands = 22050.0, 512, 256, 40
    t = np.arange(48 * hop + n) / fs
    half = t.size // 2
    x = np.where(np.arange(t.size) < half, np.sin(2 * np.pi * 440.0 * t), np.sin(2 * np.pi * 2500.0 * t)).astype(np.float32)
    frames = 1 + (x.size - n) // hop
    plan, fb = jsg.Plan(n, jsg.window(jsg.capi.WIN_HANN, n)), jsg.Filterbank(n, fs, bands, 0.0, fs / 2)
    S = torch.empty((frames, bands), dtype=torch.float32, device="cuda")
    jsg.stft_fb_db(plan, fb, torch.from_numpy(x[None]).cuda(), hop, frames, S, feedblocks=n // hop, linear_out=True)
    torch.cuda.synchronize()
    return S


def test_decompose_two_tones(jsg, torch_cuda):
    torch = torch_cuda
    S = two_tones(jsg, torch)
    V = S.cpu().numpy()
    T, K = V.shape
    assert (V >= 0).all() and np.isfinite(V).all()
    tones = {int(V[:T // 2 - 2].sum(0).argmax()), int(V[T // 2 + 2:].sum(0).argmax())}
    assert len(tones) == 2
    A0, C0 = nr.start(T, K, 2, 9)
    # decided on the restatement first: each component's peak is the band of one tone
    wa, wc = nr.nmf32(V, A0, C0, 30)
    assert {int(c.argmax()) for c in wc} == tones
    comps, acts = jsg.decompose(S, 2, n_iter=30, components=torch.from_numpy(C0).cuda(), activations=torch.from_numpy(A0).cuda())
    assert tuple(comps.shape) == (2, K) and tuple(acts.shape) == (T, 2)
    check(comps.cpu().numpy(), wc, "components")
    check(acts.cpu().numpy(), wa, "activations")
    # the seeded start: the same call twice gives the same bits, the peaks are the tones' bands, and sorting orders them
    first, second = jsg.decompose(S, 2, n_iter=30, seed=4), jsg.decompose(S, 2, n_iter=30, seed=4)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert {int(i) for i in first[0].argmax(dim=1).cpu()} == tones
    sc, sa = jsg.decompose(S, 2, n_iter=30, seed=4, sort=True)
    assert [int(i) for i in sc.argmax(dim=1).cpu()] == sorted(tones)
    order = [int(i) for i in torch.argsort(first[0].argmax(dim=1), stable=True).cpu()]
    assert torch.equal(sc, first[0][order]) and torch.equal(sa, first[1][:, order])


def test_decompose_fit_false(jsg, torch_cuda):
    torch = torch_cuda
    T, K, r = 70, 33, 5
    V, _, C0 = nr.problem(T, K, r)
    d_c = torch.from_numpy(np.array(C0)).cuda()
    comps, acts = jsg.decompose(torch.from_numpy(np.array(V)).cuda(), n_iter=4, components=d_c, fit=False)
    assert torch.equal(comps, d_c) and comps.data_ptr() != d_c.data_ptr()
    # the start is torch's float32 sqrt(mean / r): plumbing, recomputed here the way decompose states it; the contract begins behind it
    scale = torch.sqrt(torch.from_numpy(np.array(V)).cuda().mean(dim=(-2, -1), keepdim=True) / r).cpu().numpy().astype(np.float32)
    want, _ = nr.nmf32(V, np.full((T, r), scale[0, 0], np.float32), C0, 4, update_components=False)
    check(acts.cpu().numpy(), want, "activations")
    assert abs(float(scale[0, 0]) - nr.constant_start(V, r)) <= 4 * nr.U * nr.constant_start(V, r)
    with pytest.raises(jsg.JsgError):
        jsg.decompose(torch.from_numpy(np.array(V)).cuda(), 5, fit=False)


def test_decompose_problems_and_sort(jsg, torch_cuda):
    """A leading axis of problems, and sort=True with a tie: components whose peaks share a bin keep their order."""
    torch = torch_cuda
    T, K, r = 40, 20, 4
    C0 = np.full((2, r, K), 0.1, np.float32)
    for p, peaks in enumerate(((9, 3, 9, 0), (1, 1, 0, 5))):
        for c, k in enumerate(peaks):
            C0[p, c, k] = 1.0 + 0.1 * c
    A0 = np.stack([nr.start(T, K, r, 20 + p)[0] for p in range(2)])
    V = np.stack([(A0[p].astype(np.float64) @ C0[p].astype(np.float64)).astype(np.float32) for p in range(2)])
    args = dict(n_iter=1, components=torch.from_numpy(C0).cuda(), activations=torch.from_numpy(A0).cuda())
    c, a = jsg.decompose(torch.from_numpy(V).cuda(), **args)
    sc, sa = jsg.decompose(torch.from_numpy(V).cuda(), sort=True, **args)
    assert tuple(c.shape) == (2, r, K) and tuple(a.shape) == (2, T, r)
    for p in range(2):
        wa, wc = nr.nmf32(V[p], A0[p], C0[p], 1)
        check(c[p].cpu().numpy(), wc, ("C", p))
        check(a[p].cpu().numpy(), wa, ("A", p))
        peaks = wc.argmax(axis=1)
        order = sorted(range(r), key=lambda i: (peaks[i], i))
        assert len(set(peaks)) < r          # there is a tie
        check(sc[p].cpu().numpy(), wc[order], ("sorted C", p))
        check(sa[p].cpu().numpy(), wa[:, order], ("sorted A", p))

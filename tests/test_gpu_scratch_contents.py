"""No launch depends on what its scratch buffer held on entry.  The thirteen launchers that work through caller-supplied scratch memory
(include/jsg.h: stft_fb, istft, pvoc, hpss; include/jsgx.h: beat, dtw, viterbi, pyin_decode, knn, rqa, nmf, pcen, peak) state that the
layout is private, the contents on entry are undefined and a larger scratch changes nothing.  The scratch is how one kernel hands work to
the next (chunk sums and their prefixes, entering states, tile bests, partial neighbour lists, back-pointers, paths written backwards,
overlap frames), so a kernel that reads a cell no earlier kernel wrote is a real way to be wrong, and a run on fresh zero pages or on the
block the previous identical call left behind does not show it.

Every case here hands in its own scratch: exactly the size the launcher asks for, at the alignment the header demands and no better, with
guard bytes in front and behind, filled in turn with zeros, with 0x5A (a large finite float, a large positive int, 0x5A5A as a uint16),
with 0xFF (a negative NaN, -1, 65535 as a back-pointer) and with what a launch of the same launcher on a larger shape and other data left
there.  Asserted for every (case, fill): the outputs (into sentinel-filled buffers) equal the unit's own reference -- the bit-exact
restatements of tests/*_ref.py, for stft_fb and istft the float64 references under the bounds of tests/test_gpu_filterbank.py and
tests/cstft_ref.py, for pvoc the bounds of tests/test_gpu_pvoc.py -- and are bit-identical across the fills; the guard bytes are as they
were; and at least one byte of the scratch changed, so that no case passes by never reaching its scratch."""
import ctypes
import functools

import numpy as np
import pytest

import beat_ref as br
import cstft_ref as cr
import dtw_ref as dr
import hpss_ref as hr
import knn_ref as kr
import nmf_ref as nr
import pcen_ref as pc
import peak_ref as pk
import pvoc_ref as pv
import pyin_ref as py
import rqa_ref as rr
import viterbi_ref as vr
import test_gpu_beat as tb
import test_gpu_dtw as td
import test_gpu_hpss as th
import test_gpu_knn as tk
import test_gpu_nmf as tn
import test_gpu_pcen as tc
import test_gpu_peak as tp
import test_gpu_pyin as ty
import test_gpu_rqa as tr
import test_gpu_viterbi as tv
from parity_util import FLOOR_BY_N

pytestmark = pytest.mark.gpu

SENTINEL, ISENTINEL = float(np.float32(-7.25e11)), -77777
FILLS = ("zeros", "0x5A", "0xFF", "stale")
FILL_BYTE = {"zeros": 0x00, "0x5A": 0x5A, "0xFF": 0xFF, "stale": 0xFF}      # stale: what the larger launch does not write stays 0xFF
GUARD = 256
CASES = {}            # id -> (alignment of the scratch in bytes, factory(jsg, torch) -> (Work of the case, Work of the larger shape))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


class Scratch:
    """`size` bytes of scratch that start `align` bytes behind a 256-byte boundary (the alignment the header demands and no better), with
    at least GUARD bytes of the same allocation in front of them and behind them."""

    def __init__(self, torch, size, align):
        self.raw = torch.empty(GUARD + 256 + align + size + GUARD, dtype=torch.uint8, device="cuda")
        self.start = GUARD + (-(self.raw.data_ptr() + GUARD)) % 256 + align
        assert (self.raw.data_ptr() + self.start) % 256 == align and self.start + size + GUARD <= self.raw.numel()

    def fill(self, byte):
        self.raw.fill_(byte)

    def view(self, need, dtype):
        """The first `need` bytes as the tensor a launch takes: its size is exactly `need`."""
        return self.raw[self.start:self.start + need].view(dtype)

    def snapshot(self):
        return self.raw.clone()

    def guards_hold(self, before, need):
        lo, hi = self.start, self.start + need
        return bool((self.raw[:lo] == before[:lo]).all()) and bool((self.raw[hi:] == before[hi:]).all())

    def changed(self, before, need):
        lo, hi = self.start, self.start + need
        return bool((self.raw[lo:hi] != before[lo:hi]).any())


class Work:
    """One launch: alloc() -> fresh sentinel-filled output tensors; bind(outs) -> (args, kwargs) of both size(*args, **kwargs) -> the
    bytes of scratch and launch(*args, d_scratch=, **kwargs); check(outs as numpy) asserts them against the reference."""

    def __init__(self, torch, alloc, bind, size, launch, check, dtype=None):
        self.torch, self.alloc, self.bind, self.size, self.launch, self.check = torch, alloc, bind, size, launch, check
        self.dtype = torch.uint8 if dtype is None else dtype
        args, kw = bind(alloc())
        self.need = int(size(*args, **kw))

    def run(self, scratch):
        outs = self.alloc()
        args, kw = self.bind(outs)
        self.launch(*args, d_scratch=scratch.view(self.need, self.dtype), **kw)
        self.torch.cuda.synchronize()
        return tuple(o.cpu().numpy() for o in outs)


def case(name, align):
    def register(factory):
        CASES[name] = (align, factory)
        return factory
    return register


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------------- libjsg: stft_fb
FB_N, FB_HOP, FB_BANDS, FB_FS, FB_CH = 512, 128, 40, 48000.0, 2
FB_PITCH = -(-(FB_N // 2 + 1) // 32) * 32          # floats per power column in the scratch: whole 128-byte lines


def fb_float64_check(oracle, fb, win, xs, got, what):
    """The float64 bound of tests/test_gpu_filterbank.py::test_hardware_log_and_float64_bound on linear band power, batch by batch."""
    n, hop, B = FB_N, FB_HOP, fb.n_bands
    Wd = fb.matrix().astype(np.float64)
    for k, x in enumerate(xs):
        F = got.shape[1]
        idx = (np.arange(F) * hop)[:, None] + np.arange(n)[None, :]
        frames = x[:, idx].astype(np.float64) * win.astype(np.float64)[None, None, :]
        P = (np.abs(np.fft.rfft(frames, axis=-1)) ** 2).mean(axis=0)
        band64 = P @ Wd.T
        peak = P.max(axis=1, keepdims=True)
        tol = (1e-5 * P + FLOOR_BY_N[n] * peak) @ Wd.T + (fb.n_bins[None, :] + 1) * 2.0 ** -24 * (P @ np.abs(Wd).T)
        err = np.abs(got[k, :, :B].astype(np.float64) - band64)
        assert (err <= tol).all(), f"{what} batch {k}: worst ratio {np.max(err / np.maximum(tol, 1e-300)):.3g}"
        assert (got[k, :, B:] == np.float32(SENTINEL)).all(), f"{what} batch {k}: written past the bands"


def fb_step(jsg, torch, plan, fb, oracle):
    """The columns of the smallest scratch the launch accepts: below it the call is refused and enqueues nothing."""
    F = 8
    x = torch.from_numpy(oracle.synth_audio(FB_CH, (F - 1) * FB_HOP + FB_N, seed=1)).cuda()
    out = torch.zeros((F, FB_BANDS), dtype=torch.float32, device="cuda")
    for cols in range(1, 65):
        try:
            jsg.stft_fb_db(plan, fb, x, FB_HOP, F, out, d_scratch=torch.empty(cols * FB_PITCH, dtype=torch.float32, device="cuda"), linear_out=True)
            torch.cuda.synchronize()
            return cols
        except jsg.JsgError as e:
            assert e.code == jsg.capi.JSG_ERR_INVALID
    raise AssertionError("no scratch of up to 64 columns was accepted")


def fb_case(batches):
    def factory(jsg, torch):
        from oracle import jsg_oracle as oracle
        win = oracle.window(oracle.WIN_HANN, FB_N)
        plan, fb = jsg.Plan(FB_N, win), jsg.Filterbank(FB_N, FB_FS, FB_BANDS)
        step = fb_step(jsg, torch, plan, fb, oracle)
        launch = jsg.stft_fb_db_strided if batches > 1 else jsg.stft_fb_db

        def work(F, cols, seed):
            xs = np.stack([oracle.synth_audio(FB_CH, (F - 1) * FB_HOP + FB_N, seed=seed + k) for k in range(batches)])
            d_in = torch.from_numpy(xs if batches > 1 else xs[0]).cuda()
            alloc = lambda: (torch.full((batches, F, FB_BANDS + 3), SENTINEL, dtype=torch.float32, device="cuda"),)
            bind = lambda outs: ((plan, fb, d_in, FB_HOP, F, outs[0] if batches > 1 else outs[0][0]), dict(linear_out=True))
            check = lambda got: fb_float64_check(oracle, fb, win, xs, got[0], (batches, F, cols))
            return Work(torch, alloc, bind, lambda *a, **kw: 4 * cols * FB_PITCH, launch, check, torch.float32)

        return work(3 * step + 1, step, 40), work(5 * step + 2, 2 * step, 50)      # four chunks, the last of one column | three chunks
    return factory


case("stft_fb_db", 16)(fb_case(1))
case("stft_fb_db_strided-2-batches", 16)(fb_case(2))


# ---------------------------------------------------------------------------------------------------------------- libjsg: istft
def istft_case(hop, extra):
    def factory(jsg, torch):
        n, rows = 512, 2
        w = cr.window("hann", n)
        plan = jsg.CStftPlan(n, w)

        def work(F, per_row, seed):
            X = cr.random_bins(rows, F, n, seed)
            T = (F - 1) * hop + n
            ref, Y_inv = cr.inverse_f64(X, n, hop, w, T), cr.inverse_yardstick(X, n)
            d_X = torch.from_numpy(X).cuda()
            alloc = lambda: (torch.full((rows, T), SENTINEL, dtype=torch.float32, device="cuda"),)
            check = lambda got: cr.assert_inverse(got[0], ref, Y_inv, f"istft hop={hop} F={F} frames per row={per_row}", n, hop)
            return Work(torch, alloc, lambda outs: ((plan, d_X, hop, F, outs[0]), {}), lambda *a: 4 * rows * n * per_row, jsg.istft_launch, check, torch.float32)

        least = (n - 1) // hop + 1          # the frames that overlap one sample: one new frame per chunk
        return work(23, least + extra, 60 + hop), work(31, least + extra + 5, 70 + hop)
    return factory


for _hop in (128, 441):
    for _extra in (0, 3):
        case(f"istft-hop{_hop}-{'smallest' if _extra == 0 else 'three-frames-more'}", 16)(istft_case(_hop, _extra))


# ---------------------------------------------------------------------------------------------------------------- libjsg: pvoc
def pvoc_case(rate, chunk):
    def factory(jsg, torch):
        n, hop, rows = 512, 128, 2

        def work(T, seed):
            X = np.stack([pv.make_input(n, hop, T, seed=seed + r) for r in range(rows)])
            d_X = torch.from_numpy(X).cuda()
            T_out = jsg.pvoc_frames(T, rate)
            assert T_out > chunk
            alloc = lambda: (torch.full((rows, T_out, n // 2 + 1), complex(SENTINEL, 3.5e-9), dtype=torch.complex64, device="cuda"),)
            size = lambda *a, **kw: jsg.capi.lib().jsg_pvoc_scratch_bytes(ctypes.byref(jsg.spectrogram._pvoc_args(*a, chunk)))

            def check(got):      # the three assertions of tests/test_gpu_pvoc.py::test_accuracy_against_float64, row by row
                for r in range(rows):
                    f = pv.accuracy_figures(X[r], got[0][r], rate, hop, n)
                    assert f["worst"] <= pv.YARDSTICKS * f["yardstick"] and f["cap_ratio"] <= 1.0 and f["n_zero"] > 0 and f["zeros_exact"], (r, f)

            return Work(torch, alloc, lambda outs: ((d_X, rate, hop, n, outs[0]), {}), size,
                        functools.partial(jsg.phase_vocoder_launch, chunk_frames=chunk), check)

        return work(9, 0), work(14, 5)
    return factory


for _rate in (1.3, 0.5):
    for _chunk in (4, 1):
        case(f"phase_vocoder-rate{_rate}-chunk{_chunk}", 16)(pvoc_case(_rate, _chunk))


# ---------------------------------------------------------------------------------------------------------------- libjsg: hpss
def hpss_case(K, real, W):
    def factory(jsg, torch):
        rows, chunk = 2, 16

        def work(T, seed):
            X = np.stack([hr.power(hr.make_input(T, K, seed + r)) if real else hr.make_input(T, K, seed + r) for r in range(rows)])
            want = tuple(np.stack(planes) for planes in zip(*(hr.mirror(X[r], *W)[:4] for r in range(rows))))
            d_X = torch.from_numpy(X).cuda()
            new = lambda dtype: torch.full(d_X.shape, SENTINEL, dtype=dtype, device="cuda")
            alloc = lambda: (new(torch.float32), new(torch.float32), new(d_X.dtype), new(d_X.dtype))
            bind = lambda o: ((d_X,), dict(d_mask_h=o[0], d_mask_p=o[1], d_harm=o[2], d_perc=o[3], kernel_size=W, chunk_frames=chunk))
            return Work(torch, alloc, bind, jsg.hpss_scratch_bytes, jsg.hpss_launch, lambda got: th.check_all(got, want))

        return work(70, 0), work(83, 10)
    return factory


for _K, _real, _W in ((70, False, (31, 31)), (70, True, (1, 63)), (65, False, (1, 63)), (65, True, (31, 31))):      # K = 65: a tile of bins partly dead
    case(f"hpss-K{_K}-{'real' if _real else 'complex'}-windows{_W[0]}x{_W[1]}", 16)(hpss_case(_K, _real, _W))


# ---------------------------------------------------------------------------------------------------------------- libjsgx: beat
BEAT_PERIODS = (7, 16, 33, 100, 200, 255, 511)          # 64, 32, 16, 8, 4 and 2 lanes per frame, and one lane per frame


def test_the_beat_periods_cover_every_lane_split_form():
    assert set(BEAT_PERIODS) <= set(br.FORM_PERIODS)
    assert [br.form(P)[1] for P in BEAT_PERIODS[:-1]] == [64, 32, 16, 8, 4, 2] and BEAT_PERIODS[-1] >= 511
    assert {br.form(P)[1] for P in br.FORM_PERIODS if P < 511} == {64, 32, 16, 8, 4, 2}


def beat_case(P, smooth):
    def factory(jsg, torch):
        d_log = torch.from_numpy(jsg.beat_log_table()).cuda()

        def work(T):
            o = np.stack([br.envelope("random", T, P), br.envelope("random", T, P + 1), br.envelope("train", T, P)]).copy()
            o[1, T // 2] = np.nan                                   # a NaN row between good rows
            want = [br.beat32(row, P, smooth=smooth) for row in o]
            assert want[1]["n"] == -1 and want[0]["n"] >= 1
            d_in = torch.from_numpy(o).cuda()
            ints = lambda *shape: torch.full(shape, ISENTINEL, dtype=torch.int32, device="cuda")
            floats = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda")
            alloc = lambda: (ints(3, T), ints(3), floats(3, T), floats(3, T))
            bind = lambda b: ((d_in, d_log, b[0], b[1]), dict(period=P, smooth=smooth, d_local_score=b[2], d_cum_score=b[3]))
            return Work(torch, alloc, bind, jsg.beat_scratch_bytes, jsg.beat_launch, lambda got: tb.check_rows(got, want, (P, T, smooth)))

        # 300 frames; at P = 511 a look-back is 256 frames or more, so that every link of 300 frames is the -1 that the fill 0xFF holds too
        T = 300 if P < 511 else 2 * P + 78
        return work(T), work(T + 117)
    return factory


for _P in BEAT_PERIODS:
    for _smooth in (False, True):
        case(f"beat-period{_P}-smooth{int(_smooth)}", 4)(beat_case(_P, _smooth))


# ---------------------------------------------------------------------------------------------------------------- libjsgx: dtw, rqa
def dtw_case(subseq, band):
    def factory(jsg, torch):
        def work(N, M, seed):
            costs = [dr.float_costs(N, M, seed), dr.integer_costs(N, M, seed + 1), dr.float_costs(N, M, seed + 2)]
            wants = []
            for C in costs:
                D = dr.dtw32(C, None, None, subseq, band)
                wants.append((C, D) + tuple(dr.backtrace32(D, C, None, None, subseq)))
            assert all(w[2] is not None for w in wants)
            if band:
                assert np.isinf(wants[0][1][64:, :64]).all()       # whole tiles lie outside the band
            d_cost = torch.from_numpy(np.stack(costs)).cuda()
            L = N + M - 1
            alloc = lambda: (torch.full((3, N, M), SENTINEL, dtype=torch.float32, device="cuda"), torch.full((3, L), ISENTINEL, dtype=torch.int32, device="cuda"),
                             torch.full((3, L), ISENTINEL, dtype=torch.int32, device="cuda"), torch.full((3,), ISENTINEL, dtype=torch.int32, device="cuda"),
                             torch.full((3,), SENTINEL, dtype=torch.float32, device="cuda"))
            bind = lambda o: ((d_cost, o[0]), dict(subseq=subseq, band=band, d_path_i=o[1], d_path_j=o[2], d_path_len=o[3], d_total=o[4]))

            def check(got):
                for p in range(3):
                    td.check_pair(got, p, wants[p], (N, M, subseq, band, p))

            return Work(torch, alloc, bind, jsg.dtw_scratch_bytes, jsg.dtw_launch, check)

        return work(65, 130, 100), work(70, 140, 200)
    return factory


case("dtw-global", 4)(dtw_case(False, 0))
case("dtw-subseq", 4)(dtw_case(True, 0))
case("dtw-band2-whole-tiles-outside", 4)(dtw_case(False, 2))


def rqa_case(knight):
    def factory(jsg, torch):
        def work(N, M, seed):
            planes = [rr.float_links(N, M, seed), np.zeros((N, M), np.float32), rr.integer_links(N, M, seed + 1)]      # no tile of the second has a best cell
            wants = [tr.reference_of(R, 0.5, 0.25, knight) for R in planes]
            assert len(wants[1][3]) == 0 and len(wants[0][3]) > 1
            d_sim = torch.from_numpy(np.stack(planes)).cuda()
            L = min(N, M)
            ints = lambda *shape: torch.full(shape, ISENTINEL, dtype=torch.int32, device="cuda")
            alloc = lambda: (torch.full((3, N, M), SENTINEL, dtype=torch.float32, device="cuda"), torch.full((3, N, M), int(tr.BSENTINEL), dtype=torch.int8, device="cuda"),
                             ints(3, L), ints(3, L), ints(3), ints(3, 2), torch.full((3,), SENTINEL, dtype=torch.float32, device="cuda"))
            bind = lambda o: ((d_sim, o[0]), dict(gap_onset=0.5, gap_extend=0.25, knight_moves=knight, d_step=o[1], d_path_i=o[2], d_path_j=o[3],
                                                  d_path_len=o[4], d_end=o[5].view(-1), d_total=o[6]))

            def check(got):
                for p in range(3):
                    tr.check_pair(got, p, wants[p], (N, M, knight, p))

            return Work(torch, alloc, bind, jsg.rqa_scratch_bytes, jsg.rqa_launch, check)

        return work(65, 130, 300), work(70, 140, 400)
    return factory


case("rqa-diagonal-steps", 4)(rqa_case(False))
case("rqa-knight-moves", 4)(rqa_case(True))


# ---------------------------------------------------------------------------------------------------------------- libjsgx: viterbi, pyin_decode
DECODE_FRAMES = 2 * 256 + 1          # three blocks of the backtrace, the last of one frame


def viterbi_case(S, W):
    def factory(jsg, torch):
        assert jsg.capix.VITERBI_BLOCK == 256

        def work(T, seed):
            b0, p0, A = vr.inputs("floats", T, S, seed, band_half=W)
            emits = [b0, vr.inputs("eighths", T, S, seed, band_half=W)[0], vr.inputs("floats", T, S, seed + 1, band_half=W)[0]]
            wants = []
            for b in emits:
                V, _, states, logp = vr.viterbi32(b, p0, A, band_half=W)
                wants.append((b, p0, A, V, states, logp))
            d_emit, d_init, d_trans = torch.from_numpy(np.stack(emits)).cuda(), torch.from_numpy(np.array(p0)).cuda(), torch.from_numpy(np.array(A)).cuda()
            alloc = lambda: (torch.full((3, T, S), SENTINEL, dtype=torch.float32, device="cuda"), torch.full((3, T), ISENTINEL, dtype=torch.int32, device="cuda"),
                             torch.full((3,), SENTINEL, dtype=torch.float32, device="cuda"))
            bind = lambda o: ((d_emit, d_init, d_trans, o[1]), dict(band_half=W, d_logp=o[2], d_value=o[0]))

            def check(got):
                for q in range(3):
                    tv.check_seq(got, q, wants[q], (T, S, W, q))

            return Work(torch, alloc, bind, jsg.viterbi_scratch_bytes, jsg.viterbi_launch, check)

        return work(DECODE_FRAMES, 500), work(DECODE_FRAMES + 40, 600)
    return factory


case("viterbi-dense-7-states", 4)(viterbi_case(7, None))
case("viterbi-dense-193-states", 4)(viterbi_case(193, None))
case("viterbi-band-65-states-half-30", 4)(viterbi_case(65, 30))


def pyin_case(P, W):
    def factory(jsg, torch):
        def work(T, seed):
            inp = py.decode_inputs("floats", T, P, W, seed)
            emits = [inp[0], py.decode_inputs("eighths", T, P, W, seed)[0], py.decode_inputs("floats", T, P, W, seed + 1)[0]]
            wants = []
            for b in emits:
                V, _, states, logp = py.decode32(b, *inp[1:])
                wants.append((inp, V, states, logp))
            d_emit = torch.from_numpy(np.stack(emits)).cuda()
            d_tab = [torch.from_numpy(np.array(a)).cuda() for a in inp[1:]]
            alloc = lambda: (torch.full((3, T, 2 * P), SENTINEL, dtype=torch.float32, device="cuda"), torch.full((3, T), ISENTINEL, dtype=torch.int32, device="cuda"),
                             torch.full((3,), SENTINEL, dtype=torch.float32, device="cuda"))
            bind = lambda o: ((d_emit, *d_tab, o[1]), dict(d_logp=o[2], d_value=o[0]))

            def check(got):
                for q in range(3):
                    ty.check_seq(got, q, wants[q], (T, P, W, q))

            return Work(torch, alloc, bind, jsg.pyin_decode_scratch_bytes, jsg.pyin_decode_launch, check)

        return work(DECODE_FRAMES, 700), work(DECODE_FRAMES + 40, 800)
    return factory


case("pyin_decode-7-bins-half-2", 4)(pyin_case(7, 2))
case("pyin_decode-129-bins-half-50", 4)(pyin_case(129, 50))


# ---------------------------------------------------------------------------------------------------------------- libjsgx: knn
def knn_case(k, split, width):
    def factory(jsg, torch):
        def work(N, M, seed):
            pairs = [kr.frames(kind, N, M, 6, seed + i) for i, kind in enumerate(("floats", "integers", "floats"))]
            wants = [(X, Y) + tuple(kr.knn32(X, Y, k, width, "euclidean")) for X, Y in pairs]
            d_x, d_y = (torch.from_numpy(np.stack([p[i] for p in pairs])).cuda() for i in (0, 1))
            alloc = lambda: (torch.full((3, N, k), ISENTINEL, dtype=torch.int32, device="cuda"), torch.full((3, N, k), SENTINEL, dtype=torch.float32, device="cuda"))
            bind = lambda o: ((d_x, d_y, o[0], o[1]), dict(width=width, split=split))

            def check(got):
                for p in range(3):
                    tk.check(got, p, wants[p], (N, M, k, split, width, p))

            return Work(torch, alloc, bind, jsg.knn_scratch_bytes, jsg.knn_launch, check)

        assert jsg.knn_plan(70, 130, 6, k, 3, split=split)[2] == split      # 130 columns are three tiles: the third piece of a split in three holds two
        return work(70, 130, 900), work(75, 150, 950)
    return factory


for _k in (5, 65):
    for _split in (2, 3):
        for _width in (0, 2):
            case(f"knn-k{_k}-split{_split}-width{_width}", 4)(knn_case(_k, _split, _width))


# ---------------------------------------------------------------------------------------------------------------- libjsgx: nmf, pcen, peak
@case("nmf-257-frames-257-bins-5-components", 4)
def nmf_case(jsg, torch):
    r, n_iter = 5, 2

    def work(T, K, seed):
        problems = [nr.problem(T, K, r, seed), nr.problem(T, K, r, seed + 1)]
        wants = [nr.nmf32(V, A0, C0, n_iter, True) for V, A0, C0 in problems]
        d_v = torch.from_numpy(np.stack([p[0] for p in problems])).cuda()
        alloc = lambda: tuple(torch.from_numpy(np.stack([p[i] for p in problems])).cuda() for i in (1, 2))      # A and C are updated in place
        bind = lambda o: ((d_v, o[0], o[1]), dict(n_iter=n_iter))

        def check(got):
            for p in range(2):
                tn.check(got[0][p], wants[p][0], (T, K, p, "A"))
                tn.check(got[1][p], wants[p][1], (T, K, p, "C"))

        return Work(torch, alloc, bind, jsg.nmf_scratch_bytes, jsg.nmf_launch, check)

    assert nr.CHUNK_T == nr.CHUNK_K == 256          # two chunks each way, the second one element long
    return work(257, 257, 0), work(300, 290, 7)


@case("pcen-513-frames-state-in", 4)
def pcen_case(jsg, torch):
    R, B, params = 2, 40, tc.DEFAULTS
    d_decay = torch.from_numpy(jsg.pcen_decay(params["b"])).cuda()

    def work(T, seed):
        M = pc.plane(T, B, seed, rows=R)
        state = pc.plane(1, B, seed + 1, rows=R)[:, 0, :]
        want = pc.pcen32(M, state=state, **params)
        d_in, d_state = torch.from_numpy(M).cuda(), torch.from_numpy(np.ascontiguousarray(state)).cuda()
        new = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda")
        alloc = lambda: (new(R, T, B), new(R, T, B), new(R, B))
        bind = lambda o: ((d_in, d_decay, o[0]), dict(params, d_state_in=d_state, d_smooth=o[1], d_state_out=o[2]))
        return Work(torch, alloc, bind, jsg.pcen_scratch_bytes, jsg.pcen_launch, lambda got: tc.check_all(got, want, (T, "state in")))

    assert pc.CHUNK == 256          # three chunks, the last of one frame
    return work(513, 0), work(770, 5)


@case("peak-two-blocks-and-five-frames-long-wait-backtracking", 4)
def peak_case(jsg, torch):
    R, params = 2, dict(pk.DEFAULT, wait=pk.BLOCK + 1)

    def work(T, seed):
        X, E = pk.quantised(T, seed, R), np.array(pk.smooth(T, seed + 1, R), np.float32)
        want = tp.expected(X, energy=E, **params)
        assert all(w[0] >= 2 for w in want)
        d_in, d_energy = torch.from_numpy(X).cuda(), torch.from_numpy(E).cuda()
        ints = lambda *shape: torch.full(shape, tp.INT_SENTINEL, dtype=torch.int32, device="cuda")
        alloc = lambda: (ints(R), ints(R, T), ints(R, T), torch.full((R, T), tp.BYTE_SENTINEL, dtype=torch.uint8, device="cuda"))
        bind = lambda o: ((d_in, o[1], o[0]), dict(params, d_energy=d_energy, d_backtracked=o[2], d_candidate=o[3]))

        def check(got):
            n, peaks, backs, cand = got
            rows = []
            for r in range(R):
                kept = int(n[r])
                assert 0 <= kept <= T and (peaks[r, kept:] == tp.INT_SENTINEL).all() and (backs[r, kept:] == tp.INT_SENTINEL).all(), "written behind the list"
                rows.append((kept, peaks[r, :kept].tolist(), backs[r, :kept].tolist(), cand[r]))
            tp.check(rows, want, (T, "backtracking"))

        return Work(torch, alloc, bind, jsg.peak_scratch_bytes, jsg.peak_launch, check)

    return work(2 * pk.BLOCK + 5, 21), work(3 * pk.BLOCK + 7, 31)


# ---------------------------------------------------------------------------------------------------------------- the test
@functools.lru_cache(maxsize=None)
def built(jsg, torch, name):
    """The two launches of a case with their references, made once and shared by its four fills."""
    main, other = CASES[name][1](jsg, torch)
    assert 0 < main.need < other.need, (name, main.need, other.need)
    return main, other


FIRST = {}            # case -> the outputs of the first fill that ran


def test_every_launcher_has_a_case():
    for launcher in ("stft_fb_db", "stft_fb_db_strided", "istft", "phase_vocoder", "hpss", "beat", "dtw", "viterbi", "pyin_decode", "knn", "rqa", "nmf", "pcen", "peak"):
        assert any(name.split("-")[0] == launcher for name in CASES), launcher


@pytest.mark.parametrize("name, fill", [(name, fill) for name in CASES for fill in FILLS], ids=lambda v: v)
def test_outputs_do_not_depend_on_the_scratch_contents(jsg, torch_cuda, name, fill):
    torch = torch_cuda
    main, other = built(jsg, torch, name)
    scratch = Scratch(torch, other.need if fill == "stale" else main.need, CASES[name][0])
    scratch.fill(FILL_BYTE[fill])
    if fill == "stale":                     # the same launcher on a larger shape and other data, its scratch not refilled
        other.check(other.run(scratch))
    before = scratch.snapshot()
    got = main.run(scratch)
    print(f"{name}: need = {main.need} bytes (the larger shape: {other.need})")
    main.check(got)
    assert scratch.guards_hold(before, main.need), "a byte in front of the scratch or behind its stated size was written"
    assert scratch.changed(before, main.need), "the launch left its scratch as it was: the case does not reach it"
    first = FIRST.setdefault(name, got)
    assert all(same_bytes(a, b) for a, b in zip(got, first)), "the outputs differ in their bits from those of another fill"

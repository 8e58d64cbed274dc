"""YIN fundamental-frequency tracking on the GPU (include/jsg.h section 2i) against tests/yin_ref.py: graph capture of a first launch,
accuracy under both bounds in pitched buffers with sentinels, the lag on decided frames, f0 and aper recomputed to the bit from the
GPU's own d' plane, the shapes where the kernel changes its path, large frames, a launch of many items, 65 535 rows, identical bits
over chunk lengths, pitches, offsets, row counts and null outputs, NaN containment, silence, and the Python layer."""
import numpy as np
import pytest

import yin_ref as yr

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25e11)
T = yr.frames(yr.L, yr.W, yr.TAU_MAX, yr.HOP)
SHARED = dict(w=yr.W, lo=yr.TAU_MIN, hi=yr.TAU_MAX, hop=yr.HOP, thr=yr.THRESHOLD, sr=yr.SR)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def raw(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(raw(a), raw(b))


def run(jsg, torch, x, n_frames, *, w, lo, hi, hop, thr=yr.THRESHOLD, sr=yr.SR, outputs="fac", chunk_frames=0, pad_in=0, pad_out=0, pad_frame=0,
        pad_row=0, offset=0):
    """x numpy [rows][n] -> dict(f0, aper [rows][n_frames], cmnd [rows][n_frames][hi + 1]) of one launch; `outputs` names the ones that are
    given (f, a, c), the others are NULL.  Input rows lie pad_in floats apart beyond their length, f0 / aper rows pad_out, cmnd frames
    pad_frame and cmnd rows pad_row floats apart beyond theirs; every buffer starts `offset` floats into its allocation.  The input
    allocation holds NaN outside the rows.  Every output allocation is filled with a sentinel first, and every element of it that the
    launch must not write is checked to hold it still."""
    x = np.atleast_2d(x)
    R, n = x.shape
    b_in = torch.full((offset + R * (n + pad_in),), float("nan"), dtype=torch.float32, device="cuda")
    d_in = b_in[offset:].view(R, n + pad_in)[:, :n]
    d_in.copy_(torch.from_numpy(np.array(x)))
    lp = n_frames + pad_out
    lines = {}
    for key in "fa":
        if key in outputs:
            flat = torch.full((offset + R * lp + 3,), float(SENTINEL), dtype=torch.float32, device="cuda")
            lines[key] = (flat, torch.as_strided(flat, (R, n_frames), (lp, 1), storage_offset=offset))
    fp = hi + 1 + pad_frame
    rp = n_frames * fp + pad_row
    plane = None
    if "c" in outputs:
        flat = torch.full((offset + R * rp + 3,), float(SENTINEL), dtype=torch.float32, device="cuda")
        plane = (flat, torch.as_strided(flat, (R, n_frames, hi + 1), (rp, fp, 1), storage_offset=offset))
    view = lambda k: lines[k][1] if k in lines else None
    jsg.yin_launch(d_in, w, lo, hi, hop, n_frames, thr, sr, d_f0=view("f"), d_aper=view("a"), d_cmnd=plane[1] if plane else None, chunk_frames=chunk_frames)
    torch.cuda.synchronize()
    out = {}
    for key, name in (("f", "f0"), ("a", "aper")):
        if key in lines:
            got = lines[key][0].cpu().numpy()
            at = offset + np.arange(R)[:, None] * lp + np.arange(n_frames)[None, :]
            written = np.zeros(got.size, bool)
            written[at.ravel()] = True
            assert (got[~written] == SENTINEL).all(), name
            out[name] = got[at]
    if plane:
        got = plane[0].cpu().numpy()
        at = offset + np.arange(R)[:, None, None] * rp + np.arange(n_frames)[None, :, None] * fp + np.arange(hi + 1)[None, None, :]
        written = np.zeros(got.size, bool)
        written[at.ravel()] = True
        assert (got[~written] == SENTINEL).all(), "cmnd"
        out["cmnd"] = got[at]
    return out


_tight = {}


def tight(jsg, torch):
    """The GPU's result of the shared signals in tight buffers with the default chunk, computed once."""
    if not _tight:
        _tight.update(run(jsg, torch, yr.signals(), T, **SHARED))
    return _tight


def check(out, ref, *, lo, hi, thr, sr, what=""):
    """Cap (b) on d', bound (a) per row, f0 and aper to the bit from the GPU's own d', the lag and the f0 error on decided frames; prints the
    figures first."""
    cm, f0, aper = out["cmnd"], out["f0"], out["aper"]
    R, n_frames = f0.shape
    e_gpu, e_ref = yr.cap_units(cm, ref), yr.cap_units(ref["dp32"], ref)
    differ = int((raw(cm) != raw(ref["dp32"])).sum())
    ok = ref["decided"]
    lag = np.zeros((R, n_frames), np.int64)
    own = True
    for r in range(R):
        for t in range(n_frames):
            tau, _, f, a = yr.select(cm[r, t], lo, hi, thr, sr)
            own = own and same(np.float32(f).reshape(1), f0[r, t].reshape(1)) and same(np.float32(a).reshape(1), aper[r, t].reshape(1))
            lag[r, t] = tau
            if ok[r, t]:
                assert yr.implied_lag(f0[r, t], aper[r, t], cm[r, t], sr, lo, hi) == ref["tau64"][r, t], (what, r, t)
    f_gpu = np.array([np.abs(f0[r][ok[r]].astype(np.float64) - ref["f064"][r][ok[r]]).max(initial=0.0) for r in range(R)])
    f_ref = np.array([np.abs(ref["f032"][r][ok[r]].astype(np.float64) - ref["f064"][r][ok[r]]).max(initial=0.0) for r in range(R)])
    print(f"{what}: d' error in units of cap (b), GPU {e_gpu}, restatement {e_ref}; f0 error on decided frames, GPU {f_gpu}, restatement {f_ref}; "
          f"{differ} of {cm.size} d' differ in bits from the restatement; {int(ok.sum())} of {ok.size} frames decided")
    assert (np.abs(cm.astype(np.float64) - ref["dp64"]) <= ref["cap"]).all(), e_gpu
    assert (e_gpu <= yr.YARDSTICKS * e_ref).all(), (e_gpu, e_ref)
    assert own, "f0 / aper are not what steps 3 to 5 give on the GPU's own d'"
    assert (lag[ok] == ref["tau64"][ok]).all()
    assert (f_gpu <= yr.YARDSTICKS * f_ref).all(), (f_gpu, f_ref)


def test_graph_capture_of_a_first_launch(jsg, torch_cuda):
    """The first launch of the two-lags-per-lane path in this process (this test comes first in the file and no other file launches YIN)
    sits inside a capture; replayed twice, equals eager."""
    torch = torch_cuda
    kw = dict(w=100, lo=3, hi=100, hop=50)
    x = np.array(yr.signals()[:3, :1000])
    n_frames = yr.frames(1000, 100, 100, 50)
    d_in = torch.from_numpy(x).cuda()
    d_f0, d_aper = (torch.zeros((3, n_frames), dtype=torch.float32, device="cuda") for _ in range(2))
    d_cm = torch.zeros((3, n_frames, 101), dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=s):
        jsg.yin_launch(d_in, 100, 3, 100, 50, n_frames, yr.THRESHOLD, yr.SR, d_f0=d_f0, d_aper=d_aper, d_cmnd=d_cm, stream=s.cuda_stream)
    eager = run(jsg, torch, x, n_frames, **kw)
    assert jsg.yin_kernel_name(d_in, 100, 3, 100, 50, n_frames, yr.THRESHOLD, yr.SR, d_f0=d_f0) == "yin_lags2"
    for _ in range(2):
        for d in (d_f0, d_aper, d_cm):
            d.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert same(d_f0.cpu().numpy(), eager["f0"]) and same(d_aper.cpu().numpy(), eager["aper"]) and same(d_cm.cpu().numpy(), eager["cmnd"])
    check(eager, yr.evaluate(x, 100, 3, 100, 50, n_frames, yr.THRESHOLD, yr.SR), lo=3, hi=100, thr=yr.THRESHOLD, sr=yr.SR, what="w 100, lags 3..100")


def test_first_launch_of_a_path_with_more_than_48_kib_of_lds(jsg, torch_cuda):
    """The first launch of the eight-lags-per-lane path in this process (only the capture above precedes it, on another path) asks for
    more dynamic LDS than a kernel may have without saying so: the launch itself has to say it."""
    size, hi, n_frames, hop = 8192, 2048, 2, 100
    n = (n_frames - 1) * hop + size + hi
    x = (0.4 * np.sin(2 * np.pi * np.arange(n) / 97.3) + 0.05 * np.random.default_rng(size).standard_normal(n)).astype(np.float32)[None]
    d_x, d_f0 = torch_cuda.zeros((1, n), device="cuda"), torch_cuda.zeros((1, n_frames), device="cuda")
    name, _, lds = jsg.yin_plan(d_x, size, 50, hi, hop, n_frames, 0.2, 48000.0, d_f0=d_f0)
    assert name == "yin_lags8" and lds > 49152, (name, lds)
    ref = yr.evaluate(x, size, 50, hi, hop, n_frames, 0.2, 48000.0)
    out = run(jsg, torch_cuda, x, n_frames, w=size, lo=50, hi=hi, hop=hop, thr=0.2, sr=48000.0, offset=1)
    check(out, ref, lo=50, hi=hi, thr=0.2, sr=48000.0, what=f"w {size}, tau_max {hi}, first on its path")
    assert ref["decided"].all() and (np.abs(ref["tau64"] - 97) <= 1).all()
    again = run(jsg, torch_cuda, x, n_frames, w=size, lo=50, hi=hi, hop=hop, thr=0.2, sr=48000.0, chunk_frames=1)
    assert all(same(again[k], out[k]) for k in out)


def test_accuracy_pitched_rows_at_an_odd_offset(jsg, torch_cuda):
    out = run(jsg, torch_cuda, yr.signals(), T, pad_in=5, pad_out=3, pad_frame=3, pad_row=7, offset=1, **SHARED)
    assert out["cmnd"].shape == (6, T, yr.TAU_MAX + 1) and out["f0"].shape == (6, T)
    check(out, yr.shared(), lo=yr.TAU_MIN, hi=yr.TAU_MAX, thr=yr.THRESHOLD, sr=yr.SR, what="shared signals")
    for key in ("f0", "aper", "cmnd"):
        assert same(out[key], tight(jsg, torch_cuda)[key]), key
    i = yr.NAMES.index("silence")
    assert (out["cmnd"][i] == 1).all() and (out["f0"][i] == np.float32(yr.SR) / np.float32(yr.TAU_MIN)).all() and (out["aper"][i] == 1).all()
    voiced = out["aper"][yr.NAMES.index("tone")] < yr.THRESHOLD
    assert voiced.all() and (np.abs(out["f0"][yr.NAMES.index("tone")] / 220.0 - 1.0) <= 0.005).all()
    assert (np.abs(out["f0"][yr.NAMES.index("pulses")] / (yr.SR / yr.PULSE_PERIOD) - 1.0) <= 0.005).all()


@pytest.mark.parametrize("w", [1, 63, 64, 65, 256, 1000])
def test_shapes_where_the_kernel_changes_its_path(jsg, torch_cuda, w):
    """Every tau_max around the lane blocks against every hop (the last one larger than the span: the frames lie back to back in LDS),
    tau_min = 1; at hop 7 also tau_min = tau_max."""
    rng = np.random.default_rng(w)
    for hi in (1, 2, 63, 64, 65, 200, 1000):
        for hop in (1, 7, 64, 5000):
            n_frames = 5 if hop < 5000 else 3
            n = (n_frames - 1) * hop + w + hi + 2
            x = np.zeros((2, n), np.float32)
            x[0] = rng.standard_normal(n).astype(np.float32)
            x[1] = (0.5 * np.sin(2 * np.pi * np.arange(n) / 23.5)).astype(np.float32)
            assert yr.frames(n, w, hi, hop) >= n_frames          # the two samples past the last frame are none of its business
            for lo in ((1, hi) if hop == 7 else (1,)):
                ref = yr.evaluate(x, w, lo, hi, hop, n_frames, 0.15, 4000.0)
                out = run(jsg, torch_cuda, x, n_frames, w=w, lo=lo, hi=hi, hop=hop, thr=0.15, sr=4000.0, pad_frame=1, pad_out=1)
                check(out, ref, lo=lo, hi=hi, thr=0.15, sr=4000.0, what=f"w {w}, lags {lo}..{hi}, hop {hop}")


@pytest.mark.parametrize("size,n_frames,hop", [(8192, 2, 100), (2048, 8, 300)])
def test_large_frames(jsg, torch_cuda, size, n_frames, hop):
    n = (n_frames - 1) * hop + 2 * size
    rng = np.random.default_rng(size)
    x = (0.4 * np.sin(2 * np.pi * np.arange(n) / 97.3) + 0.05 * rng.standard_normal(n)).astype(np.float32)[None]
    ref = yr.evaluate(x, size, 50, size, hop, n_frames, 0.2, 48000.0)
    out = run(jsg, torch_cuda, x, n_frames, w=size, lo=50, hi=size, hop=hop, thr=0.2, sr=48000.0, offset=1)
    check(out, ref, lo=50, hi=size, thr=0.2, sr=48000.0, what=f"w = tau_max = {size}")
    assert ref["decided"].any() and (np.abs(ref["tau64"][ref["decided"]] - 97) <= 1).all()
    for chunk in (1, 3):
        again = run(jsg, torch_cuda, x, n_frames, w=size, lo=50, hi=size, hop=hop, thr=0.2, sr=48000.0, chunk_frames=chunk)
        assert all(same(again[k], out[k]) for k in out), chunk


def test_many_items_in_one_launch(jsg, torch_cuda):
    """8 rows x 1200 frames at chunk_frames = 1: 9600 work items, several times the grid."""
    kw = dict(w=4, lo=1, hi=5, hop=3, thr=0.3, sr=100.0)
    n_frames = 1200
    n = (n_frames - 1) * 3 + 9
    x = np.random.default_rng(8).standard_normal((8, n)).astype(np.float32)
    props = torch_cuda.cuda.get_device_properties(0)
    assert 8 * n_frames >= 3 * 8 * props.multi_processor_count
    out = run(jsg, torch_cuda, x, n_frames, chunk_frames=1, **kw)
    other = run(jsg, torch_cuda, x, n_frames, pad_frame=2, pad_out=1, **kw)
    assert all(same(other[k], out[k]) for k in out)
    check(out, yr.evaluate(x, 4, 1, 5, 3, n_frames, 0.3, 100.0), lo=1, hi=5, thr=0.3, sr=100.0, what="tiny frames, chunk 1")


def test_bits_do_not_depend_on_the_row_count(jsg, torch_cuda):
    kw = dict(w=4, lo=1, hi=5, hop=3, thr=0.3, sr=100.0)
    base = np.array(yr.signals()[:3, 1000:1009])
    three = run(jsg, torch_cuda, base, 1, **kw)
    check(three, yr.evaluate(base, 4, 1, 5, 3, 1, 0.3, 100.0), lo=1, hi=5, thr=0.3, sr=100.0, what="one frame of 9 samples")
    for r in range(3):
        one = run(jsg, torch_cuda, base[r], 1, **kw)
        assert all(same(one[k], three[k][r:r + 1]) for k in three)
    many = run(jsg, torch_cuda, np.tile(base, (21845, 1)), 1, pad_in=1, **kw)
    assert many["f0"].shape[0] == 65535
    assert same(many["f0"], np.tile(three["f0"], (21845, 1))) and same(many["aper"], np.tile(three["aper"], (21845, 1)))
    assert same(many["cmnd"], np.tile(three["cmnd"], (21845, 1, 1)))


def test_bits_do_not_depend_on_the_chunk_the_pitches_or_the_outputs(jsg, torch_cuda):
    want = tight(jsg, torch_cuda)
    for chunk in (1, 2, 3, 17, T + 5, 65536):
        out = run(jsg, torch_cuda, yr.signals(), T, chunk_frames=chunk, pad_in=chunk % 7, pad_out=chunk % 4, pad_frame=chunk % 5, pad_row=chunk % 3, offset=chunk % 2, **SHARED)
        assert all(same(out[k], want[k]) for k in want), chunk
    names = dict(f="f0", a="aper", c="cmnd")
    for outputs in ("f", "a", "c", "fa", "fc", "ac"):
        out = run(jsg, torch_cuda, yr.signals(), T, outputs=outputs, pad_out=1, **SHARED)
        assert sorted(out) == sorted(names[k] for k in outputs) and all(same(out[k], want[k]) for k in out), outputs
    # fewer frames than the row holds: the first frames, the same bits
    out = run(jsg, torch_cuda, yr.signals(), T - 7, **SHARED)
    assert all(same(out[k], want[k][:, :T - 7]) for k in out)


def test_nan_is_contained(jsg, torch_cuda):
    clean = tight(jsg, torch_cuda)
    span = yr.W + yr.TAU_MAX
    for m0 in (0, 1499, yr.L - 1, (T - 1) * yr.HOP + span - 1):
        x = np.array(yr.signals())
        x[1, m0] = np.nan
        out = run(jsg, torch_cuda, x, T, **SHARED)
        start = np.arange(T) * yr.HOP
        hit = (start <= m0) & (m0 < start + span)
        assert (hit.any() or m0 == yr.L - 1) and not hit.all()
        for r in (0, 2, 3, 4, 5):
            assert all(same(out[k][r], clean[k][r]) for k in out)
        assert np.isnan(out["f0"][1][hit]).all() and np.isnan(out["aper"][1][hit]).all() and np.isnan(out["cmnd"][1][hit][:, yr.TAU_MAX]).all()
        assert all(same(out[k][1][~hit], clean[k][1][~hit]) for k in out)


def test_python_layer(jsg, torch_cuda):
    torch = torch_cuda
    sr, fmin, fmax, frame = 8000.0, 40.0, 1000.0, 512
    lo, hi = 8, 200
    w = frame - hi
    x = np.array(yr.signals()[:4])
    f0, ap = jsg.yin(x, sr, fmin, fmax, frame_length=frame, center=False)                 # numpy in, numpy out; hop = 128
    n_frames = yr.frames(yr.L, w, hi, 128)
    assert isinstance(f0, np.ndarray) and f0.dtype == np.float32 and f0.shape == ap.shape == (4, n_frames)
    direct = run(jsg, torch, x, n_frames, w=w, lo=lo, hi=hi, hop=128, thr=0.1, sr=sr)
    assert same(f0, direct["f0"]) and same(ap, direct["aper"])
    check(direct, yr.evaluate(x, w, lo, hi, 128, n_frames, 0.1, sr), lo=lo, hi=hi, thr=0.1, sr=sr, what="yin(), frame 512")
    assert (np.abs(f0[0] / 220.0 - 1.0) <= 0.005).all() and (ap[0] < 0.1).all() and (ap[2] > 0.1).all()
    xt = torch.from_numpy(x).cuda()
    g0, gp = jsg.yin(xt, sr, fmin, fmax, frame_length=frame, center=False)
    assert g0.is_cuda and same(g0.cpu().numpy(), f0) and same(gp.cpu().numpy(), ap)
    # center: frame_length // 2 zeros at both ends
    c0, cp = jsg.yin(xt, sr, fmin, fmax, frame_length=frame, hop_length=64, threshold=0.2)
    padded = np.pad(x, ((0, 0), (frame // 2, frame // 2)))
    p0, pp = jsg.yin(padded, sr, fmin, fmax, frame_length=frame, hop_length=64, threshold=0.2, center=False)
    assert c0.shape == (4, 1 + yr.L // 64) and same(c0.cpu().numpy(), p0) and same(cp.cpu().numpy(), pp)
    # batch dimensions and one-dimensional input
    b0, bp = jsg.yin(xt.reshape(2, 2, -1), sr, fmin, fmax, frame_length=frame, center=False)
    assert b0.shape == (2, 2, n_frames) and same(b0.reshape(4, -1).cpu().numpy(), f0) and same(bp.reshape(4, -1).cpu().numpy(), ap)
    o0, op = jsg.yin(xt[1], sr, fmin, fmax, frame_length=frame, center=False)
    assert o0.shape == (n_frames,) and same(o0.cpu().numpy(), f0[1]) and same(op.cpu().numpy(), ap[1])
    # the d' plane, and its way through db_from_power and colormap
    plane = jsg.yin_cmnd(xt, sr, fmin, fmax, frame_length=frame, center=False)
    assert plane.shape == (4, n_frames, hi + 1) and same(plane.cpu().numpy(), direct["cmnd"])
    assert same(jsg.yin_cmnd(x[1], sr, fmin, fmax, frame_length=frame, center=False), direct["cmnd"][1])
    one = plane[1].contiguous()
    db = torch.empty_like(one)
    jsg.spectrogram.db_from_power(one, db)
    torch.cuda.synchronize()
    want = 10.0 * np.log10(direct["cmnd"][1].astype(np.float64) + 1e-11)
    assert np.abs(db.cpu().numpy() - want).max() <= 1e-3
    d_lut = torch.from_numpy(jsg.colormap_lut(256, 6)).cuda()
    img = torch.zeros((hi + 1, n_frames), dtype=torch.int32, device="cuda")
    jsg.colormap(db, d_lut, -30.0, 3.0, d_argb=img)
    torch.cuda.synchronize()
    assert len(np.unique(img.cpu().numpy())) > 8
    with pytest.raises(jsg.JsgError):
        jsg.yin(xt, sr, 10.0, fmax, frame_length=frame)                  # tau_max = 800 leaves no window in 512

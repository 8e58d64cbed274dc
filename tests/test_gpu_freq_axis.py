"""Display frequency axes on the MI355X (include/jsg.h, section 2c): jsg_colormap_axis_launch and the engine's display over an axis,
pixel for pixel against a model built from the library's own row table (jsg_freq_axis_build), section 2c's pixel rule in float32 numpy
(NaN -> palette index 0) and the oracle's palette (OracleColorPalette, render_all)."""
import ctypes
import json
import subprocess

import numpy as np
import pytest

from test_freq_axis_host import build_cpp_driver

pytestmark = pytest.mark.gpu

FS = 48000.0
SENTINEL = np.uint32(0x12345678)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


# ---------------------------------------------------------------------------------------------------------------------------------
# model
# ---------------------------------------------------------------------------------------------------------------------------------
def axis_values(db, axis):
    """[W][height] float32 row values of the dB columns db [W][>= n/2+1] (section 2c)."""
    first, count, t, _ = axis.rows()
    db = np.asarray(db, np.float32)
    W, H = db.shape[0], first.size
    out = np.empty((W, H), np.float32)
    red = np.flatnonzero(count > 0)
    if red.size:
        s0, e1 = int(first[red[0]]), int(first[red[-1]] + count[red[-1]])
        out[:, red] = np.maximum.reduceat(db[:, s0:e1], first[red] - s0, axis=1)   # np.maximum keeps a NaN
    with np.errstate(invalid="ignore"):                                    # inf - inf and 0 * inf are NaN, as on the GPU
        for r in np.flatnonzero(count == 0):
            a, b = db[:, first[r]], db[:, first[r] + 1]
            d = (b - a).astype(np.float32)
            p = (np.float32(t[r]) * d).astype(np.float32)
            out[:, r] = (a + p).astype(np.float32)
    return out


def palette_index(pal, v):
    return pal.index(np.where(np.isnan(v), pal.vmin, v))   # NaN: index 0, like v_cvt_i32_f32(NaN) in color_index


def axis_image(oracle, pal, db, axis, pos, running):
    """What the display draws for the whole ring: render_all over the mapped [W][height] ring."""
    v = axis_values(db, axis)
    return oracle.render_all(np.where(np.isnan(v), pal.vmin, v), pos, pal, running=running)


def db_columns(W, n, seed, specials=True):
    rng = np.random.default_rng(seed)
    H = n // 2 + 1
    db = rng.normal(-45.0, 25.0, (W, H)).astype(np.float32)
    db[:, rng.integers(0, H, 8)] += 60.0                                   # narrow tones
    if specials:
        db[3, :] = -110.0                                                  # silent column: the -110 dB floor
        db[5, rng.integers(0, H, 40)] = np.nan
        db[7, rng.integers(0, H, 40)] = np.inf
        db[8, rng.integers(0, H, 40)] = -np.inf
        db[9, :] = np.nan
        db[11, H // 3:H // 3 + 50] = np.inf
        db[11, H // 3 + 50:H // 3 + 100] = -np.inf
        db[12, :H // 2] = -np.inf
        db[12, H // 2:] = np.inf
    return db


def heights(n):
    return [h for h in (2, 37, 1080, n // 2 + 1, 4 * (n // 2 + 1)) if h <= 16384]


def run_launch(jsg, oracle, torch, db, axis, n_colors, scheme, lo, hi, *, col_first=0, n_cols=None, x_first=0, x_wrap=None,
               with_index=False, pitch_pad=0):
    W, H0 = db.shape
    n_cols = W if n_cols is None else n_cols
    x_wrap = W if x_wrap is None else x_wrap
    d_db = torch.full((W, H0 + pitch_pad), float("nan"), dtype=torch.float32, device="cuda")
    d_db[:, :H0] = torch.from_numpy(db).cuda()
    d_lut = torch.from_numpy(jsg.colormap_lut(n_colors, scheme)).cuda()
    d_img = torch.full((axis.height, x_wrap + 5), int(SENTINEL.view(np.int32)), dtype=torch.int32, device="cuda")
    d_idx = torch.full((axis.height, x_wrap), 77, dtype=torch.uint8, device="cuda") if with_index else None
    jsg.colormap_axis(d_db, d_lut, lo, hi, axis, d_argb=d_img[:, :x_wrap], d_index=d_idx, col_first=col_first, n_cols=n_cols,
                      x_first=x_first)
    torch.cuda.synchronize()
    img = d_img.cpu().numpy().view(np.uint32)
    pal = oracle.OracleColorPalette(n_colors, scheme)
    pal.set_value_range(lo, hi)
    idx = palette_index(pal, axis_values(db, axis))                        # [W][height]
    ref = np.full(img.shape, SENTINEL, np.uint32)
    ref_idx = np.full((axis.height, x_wrap), 77, np.uint8)
    for i in range(n_cols):
        c, x = (col_first + i) % W, (x_first + i) % x_wrap
        ref[::-1, x] = (pal.lut[idx[c]].astype(np.int64) | 0xFF000000).astype(np.uint32)
        ref_idx[::-1, x] = idx[c].astype(np.uint8)
    bad = int((img != ref).sum())
    assert bad == 0, f"{bad} of {img.size} pixels differ"
    if with_index:
        got = d_idx.cpu().numpy()
        assert (got == ref_idx).all(), f"{int((got != ref_idx).sum())} palette indices differ"
    return img


# ---------------------------------------------------------------------------------------------------------------------------------
# stateless launch
# ---------------------------------------------------------------------------------------------------------------------------------
AXES = {"linear": (1, 0.0, FS / 2), "linear_zoom": (1, 250.0, 4000.0), "log": (2, 20.0, 20000.0), "mel": (3, 0.0, FS / 2)}


@pytest.mark.parametrize("n", [512, 1024, 2048, 4096, 8192])
@pytest.mark.parametrize("axis_name", list(AXES))
def test_axis_launch_every_size_scale_and_height(jsg, oracle, torch_cuda, n, axis_name):
    scale, lo, hi = AXES[axis_name]
    db = db_columns(70, n, seed=n + scale)
    for k, h in enumerate(heights(n)):
        axis = jsg.FreqAxis(n, FS, h, lo, hi, scale)
        run_launch(jsg, oracle, torch_cuda, db, axis, 256, oracle.CM_JADE, -90.0, 10.0, with_index=(k % 2 == 0), pitch_pad=(k * 7) % 32)


@pytest.mark.parametrize("n_colors,scheme", [(256, 4), (1024, 6), (4096, 2), (64, 3)])
def test_axis_launch_ring_wrap_image_wrap_and_palettes(jsg, oracle, torch_cuda, n_colors, scheme):
    n = 2048
    db = db_columns(150, n, seed=n_colors)
    for scale, lo, hi, h in ((2, 30.0, 16000.0, 600), (1, 100.0, 900.0, 333), (3, 0.0, 24000.0, 128)):
        axis = jsg.FreqAxis(n, FS, h, lo, hi, scale)
        run_launch(jsg, oracle, torch_cuda, db, axis, n_colors, scheme, -80.0, 0.0, col_first=131, n_cols=100, x_first=57, x_wrap=140,
                   with_index=n_colors <= 256)
        run_launch(jsg, oracle, torch_cuda, db, axis, n_colors, scheme, 20.0, -60.0, col_first=10, n_cols=150, x_first=149, x_wrap=150)


@pytest.mark.parametrize("n", [512, 1024, 2048, 4096, 8192])
def test_identity_axis_equals_colormap_launch(jsg, oracle, torch_cuda, n):
    torch = torch_cuda
    H = n // 2 + 1
    db = db_columns(130, n, seed=3 * n)
    axis = jsg.FreqAxis(n, FS, H, 0.0, FS / 2, jsg.capi.AXIS_LINEAR)
    d_db = torch.from_numpy(db).cuda()
    d_lut = torch.from_numpy(jsg.colormap_lut(256, oracle.CM_JADE)).cuda()
    outs = []
    for use_axis in (False, True):
        d_img = torch.zeros((H, 130), dtype=torch.int32, device="cuda")
        d_idx = torch.zeros((H, 130), dtype=torch.uint8, device="cuda")
        kw = dict(d_argb=d_img, d_index=d_idx, col_first=40, n_cols=120, x_first=9)
        if use_axis:
            jsg.colormap_axis(d_db, d_lut, -70.0, 5.0, axis, **kw)
        else:
            jsg.colormap(d_db, d_lut, -70.0, 5.0, **kw)
        torch.cuda.synchronize()
        outs.append((d_img.cpu().numpy(), d_idx.cpu().numpy()))
    assert (outs[0][0] == outs[1][0]).all() and (outs[0][1] == outs[1][1]).all()


def test_axis_launch_graph_capture_replays(jsg, oracle, torch_cuda):
    torch = torch_cuda
    n, W = 4096, 200
    axis = jsg.FreqAxis(n, FS, 700, 25.0, 20000.0, jsg.capi.AXIS_LOG)
    db0, db1 = db_columns(W, n, seed=1), db_columns(W, n, seed=2)
    d_db = torch.from_numpy(db0).cuda()
    d_lut = torch.from_numpy(jsg.colormap_lut(256, oracle.CM_JADE)).cuda()
    d_img = torch.zeros((700, W), dtype=torch.int32, device="cuda")
    axis.handle(0)                                                         # created (and uploaded) before the capture
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        jsg.colormap_axis(d_db, d_lut, -90.0, 10.0, axis, d_argb=d_img, stream=st.cuda_stream)   # warm-up outside the capture
        st.synchronize()
        with torch.cuda.graph(g, stream=st):
            jsg.colormap_axis(d_db, d_lut, -90.0, 10.0, axis, d_argb=d_img, stream=st.cuda_stream)
    torch.cuda.synchronize()
    d_db.copy_(torch.from_numpy(db1))
    d_img.zero_()
    g.replay()
    torch.cuda.synchronize()
    pal = oracle.OracleColorPalette(256, oracle.CM_JADE)
    pal.set_value_range(-90.0, 10.0)
    ref = axis_image(oracle, pal, db1, axis, 0, running=True)             # pos 0: x = column
    assert (d_img.cpu().numpy().view(np.uint32) == ref).all()


def test_axis_launch_refusals(jsg, oracle, torch_cuda):
    torch = torch_cuda
    C = jsg.capi
    n, W = 1024, 20
    axis = jsg.FreqAxis(n, FS, 100, 20.0, 20000.0, C.AXIS_LOG)
    d_db = torch.zeros((W, n // 2 + 1), dtype=torch.float32, device="cuda")
    d_lut = torch.from_numpy(jsg.colormap_lut(256, 6)).cuda()
    d_img = torch.zeros((100, W), dtype=torch.int32, device="cuda")
    d_idx = torch.zeros((100, W), dtype=torch.uint8, device="cuda")
    other = jsg.FreqAxis(2048, FS, 100, 20.0, 20000.0, C.AXIS_LOG)

    def launch(ax=axis, **over):
        a = jsg.spectrogram._colormap_args(d_db, d_lut, -50.0, 50.0, d_img, None, 0, None, 0, n // 2 + 1)
        for k, v in over.items():
            setattr(a, k, v)
        return C.lib().jsg_colormap_axis_launch(ctypes.byref(a), ax.handle(0) if ax is not None else None, None)

    assert launch() == C.JSG_OK
    assert launch(ax=None) == C.JSG_ERR_INVALID
    assert launch(ax=other) == C.JSG_ERR_INVALID                             # another FFT size
    assert launch(height=n // 2) == C.JSG_ERR_INVALID
    assert launch(db=None) == C.JSG_ERR_INVALID
    assert launch(lut=None) == C.JSG_ERR_INVALID
    assert launch(n_cols=W + 1) == C.JSG_ERR_INVALID
    assert launch(n_cols=-1) == C.JSG_ERR_INVALID
    assert launch(col_first=-1) == C.JSG_ERR_INVALID
    assert launch(x_first=-1) == C.JSG_ERR_INVALID
    assert launch(x_wrap=0) == C.JSG_ERR_INVALID
    assert launch(argb_pitch=W - 1) == C.JSG_ERR_INVALID
    assert launch(argb_out=None) == C.JSG_ERR_INVALID
    assert launch(n_colors=0) == C.JSG_ERR_INVALID
    assert launch(argb_out=None, index_out=d_idx.data_ptr(), index_pitch=W, n_colors=257) == C.JSG_ERR_INVALID
    assert launch(n_colors=70000) == C.JSG_ERR_UNSUPPORTED
    assert launch(n_cols=0) == C.JSG_OK                                      # nothing to do
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------------------------------------------------------------
def make_engine(jsg, n=2048, mem_s=1.0, channels=2):
    s = jsg.Spectrogram(channels)
    s.setSamplerate(FS)
    s.setFFTSize(n)
    s.setmemoryTime_s(mem_s)
    s.setfeed_percent(1)                                                   # 50 %
    return s


def feed(s, oracle, blocks, seed):
    n = s.getFFTSize()
    x = oracle.synth_audio(s.getChannels(), blocks * n, fs=s.getSamplerate(), seed=seed)
    for b in range(blocks):
        assert s.processSynchronBlock(x[:, b * n:(b + 1) * n]) == 0


def peek(jsg, s):
    W, H = s.getMemorySize(), s.getSpectrumSize()
    ring = np.zeros((W, H), np.float32)
    pos = ctypes.c_int()
    s._c(jsg.capi.lib().jsg_peek_mem(s._h, ring.ctypes.data, W, ctypes.byref(pos)))
    return ring, pos.value


def engine_axis(jsg, s, scale, height, lo, hi):
    return jsg.FreqAxis(s.getFFTSize(), s.getSamplerate(), height, lo, hi, scale)


def palette(oracle, lo, hi, n_colors=256, scheme=None):
    pal = oracle.OracleColorPalette(n_colors, oracle.CM_JADE if scheme is None else scheme)
    pal.set_value_range(lo, hi)
    return pal


def with_cursor(oracle, img, pos, width):
    img = img.copy()
    W = img.shape[1]
    for d in range(width):
        x = pos + d
        if x == W:
            x -= W
        if x < W:
            img[:, x] = oracle.JUCE_RED_ARGB
    return img


@pytest.mark.parametrize("running", [True, False])
@pytest.mark.parametrize("scale,height,lo,hi", [(2, 480, 20.0, 20000.0), (3, 1500, 0.0, 24000.0), (1, 900, 0.0, 3000.0)])
def test_engine_display_against_model_incremental_and_full(jsg, oracle, torch_cuda, running, scale, height, lo, hi):
    s = make_engine(jsg)
    d = jsg.SpectrogramDisplay(s)
    d.setRunning(running)
    d.setFrequencyAxis(scale, height, lo, hi)
    assert d.height() == height
    axis = engine_axis(jsg, s, scale, height, lo, hi)
    assert np.array_equal(d.centres(), axis.rows()[3])
    pal = palette(oracle, -90.0, 10.0)
    W = s.getMemorySize()
    img = np.zeros((height, W), np.uint32)
    for tick, blocks in enumerate((7, 3, 1, 0, 5, 9)):
        feed(s, oracle, blocks, seed=100 + tick)
        nv, pos = d.timerCallback(img, -90.0, 10.0)
        ring, ppos = peek(jsg, s)
        assert ppos == pos
        ref = axis_image(oracle, pal, ring, axis, pos, running=running)
        if not running:   # the red cursor spans the axis height: one column after a full recolour, wider on incremental ticks
            ref = with_cursor(oracle, ref, pos, 1 if tick == 0 else 1 + (height < 2048) + 2 * (height < 1024))
        bad = int((img != ref).sum())
        assert bad == 0, f"tick {tick}: {bad} pixels differ"
    # the incremental ticks above agree with a full recolour of the same ring
    inc = img.copy()
    d.invalidate()
    nv, pos = d.timerCallback(img, -90.0, 10.0)
    if running:
        assert (img == inc).all()
    else:
        assert (img == with_cursor(oracle, axis_image(oracle, pal, peek(jsg, s)[0], axis, pos, running=False), pos, 1)).all()


def test_engine_tile_path_and_axis_change(jsg, oracle, torch_cuda):
    s = make_engine(jsg, n=4096)
    d = jsg.SpectrogramDisplay(s)
    d.setFrequencyAxis(jsg.capi.AXIS_LOG, 300, 40.0, 18000.0)
    axis = engine_axis(jsg, s, 2, 300, 40.0, 18000.0)
    pal = palette(oracle, -100.0, 0.0)
    W = s.getMemorySize()
    feed(s, oracle, 6, seed=1)
    img = np.zeros((300, W), np.uint32)
    d.timerCallback(img, -100.0, 0.0)
    tile = np.zeros((300, 16), np.uint32)
    for k, blocks in enumerate((2, 5, 1)):
        feed(s, oracle, blocks, seed=10 + k)
        need_full, nv, pos = d.timerCallbackTile(tile, -100.0, 0.0)
        assert not need_full and nv == 2 * blocks
        ring, _ = peek(jsg, s)
        full = axis_image(oracle, pal, ring, axis, pos, running=True)     # newest column at x = W-1
        assert (tile[:, :nv] == full[:, W - nv:]).all()
    # a new axis re-renders the history: the tile path refuses until a full update has run
    d.setFrequencyAxis(jsg.capi.AXIS_MEL, 200, 0.0, 16000.0)
    assert d.height() == 200
    mel = engine_axis(jsg, s, 3, 200, 0.0, 16000.0)
    need_full, nv, pos = d.timerCallbackTile(np.zeros((200, 16), np.uint32), -100.0, 0.0)
    assert need_full
    img = np.zeros((200, W), np.uint32)
    d.timerCallback(img, -100.0, 0.0)
    ring, pos = peek(jsg, s)
    assert (img == axis_image(oracle, pal, ring, mel, pos, running=True)).all()
    assert not (ring[:, :] == -120.0).all()
    feed(s, oracle, 1, seed=99)
    need_full, nv, pos = d.timerCallbackTile(np.zeros((200, 16), np.uint32), -100.0, 0.0)
    assert not need_full and nv == 2


def test_engine_samplerate_and_fft_size_clamp_and_restore(jsg, oracle, torch_cuda):
    s = make_engine(jsg, n=2048)
    d = jsg.SpectrogramDisplay(s)
    d.setFrequencyAxis(jsg.capi.AXIS_LOG, 400, 20.0, 20000.0)
    c48 = engine_axis(jsg, s, 2, 400, 20.0, 20000.0).rows()[3]
    assert np.array_equal(d.centres(), c48)
    pal = palette(oracle, -90.0, 10.0)
    # 32 kHz: fmax >= fs/2 -> fs/2
    s.setSamplerate(32000.0)
    assert d.height() == 400
    clamped = jsg.FreqAxis(2048, 32000.0, 400, 20.0, 16000.0, jsg.capi.AXIS_LOG)
    assert np.array_equal(d.centres(), clamped.rows()[3])
    feed(s, oracle, 8, seed=5)
    img = np.zeros((400, s.getMemorySize()), np.uint32)
    d.timerCallback(img, -90.0, 10.0)
    ring, pos = peek(jsg, s)
    assert (img == axis_image(oracle, pal, ring, clamped, pos, running=True)).all()
    # back at 48 kHz the requested range returns
    s.setSamplerate(48000.0)
    assert np.array_equal(d.centres(), c48)
    # another FFT size: the same rows for the new bins, and a full recolour (the tile path refuses first)
    s.setFFTSize(4096)
    feed(s, oracle, 5, seed=6)
    need_full, _, _ = d.timerCallbackTile(np.zeros((400, 64), np.uint32), -90.0, 10.0)
    assert need_full
    img = np.zeros((400, s.getMemorySize()), np.uint32)
    d.timerCallback(img, -90.0, 10.0)
    ring, pos = peek(jsg, s)
    a4096 = jsg.FreqAxis(4096, 48000.0, 400, 20.0, 20000.0, jsg.capi.AXIS_LOG)
    assert (img == axis_image(oracle, pal, ring, a4096, pos, running=True)).all()
    # fmin >= fs/2 -> 0.9 fs/2 (and fmax -> fs/2)
    d.setFrequencyAxis(jsg.capi.AXIS_LINEAR, 300, 18000.0, 20000.0)
    s.setSamplerate(32000.0)
    ref = jsg.FreqAxis(4096, 32000.0, 300, float(np.float32(0.9 * 16000.0)), 16000.0, jsg.capi.AXIS_LINEAR)
    assert np.array_equal(d.centres(), ref.rows()[3])
    feed(s, oracle, 4, seed=7)
    img = np.zeros((300, s.getMemorySize()), np.uint32)
    d.timerCallback(img, -90.0, 10.0)
    ring, pos = peek(jsg, s)
    assert (img == axis_image(oracle, pal, ring, ref, pos, running=True)).all()
    s.setSamplerate(48000.0)
    assert np.array_equal(d.centres(), jsg.FreqAxis(4096, 48000.0, 300, 18000.0, 20000.0, jsg.capi.AXIS_LINEAR).rows()[3])


def test_engine_refused_axis_keeps_the_old_image(jsg, oracle, torch_cuda):
    s = make_engine(jsg, n=1024)
    d = jsg.SpectrogramDisplay(s)
    d.setFrequencyAxis(jsg.capi.AXIS_MEL, 250, 0.0, 12000.0)
    feed(s, oracle, 6, seed=3)
    W = s.getMemorySize()
    img = np.zeros((250, W), np.uint32)
    d.timerCallback(img, -90.0, 10.0)
    before = img.copy()
    C = jsg.capi
    for args in ((C.AXIS_LOG, 300, 0.0, 1000.0), (C.AXIS_LINEAR, 300, 0.0, 30000.0), (C.AXIS_MEL, 1, 0.0, 1000.0), (7, 300, 0.0, 1000.0),
                 (C.AXIS_LINEAR, 20000, 0.0, 1000.0)):
        with pytest.raises(jsg.JsgError) as e:
            d.setFrequencyAxis(*args)
        assert e.value.code == C.JSG_ERR_INVALID
    assert d.height() == 250
    need_full, nv, _ = d.timerCallbackTile(np.zeros((250, 8), np.uint32), -90.0, 10.0)
    assert not need_full and nv == 0                                       # no recolour was forced
    d.timerCallback(img, -90.0, 10.0)
    assert (img == before).all()


@pytest.mark.parametrize("running", [True, False])
def test_engine_default_and_bins_axis_equal_an_untouched_engine(jsg, oracle, torch_cuda, running):
    a, b = make_engine(jsg, n=2048), make_engine(jsg, n=2048)
    da, db_ = jsg.SpectrogramDisplay(a), jsg.SpectrogramDisplay(b)
    da.setRunning(running)
    db_.setRunning(running)
    assert da.height() == 1025 and a.getSpectrumSize() == 1025
    assert np.allclose(da.centres(), np.arange(1025) * FS / 2048)
    db_.setFrequencyAxis(jsg.capi.AXIS_LOG, 640, 20.0, 20000.0)
    W = a.getMemorySize()
    tmp = np.zeros((640, W), np.uint32)
    feed(b, oracle, 2, seed=1)
    db_.timerCallback(tmp, -90.0, 10.0)
    db_.setFrequencyAxis(jsg.capi.AXIS_BINS)
    assert db_.height() == 1025
    feed(a, oracle, 2, seed=1)
    ia, ib = np.zeros((1025, W), np.uint32), np.zeros((1025, W), np.uint32)
    for k, blocks in enumerate((3, 1, 4)):
        feed(a, oracle, blocks, seed=20 + k)
        feed(b, oracle, blocks, seed=20 + k)
        ra, rb = da.timerCallback(ia, -90.0, 10.0), db_.timerCallback(ib, -90.0, 10.0)
        assert ra[1] == rb[1]
        assert (ia == ib).all()
    ring, pos = peek(jsg, a)
    ref = oracle.render_all(ring, pos, palette(oracle, -90.0, 10.0), running=running)
    assert (ia == (ref if running else with_cursor(oracle, ref, pos, 2))).all()


def test_cpp_driver_draws_a_tone_on_a_log_axis(jsg):
    exe = build_cpp_driver(jsg)
    out = subprocess.check_output([exe, "600", "4096", "1000"], timeout=120).decode()
    info = json.loads(out.strip().splitlines()[-1])
    assert info["H"] == 600
    assert abs(info["centre_lo"] - 20.0) < 1e-3 and abs(info["centre_hi"] - 20000.0) < 1e-2
    assert abs(info["tone_row_hz"] / 1000.0 - 1.0) < 0.03

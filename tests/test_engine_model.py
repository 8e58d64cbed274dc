"""CPU checks of oracle/engine_model.EngineModel, the engine model the GPU engine walks compare against (no GPU needed).

* default backend: bit for bit OracleSpectrogram on the seeded scenarios of test_gpu_parity.py (the model only ADDS to the oracle);
* mirror backend with the exact logarithm: within parity_util's bound of the float64 oracle (stft_db_reference), every mix and
  per-channel mode;
* the engine semantics the model claims (csrc/jsg_engine.cpp): what survives which setter, what is refused."""
import numpy as np
import pytest

from parity_util import assert_db_close, mixed_power_f64


def _scenario(oracle, model_cls, seed):
    """test_gpu_parity.py::test_seeded_random_engine_scenarios' event sequence on the oracle and on the model side by side."""
    rng = np.random.default_rng(1000 + seed)
    C = int(rng.integers(1, 5))
    o = oracle.OracleSpectrogram(C); m = model_cls(C)
    n = int(rng.choice([512, 1024, 2048]))
    for e in (o, m):
        e.set_samplerate(48000.0); e.set_memory_time_s(0.2); e.set_fft_size(n)
    x = oracle.synth_audio(C, 64 * 4096, seed=seed, kind="mix")
    at, reads = 0, 0
    for step in range(60):
        ev = rng.choice(["block"] * 12 + ["getmem"] * 3 + ["pause", "feed", "window", "mix", "fft", "memtime"])
        if ev == "block":
            if at + n > x.shape[1]:
                at = 0
            blk = x[:, at:at + n]; at += n
            o.process_synchron_block(blk); m.process_synchron_block(blk)
        elif ev == "pause":
            p = bool(rng.integers(0, 2)); o.set_pause_mode(p); m.set_pause_mode(p)
        elif ev == "feed":
            f = int(rng.integers(0, 4)); o.set_feed_percent(f); m.set_feed_percent(f)
        elif ev == "window":
            w = int(rng.integers(0, 6)); o.set_window(w); m.set_window(w)
        elif ev == "mix":
            mm = int(rng.integers(0, 5 if C > 1 else 4)); o.mode = mm; m.set_mix_mode(mm)
        elif ev == "fft":
            n = int(rng.choice([512, 1024, 2048, 4096])); o.set_fft_size(n); m.set_fft_size(n)
        elif ev == "memtime":
            t = float(rng.choice([0.1, 0.2, 0.5])); o.set_memory_time_s(t); m.set_memory_time_s(t)
        if ev == "getmem" or step == 59:
            assert (m.memsize_blocks, m.freqsize, m.hop, m.feedblocks) == (o.memsize_blocks, o.freqsize, o.hop, o.feedblocks)
            W, H = o.memsize_blocks, o.freqsize
            mo = np.zeros((W, H), np.float32); mm_ = np.zeros((W, H), np.float32)
            assert o.get_mem(mo) == m.get_mem(mm_), (seed, step)
            assert (mo.view(np.uint32) == mm_.view(np.uint32)).all(), (seed, step)
            assert (o.mem.view(np.uint32) == m.mem.view(np.uint32)).all(), (seed, step)
            reads += 1
    return reads


@pytest.mark.parametrize("seed", range(10))
def test_default_model_reproduces_the_oracle_bit_for_bit(oracle, seed):
    from oracle.engine_model import EngineModel
    assert _scenario(oracle, EngineModel, seed) > 0


def test_default_model_reproduces_the_block_by_block_stream(oracle):
    """test_gpu_parity.py::test_block_by_block_stream_pause_and_getmem's stream (pause, two ring wraps)."""
    from oracle.engine_model import EngineModel
    C, n = 2, 1024
    o = oracle.OracleSpectrogram(C); m = EngineModel(C)
    for e in (o, m):
        e.set_samplerate(48000.0); e.set_memory_time_s(0.25); e.set_fft_size(n); e.set_feed_percent(1)
    x = oracle.synth_audio(C, 40 * n, seed=9)
    mo = np.zeros((23, n // 2 + 1), np.float32); mm = mo.copy()
    for b in range(40):
        if b in (10, 14):
            o.set_pause_mode(b == 10); m.set_pause_mode(b == 10)
        o.process_synchron_block(x[:, b * n:(b + 1) * n]); m.process_synchron_block(x[:, b * n:(b + 1) * n])
        if b % 4 == 3:
            assert o.get_mem(mo) == m.get_mem(mm)
            assert (mo.view(np.uint32) == mm.view(np.uint32)).all()


@pytest.mark.parametrize("n,C,feed,mix", [(512, 2, 1, 0), (1024, 3, 2, 1), (1024, 2, 3, 2), (2048, 2, 1, 3), (2048, 4, 0, 4),
                                          (4096, 3, 1, 0), (8192, 1, 1, 0), (1024, 3, 1, 100)])
def test_mirror_backend_exact_columns_within_the_oracle_bound(oracle, n, C, feed, mix):
    """The mirror backend with the exact logarithm against the float64 oracle (stft_db_reference), parity_util's bound, and the
    model's own records (p64, peak) against mixed_power_f64."""
    from oracle.engine_model import EngineModel
    K = 5
    x = oracle.synth_audio(C, K * n, seed=n + C)
    m = EngineModel(C, backend="mirror")
    m.set_memory_time_s(1.0); m.set_fft_size(n); m.set_feed_percent(feed); m.set_window(oracle.WIN_BLACKMANHARRIS)
    m.set_power_scale(0.5); m.set_exact_log(True); m.set_mix_mode(mix)
    m.process_blocks(x)
    F, W = K * m.feedblocks, m.memsize_blocks
    assert m.exact[[p * W + j for p in range(m.planes) for j in range(F)]].all() and not m.written[F:W].any()
    if mix == 100:
        pw = oracle.stft_db_reference(x, n, m.hop, m.feedblocks, m.window, power_scale=0.5, return_power=True)
        for c in range(C):
            ref = oracle.to_db(pw[c].astype(np.float32))
            p64 = pw[c].astype(np.float32).astype(np.float64)
            assert (m.p64[c * W:c * W + F] == p64).all() and (m.ref_db[c * W:c * W + F].view(np.uint32) == ref.view(np.uint32)).all()
            assert_db_close(m.mem[c * W:c * W + F], ref, p64, f"plane {c}")
        return
    ref = oracle.stft_db_reference(x, n, m.hop, m.feedblocks, m.window, mode=mix, power_scale=0.5)
    p64 = mixed_power_f64(oracle, x, n, m.hop, m.feedblocks, m.window, mix, power_scale=0.5)
    assert (m.p64[:F] == p64).all() and (m.ref_db[:F].view(np.uint32) == ref.view(np.uint32)).all()
    peak = None
    if mix != 0:
        pc = oracle.stft_db_reference(x, n, m.hop, m.feedblocks, m.window, power_scale=0.5, return_power=True)
        peak = pc.max(axis=(0, 2))[:, None]
        assert (m.peak[:F] == peak[:, 0]).all()
    assert_db_close(m.mem[:F], ref, p64, f"n={n} C={C} mix={mix}", peak=peak)
    assert (m.mem[F:] == np.float32(-120.0)).all()


def test_model_setter_semantics(oracle):
    from oracle.engine_model import EngineModel
    m = EngineModel(2)
    m.set_fft_size(1024)
    w = np.linspace(0.5, 1.5, 1024).astype(np.float32)
    m.set_window_table(w)
    m.process_synchron_block(np.ones((2, 1024), np.float32))
    ring = m.mem.copy()
    m.set_power_scale(2.0); m.set_exact_log(True); m.set_mix_mode(oracle.MIX_MAX)   # none of these wipes the ring
    assert (m.mem.view(np.uint32) == ring.view(np.uint32)).all() and m.mem_counter == 1
    m.set_channels(3); m.set_feed_percent(2); m.set_samplerate(44100.0); m.set_memory_time_s(0.3)   # a custom table survives these
    assert m.window_custom and (m.window == w).all()
    m.set_mix_mode(100)                                                              # to per-channel: rebuilt, three planes
    assert m.mem.shape == (3 * m.memsize_blocks, 513) and not m.written.any() and m.window_custom
    m.set_window(oracle.WIN_HANN)
    assert not m.window_custom
    m.set_window_table(w); m.set_fft_size(1024)
    assert not m.window_custom and (m.window == oracle.window(oracle.WIN_HANN, 1024)).all()
    m.set_feed_percent_ext(30.0)
    assert (m.hop, m.feedblocks) == (307, 3)
    m.set_fft_size(2048)                                                             # feedblocks stay; the hop follows the percentage
    assert (m.hop, m.feedblocks) == (614, 3)
    m.set_mix_mode(oracle.MIX_RIGHT)
    with pytest.raises(ValueError):
        m.set_channels(1)
    assert m.channels == 3 and m.mode == oracle.MIX_RIGHT
    m1 = EngineModel(1)
    with pytest.raises(ValueError):
        m1.set_mix_mode(oracle.MIX_RIGHT)

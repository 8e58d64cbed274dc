"""Seeded walks over the whole stateful engine surface (jsg_create ... jsg_process_block ... jsg_get_mem), mirrored step by step on
the engine model (oracle/engine_model.py, mirror backend).

Each walk starts an engine and the model with the same random settings and then draws events: blocks (processSynchronBlock -- the
lossless queue --, processBlocks with 1 to 40 blocks, processBlocksDevice), "NaN blocks" (one NaN sample at a random channel and
position), every setter (sample rate, channels, FFT size, closest FFT size in ms, memory time, feed percentage and its extension,
pause, window, window table, mix mode including per-channel and Right, power scale, exact logarithm) and reads through getMem,
jsg_peek_mem and jsg_get_mem_rows (some rows NULL).  After every read:

  * counters: newVals, pos, W, H, hop, feedblocks, FFT size and channel count equal the model's (peek does not reset newVals);
  * bits: every column written under the exact logarithm is identical to the kernel mirror's (the engine pins plan_select = 1);
  * accuracy: every column, under either logarithm, is within parity_util.assert_db_close of the model's float64 record;
  * fill: unwritten columns hold exactly -120 dB;
  * NaN tracer: NaN appears in exactly the columns whose frames read a NaN sample (through the carried history too; Max / Min skip a
    NaN channel as the reference's comparisons do), in every bin of them; every other column passes the checks above;
  * refusals: setchannels(1) under a Right mix and setMixMode(Right) with one channel raise and change nothing.

At the end a second engine replays the same events with every run of blocks cut differently (batches where the walk had single blocks
and single blocks where it had batches): its ring must equal the walk's bit for bit.

JSG_FUZZ_WALKS / JSG_FUZZ_WALK_EVENTS / JSG_FUZZ_SEED widen the campaign (defaults: 16 walks of 80 events)."""
import ctypes as C
import os

import numpy as np
import pytest

from parity_util import assert_ring_matches

pytestmark = pytest.mark.gpu

WALKS = int(os.environ.get("JSG_FUZZ_WALKS", "16"))
EVENTS = int(os.environ.get("JSG_FUZZ_WALK_EVENTS", "80"))
SEED0 = int(os.environ.get("JSG_FUZZ_SEED", "0"))

EVENT_WEIGHTS = {"block": 14, "nan": 3, "getmem": 4, "peek": 2, "rows": 2, "fs": 1, "channels": 1, "fft": 1, "fft_ms": 1, "memtime": 1,
                 "feed": 1, "feed_ext": 1, "pause": 1, "window": 1, "window_table": 1, "mix": 2, "power": 1, "exact": 2}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


class Walk:
    def __init__(self, jsg, oracle, torch, seed):
        from oracle.engine_model import EngineModel
        self.jsg, self.oracle, self.torch = jsg, oracle, torch
        self.rng = np.random.default_rng(7000 + seed + 1009 * SEED0)
        self.seed = seed
        self.log = []                       # the events that reached the engine, for the replay
        self.C0 = int(self.rng.integers(1, 5))
        self.s = jsg.Spectrogram(self.C0)
        self.m = EngineModel(self.C0, backend="mirror")
        self.bufs = {}
        self.nan_columns_seen = 0
        self.t = 0.0
        # same random start on both sides
        for ev in ("fs", "memtime", "fft", "feed", "window", "mix", "exact"):
            self.setter(ev)

    # ---- inputs ----
    def samples(self, k):
        C, n = self.m.channels, self.m.fftsize
        t = self.t + np.arange(k * n, dtype=np.float64)
        self.t += k * n
        amp = float(self.rng.choice([1e-3, 0.3, 1.0]))
        x = np.empty((C, k * n), np.float32)
        for c in range(C):
            f = float(self.rng.uniform(50.0, 12000.0))
            x[c] = (amp * (0.7 * np.sin(2 * np.pi * f * t / 48000.0) + 0.3 * self.rng.uniform(-1.0, 1.0, k * n))).astype(np.float32)
        return x

    def blocks(self, with_nan=False):
        n = self.m.fftsize
        path = str(self.rng.choice(["sync", "batch", "device"]))
        k = 1 if path == "sync" else int(self.rng.integers(1, 41 if n <= 2048 else 11) if path == "batch" else self.rng.integers(1, 9))
        x = self.samples(k)
        if with_nan:
            c = int(self.rng.integers(0, x.shape[0]))
            where = self.rng.choice(["first", "last", "any"])
            pos = 0 if where == "first" else x.shape[1] - 1 if where == "last" else int(self.rng.integers(0, x.shape[1]))
            x[c, pos] = np.nan
        self.run_blocks(self.s, x, path)
        self.m.process_blocks(x)
        self.log.append(("blocks", x, path))

    def run_blocks(self, s, x, path):
        n = s.getFFTSize()
        if path == "sync":
            for b in range(x.shape[1] // n):
                assert s.processSynchronBlock(x[:, b * n:(b + 1) * n]) == 0
        elif path == "batch":
            assert s.processBlocks(x) == 0
        else:
            d = self.torch.from_numpy(x).cuda()
            assert s.processBlocksDevice(d) == 0
            self.torch.cuda.synchronize()

    # ---- setters: the model decides whether the engine must refuse ----
    def setter(self, ev):
        r, m = self.rng, self.m
        if ev == "fs":
            call = ("setSamplerate", "set_samplerate", float(r.choice([44100.0, 48000.0, 96000.0])))
        elif ev == "channels":
            c = int(r.integers(1, 5))
            if m.mode == 4 and m.channels >= 2 and r.random() < 0.5:
                c = 1                                               # exercise the refusal under a Right mix
            call = ("setchannels", "set_channels", c)
        elif ev == "fft":
            call = ("setFFTSize", "set_fft_size", int(r.choice([512, 1024, 2048, 4096, 8192])))
        elif ev == "fft_ms":
            ms = float(r.choice([6.0, 11.0, 20.0, 42.0, 85.0, 170.0]))
            if self.oracle.next_power_of_2(ms, m.fs) not in (512, 1024, 2048, 4096, 8192):
                return
            call = ("setclosestFFTSize_ms", "set_closest_fft_size_ms", ms)
        elif ev == "memtime":
            call = ("setmemoryTime_s", "set_memory_time_s", float(r.choice([0.25, 0.5, 1.0])))
        elif ev == "feed":
            call = ("setfeed_percent", "set_feed_percent", int(r.integers(0, 4)))
        elif ev == "feed_ext":
            call = ("setfeed_percent_ext", "set_feed_percent_ext", float(r.choice([12.5, 30.0, 100.0 / 3.0, 80.0, 50.0])))
        elif ev == "pause":
            call = ("setPauseMode", "set_pause_mode", bool(r.random() < 0.3))
        elif ev == "window":
            call = ("setWindow", "set_window", int(r.integers(0, 6)))
        elif ev == "window_table":
            n = m.fftsize
            w = (self.oracle.window(int(r.integers(0, 6)), n) * r.uniform(0.5, 1.5, n) + 0.01).astype(np.float32)
            call = ("setWindowTable", "set_window_table", w)
        elif ev == "mix":
            mode = int(r.choice([0, 1, 2, 3, 4, 4, 100, 100]))
            call = ("setMixMode", "set_mix_mode", mode)
        elif ev == "power":
            call = ("setPowerScale", "set_power_scale", float(r.choice([1.0, 0.25, 2.0, 1e-3, 3.7])))
        elif ev == "exact":
            call = ("setExactLog", "set_exact_log", bool(r.random() < 0.6))
        else:
            raise AssertionError(ev)
        self.apply(self.s, self.m, call, check=True)
        self.log.append(("set", call))

    def apply(self, s, m, call, check):
        eng_name, model_name, arg = call
        refused = False
        if m is not None:
            try:
                getattr(m, model_name)(arg)
            except ValueError:
                refused = True
        if refused:
            before = self.geometry()
            with pytest.raises(self.jsg.capi.JsgError):
                getattr(s, eng_name)(arg)
            assert self.geometry() == before, f"walk {self.seed}: a refused {eng_name}({arg}) changed the engine"
            self.read("peek")                                       # and the ring / counters are those of the model still
        elif m is not None or check:
            getattr(s, eng_name)(arg)
        else:                                                       # replay: the model is not involved
            try:
                getattr(s, eng_name)(arg)
            except self.jsg.capi.JsgError:
                pass

    def geometry(self, s=None):
        s = s or self.s
        return (s.getMemorySize(), s.getSpectrumSize(), s.getFeedSamples(), s.getFeedBlocks(), s.getFFTSize(), s.getChannels(),
                s.getSamplerate())

    # ---- reads ----
    def read(self, kind):
        from oracle.engine_model import empty_records
        jsg, m, s = self.jsg, self.m, self.s
        geo = self.geometry()
        assert geo == (m.memsize_blocks, m.freqsize, m.hop, m.feedblocks, m.fftsize, m.channels, float(m.fs)), \
            f"walk {self.seed}: engine {geo} vs model"
        R, H = m.planes * m.memsize_blocks, m.freqsize
        if kind not in self.bufs or self.bufs[kind][0].shape != (R, H):
            self.bufs[kind] = (np.full((R, H), -120.0, np.float32), empty_records(R, H))
        buf, rec = self.bufs[kind]
        lib, pos = jsg.capi.lib(), C.c_int(-1)
        if kind == "getmem":
            nv, p = s.getMem(buf)
            nv_m, p_m = m.get_mem(rec["mem"], records=rec)
        elif kind == "peek":
            nv = jsg.capi.check(lib.jsg_peek_mem(s._h, buf.ctypes.data, R, C.byref(pos)), s._h); p = pos.value
            nv_m, p_m = m.peek_mem(rec["mem"], records=rec)
        else:
            present = self.rng.random(R) >= 0.25
            rows = (C.c_void_p * R)(*[buf[i].ctypes.data if present[i] else None for i in range(R)])
            nv = jsg.capi.check(lib.jsg_get_mem_rows(s._h, rows, R, H, C.byref(pos)), s._h); p = pos.value
            nv_m, p_m = m.get_mem(rec["mem"], rows_present=present, records=rec)
        assert (nv, p) == (nv_m, p_m), f"walk {self.seed} {kind}: (newVals, pos) engine {(nv, p)} vs model {(nv_m, p_m)}"
        assert_ring_matches(buf, rec, f"walk {self.seed} {kind}")
        self.nan_columns_seen += int(np.isnan(rec["mem"]).any(axis=1).sum())

    def step(self):
        names = list(EVENT_WEIGHTS)
        w = np.array([EVENT_WEIGHTS[k] for k in names], np.float64)
        ev = str(self.rng.choice(names, p=w / w.sum()))
        if ev in ("block", "nan"):
            self.blocks(with_nan=ev == "nan")
        elif ev in ("getmem", "peek", "rows"):
            self.read(ev)
        else:
            self.setter(ev)


def _replay(walk, jsg, C0):
    """A second engine fed the walk's events with every run of blocks cut the other way."""
    s2 = jsg.Spectrogram(C0)
    pending = []

    def flush():
        if pending:
            x = np.concatenate(pending, axis=1)
            s2.processBlocks(x)
            pending.clear()

    for e in walk.log:
        if e[0] == "set":
            flush()
            walk.apply(s2, None, e[1], check=False)
        else:
            _, x, path = e
            if path == "sync":
                pending.append(x)                                   # single blocks -> one batch
            else:
                flush()
                walk.run_blocks(s2, x, "sync")                      # batches -> single blocks
    flush()
    return s2


def _peek_all(jsg, s, planes):
    R = s.getMemorySize() * planes
    buf = np.zeros((R, s.getSpectrumSize()), np.float32)
    pos = C.c_int(-1)
    jsg.capi.check(jsg.capi.lib().jsg_peek_mem(s._h, buf.ctypes.data, R, C.byref(pos)), s._h)
    return buf, pos.value


@pytest.mark.parametrize("seed", range(WALKS))
def test_engine_walk(jsg, oracle, torch_cuda, seed):
    walk = Walk(jsg, oracle, torch_cuda, seed)
    for _ in range(EVENTS):
        walk.step()
    walk.read("peek")
    walk.read("getmem")
    s2 = _replay(walk, jsg, walk.C0)
    a, pa = _peek_all(jsg, walk.s, walk.m.planes)
    b, pb = _peek_all(jsg, s2, walk.m.planes)
    assert pa == pb and a.shape == b.shape, f"walk {seed}: replay with other block cuts ends at {pb}, the walk at {pa}"
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    assert (nan_a == nan_b).all() and (a[~nan_a].view(np.uint32) == b[~nan_b].view(np.uint32)).all(), \
        f"walk {seed}: the ring depends on how the blocks were cut into calls"
    s2.close()
    walk.s.close()

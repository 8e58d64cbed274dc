"""CPU MODEL OF THE STATEFUL ENGINE -- TEST INFRASTRUCTURE ONLY.

EngineModel extends OracleSpectrogram (oracle/jsg_oracle.py, whose behaviour it leaves untouched) with what the engine of
csrc/jsg_engine.cpp offers beyond the reference's class, with the engine's semantics:

  * per-channel mode (JSG_MIX_PER_CHANNEL): the ring holds C planes of W columns, get_mem fills C*W rows plane by plane;
  * set_window_table / set_power_scale / set_exact_log: none of them wipes the ring or the history, they act on later columns,
    and a custom window table survives every setter except set_fft_size (set_closest_fft_size_ms) and set_window;
  * set_mix_mode rebuilds (buildmem) only when it switches to or from per-channel mode; Right needs two channels, and
    set_channels(1) under a Right mix is refused like set_mix_mode(Right) with one channel;
  * peek_mem (jsg_peek_mem: the whole ring, the counter is not reset);
  * backend="mirror": every column is computed by the kernel mirror (oracle/mirror.py) with the plan the engine pins
    (plan_select = 1), the power scale in force, and -- when the column is written under set_exact_log(True) -- the shared
    exact logarithm, so those columns are bit for bit what the GPU writes.

Next to every ring column the model keeps a record: the float64 view of the mixed power the oracle took the log of (`p64`), the
yardstick peak that parity_util.assert_db_close needs (`peak`: the column's own peak for AbsMean and per-channel planes, the
largest per-channel peak of the frame for Max, Min, Left and Right), the oracle's dB column (`ref_db`), and whether the column was
written at all (`written`) and with the exact logarithm (`exact`).  In the default backend `mem` is exactly OracleSpectrogram's.
"""
from __future__ import annotations

import numpy as np

from .jsg_oracle import (MIX_ABSMEAN, MIX_RIGHT, NEW_ENTRY_SENTINEL, RING_FILL_DB, WIN_HANN, OracleSpectrogram, f32, mix_channels,
                         next_power_of_2, power_spectrum_f64, to_db, window)

MIX_PER_CHANNEL = 100                                    # include/jsg.h
FFT_SIZES = (512, 1024, 2048, 4096, 8192)
PINNED_PLAN = {512: "Cfg512", 1024: "Cfg1024", 2048: "Cfg2048", 4096: "Cfg4096", 8192: "Cfg8192"}   # run_blocks: plan_select = 1
RECORD_FIELDS = ("mem", "ref_db", "p64", "peak", "exact", "written")


def empty_records(rows: int, H: int) -> dict:
    """A caller-side buffer and its records, as get_mem(..., records=) fills them (mem: what the caller's float buffer holds; it starts
    at the -120 dB fill, so rows that no read has reached yet look unwritten -- give the engine's buffer the same start)."""
    return {"mem": np.full((rows, H), RING_FILL_DB, f32), "ref_db": np.full((rows, H), RING_FILL_DB, f32), "p64": np.zeros((rows, H)),
            "peak": np.zeros(rows), "exact": np.zeros(rows, bool), "written": np.zeros(rows, bool)}


class EngineModel(OracleSpectrogram):
    def __init__(self, channels: int = 2, backend: str = "oracle"):
        assert backend in ("oracle", "mirror")
        self.backend = backend
        self.window_custom = False
        self.exact_log = False
        self._mirror = None
        if backend == "mirror":
            from . import mirror
            self._mirror = mirror.load()
        super().__init__(channels)
        self.window = window(self.window_choice, self.fftsize)    # jsg_create builds the window (the reference leaves it empty)

    # ---- geometry ----
    @property
    def planes(self) -> int:
        return self.channels if self.mode == MIX_PER_CHANNEL else 1

    def _buildmem(self):
        super()._buildmem()
        rows, H = self.planes * self.memsize_blocks, self.freqsize
        self.mem = np.full((rows, H), RING_FILL_DB, dtype=f32)
        self.ref_db = self.mem.copy()
        self.p64 = np.zeros((rows, H))
        self.peak = np.zeros(rows)
        self.exact = np.zeros(rows, bool)
        self.written = np.zeros(rows, bool)

    def _set_window_fkt(self):                             # build_window after set_fft_size / set_window: the table is recomputed
        self.window_custom = False
        super()._set_window_fkt()

    # ---- setters with the engine's checks and semantics (csrc/jsg_engine.cpp) ----
    def set_channels(self, c):
        if int(c) <= 0 or (int(c) < 2 and self.mode == MIX_RIGHT):
            raise ValueError("refused: channel count")
        super().set_channels(c)

    def set_fft_size(self, n):
        if int(n) not in FFT_SIZES:
            raise ValueError("unsupported FFT size")
        super().set_fft_size(n)

    def set_closest_fft_size_ms(self, ms):
        self.set_fft_size(next_power_of_2(ms, self.fs))

    def set_window_table(self, w):
        w = np.asarray(w, dtype=f32)
        if w.shape != (self.fftsize,):
            raise ValueError("window table must have fft-size entries")
        self.window = w.copy()
        self.window_custom = True

    def set_power_scale(self, s):
        if not float(s) > 0.0:
            raise ValueError("power scale must be positive")
        self.power_scale = float(f32(s))

    def set_exact_log(self, on):
        self.exact_log = bool(on)

    def set_mix_mode(self, m):
        m = int(m)
        if m not in (0, 1, 2, 3, 4, MIX_PER_CHANNEL):
            raise ValueError("unknown mix mode")
        if m == MIX_RIGHT and self.channels < 2:
            raise ValueError("Right needs two channels")
        replane = (m == MIX_PER_CHANNEL) != (self.mode == MIX_PER_CHANNEL)
        self.mode = m
        if replane:
            self._buildmem()

    # ---- processSynchronBlock ----
    def _columns(self):
        """The feedblocks columns of the block that sits in indatamem[:, n:2n]: list of (rows of this column, one per plane) as
        (mem, ref_db, p64, peak) arrays of shape [planes][H] / [planes]."""
        n, hop, fb = self.fftsize, self.hop, self.feedblocks
        starts = np.arange(fb) * hop
        frames = (self.indatamem[:, starts[:, None] + np.arange(n)[None, :]] * self.window[None, None, :]).astype(f32)   # [C][fb][n]
        pw64 = power_spectrum_f64(frames, self.power_scale)                                # [C][fb][H]
        pw32 = pw64.astype(f32)
        with np.errstate(invalid="ignore"):
            if self.mode == MIX_PER_CHANNEL:
                ref_db = to_db(pw32).transpose(1, 0, 2)                                     # [fb][C][H]
                p64 = pw32.astype(np.float64).transpose(1, 0, 2)
                peak = p64.max(axis=2)                                                      # [fb][C]
            else:
                mixed = mix_channels(pw32, self.mode)                                      # [fb][H]
                ref_db = to_db(mixed)[:, None, :]
                p64 = mixed.astype(np.float64)[:, None, :]
                if self.mode == MIX_ABSMEAN:
                    peak = p64.max(axis=2)
                else:   # a selecting mix: the largest per-channel peak of the frame (a NaN channel, which Max / Min skip, left out)
                    allnan = np.isnan(pw64).all(axis=(0, 2))
                    peak = np.where(allnan, np.nan, np.nanmax(np.where(np.isnan(pw64), -np.inf, pw64), axis=(0, 2)))[:, None]
        mem = ref_db
        if self.backend == "mirror" and self.exact_log:   # (hardware-log columns are checked against the float64 record only)
            x = np.ascontiguousarray(self.indatamem)
            plan = PINNED_PLAN[n]
            if self.mode == MIX_PER_CHANNEL:
                cols = [self._mirror.columns(plan, x[c:c + 1], hop, fb, self.window, feedblocks=fb, mix=0, power_scale=self.power_scale,
                                             exact_db=True) for c in range(self.channels)]
                mir = np.stack(cols, axis=1)                                                # [fb][C][H]
            else:
                mir = self._mirror.columns(plan, x, hop, fb, self.window, feedblocks=fb, mix=self.mode, power_scale=self.power_scale,
                                           exact_db=True)[:, None, :]
            mem = mir
        return mem, ref_db, p64, peak

    def process_synchron_block(self, data: np.ndarray) -> int:
        n = self.fftsize
        data = np.asarray(data, dtype=f32)
        assert data.shape == (self.channels, n)
        self.indatamem[:, n:] = data
        if not self.pause:   # (paused: the reference computes and drops the columns, Spectrogram.cpp:111)
            mem, ref_db, p64, peak = self._columns()
            W = self.memsize_blocks
            for bb in range(self.feedblocks):
                rows = np.arange(self.planes) * W + self.mem_counter
                self.mem[rows] = mem[bb]
                self.ref_db[rows] = ref_db[bb]
                self.p64[rows] = p64[bb]
                self.peak[rows] = peak[bb]
                self.exact[rows] = self.exact_log and self.backend == "mirror"
                self.written[rows] = True
                self.new_entry_counter += 1
                self.mem_counter = (self.mem_counter + 1) % W
        self.indatamem[:, :n] = self.indatamem[:, n:].copy()
        return 0

    def process_blocks(self, samples: np.ndarray) -> int:
        n = self.fftsize
        for k in range(samples.shape[1] // n):
            self.process_synchron_block(samples[:, k * n:(k + 1) * n])
        return 0

    # ---- getMem / peekMem ----
    def _read_rows(self, peek: bool):
        W, nec, pos = self.memsize_blocks, self.new_entry_counter, self.mem_counter
        if peek or nec >= W:
            cols = np.arange(W)
        else:
            cols = np.arange(pos - nec, pos) % W                                           # Spectrogram.cpp:307-319
        return (np.arange(self.planes)[:, None] * W + cols[None, :]).ravel()

    def get_mem(self, mem: np.ndarray, rows_present=None, records: dict | None = None, peek: bool = False):
        """mem: the caller's [planes*W][H] buffer, updated in place; rows_present: optional bool mask of the rows the caller passed
        (jsg_get_mem_rows with NULL rows); records: a dict of empty_records() that is updated alongside.  Returns (newVals, pos)."""
        if mem.shape[0] != self.planes * self.memsize_blocks:
            return -1, None
        rows = self._read_rows(peek)
        if rows_present is not None:
            rows = rows[np.asarray(rows_present, bool)[rows]]
        mem[rows] = self.mem[rows]
        if records is not None:
            for k in RECORD_FIELDS:
                records[k][rows] = getattr(self, k)[rows]
        nec = self.new_entry_counter
        if peek:
            return min(nec, 2000000000), self.mem_counter
        self.new_entry_counter = 0
        return nec, self.mem_counter

    def peek_mem(self, mem: np.ndarray, records: dict | None = None):
        return self.get_mem(mem, records=records, peek=True)


__all__ = ["EngineModel", "empty_records", "MIX_PER_CHANNEL", "FFT_SIZES", "PINNED_PLAN", "NEW_ENTRY_SENTINEL"]

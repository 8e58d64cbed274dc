"""Python mirror of the reference's host interface for the hot path, on top of the C-ABI (include/jsg.h).

    Spectrogram          <-> class Spectrogram          (reference Spectrogram.h:81-169)   method names kept
    CColorPalette        <-> class CColorPalette        (reference CColorpalette.h:6-61)
    SpectrogramDisplay   <-> the colour half of SpectrogramComponent::timerCallback (Spectrogram.cpp:590-731)
    Plan / stft_db / colormap : the stateless device ops on torch tensors that live in HBM (used by bench.py)

Everything computes on the GPU through libjsg.so; numpy/torch are used for buffers only.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi, capix
from .capi import JsgError, check, lib


# --------------------------------------------------------------------------------------------------
# host-side precompute (same arithmetic as the reference, done in the library)
# --------------------------------------------------------------------------------------------------
def feed_samples(feed_percent: float, fftsize: int) -> int:
    return check(lib().jsg_feed_samples(feed_percent, fftsize))


def memsize_blocks(memsize_s: float, fs: float, hop: int) -> int:
    return check(lib().jsg_memsize_blocks(memsize_s, fs, hop))


def next_power_of_2(ms: float, fs: float) -> int:
    return check(lib().jsg_next_power_of_2(ms, fs))


def window(kind: int, n: int) -> np.ndarray:
    out = np.zeros(n, dtype=np.float32)
    check(lib().jsg_window_build(kind, n, out.ctypes.data))
    return out


def colormap_lut(n_colors: int, scheme: int) -> np.ndarray:
    out = np.zeros(n_colors, dtype=np.int32)
    check(lib().jsg_colormap_build(n_colors, scheme, out.ctypes.data))
    return out


def colormap_range(n_colors: int, lo: float, hi: float):
    a, b, m = C.c_float(), C.c_float(), C.c_float()
    check(lib().jsg_colormap_range(n_colors, lo, hi, C.byref(a), C.byref(b), C.byref(m)))
    return np.float32(a.value), np.float32(b.value), np.float32(m.value)


# --------------------------------------------------------------------------------------------------
# class Spectrogram
# --------------------------------------------------------------------------------------------------
class _NativeHandle:
    """One native object behind the attribute that `_handle` names, freed by the library call that `_destroy` names."""
    _destroy: str
    _handle = "_p"

    def close(self):
        p = getattr(self, self._handle, None)
        if p:
            getattr(lib(), self._destroy)(p)
            setattr(self, self._handle, C.c_void_p())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Spectrogram(_NativeHandle):
    """Drop-in mirror of the reference's `Spectrogram` (engine half).  The channel count is explicit."""
    _destroy, _handle = "jsg_destroy", "_h"

    ChannelMixMode = type("ChannelMixMode", (), dict(AbsMean=0, Max=1, Min=2, Left=3, Right=4, PerChannel=100))
    Windows = type("Windows", (), dict(Rect=0, Hann=1, Hamming=2, BlackmanHarris=3, FlatTop=4, HannPoisson=5))
    FeedPercentage = type("FeedPercentage", (), dict(perc100=0, perc50=1, perc25=2, perc10=3))

    def __init__(self, channels: int = 2):
        self._h = C.c_void_p()
        check(lib().jsg_create(C.byref(self._h), int(channels)))

    def _c(self, rc):
        return check(rc, self._h)

    # setters (Spectrogram.h:116-123)
    def setSamplerate(self, fs): self._c(lib().jsg_set_samplerate(self._h, fs))
    def setchannels(self, c): self._c(lib().jsg_set_channels(self._h, int(c)))
    def setFFTSize(self, n): self._c(lib().jsg_set_fft_size(self._h, int(n)))
    def setclosestFFTSize_ms(self, ms): self._c(lib().jsg_set_closest_fft_size_ms(self._h, ms))
    def setmemoryTime_s(self, s): self._c(lib().jsg_set_memory_time_s(self._h, s))
    def setfeed_percent(self, feed): self._c(lib().jsg_set_feed_percent(self._h, int(feed)))
    def setfeed_percent_ext(self, pct): self._c(lib().jsg_set_feed_percent_ext(self._h, pct))
    def setPauseMode(self, mode): self._c(lib().jsg_set_pause_mode(self._h, int(bool(mode))))
    def setWindow(self, win): self._c(lib().jsg_set_window(self._h, int(win)))
    def setMixMode(self, mode): self._c(lib().jsg_set_mix_mode(self._h, int(mode)))
    def setPowerScale(self, s): self._c(lib().jsg_set_power_scale(self._h, s))
    def setExactLog(self, on): self._c(lib().jsg_set_exact_log(self._h, int(bool(on))))

    def setWindowTable(self, w):
        w = np.ascontiguousarray(w, dtype=np.float32)
        self._c(lib().jsg_set_window_table(self._h, w.ctypes.data, w.size))

    def getnextpowerof2(self, ms): return next_power_of_2(ms, self.getSamplerate())
    def getSpectrumSize(self): return lib().jsg_get_spectrum_size(self._h)
    def getMemorySize(self): return lib().jsg_get_memory_size(self._h)
    def getSamplerate(self): return lib().jsg_get_samplerate(self._h)
    def getFFTSize(self): return lib().jsg_get_fft_size(self._h)
    def getFeedSamples(self): return lib().jsg_get_feed_samples(self._h)
    def getFeedBlocks(self): return lib().jsg_get_feedblocks(self._h)
    def getChannels(self): return lib().jsg_get_channels(self._h)

    def getWindow(self):
        w = np.zeros(self.getFFTSize(), dtype=np.float32)
        self._c(lib().jsg_get_window(self._h, w.ctypes.data, w.size))
        return w

    def processSynchronBlock(self, data, midi=None, realtime: bool = False, timeout_ms: int = 10000) -> int:
        """data: [channels][fft size] float32 (reference: vector<vector<float>>&, Spectrogram.cpp:37).

        A Python caller is not an audio thread, so the default is the LOSSLESS entry point (jsg_process_block_wait): like the reference,
        no block is ever lost -- when the engine's 64-slot ring is full the call waits for the worker.  A block that still cannot be
        queued (geometry change in progress, timeout) raises instead of vanishing.  realtime=True: the wait-free call of a live host
        (jsg_process_block), which DROPS when the ring is full and returns 1; droppedBlocks() counts them."""
        data = np.ascontiguousarray(data, dtype=np.float32)
        n, ch = self.getFFTSize(), self.getChannels()
        if data.shape != (ch, n):
            raise JsgError(capi.JSG_ERR_SIZE_MISMATCH, f"block must be [{ch}][{n}], got {data.shape}")
        ptrs = (C.c_void_p * ch)(*[data[c].ctypes.data for c in range(ch)])
        if realtime:
            return self._c(lib().jsg_process_block(self._h, ptrs))
        rc = self._c(lib().jsg_process_block_wait(self._h, ptrs, ch, n, int(timeout_ms)))
        if rc == 1:
            raise JsgError(1, "processSynchronBlock: the block was dropped (geometry change in progress, or the ring stayed full "
                              f"for {timeout_ms} ms); pass realtime=True to get the wait-free, lossy call of a live host")
        return rc

    def droppedBlocks(self) -> int:
        return int(lib().jsg_get_dropped_blocks(self._h))

    def processBlocks(self, samples) -> int:
        """samples: [channels][K * fft size]; the same as K processSynchronBlock calls, one kernel launch."""
        samples = np.ascontiguousarray(samples, dtype=np.float32)
        n, ch = self.getFFTSize(), self.getChannels()
        if samples.ndim != 2 or samples.shape[0] != ch or samples.shape[1] % n:
            raise JsgError(capi.JSG_ERR_SIZE_MISMATCH, "samples must be [channels][K*fftsize]")
        return self._c(lib().jsg_process_blocks(self._h, samples.ctypes.data, samples.shape[1], samples.shape[1] // n))

    def processBlocksDevice(self, d_samples) -> int:
        """d_samples: torch float32 CUDA tensor [channels][K * fft size] already resident in HBM."""
        n, ch = self.getFFTSize(), self.getChannels()
        assert d_samples.is_cuda and d_samples.dtype.is_floating_point and d_samples.element_size() == 4
        assert d_samples.dim() == 2 and d_samples.shape[0] == ch and d_samples.shape[1] % n == 0
        assert d_samples.stride(1) == 1
        return self._c(lib().jsg_process_blocks_device(self._h, d_samples.data_ptr(), d_samples.stride(0),
                                                       d_samples.shape[1] // n))

    def getMem(self, mem: np.ndarray):
        """mem: caller's [W][H] float32 array, updated in place.  Returns (newVals, pos); newVals == -1 on a
        size mismatch like the reference (Spectrogram.cpp:297-298)."""
        if mem.dtype != np.float32 or not mem.flags.c_contiguous or mem.ndim != 2 or mem.shape[1] != self.getSpectrumSize():
            return -1, None
        pos = C.c_int(0)
        rc = lib().jsg_get_mem(self._h, mem.ctypes.data, mem.shape[0], C.byref(pos))
        if rc == capi.JSG_ERR_SIZE_MISMATCH:
            return -1, None
        self._c(rc)
        return rc, pos.value

    def ring_device(self):
        p, pitch, w, pos = C.c_void_p(), C.c_int64(), C.c_int(), C.c_int()
        self._c(lib().jsg_ring_device(self._h, C.byref(p), C.byref(pitch), C.byref(w), C.byref(pos)))
        return p.value, pitch.value, w.value, pos.value

    def sync(self): self._c(lib().jsg_sync(self._h))


class SpectrogramDisplay:
    """timerCallback's colour loop on the engine's device-resident ring (Spectrogram.cpp:590-731)."""

    def __init__(self, spectrogram: Spectrogram, n_colors: int = 256, scheme: int = capi.CM_JADE):
        self.spec = spectrogram
        spectrogram._c(lib().jsg_display_set_colormap(spectrogram._h, n_colors, scheme))

    def setColorSceme(self, scheme, n_colors: int = 256):
        self.spec._c(lib().jsg_display_set_colormap(self.spec._h, n_colors, int(scheme)))

    def setRunning(self, running: bool):
        self.spec._c(lib().jsg_display_set_running(self.spec._h, int(bool(running))))

    def invalidate(self):
        self.spec._c(lib().jsg_display_invalidate(self.spec._h))

    def setFrequencyAxis(self, scale: int, height: int = 0, fmin: float = 0.0, fmax: float = 0.0):
        """Image rows on a LINEAR / LOG / MEL axis over [fmin, fmax] Hz (capi.AXIS_BINS: one row per bin, the default).  Forces a full
        recolour; the image then has height() rows."""
        self.spec._c(lib().jsg_display_set_freq_axis(self.spec._h, int(scale), int(height), float(fmin), float(fmax)))

    def height(self) -> int:
        """Rows of the image the next timerCallback / timerCallbackTile writes."""
        return self.spec._c(lib().jsg_display_height(self.spec._h))

    def centres(self) -> np.ndarray:
        """Centre frequency (Hz) of every image row, bottom row first."""
        out = np.zeros(self.height(), np.float32)
        self.spec._c(lib().jsg_display_axis_centres(self.spec._h, out.ctypes.data, out.size))
        return out

    def timerCallback(self, img: np.ndarray, min_color=-50.0, max_color=50.0):
        """img: [height()][W] uint32 ARGB, updated in place.  Returns (newVals, pos)."""
        assert img.dtype == np.uint32 and img.ndim == 2 and img.strides[1] == 4
        assert img.shape[0] >= self.height(), "the image needs height() rows (the frequency axis sets them)"
        nv, pos = C.c_int(), C.c_int()
        self.spec._c(lib().jsg_display_update(self.spec._h, min_color, max_color, img.ctypes.data, img.strides[0] // 4,
                                              C.byref(nv), C.byref(pos)))
        return nv.value, pos.value


    def timerCallbackTile(self, tile: np.ndarray, min_color=-50.0, max_color=50.0):
        """Incremental tick: only the new columns, as a [height()][max_cols] tile (oldest first).  Returns
        (need_full, newVals, pos); need_full=True means call timerCallback() for the whole image instead."""
        assert tile.dtype == np.uint32 and tile.ndim == 2 and tile.strides[1] == 4
        assert tile.shape[0] >= self.height(), "the tile needs height() rows (the frequency axis sets them)"
        nv, pos = C.c_int(), C.c_int()
        rc = self.spec._c(lib().jsg_display_update_tile(self.spec._h, min_color, max_color, tile.ctypes.data,
                                                        tile.strides[0] // 4, tile.shape[1], C.byref(nv), C.byref(pos)))
        return rc == 1, nv.value, pos.value


def display_freq_rows(fs: float, height: int, min_freq: float, max_freq: float):
    """paint()'s frequency window (reference Spectrogram.cpp:441-459): (startPixel, endPixel, heightInterval, hStart)."""
    a, b, c, d = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    check(lib().jsg_display_freq_rows(fs, height, min_freq, max_freq, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
    return a.value, b.value, c.value, d.value


class CColorPalette:
    """Host mirror of the reference's CColorPalette: table + range on the host, bulk mapping on the GPU."""
    kMono, kBW, kHot, kRainbow, kViridis, kPlasma, kJade = range(7)

    def __init__(self, NrOfColors: int = 2, ColorScheme: int = 0):
        self.m_NrOfColors, self.m_ColorScheme = int(NrOfColors), int(ColorScheme)
        self.m_Color = colormap_lut(self.m_NrOfColors, self.m_ColorScheme)
        self.m_Min, self.m_Max, self.m_AccessMult = colormap_range(self.m_NrOfColors, 0.0, 1.0)
        self.m_Min, self.m_Max = np.float32(0.0), np.float32(1.0)

    def setValueRange(self, Min, Max):
        self.m_Min, self.m_Max, self.m_AccessMult = colormap_range(self.m_NrOfColors, Min, Max)

    def setNrOfColors(self, n):
        self.m_NrOfColors = int(n)
        self.m_AccessMult = np.float32(self.m_NrOfColors) / np.float32(self.m_Max - self.m_Min)
        self.m_Color = colormap_lut(self.m_NrOfColors, self.m_ColorScheme)

    def setColorSceme(self, scheme):
        self.m_ColorScheme = int(scheme)
        self.m_Color = colormap_lut(self.m_NrOfColors, self.m_ColorScheme)


# --------------------------------------------------------------------------------------------------
# stateless device ops on torch tensors
# --------------------------------------------------------------------------------------------------
class _PerDeviceHandles:
    """A description on the host and the native objects made from it in `_handles`, one per device: `_create(h)` makes the one of the
    current device, the library call that `_destroy` names frees one."""
    _destroy: str

    def handle(self, device: int | None = None) -> C.c_void_p:
        """The jsg_filterbank / jsg_freq_axis on `device` (default: the current one), created on first use."""
        import torch
        dev = torch.cuda.current_device() if device is None else int(device)
        h = self._handles.get(dev)
        if h is None:
            h = C.c_void_p()
            with torch.cuda.device(dev):
                self._create(h)
            self._handles[dev] = h
        return h

    def close(self):
        for h in getattr(self, "_handles", {}).values():
            getattr(lib(), self._destroy)(h)
        self._handles = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Plan(_NativeHandle):
    _destroy = "jsg_plan_destroy"

    def __init__(self, n: int, window_table: np.ndarray, power_scale: float = 1.0):
        w = np.ascontiguousarray(window_table, dtype=np.float32)
        assert w.size == n
        self._p = C.c_void_p()
        check(lib().jsg_plan_create(C.byref(self._p), int(n), w.ctypes.data, power_scale))
        self.n = int(n)


def _stream_handle(stream, tensor) -> C.c_void_p:
    """The caller's stream, or torch's current stream on the device of `tensor`, as the library takes it."""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream(tensor.device).cuda_stream
    return C.c_void_p(stream)


def _device_index(tensor) -> int:
    """The index of the tensor's device (a bare "cuda" device: the current one)."""
    if tensor.device.index is not None:
        return tensor.device.index
    import torch
    return torch.cuda.current_device()


def _scratch_and_stream(d_scratch, stream, tensor, count, dtype, any_dtype: bool = False):
    """(scratch, stream handle) of a launch that works through scratch memory, on the device of `tensor`.  d_scratch None: count()
    elements of `dtype` are allocated with torch for this call."""
    import torch
    temporary = d_scratch is None
    if temporary:
        d_scratch = torch.empty(int(count()), dtype=dtype, device=tensor.device)
    assert d_scratch.is_cuda and d_scratch.is_contiguous() and (any_dtype or d_scratch.dtype == dtype)
    if temporary and stream is not None:   # the caching allocator must not hand the block out again before the launch on the caller's stream is done
        d_scratch.record_stream(torch.cuda.ExternalStream(stream, device=tensor.device))
    return d_scratch, _stream_handle(stream, tensor)


def _kernel_name(query, *args) -> str:
    """The text a jsg_*_kernel_name query writes for `args`."""
    buf = C.create_string_buffer(32)
    check(query(*args, buf, 32))
    return buf.value.decode()


class StftLaunch:
    """A prepared launch: the argument block is filled once, `launch(stream)` is then a single FFI call
    (the per-call Python work of stft_db() is ~2 us, comparable to a short kernel)."""

    def __init__(self, plan: Plan, d_in, hop: int, n_frames: int, d_out, **kw):
        self._plan = plan
        self._keep = (d_in, d_out)
        self._args = _stft_args(plan, d_in, hop, n_frames, d_out, **kw)
        self._ref = C.byref(self._args)
        self._fn = lib().jsg_stft_db_launch

    def launch(self, stream: int):
        rc = self._fn(self._plan._p, self._ref, stream)
        if rc < 0:
            check(rc)


def stft_db(plan: Plan, d_in, hop: int, n_frames: int, d_out, *, feedblocks: int | None = None, mix_mode: int = 0,
            first_frame: int = 0, ring_pos: int = 0, linear_out: bool = False, blocks_per_cu: int = 0,
            stream: int | None = None, plan_select: int = 0, exact_log: bool = False, d_tail=None):
    """Enqueue one fused STFT->dB launch.  d_in: torch CUDA float32 [C][samples]; d_out: [W][pitch] (or
    [C][W][pitch] with mix_mode PER_CHANNEL).  Frame j starts at sample (j//feedblocks)*n + (j%feedblocks)*hop.
    d_tail: see _stft_args (jsg_stft_args.out_tail: bin n/2 in a dense plane, columns of n/2 floats)."""
    a = _stft_args(plan, d_in, hop, n_frames, d_out, feedblocks=feedblocks, mix_mode=mix_mode, first_frame=first_frame,
                   ring_pos=ring_pos, linear_out=linear_out, blocks_per_cu=blocks_per_cu, plan_select=plan_select, exact_log=exact_log, d_tail=d_tail)
    check(lib().jsg_stft_db_launch(plan._p, C.byref(a), _stream_handle(stream, d_in)))


def columns_from_tail_layout(d_db, d_tail, d_dst, *, n: int | None = None, stream: int | None = None):
    """jsg_columns_from_tail_layout_launch: d_db [W][pitch >= n/2] + d_tail [W] (the tail-plane layout of stft_db(..., d_tail=)) -> d_dst [W][>= n/2+1],
    the reference's dense column shape (what getMem hands out).  `n` = the FFT size (a Plan's .n); without it the rows of d_db must be
    exactly n/2 floats wide (the shape stft_db's tail layout is normally given) -- the height is never guessed from padded rows."""
    assert d_db.is_cuda and d_tail.is_cuda and d_dst.is_cuda and d_db.dim() == 2 and d_dst.dim() == 2 and d_db.stride(1) == 1 and d_dst.stride(1) == 1
    W = d_db.shape[0]
    assert d_tail.numel() == W and d_tail.is_contiguous() and d_dst.shape[0] == W
    if n is None:
        n = 2 * d_db.shape[1]
        if n < 2 or n & (n - 1):
            raise JsgError(capi.JSG_ERR_INVALID, f"columns_from_tail_layout: rows of {d_db.shape[1]} floats are not n/2 of a power-of-two FFT size; pass n=")
    H = n // 2 + 1
    if d_db.shape[1] < H - 1 or d_dst.shape[1] < H:
        raise JsgError(capi.JSG_ERR_INVALID, f"columns_from_tail_layout: n = {n} needs source rows of >= {H - 1} and destination rows of >= {H} floats")
    check(lib().jsg_columns_from_tail_layout_launch(d_db.data_ptr(), d_db.stride(0), d_tail.data_ptr(), W, H, d_dst.data_ptr(), d_dst.stride(0),
                                                    _stream_handle(stream, d_db)))


def stft_db_batches(plan: Plan, batches, hop: int, n_frames: int, *, stream: int | None = None, **kw):
    """jsg_stft_db_launch_batches: `batches` = [(d_in, d_out), ...] independent launches of the same geometry, stream-ordered with
    respect to `stream` like one launch but overlapped on the library's own working streams (include/jsg.h)."""
    arr = (capi.StftArgs * len(batches))()
    for i, (d_in, d_out) in enumerate(batches):
        a = _stft_args(plan, d_in, hop, n_frames, d_out, **kw)
        C.memmove(C.byref(arr, i * C.sizeof(capi.StftArgs)), C.byref(a), C.sizeof(capi.StftArgs))
    check(lib().jsg_stft_db_launch_batches(plan._p, arr, len(batches), _stream_handle(stream, batches[0][0])))


def _strided_args(plan: Plan, d_in, hop: int, n_frames: int, d_out, **kw):
    """d_in float32 [k][channels][samples], d_out [k][W][pitch] (per-channel mode: [k][channels][W][pitch]): batch b = d_in[b] -> d_out[b]."""
    assert d_in.dim() == 3 and d_in.stride(2) == 1 and d_out.shape[0] == d_in.shape[0] and d_out.stride(-1) == 1
    a = _stft_args(plan, d_in[0], hop, n_frames, d_out[0], **kw)
    return a, int(d_in.shape[0]), int(d_in.stride(0)), int(d_out.stride(0))


def stft_db_strided(plan: Plan, d_in, hop: int, n_frames: int, d_out, *, stream: int | None = None, **kw):
    """jsg_stft_db_launch_strided: k independent batches of one geometry in ONE kernel launch on one stream (include/jsg.h)."""
    a, k, s_in, s_out = _strided_args(plan, d_in, hop, n_frames, d_out, **kw)
    check(lib().jsg_stft_db_launch_strided(plan._p, C.byref(a), k, s_in, s_out, _stream_handle(stream, d_in)))


def stft_db_strided_kernel_name(plan: Plan, d_in, hop: int, n_frames: int, d_out, **kw) -> str:
    """The kernel every launch of a strided call takes: as stft_kernel_name, judged by the frames of the whole call (Max / Min, which go
    out batch by batch: of one batch)."""
    a, k, s_in, _ = _strided_args(plan, d_in, hop, n_frames, d_out, **kw)
    return _kernel_name(lib().jsg_stft_db_strided_kernel_name, plan._p, C.byref(a), k, s_in)


def stft_kernel_name(plan: Plan, d_in, hop: int, n_frames: int, d_out, **kw) -> str:
    """The kernel configuration jsg_stft_db_launch picks for this launch ("Cfg1024", "Cfg2048B", ...)."""
    a = _stft_args(plan, d_in, hop, n_frames, d_out, **kw)
    return _kernel_name(lib().jsg_stft_kernel_name, plan._p, C.byref(a))


def _stft_input_args(plan: Plan, d_in, hop, n_frames, ring_width, feedblocks, mix_mode, first_frame, ring_pos, linear_out, blocks_per_cu,
                     plan_select, exact_log) -> capi.StftArgs:
    """jsg_stft_args without its output pointers and pitches: the input rows, the framing, the ring geometry and the kernel switches."""
    import torch
    assert d_in.is_cuda and d_in.dtype == torch.float32 and d_in.dim() == 2 and d_in.stride(1) == 1
    channels, samples = d_in.shape
    a = capi.StftArgs()
    a.in_ = d_in.data_ptr()
    a.in_pitch = d_in.stride(0) if channels > 1 else samples
    a.in_samples = samples            # the launcher refuses frames that would read past the rows
    a.channels = channels
    a.hop = hop
    a.feedblocks = feedblocks if feedblocks is not None else max(1, plan.n // hop)
    a.mix_mode = mix_mode
    a.first_frame = first_frame
    a.n_frames = n_frames
    a.ring_width = ring_width
    a.ring_pos = ring_pos
    a.linear_out = bool(linear_out)
    a.blocks_per_cu = int(blocks_per_cu)
    a.exact_log = bool(exact_log)          # dB by the shared float32 routine (bit-reproducible on a CPU) instead of v_log_f32
    a.plan_select = int(plan_select)       # 0 automatic, 1 small-workgroup kernel, 2 "B" kernel (2048 / 4096 points), 3 pair plan (2048 points, even channel
                                           # counts, sum-type mixes); 1024 points: 2 = the two-stage kernel Cfg1024B (include/jsg.h)
    return a


def _stft_args(plan: Plan, d_in, hop: int, n_frames: int, d_out, *, feedblocks: int | None = None, mix_mode: int = 0,
               first_frame: int = 0, ring_pos: int = 0, linear_out: bool = False, blocks_per_cu: int = 0, plan_select: int = 0,
               exact_log: bool = False, d_tail=None, col_height: int | None = None):
    """d_tail (jsg_stft_args.out_tail): float32 CUDA tensor of rows x W floats (rows = 1, or channels in per-channel mode, times the batches
    of a strided launch), contiguous -- bin n/2 of every column goes there and a column of d_out is then n/2 floats.
    col_height: floats a column of d_out needs (default: the bins of the plan; the band count of a filterbank launch)."""
    a = _stft_input_args(plan, d_in, hop, n_frames, d_out.shape[-2], feedblocks, mix_mode, first_frame, ring_pos, linear_out, blocks_per_cu,
                         plan_select, exact_log)
    float32 = d_in.dtype               # (checked just above)
    assert d_out.is_cuda and d_out.dtype == float32 and d_out.stride(-1) == 1
    H = (plan.n // 2 + 1 - (1 if d_tail is not None else 0)) if col_height is None else int(col_height)
    if d_out.shape[-1] < H:
        raise JsgError(capi.JSG_ERR_INVALID, f"output rows hold {d_out.shape[-1]} floats, a column needs {H}")
    if mix_mode == capi.MIX_PER_CHANNEL and (d_out.dim() != 3 or d_out.shape[0] != a.channels):
        raise JsgError(capi.JSG_ERR_INVALID, "per-channel mode needs an output of [channels][W][pitch]")
    a.out_db = d_out.data_ptr()
    a.out_pitch = d_out.stride(-2)
    a.out_channel_pitch = d_out.stride(0) if d_out.dim() == 3 else 0
    if d_tail is not None:
        assert d_tail.is_cuda and d_tail.dtype == float32 and d_tail.is_contiguous() and d_tail.shape[-1] == a.ring_width
        a.out_tail = d_tail.data_ptr()
    return a


def colormap(d_db, d_lut, lo: float, hi: float, *, d_argb=None, d_index=None, col_first: int = 0, n_cols: int | None = None,
             x_first: int = 0, height: int | None = None, stream: int | None = None):
    """Enqueue the colour loop: d_db [W][pitch] float32 CUDA -> d_argb [H][Wimg] int32/uint32 and/or d_index uint8."""
    a = _colormap_args(d_db, d_lut, lo, hi, d_argb, d_index, col_first, n_cols, x_first, height)
    check(lib().jsg_colormap_launch(C.byref(a), _stream_handle(stream, d_db)))


def colormap_axis(d_db, d_lut, lo: float, hi: float, axis: "FreqAxis", *, d_argb=None, d_index=None, col_first: int = 0,
                  n_cols: int | None = None, x_first: int = 0, stream: int | None = None):
    """colormap() over the rows of a FreqAxis: d_db [W][pitch >= n/2+1] float32 CUDA -> d_argb / d_index of axis.height rows."""
    a = _colormap_args(d_db, d_lut, lo, hi, d_argb, d_index, col_first, n_cols, x_first, axis.n // 2 + 1)
    check(lib().jsg_colormap_axis_launch(C.byref(a), axis.handle(d_db.device.index), _stream_handle(stream, d_db)))


def _colour_args(ring_width, height, col_first, n_cols, x_first, d_lut, lo, hi, d_argb, d_index) -> capi.ColormapArgs:
    """jsg_colormap_args without its dB ring: the columns, the palette with its range, and the image(s) they go to."""
    a = capi.ColormapArgs()
    a.ring_width = ring_width
    a.height = height
    a.col_first = col_first
    a.n_cols = n_cols
    a.x_first = x_first
    a.lut = d_lut.data_ptr()
    a.n_colors = d_lut.numel()
    F = capi.ColormapArgs       # the library writes the range straight into the block
    check(lib().jsg_colormap_range(a.n_colors, lo, hi, C.byref(a, F.vmin.offset), C.byref(a, F.vmax.offset), C.byref(a, F.access_mult.offset)))
    if d_argb is not None:
        a.argb_out = d_argb.data_ptr()
        a.argb_pitch = d_argb.stride(0)
        a.x_wrap = d_argb.shape[1]
    if d_index is not None:
        a.index_out = d_index.data_ptr()
        a.index_pitch = d_index.stride(0)
        a.x_wrap = d_index.shape[1]
    return a


def _colormap_args(d_db, d_lut, lo, hi, d_argb, d_index, col_first, n_cols, x_first, height) -> capi.ColormapArgs:
    a = _colour_args(d_db.shape[0], height if height is not None else d_db.shape[1], col_first, n_cols if n_cols is not None else d_db.shape[0],
                     x_first, d_lut, lo, hi, d_argb, d_index)
    a.db = d_db.data_ptr()
    a.db_pitch = d_db.stride(0)
    return a


def _stft_image_args(plan: Plan, d_in, hop: int, n_frames: int, d_lut, lo: float, hi: float, d_argb, d_index_scratch, *,
                     feedblocks: int | None = None, mix_mode: int = 0, first_frame: int = 0, ring_pos: int = 0,
                     ring_width: int | None = None, x_first: int | None = None, plan_select: int = 0, exact_log: bool = False,
                     blocks_per_cu: int = 0):
    assert d_argb.is_cuda and d_argb.element_size() == 4 and d_argb.dim() == 2 and d_argb.stride(1) == 1
    if d_index_scratch is not None:
        import torch
        assert d_index_scratch.is_cuda and d_index_scratch.dtype == torch.uint8 and d_index_scratch.dim() == 2 and d_index_scratch.stride(1) == 1
    W = ring_width if ring_width is not None else (d_index_scratch.shape[0] if d_index_scratch is not None else n_frames)
    a = capi.StftImageArgs()
    a.stft = _stft_input_args(plan, d_in, hop, n_frames, W, feedblocks, mix_mode, first_frame, ring_pos, False, blocks_per_cu, plan_select, exact_log)
    a.colour = _colour_args(W, plan.n // 2 + 1, ring_pos, n_frames, ring_pos if x_first is None else x_first, d_lut, lo, hi, d_argb, None)
    if d_index_scratch is not None:
        a.index_scratch = d_index_scratch.data_ptr()
        a.index_scratch_pitch = d_index_scratch.stride(0)
    return a


def stft_image(plan: Plan, d_in, hop: int, n_frames: int, d_lut, lo: float, hi: float, d_argb, d_index_scratch=None, *,
               stream: int | None = None, **kw):
    """Fused display path (jsg_stft_image_launch): STFT -> palette index -> ARGB rows of d_argb [n/2+1][Wimg]; no dB column is
    written.  One kernel where the plan's workgroups hold eight whole columns (1024 points; 4096 points when the launch takes
    the "B" kernel), else two kernels through d_index_scratch (uint8 [ring_width][pitch >= n/2+1]; stft_image_needs_scratch()).
    The image equals stft_db() + colormap() bit for bit, with the same plan_select -- except at 1024 points, where the display launches
    always take the three-stage arithmetic: the image is that of stft_db(plan_select=1) + colormap() whatever plan_select says."""
    a = _stft_image_args(plan, d_in, hop, n_frames, d_lut, lo, hi, d_argb, d_index_scratch, **kw)
    check(lib().jsg_stft_image_launch(plan._p, C.byref(a), _stream_handle(stream, d_in)))


def stft_image_needs_scratch(plan: Plan, d_in, hop: int, n_frames: int, d_lut, lo: float, hi: float, d_argb, d_index_scratch=None, **kw) -> bool:
    """True when jsg_stft_image_launch runs as two kernels for this launch and therefore needs the index scratch."""
    a = _stft_image_args(plan, d_in, hop, n_frames, d_lut, lo, hi, d_argb, d_index_scratch, **kw)
    return bool(check(lib().jsg_stft_image_needs_scratch(plan._p, C.byref(a))))


def stft_image_strided(plan: Plan, d_in, hop: int, n_frames: int, d_lut, lo: float, hi: float, d_argb, d_index_scratch=None, *,
                       stream: int | None = None, **kw):
    """`k` images of one geometry from one call (jsg_stft_image_launch_strided): d_in float32 [k][channels][samples], d_argb
    int32 / uint32 [k][n/2+1][Wimg].  One kernel launch for all of them where the single-kernel form applies to the total size
    (stft_image_strided_needs_scratch() tells), else k launches in stream order."""
    assert d_in.dim() == 3 and d_argb.dim() == 3 and d_in.shape[0] == d_argb.shape[0] and d_in.stride(2) == 1 and d_argb.stride(2) == 1
    assert d_argb.shape[1] >= plan.n // 2 + 1, "image rows: one per bin"
    assert d_in.shape[0] == 1 or d_in.stride(0) == 0 or d_in.stride(0) >= (d_in.shape[1] - 1) * d_in.stride(1) + d_in.shape[2], "images overlap in the input"
    a = _stft_image_args(plan, d_in[0], hop, n_frames, d_lut, lo, hi, d_argb[0], d_index_scratch, **kw)
    check(lib().jsg_stft_image_launch_strided(plan._p, C.byref(a), int(d_in.shape[0]), int(d_in.stride(0)), int(d_argb.stride(0)),
                                              _stream_handle(stream, d_in)))


def stft_image_strided_needs_scratch(plan: Plan, d_in, hop: int, n_frames: int, d_lut, lo: float, hi: float, d_argb, d_index_scratch=None,
                                     **kw) -> bool:
    a = _stft_image_args(plan, d_in[0], hop, n_frames, d_lut, lo, hi, d_argb[0], d_index_scratch, **kw)
    return bool(check(lib().jsg_stft_image_strided_needs_scratch(plan._p, C.byref(a), int(d_in.shape[0]))))


def db_from_power(d_power, d_out, divisor: float = 1.0, stream: int | None = None, *, exact_log: bool = False):
    """out = 10*log10(power/divisor + 1e-11f) elementwise on the GPU (finishes a cross-GPU AbsMean).  exact_log: the shared float32
    logarithm of jsg_stft_args.exact_log (bit-reproducible on a CPU) instead of the hardware unit (jsg_db_from_power_launch_ex)."""
    import torch
    assert d_power.is_cuda and d_power.dtype == torch.float32 and d_power.is_contiguous()
    assert d_out.is_cuda and d_out.dtype == torch.float32 and d_out.is_contiguous() and d_out.numel() == d_power.numel()
    check(lib().jsg_db_from_power_launch_ex(d_power.data_ptr(), d_out.data_ptr(), d_power.numel(), divisor, int(bool(exact_log)),
                                            _stream_handle(stream, d_power)))


# --------------------------------------------------------------------------------------------------
# filterbank spectrograms: mel and log-frequency rows (include/jsg.h, section 2b)
# --------------------------------------------------------------------------------------------------
class Filterbank(_PerDeviceHandles):
    """A sparse, banded filterbank over the n/2+1 bins of an n-point FFT (CSR: band b = weights[offset[b] : offset[b] + n_bins[b]]
    over the bins first_bin[b] ..).  Built on the host by jsg_filterbank_build (no GPU needed) or taken from a dense matrix; uploaded to
    a device once, the first time a launch on that device needs it.

        Filterbank(n, fs, n_bands, fmin, fmax, scale=capi.FB_MEL_SLANEY, norm=None)
            norm None: NORM_SLANEY for the mel scales (librosa's default), NORM_UNIT_SUM for LOG / LINEAR.
        Filterbank.from_matrix(W)       W [n_bands][n/2+1]: every row keeps the span from its first to its last nonzero
    """
    _destroy = "jsg_filterbank_destroy"

    def __init__(self, n: int, fs: float, n_bands: int, fmin: float = 0.0, fmax: float | None = None, scale: int = capi.FB_MEL_SLANEY,
                 norm: int | None = None):
        if fmax is None:
            fmax = fs / 2.0
        if norm is None:
            norm = capi.FB_NORM_SLANEY if scale in (capi.FB_MEL_SLANEY, capi.FB_MEL_HTK) else capi.FB_NORM_UNIT_SUM
        self.spec = capi.FbSpec(int(n), float(fs), int(n_bands), float(fmin), float(fmax), int(scale), int(norm))
        nnz = C.c_int64()
        check(lib().jsg_filterbank_build(C.byref(self.spec), None, None, None, None, None, 0, C.byref(nnz)))
        B = int(n_bands)
        self.first_bin = np.zeros(B, np.int32)
        self.n_bins = np.zeros(B, np.int32)
        self.offset = np.zeros(B, np.int32)
        self.centres_hz = np.zeros(B, np.float32)
        self.weights = np.zeros(max(1, nnz.value), np.float32)
        check(lib().jsg_filterbank_build(C.byref(self.spec), self.first_bin.ctypes.data, self.n_bins.ctypes.data, self.offset.ctypes.data,
                                         self.centres_hz.ctypes.data, self.weights.ctypes.data, self.weights.size, C.byref(nnz)))
        self.weights = self.weights[:nnz.value]
        self.n, self.n_bands, self._dense = int(n), B, None
        self._handles = {}

    @classmethod
    def from_matrix(cls, W) -> "Filterbank":
        W = np.ascontiguousarray(W, dtype=np.float32)
        assert W.ndim == 2 and W.shape[1] >= 257
        self = cls.__new__(cls)
        self.n, self.n_bands = 2 * (W.shape[1] - 1), W.shape[0]
        self.spec, self._dense, self._handles = None, W, {}
        first, count, off, w = [], [], [], []
        for row in W:
            nz = np.flatnonzero(row)
            a, e = (int(nz[0]), int(nz[-1]) + 1) if nz.size else (0, 0)
            first.append(a)
            count.append(e - a)
            off.append(sum(len(x) for x in w))
            w.append(row[a:e])
        self.first_bin, self.n_bins, self.offset = (np.array(v, np.int32) for v in (first, count, off))
        self.weights = np.concatenate(w).astype(np.float32) if w else np.zeros(0, np.float32)
        self.centres_hz = None
        return self

    def matrix(self) -> np.ndarray:
        """The bank as a dense [n_bands][n/2+1] float32 matrix (zeros outside every band's span)."""
        out = np.zeros((self.n_bands, self.n // 2 + 1), np.float32)
        for b in range(self.n_bands):
            out[b, self.first_bin[b]:self.first_bin[b] + self.n_bins[b]] = self.weights[self.offset[b]:self.offset[b] + self.n_bins[b]]
        return out

    def _create(self, h):
        if self.spec is not None:
            check(lib().jsg_filterbank_create(C.byref(h), C.byref(self.spec)))
        else:
            check(lib().jsg_filterbank_create_matrix(C.byref(h), self.n, self.n_bands, self._dense.ctypes.data))

    def device_weights(self, device: int | None = None) -> np.ndarray:
        """jsg_filterbank_weights of the device object: the bank as the library holds it."""
        out = np.zeros((self.n_bands, self.n // 2 + 1), np.float32)
        check(lib().jsg_filterbank_weights(self.handle(device), out.ctypes.data))
        return out


# --------------------------------------------------------------------------------------------------
# display frequency axes: linear / log / mel image rows (include/jsg.h, section 2c)
# --------------------------------------------------------------------------------------------------
class FreqAxis(_PerDeviceHandles):
    """`height` image rows over [fmin, fmax] Hz of an n-point FFT at fs, on a LINEAR, LOG or MEL axis (row 0 = bottom row).  The row
    table is built on the host by jsg_freq_axis_build (no GPU needed); uploaded to a device once, the first time it is used there.
    The defaults (LINEAR over [0, fs/2]) are valid for every scale but LOG, which needs fmin > 0."""
    _destroy = "jsg_freq_axis_destroy"

    def __init__(self, n: int, fs: float, height: int, fmin: float = 0.0, fmax: float | None = None, scale: int = capi.AXIS_LINEAR):
        if fmax is None:
            fmax = fs / 2.0
        self.spec = capi.AxisSpec(int(n), float(fs), int(scale), int(height), float(fmin), float(fmax))
        self.n, self.height = int(n), int(height)
        H = max(0, self.height)
        self.first_bin, self.n_bins = np.zeros(H, np.int32), np.zeros(H, np.int32)
        self.interp_t, self.centres_hz = np.zeros(H, np.float32), np.zeros(H, np.float32)
        check(lib().jsg_freq_axis_build(C.byref(self.spec), self.first_bin.ctypes.data, self.n_bins.ctypes.data,
                                        self.interp_t.ctypes.data, self.centres_hz.ctypes.data))
        self._handles = {}

    def rows(self):
        """(first_bin, n_bins, interp_t, centre_hz): the row table, height entries each."""
        return self.first_bin, self.n_bins, self.interp_t, self.centres_hz

    def _create(self, h):
        check(lib().jsg_freq_axis_create(C.byref(h), C.byref(self.spec)))


def _fb_args(plan: Plan, fb: Filterbank, d_in, hop: int, n_frames: int, d_out, strided: bool, **kw):
    if strided:
        return _strided_args(plan, d_in, hop, n_frames, d_out, col_height=fb.n_bands, **kw)
    return _stft_args(plan, d_in, hop, n_frames, d_out, col_height=fb.n_bands, **kw), 1, 0, 0


def stft_fb_scratch_floats(plan: Plan, fb: Filterbank, d_in, hop: int, n_frames: int, d_out, *, strided: bool = False, **kw) -> int:
    """jsg_stft_fb_scratch_floats: the scratch size (floats) the library recommends for this call."""
    a, k, _, _ = _fb_args(plan, fb, d_in, hop, n_frames, d_out, strided, **kw)
    return int(check(lib().jsg_stft_fb_scratch_floats(plan._p, fb.handle(d_in.device.index), C.byref(a), k)))


def _fb_launch(plan, fb, d_in, hop, n_frames, d_out, strided, d_scratch, stream, kw):
    import torch
    a, k, s_in, s_out = _fb_args(plan, fb, d_in, hop, n_frames, d_out, strided, **kw)
    h = fb.handle(d_in.device.index)
    d_scratch, stream = _scratch_and_stream(d_scratch, stream, d_in, lambda: check(lib().jsg_stft_fb_scratch_floats(plan._p, h, C.byref(a), k)),
                                            torch.float32)
    check(lib().jsg_stft_fb_launch_strided(plan._p, h, C.byref(a), k, s_in, s_out, d_scratch.data_ptr(), d_scratch.numel(), stream))


def stft_fb_db(plan: Plan, fb: Filterbank, d_in, hop: int, n_frames: int, d_out, *, d_scratch=None, stream: int | None = None, **kw):
    """jsg_stft_fb_launch: the columns of stft_db with the filterbank applied.  d_out [W][pitch >= n_bands] (per-channel mode:
    [C][W][pitch]); d_scratch: float32 CUDA tensor (None: one of the recommended size is allocated with torch for this call).
    Keywords as stft_db (linear_out: band power instead of dB; exact_log: the bit-reproducible logarithm)."""
    _fb_launch(plan, fb, d_in, hop, n_frames, d_out, False, d_scratch, stream, kw)


def stft_fb_db_strided(plan: Plan, fb: Filterbank, d_in, hop: int, n_frames: int, d_out, *, d_scratch=None, stream: int | None = None, **kw):
    """jsg_stft_fb_launch_strided: d_in [k][channels][samples] -> d_out [k][W][pitch] (per-channel: [k][C][W][pitch]), one call."""
    _fb_launch(plan, fb, d_in, hop, n_frames, d_out, True, d_scratch, stream, kw)


def stft_fb_kernel_name(plan: Plan, fb: Filterbank, d_in, hop: int, n_frames: int, d_out, *, strided: bool = False, **kw) -> str:
    """The STFT kernel every chunk of this filterbank call takes (decided once for the whole call)."""
    a, k, _, _ = _fb_args(plan, fb, d_in, hop, n_frames, d_out, strided, **kw)
    return _kernel_name(lib().jsg_stft_fb_kernel_name, plan._p, fb.handle(d_in.device.index), C.byref(a), k)


def fb_band_plan(n: int, n_bands: int, nnz: int, n_cols: int, n_cu: int) -> dict:
    """jsg_fb_band_plan: how the band kernel of one chunk of n_cols power columns is launched -- tile_cols, bank_in_lds, pw_pitch,
    lds_bytes, grid (host arithmetic only; what the launcher itself uses)."""
    v = [C.c_int32() for _ in range(5)]
    check(lib().jsg_fb_band_plan(int(n), int(n_bands), int(nnz), int(n_cols), int(n_cu), *(C.byref(x) for x in v)))
    tile_cols, bank_in_lds, pw_pitch, lds_bytes, grid = (x.value for x in v)
    return dict(tile_cols=tile_cols, bank_in_lds=bool(bank_in_lds), pw_pitch=pw_pitch, lds_bytes=lds_bytes, grid=grid)


_mel_cache: dict = {}
_window_table = window      # (mel_spectrogram_db takes a `window` argument)


def mel_spectrogram_db(x, fs: float, n_fft: int, hop: int, n_mels: int, fmin: float = 0.0, fmax: float | None = None,
                       window: int = capi.WIN_HANN, mix_mode: int = capi.MIX_ABSMEAN, exact_log: bool = False):
    """Mel spectrogram in dB of a torch CUDA tensor x ([samples] or [channels][samples], float32): Slaney mels with Slaney
    normalisation (librosa.feature.melspectrogram's bank), frames at t * hop (no padding), 10*log10(band power + 1e-11).
    hop must divide n_fft (the kernels' regular framing, hop * feedblocks = n_fft; other hops are refused with JSG_ERR_INVALID).
    Returns a new tensor [frames][n_mels] on x.device.  Plan and Filterbank are cached per geometry."""
    return _mel_plane(x, fs, n_fft, hop, n_mels, fmin, fmax, window, mix_mode, exact_log, False)


def _mel_plane(x, fs, n_fft, hop, n_mels, fmin, fmax, window, mix_mode, exact_log, linear_out):
    """mel_spectrogram_db, or with linear_out the band power in front of its logarithm."""
    import torch
    if hop <= 0 or hop > n_fft or n_fft % hop:
        raise JsgError(capi.JSG_ERR_INVALID, f"mel_spectrogram_db: hop {hop} must divide n_fft {n_fft} (frames at t * hop)")
    if x.dim() == 1:
        x = x[None, :]
    x = x.contiguous().float()
    assert x.is_cuda
    frames = 1 + (x.shape[1] - n_fft) // hop
    if frames < 1:
        raise JsgError(capi.JSG_ERR_INVALID, f"mel_spectrogram_db: {x.shape[1]} samples hold no frame of {n_fft}")
    dev = _device_index(x)
    key = (dev, int(n_fft), int(window), float(fs), int(n_mels), float(fmin), None if fmax is None else float(fmax))
    if key not in _mel_cache:
        with torch.cuda.device(dev):
            _mel_cache[key] = (Plan(n_fft, _window_table(window, n_fft)),
                               Filterbank(n_fft, fs, n_mels, fmin, fmax, scale=capi.FB_MEL_SLANEY, norm=capi.FB_NORM_SLANEY))
    plan, fb = _mel_cache[key]
    out = torch.empty((frames, n_mels), dtype=torch.float32, device=x.device)
    with torch.cuda.device(dev):
        stft_fb_db(plan, fb, x, hop, frames, out, feedblocks=n_fft // hop, mix_mode=mix_mode, exact_log=exact_log, linear_out=linear_out)
    return out


# --------------------------------------------------------------------------------------------------
# complex STFT and inverse STFT with any hop (include/jsg.h, section 2d)
# --------------------------------------------------------------------------------------------------
class CStftPlan(_NativeHandle):
    """jsg_cstft: window, twiddle tables and w^2 for one FFT size, resident on the current device."""
    _destroy = "jsg_cstft_destroy"

    def __init__(self, n: int, window_table: np.ndarray):
        import torch
        w = np.ascontiguousarray(window_table, dtype=np.float32)
        assert w.size == n
        self.window = w
        self._p = C.c_void_p()
        check(lib().jsg_cstft_create(C.byref(self._p), int(n), w.ctypes.data))
        self.n = int(n)
        self.device = torch.cuda.current_device()


def _rows3(t, what: str):
    """[rows][frames][bins] view of a 2- or 3-dimensional tensor (a 2-dimensional one is one row)."""
    if t.dim() == 2:
        t = t[None]
    assert t.dim() == 3, f"{what}: expected [rows][frames][bins]"
    return t


def _frame_major(X):
    """complex64 [rows][frames][bins] with unit bin stride of a [..., bins, frames] tensor (the library's frame-major layout)."""
    import torch
    Xf = X.to(torch.complex64).transpose(-1, -2).reshape(-1, X.shape[-1], X.shape[-2])
    return Xf if Xf.stride(2) == 1 else Xf.contiguous()


def _cstft_args(plan: CStftPlan, d_in, hop: int, n_frames: int, d_out, in_samples: int | None) -> capi.CstftArgs:
    import torch
    x = d_in[None] if d_in.dim() == 1 else d_in
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1, "d_in: float32 CUDA [rows][samples]"
    o = _rows3(d_out, "d_out")
    assert o.is_cuda and o.dtype == torch.complex64 and o.stride(2) == 1 and o.shape[0] == x.shape[0], "d_out: complex64 CUDA [rows][frames][bins]"
    return capi.CstftArgs(x.data_ptr(), x.stride(0), x.shape[0], int(hop), int(n_frames),
                          x.shape[1] if in_samples is None else int(in_samples), o.data_ptr(), o.stride(1), o.stride(0))


def cstft(plan: CStftPlan, d_in, hop: int, n_frames: int, d_out, *, in_samples: int | None = None, stream: int | None = None):
    """jsg_cstft_launch: d_in float32 [rows][samples] (frame j of a row at j * hop, any hop 1..n) -> d_out complex64 [rows][frames][>= n/2+1],
    the bins of numpy.fft.rfft(window * frame).  in_samples: the readable length of a row (default d_in.shape[-1]; 0: not checked)."""
    a = _cstft_args(plan, d_in, hop, n_frames, d_out, in_samples)
    check(lib().jsg_cstft_launch(plan._p, C.byref(a), _stream_handle(stream, d_in)))


def _istft_args(plan: CStftPlan, d_X, hop: int, n_frames: int, d_out, out_samples: int | None) -> capi.IstftArgs:
    import torch
    X = _rows3(d_X, "d_X")
    assert X.is_cuda and X.dtype == torch.complex64 and X.stride(2) == 1, "d_X: complex64 CUDA [rows][frames][>= n/2+1]"
    y = d_out[None] if d_out.dim() == 1 else d_out
    assert y.is_cuda and y.dtype == torch.float32 and y.dim() == 2 and y.stride(1) == 1 and y.shape[0] == X.shape[0], "d_out: float32 CUDA [rows][samples]"
    T = int(y.shape[1]) if out_samples is None else int(out_samples)
    return capi.IstftArgs(X.data_ptr(), X.stride(1), X.stride(0), X.shape[0], int(hop), int(n_frames), y.data_ptr(), y.stride(0), T)


def istft_scratch_floats(plan: CStftPlan, d_X, hop: int, n_frames: int, d_out, out_samples: int | None = None) -> int:
    """jsg_istft_scratch_floats: the scratch size (floats) the library recommends for this call."""
    a = _istft_args(plan, d_X, hop, n_frames, d_out, out_samples)
    return int(check(lib().jsg_istft_scratch_floats(plan._p, C.byref(a))))


def istft_launch(plan: CStftPlan, d_X, hop: int, n_frames: int, d_out, out_samples: int | None = None, *, d_scratch=None,
                 stream: int | None = None):
    """jsg_istft_launch: d_X complex64 [rows][frames][>= n/2+1] -> d_out float32 [rows][>= out_samples], torch.istft's overlap-add
    (frames at j * hop, no centring; 0 where the envelope is <= 1e-11).  d_scratch: float32 CUDA tensor (None: one of the recommended
    size is allocated with torch for this call); any accepted size gives the same bits."""
    import torch
    a = _istft_args(plan, d_X, hop, n_frames, d_out, out_samples)
    d_scratch, stream = _scratch_and_stream(d_scratch, stream, d_out, lambda: check(lib().jsg_istft_scratch_floats(plan._p, C.byref(a))), torch.float32)
    check(lib().jsg_istft_launch(plan._p, C.byref(a), d_scratch.data_ptr(), d_scratch.numel(), stream))


def istft_nola(n: int, hop: int, window_table) -> tuple[bool, float]:
    """jsg_istft_nola: (passes, smallest interior envelope min_rho sum_{m = rho mod hop} w[m]^2)."""
    w = np.ascontiguousarray(window_table, dtype=np.float32)
    assert w.size == n
    v = C.c_float()
    rc = lib().jsg_istft_nola(int(n), int(hop), w.ctypes.data, C.byref(v))
    if rc == capi.JSG_ERR_INVALID and np.isfinite(v.value) and 1 <= hop <= n:
        return False, float(v.value)
    check(rc)
    return True, float(v.value)


_cstft_cache: dict = {}


def _stft_window(window, n_fft: int, win_length: int) -> np.ndarray:
    """torch.stft's window: None = rectangular, a tensor / array, or a jsg_window id; a shorter one is zero-padded to the centre."""
    if window is None:
        w = np.ones(win_length, np.float32)
    elif isinstance(window, (int, np.integer)):
        w = _window_table(int(window), win_length)
    else:
        w = (window.detach().cpu().numpy() if hasattr(window, "detach") else np.asarray(window)).astype(np.float32).ravel()
    if w.size != win_length:
        raise JsgError(capi.JSG_ERR_INVALID, f"window has {w.size} samples, win_length is {win_length}")
    if win_length > n_fft:
        raise JsgError(capi.JSG_ERR_INVALID, f"win_length {win_length} > n_fft {n_fft}")
    out = np.zeros(n_fft, np.float32)
    left = (n_fft - win_length) // 2
    out[left:left + win_length] = w
    return out


def _cstft_plan(dev: int, n_fft: int, w: np.ndarray) -> CStftPlan:
    import torch
    key = (dev, int(n_fft), w.tobytes())
    if key not in _cstft_cache:
        with torch.cuda.device(dev):
            _cstft_cache[key] = CStftPlan(n_fft, w)
    return _cstft_cache[key]


def stft(x, n_fft: int, hop_length: int | None = None, win_length: int | None = None, window=None, center: bool = True,
         pad_mode: str = "reflect"):
    """torch.stft(..., return_complex=True, onesided=True, normalized=False) on the GPU: x float32 CUDA [..., samples] ->
    complex64 [..., n_fft//2+1, frames] (the transposed view of the library's frame-major buffer).  Any hop in 1..n_fft."""
    import torch
    import torch.nn.functional as Fn
    hop = n_fft // 4 if hop_length is None else int(hop_length)
    wl = n_fft if win_length is None else int(win_length)
    w = _stft_window(window, n_fft, wl)
    assert x.is_cuda, "stft: x must be a CUDA tensor"
    batch = tuple(x.shape[:-1])
    xr = x.reshape(-1, x.shape[-1]).float()
    if center:
        xr = Fn.pad(xr[:, None, :], (n_fft // 2, n_fft // 2), mode=pad_mode)[:, 0]
    xr = xr.contiguous()
    L = int(xr.shape[1])
    if L < n_fft:
        raise JsgError(capi.JSG_ERR_INVALID, f"stft: {L} samples hold no frame of {n_fft}")
    frames = 1 + (L - n_fft) // hop
    dev = _device_index(x)
    plan = _cstft_plan(dev, n_fft, w)
    out = torch.empty((xr.shape[0], frames, n_fft // 2 + 1), dtype=torch.complex64, device=x.device)
    with torch.cuda.device(dev):
        cstft(plan, xr, hop, frames, out)
    return out.reshape(*batch, frames, n_fft // 2 + 1).transpose(-1, -2)


def _envelope(w: np.ndarray, hop: int, frames: int) -> np.ndarray:
    """sum_j w[t - j hop]^2 in float64 for t < (frames-1) hop + n."""
    n = w.size
    w2 = w.astype(np.float64) ** 2
    P = -(-n // hop)
    pieces = np.zeros((P, hop))
    pieces.ravel()[:n] = w2
    E = np.zeros((frames + P, hop))
    for p in range(P):
        E[p:p + frames] += pieces[p]
    return E.ravel()[:(frames - 1) * hop + n]


def istft(X, n_fft: int, hop_length: int | None = None, win_length: int | None = None, window=None, center: bool = True,
          length: int | None = None):
    """torch.istft on the GPU: X complex CUDA [..., n_fft//2+1, frames] -> float32 [..., samples].  Raises JsgError where torch raises:
    the window envelope is <= 1e-11 somewhere inside the returned span."""
    import torch
    import torch.nn.functional as Fn
    hop = n_fft // 4 if hop_length is None else int(hop_length)
    wl = n_fft if win_length is None else int(win_length)
    w = _stft_window(window, n_fft, wl)
    assert X.is_cuda and X.is_complex(), "istft: X must be a complex CUDA tensor"
    if X.shape[-2] != n_fft // 2 + 1:
        raise JsgError(capi.JSG_ERR_INVALID, f"istft: {X.shape[-2]} bins, expected n_fft//2+1 = {n_fft // 2 + 1}")
    batch = tuple(X.shape[:-2])
    frames = int(X.shape[-1])
    Xf = _frame_major(X)
    T = (frames - 1) * hop + n_fft
    start = n_fft // 2 if center else 0
    end = (T - n_fft // 2 if center else T) if length is None else start + int(length)
    stop = min(end, T)
    env = _envelope(w, hop, frames)[start:stop]
    if env.size and not (np.abs(env) > 1e-11).all():
        raise JsgError(capi.JSG_ERR_INVALID, f"istft: window overlap-add envelope <= 1e-11 at sample {start + int(np.argmin(np.abs(env)))}")
    dev = _device_index(X)
    plan = _cstft_plan(dev, n_fft, w)
    y = torch.empty((Xf.shape[0], max(stop, 1)), dtype=torch.float32, device=X.device)
    with torch.cuda.device(dev):
        istft_launch(plan, Xf, hop, frames, y, max(stop, 1))
    y = y[:, start:stop]
    if end > stop:
        y = Fn.pad(y, (0, end - stop))
    return y.contiguous().reshape(*batch, -1)


# --------------------------------------------------------------------------------------------------
# phase vocoder and time stretch (include/jsg.h, section 2e)
# --------------------------------------------------------------------------------------------------
def pvoc_frames(n_frames: int, rate: float) -> int:
    """jsg_pvoc_frames: the number of output frames i >= 0 with float(i) * rate < n_frames."""
    return int(check(lib().jsg_pvoc_frames(int(n_frames), float(rate))))


def _pvoc_args(d_X, rate: float, hop: int, n: int, d_out, chunk_frames: int) -> capi.PvocArgs:
    import torch
    X, Y = _rows3(d_X, "d_X"), _rows3(d_out, "d_out")
    assert X.is_cuda and X.dtype == torch.complex64 and X.stride(2) == 1, "d_X: complex64 CUDA [rows][frames][>= n/2+1]"
    assert Y.is_cuda and Y.dtype == torch.complex64 and Y.stride(2) == 1 and Y.shape[0] == X.shape[0], "d_out: complex64 CUDA [rows][frames][>= n/2+1]"
    return capi.PvocArgs(X.data_ptr(), X.stride(1), X.stride(0), X.shape[0], int(n), int(hop), X.shape[1], float(rate),
                         Y.data_ptr(), Y.stride(1), Y.stride(0), Y.shape[1], int(chunk_frames))


def phase_vocoder_launch(d_X, rate: float, hop: int, n: int, d_out, *, chunk_frames: int = 0, d_scratch=None, stream: int | None = None):
    """jsg_pvoc_launch: d_X complex64 [rows][T][>= n/2+1] (frames taken with `hop` at FFT size n) -> d_out complex64
    [rows][pvoc_frames(T, rate)][>= n/2+1], torchaudio.functional.phase_vocoder's formula with the phase summed exactly.  chunk_frames
    (0: the library's choice) never changes the result.  d_scratch: a contiguous CUDA tensor of at least jsg_pvoc_scratch_bytes bytes
    (None: one is allocated with torch for this call)."""
    import torch
    a = _pvoc_args(d_X, rate, hop, n, d_out, chunk_frames)
    d_scratch, stream = _scratch_and_stream(d_scratch, stream, d_out, lambda: check(lib().jsg_pvoc_scratch_bytes(C.byref(a))) // 4, torch.int32,
                                            any_dtype=True)
    check(lib().jsg_pvoc_launch(C.byref(a), d_scratch.data_ptr(), d_scratch.numel() * d_scratch.element_size(), stream))


def phase_vocoder(X, rate: float, hop_length: int, n_fft: int | None = None):
    """torchaudio.functional.phase_vocoder on the GPU: X complex CUDA [..., bins, frames] -> complex64 [..., bins, pvoc_frames(frames,
    rate)] (the transposed view of the library's frame-major buffer, as stft returns).  n_fft defaults to 2 * (bins - 1)."""
    import torch
    assert X.is_cuda and X.is_complex(), "phase_vocoder: X must be a complex CUDA tensor"
    bins, frames = int(X.shape[-2]), int(X.shape[-1])
    n = 2 * (bins - 1) if n_fft is None else int(n_fft)
    if bins != n // 2 + 1:
        raise JsgError(capi.JSG_ERR_INVALID, f"phase_vocoder: {bins} bins, expected n_fft//2+1 = {n // 2 + 1}")
    batch = tuple(X.shape[:-2])
    Xf = _frame_major(X)
    out = torch.empty((Xf.shape[0], pvoc_frames(frames, rate), bins), dtype=torch.complex64, device=X.device)
    dev = _device_index(X)
    with torch.cuda.device(dev):
        phase_vocoder_launch(Xf, rate, hop_length, n, out)
    return out.reshape(*batch, out.shape[1], bins).transpose(-1, -2)


def time_stretch(x, rate: float, n_fft: int = 2048, hop_length: int | None = None, win_length: int | None = None, window=None,
                 center: bool = True, length: int | None = None):
    """Time stretch without a change of pitch (rate > 1 shortens): x float32 CUDA [..., L] -> float32 [..., length or round(L / rate)].
    Exactly istft(phase_vocoder(stft(x, ...), rate, hop), ..., length=length or round(L / rate)) with the same n_fft, hop, win_length,
    window and center on both sides.  window = None means a Hann window here, unlike stft and istft: a rectangular window at hop
    n_fft / 4 is a poor default for resynthesis."""
    hop = n_fft // 4 if hop_length is None else int(hop_length)
    w = capi.WIN_HANN if window is None else window
    X = stft(x, n_fft, hop, win_length, w, center)
    Y = phase_vocoder(X, rate, hop, n_fft)
    return istft(Y, n_fft, hop, win_length, w, center, length=length or int(round(x.shape[-1] / rate)))


# --------------------------------------------------------------------------------------------------
# harmonic-percussive separation by median filtering (include/jsg.h, section 2f)
# --------------------------------------------------------------------------------------------------
def _pair(v, kind):
    """(harmonic / time, percussive / frequency) of a scalar or a pair."""
    if isinstance(v, (tuple, list)):
        assert len(v) == 2, "a pair (harmonic/time, percussive/frequency)"
        return kind(v[0]), kind(v[1])
    return kind(v), kind(v)


def _hpss_args(d_in, d_harm, d_perc, d_mask_h, d_mask_p, kernel_size, margin, chunk_frames: int) -> capi.HpssArgs:
    import torch
    X = _rows3(d_in, "d_in")
    assert X.is_cuda and X.dtype in (torch.complex64, torch.float32) and X.stride(2) == 1, "d_in: complex64 or float32 CUDA [rows][frames][bins]"

    def plane(t, what, dtype):
        if t is None:
            return None
        t = _rows3(t, what)
        assert t.is_cuda and t.dtype == dtype and t.stride(2) == 1 and tuple(t.shape) == tuple(X.shape), \
            f"{what}: {dtype} CUDA [rows][frames][bins] of d_in's shape"
        return t

    def pitches(a, b, what):
        if a is not None and b is not None:
            assert (a.stride(1), a.stride(0)) == (b.stride(1), b.stride(0)), f"{what}: the two buffers share one frame pitch and one row pitch"
        t = a if a is not None else b
        return (0, 0) if t is None else (t.stride(1), t.stride(0))

    oh, op = plane(d_harm, "d_harm", X.dtype), plane(d_perc, "d_perc", X.dtype)
    mh, mp = plane(d_mask_h, "d_mask_h", torch.float32), plane(d_mask_p, "d_mask_p", torch.float32)
    ptr = lambda t: None if t is None else t.data_ptr()
    (w_t, w_f), (m_h, m_p) = _pair(kernel_size, int), _pair(margin, float)
    return capi.HpssArgs(X.data_ptr(), int(X.dtype == torch.complex64), X.stride(1), X.stride(0), X.shape[0], X.shape[2], X.shape[1], w_t, w_f, m_h, m_p,
                         ptr(oh), ptr(op), *pitches(oh, op, "d_harm, d_perc"), ptr(mh), ptr(mp), *pitches(mh, mp, "d_mask_h, d_mask_p"),
                         int(chunk_frames))


def hpss_scratch_bytes(d_in, *, d_harm=None, d_perc=None, d_mask_h=None, d_mask_p=None, kernel_size=31, margin=1.0, chunk_frames: int = 0) -> int:
    """jsg_hpss_scratch_bytes: the bytes of scratch hpss_launch needs for these arguments."""
    a = _hpss_args(d_in, d_harm, d_perc, d_mask_h, d_mask_p, kernel_size, margin, chunk_frames)
    return int(check(lib().jsg_hpss_scratch_bytes(C.byref(a))))


def hpss_launch(d_in, *, d_harm=None, d_perc=None, d_mask_h=None, d_mask_p=None, kernel_size=31, margin=1.0, chunk_frames: int = 0,
                d_scratch=None, stream: int | None = None):
    """jsg_hpss_launch: d_in complex64 (frames of a complex STFT) or float32 (power) [rows][frames][bins] -> the harmonic and the
    percussive part (d_harm, d_perc: d_in's dtype and shape) and / or their soft masks (d_mask_h, d_mask_p: float32), median filtering
    as librosa.decompose.hpss with power = 2.  kernel_size and margin: a scalar or a pair (harmonic / time, percussive / frequency).
    chunk_frames (0: the library's choice) never changes the result.  d_scratch: a contiguous CUDA tensor of at least
    hpss_scratch_bytes bytes (None: one is allocated with torch for this call)."""
    import torch
    a = _hpss_args(d_in, d_harm, d_perc, d_mask_h, d_mask_p, kernel_size, margin, chunk_frames)
    d_scratch, stream = _scratch_and_stream(d_scratch, stream, d_in, lambda: check(lib().jsg_hpss_scratch_bytes(C.byref(a))) // 4, torch.float32,
                                            any_dtype=True)
    check(lib().jsg_hpss_launch(C.byref(a), d_scratch.data_ptr(), d_scratch.numel() * d_scratch.element_size(), stream))


def hpss(X, kernel_size=31, margin=1.0, *, masks: bool = False):
    """librosa.decompose.hpss with power = 2 on the GPU: X complex CUDA [..., bins, frames] (what stft returns) or a float32 power
    tensor of that shape -> (harmonic, percussive) in X's shape and kind (the transposed views of the library's frame-major buffers,
    as stft returns), or with masks = True the two float32 soft masks.  kernel_size and margin: a scalar or a pair (harmonic / time,
    percussive / frequency)."""
    import torch
    assert X.is_cuda and (X.is_complex() or X.dtype == torch.float32), "hpss: X must be a complex or a float32 CUDA tensor"
    bins, frames = int(X.shape[-2]), int(X.shape[-1])
    batch = tuple(X.shape[:-2])
    if X.is_complex():
        Xf = _frame_major(X)
    else:
        Xf = X.transpose(-1, -2).reshape(-1, frames, bins)
        Xf = Xf if Xf.stride(2) == 1 else Xf.contiguous()
    a, b = (torch.empty(Xf.shape, dtype=torch.float32 if masks else Xf.dtype, device=X.device) for _ in range(2))
    with torch.cuda.device(_device_index(X)):
        if masks:
            hpss_launch(Xf, d_mask_h=a, d_mask_p=b, kernel_size=kernel_size, margin=margin)
        else:
            hpss_launch(Xf, d_harm=a, d_perc=b, kernel_size=kernel_size, margin=margin)
    return tuple(t.reshape(*batch, frames, bins).transpose(-1, -2) for t in (a, b))


def hpss_audio(x, n_fft: int = 2048, hop_length: int | None = None, win_length: int | None = None, window=None, center: bool = True,
               kernel_size=31, margin=1.0):
    """The harmonic and the percussive part of a signal: x float32 CUDA [..., L] -> (y_harm, y_perc), each float32 [..., L].  Exactly
    istft(hpss(stft(x, ...), kernel_size, margin)[i], ..., length=L) with the same n_fft, hop, win_length, window and center on both
    sides.  window = None means a Hann window, as in time_stretch."""
    hop = n_fft // 4 if hop_length is None else int(hop_length)
    w = capi.WIN_HANN if window is None else window
    X = stft(x, n_fft, hop, win_length, w, center)
    H, P = hpss(X, kernel_size, margin)
    L = int(x.shape[-1])
    return istft(H, n_fft, hop, win_length, w, center, length=L), istft(P, n_fft, hop, win_length, w, center, length=L)


# --------------------------------------------------------------------------------------------------
# band-limited resampling and pitch shift (include/jsg.h, section 2g)
# --------------------------------------------------------------------------------------------------
SINC_TABLES = {"best": (64, 512, 0.9475937167399596, 14.769656459379492), "fast": (16, 512, 0.85, 8.555504641634386)}


def sinc_table(num_zeros: int, per_zero: int, rolloff: float, beta: float) -> np.ndarray:
    """jsg_sinc_table_build: the Kaiser-windowed sinc table, num_zeros * per_zero + 1 float32 entries (no GPU needed)."""
    out = np.zeros(max(0, int(num_zeros)) * max(0, int(per_zero)) + 1, np.float32)
    check(lib().jsg_sinc_table_build(int(num_zeros), int(per_zero), float(rolloff), float(beta), out.ctypes.data))
    return out


class Resampler(_PerDeviceHandles):
    """The interpolation table of jsg_resample_launch: `num_zeros` zero crossings per wing, `per_zero` entries per zero crossing.  Built
    on the host; uploaded to a device once, the first time a launch on that device needs it.  One table serves every ratio.

        Resampler("best" | "fast")                          the Kaiser designs of SINC_TABLES
        Resampler.from_table(table, num_zeros, per_zero)    any table of num_zeros * per_zero + 1 finite floats
    """
    _destroy = "jsg_resampler_destroy"

    def __init__(self, quality: str = "best"):
        if quality not in SINC_TABLES:
            raise JsgError(capi.JSG_ERR_INVALID, f"Resampler: quality must be one of {sorted(SINC_TABLES)}, not {quality!r}")
        Z, P, rolloff, beta = SINC_TABLES[quality]
        self.table, self.num_zeros, self.per_zero, self._handles = sinc_table(Z, P, rolloff, beta), Z, P, {}

    @classmethod
    def from_table(cls, table, num_zeros: int, per_zero: int) -> "Resampler":
        t = np.ascontiguousarray(table, dtype=np.float32).ravel()
        assert t.size == int(num_zeros) * int(per_zero) + 1, "table: num_zeros * per_zero + 1 entries"
        self = cls.__new__(cls)
        self.table, self.num_zeros, self.per_zero, self._handles = t, int(num_zeros), int(per_zero), {}
        return self

    def _create(self, h):
        check(lib().jsg_resampler_create(C.byref(h), self.num_zeros, self.per_zero, self.table.ctypes.data))


def resample_length(in_samples: int, step: float) -> int:
    """jsg_resample_length: the number of outputs i >= 0 with float(i) * step < in_samples."""
    return int(check(lib().jsg_resample_length(int(in_samples), float(step))))


def _resample_args(d_in, step: float, d_out, chunk_outputs: int) -> capi.ResampleArgs:
    import torch
    x = d_in[None] if d_in.dim() == 1 else d_in
    y = d_out[None] if d_out.dim() == 1 else d_out
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1, "d_in: float32 CUDA [rows][samples]"
    assert y.is_cuda and y.dtype == torch.float32 and y.dim() == 2 and y.stride(1) == 1 and y.shape[0] == x.shape[0], "d_out: float32 CUDA [rows][samples]"
    return capi.ResampleArgs(x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], float(step), y.data_ptr(), y.stride(0), y.shape[1], int(chunk_outputs))


def resample_launch(rs: Resampler, d_in, step: float, d_out, *, chunk_outputs: int = 0, stream: int | None = None):
    """jsg_resample_launch: d_in float32 [rows][L] -> d_out float32 [rows][resample_length(L, step)], step = input samples per output
    sample.  chunk_outputs (0: the library's choice) never changes the result."""
    a = _resample_args(d_in, step, d_out, chunk_outputs)
    check(lib().jsg_resample_launch(rs.handle(_device_index(d_in)), C.byref(a), _stream_handle(stream, d_in)))


def resample_kernel_name(rs: Resampler, d_in, step: float, d_out, *, chunk_outputs: int = 0) -> str:
    """The path resample_launch takes for these arguments: "resample_lds", "resample_l2" or "resample_direct"."""
    a = _resample_args(d_in, step, d_out, chunk_outputs)
    return _kernel_name(lib().jsg_resample_kernel_name, rs.handle(_device_index(d_in)), C.byref(a))


def resample_plan(rs: Resampler, d_in, step: float, d_out, *, chunk_outputs: int = 0):
    """jsg_resample_plan: (path, outputs per pass, bytes of LDS per workgroup) of resample_launch for these arguments.  Needs no device."""
    a = _resample_args(d_in, step, d_out, chunk_outputs)
    name, sub, lds = C.create_string_buffer(32), C.c_int32(), C.c_int32()
    check(lib().jsg_resample_plan(rs.num_zeros, rs.per_zero, C.byref(a), name, 32, C.byref(sub), C.byref(lds)))
    return name.value.decode(), sub.value, lds.value


_resamplers: dict = {}


def _default_resampler(quality: str = "best") -> Resampler:
    if quality not in _resamplers:
        _resamplers[quality] = Resampler(quality)
    return _resamplers[quality]


def _resample_rows(rs: Resampler, xr, step: float):
    """xr float32 CUDA [rows][L] (unit sample stride) -> a new [rows][resample_length(L, step)]."""
    import torch
    out = torch.empty((xr.shape[0], resample_length(xr.shape[1], step)), dtype=torch.float32, device=xr.device)
    with torch.cuda.device(_device_index(xr)):
        resample_launch(rs, xr, step, out)
    return out


def resample(x, orig_sr: float, new_sr: float, *, resampler: Resampler | None = None):
    """Band-limited sample-rate conversion on the GPU: x float32 CUDA [..., L] -> float32 [..., resample_length(L, orig_sr / new_sr)]
    (ceil(L new_sr / orig_sr) for integer rates, torchaudio's length).  resampler: default Resampler("best")."""
    import torch
    assert x.is_cuda and x.dtype == torch.float32, "resample: x must be a float32 CUDA tensor"
    rs = _default_resampler() if resampler is None else resampler
    batch = tuple(x.shape[:-1])
    xr = x.reshape(-1, x.shape[-1]).contiguous()
    return _resample_rows(rs, xr, float(orig_sr) / float(new_sr)).reshape(*batch, -1)


def pitch_shift(x, n_steps: float, bins_per_octave: int = 12, n_fft: int = 2048, hop_length: int | None = None, win_length: int | None = None,
                window=None, center: bool = True, *, resampler: Resampler | None = None):
    """librosa.effects.pitch_shift's composition on the GPU: x float32 CUDA [..., L] -> float32 [..., L], the pitch moved by n_steps
    steps of 1 / bins_per_octave octave.  With rate = 2.0 ** (-n_steps / bins_per_octave): time_stretch(x, rate, ...) and then
    resample_launch with step = 1 / rate, cut or zero-padded to L."""
    import torch.nn.functional as Fn
    import torch
    assert x.is_cuda and x.dtype == torch.float32, "pitch_shift: x must be a float32 CUDA tensor"
    rs = _default_resampler() if resampler is None else resampler
    rate = 2.0 ** (-float(n_steps) / float(bins_per_octave))
    L = int(x.shape[-1])
    batch = tuple(x.shape[:-1])
    z = time_stretch(x, rate, n_fft, hop_length, win_length, window, center)
    y = _resample_rows(rs, z.reshape(-1, z.shape[-1]).contiguous(), 1.0 / rate)
    y = y[:, :L] if y.shape[1] >= L else Fn.pad(y, (0, L - y.shape[1]))
    return y.contiguous().reshape(*batch, L)


# --------------------------------------------------------------------------------------------------
# constant-Q and variable-Q spectrograms by direct evaluation (include/jsg.h, section 2h)
# --------------------------------------------------------------------------------------------------
CQT_FMIN_C1 = 32.70319566257483


class CqtBasis(_PerDeviceHandles):
    """The basis of jsg_cqt_launch: n_bins bins, bin k with half length half_lengths[k] and 2 half_lengths[k] + 1 complex64 taps at
    taps[offsets[k] :].  Built on the host by jsg_cqt_basis_build (no GPU needed) or taken from a caller's tables; uploaded to a device
    once, the first time a launch on that device needs it.

        CqtBasis(fs, fmin, n_bins, bins_per_octave=12, filter_scale=1.0, gamma=0.0, scale=True)    the standard basis (gamma > 0: variable-Q)
        CqtBasis.from_tables(half_len, taps)                                                       any basis inside the size limits
    """
    _destroy = "jsg_cqt_destroy"

    def __init__(self, fs: float, fmin: float, n_bins: int, bins_per_octave: int = 12, filter_scale: float = 1.0, gamma: float = 0.0,
                 scale: bool = True):
        spec = capi.CqtSpec(float(fs), float(fmin), int(n_bins), int(bins_per_octave), float(filter_scale), float(gamma), int(bool(scale)))
        total = C.c_int64()
        check(lib().jsg_cqt_basis_build(C.byref(spec), None, None, None, None, 0, C.byref(total)))
        K = int(n_bins)
        half, offset, freq = np.zeros(K, np.int32), np.zeros(K, np.int64), np.zeros(K, np.float32)
        taps = np.zeros(total.value, np.complex64)
        check(lib().jsg_cqt_basis_build(C.byref(spec), half.ctypes.data, offset.ctypes.data, freq.ctypes.data, taps.ctypes.data, total.value,
                                        C.byref(total)))
        self.half_lengths, self.offsets, self.frequencies, self.taps, self._handles = half, offset, freq, taps, {}

    @classmethod
    def from_tables(cls, half_len, taps) -> "CqtBasis":
        h = np.ascontiguousarray(half_len, dtype=np.int32).ravel()
        t = np.ascontiguousarray(taps, dtype=np.complex64).ravel()
        n = 2 * h.astype(np.int64) + 1
        assert h.size >= 1 and (h >= 0).all() and t.size == int(n.sum()), "taps: the sum of 2 half_len + 1 complex entries"
        self = cls.__new__(cls)
        self.half_lengths, self.offsets, self.frequencies, self.taps, self._handles = h, np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64), None, t, {}
        return self

    @property
    def n_bins(self) -> int:
        return int(self.half_lengths.size)

    def _create(self, h):
        check(lib().jsg_cqt_create_tables(C.byref(h), self.n_bins, self.half_lengths.ctypes.data, self.taps.ctypes.data))


def cqt_frames(in_samples: int, hop: int) -> int:
    """jsg_cqt_frames: 1 + in_samples // hop, the frames whose centre t * hop lies in 0..in_samples."""
    return int(check(lib().jsg_cqt_frames(int(in_samples), int(hop))))


def cqt_frequencies(n_bins: int, fmin: float | None = None, bins_per_octave: int = 12) -> np.ndarray:
    """fmin * 2 ** (k / bins_per_octave) for k < n_bins, float64 (fmin None: C1)."""
    f0 = CQT_FMIN_C1 if fmin is None else float(fmin)
    return f0 * 2.0 ** (np.arange(int(n_bins), dtype=np.float64) / float(bins_per_octave))


def _cqt_args(basis: CqtBasis, d_in, hop: int, n_frames: int, d_out, power: bool, chunk_frames: int) -> capi.CqtArgs:
    import torch
    x = d_in[None] if d_in.dim() == 1 else d_in
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1, "d_in: float32 CUDA [rows][samples]"
    o = _rows3(d_out, "d_out")
    want = torch.float32 if power else torch.complex64
    assert o.is_cuda and o.dtype == want and o.stride(2) == 1 and o.shape[0] == x.shape[0] and o.shape[1] >= n_frames and o.shape[2] >= basis.n_bins, \
        "d_out: CUDA [rows][>= n_frames][>= n_bins], complex64 (power: float32)"
    return capi.CqtArgs(x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], int(hop), int(n_frames), o.data_ptr(), o.stride(1), o.stride(0),
                        int(bool(power)), int(chunk_frames))


def cqt_launch(basis: CqtBasis, d_in, hop: int, n_frames: int, d_out, *, power: bool = False, chunk_frames: int = 0, stream: int | None = None):
    """jsg_cqt_launch: d_in float32 [rows][L] -> d_out [rows][n_frames][>= n_bins], complex64 or (power) float32 re*re + im*im; frame t is
    centred on sample t * hop.  chunk_frames (0: the library's choice) never changes the result."""
    a = _cqt_args(basis, d_in, hop, n_frames, d_out, power, chunk_frames)
    check(lib().jsg_cqt_launch(basis.handle(_device_index(d_in)), C.byref(a), _stream_handle(stream, d_in)))


def cqt_kernel_name(basis: CqtBasis, d_in, hop: int, n_frames: int, d_out, *, power: bool = False, chunk_frames: int = 0) -> str:
    """The path cqt_launch takes for these arguments: "cqt_span" or "cqt_passes"."""
    a = _cqt_args(basis, d_in, hop, n_frames, d_out, power, chunk_frames)
    return _kernel_name(lib().jsg_cqt_kernel_name, basis.handle(_device_index(d_in)), C.byref(a))


def cqt_plan(basis: CqtBasis, d_in, hop: int, n_frames: int, d_out, *, power: bool = False, chunk_frames: int = 0):
    """jsg_cqt_plan: (path, [(largest taps of the class, frames per item, taps per pass, bytes of LDS), ...] longest class first) of
    cqt_launch for these arguments.  Needs no device."""
    a = _cqt_args(basis, d_in, hop, n_frames, d_out, power, chunk_frames)
    name, n = C.create_string_buffer(32), C.c_int32()
    cols = [np.zeros(capi.CQT_MAX_CLASSES, np.int32) for _ in range(4)]
    check(lib().jsg_cqt_plan(basis.n_bins, basis.half_lengths.ctypes.data, C.byref(a), name, 32, C.byref(n), *[c.ctypes.data for c in cols]))
    return name.value.decode(), [tuple(int(c[i]) for c in cols) for i in range(n.value)]


_cqt_bases: dict = {}


def _cqt_basis(sr, fmin, n_bins, bins_per_octave, filter_scale, gamma, scale) -> CqtBasis:
    key = (float(sr), CQT_FMIN_C1 if fmin is None else float(fmin), int(n_bins), int(bins_per_octave), float(filter_scale), float(gamma), bool(scale))
    if key not in _cqt_bases:
        _cqt_bases[key] = CqtBasis(*key)
    return _cqt_bases[key]


def _cqt_rows(x, basis: CqtBasis, hop: int, power: bool):
    """x numpy array or CUDA tensor [..., L] -> (frame-major CUDA tensor [rows][frames][bins], batch shape, whether x was numpy)."""
    import torch
    was_numpy = not hasattr(x, "is_cuda")
    if was_numpy:
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    assert x.is_cuda and x.dtype == torch.float32, "x must be a numpy array or a float32 CUDA tensor"
    batch = tuple(x.shape[:-1])
    xr = x.reshape(-1, x.shape[-1]).contiguous()
    frames = cqt_frames(xr.shape[1], hop)
    out = torch.empty((xr.shape[0], frames, basis.n_bins), dtype=torch.float32 if power else torch.complex64, device=x.device)
    with torch.cuda.device(_device_index(x)):
        cqt_launch(basis, xr, hop, frames, out, power=power)
    return out, batch, was_numpy


def vqt(x, sr: float, hop_length: int = 512, fmin: float | None = None, n_bins: int = 84, gamma: float = 0.0, bins_per_octave: int = 12,
        filter_scale: float = 1.0, scale: bool = True):
    """Variable-Q transform on the GPU: x [..., L] (numpy array or float32 CUDA tensor) -> complex64 [..., n_bins, 1 + L // hop_length]
    (the transposed view of the library's frame-major buffer, as stft returns it; a numpy array for numpy input).  gamma = 0 is cqt."""
    basis = _cqt_basis(sr, fmin, n_bins, bins_per_octave, filter_scale, gamma, scale)
    out, batch, was_numpy = _cqt_rows(x, basis, int(hop_length), False)
    out = out.reshape(*batch, out.shape[1], out.shape[2]).transpose(-1, -2)
    return out.cpu().numpy() if was_numpy else out


def cqt(x, sr: float, hop_length: int = 512, fmin: float | None = None, n_bins: int = 84, bins_per_octave: int = 12, filter_scale: float = 1.0,
        scale: bool = True):
    """Constant-Q transform on the GPU (fmin None: C1 = 32.70319566257483 Hz): vqt with gamma = 0."""
    return vqt(x, sr, hop_length, fmin, n_bins, 0.0, bins_per_octave, filter_scale, scale)


def cqt_db(x, sr: float, hop_length: int = 512, fmin: float | None = None, n_bins: int = 84, bins_per_octave: int = 12, filter_scale: float = 1.0,
           scale: bool = True, gamma: float = 0.0, divisor: float = 1.0):
    """10 log10(|C|^2 / divisor + 1e-11) of the constant-Q (gamma > 0: variable-Q) transform: the power plane of jsg_cqt_launch through
    db_from_power.  float32 [..., n_bins, frames], a transposed view: result.transpose(-1, -2) of one row is the contiguous
    [frames][n_bins] plane that colormap takes (height = n_bins)."""
    basis = _cqt_basis(sr, fmin, n_bins, bins_per_octave, filter_scale, gamma, scale)
    power, batch, was_numpy = _cqt_rows(x, basis, int(hop_length), True)
    import torch
    db = torch.empty_like(power)
    db_from_power(power, db, divisor)
    db = db.reshape(*batch, db.shape[1], db.shape[2]).transpose(-1, -2)
    return db.cpu().numpy() if was_numpy else db


# --------------------------------------------------------------------------------------------------
# YIN fundamental-frequency tracking (include/jsg.h, section 2i)
# --------------------------------------------------------------------------------------------------
def yin_frames(in_samples: int, window: int, tau_max: int, hop: int) -> int:
    """jsg_yin_frames: 1 + (in_samples - window - tau_max) // hop, the frames whose span lies inside the row (0 for a shorter row)."""
    return int(check(lib().jsg_yin_frames(int(in_samples), int(window), int(tau_max), int(hop))))


def _yin_args(d_in, window: int, tau_min: int, tau_max: int, hop: int, n_frames: int, threshold: float, sample_rate: float, d_f0, d_aper, d_cmnd,
              chunk_frames: int) -> capi.YinArgs:
    import torch
    x = d_in[None] if d_in.dim() == 1 else d_in
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1, "d_in: float32 CUDA [rows][samples]"
    R = x.shape[0]
    line_pitch = 0
    lines = []
    for o, what in ((d_f0, "d_f0"), (d_aper, "d_aper")):
        if o is not None:
            o = o[None] if o.dim() == 1 else o
            assert o.is_cuda and o.dtype == torch.float32 and o.dim() == 2 and o.stride(1) == 1 and o.shape[0] == R and o.shape[1] >= n_frames, \
                f"{what}: float32 CUDA [rows][>= n_frames]"
            assert all(v is None for v in lines) or R == 1 or o.stride(0) == line_pitch, "d_f0 and d_aper share one row pitch"
            line_pitch = o.stride(0)
        lines.append(o)
    c = None
    if d_cmnd is not None:
        c = _rows3(d_cmnd, "d_cmnd")
        assert c.is_cuda and c.dtype == torch.float32 and c.stride(2) == 1 and c.shape[0] == R and c.shape[1] >= n_frames and c.shape[2] >= tau_max + 1, \
            "d_cmnd: float32 CUDA [rows][>= n_frames][>= tau_max + 1]"
    ptr = lambda t: None if t is None else t.data_ptr()
    return capi.YinArgs(x.data_ptr(), x.stride(0), R, int(window), x.shape[1], int(tau_min), int(tau_max), int(hop), int(n_frames), float(threshold),
                        float(sample_rate), ptr(lines[0]), ptr(lines[1]), line_pitch, ptr(c), 0 if c is None else c.stride(1), 0 if c is None else c.stride(0),
                        int(chunk_frames))


def yin_launch(d_in, window: int, tau_min: int, tau_max: int, hop: int, n_frames: int, threshold: float, sample_rate: float, *, d_f0=None, d_aper=None,
               d_cmnd=None, chunk_frames: int = 0, stream: int | None = None):
    """jsg_yin_launch: d_in float32 [rows][L] -> d_f0, d_aper float32 [rows][n_frames] and d_cmnd float32 [rows][n_frames][>= tau_max + 1]
    (any of the three may be None, not all); frame t covers the samples t * hop .. t * hop + window + tau_max.  chunk_frames (0: the
    library's choice) never changes the result."""
    a = _yin_args(d_in, window, tau_min, tau_max, hop, n_frames, threshold, sample_rate, d_f0, d_aper, d_cmnd, chunk_frames)
    check(lib().jsg_yin_launch(C.byref(a), _stream_handle(stream, d_in)))


def yin_kernel_name(d_in, window: int, tau_min: int, tau_max: int, hop: int, n_frames: int, threshold: float, sample_rate: float, *, d_f0=None,
                    d_aper=None, d_cmnd=None, chunk_frames: int = 0) -> str:
    """The path yin_launch takes for these arguments: "yin_lags1", "yin_lags2", "yin_lags4" or "yin_lags8"."""
    a = _yin_args(d_in, window, tau_min, tau_max, hop, n_frames, threshold, sample_rate, d_f0, d_aper, d_cmnd, chunk_frames)
    return _kernel_name(lib().jsg_yin_kernel_name, C.byref(a))


def yin_plan(d_in, window: int, tau_min: int, tau_max: int, hop: int, n_frames: int, threshold: float, sample_rate: float, *, d_f0=None, d_aper=None,
             d_cmnd=None, chunk_frames: int = 0):
    """jsg_yin_plan: (path, frames per work item, bytes of LDS per workgroup) of yin_launch for these arguments.  Needs no device."""
    a = _yin_args(d_in, window, tau_min, tau_max, hop, n_frames, threshold, sample_rate, d_f0, d_aper, d_cmnd, chunk_frames)
    name, frames, lds = C.create_string_buffer(32), C.c_int32(), C.c_int32()
    check(lib().jsg_yin_plan(C.byref(a), name, 32, C.byref(frames), C.byref(lds)))
    return name.value.decode(), frames.value, lds.value


def _yin_rows(x, sr, fmin, fmax, frame_length, hop_length, threshold, center, want_cmnd: bool):
    """x numpy array or CUDA tensor [..., L] -> (f0, aper or the d' plane [rows][frames][tau_max + 1], batch shape, whether x was numpy)."""
    import math
    import torch
    frame_length = int(frame_length)
    hop = frame_length // 4 if hop_length is None else int(hop_length)
    tau_min = max(1, int(math.floor(float(sr) / float(fmax))))
    tau_max = int(math.ceil(float(sr) / float(fmin)))
    window = frame_length - tau_max
    if window < 1:
        raise JsgError(capi.JSG_ERR_INVALID, f"yin: frame_length {frame_length} leaves no window beside tau_max {tau_max} (= ceil(sr / fmin))")
    was_numpy = not hasattr(x, "is_cuda")
    if was_numpy:
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    assert x.is_cuda and x.dtype == torch.float32, "x must be a numpy array or a float32 CUDA tensor"
    batch = tuple(x.shape[:-1])
    xr = x.reshape(-1, x.shape[-1])
    if center:
        xr = torch.nn.functional.pad(xr, (frame_length // 2, frame_length // 2))
    xr = xr.contiguous()
    T = yin_frames(xr.shape[1], window, tau_max, hop)
    if T < 1:
        raise JsgError(capi.JSG_ERR_INVALID, f"yin: {xr.shape[1]} samples hold no frame of {frame_length}")
    R = xr.shape[0]
    with torch.cuda.device(_device_index(x)):
        if want_cmnd:
            plane = torch.empty((R, T, tau_max + 1), dtype=torch.float32, device=x.device)
            yin_launch(xr, window, tau_min, tau_max, hop, T, threshold, sr, d_cmnd=plane)
            return plane, None, batch, was_numpy
        f0 = torch.empty((R, T), dtype=torch.float32, device=x.device)
        aper = torch.empty((R, T), dtype=torch.float32, device=x.device)
        yin_launch(xr, window, tau_min, tau_max, hop, T, threshold, sr, d_f0=f0, d_aper=aper)
    return f0, aper, batch, was_numpy


def yin(x, sr: float, fmin: float, fmax: float, frame_length: int = 2048, hop_length: int | None = None, threshold: float = 0.1, center: bool = True):
    """YIN fundamental-frequency tracking on the GPU: x [..., L] (numpy array or float32 CUDA tensor) -> (f0, aperiodicity), float32
    [..., frames] each (numpy arrays for numpy input).  tau_min = max(1, floor(sr / fmax)), tau_max = ceil(sr / fmin), the integration
    window is frame_length - tau_max samples (refused below 1), hop_length defaults to frame_length // 4, and center pads
    frame_length // 2 zeros at both ends.  A frame is voiced where aperiodicity < threshold; f0 of an unvoiced frame is the lag of the
    global minimum of d'.  The difference function is summed directly in the time domain (librosa.yin takes it from an FFT
    autocorrelation and differs in further details; agreement with it has not been measured)."""
    f0, aper, batch, was_numpy = _yin_rows(x, sr, fmin, fmax, frame_length, hop_length, threshold, center, False)
    f0, aper = f0.reshape(*batch, -1), aper.reshape(*batch, -1)
    return (f0.cpu().numpy(), aper.cpu().numpy()) if was_numpy else (f0, aper)


def yin_cmnd(x, sr: float, fmin: float, fmax: float, frame_length: int = 2048, hop_length: int | None = None, threshold: float = 0.1, center: bool = True):
    """The cumulative-mean-normalised difference d' of yin's frames, a correlogram: float32 [..., frames, tau_max + 1], lag tau at index
    tau (d'[0] = 1).  One row of it is a contiguous [frames][lags] plane that db_from_power and colormap (height = tau_max + 1) take
    like any spectrogram plane."""
    plane, _, batch, was_numpy = _yin_rows(x, sr, fmin, fmax, frame_length, hop_length, threshold, center, True)
    plane = plane.reshape(*batch, plane.shape[1], plane.shape[2])
    return plane.cpu().numpy() if was_numpy else plane


# --------------------------------------------------------------------------------------------------
# onset strength, autocorrelation tempogram and tempo (include/jsg.h, section 2j)
# --------------------------------------------------------------------------------------------------
def _lines(t, rows: int, least: int, what: str):
    """[rows][>= least] float32 CUDA view with unit stride of a 1- or 2-dimensional tensor."""
    import torch
    t = t[None] if t.dim() == 1 else t
    assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] == rows and t.shape[1] >= least, \
        f"{what}: float32 CUDA [rows][>= {least}]"
    return t


def _plane(t, what: str):
    """[rows][frames][bins] float32 CUDA view with unit bin stride."""
    import torch
    t = _rows3(t, what)
    assert t.is_cuda and t.dtype == torch.float32 and t.stride(2) == 1, f"{what}: float32 CUDA [rows][frames][bins]"
    return t


def onset_strength_launch(d_S, d_out, *, lag: int = 1, max_size: int = 1, stream: int | None = None):
    """jsg_onset_strength_launch: d_S float32 [rows][frames][bands] (or one [frames][bands] plane; views with pitches) -> d_out float32
    [rows][frames]: the mean over the bands of max(0, S[t][b] - ref[t - lag][b]), ref the maximum over max_size neighbouring bands;
    +0 for t < lag."""
    s = _plane(d_S, "d_S")
    R, T, B = s.shape
    o = _lines(d_out, R, T, "d_out")
    a = capi.OnsetArgs(s.data_ptr(), s.stride(1), s.stride(0), R, B, T, int(lag), int(max_size), o.data_ptr(), o.stride(0))
    check(lib().jsg_onset_strength_launch(C.byref(a), _stream_handle(stream, s)))


def tempogram_frames(n_in: int, hop: int = 1) -> int:
    """jsg_tempogram_frames: 1 + (n_in - 1) // hop frames, frame i centred on sample i * hop of the envelope."""
    return int(check(lib().jsg_tempogram_frames(int(n_in), int(hop))))


def _tempogram_args(d_in, d_window, d_out, lags, hop, n_frames, normalise, chunk_frames) -> capi.TempogramArgs:
    import torch
    x = d_in[None] if d_in.dim() == 1 else d_in
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1, "d_in: float32 CUDA [rows][samples]"
    assert d_window.is_cuda and d_window.dtype == torch.float32 and d_window.dim() == 1 and d_window.stride(0) == 1, "d_window: float32 CUDA [win_length]"
    Wn = d_window.shape[0]
    lags = Wn if lags is None else int(lags)
    n_frames = tempogram_frames(x.shape[1], hop) if n_frames is None else int(n_frames)
    o = _plane(d_out, "d_out")
    assert o.shape[0] == x.shape[0] and o.shape[1] >= n_frames and o.shape[2] >= lags, "d_out: float32 CUDA [rows][>= n_frames][>= lags]"
    return capi.TempogramArgs(x.data_ptr(), x.stride(0), x.shape[0], Wn, x.shape[1], int(hop), n_frames, lags, int(bool(normalise)), d_window.data_ptr(),
                              o.data_ptr(), o.stride(1), o.stride(0), int(chunk_frames))


def tempogram_launch(d_in, d_window, d_out, *, lags: int | None = None, hop: int = 1, n_frames: int | None = None, normalise: bool = True,
                     chunk_frames: int = 0, stream: int | None = None):
    """jsg_tempogram_launch: d_in float32 [rows][T] (an onset envelope), d_window float32 [win_length] -> d_out float32
    [rows][n_frames][>= lags]: the autocorrelation of the windowed envelope around sample i * hop at the lags 0..lags-1 (default: all
    win_length of them), divided by its lag 0 where normalise.  chunk_frames (0: the library's choice) never changes the result."""
    a = _tempogram_args(d_in, d_window, d_out, lags, hop, n_frames, normalise, chunk_frames)
    check(lib().jsg_tempogram_launch(C.byref(a), _stream_handle(stream, d_in)))


def tempogram_kernel_name(d_in, d_window, d_out, *, lags: int | None = None, hop: int = 1, n_frames: int | None = None, normalise: bool = True,
                          chunk_frames: int = 0) -> str:
    """The path tempogram_launch takes for these arguments: "tempogram_lags1", "tempogram_lags2", "tempogram_lags4" or "tempogram_lags8"."""
    a = _tempogram_args(d_in, d_window, d_out, lags, hop, n_frames, normalise, chunk_frames)
    return _kernel_name(lib().jsg_tempogram_kernel_name, C.byref(a))


def tempogram_plan(d_in, d_window, d_out, *, lags: int | None = None, hop: int = 1, n_frames: int | None = None, normalise: bool = True,
                   chunk_frames: int = 0):
    """jsg_tempogram_plan: (path, frames per work item, bytes of LDS per workgroup) of tempogram_launch for these arguments.  Needs no
    device."""
    a = _tempogram_args(d_in, d_window, d_out, lags, hop, n_frames, normalise, chunk_frames)
    name, frames, lds = C.create_string_buffer(32), C.c_int32(), C.c_int32()
    check(lib().jsg_tempogram_plan(C.byref(a), name, 32, C.byref(frames), C.byref(lds)))
    return name.value.decode(), frames.value, lds.value


def tempo_prior(lags: int, frame_rate: float, start_bpm: float = 120.0, std_bpm: float = 1.0, max_bpm: float = 320.0) -> np.ndarray:
    """jsg_tempo_prior_build: the log-normal tempo prior of librosa.feature.tempo over the lags 0..lags-1 of an envelope of frame_rate
    frames per second (0 at lag 0 and where 60 * frame_rate / lag exceeds max_bpm; max_bpm <= 0: no limit), float32."""
    out = np.zeros(int(lags), dtype=np.float32)
    check(lib().jsg_tempo_prior_build(int(lags), float(frame_rate), float(start_bpm), float(std_bpm), float(max_bpm), out.ctypes.data))
    return out


def tempo_launch(d_tg, d_prior, frame_rate: float, *, d_bpm=None, d_lag=None, d_profile=None, lags: int | None = None, n_frames: int | None = None,
                 stream: int | None = None):
    """jsg_tempo_launch: d_tg float32 [rows][frames][>= lags] (a tempogram), d_prior float32 [lags] -> d_bpm float32 [rows], d_lag int32
    [rows], d_profile float32 [rows][>= lags] (the mean over the frames); any of the three may be None, not all."""
    import torch
    tg = _plane(d_tg, "d_tg")
    R = tg.shape[0]
    lags = d_prior.shape[0] if lags is None else int(lags)
    n_frames = tg.shape[1] if n_frames is None else int(n_frames)
    assert d_prior.is_cuda and d_prior.dtype == torch.float32 and d_prior.dim() == 1 and d_prior.stride(0) == 1 and d_prior.shape[0] >= lags, "d_prior: float32 CUDA [lags]"
    assert tg.shape[1] >= n_frames and tg.shape[2] >= lags, "d_tg: float32 CUDA [rows][>= n_frames][>= lags]"
    for o, dtype, what in ((d_bpm, torch.float32, "d_bpm"), (d_lag, torch.int32, "d_lag")):
        assert o is None or (o.is_cuda and o.dtype == dtype and o.dim() == 1 and o.stride(0) == 1 and o.shape[0] >= R), f"{what}: CUDA [rows]"
    p = None if d_profile is None else _lines(d_profile, R, lags, "d_profile")
    ptr = lambda t: None if t is None else t.data_ptr()
    a = capi.TempoArgs(tg.data_ptr(), tg.stride(1), tg.stride(0), R, lags, n_frames, float(frame_rate), d_prior.data_ptr(), ptr(d_bpm), ptr(d_lag), ptr(p),
                       0 if p is None else p.stride(0))
    check(lib().jsg_tempo_launch(C.byref(a), _stream_handle(stream, tg)))


def _to_cuda(x):
    """(float32 CUDA tensor, whether x was a numpy array)."""
    import torch
    was_numpy = not hasattr(x, "is_cuda")
    if was_numpy:
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    assert x.is_cuda and x.dtype == torch.float32, "expected a numpy array or a float32 CUDA tensor"
    return x, was_numpy


def onset_strength(S, lag: int = 1, max_size: int = 1):
    """Onset strength (spectral flux) of S [..., frames, bands] (numpy array or float32 CUDA tensor; what mel_spectrogram_db returns) ->
    float32 [..., frames], the same kind.  Differs from librosa.onset.onset_strength on purpose: no centring shift of the envelope, the
    maximum filter is clipped at the band edges (not reflected), and the bands lie along the last axis."""
    import torch
    s, was_numpy = _to_cuda(S)
    batch = tuple(s.shape[:-2])
    sr = s.reshape(-1, s.shape[-2], s.shape[-1]).contiguous()
    out = torch.empty((sr.shape[0], sr.shape[1]), dtype=torch.float32, device=s.device)
    with torch.cuda.device(_device_index(s)):
        onset_strength_launch(sr, out, lag=lag, max_size=max_size)
    out = out.reshape(*batch, -1)
    return out.cpu().numpy() if was_numpy else out


def _hann_window(win_length: int, device):
    import torch
    return torch.from_numpy(window(capi.WIN_HANN, int(win_length))).to(device)


def tempogram(onset_envelope, win_length: int = 384, hop_length: int = 1, lags: int | None = None, window_table=None, normalise: bool = True):
    """Autocorrelation tempogram of an onset envelope [..., T] (numpy array or float32 CUDA tensor) -> float32 [..., frames, lags], lag tau
    at index tau, frames = 1 + (T - 1) // hop_length, the same kind.  window_table: win_length floats (default: the library's periodic
    Hann).  One row of the result is a contiguous [frames][lags] plane that db_from_power and colormap (height = lags) take.  Differs from
    librosa.feature.tempogram on purpose: zeros (not a linear ramp) outside the envelope, and a direct (not FFT) autocorrelation."""
    import torch
    x, was_numpy = _to_cuda(onset_envelope)
    batch = tuple(x.shape[:-1])
    xr = x.reshape(-1, x.shape[-1]).contiguous()
    w = _hann_window(win_length, x.device) if window_table is None else torch.as_tensor(np.ascontiguousarray(window_table, dtype=np.float32)).to(x.device)
    lags = w.shape[0] if lags is None else int(lags)
    n_frames = tempogram_frames(xr.shape[1], hop_length)
    out = torch.empty((xr.shape[0], n_frames, lags), dtype=torch.float32, device=x.device)
    with torch.cuda.device(_device_index(x)):
        tempogram_launch(xr, w, out, lags=lags, hop=hop_length, normalise=normalise)
    out = out.reshape(*batch, n_frames, lags)
    return out.cpu().numpy() if was_numpy else out


def tempo(tg, frame_rate: float, start_bpm: float = 120.0, std_bpm: float = 1.0, max_bpm: float = 320.0):
    """Tempo of a tempogram [..., frames, lags] (numpy array or float32 CUDA tensor) over all its frames -> (bpm float32 [...], lag int32
    [...]), the same kind: the lag >= 1 that maximises (1 + 1e6 * mean autocorrelation) * prior, the rule of librosa.feature.tempo with
    aggregate = mean.  frame_rate: frames of the onset envelope per second (sr / hop).  bpm is NaN and lag -1 where the mean holds a NaN."""
    import torch
    t, was_numpy = _to_cuda(tg)
    batch = tuple(t.shape[:-2])
    tr = t.reshape(-1, t.shape[-2], t.shape[-1])
    tr = tr if tr.stride(2) == 1 else tr.contiguous()
    prior = torch.from_numpy(tempo_prior(tr.shape[2], frame_rate, start_bpm, std_bpm, max_bpm)).to(t.device)
    bpm = torch.empty((tr.shape[0],), dtype=torch.float32, device=t.device)
    lag = torch.empty((tr.shape[0],), dtype=torch.int32, device=t.device)
    with torch.cuda.device(_device_index(t)):
        tempo_launch(tr, prior, frame_rate, d_bpm=bpm, d_lag=lag)
    bpm, lag = bpm.reshape(batch), lag.reshape(batch)
    return (bpm.cpu().numpy(), lag.cpu().numpy()) if was_numpy else (bpm, lag)


def estimate_tempo(x, sr: float, n_fft: int = 2048, hop: int = 512, n_mels: int = 128, win_length: int = 384, start_bpm: float = 120.0,
                   std_bpm: float = 1.0, max_bpm: float = 320.0):
    """Tempo of audio x [samples] (numpy array or float32 CUDA tensor): mel_spectrogram_db -> onset_strength -> tempogram (periodic Hann of
    win_length envelope frames, every frame) -> tempo, all on the GPU with nothing returned to the host in between.  Returns (bpm, lag):
    floats and ints of the host for numpy input, 0-dimensional CUDA tensors otherwise."""
    import torch
    xt, was_numpy = _to_cuda(x)
    assert xt.dim() == 1, "estimate_tempo: x is one channel [samples]"
    with torch.cuda.device(_device_index(xt)):
        S = mel_spectrogram_db(xt, sr, n_fft, hop, n_mels)
        env = onset_strength(S)
        tg = tempogram(env, win_length=win_length)
        bpm, lag = tempo(tg, float(sr) / float(hop), start_bpm, std_bpm, max_bpm)
    return (float(bpm.cpu()), int(lag.cpu())) if was_numpy else (bpm, lag)


# --------------------------------------------------------------------------------------------------
# beat tracking by dynamic programming (include/jsgx.h, section 1: the companion library libjsgx.so)
# --------------------------------------------------------------------------------------------------
_beat_cache: dict = {}


def beat_log_table(n: int = capix.BEAT_LOG_TABLE) -> np.ndarray:
    """jsgx_log_table_build: float32 [n], 0 at index 0 and ln(k) at index k (in double, rounded once).  beat_launch takes the table of
    2 * BEAT_MAX_PERIOD + 1 entries on the device."""
    out = np.zeros(int(n), dtype=np.float32)
    capix.check(capix.lib().jsgx_log_table_build(int(n), out.ctypes.data))
    return out


def _device_table(key, device, make):
    """A host table uploaded once per device and key (so that a steady-state call copies nothing from the host)."""
    import torch
    key = (str(device),) + key
    if key not in _beat_cache:
        _beat_cache[key] = torch.from_numpy(np.ascontiguousarray(make(), dtype=np.float32)).to(device)
    return _beat_cache[key]


def _beat_args(d_in, d_log_table, d_beats, d_n_beats, d_period, period, tightness, smooth, normalise, max_beats, d_local_score, d_cum_score) -> capix.BeatArgs:
    import torch
    x = d_in[None] if d_in.dim() == 1 else d_in
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1, "d_in: float32 CUDA [rows][frames]"
    R, T = x.shape
    assert d_log_table.is_cuda and d_log_table.dtype == torch.float32 and d_log_table.dim() == 1 and d_log_table.stride(0) == 1 and \
        d_log_table.shape[0] >= capix.BEAT_LOG_TABLE, f"d_log_table: float32 CUDA [{capix.BEAT_LOG_TABLE}]"
    b = d_beats[None] if d_beats.dim() == 1 else d_beats
    assert b.is_cuda and b.dtype == torch.int32 and b.dim() == 2 and b.stride(1) == 1 and b.shape[0] == R, "d_beats: int32 CUDA [rows][max_beats]"
    max_beats = b.shape[1] if max_beats is None else int(max_beats)
    assert b.shape[1] >= max_beats, "d_beats: int32 CUDA [rows][>= max_beats]"
    for o, what in ((d_n_beats, "d_n_beats"), (d_period, "d_period")):
        assert o is None or (o.is_cuda and o.dtype == torch.int32 and o.dim() == 1 and o.stride(0) == 1 and o.shape[0] >= R), f"{what}: int32 CUDA [rows]"
    assert d_n_beats is not None and (d_period is None) != (period is None), "d_n_beats, and exactly one of d_period and period"
    ls = None if d_local_score is None else _lines(d_local_score, R, T, "d_local_score")
    cs = None if d_cum_score is None else _lines(d_cum_score, R, T, "d_cum_score")
    ptr = lambda t: None if t is None else t.data_ptr()
    return capix.BeatArgs(x.data_ptr(), x.stride(0), R, T, ptr(d_period), 0 if period is None else int(period), int(bool(smooth)), d_log_table.data_ptr(),
                          float(tightness), int(bool(normalise)), b.data_ptr(), b.stride(0), max_beats, 0, d_n_beats.data_ptr(),
                          ptr(ls), 0 if ls is None else ls.stride(0), ptr(cs), 0 if cs is None else cs.stride(0))


def beat_scratch_bytes(d_in, d_log_table, d_beats, d_n_beats, *, d_period=None, period: int | None = None, tightness: float = 100.0, smooth: bool = True,
                       normalise: bool = True, max_beats: int | None = None, d_local_score=None, d_cum_score=None) -> int:
    """jsgx_beat_scratch_bytes: the bytes of scratch beat_launch needs for these arguments."""
    a = _beat_args(d_in, d_log_table, d_beats, d_n_beats, d_period, period, tightness, smooth, normalise, max_beats, d_local_score, d_cum_score)
    return int(capix.check(capix.lib().jsgx_beat_scratch_bytes(C.byref(a))))


def beat_launch(d_in, d_log_table, d_beats, d_n_beats, *, d_period=None, period: int | None = None, tightness: float = 100.0, smooth: bool = True,
                normalise: bool = True, max_beats: int | None = None, d_local_score=None, d_cum_score=None, d_scratch=None, stream: int | None = None):
    """jsgx_beat_launch: d_in float32 [rows][frames] (an onset envelope), d_log_table float32 [2049] (beat_log_table on the device), the
    period of every row in d_period (int32 [rows], what tempo_launch writes into d_lag) or one `period` for all -> d_beats int32
    [rows][max_beats] (the beat frames, ascending) and d_n_beats int32 [rows] (their number; -1 for a row whose period is outside
    1..1024 or whose envelope holds a NaN).  d_local_score, d_cum_score: float32 [rows][>= frames] or None.  d_scratch: a contiguous
    CUDA tensor of at least beat_scratch_bytes bytes (None: one is allocated with torch for this call)."""
    import torch
    a = _beat_args(d_in, d_log_table, d_beats, d_n_beats, d_period, period, tightness, smooth, normalise, max_beats, d_local_score, d_cum_score)
    d_scratch, stream = _scratch_and_stream(d_scratch, stream, d_in, lambda: capix.check(capix.lib().jsgx_beat_scratch_bytes(C.byref(a))) // 4, torch.int32,
                                            any_dtype=True)
    capix.check(capix.lib().jsgx_beat_launch(C.byref(a), d_scratch.data_ptr(), d_scratch.numel() * d_scratch.element_size(), stream))


def beat_plan(period: int, n_frames: int = 1024, rows: int = 1):
    """jsgx_beat_plan: (form, lanes per workgroup, bytes of LDS per workgroup) of the kernel for a row of this period: "beat_frames" (one
    lane per frame) from period 511 on, "beat_split" (the lanes of a frame split the look-back range) below.  Needs no device."""
    a = capix.BeatArgs(in_=1 << 44, in_pitch=int(n_frames), rows=int(rows), n_frames=int(n_frames), period_all=int(period) if 1 <= period <= capix.BEAT_MAX_PERIOD else 1,
                       log_table=2 << 44, tightness=100.0, beats=3 << 44, beats_pitch=int(n_frames), max_beats=int(n_frames), n_beats=4 << 44)   # never dereferenced
    name, threads, lds = C.create_string_buffer(32), C.c_int32(), C.c_int32()
    capix.check(capix.lib().jsgx_beat_plan(C.byref(a), int(period), name, 32, C.byref(threads), C.byref(lds)))
    return name.value.decode(), threads.value, lds.value


def beat_track(onset_envelope, period=None, bpm=None, frame_rate=None, tightness=100.0, smooth=True, normalise=True, max_beats=None):
    """Beat frames of an onset envelope [..., T] (numpy array or float32 CUDA tensor) by dynamic programming (Ellis 2007, the core of
    librosa.beat.beat_track) -> (beats int32 [..., max_beats], n_beats int32 [...]) as CUDA tensors: beats[..., :n_beats] ascending.
    period: an int (frames per beat, for every row), an int32 CUDA tensor with one period per row (what tempo returns as lag), or None:
    round(60 * frame_rate / bpm).  max_beats None: as many as a row can hold.  Differs from librosa on purpose: an integer period, Ellis'
    end rule, no trimming of weak beats (include/jsgx.h)."""
    import torch
    x, _ = _to_cuda(onset_envelope)
    batch = tuple(x.shape[:-1])
    xr = x.reshape(-1, x.shape[-1]).contiguous()
    R, T = xr.shape
    d_period = None
    if period is None:
        assert bpm is not None and frame_rate is not None, "beat_track: a period, or bpm and frame_rate"
        period = int(round(60.0 * float(frame_rate) / float(bpm)))
    elif hasattr(period, "is_cuda"):
        d_period, period = period.reshape(-1).to(torch.int32).contiguous(), None
        assert d_period.is_cuda and d_period.shape[0] == R, "beat_track: one period per row"
    if max_beats is None:
        max_beats = T if period is None else 1 + (T - 1) // max(1, (int(period) + 1) // 2)
    beats = torch.zeros((R, int(max_beats)), dtype=torch.int32, device=x.device)
    n_beats = torch.empty((R,), dtype=torch.int32, device=x.device)
    with torch.cuda.device(_device_index(x)):
        beat_launch(xr, _device_table(("log",), x.device, beat_log_table), beats, n_beats, d_period=d_period, period=period, tightness=tightness,
                    smooth=smooth, normalise=normalise)
    return beats.reshape(*batch, int(max_beats)), n_beats.reshape(batch)


def beat_track_audio(x, sr, n_fft=2048, hop=512, n_mels=128, win_length=384, start_bpm=120.0, std_bpm=1.0, max_bpm=320.0, tightness=100.0, smooth=True,
                     normalise=True, max_beats=None):
    """Tempo and beats of audio x [samples] (numpy array or float32 CUDA tensor): mel_spectrogram_db -> onset_strength_launch ->
    tempogram_launch -> tempo_launch (its lag stays on the device) -> beat_launch, enqueued one after the other with no host
    synchronisation and, from the second call of a geometry on, no host copy.  Returns (bpm float32 [], beats int32 [max_beats], n_beats
    int32 []) as CUDA tensors; the beat frames are frames of the mel spectrogram (frame t starts at sample t * hop)."""
    import torch
    xt, _ = _to_cuda(x)
    assert xt.dim() == 1, "beat_track_audio: x is one channel [samples]"
    dev = xt.device
    rate = float(sr) / float(hop)
    with torch.cuda.device(_device_index(xt)):
        S = mel_spectrogram_db(xt, sr, n_fft, hop, n_mels)
        T = S.shape[0]
        env = torch.empty((1, T), dtype=torch.float32, device=dev)
        onset_strength_launch(S, env)
        w = _device_table(("hann", int(win_length)), dev, lambda: window(capi.WIN_HANN, int(win_length)))
        tg = torch.empty((1, T, int(win_length)), dtype=torch.float32, device=dev)
        tempogram_launch(env, w, tg)
        prior = _device_table(("prior", int(win_length), rate, float(start_bpm), float(std_bpm), float(max_bpm)), dev,
                              lambda: tempo_prior(int(win_length), rate, start_bpm, std_bpm, max_bpm))
        bpm = torch.empty((1,), dtype=torch.float32, device=dev)
        lag = torch.empty((1,), dtype=torch.int32, device=dev)
        tempo_launch(tg, prior, rate, d_bpm=bpm, d_lag=lag)
        max_beats = T if max_beats is None else int(max_beats)
        beats = torch.zeros((1, max_beats), dtype=torch.int32, device=dev)
        n_beats = torch.empty((1,), dtype=torch.int32, device=dev)
        beat_launch(env, _device_table(("log",), dev, beat_log_table), beats, n_beats, d_period=lag, tightness=tightness, smooth=smooth, normalise=normalise)
    return bpm[0], beats[0], n_beats[0]


# --------------------------------------------------------------------------------------------------
# pairwise cost and dynamic time warping (include/jsgx.h, sections 2 and 3: libjsgx.so)
# --------------------------------------------------------------------------------------------------
_METRICS = {"sqeuclidean": capix.METRIC_SQEUCLIDEAN, "euclidean": capix.METRIC_EUCLIDEAN, "cosine": capix.METRIC_COSINE}


def _planes(t, what: str, dtype=None):
    """A float32 CUDA tensor [rows][cols] or [pairs][rows][cols] with unit stride along cols, as [pairs][rows][cols]."""
    import torch
    t = t[None] if t.dim() == 2 else t
    assert t.is_cuda and t.dtype == (dtype or torch.float32) and t.dim() == 3 and (t.stride(2) == 1 or t.shape[2] == 1), \
        f"{what}: CUDA [rows][cols] or [pairs][rows][cols], unit stride along cols"
    return t


def _pair_pitch(t) -> int:
    return 0 if t.shape[0] == 1 else t.stride(0)      # one plane for every pair: a pair pitch of 0


def _plan_xy(n, m, n_features):
    """The x and y of a ..._plan call's argument block, dense and per pair; never dereferenced."""
    return 1 << 44, int(n_features), int(n) * int(n_features), 2 << 44, int(n_features), int(m) * int(n_features)


def _cdist_args(d_x, d_y, d_cost, metric) -> capix.CdistArgs:
    c = _planes(d_cost, "d_cost")
    P, N, M = c.shape
    x, y = _planes(d_x, "d_x"), _planes(d_y, "d_y")
    K = x.shape[2]
    assert x.shape[1] == N and y.shape[1] == M and y.shape[2] == K and x.shape[0] in (1, P) and y.shape[0] in (1, P), \
        "d_x [pairs or 1][n][features], d_y [pairs or 1][m][features], d_cost [pairs][n][m]"
    return capix.CdistArgs(x.data_ptr(), x.stride(1), _pair_pitch(x), y.data_ptr(), y.stride(1), _pair_pitch(y), P, K, N, M, _named(_METRICS, metric, "metric"), 0,
                           c.data_ptr(), c.stride(1), c.stride(0))


def cdist_launch(d_x, d_y, d_cost, *, metric: str = "euclidean", stream: int | None = None):
    """jsgx_cdist_launch: d_x float32 [n][features] or [pairs][n][features], d_y likewise with m frames (frame-major, what the feature
    kernels write; a 2-D tensor, a leading 1 or an expanded tensor is one sequence shared by every pair) -> d_cost float32 [n][m] or
    [pairs][n][m].  metric: "sqeuclidean", "euclidean" or "cosine" (1 for a zero vector).  Enqueue only."""
    a = _cdist_args(d_x, d_y, d_cost, metric)
    capix.check(capix.lib().jsgx_cdist_launch(C.byref(a), _stream_handle(stream, d_cost)))


def cdist_plan(n: int, m: int, n_features: int, pairs: int = 1, metric: str = "euclidean"):
    """jsgx_cdist_plan: (kernel name, lanes per workgroup, bytes of LDS per workgroup) for this shape.  Needs no device."""
    a = capix.CdistArgs(*_plan_xy(n, m, n_features), int(pairs), int(n_features), int(n), int(m), _named(_METRICS, metric, "metric"), 0,
                        3 << 44, int(m), int(n) * int(m))      # never dereferenced
    name, threads, lds = C.create_string_buffer(32), C.c_int32(), C.c_int32()
    capix.check(capix.lib().jsgx_cdist_plan(C.byref(a), name, 32, C.byref(threads), C.byref(lds)))
    return name.value.decode(), threads.value, lds.value


def cdist(X, Y, metric: str = "euclidean"):
    """The pairwise cost of two feature sequences X [N, K] and Y [M, K] (numpy arrays or float32 CUDA tensors, frame-major; a leading
    axis of P pairs on either or both) -> a CUDA tensor [N, M] or [P, N, M]: scipy.spatial.distance.cdist for "sqeuclidean", "euclidean"
    and "cosine", with every operation as include/jsgx.h states it."""
    import torch
    x, _ = _to_cuda(X)
    y, _ = _to_cuda(Y)
    assert x.dim() in (2, 3) and y.dim() in (2, 3), "cdist: X [N, K] or [P, N, K], Y [M, K] or [P, M, K]"
    x, y = x.contiguous(), y.contiguous()
    P = max(x.shape[0] if x.dim() == 3 else 1, y.shape[0] if y.dim() == 3 else 1)
    shape = (x.shape[-2], y.shape[-2])
    cost = torch.empty(((P,) if x.dim() == 3 or y.dim() == 3 else ()) + shape, dtype=torch.float32, device=x.device)
    with torch.cuda.device(_device_index(x)):
        cdist_launch(x, y, cost, metric=metric)
    return cost


def _path_args(d_path_i, d_path_j, P):
    """(path_pitch, max_path) of the path outputs of a dtw or rqa launch; 0, 0 unless both are given (the library refuses one alone)."""
    import torch
    if d_path_i is None or d_path_j is None:
        return 0, 0
    pi, pj = (t[None] if t.dim() == 1 else t for t in (d_path_i, d_path_j))
    for t in (pi, pj):
        assert t.is_cuda and t.dtype == torch.int32 and t.dim() == 2 and t.shape[0] == P and (t.stride(1) == 1 or t.shape[1] == 1), "d_path_i, d_path_j: int32 CUDA [pairs][max_path]"
    assert pi.shape == pj.shape and pi.stride(0) == pj.stride(0), "d_path_i and d_path_j: one shape and pitch"
    return pi.stride(0), pi.shape[1]


def _tiles_plan(fn, args):
    """The tail of dtw_plan and rqa_plan: the call and its six results."""
    name, out = C.create_string_buffer(32), [C.c_int32() for _ in range(5)]
    capix.check(fn(C.byref(args), name, 32, *[C.byref(o) for o in out]))
    return (name.value.decode(),) + tuple(o.value for o in out)


def _cut_paths(path, lengths):
    """path int32 [2][pairs][max_path] and the pairs' lengths -> the list of [L, 2] tensors."""
    import torch
    return [torch.stack((path[0, p, :L], path[1, p, :L]), dim=1) for p, L in enumerate(lengths)]


def _dtw_args(d_cost, d_acc, weights_mul, weights_add, subseq, band, d_path_i, d_path_j, d_path_len, d_total) -> capix.DtwArgs:
    import torch
    c, d = _planes(d_cost, "d_cost"), _planes(d_acc, "d_acc")
    P, N, M = c.shape
    assert tuple(d.shape) == (P, N, M), "d_acc: the shape of d_cost"
    ptr = lambda t: None if t is None else t.data_ptr()
    path_pitch, max_path = _path_args(d_path_i, d_path_j, P)
    for t, dtype, what in ((d_path_len, torch.int32, "d_path_len: int32"), (d_total, torch.float32, "d_total: float32")):
        assert t is None or (t.is_cuda and t.dtype == dtype and t.dim() == 1 and t.shape[0] >= P and t.is_contiguous()), f"{what} CUDA [pairs]"
    wm = (1.0, 1.0, 1.0) if weights_mul is None else tuple(float(w) for w in weights_mul)
    wa = (0.0, 0.0, 0.0) if weights_add is None else tuple(float(w) for w in weights_add)
    assert len(wm) == 3 and len(wa) == 3, "weights_mul, weights_add: three values, for the steps (1, 1), (0, 1), (1, 0)"
    return capix.DtwArgs(c.data_ptr(), c.stride(1), c.stride(0), P, N, M, int(bool(subseq)), int(band), 0, (C.c_float * 3)(*wm), (C.c_float * 3)(*wa),
                         d.data_ptr(), d.stride(1), d.stride(0), ptr(d_path_i), ptr(d_path_j), path_pitch, max_path, ptr(d_path_len), ptr(d_total))


def dtw_scratch_bytes(d_cost, d_acc, *, weights_mul=None, weights_add=None, subseq: bool = False, band: int = 0, d_path_i=None, d_path_j=None,
                      d_path_len=None, d_total=None) -> int:
    """jsgx_dtw_scratch_bytes: the bytes of scratch dtw_launch needs for these arguments (0 without paths)."""
    a = _dtw_args(d_cost, d_acc, weights_mul, weights_add, subseq, band, d_path_i, d_path_j, d_path_len, d_total)
    return int(capix.check(capix.lib().jsgx_dtw_scratch_bytes(C.byref(a))))


def dtw_launch(d_cost, d_acc, *, weights_mul=None, weights_add=None, subseq: bool = False, band: int = 0, d_path_i=None, d_path_j=None,
               d_path_len=None, d_total=None, d_scratch=None, stream: int | None = None):
    """jsgx_dtw_launch: d_cost float32 [n][m] or [pairs][n][m] -> d_acc (the accumulated cost D, the same shape), and where given
    d_path_i, d_path_j int32 [pairs][max_path >= n + m - 1] (the warping path, ascending), d_path_len int32 [pairs] (its length; -1:
    no path) and d_total float32 [pairs] (D at the end cell).  The steps are (1, 1), (0, 1), (1, 0) with librosa's weights_mul and
    weights_add; band: 0 or the half-width R of include/jsgx.h.  Enqueue only: one kernel per tile anti-diagonal, then the backtrace."""
    import torch
    a = _dtw_args(d_cost, d_acc, weights_mul, weights_add, subseq, band, d_path_i, d_path_j, d_path_len, d_total)
    d_scratch, stream = _scratch_and_stream(d_scratch, stream, d_cost, lambda: max(1, capix.check(capix.lib().jsgx_dtw_scratch_bytes(C.byref(a))) // 4), torch.int32,
                                            any_dtype=True)
    capix.check(capix.lib().jsgx_dtw_launch(C.byref(a), d_scratch.data_ptr(), d_scratch.numel() * d_scratch.element_size(), stream))


def dtw_plan(n: int, m: int, pairs: int = 1, backtrack: bool = True):
    """jsgx_dtw_plan: (kernel name, tile rows, tile columns, kernel launches, lanes per workgroup, bytes of LDS per workgroup) for this
    shape: one launch per tile anti-diagonal and one for the backtrace.  Needs no device."""
    a = capix.DtwArgs(cost=1 << 44, cost_pitch=int(m), cost_pair_pitch=int(n) * int(m), pairs=int(pairs), n=int(n), m=int(m), weights_mul=(C.c_float * 3)(1, 1, 1),
                      acc=2 << 44, acc_pitch=int(m), acc_pair_pitch=int(n) * int(m), path_len=(3 << 44) if backtrack else None)      # never dereferenced
    return _tiles_plan(capix.lib().jsgx_dtw_plan, a)


def dtw(X=None, Y=None, *, C=None, metric="euclidean", weights_mul=None, weights_add=None, subseq=False, band=0, backtrack=True):
    """librosa.sequence.dtw on the GPU for the default steps: from two feature sequences X [N, K] and Y [M, K] (frame-major; numpy arrays
    or float32 CUDA tensors) or a cost plane C [N, M] -> (D, wp): the accumulated cost [N, M] and the warping path wp int32 [L, 2] as CUDA
    tensors, ascending from the start (librosa returns it descending).  backtrack False: D alone.  A leading axis of P pairs is allowed:
    D is [P, N, M] and wp a list.  Reading the path lengths is the one host synchronisation; JsgError where a pair has no path (a band too
    narrow, a NaN).  band: 0 or the half-width R of include/jsgx.h; differences from librosa are listed there."""
    import torch
    assert (C is None) != (X is None and Y is None) and (X is None) == (Y is None), "dtw: X and Y, or C"
    if C is None:
        cost = cdist(X, Y, metric)
    else:
        cost, _ = _to_cuda(C)
        assert cost.dim() in (2, 3), "dtw: C [N, M] or [P, N, M]"
        cost = cost.contiguous()
    batched = cost.dim() == 3
    c3 = cost if batched else cost[None]
    P, N, M = c3.shape
    D = torch.empty_like(c3)
    with torch.cuda.device(_device_index(cost)):
        if not backtrack:
            dtw_launch(c3, D, weights_mul=weights_mul, weights_add=weights_add, subseq=subseq, band=band)
            return D if batched else D[0]
        path = torch.empty((2, P, N + M - 1), dtype=torch.int32, device=cost.device)
        length = torch.empty((P,), dtype=torch.int32, device=cost.device)
        dtw_launch(c3, D, weights_mul=weights_mul, weights_add=weights_add, subseq=subseq, band=band, d_path_i=path[0], d_path_j=path[1], d_path_len=length)
    lengths = length.tolist()           # the one host synchronisation
    if min(lengths) < 0:
        raise JsgError(capix.JSGX_ERR_INVALID, f"dtw: no warping path for pair {lengths.index(min(lengths))} (a band too narrow for the shape, or a NaN)")
    wp = _cut_paths(path, lengths)
    return (D, wp) if batched else (D[0], wp[0])


# --------------------------------------------------------------------------------------------------
# recurrence quantification alignment (include/jsgx.h, section 9: libjsgx.so)
# --------------------------------------------------------------------------------------------------
def _rqa_args(d_sim, d_score, gap_onset, gap_extend, knight_moves, d_step, d_path_i, d_path_j, d_path_len, d_end, d_total) -> capix.RqaArgs:
    import torch
    r, s = _planes(d_sim, "d_sim"), _planes(d_score, "d_score")
    P, N, M = r.shape
    assert tuple(s.shape) == (P, N, M), "d_score: the shape of d_sim"
    ptr = lambda t: None if t is None else t.data_ptr()
    step_ptr, step_pitch, step_pair_pitch = None, 0, 0
    if d_step is not None:
        st = _planes(d_step, "d_step", torch.int8)
        assert tuple(st.shape) == (P, N, M), "d_step: int8, the shape of d_sim"
        step_ptr, step_pitch, step_pair_pitch = st.data_ptr(), st.stride(1), st.stride(0)
    path_pitch, max_path = _path_args(d_path_i, d_path_j, P)
    for t, dtype, count, what in ((d_path_len, torch.int32, P, "d_path_len: int32 CUDA [pairs]"), (d_end, torch.int32, 2 * P, "d_end: int32 CUDA [pairs][2]"),
                                  (d_total, torch.float32, P, "d_total: float32 CUDA [pairs]")):
        assert t is None or (t.is_cuda and t.dtype == dtype and t.numel() >= count and t.is_contiguous()), what
    return capix.RqaArgs(r.data_ptr(), r.stride(1), r.stride(0), P, N, M, int(bool(knight_moves)), float(gap_onset), float(gap_extend), 0, max_path,
                         s.data_ptr(), s.stride(1), s.stride(0), step_ptr, step_pitch, step_pair_pitch, ptr(d_path_i), ptr(d_path_j), path_pitch,
                         ptr(d_path_len), ptr(d_end), ptr(d_total))


def rqa_scratch_bytes(d_sim, d_score, *, gap_onset: float = 1.0, gap_extend: float = 1.0, knight_moves: bool = True, d_step=None, d_path_i=None,
                      d_path_j=None, d_path_len=None, d_end=None, d_total=None) -> int:
    """jsgx_rqa_scratch_bytes: the bytes of scratch rqa_launch needs for these arguments (0 for the score alone)."""
    a = _rqa_args(d_sim, d_score, gap_onset, gap_extend, knight_moves, d_step, d_path_i, d_path_j, d_path_len, d_end, d_total)
    return int(capix.check(capix.lib().jsgx_rqa_scratch_bytes(C.byref(a))))


def rqa_launch(d_sim, d_score, *, gap_onset: float = 1.0, gap_extend: float = 1.0, knight_moves: bool = True, d_step=None, d_path_i=None,
               d_path_j=None, d_path_len=None, d_end=None, d_total=None, d_scratch=None, stream: int | None = None):
    """jsgx_rqa_launch: d_sim float32 [n][m] or [pairs][n][m] (a cell is a link where it is > 0) -> d_score (S, the same shape), and where
    given d_step int8 (the step of every cell: 0, 1, 2, -1 no step, -2 a start on the border), d_path_i, d_path_j int32
    [pairs][max_path >= min(n, m)] (the best aligned run, ascending), d_path_len int32 [pairs] (its length; 0: no cell with S > 0),
    d_end int32 [pairs][2] (its last cell, or -1, -1) and d_total float32 [pairs] (S there).  Enqueue only: one kernel per tile
    anti-diagonal, then the backtrace."""
    import torch
    a = _rqa_args(d_sim, d_score, gap_onset, gap_extend, knight_moves, d_step, d_path_i, d_path_j, d_path_len, d_end, d_total)
    d_scratch, stream = _scratch_and_stream(d_scratch, stream, d_sim, lambda: max(1, capix.check(capix.lib().jsgx_rqa_scratch_bytes(C.byref(a))) // 4), torch.int32,
                                            any_dtype=True)
    capix.check(capix.lib().jsgx_rqa_launch(C.byref(a), d_scratch.data_ptr(), d_scratch.numel() * d_scratch.element_size(), stream))


def rqa_plan(n: int, m: int, pairs: int = 1, backtrack: bool = True):
    """jsgx_rqa_plan: (kernel name, tile rows, tile columns, kernel launches, lanes per workgroup, bytes of LDS per workgroup) for this
    shape: one launch per tile anti-diagonal and one for the backtrace.  Needs no device."""
    a = capix.RqaArgs(sim=1 << 44, sim_pitch=int(m), sim_pair_pitch=int(n) * int(m), pairs=int(pairs), n=int(n), m=int(m), knight=1, gap_onset=1.0, gap_extend=1.0,
                      score=2 << 44, score_pitch=int(m), score_pair_pitch=int(n) * int(m), path_len=(3 << 44) if backtrack else None)      # never dereferenced
    return _tiles_plan(capix.lib().jsgx_rqa_plan, a)


def rqa(sim, gap_onset=1.0, gap_extend=1.0, knight_moves=True, backtrack=True):
    """librosa.sequence.rqa on the GPU: from a similarity plane sim [N, M] (a numpy array or a float32 CUDA tensor; recurrence_matrix in
    affinity mode and cross_similarity make one) -> (score, path): the alignment score of every cell [N, M] and the best aligned run,
    int32 [L, 2] ascending, as CUDA tensors; backtrack False: score alone.  A plane without a positive score has an empty path.  A leading
    axis of P pairs is allowed: score is [P, N, M] and path a list.  Reading the path lengths is the one host synchronisation.  A cell
    is a link where sim > 0; the differences from librosa are listed in include/jsgx.h section 9."""
    import torch
    s, _ = _to_cuda(sim)
    assert s.dim() in (2, 3), "rqa: sim [N, M] or [P, N, M]"
    s = s.contiguous()
    batched = s.dim() == 3
    s3 = s if batched else s[None]
    P, N, M = s3.shape
    score = torch.empty_like(s3)
    with torch.cuda.device(_device_index(s)):
        if not backtrack:
            rqa_launch(s3, score, gap_onset=gap_onset, gap_extend=gap_extend, knight_moves=knight_moves)
            return score if batched else score[0]
        path = torch.empty((2, P, min(N, M)), dtype=torch.int32, device=s.device)
        length = torch.empty((P,), dtype=torch.int32, device=s.device)
        rqa_launch(s3, score, gap_onset=gap_onset, gap_extend=gap_extend, knight_moves=knight_moves, d_path_i=path[0], d_path_j=path[1], d_path_len=length)
    wp = _cut_paths(path, length.tolist())           # the one host synchronisation
    return (score, wp) if batched else (score[0], wp[0])


# --------------------------------------------------------------------------------------------------
# path enhancement and time-lag conversion of a recurrence plane (include/jsgx.h, sections 10 and 11: libjsgx.so)
# --------------------------------------------------------------------------------------------------
def _pe_window(window, n: int) -> np.ndarray:
    """The n window samples in double: "hann" is the symmetric form (scipy's get_window(..., fftbins=False)); an array is taken as given."""
    n = int(n)
    if isinstance(window, str):
        if window != "hann":
            raise JsgError(capix.JSGX_ERR_INVALID, f"window must be 'hann' or an array of n samples, not {window!r}")
        return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / max(n - 1, 1))
    w = np.ascontiguousarray(window, dtype=np.float64)
    if w.shape != (n,):
        raise JsgError(capix.JSGX_ERR_INVALID, f"window must be 'hann' or an array of n = {n} samples, not one of shape {w.shape}")
    return w


def diagonal_filter(window, n: int, slope: float = 1.0, zero_mean: bool = False) -> np.ndarray:
    """librosa.segment.path_enhance's filter of one slope as a dense float64 table (jsgx_diagonal_filter_table): diag(window), rotated as
    scipy.ndimage.rotate(order=5, prefilter=False) does unless the slope is 1, clipped at 0, normalised to sum 1; zero_mean subtracts the
    table's mean.  Host only."""
    w = _pe_window(window, n)
    rows, cols = C.c_int32(), C.c_int32()
    capix.check(capix.lib().jsgx_diagonal_filter_table(w.ctypes.data, int(n), float(slope), int(bool(zero_mean)), C.byref(rows), C.byref(cols), None, 0))
    table = np.zeros((rows.value, cols.value), dtype=np.float64)
    capix.check(capix.lib().jsgx_diagonal_filter_table(w.ctypes.data, int(n), float(slope), int(bool(zero_mean)), C.byref(rows), C.byref(cols), table.ctypes.data, table.size))
    return table


def path_enhance_filters(n: int, *, window="hann", max_ratio: float = 2.0, min_ratio=None, n_filters: int = 7, zero_mean: bool = False, drop_below: float = 0.0):
    """The bank of librosa.segment.path_enhance as the tap list of include/jsgx.h section 10 (jsgx_diagonal_filter_build) -> (tap_w
    float32 [T], tap_at int32 [T] ((di << 16) | (dj & 0xffff)), filter_first int32 [n_filters + 1], reach_i, reach_j) on the host.
    min_ratio None: 1 / max_ratio.  drop_below: taps below this fraction of their table's largest are dropped (0: librosa's filters)."""
    w = _pe_window(window, n)
    lo = 1.0 / float(max_ratio) if min_ratio is None else float(min_ratio)
    head = (w.ctypes.data, int(n), lo, float(max_ratio), int(n_filters), int(bool(zero_mean)), float(drop_below))
    count, ri, rj = C.c_int32(), C.c_int32(), C.c_int32()
    capix.check(capix.lib().jsgx_diagonal_filter_build(*head, C.byref(count), C.byref(ri), C.byref(rj), None, None, None, 0))
    tap_w, tap_at, first = np.zeros(count.value, np.float32), np.zeros(count.value, np.int32), np.zeros(int(n_filters) + 1, np.int32)
    capix.check(capix.lib().jsgx_diagonal_filter_build(*head, C.byref(count), C.byref(ri), C.byref(rj), tap_w.ctypes.data, tap_at.ctypes.data, first.ctypes.data, count.value))
    return tap_w, tap_at, first, ri.value, rj.value


def _pe_args(d_r, d_tap_w, d_tap_at, d_filter_first, d_out, reach_i, reach_j, clip) -> capix.PathEnhanceArgs:
    import torch
    r, o = _planes(d_r, "d_r"), _planes(d_out, "d_out")
    P, N, M = r.shape
    assert tuple(o.shape) == (P, N, M), "d_out: the shape of d_r"
    for t, dtype, what in ((d_tap_w, torch.float32, "d_tap_w: float32"), (d_tap_at, torch.int32, "d_tap_at: int32"), (d_filter_first, torch.int32, "d_filter_first: int32")):
        assert t.is_cuda and t.dtype == dtype and t.dim() == 1 and t.is_contiguous(), f"{what} CUDA, contiguous"
    assert d_tap_at.numel() == d_tap_w.numel() and d_filter_first.numel() >= 2, "d_tap_w and d_tap_at [n_taps], d_filter_first [n_filters + 1]"
    return capix.PathEnhanceArgs(r.data_ptr(), r.stride(1), r.stride(0), d_tap_w.data_ptr(), d_tap_at.data_ptr(), d_filter_first.data_ptr(), P, N, M,
                                 d_filter_first.numel() - 1, d_tap_w.numel(), int(reach_i), int(reach_j), int(bool(clip)), o.data_ptr(), o.stride(1), o.stride(0))


def path_enhance_launch(d_r, d_tap_w, d_tap_at, d_filter_first, d_out, *, reach_i: int, reach_j: int, clip: bool = True, stream: int | None = None):
    """jsgx_path_enhance_launch: d_r float32 [n][m] or [pairs][n][m] and a tap list on the device (path_enhance_filters, or the caller's:
    weights, packed offsets, the first tap of every filter and the end) -> d_out, the same shape: per cell the maximum over the filters
    of the fmaf chain of its taps in list order, +0 outside the plane; clip: negative results become +0.  A tap further than reach_i
    rows or reach_j columns is skipped.  Enqueue only."""
    a = _pe_args(d_r, d_tap_w, d_tap_at, d_filter_first, d_out, reach_i, reach_j, clip)
    capix.check(capix.lib().jsgx_path_enhance_launch(C.byref(a), _stream_handle(stream, d_out)))


def path_enhance_plan(reach_i: int, reach_j: int, n: int = 64, m: int = 64, pairs: int = 1):
    """jsgx_path_enhance_plan: (kernel name, tile rows, tile columns, lanes per workgroup, bytes of LDS per workgroup) for these reaches.
    Needs no device."""
    a = capix.PathEnhanceArgs(r=1 << 44, r_pitch=int(m), r_pair_pitch=int(n) * int(m), tap_w=2 << 44, tap_at=3 << 44, filter_first=4 << 44, pairs=int(pairs), n=int(n),
                              m=int(m), n_filters=1, n_taps=1, reach_i=int(reach_i), reach_j=int(reach_j), clip=1, out=5 << 44, out_pitch=int(m),
                              out_pair_pitch=int(n) * int(m))      # never dereferenced
    name, out = C.create_string_buffer(32), [C.c_int32() for _ in range(4)]
    capix.check(capix.lib().jsgx_path_enhance_plan(C.byref(a), name, 32, *[C.byref(o) for o in out]))
    return (name.value.decode(),) + tuple(o.value for o in out)


def path_enhance(R, n: int, *, window="hann", max_ratio: float = 2.0, min_ratio=None, n_filters: int = 7, zero_mean: bool = False, drop_below: float = 0.0,
                 clip: bool = True, out=None):
    """librosa.segment.path_enhance on the GPU: R float32 CUDA [N][M] or [P][N][M] (recurrence_matrix in affinity mode, cross_similarity)
    -> the plane smoothed along diagonals of n_filters slopes between min_ratio and max_ratio, the maximum over the slopes, the same
    shape.  The bank is built once per set of parameters and device (path_enhance_filters) and stays on the device.  out: a tensor of
    R's shape to write into (it must not overlap R).  Query-major like section 7: row i holds the neighbours of frame i; a bank of
    slopes min_ratio..max_ratio with min_ratio = 1 / max_ratio is its own transpose, so the orientation does not change the result's
    meaning.  Every operation is as include/jsgx.h section 10 states it: float32 fmaf chains in list order (scipy sums in float64)."""
    import torch
    assert hasattr(R, "is_cuda") and R.is_cuda and R.dtype == torch.float32 and R.dim() in (2, 3), "path_enhance: R float32 CUDA [N][M] or [P][N][M]"
    r = R if R.stride(-1) == 1 else R.contiguous()
    key = ("path_enhance", int(n), window if isinstance(window, str) else tuple(float(v) for v in window), float(max_ratio), None if min_ratio is None else float(min_ratio),
           int(n_filters), bool(zero_mean), float(drop_below))
    dev_key = (str(r.device),) + key
    if dev_key not in _beat_cache:
        tap_w, tap_at, first, ri, rj = path_enhance_filters(n, window=window, max_ratio=max_ratio, min_ratio=min_ratio, n_filters=n_filters, zero_mean=zero_mean,
                                                            drop_below=drop_below)
        _beat_cache[dev_key] = (torch.from_numpy(tap_w).to(r.device), torch.from_numpy(tap_at).to(r.device), torch.from_numpy(first).to(r.device), ri, rj)
    d_w, d_at, d_first, ri, rj = _beat_cache[dev_key]
    if out is None:
        out = torch.empty(tuple(r.shape), dtype=torch.float32, device=r.device)
    assert tuple(out.shape) == tuple(r.shape), "out: the shape of R"
    with torch.cuda.device(_device_index(r)):
        path_enhance_launch(r, d_w, d_at, d_first, out, reach_i=ri, reach_j=rj, clip=clip)
    return out


def _lag_axis(axis: int) -> int:
    if axis not in (-1, 1, 0, -2):
        raise JsgError(capix.JSGX_ERR_INVALID, f"axis must be -1, 1, 0 or -2 (of the plane's two axes), not {axis!r}")
    return 1 if axis in (-1, 1) else 0


def lag_launch(d_in, d_out, *, pad: bool = True, axis: int = -1, inverse: bool = False, stream: int | None = None):
    """jsgx_lag_launch: the time-lag conversion of square planes.  To lag (inverse False): d_in float32 [n][n] or [pairs][n][n] -> d_out
    [L][n] (axis -1 or 1: lag[l][j] = R[(l + j) mod L][j]) or [n][L] (axis 0 or -2), L = 2 n with pad else n; from lag (inverse True) the
    shapes are exchanged and pad says which L the input has.  A pure permutation; the padding is +0.  Enqueue only."""
    i, o = _planes(d_in, "d_in"), _planes(d_out, "d_out")
    ax = _lag_axis(axis)
    square, lagged = (o, i) if inverse else (i, o)
    P, N = square.shape[0], square.shape[1]
    L = 2 * N if pad else N
    assert square.shape[2] == N and tuple(lagged.shape) == ((P, L, N) if ax == 1 else (P, N, L)), "lag_launch: a square plane and its lag plane for this pad and axis"
    a = capix.LagArgs(i.data_ptr(), i.stride(1), i.stride(0), P, N, int(bool(pad)), ax, int(bool(inverse)), 0, o.data_ptr(), o.stride(1), o.stride(0))
    capix.check(capix.lib().jsgx_lag_launch(C.byref(a), _stream_handle(stream, d_out)))


def recurrence_to_lag(R, pad: bool = True, axis: int = -1):
    """librosa.segment.recurrence_to_lag on the GPU: R float32 CUDA [N][N] or [P][N][N] -> the lag plane, [L][N] for axis -1 (lag[l][j] =
    R[(l + j) mod L][j]) or [N][L] for axis 0 (of the plane's two axes), L = 2 N with pad (the added half is +0) else N.  Query-major as
    section 7: with axis -1 the lag l of column j is the row distance i - j of a frame i that has j among its neighbours."""
    import torch
    assert hasattr(R, "is_cuda") and R.is_cuda and R.dtype == torch.float32 and R.dim() in (2, 3) and R.shape[-1] == R.shape[-2], "recurrence_to_lag: R float32 CUDA, square"
    r = R if R.stride(-1) == 1 else R.contiguous()
    N = r.shape[-1]
    L = 2 * N if pad else N
    shape = tuple(r.shape[:-2]) + ((L, N) if _lag_axis(axis) == 1 else (N, L))
    out = torch.empty(shape, dtype=torch.float32, device=r.device)
    with torch.cuda.device(_device_index(r)):
        lag_launch(r, out, pad=pad, axis=axis)
    return out


def lag_to_recurrence(lag, axis: int = -1):
    """librosa.segment.lag_to_recurrence on the GPU: the inverse of recurrence_to_lag; whether the lag plane was padded is read from its
    shape ([L][N] for axis -1, [N][L] for axis 0, L = N or 2 N)."""
    import torch
    assert hasattr(lag, "is_cuda") and lag.is_cuda and lag.dtype == torch.float32 and lag.dim() in (2, 3), "lag_to_recurrence: lag float32 CUDA"
    g = lag if lag.stride(-1) == 1 else lag.contiguous()
    ax = _lag_axis(axis)
    N, L = (g.shape[-1], g.shape[-2]) if ax == 1 else (g.shape[-2], g.shape[-1])
    if L not in (N, 2 * N):
        raise JsgError(capix.JSGX_ERR_INVALID, f"lag_to_recurrence: a lag plane of {N} frames has {N} or {2 * N} lags, not {L}")
    out = torch.empty(tuple(g.shape[:-2]) + (N, N), dtype=torch.float32, device=g.device)
    with torch.cuda.device(_device_index(g)):
        lag_launch(g, out, pad=(L == 2 * N and N > 0), axis=axis, inverse=True)
    return out


# --------------------------------------------------------------------------------------------------
# Non-negative matrix factorisation (include/jsgx.h, section 12: libjsgx.so)
# --------------------------------------------------------------------------------------------------
def _nmf_args(d_v, d_a, d_c, n_iter, update_components) -> capix.NmfArgs:
    v, a, c = _planes(d_v, "d_v"), _planes(d_a, "d_a"), _planes(d_c, "d_c")
    P, T, K = v.shape
    r = c.shape[1]
    assert tuple(a.shape) == (P, T, r) and tuple(c.shape) == (P, r, K), "nmf: d_v [T][K], d_a [T][r], d_c [r][K], with the same leading problems if any"
    # a row of one element may carry any stride: the pitch the library sees is then the row length or more
    pitch = lambda t: t.stride(1) if t.shape[1] > 1 else max(t.shape[2], t.stride(1))
    return capix.NmfArgs(v.data_ptr(), pitch(v), v.stride(0), a.data_ptr(), pitch(a), a.stride(0), c.data_ptr(), pitch(c), c.stride(0), P, T, K, r, int(n_iter),
                         int(bool(update_components)), capix.NMF_FROBENIUS, 0)


def nmf_scratch_bytes(d_v, d_a, d_c, *, n_iter: int = 1, update_components: bool = True) -> int:
    """jsgx_nmf_scratch_bytes: the bytes of scratch nmf_launch needs for these arguments."""
    return int(capix.check(capix.lib().jsgx_nmf_scratch_bytes(C.byref(_nmf_args(d_v, d_a, d_c, n_iter, update_components)))))


def nmf_launch(d_v, d_a, d_c, *, n_iter: int, update_components: bool = True, d_scratch=None, stream: int | None = None):
    """jsgx_nmf_launch: n_iter multiplicative updates (Frobenius loss, scikit-learn's solver="mu" order) of d_a float32 [T][r] and, with
    update_components, d_c float32 [r][K], in place, for d_v float32 [T][K] ~ d_a d_c; a leading axis of problems is allowed on all three.
    d_a and d_c hold the start.  d_scratch: a contiguous CUDA tensor of at least nmf_scratch_bytes bytes (None: one is allocated with
    torch for this call).  Enqueue only."""
    import torch
    a = _nmf_args(d_v, d_a, d_c, n_iter, update_components)
    d_scratch, stream = _scratch_and_stream(d_scratch, stream, d_v, lambda: capix.check(capix.lib().jsgx_nmf_scratch_bytes(C.byref(a))) // 4, torch.float32,
                                            any_dtype=True)
    capix.check(capix.lib().jsgx_nmf_launch(C.byref(a), d_scratch.data_ptr(), d_scratch.numel() * d_scratch.element_size(), stream))


def nmf_plan(n_frames: int, n_bins: int, n_components: int, problems: int = 1, update_components: bool = True):
    """jsgx_nmf_plan: (name of the kernel that sweeps V, lanes per workgroup, bytes of LDS per workgroup, launches per iteration, frame
    chunks) for this shape.  Needs no device."""
    T, K, r = int(n_frames), int(n_bins), int(n_components)
    a = capix.NmfArgs(v=1 << 44, v_pitch=K, v_problem_pitch=T * K, a=2 << 44, a_pitch=r, a_problem_pitch=T * r, c=3 << 44, c_pitch=K, c_problem_pitch=r * K,
                      problems=int(problems), n_frames=T, n_bins=K, n_components=r, n_iter=1, update_components=int(bool(update_components)),
                      loss=capix.NMF_FROBENIUS, reserved0=0)      # never dereferenced
    name, out = C.create_string_buffer(16), [C.c_int32() for _ in range(4)]
    capix.check(capix.lib().jsgx_nmf_plan(C.byref(a), name, 16, *[C.byref(o) for o in out]))
    return (name.value.decode(),) + tuple(o.value for o in out)


def decompose(S, n_components=None, *, n_iter: int = 200, components=None, activations=None, fit: bool = True, sort: bool = False, seed: int = 0):
    """librosa.decompose.decompose on the GPU (non-negative matrix factorisation, include/jsgx.h section 12): S float32 CUDA [T][K] or
    [P][T][K], non-negative, frame-major as stft_fb, cqt and hpss write it -> (components [r][K], activations [T][r]) with S ~
    activations @ components; librosa documents the transposes.  n_components None: K (at most 64).  The start is the caller's
    `components` / `activations` (copied, not written) and else scikit-learn's init="random" rule, sqrt(mean(S) / r) * |randn| from a torch
    generator seeded with `seed` (plumbing: the contract begins at the start).  fit=False needs `components`, keeps them fixed and
    starts the activations at the constant sqrt(mean(S) / r): scikit-learn's transform.  sort=True orders the components by the bin of
    their peak, ties to the lower component, and the activations alike (librosa's axis_sort).  A fixed n_iter, no tolerance."""
    import torch
    assert hasattr(S, "is_cuda") and S.is_cuda and S.dtype == torch.float32 and S.dim() in (2, 3), "decompose: S float32 CUDA [T][K] or [P][T][K]"
    v = S if S.stride(-1) == 1 else S.contiguous()
    lead, (T, K) = tuple(v.shape[:-2]), v.shape[-2:]
    if components is not None:
        assert components.is_cuda and components.dtype == torch.float32 and tuple(components.shape[:-2]) == lead and components.shape[-1] == K, \
            "components: float32 CUDA [r][K], with the problems of S if any"
        if n_components is None:
            n_components = components.shape[-2]
    if not fit and components is None:
        raise JsgError(capix.JSGX_ERR_INVALID, "decompose: fit=False needs components")
    r = K if n_components is None else int(n_components)
    if not 1 <= r <= capix.NMF_MAX_COMPONENTS:
        raise JsgError(capix.JSGX_ERR_INVALID, f"decompose: n_components must be in 1..{capix.NMF_MAX_COMPONENTS}, not {r}")
    assert components is None or components.shape[-2] == r, "components: n_components rows"
    assert activations is None or (activations.is_cuda and activations.dtype == torch.float32 and tuple(activations.shape) == lead + (T, r)), \
        "activations: float32 CUDA [T][r], with the problems of S if any"
    with torch.cuda.device(_device_index(v)):
        scale = torch.sqrt(v.mean(dim=(-2, -1), keepdim=True) / r)
        gen = torch.Generator(device=v.device)
        gen.manual_seed(int(seed))
        rand = lambda *shape: (scale * torch.randn(lead + shape, generator=gen, device=v.device, dtype=torch.float32).abs()).contiguous()
        c = components.clone().contiguous() if components is not None else rand(r, K)
        if not fit:
            a = scale.expand(lead + (T, r)).contiguous()
        else:
            a = activations.clone().contiguous() if activations is not None else rand(T, r)
        nmf_launch(v, a, c, n_iter=n_iter, update_components=fit)
        if sort:
            order = torch.argsort(torch.argmax(c, dim=-1), dim=-1, stable=True)
            c = torch.gather(c, -2, order[..., :, None].expand_as(c))
            a = torch.gather(a, -1, order[..., None, :].expand_as(a))
    return c, a


# --------------------------------------------------------------------------------------------------
# Per-channel energy normalisation (include/jsgx.h, section 13: libjsgx.so)
# --------------------------------------------------------------------------------------------------
_pcen_decay_cache: dict = {}


def pcen_coefficient(time_constant: float, sr: float, hop_length: int) -> float:
    """librosa.pcen's smoothing coefficient b = (sqrt(1 + 4 T^2) - 1) / (2 T^2), T = time_constant * sr / hop_length, in double."""
    T = float(time_constant) * float(sr) / float(hop_length)
    return (np.sqrt(1.0 + 4.0 * T * T) - 1.0) / (2.0 * T * T)


def pcen_decay(b: float) -> np.ndarray:
    """jsgx_pcen_decay_build: the table q[j] = (float)((1 - b)^(j + 1)), j = 0..255, of the float32 b.  Needs no device."""
    out = np.empty(capix.PCEN_CHUNK, np.float32)
    capix.check(capix.lib().jsgx_pcen_decay_build(float(b), out.ctypes.data))
    return out


def _pcen_states(t, R, B, what: str):
    """(pointer, row pitch) of an optional float32 CUDA [rows][bands] (or [bands] for one row) with unit band stride."""
    import torch
    if t is None:
        return None, 0
    t = t[None] if t.dim() == 1 else t
    assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (R, B) and (t.stride(1) == 1 or B == 1), f"{what}: float32 CUDA [rows][bands]"
    return t.data_ptr(), t.stride(0)


def _pcen_args(d_in, d_decay, d_out, b, gain, bias, power, eps, d_state_in, d_state_out, d_smooth) -> capix.PcenArgs:
    import torch
    x, o = _plane(d_in, "d_in"), _plane(d_out, "d_out")
    R, T, B = x.shape
    assert tuple(o.shape) == (R, T, B), "d_out: the shape of d_in"
    assert d_decay.is_cuda and d_decay.dtype == torch.float32 and d_decay.dim() == 1 and d_decay.shape[0] >= capix.PCEN_CHUNK and d_decay.stride(0) == 1, \
        "d_decay: float32 CUDA [256], pcen_decay(b) on the device"
    # a plane of one frame may carry any frame stride: the pitch the library sees is then the frame length or more
    pitch = lambda t: t.stride(1) if T > 1 else max(B, t.stride(1))
    sm = None if d_smooth is None else _plane(d_smooth, "d_smooth")
    assert sm is None or tuple(sm.shape) == (R, T, B), "d_smooth: the shape of d_in"
    si, si_pitch = _pcen_states(d_state_in, R, B, "d_state_in")
    so, so_pitch = _pcen_states(d_state_out, R, B, "d_state_out")
    return capix.PcenArgs(x.data_ptr(), pitch(x), x.stride(0), d_decay.data_ptr(), si, si_pitch, so, so_pitch, None if sm is None else sm.data_ptr(),
                          0 if sm is None else pitch(sm), 0 if sm is None else sm.stride(0), o.data_ptr(), pitch(o), o.stride(0), R, B, T, float(b), float(gain),
                          float(bias), float(power), float(eps))


def pcen_scratch_bytes(d_in, d_decay, d_out, *, b: float, gain: float = 0.98, bias: float = 2.0, power: float = 0.5, eps: float = 1e-6, d_state_in=None,
                       d_state_out=None, d_smooth=None) -> int:
    """jsgx_pcen_scratch_bytes: the bytes of scratch pcen_launch needs for these arguments (0 up to 256 frames)."""
    a = _pcen_args(d_in, d_decay, d_out, b, gain, bias, power, eps, d_state_in, d_state_out, d_smooth)
    return int(capix.check(capix.lib().jsgx_pcen_scratch_bytes(C.byref(a))))


def pcen_launch(d_in, d_decay, d_out, *, b: float, gain: float = 0.98, bias: float = 2.0, power: float = 0.5, eps: float = 1e-6, d_state_in=None,
                d_state_out=None, d_smooth=None, d_scratch=None, stream: int | None = None):
    """jsgx_pcen_launch: d_in float32 [rows][frames][bands] (or one [frames][bands] plane; views with pitches) -> d_out of the same shape,
    (d_in * (eps + S)^-gain + bias)^power - bias^power with S the first-order smoothing of d_in along the frames with coefficient b.
    d_decay: pcen_decay(b) on the device.  d_state_in float32 [rows][bands]: the smoothed value in front of frame 0 (None: frame 0
    itself); d_state_out: the one behind the last frame; d_smooth: S.  d_scratch: a contiguous CUDA tensor of at least
    pcen_scratch_bytes bytes (None: one is allocated with torch for this call).  Enqueue only."""
    import torch
    a = _pcen_args(d_in, d_decay, d_out, b, gain, bias, power, eps, d_state_in, d_state_out, d_smooth)
    d_scratch, stream = _scratch_and_stream(d_scratch, stream, d_in, lambda: capix.check(capix.lib().jsgx_pcen_scratch_bytes(C.byref(a))) // 4, torch.float32,
                                            any_dtype=True)
    capix.check(capix.lib().jsgx_pcen_launch(C.byref(a), d_scratch.data_ptr(), d_scratch.numel() * d_scratch.element_size(), stream))


def pcen_plan(n_frames: int, n_bands: int, rows: int = 1):
    """jsgx_pcen_plan: (form, lanes per workgroup, bytes of LDS per workgroup, launches, chunks of a row) for this shape: "pcen_single" up
    to 256 frames, else "pcen_chunked".  Needs no device."""
    T, B, R = int(n_frames), int(n_bands), int(rows)
    a = capix.PcenArgs(in_=1 << 50, frame_pitch=B, row_pitch=T * B, decay=1 << 40, out=1 << 58, out_frame_pitch=B, out_row_pitch=T * B, rows=R, n_bands=B,
                       n_frames=T, b=0.5, gain=0.98, bias=2.0, power=0.5, eps=1e-6)      # never dereferenced
    name, out = C.create_string_buffer(16), [C.c_int32() for _ in range(4)]
    capix.check(capix.lib().jsgx_pcen_plan(C.byref(a), name, 16, *[C.byref(o) for o in out]))
    return (name.value.decode(),) + tuple(o.value for o in out)


def pcen(plane, *, sr: float = 22050, hop_length: int = 512, gain: float = 0.98, bias: float = 2.0, power: float = 0.5, time_constant: float = 0.4,
         eps: float = 1e-6, b: float | None = None, state=None, return_state: bool = False, return_smooth: bool = False):
    """librosa.pcen on the GPU (include/jsgx.h section 13): plane float32 CUDA [..., frames, bands], non-negative (what stft_fb_db writes with
    linear_out, or a cqt magnitude) -> a new tensor of the same shape.  b None: pcen_coefficient(time_constant, sr, hop_length).  state
    float32 CUDA [..., bands]: the smoothed value in front of frame 0, as a former call returned it (None: frame 0 itself, librosa's
    default); return_state adds the value behind the last frame and return_smooth the smoothed plane: (out[, state][, smooth]).  Differs
    from librosa.pcen on purpose: frames lie along axis -2, the state is the smoothed value itself (not scipy's zi), power > 0 only, no
    max_size, and the plane is taken as it is (librosa's documentation scales audio by 2^31 first).  A plane cut at a multiple of 256
    frames and fed block by block with the state equals the whole in every bit.  Agreement with librosa was not measured."""
    import torch
    assert hasattr(plane, "is_cuda") and plane.is_cuda and plane.dtype == torch.float32 and plane.dim() >= 2, "pcen: plane float32 CUDA [..., frames, bands]"
    lead, (T, B) = tuple(plane.shape[:-2]), plane.shape[-2:]
    x = plane.reshape(-1, T, B)
    x = x if x.stride(2) == 1 else x.contiguous()
    R = x.shape[0]
    b = pcen_coefficient(time_constant, sr, hop_length) if b is None else float(b)
    s_in = None
    if state is not None:
        assert state.is_cuda and state.dtype == torch.float32 and tuple(state.shape) == lead + (B,), "state: float32 CUDA [..., bands]"
        s_in = state.reshape(R, B).contiguous()
    with torch.cuda.device(_device_index(x)):
        key = (_device_index(x), float(np.float32(b)))
        if key not in _pcen_decay_cache:
            _pcen_decay_cache[key] = torch.from_numpy(pcen_decay(b)).to(x.device)
        out = torch.empty((R, T, B), dtype=torch.float32, device=x.device)
        s_out = torch.empty((R, B), dtype=torch.float32, device=x.device) if return_state else None
        smooth = torch.empty((R, T, B), dtype=torch.float32, device=x.device) if return_smooth else None
        pcen_launch(x, _pcen_decay_cache[key], out, b=b, gain=gain, bias=bias, power=power, eps=eps, d_state_in=s_in, d_state_out=s_out, d_smooth=smooth)
    res = (out.reshape(plane.shape),) + ((s_out.reshape(lead + (B,)),) if return_state else ()) + ((smooth.reshape(plane.shape),) if return_smooth else ())
    return res[0] if len(res) == 1 else res


def pcen_audio(x, sr: float, n_fft: int = 2048, hop: int = 512, n_mels: int = 128, fmin: float = 0.0, fmax: float | None = None, **kw):
    """PCEN of the mel power plane of audio x ([samples] or [channels][samples], float32 CUDA): the plane of mel_spectrogram_db before its
    logarithm (stft_fb_db with linear_out) -> pcen with sr and hop_length = hop, nothing returned to the host in between -> float32
    [frames, n_mels], and what pcen's return_state / return_smooth add.  kw: pcen's gain, bias, power, time_constant, eps, b, state."""
    import torch
    with torch.cuda.device(_device_index(x)):
        return pcen(_mel_plane(x, sr, n_fft, hop, n_mels, fmin, fmax, capi.WIN_HANN, capi.MIX_ABSMEAN, False, True), sr=sr, hop_length=hop, **kw)


# --------------------------------------------------------------------------------------------------
# Peak picking and onset detection (include/jsgx.h, section 14: libjsgx.so)
# --------------------------------------------------------------------------------------------------
def _peak_rows(t, rows, least, dtype, what: str):
    """(pointer, row pitch) of an optional CUDA [rows][>= least] (or [>= least] for one row) of `dtype` with unit stride."""
    if t is None:
        return None, 0
    t = t[None] if t.dim() == 1 else t
    assert t.is_cuda and t.dtype == dtype and t.dim() == 2 and t.shape[0] == rows and t.shape[1] >= least and (t.stride(1) == 1 or t.shape[1] == 1), \
        f"{what}: {dtype} CUDA [rows][>= {least}]"
    return t.data_ptr(), t.stride(0)


def _peak_args(d_in, d_peaks, d_n_peaks, pre_max, post_max, pre_avg, post_avg, delta, wait, normalise, d_energy, d_backtracked, d_candidate) -> capix.PeakArgs:
    import torch
    x = d_in[None] if d_in.dim() == 1 else d_in
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and (x.stride(1) == 1 or x.shape[1] == 1), "d_in: float32 CUDA [rows][frames]"
    R, T = x.shape
    p = d_peaks[None] if d_peaks.dim() == 1 else d_peaks
    max_peaks = p.shape[-1]
    peaks, peaks_pitch = _peak_rows(p, R, 1, torch.int32, "d_peaks")
    back, back_pitch = _peak_rows(d_backtracked, R, max_peaks, torch.int32, "d_backtracked")
    assert back is None or R == 1 or back_pitch == peaks_pitch, "d_backtracked: the row pitch of d_peaks"
    assert d_n_peaks.is_cuda and d_n_peaks.dtype == torch.int32 and d_n_peaks.numel() == R and d_n_peaks.is_contiguous(), "d_n_peaks: int32 CUDA [rows]"
    energy, energy_pitch = _peak_rows(d_energy, R, T, torch.float32, "d_energy")
    cand, cand_pitch = _peak_rows(d_candidate, R, T, torch.uint8, "d_candidate")
    return capix.PeakArgs(x.data_ptr(), x.stride(0), energy, energy_pitch, cand, cand_pitch, peaks, back, peaks_pitch, d_n_peaks.data_ptr(), R, T, int(pre_max),
                          int(post_max), int(pre_avg), int(post_avg), float(delta), int(wait), int(bool(normalise)), int(max_peaks))


def peak_scratch_bytes(d_in, d_peaks, d_n_peaks, *, pre_max: int, post_max: int, pre_avg: int, post_avg: int, delta: float, wait: int, normalise: bool = False,
                       d_energy=None, d_backtracked=None, d_candidate=None) -> int:
    """jsgx_peak_scratch_bytes: the bytes of scratch peak_launch needs for these arguments (0 up to capix.PEAK_BLOCK frames)."""
    a = _peak_args(d_in, d_peaks, d_n_peaks, pre_max, post_max, pre_avg, post_avg, delta, wait, normalise, d_energy, d_backtracked, d_candidate)
    return int(capix.check(capix.lib().jsgx_peak_scratch_bytes(C.byref(a))))


def peak_launch(d_in, d_peaks, d_n_peaks, *, pre_max: int, post_max: int, pre_avg: int, post_avg: int, delta: float, wait: int, normalise: bool = False,
                d_energy=None, d_backtracked=None, d_candidate=None, d_scratch=None, stream: int | None = None):
    """jsgx_peak_launch: d_in float32 [rows][frames] (or one [frames] row; views with a row pitch) -> d_n_peaks int32 [rows], the peaks of
    every row (-1: a row with a NaN or an infinity, nothing else is written for it), and d_peaks int32 [rows][max_peaks], the first
    max_peaks of them ascending.  A frame is a peak where it is the maximum of [t - pre_max, t + post_max], at least delta above the
    mean of [t - pre_avg, t + post_avg] (both clipped to the row) and more than wait frames behind the peak before it.  d_energy float32
    [rows][frames] with d_backtracked int32 like d_peaks: every peak moved back to the last local minimum of the energy at or before
    it.  d_candidate uint8 [rows][frames]: the frames that pass the two window tests.  d_scratch: a contiguous CUDA tensor of at least
    peak_scratch_bytes bytes (None: one is allocated with torch for this call).  Enqueue only."""
    import torch
    a = _peak_args(d_in, d_peaks, d_n_peaks, pre_max, post_max, pre_avg, post_avg, delta, wait, normalise, d_energy, d_backtracked, d_candidate)
    d_scratch, stream = _scratch_and_stream(d_scratch, stream, d_in, lambda: max(1, capix.check(capix.lib().jsgx_peak_scratch_bytes(C.byref(a))) // 4), torch.float32,
                                            any_dtype=True)
    capix.check(capix.lib().jsgx_peak_launch(C.byref(a), d_scratch.data_ptr(), d_scratch.numel() * d_scratch.element_size(), stream))


def peak_plan(n_frames: int, rows: int = 1, wait: int = 0):
    """jsgx_peak_plan: (form, lanes per workgroup, bytes of LDS per workgroup, launches, blocks of a row) for this shape: "peak_single" up
    to capix.PEAK_BLOCK frames, else "peak_blocked".  Needs no device."""
    T, R = int(n_frames), int(rows)
    a = capix.PeakArgs(in_=1 << 50, in_pitch=T, peaks=1 << 58, peaks_pitch=1, n_peaks=1 << 40, rows=R, n_frames=T, wait=int(wait), max_peaks=1)      # never dereferenced
    name, out = C.create_string_buffer(16), [C.c_int32() for _ in range(4)]
    capix.check(capix.lib().jsgx_peak_plan(C.byref(a), name, 16, *[C.byref(o) for o in out]))
    return (name.value.decode(),) + tuple(o.value for o in out)


def _peak_lists(peaks, n_peaks, one: bool):
    """The rows' lists cut at their counts (None for a refused row); one synchronising copy of the counts."""
    counts = n_peaks.cpu().tolist()
    assert all(n <= peaks.shape[1] for n in counts), "max_peaks cut a list: pass a larger one or use peak_launch"
    out = [None if n < 0 else peaks[r, :n] for r, n in enumerate(counts)]
    return out[0] if one else out


def peak_pick(x, pre_max: int, post_max: int, pre_avg: int, post_avg: int, delta: float, wait: int, *, normalise: bool = False, max_peaks: int | None = None):
    """librosa.util.peak_pick on the GPU (include/jsgx.h section 14): x [T] or [rows, T] (numpy array or float32 CUDA tensor) -> the peak
    frames, an int32 CUDA tensor for [T] or a list of them, one a row; a row with a NaN or an infinity gives None in its place.  The
    reaches and wait are whole frames; post_max and post_avg are inclusive, where librosa's are exclusive.  max_peaks None: as many as
    a row can hold.  Differs from librosa on purpose: windows clipped at both ends of the row, no special case at frame 0, float32.  The
    call waits for the device once, to read the counts.  Agreement with librosa was not measured."""
    import torch
    xt, _ = _to_cuda(x)
    assert xt.dim() in (1, 2), "peak_pick: x is [T] or [rows, T]"
    xr = (xt[None] if xt.dim() == 1 else xt).contiguous()
    R, T = xr.shape
    most = 1 + (T - 1) // (int(wait) + 1) if max_peaks is None else int(max_peaks)
    with torch.cuda.device(_device_index(xr)):
        peaks = torch.empty((R, most), dtype=torch.int32, device=xr.device)
        n_peaks = torch.empty((R,), dtype=torch.int32, device=xr.device)
        peak_launch(xr, peaks, n_peaks, pre_max=pre_max, post_max=post_max, pre_avg=pre_avg, post_avg=post_avg, delta=delta, wait=wait, normalise=normalise)
        if max_peaks is not None:
            n_peaks = torch.where(n_peaks > most, torch.full_like(n_peaks, most), n_peaks)
        return _peak_lists(peaks, n_peaks, xt.dim() == 1)


def onset_backtrack(events, energy):
    """librosa.onset.onset_backtrack on the GPU: every event frame moved back to the last local minimum of energy [T] at or before it
    (frame 0 counts as one; t is one where energy[t] <= energy[t-1] and energy[t] < energy[t+1]).  events: ints (a list, a numpy array
    or a CUDA tensor), in any order, duplicates allowed -> an int32 CUDA tensor of the same length and order.  The events are made the
    peaks of a launch of their own: a plane that is 2^30 at the events and 0 elsewhere, windows of one frame, delta = 1 and no wait,
    where x >= fl(x + 1) holds for 2^30 alone."""
    import torch
    e, _ = _to_cuda(energy)
    assert e.dim() == 1, "onset_backtrack: energy is [T]"
    e = e.contiguous()
    T = e.shape[0]
    ev = torch.as_tensor(np.asarray(events.cpu() if hasattr(events, "is_cuda") else events, dtype=np.int64), device=e.device).reshape(-1)
    if ev.numel() == 0:
        return torch.empty((0,), dtype=torch.int32, device=e.device)
    assert int(ev.min()) >= 0 and int(ev.max()) < T, "onset_backtrack: events are frames of energy"
    with torch.cuda.device(_device_index(e)):
        marks = torch.zeros((T,), dtype=torch.float32, device=e.device)
        marks[ev] = 2.0 ** 30
        distinct = torch.unique(ev)          # ascending: the order of the peaks
        peaks, back = torch.empty((2, distinct.numel()), dtype=torch.int32, device=e.device)
        n_peaks = torch.empty((1,), dtype=torch.int32, device=e.device)
        peak_launch(marks, peaks, n_peaks, pre_max=0, post_max=0, pre_avg=0, post_avg=0, delta=1.0, wait=0, d_energy=e, d_backtracked=back)
        n = int(n_peaks[0])
        if n < 0:
            raise ValueError("onset_backtrack: energy holds a NaN or an infinity")
        assert n == distinct.numel()
        return back[torch.searchsorted(distinct, ev)]


def _frames_of(seconds: float, sr: float, hop_length: int) -> int:
    return int(seconds * sr // hop_length)


def onset_detect(onset_envelope, *, sr: float = 22050, hop_length: int = 512, backtrack: bool = False, energy=None, normalise: bool = True, units: str = "frames",
                 pre_max: float = 0.03, post_max: float = 0.0, pre_avg: float = 0.10, post_avg: float = 0.10, wait: float = 0.03, delta: float = 0.07):
    """librosa.onset.onset_detect on the GPU: onset_envelope [T] or [rows, T] (numpy array or float32 CUDA tensor; what onset_strength
    returns) -> the onsets of every row: one result for [T], else a list with one a row (None for a row with a NaN or an infinity).  The
    windows and wait are seconds, converted as int(v * sr // hop_length) frames (at 22050 / 512 the defaults are the reaches (1, 0, 4, 4)
    and wait = 1); post_max and post_avg are then inclusive.  backtrack: the onsets moved back to the last local minimum of energy (None:
    the envelope itself) at or before them.  units: "frames" (an int32 CUDA tensor), or converted on the host, "samples" (numpy int64,
    frame * hop_length) and "time" (numpy float64, frame * hop_length / sr).  Differs from librosa on purpose: windows clipped at both
    ends of the row, normalise divides by max - min with nothing added, float32.  Agreement with librosa was not measured."""
    import torch
    assert units in ("frames", "samples", "time"), 'onset_detect: units is "frames", "samples" or "time"'
    xt, _ = _to_cuda(onset_envelope)
    assert xt.dim() in (1, 2), "onset_detect: onset_envelope is [T] or [rows, T]"
    xr = (xt[None] if xt.dim() == 1 else xt).contiguous()
    R, T = xr.shape
    reach = [_frames_of(v, sr, hop_length) for v in (pre_max, post_max, pre_avg, post_avg)]
    w = _frames_of(wait, sr, hop_length)
    most = 1 + (T - 1) // (w + 1)
    d_energy = back = None
    with torch.cuda.device(_device_index(xr)):
        if backtrack:
            d_energy = xr if energy is None else _to_cuda(energy)[0].reshape(R, T).contiguous()
            back = torch.empty((R, most), dtype=torch.int32, device=xr.device)
        peaks = torch.empty((R, most), dtype=torch.int32, device=xr.device)
        n_peaks = torch.empty((R,), dtype=torch.int32, device=xr.device)
        peak_launch(xr, peaks, n_peaks, pre_max=reach[0], post_max=reach[1], pre_avg=reach[2], post_avg=reach[3], delta=delta, wait=w, normalise=normalise,
                    d_energy=d_energy, d_backtracked=back)
        rows = _peak_lists(back if backtrack else peaks, n_peaks, False)
    rows = [_onset_units(f, units, sr, hop_length) for f in rows]
    return rows[0] if xt.dim() == 1 else rows


def _onset_units(frames, units: str, sr: float, hop_length: int):
    """Frames (an int32 CUDA tensor, or None) in `units`: as they are, or on the host as samples (int64) or seconds (float64)."""
    if frames is None or units == "frames":
        return frames
    samples = frames.cpu().numpy().astype(np.int64) * int(hop_length)
    return samples if units == "samples" else samples / float(sr)


def onset_detect_audio(x, sr, n_fft=2048, hop=512, n_mels=128, **kw):
    """The onsets of audio x [samples] (numpy array or float32 CUDA tensor): mel_spectrogram_db -> onset_strength_launch -> onset_detect
    with sr and hop_length = hop, the envelope never leaving the device.  An onset is reported where its window is centred: frame t of
    the mel spectrogram covers the samples t * hop .. t * hop + n_fft - 1 (no centring is applied to the audio), so an onset picked at
    frame t of the envelope is returned as t + n_fft // (2 * hop), and frame * hop (units "samples", "time") is the middle of the window
    that first heard it, as with librosa's centred frames; without that every onset lay n_fft / 2 samples early.  With backtrack the
    minimum is shifted alike.  kw: onset_detect's backtrack, energy, normalise, units, pre_max, post_max, pre_avg, post_avg, wait,
    delta (energy: a row of the envelope's length, in the envelope's own frames)."""
    import torch
    xt, _ = _to_cuda(x)
    assert xt.dim() == 1, "onset_detect_audio: x is one channel [samples]"
    with torch.cuda.device(_device_index(xt)):
        S = mel_spectrogram_db(xt, sr, n_fft, hop, n_mels)
        env = torch.empty((1, S.shape[0]), dtype=torch.float32, device=xt.device)
        onset_strength_launch(S, env)
        units = kw.pop("units", "frames")
        assert units in ("frames", "samples", "time"), 'onset_detect_audio: units is "frames", "samples" or "time"'
        frames = onset_detect(env[0], sr=sr, hop_length=hop, **kw)
        return _onset_units(None if frames is None else frames + int(n_fft) // (2 * int(hop)), units, sr, hop)


# --------------------------------------------------------------------------------------------------
# Aggregation over segments and time-delay embedding (include/jsgx.h, sections 15 and 16: libjsgx.so)
# --------------------------------------------------------------------------------------------------
_SYNC_AGGREGATES = {"mean": capix.SYNC_MEAN, "min": capix.SYNC_MIN, "max": capix.SYNC_MAX, "median": capix.SYNC_MEDIAN}
_STACK_MODES = {"constant": capix.STACK_CONSTANT, "edge": capix.STACK_EDGE}


def _sync_args(d_x, d_bounds, d_n_bounds, d_segments, d_n_segments, d_out, aggregate, pad, bounds_all) -> capix.SyncArgs:
    import torch
    x, o = _planes(d_x, "d_x"), _planes(d_out, "d_out")
    P, N, F = x.shape
    S = o.shape[1]
    assert o.shape[0] == P and o.shape[2] == F and S >= 1, "d_out: float32 CUDA [pairs][max_segments][features]"
    bounds, bounds_pitch, max_bounds = None, 0, 0
    if d_bounds is not None and d_bounds.shape[-1] > 0:
        b = d_bounds[None] if d_bounds.dim() == 1 else d_bounds          # one list: every pair's
        assert b.is_cuda and b.dtype == torch.int32 and b.dim() == 2 and b.shape[0] in (1, P) and (b.stride(1) == 1 or b.shape[1] == 1), "d_bounds: int32 CUDA [max_bounds] or [pairs][max_bounds]"
        bounds, bounds_pitch, max_bounds = b.data_ptr(), 0 if b.shape[0] == 1 else b.stride(0), b.shape[1]
    n_bounds = None
    if d_n_bounds is not None:
        assert d_n_bounds.is_cuda and d_n_bounds.dtype == torch.int32 and d_n_bounds.numel() == P and d_n_bounds.is_contiguous(), "d_n_bounds: int32 CUDA [pairs]"
        n_bounds = d_n_bounds.data_ptr()
    seg = d_segments[None] if d_segments.dim() == 1 else d_segments
    assert seg.is_cuda and seg.dtype == torch.int32 and seg.dim() == 2 and seg.shape[0] == P and seg.shape[1] >= S + 1 and (seg.stride(1) == 1 or seg.shape[1] == 1), \
        "d_segments: int32 CUDA [pairs][>= max_segments + 1]"
    assert d_n_segments.is_cuda and d_n_segments.dtype == torch.int32 and d_n_segments.numel() == P and d_n_segments.is_contiguous(), "d_n_segments: int32 CUDA [pairs]"
    return capix.SyncArgs(x.data_ptr(), x.stride(1), x.stride(0), bounds, bounds_pitch, n_bounds, seg.data_ptr(), seg.stride(0), d_n_segments.data_ptr(), o.data_ptr(),
                          o.stride(1), o.stride(0), P, N, F, max_bounds, max_bounds if bounds_all is None else int(bounds_all), S,
                          _named(_SYNC_AGGREGATES, aggregate, "aggregate"), int(bool(pad)), 0, 0)


def sync_launch(d_x, d_bounds, d_n_bounds, d_segments, d_n_segments, d_out, *, aggregate: str = "mean", pad: bool = True, bounds_all: int | None = None,
                stream: int | None = None):
    """jsgx_sync_launch: d_x float32 [frames][features] or [pairs][frames][features] (frame-major; views with pitches) aggregated over the
    segments between the frames d_bounds int32 [max_bounds] (one list for every pair) or [pairs][max_bounds] (None: no boundary), of
    which pair p takes the first min(d_n_bounds[p], max_bounds) (d_n_bounds int32 [pairs]; None: bounds_all of them, None: all) -> d_out
    float32 [pairs][max_segments][features], one row a segment, d_segments int32 [pairs][>= max_segments + 1], the frames where the
    segments begin and the last one ends, and d_n_segments int32 [pairs], the whole count (-1: a pair whose count is negative or whose
    list decreases; nothing else is written for it).  aggregate: "mean", "min", "max" or "median".  pad: frames 0 and N are boundaries
    too.  Enqueue only."""
    a = _sync_args(d_x, d_bounds, d_n_bounds, d_segments, d_n_segments, d_out, aggregate, pad, bounds_all)
    capix.check(capix.lib().jsgx_sync_launch(C.byref(a), _stream_handle(stream, d_out)))


def sync_plan(n_frames: int, n_features: int, aggregate: str = "mean", pairs: int = 1, max_bounds: int = 1, pad: bool = True):
    """jsgx_sync_plan: (the aggregate's kernel, lanes per workgroup, bytes of LDS per workgroup, launches) for this shape.  Needs no
    device."""
    N, F, P, M = int(n_frames), int(n_features), int(pairs), int(max_bounds)
    S = max(1, min(N, M + 2 * int(bool(pad)) - 1))
    a = capix.SyncArgs(x=1 << 40, x_frame_pitch=F, x_pair_pitch=N * F, bounds=(1 << 44) if M else None, bounds_pitch=M, n_bounds=1 << 42, segments=5 << 60,
                       segments_pitch=S + 1, n_segments=6 << 60, out=1 << 62, out_frame_pitch=F, out_pair_pitch=S * F, pairs=P, n_frames=N, n_features=F,
                       max_bounds=M, max_segments=S, aggregate=_named(_SYNC_AGGREGATES, aggregate, "aggregate"), pad=int(bool(pad)))      # never dereferenced
    name, out = C.create_string_buffer(16), [C.c_int32() for _ in range(3)]
    capix.check(capix.lib().jsgx_sync_plan(C.byref(a), name, 16, *[C.byref(o) for o in out]))
    return (name.value.decode(),) + tuple(o.value for o in out)


def _host_segments(idx, n_frames: int, pad: bool, who: str = "sync", what: str = "idx"):
    """The rule of include/jsgx.h section 15 on the host: the frames u of a non-decreasing list of boundaries (who, what: the caller and
    its name for the list, for the error text)."""
    b = np.asarray(idx, dtype=np.int64).reshape(-1)
    if b.size > capix.SYNC_MAX_BOUNDS:
        raise JsgError(capix.JSGX_ERR_INVALID, f"{who}: at most {capix.SYNC_MAX_BOUNDS} boundaries")
    if (np.diff(b) < 0).any():
        raise JsgError(capix.JSGX_ERR_INVALID, f"{who}: {what} must be non-decreasing (it is not sorted here)")
    c = np.clip(b, 0, n_frames)
    s = np.concatenate(([0], c, [n_frames])) if pad else c
    u = s[np.concatenate(([True], s[1:] != s[:-1]))] if s.size else s
    return c.astype(np.int32), u.astype(np.int32)


def sync(data, idx, aggregate: str = "mean", pad: bool = True, n_idx=None, max_segments: int | None = None):
    """librosa.util.sync on the GPU (include/jsgx.h section 15): data [N, F] or [P, N, F] (numpy array or float32 CUDA tensor) aggregated
    between the frames idx -> (out float32 [..., segments, F], segments int32 [..., segments + 1], n_segments int32 [...]) as CUDA
    tensors: row o of out is the aggregate of the frames segments[o] .. segments[o+1]-1.

    idx on the host (a list or numpy array of ints, one list for every plane): the count follows on the host by the same rule, the three
    results are returned trimmed to it, and nothing waits for the device.  idx on the device, an int32 CUDA tensor [max] or [P, max]
    with n_idx the int32 CUDA count(s), exactly what beat_track, peak_pick's launch or onset_detect leave there: the results have
    max_segments rows (None: as many as the list and the plane allow), of which the first n_segments are written; n_segments is -1 for
    a plane whose count is negative (a refused row upstream) or whose list decreases, and nothing waits for the device.

    Differs from librosa on purpose: the planes are frame-major ([frames][features], what the feature kernels write; librosa aggregates
    along the last axis of a feature-major plane); boundaries are clipped to 0..N, where librosa raises on a negative one; the list must be
    non-decreasing, where librosa sorts it; aggregate is one of "mean", "min", "max", "median", not a callable; float32 throughout, the
    mean summed in chunks of 256 frames.  Agreement with librosa itself was not measured: librosa is not among the test dependencies."""
    import torch
    x, _ = _to_cuda(data)
    assert x.dim() in (2, 3), "sync: data is [N, F] or [P, N, F]"
    one = x.dim() == 2
    xp = x[None] if one else x
    xp = xp if xp.stride(2) == 1 or xp.shape[2] == 1 else xp.contiguous()
    P, N, F = xp.shape
    dev = xp.device
    with torch.cuda.device(_device_index(xp)):
        on_device = hasattr(idx, "is_cuda")
        if on_device:
            assert idx.is_cuda and idx.dtype == torch.int32 and idx.dim() in (1, 2), "sync: idx on the device is int32 [max] or [P, max]"
            bounds = idx if idx.stride(-1) == 1 or idx.shape[-1] == 1 else idx.contiguous()
            n_bounds = None if n_idx is None else n_idx.reshape(-1).contiguous()
            if n_bounds is not None and n_bounds.numel() == 1 and P > 1:
                n_bounds = n_bounds.expand(P).contiguous()
            most = min(N, bounds.shape[-1] + 2 * int(bool(pad)) - 1)
            S = max(1, most) if max_segments is None else int(max_segments)
            keep = S
        else:
            assert n_idx is None, "sync: n_idx goes with idx on the device"
            c, u = _host_segments(idx, N, pad)
            bounds = torch.from_numpy(c).to(dev) if c.size else None
            n_bounds = None
            keep = max(0, u.size - 1) if max_segments is None else min(max(0, u.size - 1), int(max_segments))
            S = max(1, keep)
        out = torch.empty((P, S, F), dtype=torch.float32, device=dev)
        segments = torch.empty((P, S + 1), dtype=torch.int32, device=dev)
        n_segments = torch.empty((P,), dtype=torch.int32, device=dev)
        sync_launch(xp, bounds, n_bounds, segments, n_segments, out, aggregate=aggregate, pad=pad)
        out, segments = out[:, :keep], segments[:, :keep + 1 if keep else 0]
    return (out[0], segments[0], n_segments[0]) if one else (out, segments, n_segments)


def stack_memory_launch(d_x, d_out, *, n_steps: int = 2, delay: int = 1, mode: str = "constant", constant_values: float = 0.0, stream: int | None = None):
    """jsgx_stack_memory_launch: d_x float32 [frames][features] or [pairs][frames][features] -> d_out [pairs][frames][n_steps * features],
    d_out[t][s * features + f] = d_x[t - s * delay][f]; outside the plane constant_values ("constant") or the nearest frame ("edge").
    A negative delay stacks the future.  Bits are copied unchanged.  d_out must not overlap d_x.  Enqueue only."""
    x, o = _planes(d_x, "d_x"), _planes(d_out, "d_out")
    P, N, F = x.shape
    assert tuple(o.shape) == (P, N, int(n_steps) * F), "d_out: float32 CUDA [pairs][frames][n_steps * features]"
    a = capix.StackMemoryArgs(x.data_ptr(), x.stride(1), x.stride(0), o.data_ptr(), o.stride(1), o.stride(0), P, N, F, int(n_steps), int(delay),
                              _named(_STACK_MODES, mode, "mode"), 0.0, 0)
    C.memmove(C.byref(a, capix.StackMemoryArgs.fill.offset), np.float32(constant_values).tobytes(), 4)          # the bits, a NaN's payload included
    capix.check(capix.lib().jsgx_stack_memory_launch(C.byref(a), _stream_handle(stream, d_out)))


def stack_memory(data, n_steps: int = 2, delay: int = 1, mode: str = "constant", constant_values: float = 0.0):
    """librosa.feature.stack_memory on the GPU (include/jsgx.h section 16): data [N, F] or [P, N, F] (numpy array or float32 CUDA tensor) ->
    float32 CUDA [..., N, n_steps * F]: every frame with its n_steps - 1 predecessors delay, 2 delay, ... frames back side by side (a
    negative delay: its successors).  mode "constant" fills what lies outside the plane with constant_values, "edge" with the nearest
    frame.  Differs from librosa on purpose: frame-major planes (librosa stacks along the first axis of a feature-major one), these two
    modes of np.pad only, float32.  Agreement with librosa itself was not measured."""
    import torch
    x, _ = _to_cuda(data)
    assert x.dim() in (2, 3), "stack_memory: data is [N, F] or [P, N, F]"
    xp = x if x.stride(-1) == 1 or x.shape[-1] == 1 else x.contiguous()
    out = torch.empty(tuple(xp.shape[:-1]) + (int(n_steps) * xp.shape[-1],), dtype=torch.float32, device=xp.device)
    with torch.cuda.device(_device_index(xp)):
        stack_memory_launch(xp, out, n_steps=n_steps, delay=delay, mode=mode, constant_values=constant_values)
    return out


def beat_sync_audio(x, sr, n_fft=2048, hop=512, n_mels=128, aggregate: str = "median", pad: bool = True, **kw):
    """Beat-synchronous mel features of audio x [samples] (numpy array or float32 CUDA tensor): beat_track_audio and mel_spectrogram_db,
    then sync of the mel plane over the beat frames with the device's own count, enqueued one after the other with no host
    synchronisation between them.  Returns (bpm float32 [], out float32 [max_segments, n_mels], segments int32 [max_segments + 1],
    n_segments int32 []) as CUDA tensors: the first n_segments rows of out are written.  kw: beat_track_audio's win_length, start_bpm,
    std_bpm, max_bpm, tightness, smooth, normalise, max_beats.  The differences from librosa are sync's."""
    import torch
    xt, _ = _to_cuda(x)
    assert xt.dim() == 1, "beat_sync_audio: x is one channel [samples]"
    with torch.cuda.device(_device_index(xt)):
        bpm, beats, n_beats = beat_track_audio(xt, sr, n_fft, hop, n_mels, **kw)
        S = mel_spectrogram_db(xt, sr, n_fft, hop, n_mels)
        out, segments, n_segments = sync(S, beats, aggregate=aggregate, pad=pad, n_idx=n_beats)
    return bpm, out, segments, n_segments


# --------------------------------------------------------------------------------------------------
# Temporally constrained agglomerative segmentation (include/jsgx.h, section 17: libjsgx.so)
# --------------------------------------------------------------------------------------------------
def _agglo_args(d_x, d_bounds, d_n_bounds, d_segments, d_n_segments, d_out_bounds, d_n_out, n_clusters, pad, bounds_all, d_order, d_height) -> capix.AgglomerativeArgs:
    import torch
    x = _planes(d_x, "d_x")
    P, N, F = x.shape
    bounds, bounds_pitch, max_bounds = None, 0, 0
    if d_bounds is not None and d_bounds.shape[-1] > 0:
        b = d_bounds[None] if d_bounds.dim() == 1 else d_bounds          # one list: every pair's
        assert b.is_cuda and b.dtype == torch.int32 and b.dim() == 2 and b.shape[0] in (1, P) and (b.stride(1) == 1 or b.shape[1] == 1), "d_bounds: int32 CUDA [max_bounds] or [pairs][max_bounds]"
        bounds, bounds_pitch, max_bounds = b.data_ptr(), 0 if b.shape[0] == 1 else b.stride(0), b.shape[1]
    n_bounds = None
    if d_n_bounds is not None:
        assert d_n_bounds.is_cuda and d_n_bounds.dtype == torch.int32 and d_n_bounds.numel() == P and d_n_bounds.is_contiguous(), "d_n_bounds: int32 CUDA [pairs]"
        n_bounds = d_n_bounds.data_ptr()

    def rows(t, what, dtype=torch.int32):
        t = t[None] if t.dim() == 1 else t
        assert t.is_cuda and t.dtype == dtype and t.dim() == 2 and t.shape[0] == P and t.shape[1] >= 1 and (t.stride(1) == 1 or t.shape[1] == 1), f"{what}: {dtype} CUDA [pairs][...]"
        return t
    seg, out = rows(d_segments, "d_segments"), rows(d_out_bounds, "d_out_bounds")
    assert seg.shape[1] >= 2, "d_segments: int32 CUDA [pairs][>= max_segments + 1]"
    for t, what in ((d_n_segments, "d_n_segments"), (d_n_out, "d_n_out")):
        assert t.is_cuda and t.dtype == torch.int32 and t.numel() == P and t.is_contiguous(), f"{what}: int32 CUDA [pairs]"
    assert (d_order is None) == (d_height is None), "d_order and d_height go together"
    order = height = None
    tree_pitch = 0
    if d_order is not None:
        o, h = rows(d_order, "d_order"), rows(d_height, "d_height", torch.float32)
        assert o.shape[1] >= N and h.shape[1] >= N and (P == 1 or o.stride(0) == h.stride(0)), "d_order, d_height: [pairs][>= frames] at one row pitch"
        order, height, tree_pitch = o.data_ptr(), h.data_ptr(), o.stride(0)
    return capix.AgglomerativeArgs(x.data_ptr(), x.stride(1), x.stride(0), bounds, bounds_pitch, n_bounds, seg.data_ptr(), seg.stride(0), d_n_segments.data_ptr(),
                                   out.data_ptr(), out.stride(0), d_n_out.data_ptr(), order, height, tree_pitch, P, N, F, max_bounds,
                                   max_bounds if bounds_all is None else int(bounds_all), seg.shape[1] - 1, out.shape[1], int(n_clusters), int(bool(pad)), 0)


def agglomerative_scratch_bytes(d_x, d_bounds, d_n_bounds, d_segments, d_n_segments, d_out_bounds, d_n_out, *, n_clusters: int, pad: bool = True,
                                bounds_all: int | None = None, d_order=None, d_height=None) -> int:
    """jsgx_agglomerative_scratch_bytes: the bytes of scratch agglomerative_launch needs for these arguments (the plane once more, and a
    few words a frame)."""
    a = _agglo_args(d_x, d_bounds, d_n_bounds, d_segments, d_n_segments, d_out_bounds, d_n_out, n_clusters, pad, bounds_all, d_order, d_height)
    return int(capix.check(capix.lib().jsgx_agglomerative_scratch_bytes(C.byref(a))))


def agglomerative_launch(d_x, d_bounds, d_n_bounds, d_segments, d_n_segments, d_out_bounds, d_n_out, *, n_clusters: int, pad: bool = True,
                         bounds_all: int | None = None, d_order=None, d_height=None, d_scratch=None, stream: int | None = None):
    """jsgx_agglomerative_launch: every stretch of d_x float32 [frames][features] or [pairs][frames][features] (frame-major; views with
    pitches) between two boundaries clustered into min(n_clusters, its frames) runs of frames by Ward's criterion.  d_bounds, d_n_bounds,
    bounds_all, pad, d_segments int32 [pairs][>= stretches + 1] and d_n_segments int32 [pairs]: as in sync_launch (d_bounds None with
    pad: the whole plane is one stretch) -> d_out_bounds int32 [pairs][max_out], the first frames of the clusters of all stretches,
    ascending, and d_n_out int32 [pairs], their whole count (-1: a refused pair, nothing else is written for it: a negative count or a
    decreasing list, a NaN or an infinity between the first and the last boundary, a stretch of more than capix.AGGLO_MAX_STRETCH
    frames).  d_order int32 and d_height float32 [pairs][>= frames], both or neither: step j of the stretch that begins at frame u
    writes the boundary it removes and its cost at index u + j.  d_scratch: a contiguous CUDA tensor of at least
    agglomerative_scratch_bytes bytes (None: one is allocated with torch for this call).  Enqueue only."""
    import torch
    a = _agglo_args(d_x, d_bounds, d_n_bounds, d_segments, d_n_segments, d_out_bounds, d_n_out, n_clusters, pad, bounds_all, d_order, d_height)
    d_scratch, stream = _scratch_and_stream(d_scratch, stream, d_x, lambda: capix.check(capix.lib().jsgx_agglomerative_scratch_bytes(C.byref(a))) // 4, torch.int32,
                                            any_dtype=True)
    capix.check(capix.lib().jsgx_agglomerative_launch(C.byref(a), d_scratch.data_ptr(), d_scratch.numel() * d_scratch.element_size(), stream))


def agglomerative_plan(n_frames: int, n_features: int, pairs: int = 1, max_bounds: int = 0, pad: bool = True):
    """jsgx_agglomerative_plan: (the merge kernel that takes the longest stretch the shape allows, its lanes per workgroup, its bytes of LDS
    per workgroup, launches): "agglo_wave" up to capix.AGGLO_SHORT frames, else "agglo_group".  Needs no device."""
    N, F, P, M = int(n_frames), int(n_features), int(pairs), int(max_bounds)
    S = max(1, min(N, M + 2 * int(bool(pad)) - 1))
    a = capix.AgglomerativeArgs(x=1 << 40, x_frame_pitch=F, x_pair_pitch=N * F, bounds=(1 << 44) if M else None, bounds_pitch=M, n_bounds=(1 << 42) if M else None,
                                segments=5 << 60, segments_pitch=S + 1, n_segments=6 << 60, out_bounds=1 << 62, out_pitch=1, n_out=7 << 60, pairs=P, n_frames=N,
                                n_features=F, max_bounds=M, max_segments=S, max_out=1, n_clusters=1, pad=int(bool(pad)))      # never dereferenced
    name, out = C.create_string_buffer(16), [C.c_int32() for _ in range(3)]
    capix.check(capix.lib().jsgx_agglomerative_plan(C.byref(a), name, 16, *[C.byref(o) for o in out]))
    return (name.value.decode(),) + tuple(o.value for o in out)


def agglomerative(data, k: int, return_tree: bool = False):
    """librosa.segment.agglomerative on the GPU (include/jsgx.h section 17): data [N, F] or [P, N, F] (numpy array or float32 CUDA tensor)
    cut into min(k, N) runs of consecutive frames by temporally constrained Ward clustering -> (bounds int32 [..., min(k, N)], the
    first frame of every run, ascending, and n_bounds int32 [...], their count, -1 for a plane with a NaN or an infinity) as CUDA
    tensors; with return_tree also (order int32 [..., N], height float32 [..., N]): entry j < N - min(k, N) is the boundary step j
    removed and the cost of that step, the other entries are 0.  With k = 1 that is the whole tree: the boundaries for any k' are frame
    0 and those of the last k' - 1 steps.  At most capix.AGGLO_MAX_STRETCH frames.  Nothing waits for the device.

    Differs from librosa (which calls scikit-learn's AgglomerativeClustering) on purpose: the planes are frame-major ([frames][features];
    librosa clusters along the last axis of a feature-major plane); where two merges cost the same the one at the lower frame is
    taken, where sklearn's heap order decides; float32 throughout, where sklearn computes in float64; Ward linkage on the chain of
    frames only.  The float64 form of the same definition gave scikit-learn's boundaries on every plane of tests/test_agglo_ref.py.
    Agreement with librosa itself was not measured: librosa is not among the test dependencies."""
    import torch
    x, _ = _to_cuda(data)
    assert x.dim() in (2, 3), "agglomerative: data is [N, F] or [P, N, F]"
    one = x.dim() == 2
    xp = x[None] if one else x
    xp = xp if xp.stride(2) == 1 or xp.shape[2] == 1 else xp.contiguous()
    P, N, _ = xp.shape
    dev = xp.device
    with torch.cuda.device(_device_index(xp)):
        bounds = torch.empty((P, min(int(k), N) if int(k) >= 1 else 1), dtype=torch.int32, device=dev)
        segments = torch.empty((P, 2), dtype=torch.int32, device=dev)
        n_segments, n_out = torch.empty((2, P), dtype=torch.int32, device=dev)
        order = torch.zeros((P, N), dtype=torch.int32, device=dev) if return_tree else None
        height = torch.zeros((P, N), dtype=torch.float32, device=dev) if return_tree else None
        agglomerative_launch(xp, None, None, segments, n_segments, bounds, n_out, n_clusters=k, pad=True, d_order=order, d_height=height)
    res = (bounds, n_out) + ((order, height) if return_tree else ())
    return tuple(r[0] for r in res) if one else res


def subsegment(data, frames, n_segments: int = 4, pad: bool = True, n_frames=None, max_bounds: int | None = None):
    """librosa.segment.subsegment on the GPU (include/jsgx.h section 17): every stretch of data [N, F] or [P, N, F] (numpy array or
    float32 CUDA tensor) between two of the boundaries `frames` cut into min(n_segments, its frames) runs by temporally constrained Ward
    clustering -> (bounds int32 [..., max_bounds], the first frames of all runs, ascending: the boundaries among them, and n_bounds
    int32 [...], their count) as CUDA tensors.

    frames on the host (a list or numpy array of ints, one list for every plane): the count follows on the host, bounds is returned
    trimmed to it (max_bounds cuts it), and nothing waits for the device.  frames on the device, an int32 CUDA tensor [max] or [P, max]
    with n_frames the int32 CUDA count(s) of the boundaries in it (the name is librosa's word for the list; it is not the number of
    frames of the plane, which is N = data.shape[-2]), exactly what beat_track, peak_pick's launch or onset_detect leave there: bounds has
    max_bounds entries a plane (None: as many as the list and the plane allow), of which the first n_bounds are written, and nothing
    waits for the device.  n_bounds is -1 for a plane whose count is negative (a refused row upstream) or whose list decreases, that
    holds a NaN or an infinity between its first and its last boundary, or that has a stretch of more than capix.AGGLO_MAX_STRETCH frames.

    Differs from librosa on purpose: the planes are frame-major; the boundaries are clipped to 0..N and the list must be non-decreasing,
    as in sync (librosa sorts, and raises on a boundary outside the plane); pad adds both frame 0 and frame N; where two merges cost the
    same the one at the lower frame is taken, where sklearn's heap order decides; float32 throughout.  Agreement with librosa itself
    was not measured: librosa is not among the test dependencies."""
    import torch
    x, _ = _to_cuda(data)
    assert x.dim() in (2, 3), "subsegment: data is [N, F] or [P, N, F]"
    one = x.dim() == 2
    xp = x[None] if one else x
    xp = xp if xp.stride(2) == 1 or xp.shape[2] == 1 else xp.contiguous()
    P, N, _ = xp.shape
    dev = xp.device
    k = int(n_segments)
    with torch.cuda.device(_device_index(xp)):
        if hasattr(frames, "is_cuda"):
            assert frames.is_cuda and frames.dtype == torch.int32 and frames.dim() in (1, 2), "subsegment: frames on the device is int32 [max] or [P, max]"
            bounds = frames if frames.stride(-1) == 1 or frames.shape[-1] == 1 else frames.contiguous()
            n_bounds = None if n_frames is None else n_frames.reshape(-1).contiguous()
            if n_bounds is not None and n_bounds.numel() == 1 and P > 1:
                n_bounds = n_bounds.expand(P).contiguous()
            S = max(1, min(N, bounds.shape[-1] + 2 * int(bool(pad)) - 1))
            keep = max(1, min(N, S * max(k, 1))) if max_bounds is None else int(max_bounds)
        else:
            assert n_frames is None, "subsegment: n_frames goes with frames on the device"
            c, u = _host_segments(frames, N, pad, "subsegment", "frames")
            bounds = torch.from_numpy(c).to(dev) if c.size else None
            n_bounds = None
            S = max(1, min(N, c.size + 2 * int(bool(pad)) - 1))          # what the list could give before its repeats are dropped
            keep = int(np.minimum(np.diff(u), max(k, 1)).sum()) if u.size > 1 else 0
            keep = keep if max_bounds is None else min(keep, int(max_bounds))
        out = torch.empty((P, max(1, keep)), dtype=torch.int32, device=dev)
        segments = torch.empty((P, S + 1), dtype=torch.int32, device=dev)
        n_seg, n_out = torch.empty((2, P), dtype=torch.int32, device=dev)
        agglomerative_launch(xp, bounds, n_bounds, segments, n_seg, out, n_out, n_clusters=k, pad=pad)
        out = out[:, :keep]
    return (out[0], n_out[0]) if one else (out, n_out)


# --------------------------------------------------------------------------------------------------
# Viterbi decoding of hidden Markov models (include/jsgx.h, section 4: libjsgx.so)
# --------------------------------------------------------------------------------------------------
def _viterbi_args(d_log_emit, d_log_init, d_log_trans, d_states, band_half, d_logp, d_value) -> capix.ViterbiArgs:
    import torch
    b = _planes(d_log_emit, "d_log_emit")
    Q, T, S = b.shape
    band = band_half is not None
    rows = 2 * int(band_half) + 1 if band else S
    a = d_log_trans
    assert a.is_cuda and a.dtype == torch.float32 and a.dim() == 2 and tuple(a.shape) == (rows, S) and (a.stride(1) == 1 or S == 1), \
        "d_log_trans: float32 CUDA [states][states], or [2 * band_half + 1][states] with band_half"
    assert d_log_init.is_cuda and d_log_init.dtype == torch.float32 and d_log_init.dim() == 1 and d_log_init.shape[0] == S and d_log_init.is_contiguous(), \
        "d_log_init: float32 CUDA [states]"
    st = d_states[None] if d_states.dim() == 1 else d_states
    assert st.is_cuda and st.dtype == torch.int32 and st.dim() == 2 and tuple(st.shape) == (Q, T) and (st.stride(1) == 1 or T == 1), "d_states: int32 CUDA [seqs][frames]"
    assert d_logp is None or (d_logp.is_cuda and d_logp.dtype == torch.float32 and d_logp.dim() == 1 and d_logp.shape[0] >= Q and d_logp.is_contiguous()), \
        "d_logp: float32 CUDA [seqs]"
    v = None if d_value is None else _planes(d_value, "d_value")
    assert v is None or tuple(v.shape) == (Q, T, S), "d_value: the shape of d_log_emit"
    ptr = lambda t: None if t is None else t.data_ptr()
    return capix.ViterbiArgs(b.data_ptr(), b.stride(1), b.stride(0), d_log_init.data_ptr(), a.data_ptr(), a.stride(0) if rows > 1 else max(S, a.stride(0)),
                             capix.TRANS_BAND if band else capix.TRANS_DENSE, int(band_half) if band else 0, Q, S, T, 0, st.data_ptr(), st.stride(0), ptr(d_logp),
                             ptr(v), 0 if v is None else v.stride(1), 0 if v is None else v.stride(0))


def viterbi_scratch_bytes(d_log_emit, d_log_init, d_log_trans, d_states, *, band_half: int | None = None, d_logp=None, d_value=None) -> int:
    """jsgx_viterbi_scratch_bytes: the bytes of scratch viterbi_launch needs for these arguments."""
    a = _viterbi_args(d_log_emit, d_log_init, d_log_trans, d_states, band_half, d_logp, d_value)
    return int(capix.check(capix.lib().jsgx_viterbi_scratch_bytes(C.byref(a))))


def viterbi_launch(d_log_emit, d_log_init, d_log_trans, d_states, *, band_half: int | None = None, d_logp=None, d_value=None, d_scratch=None,
                   stream: int | None = None):
    """jsgx_viterbi_launch: d_log_emit float32 [frames][states] or [seqs][frames][states] (log-likelihoods, frame-major), d_log_init float32
    [states], d_log_trans float32 [states][states] (source, destination) or, with band_half = W, the diagonal-major band table
    [2W + 1][states] of viterbi_band_transition -> d_states int32 [seqs][frames] (the most likely path), and where given d_logp float32
    [seqs] (its log-probability; -inf: no path has a probability above zero) and d_value float32, the shape of d_log_emit (V).
    d_scratch: a contiguous CUDA tensor of at least viterbi_scratch_bytes bytes (None: one is allocated with torch for this call).
    Enqueue only: the forward kernel, then the blocked backtrace."""
    import torch
    a = _viterbi_args(d_log_emit, d_log_init, d_log_trans, d_states, band_half, d_logp, d_value)
    d_scratch, stream = _scratch_and_stream(d_scratch, stream, d_log_emit, lambda: capix.check(capix.lib().jsgx_viterbi_scratch_bytes(C.byref(a))) // 4, torch.int32,
                                            any_dtype=True)
    capix.check(capix.lib().jsgx_viterbi_launch(C.byref(a), d_scratch.data_ptr(), d_scratch.numel() * d_scratch.element_size(), stream))


def viterbi_plan(n_states: int, n_frames: int, seqs: int = 1, band_half: int | None = None):
    """jsgx_viterbi_plan: (form of the forward kernel, lanes per workgroup, bytes of LDS per workgroup, kernel launches) for this shape:
    "viterbi_dense_lds" / "viterbi_dense_mem" without band_half, "viterbi_band_lds" / "viterbi_band_mem" with it.  Needs no device."""
    S, T = int(n_states), int(n_frames)
    a = capix.ViterbiArgs(log_emit=1 << 44, emit_frame_pitch=S, emit_seq_pitch=S * T, log_init=2 << 44, trans=3 << 44, trans_pitch=S,
                          trans_form=capix.TRANS_DENSE if band_half is None else capix.TRANS_BAND, band_half=0 if band_half is None else int(band_half),
                          seqs=int(seqs), n_states=S, n_frames=T, states=4 << 44, states_pitch=T)      # never dereferenced
    name, out = C.create_string_buffer(32), [C.c_int32() for _ in range(3)]
    capix.check(capix.lib().jsgx_viterbi_plan(C.byref(a), name, 32, *[C.byref(o) for o in out]))
    return (name.value.decode(),) + tuple(o.value for o in out)


def viterbi_band_transition(n_states: int, window) -> np.ndarray:
    """jsgx_viterbi_band_build: the locally normalised band transition of a window of 2W + 1 non-negative weights (window[W] > 0), as
    float32 [2W + 1][n_states], diagonal-major: row i - j + W, column j holds log(window[j - i + W] / the sum of the window over the
    destinations of i inside the matrix), -inf where the source lies outside.  What viterbi_launch takes with band_half = W."""
    w = np.ascontiguousarray(window, dtype=np.float64).reshape(-1)
    if w.size % 2 != 1:
        raise JsgError(capix.JSGX_ERR_INVALID, "viterbi_band_transition: the window has 2 * band_half + 1 entries")
    out = np.empty((w.size, int(n_states)), dtype=np.float32)
    capix.check(capix.lib().jsgx_viterbi_band_build(int(n_states), w.size // 2, w.ctypes.data, out.ctypes.data, int(n_states)))
    return out


def viterbi(log_emit, log_trans, log_init=None, *, band_half=None):
    """The most likely state sequence of a hidden Markov model (librosa.sequence.viterbi, in logarithms): log_emit [T, S] or [Q, T, S]
    (frame-major log-likelihoods), log_trans [S, S] (source, destination) or with band_half = W the band table [2W + 1, S], log_init [S]
    (None: uniform, log(1 / S)); numpy arrays or float32 CUDA tensors -> (states int32 [T] or [Q, T], logp float32 [] or [Q]) as CUDA
    tensors.  logp = -inf: no path has a probability above zero.  Differences from librosa are listed in include/jsgx.h."""
    import torch
    b, _ = _to_cuda(log_emit)
    assert b.dim() in (2, 3), "viterbi: log_emit [T, S] or [Q, T, S]"
    batched = b.dim() == 3
    b3 = (b if batched else b[None]).contiguous()
    Q, T, S = b3.shape
    a = _to_cuda(log_trans)[0].to(b.device).contiguous()
    if log_init is None:
        p0 = torch.full((S,), float(np.float32(np.log(1.0 / S))), dtype=torch.float32, device=b.device)
    else:
        p0 = _to_cuda(log_init)[0].to(b.device).contiguous()
    states = torch.empty((Q, T), dtype=torch.int32, device=b.device)
    logp = torch.empty((Q,), dtype=torch.float32, device=b.device)
    with torch.cuda.device(_device_index(b)):
        viterbi_launch(b3, p0, a, states, band_half=band_half, d_logp=logp)
    return (states, logp) if batched else (states[0], logp[0])


# --------------------------------------------------------------------------------------------------
# pYIN pitch tracking (include/jsgx.h, section 5: libjsgx.so)
# --------------------------------------------------------------------------------------------------
def pyin_prior(n_thresholds: int = 100, beta_parameters=(2, 18)) -> np.ndarray:
    """jsgx_pyin_prior_build: the prior over the n_thresholds thresholds (k + 1) / n_thresholds, float32 [n_thresholds]: the mass of the
    Beta(a, b) distribution between k / N and (k + 1) / N.  Needs no device."""
    out = np.empty((int(n_thresholds),) if 1 <= int(n_thresholds) <= capix.PYIN_MAX_THRESHOLDS else (1,), dtype=np.float32)
    capix.check(capix.lib().jsgx_pyin_prior_build(int(n_thresholds), float(beta_parameters[0]), float(beta_parameters[1]), out.ctypes.data))
    return out


def pyin_tables(sr: float, fmin: float, n_bins: int, bins_per_semitone: int, band_half: int, window, tau_min: int, tau_max: int,
                n_thresholds: int = 100, beta_parameters=(2, 18), boltzmann_parameter: float = 2.0, switch_prob: float = 0.01) -> dict:
    """Every table of pyin_observe_launch and pyin_decode_launch as float32 numpy arrays, from the four host builders of include/jsgx.h
    section 5a: prior [N], decay [n], norm [n + 1] with n = max(1, (tau_max - tau_min + 1) // 2) (the most troughs of a frame), edges
    [n_bins + 1] (descending periods), freqs [n_bins], log_window [2 * band_half + 1], src_offset [n_bins], log_switch [4] and log_init
    [2 * n_bins] (-inf on the voiced states, log(1 / n_bins) on the unvoiced ones).  window: 2 * band_half + 1 non-negative weights.
    Needs no device."""
    l = capix.lib()
    P, W = int(n_bins), int(band_half)
    w = np.ascontiguousarray(window, dtype=np.float64).reshape(-1)
    if w.size != 2 * W + 1:
        raise JsgError(capix.JSGX_ERR_INVALID, "pyin_tables: the window has 2 * band_half + 1 entries")
    n = max(1, (int(tau_max) - int(tau_min) + 1) // 2)
    sized = lambda count, limit: np.empty((count if 1 <= count <= limit else 1,), dtype=np.float32)      # a refused size is refused by the builder
    t = dict(prior=pyin_prior(n_thresholds, beta_parameters), decay=sized(n, capix.PYIN_MAX_LAG), norm=sized(n + 1, capix.PYIN_MAX_LAG + 1),
             edges=sized(P + 1, capix.PYIN_MAX_BINS + 1), freqs=sized(P, capix.PYIN_MAX_BINS),
             log_window=np.empty((w.size,), np.float32), src_offset=sized(P, capix.PYIN_MAX_BINS), log_switch=np.empty((4,), np.float32))
    capix.check(l.jsgx_pyin_boltzmann_build(float(boltzmann_parameter), n, t["decay"].ctypes.data, t["norm"].ctypes.data))
    capix.check(l.jsgx_pyin_bins_build(float(sr), float(fmin), int(bins_per_semitone), P, t["edges"].ctypes.data, t["freqs"].ctypes.data))
    capix.check(l.jsgx_pyin_transition_build(P, W, w.ctypes.data, float(switch_prob), t["log_window"].ctypes.data, t["src_offset"].ctypes.data,
                                             t["log_switch"].ctypes.data))
    t["log_init"] = np.concatenate([np.full(P, -np.inf, np.float32), np.full(P, np.float32(np.log(1.0 / P)), np.float32)])
    return t


def _pyin_vector(t, count: int, what: str):
    import torch
    assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 1 and t.shape[0] >= count and t.is_contiguous(), f"{what}: float32 CUDA [>= {count}]"
    return t.data_ptr()


def _pyin_observe_args(d_cmnd, tau_min, tau_max, d_prior, d_decay, d_norm, d_edges, no_trough_prob, d_log_emit, d_obs, d_voiced_prob) -> capix.PyinObserveArgs:
    import torch
    c = _planes(d_cmnd, "d_cmnd")
    R, T, lags = c.shape
    assert lags >= int(tau_max) + 1, "d_cmnd: float32 CUDA [rows][frames][>= tau_max + 1]"
    e = _planes(d_log_emit, "d_log_emit")
    assert e.shape[0] == R and e.shape[1] == T and e.shape[2] % 2 == 0, "d_log_emit: float32 CUDA [rows][frames][2 * n_bins]"
    P = e.shape[2] // 2
    o = None if d_obs is None else _planes(d_obs, "d_obs")
    assert o is None or tuple(o.shape) == (R, T, P), "d_obs: float32 CUDA [rows][frames][n_bins]"
    v = None
    if d_voiced_prob is not None:
        v = d_voiced_prob[None] if d_voiced_prob.dim() == 1 else d_voiced_prob
        assert v.is_cuda and v.dtype == torch.float32 and v.dim() == 2 and tuple(v.shape) == (R, T) and (v.stride(1) == 1 or T == 1), \
            "d_voiced_prob: float32 CUDA [rows][frames]"
    n = d_decay.shape[0]
    ptr = lambda t: None if t is None else t.data_ptr()
    return capix.PyinObserveArgs(c.data_ptr(), c.stride(1), c.stride(0), R, T, int(tau_min), int(tau_max), _pyin_vector(d_prior, 1, "d_prior"),
                                 _pyin_vector(d_decay, 1, "d_decay"), _pyin_vector(d_norm, n + 1, "d_norm"), _pyin_vector(d_edges, P + 1, "d_edges"),
                                 d_prior.shape[0], n, P, float(no_trough_prob), e.data_ptr(), e.stride(1), e.stride(0), ptr(o), 0 if o is None else o.stride(1),
                                 0 if o is None else o.stride(0), ptr(v), 0 if v is None else v.stride(0))


def pyin_observe_launch(d_cmnd, tau_min: int, tau_max: int, d_prior, d_decay, d_norm, d_edges, d_log_emit, *, no_trough_prob: float = 0.01, d_obs=None,
                        d_voiced_prob=None, stream: int | None = None):
    """jsgx_pyin_observe_launch: d_cmnd float32 [rows][frames][>= tau_max + 1] (the d' plane of yin_launch) and the tables of pyin_tables
    (d_prior [N], d_decay [n], d_norm [n + 1], d_edges [n_bins + 1]) -> d_log_emit float32 [rows][frames][2 * n_bins] (state u * n_bins + p,
    u = 0 voiced), and where given d_obs float32 [rows][frames][n_bins] (the voiced probabilities) and d_voiced_prob float32 [rows][frames].
    Enqueue only: one kernel, no scratch."""
    a = _pyin_observe_args(d_cmnd, tau_min, tau_max, d_prior, d_decay, d_norm, d_edges, no_trough_prob, d_log_emit, d_obs, d_voiced_prob)
    capix.check(capix.lib().jsgx_pyin_observe_launch(C.byref(a), _stream_handle(stream, d_cmnd)))


def pyin_observe_plan(tau_min: int, tau_max: int, n_bins: int, n_frames: int = 1, rows: int = 1, n_thresholds: int = 100):
    """jsgx_pyin_observe_plan: (kernel name, lanes per workgroup, bytes of LDS per workgroup, frames per workgroup).  Needs no device."""
    P, T, lags = int(n_bins), int(n_frames), int(tau_max) + 1
    a = capix.PyinObserveArgs(cmnd=1 << 44, cmnd_frame_pitch=lags, cmnd_row_pitch=lags * T, rows=int(rows), n_frames=T, tau_min=int(tau_min), tau_max=int(tau_max),
                              prior=2 << 44, decay=3 << 44, norm=4 << 44, edges=5 << 44, n_thresholds=int(n_thresholds),
                              boltz_len=max(1, (int(tau_max) - int(tau_min) + 1) // 2), n_bins=P, no_trough_prob=0.01, log_emit=6 << 44, emit_frame_pitch=2 * P,
                              emit_row_pitch=2 * P * T)      # never dereferenced
    name, out = C.create_string_buffer(32), [C.c_int32() for _ in range(3)]
    capix.check(capix.lib().jsgx_pyin_observe_plan(C.byref(a), name, 32, *[C.byref(o) for o in out]))
    return (name.value.decode(),) + tuple(o.value for o in out)


def _pyin_decode_args(d_log_emit, d_log_init, d_log_window, d_src_offset, d_log_switch, d_states, d_logp, d_value) -> capix.PyinDecodeArgs:
    import torch
    b = _planes(d_log_emit, "d_log_emit")
    Q, T, S = b.shape
    assert S % 2 == 0, "d_log_emit: float32 CUDA [seqs][frames][2 * n_bins]"
    P = S // 2
    assert d_log_window.dim() == 1 and d_log_window.shape[0] % 2 == 1, "d_log_window: float32 CUDA [2 * band_half + 1]"
    W = d_log_window.shape[0] // 2
    st = d_states[None] if d_states.dim() == 1 else d_states
    assert st.is_cuda and st.dtype == torch.int32 and st.dim() == 2 and tuple(st.shape) == (Q, T) and (st.stride(1) == 1 or T == 1), "d_states: int32 CUDA [seqs][frames]"
    assert d_logp is None or (d_logp.is_cuda and d_logp.dtype == torch.float32 and d_logp.dim() == 1 and d_logp.shape[0] >= Q and d_logp.is_contiguous()), \
        "d_logp: float32 CUDA [seqs]"
    v = None if d_value is None else _planes(d_value, "d_value")
    assert v is None or tuple(v.shape) == (Q, T, S), "d_value: the shape of d_log_emit"
    ptr = lambda t: None if t is None else t.data_ptr()
    return capix.PyinDecodeArgs(b.data_ptr(), b.stride(1), b.stride(0), _pyin_vector(d_log_init, S, "d_log_init"), _pyin_vector(d_log_window, 2 * W + 1, "d_log_window"),
                                _pyin_vector(d_src_offset, P, "d_src_offset"), _pyin_vector(d_log_switch, 4, "d_log_switch"), P, W, Q, T, st.data_ptr(), st.stride(0),
                                ptr(d_logp), ptr(v), 0 if v is None else v.stride(1), 0 if v is None else v.stride(0))


def pyin_decode_scratch_bytes(d_log_emit, d_log_init, d_log_window, d_src_offset, d_log_switch, d_states, *, d_logp=None, d_value=None) -> int:
    """jsgx_pyin_decode_scratch_bytes: the bytes of scratch pyin_decode_launch needs for these arguments."""
    a = _pyin_decode_args(d_log_emit, d_log_init, d_log_window, d_src_offset, d_log_switch, d_states, d_logp, d_value)
    return int(capix.check(capix.lib().jsgx_pyin_decode_scratch_bytes(C.byref(a))))


def pyin_decode_launch(d_log_emit, d_log_init, d_log_window, d_src_offset, d_log_switch, d_states, *, d_logp=None, d_value=None, d_scratch=None,
                       stream: int | None = None):
    """jsgx_pyin_decode_launch: d_log_emit float32 [frames][2P] or [seqs][frames][2P] (state u * P + p), d_log_init float32 [2P] and the
    factored transition of pyin_tables (d_log_window [2W + 1], d_src_offset [P], d_log_switch [4]) -> d_states int32 [seqs][frames], and
    where given d_logp float32 [seqs] and d_value float32, the shape of d_log_emit (V).  d_scratch: a contiguous CUDA tensor of at least
    pyin_decode_scratch_bytes bytes (None: one is allocated with torch for this call).  Enqueue only: the forward kernel, then the blocked
    backtrace of viterbi_launch."""
    import torch
    a = _pyin_decode_args(d_log_emit, d_log_init, d_log_window, d_src_offset, d_log_switch, d_states, d_logp, d_value)
    d_scratch, stream = _scratch_and_stream(d_scratch, stream, d_log_emit, lambda: capix.check(capix.lib().jsgx_pyin_decode_scratch_bytes(C.byref(a))) // 4,
                                            torch.int32, any_dtype=True)
    capix.check(capix.lib().jsgx_pyin_decode_launch(C.byref(a), d_scratch.data_ptr(), d_scratch.numel() * d_scratch.element_size(), stream))


def pyin_decode_plan(n_bins: int, band_half: int, n_frames: int, seqs: int = 1):
    """jsgx_pyin_decode_plan: (name of the forward kernel, lanes that share a pitch bin, lanes per workgroup, bytes of LDS per workgroup,
    kernel launches) for this shape.  Needs no device."""
    P, T = int(n_bins), int(n_frames)
    a = capix.PyinDecodeArgs(log_emit=1 << 44, emit_frame_pitch=2 * P, emit_seq_pitch=2 * P * T, log_init=2 << 44, log_window=3 << 44, src_offset=4 << 44,
                             log_switch=5 << 44, n_bins=P, band_half=int(band_half), seqs=int(seqs), n_frames=T, states=6 << 44, states_pitch=T)      # never dereferenced
    name, out = C.create_string_buffer(32), [C.c_int32() for _ in range(4)]
    capix.check(capix.lib().jsgx_pyin_decode_plan(C.byref(a), name, 32, *[C.byref(o) for o in out]))
    return (name.value.decode(),) + tuple(o.value for o in out)


def pyin_geometry(sr: float, fmin: float, fmax: float, frame_length: int = 2048, hop_length: int | None = None, resolution: float = 0.1,
                  max_transition_rate: float = 35.92):
    """The model pyin decodes for these arguments, as librosa.pyin lays it out: (bins_per_semitone, n_bins, band_half, tau_min, tau_max).
    bins_per_semitone = ceil(1 / resolution); n_bins = floor(12 bps log2(fmax / fmin)) + 1; the pitch transition is a triangle of
    round(max_transition_rate * 12 * hop / sr) * bps + 1 points (the width librosa passes to transition_local), so its half-width is
    band_half = (round(...) * bps) // 2: 50 at the defaults (hop 512 at 22 050 Hz, 0.1 semitone); tau_min = max(1, floor(sr / fmax)) and
    tau_max = ceil(sr / fmin) are yin's.  Needs no device and refuses nothing: pyin refuses what the library does not serve."""
    import math
    hop = int(frame_length) // 4 if hop_length is None else int(hop_length)
    bps = int(math.ceil(1.0 / float(resolution)))
    P = int(math.floor(12 * bps * math.log2(float(fmax) / float(fmin)))) + 1
    W = (int(round(float(max_transition_rate) * 12 * hop / float(sr))) * bps) // 2
    return bps, P, W, max(1, int(math.floor(float(sr) / float(fmax)))), int(math.ceil(float(sr) / float(fmin)))


def pyin(x, sr: float, fmin: float, fmax: float, frame_length: int = 2048, hop_length: int | None = None, n_thresholds: int = 100, beta_parameters=(2, 18),
         boltzmann_parameter: float = 2, resolution: float = 0.1, max_transition_rate: float = 35.92, switch_prob: float = 0.01, no_trough_prob: float = 0.01,
         fill_na=float("nan"), center: bool = True):
    """Probabilistic YIN on the GPU (librosa.pyin): x [..., L] (numpy array or float32 CUDA tensor) -> (f0 float32 [..., frames], voiced_flag
    bool [..., frames], voiced_prob float32 [..., frames]); numpy arrays for numpy input.  The framing is yin's; the d' plane of yin_launch
    goes through pyin_observe_launch and pyin_decode_launch, and nothing returns to the host between the audio and the states.  The
    geometry is librosa's (pyin_geometry): bins_per_semitone = ceil(1 / resolution), n_bins = floor(12 bps log2(fmax / fmin)) + 1, the pitch
    transition is a triangle of round(max_transition_rate * 12 * hop / sr) * bps + 1 points without zero ends (half-width 50 at the
    defaults), the initial distribution is unvoiced and uniform.  f0
    of an unvoiced frame is fill_na (None: the frequency of the decoded bin).  The differences from librosa are listed in
    include/jsgx.h section 5; agreement with it has not been measured."""
    import math
    import torch
    frame_length = int(frame_length)
    hop = frame_length // 4 if hop_length is None else int(hop_length)
    bps, P, W, tau_min, tau_max = pyin_geometry(sr, fmin, fmax, frame_length, hop, resolution, max_transition_rate)
    if P < 1 or P > capix.PYIN_MAX_BINS:
        raise JsgError(capix.JSGX_ERR_INVALID, f"pyin: {P} pitch bins between fmin and fmax at this resolution; 1..{capix.PYIN_MAX_BINS} are served")
    if W > capix.PYIN_MAX_BAND_HALF:
        raise JsgError(capix.JSGX_ERR_INVALID, f"pyin: a pitch transition of half-width {W} bins; at most {capix.PYIN_MAX_BAND_HALF} are served")
    if tau_max > capix.PYIN_MAX_LAG:
        raise JsgError(capix.JSGX_ERR_INVALID, f"pyin: tau_max {tau_max} (= ceil(sr / fmin)); at most {capix.PYIN_MAX_LAG} is served")
    window = np.concatenate([np.arange(1, W + 2), np.arange(W, 0, -1)]).astype(np.float64)        # a triangle of 2W + 1 points without zero ends
    tables = pyin_tables(sr, fmin, P, bps, W, window, tau_min, tau_max, n_thresholds, beta_parameters, boltzmann_parameter, switch_prob)
    plane, _, batch, was_numpy = _yin_rows(x, sr, fmin, fmax, frame_length, hop, 0.1, center, True)
    R, T = plane.shape[0], plane.shape[1]
    dev = plane.device
    with torch.cuda.device(_device_index(plane)):
        d = {k: torch.from_numpy(v).to(dev) for k, v in tables.items()}
        emit = torch.empty((R, T, 2 * P), dtype=torch.float32, device=dev)
        voiced_prob = torch.empty((R, T), dtype=torch.float32, device=dev)
        states = torch.empty((R, T), dtype=torch.int32, device=dev)
        pyin_observe_launch(plane, tau_min, tau_max, d["prior"], d["decay"], d["norm"], d["edges"], emit, no_trough_prob=no_trough_prob, d_voiced_prob=voiced_prob)
        pyin_decode_launch(emit, d["log_init"], d["log_window"], d["src_offset"], d["log_switch"], states)
        voiced_flag = states < P
        f0 = d["freqs"][(states % P).long()]
        if fill_na is not None:
            f0 = torch.where(voiced_flag, f0, torch.full_like(f0, float(fill_na)))
    f0, voiced_flag, voiced_prob = (v.reshape(*batch, -1) for v in (f0, voiced_flag, voiced_prob))
    return (f0.cpu().numpy(), voiced_flag.cpu().numpy(), voiced_prob.cpu().numpy()) if was_numpy else (f0, voiced_flag, voiced_prob)


# --------------------------------------------------------------------------------------------------
# k nearest frames, recurrence planes and neighbour aggregation (include/jsgx.h, sections 6 to 8: libjsgx.so)
# --------------------------------------------------------------------------------------------------
_REC_MODES = {"connectivity": capix.REC_CONNECTIVITY, "distance": capix.REC_DISTANCE, "affinity": capix.REC_AFFINITY}


def _knn_args(d_x, d_y, d_index, d_dist, width, metric, split) -> capix.KnnArgs:
    import torch
    ix, ds = _planes(d_index, "d_index", torch.int32), _planes(d_dist, "d_dist")
    P, N, k = ix.shape
    x, y = _planes(d_x, "d_x"), _planes(d_y, "d_y")
    K, M = x.shape[2], y.shape[1]
    assert tuple(ds.shape) == (P, N, k) and x.shape[1] == N and y.shape[2] == K and x.shape[0] in (1, P) and y.shape[0] in (1, P), \
        "d_x [pairs or 1][n][features], d_y [pairs or 1][m][features], d_index int32 and d_dist float32 [pairs][n][k]"
    return capix.KnnArgs(x.data_ptr(), x.stride(1), _pair_pitch(x), y.data_ptr(), y.stride(1), _pair_pitch(y), P, K, N, M, _named(_METRICS, metric, "metric"),
                         k, int(width), int(split), ix.data_ptr(), ix.stride(1), ix.stride(0), ds.data_ptr(), ds.stride(1), ds.stride(0))


def knn_scratch_bytes(d_x, d_y, d_index, d_dist, *, width: int = 0, metric: str = "euclidean", split: int = 0) -> int:
    """jsgx_knn_scratch_bytes: the bytes of scratch knn_launch needs for these arguments (0 where one workgroup sweeps all columns of a strip)."""
    a = _knn_args(d_x, d_y, d_index, d_dist, width, metric, split)
    return int(capix.check(capix.lib().jsgx_knn_scratch_bytes(C.byref(a))))


def knn_launch(d_x, d_y, d_index, d_dist, *, width: int = 0, metric: str = "euclidean", split: int = 0, d_scratch=None, stream: int | None = None):
    """jsgx_knn_launch: d_x float32 [n][features] or [pairs][n][features], d_y likewise with m frames (a 2-D tensor or a leading 1 is one
    sequence shared by every pair) -> d_index int32 and d_dist float32 [n][k] or [pairs][n][k]: for every frame of x the k frames j of y
    with |i - j| >= width and the lowest cost, ascending by (cost, j); -1 and +inf behind the last candidate.  k is the last axis of the
    outputs, 1..256.  split: 0 (automatic) or the workgroups 1..16 that share the columns of a strip; the result does not depend on it.
    Enqueue only."""
    import torch
    a = _knn_args(d_x, d_y, d_index, d_dist, width, metric, split)
    d_scratch, stream = _scratch_and_stream(d_scratch, stream, d_index, lambda: max(1, capix.check(capix.lib().jsgx_knn_scratch_bytes(C.byref(a))) // 4), torch.int32,
                                            any_dtype=True)
    capix.check(capix.lib().jsgx_knn_launch(C.byref(a), d_scratch.data_ptr(), d_scratch.numel() * d_scratch.element_size(), stream))


def knn_plan(n: int, m: int, n_features: int, k: int, pairs: int = 1, metric: str = "euclidean", split: int = 0, n_cu: int = 256):
    """jsgx_knn_plan: (kernel name, rows of a strip, workgroups per strip S, lanes per workgroup, bytes of LDS per workgroup) for this
    shape on a device of n_cu compute units.  Needs no device."""
    a = capix.KnnArgs(*_plan_xy(n, m, n_features), int(pairs), int(n_features), int(n), int(m), _named(_METRICS, metric, "metric"), int(k), 0, int(split),
                      3 << 44, int(k), int(n) * int(k), 4 << 44, int(k), int(n) * int(k))      # never dereferenced
    name, out = C.create_string_buffer(32), [C.c_int32() for _ in range(4)]
    capix.check(capix.lib().jsgx_knn_plan(C.byref(a), int(n_cu), name, 32, *[C.byref(o) for o in out]))
    return (name.value.decode(),) + tuple(o.value for o in out)


def knn_default_k(n: int, width: int = 0) -> int:
    """librosa's default number of neighbours, 2 * ceil(sqrt(n - 2 * width + 1)), clamped to 1..256 (the clamp is a difference: librosa
    has no upper limit, and none below either where the root is of a number below 1)."""
    import math
    t = int(n) - 2 * int(width) + 1
    root = 0 if t <= 0 else math.isqrt(t - 1) + 1      # ceil(sqrt(t)), exactly
    return max(1, min(capix.KNN_MAX_K, 2 * root))


def knn(x, y=None, k=None, *, width: int = 0, metric: str = "euclidean", split: int = 0):
    """The k nearest frames: x [N, K] and y [M, K] (numpy arrays or float32 CUDA tensors, frame-major; a leading axis of P pairs on either
    or both; y None: x itself) -> (index int32, dist float32) as CUDA tensors [N, k] or [P, N, k].  Row i holds the k frames j of y with
    |i - j| >= width and the lowest cost under `metric`, ascending by (cost, j), and their costs; -1 and +inf behind the last candidate.
    k None: knn_default_k(M, width).  Every operation is as include/jsgx.h section 6 states it."""
    import torch
    x, _ = _to_cuda(x)
    y = x if y is None else _to_cuda(y)[0]
    assert x.dim() in (2, 3) and y.dim() in (2, 3), "knn: x [N, K] or [P, N, K], y [M, K] or [P, M, K]"
    x, y = x.contiguous(), y.contiguous()
    batched = x.dim() == 3 or y.dim() == 3
    P = max(x.shape[0] if x.dim() == 3 else 1, y.shape[0] if y.dim() == 3 else 1)
    k = knn_default_k(y.shape[-2], width) if k is None else int(k)
    shape = ((P,) if batched else ()) + (x.shape[-2], max(k, 1))
    index = torch.empty(shape, dtype=torch.int32, device=x.device)
    dist = torch.empty(shape, dtype=torch.float32, device=x.device)
    if k < 1:
        raise JsgError(capix.JSGX_ERR_INVALID, "knn: k must be in 1..256")
    with torch.cuda.device(_device_index(x)):
        knn_launch(x, y, index, dist, width=width, metric=metric, split=split)
    return index, dist


def recurrence_launch(d_index, d_dist, d_out, *, mode: str = "connectivity", sym: bool = False, diag: bool = False, d_bandwidth=None, stream: int | None = None):
    """jsgx_recurrence_launch: the lists d_index int32 and d_dist float32 [n][k] or [pairs][n][k] (d_dist may be None in connectivity mode)
    -> d_out float32 [n][m] or [pairs][n][m], every element written: the value of a link where j is in the list of i (with sym: and i in
    the list of j; n == m), +0 elsewhere.  mode "connectivity": 1; "distance": the list's distance; "affinity": exp(-d / bw) with
    bw = d_bandwidth float32 [pairs] read on the device (NaN where bw is not > 0).  diag: the main diagonal is 1 (distance mode: 0).
    Query-major: row i holds the neighbours of frame i (librosa documents the transpose).  Enqueue only."""
    import torch
    ix, o = _planes(d_index, "d_index", torch.int32), _planes(d_out, "d_out")
    P, N, k = ix.shape
    M = o.shape[2]
    assert o.shape[0] == P and o.shape[1] == N, "d_out [pairs][n][m]"
    ds = None if d_dist is None else _planes(d_dist, "d_dist")
    assert ds is None or tuple(ds.shape) == (P, N, k), "d_dist: the shape of d_index"
    bw = d_bandwidth
    assert bw is None or (bw.is_cuda and bw.dtype == torch.float32 and bw.dim() == 1 and bw.shape[0] >= P and bw.is_contiguous()), "d_bandwidth: float32 CUDA [pairs]"
    a = capix.RecurrenceArgs(ix.data_ptr(), ix.stride(1), ix.stride(0), None if ds is None else ds.data_ptr(), 0 if ds is None else ds.stride(1),
                             0 if ds is None else ds.stride(0), None if bw is None else bw.data_ptr(), P, N, M, k, _named(_REC_MODES, mode, "mode"), int(bool(sym)),
                             int(bool(diag)), 0, o.data_ptr(), o.stride(1), o.stride(0))
    capix.check(capix.lib().jsgx_recurrence_launch(C.byref(a), _stream_handle(stream, d_out)))


def _median_k_bandwidth(dist):
    """librosa's med_k_scalar bandwidth per pair, on the device and without a host synchronisation: of the finite dist[p][i][k-1] (a row
    with fewer than k candidates has +inf there and does not count), sorted ascending as v[0..c-1], bw = 0.5f * (v[(c-1)//2] + v[c//2]) in
    float32: the median, the mean of the two middle ones for an even count.  No finite entry at all: +inf."""
    import torch
    last = dist[:, :, -1]
    finite = torch.isfinite(last)
    v, _ = torch.sort(torch.where(finite, last, torch.full_like(last, float("inf"))), dim=1)
    c = finite.sum(dim=1, keepdim=True)
    lo, hi = torch.clamp((c - 1) // 2, min=0), c // 2
    hi = torch.clamp(hi, max=last.shape[1] - 1)
    return (0.5 * (torch.gather(v, 1, lo) + torch.gather(v, 1, hi)))[:, 0].contiguous()


def _recurrence(x, y, k, width, metric, sym, mode, bandwidth, diag, what):
    import torch
    index, dist = knn(x, y, k, width=width, metric=metric)
    batched = index.dim() == 3
    ix, ds = (index, dist) if batched else (index[None], dist[None])
    P, N, _ = ix.shape
    M = N if y is None else (y.shape[-2])
    bw = None
    if _named(_REC_MODES, mode, "mode") == capix.REC_AFFINITY:
        if bandwidth is None:
            bw = _median_k_bandwidth(ds)
        elif hasattr(bandwidth, "is_cuda"):
            bw = bandwidth.to(device=ix.device, dtype=torch.float32).reshape(-1).expand(P).contiguous() if bandwidth.numel() == 1 else bandwidth.to(torch.float32).contiguous()
        else:
            bw = torch.full((P,), float(bandwidth), dtype=torch.float32, device=ix.device)
    out = torch.empty((P, N, M), dtype=torch.float32, device=ix.device)
    with torch.cuda.device(_device_index(ix)):
        recurrence_launch(ix, ds, out, mode=mode, sym=sym, diag=diag, d_bandwidth=bw)
    return out if batched else out[0]


def recurrence_matrix(data, k=None, width: int = 1, metric: str = "euclidean", sym: bool = False, mode: str = "connectivity", bandwidth=None, self: bool = False):
    """librosa.segment.recurrence_matrix on the GPU: data [N, K] or [P, N, K] (frame-major; numpy array or float32 CUDA tensor) -> a
    float32 CUDA tensor [N, N] or [P, N, N].  rec[i, j] is non-zero where j is one of the k nearest frames of i outside |i - j| < width
    (sym: and i one of j's): 1 ("connectivity"), the distance ("distance") or exp(-distance / bandwidth) ("affinity").  k None:
    knn_default_k(N, width).  bandwidth None: librosa's med_k_scalar, the median over the frames of the distance to the k-th neighbour,
    computed with torch on the device without a host synchronisation (of the finite dist[i][k-1] sorted ascending, c of them,
    0.5f * (v[(c-1)//2] + v[c//2])); a number or a float32 CUDA tensor [P] is taken as given.  self: the main diagonal is set (1; 0 in
    distance mode).  Differences from librosa: query-major (librosa returns the transpose unless sym), a dense float32 plane, ties to the
    lower frame, k at most 256; include/jsgx.h sections 6 and 7 state every operation.  Agreement with librosa has not been measured."""
    x, _ = _to_cuda(data)
    return _recurrence(x, None, k, width, metric, sym, mode, bandwidth, self, "recurrence_matrix")


def cross_similarity(data, data_ref, k=None, metric: str = "euclidean", mode: str = "connectivity", bandwidth=None):
    """librosa.segment.cross_similarity on the GPU: data [N, K] and data_ref [M, K] (a leading axis of P pairs on either or both) -> a
    float32 CUDA tensor [N, M] or [P, N, M]: row i marks the k frames of data_ref nearest to frame i of data (query-major; librosa
    returns the transpose).  k None: librosa's min(M, 2 * ceil(sqrt(M))), clamped to 256.  mode and bandwidth as recurrence_matrix."""
    import math
    x, _ = _to_cuda(data)
    y, _ = _to_cuda(data_ref)
    M = y.shape[-2]
    if k is None:
        k = max(1, min(M, 2 * (math.isqrt(M - 1) + 1 if M > 0 else 0), capix.KNN_MAX_K))
    return _recurrence(x, y, k, 0, metric, False, mode, bandwidth, False, "cross_similarity")


def nn_filter_launch(d_s, d_index, d_out, *, d_weights=None, stream: int | None = None):
    """jsgx_nn_filter_launch: d_s float32 [n][features] or [pairs][n][features] and the lists d_index int32 [n][k] or [pairs][n][k] ->
    d_out, the shape of d_s: every frame replaced by the mean of its neighbours, or with d_weights float32 (the shape of d_index) by
    their weighted mean; a frame without neighbours (or with a zero weight sum) keeps its own values.  Enqueue only."""
    import torch
    s, o, ix = _planes(d_s, "d_s"), _planes(d_out, "d_out"), _planes(d_index, "d_index", torch.int32)
    P, N, F = s.shape
    k = ix.shape[2]
    assert tuple(o.shape) == (P, N, F) and ix.shape[0] == P and ix.shape[1] == N, "d_out: the shape of d_s; d_index [pairs][n][k]"
    w = None if d_weights is None else _planes(d_weights, "d_weights")
    assert w is None or tuple(w.shape) == (P, N, k), "d_weights: the shape of d_index"
    a = capix.NnFilterArgs(s.data_ptr(), s.stride(1), s.stride(0), ix.data_ptr(), ix.stride(1), ix.stride(0), None if w is None else w.data_ptr(),
                           0 if w is None else w.stride(1), 0 if w is None else w.stride(0), P, N, F, k, o.data_ptr(), o.stride(1), o.stride(0))
    capix.check(capix.lib().jsgx_nn_filter_launch(C.byref(a), _stream_handle(stream, d_out)))


def nn_filter(S, index, weights=None):
    """librosa.decompose.nn_filter with aggregate = mean (weights None) or a weighted mean, on the GPU: S [N, F] or [P, N, F] (frame-major;
    numpy array or float32 CUDA tensor), index int32 [N, k] or [P, N, k] (what knn returns; -1 marks no neighbour) -> a float32 CUDA
    tensor of the shape of S.  A frame without neighbours keeps its own values.  The median aggregate, librosa's default, is not served."""
    import torch
    s, _ = _to_cuda(S)
    s = s.contiguous()
    ix = index if hasattr(index, "is_cuda") else torch.from_numpy(np.ascontiguousarray(index, dtype=np.int32)).to(s.device)
    w = None if weights is None else _to_cuda(weights)[0].contiguous()
    out = torch.empty_like(s)
    with torch.cuda.device(_device_index(s)):
        nn_filter_launch(s, ix.contiguous(), out, d_weights=w)
    return out


# --------------------------------------------------------------------------------------------------
# cepstral coefficients and delta features (include/jsg.h, section 2k)
# --------------------------------------------------------------------------------------------------
_NORMS = {"ortho": capi.DCT_NORM_ORTHO, None: capi.DCT_NORM_NONE, "none": capi.DCT_NORM_NONE}
_EDGES = {"interp": capi.DELTA_EDGE_INTERP, "nearest": capi.DELTA_EDGE_NEAREST}
_cepstral_cache: dict = {}


def _named(table: dict, key, what: str) -> int:
    if key not in table:
        raise JsgError(capi.JSG_ERR_INVALID, f"{what} must be one of {sorted(k for k in table if k is not None)}, not {key!r}")
    return table[key]


def mfcc_table(n_bands: int, n_coeffs: int = 20, norm="ortho", lifter: float = 0.0, inverse: bool = False) -> np.ndarray:
    """jsg_mfcc_table_build: the DCT-II table of scipy.fft.dct(type=2, norm=norm) with the lifter of librosa.feature.mfcc folded in,
    float32 [n_coeffs][n_bands]; inverse: the zero-padded inverse of scipy.fft.idct(type=2, n=n_bands) with the lifter divided out,
    float32 [n_bands][n_coeffs] (the table of a launch from n_coeffs to n_bands values per frame).  Built in double, rounded once."""
    B, M = int(n_bands), int(n_coeffs)
    out = np.zeros((B, M) if inverse else (M, B), dtype=np.float32)
    check(lib().jsg_mfcc_table_build(B, M, _named(_NORMS, norm, "norm"), float(lifter), int(bool(inverse)), out.ctypes.data if out.size else None))
    return out


def _mfcc_args(d_S, d_table, d_out, chunk_frames) -> capi.MfccArgs:
    import torch
    s = _plane(d_S, "d_S")
    R, T, B = s.shape
    assert d_table.is_cuda and d_table.dtype == torch.float32 and d_table.dim() == 2 and d_table.is_contiguous() and d_table.shape[1] == B, \
        "d_table: contiguous float32 CUDA [n_out][n_in]"
    M = d_table.shape[0]
    o = _plane(d_out, "d_out")
    assert o.shape[0] == R and o.shape[1] >= T and o.shape[2] >= M, "d_out: float32 CUDA [rows][>= frames][>= n_out]"
    return capi.MfccArgs(s.data_ptr(), s.stride(1), s.stride(0), R, B, T, d_table.data_ptr(), M, o.data_ptr(), o.stride(1), o.stride(0), int(chunk_frames))


def mfcc_launch(d_S, d_table, d_out, *, chunk_frames: int = 0, stream: int | None = None):
    """jsg_mfcc_launch: d_S float32 [rows][frames][n_in] (or one [frames][n_in] plane; views with pitches), d_table float32
    [n_out][n_in] -> d_out float32 [rows][frames][>= n_out]: out[t][m] = sum over b ascending of fmaf(table[m][b], S[t][b], acc).
    Applies any dense table: mfcc_table(...) gives MFCCs, mfcc_table(..., inverse=True) takes them back to the mel dB plane.
    chunk_frames (0: the library's choice) never changes the result."""
    a = _mfcc_args(d_S, d_table, d_out, chunk_frames)
    check(lib().jsg_mfcc_launch(C.byref(a), _stream_handle(stream, d_S)))


def mfcc_kernel_name(d_S, d_table, d_out, *, chunk_frames: int = 0) -> str:
    """The path mfcc_launch takes for these arguments: "mfcc_block4", "mfcc_block5", "mfcc_block8", "mfcc_block10" or "mfcc_block16"."""
    a = _mfcc_args(d_S, d_table, d_out, chunk_frames)
    return _kernel_name(lib().jsg_mfcc_kernel_name, C.byref(a))


def mfcc_plan(d_S, d_table, d_out, *, chunk_frames: int = 0):
    """jsg_mfcc_plan: (path, frames per work item, bytes of LDS per workgroup) of mfcc_launch for these arguments.  Needs no device."""
    a = _mfcc_args(d_S, d_table, d_out, chunk_frames)
    name, frames, lds = C.create_string_buffer(32), C.c_int32(), C.c_int32()
    check(lib().jsg_mfcc_plan(C.byref(a), name, 32, C.byref(frames), C.byref(lds)))
    return name.value.decode(), frames.value, lds.value


def delta_weights(width: int = 9, order: int = 1) -> np.ndarray:
    """jsg_delta_weights_build: the Savitzky-Golay weights of the order-th derivative of a degree-order fit over `width` frames
    (scipy.signal.savgol_filter(deriv=order, polyorder=order), what librosa.feature.delta uses), float32 [width], to be applied as
    sum over j of w[j] * X[first frame of the window + j]."""
    out = np.zeros(max(int(width), 1), dtype=np.float32)
    check(lib().jsg_delta_weights_build(int(width), int(order), out.ctypes.data))
    return out[:int(width)]


def delta_launch(d_X, d_weights, d_out, *, mode: str = "interp", stream: int | None = None):
    """jsg_delta_launch: d_X float32 [rows][frames][n_coeffs] (or one plane; views with pitches), d_weights float32 [width] -> d_out
    float32 [rows][frames][>= n_coeffs]: the weighted sum over a window of `width` frames around every frame, j ascending.  mode
    "interp": the window is shifted to stay inside the row (needs frames >= width); "nearest": frames outside repeat the edge."""
    import torch
    x = _plane(d_X, "d_X")
    R, T, M = x.shape
    assert d_weights.is_cuda and d_weights.dtype == torch.float32 and d_weights.dim() == 1 and d_weights.stride(0) == 1, "d_weights: float32 CUDA [width]"
    o = _plane(d_out, "d_out")
    assert o.shape[0] == R and o.shape[1] >= T and o.shape[2] >= M, "d_out: float32 CUDA [rows][>= frames][>= n_coeffs]"
    a = capi.DeltaArgs(x.data_ptr(), x.stride(1), x.stride(0), R, M, T, d_weights.data_ptr(), d_weights.shape[0], _named(_EDGES, mode, "mode"),
                       o.data_ptr(), o.stride(1), o.stride(0))
    check(lib().jsg_delta_launch(C.byref(a), _stream_handle(stream, x)))


def _cepstral_table(device, key, build):
    """A host-built table on `device`, cached per (device, geometry) like _mel_cache."""
    import torch
    key = (_device_index(torch.empty(0, device=device)),) + key
    if key not in _cepstral_cache:
        _cepstral_cache[key] = torch.from_numpy(build()).to(device)
    return _cepstral_cache[key]


def _project(S, table_of):
    import torch
    s, was_numpy = _to_cuda(S)
    assert s.dim() >= 2, "expected [..., frames, values]"
    batch = tuple(s.shape[:-2])
    sr = s.reshape(-1, s.shape[-2], s.shape[-1])
    sr = sr if sr.stride(2) == 1 else sr.contiguous()
    table = table_of(s.device, sr.shape[2])
    out = torch.empty((sr.shape[0], sr.shape[1], table.shape[0]), dtype=torch.float32, device=s.device)
    with torch.cuda.device(_device_index(s)):
        mfcc_launch(sr, table, out)
    out = out.reshape(*batch, sr.shape[1], table.shape[0])
    return out.cpu().numpy() if was_numpy else out


def mfcc(S, n_mfcc: int = 20, norm="ortho", lifter: float = 0.0):
    """MFCCs of a log-mel plane S [..., frames, bands] (numpy array or float32 CUDA tensor; what mel_spectrogram_db returns) -> float32
    [..., frames, n_mfcc], the same kind: the DCT-II (scipy.fft.dct type 2, norm) over the bands, first n_mfcc coefficients, times the
    lifter of librosa.feature.mfcc.  Differs from librosa.feature.mfcc on purpose: the frames lie along axis -2 and the coefficients
    along the last axis, and the lifter is folded into the table before its one rounding to float32.  Agreement with librosa was not
    measured."""
    M = int(n_mfcc)
    return _project(S, lambda dev, B: _cepstral_table(dev, ("dct", B, M, norm, float(lifter)), lambda: mfcc_table(B, M, norm, lifter)))


def mfcc_to_mel_db(C, n_mels: int = 128, norm="ortho", lifter: float = 0.0):
    """The log-mel plane of MFCCs C [..., frames, n_mfcc] (numpy array or float32 CUDA tensor) -> float32 [..., frames, n_mels], the
    same kind: the lifter divided out and the zero-padded inverse DCT (scipy.fft.idct type 2, n = n_mels), the first step of
    librosa.feature.inverse.mfcc_to_mel (which goes on to power; this stays in dB).  Frames along axis -2; agreement with librosa was
    not measured."""
    B = int(n_mels)
    return _project(C, lambda dev, M: _cepstral_table(dev, ("idct", B, M, norm, float(lifter)), lambda: mfcc_table(B, M, norm, lifter, inverse=True)))


def delta(X, width: int = 9, order: int = 1, mode: str = "interp"):
    """Delta features of X [..., frames, coefficients] (numpy array or float32 CUDA tensor) -> float32 of the same shape and kind: the
    order-th Savitzky-Golay derivative along the frames over `width` frames (librosa.feature.delta: savgol_filter with polyorder =
    deriv = order).  mode "interp" needs frames >= width; "nearest" repeats the edge frames.  Differs from librosa.feature.delta on
    purpose: the frames lie along axis -2.  Agreement with librosa was not measured."""
    import torch
    x, was_numpy = _to_cuda(X)
    assert x.dim() >= 2, "expected [..., frames, coefficients]"
    xr = x.reshape(-1, x.shape[-2], x.shape[-1])
    xr = xr if xr.stride(2) == 1 else xr.contiguous()
    w = _cepstral_table(x.device, ("delta", int(width), int(order)), lambda: delta_weights(width, order))
    out = torch.empty(xr.shape, dtype=torch.float32, device=x.device)
    with torch.cuda.device(_device_index(x)):
        delta_launch(xr, w, out, mode=mode)
    out = out.reshape(x.shape)
    return out.cpu().numpy() if was_numpy else out


def mfcc_audio(x, sr: float, n_mfcc: int = 20, n_fft: int = 2048, hop: int = 512, n_mels: int = 128, fmin: float = 0.0, fmax: float | None = None,
               lifter: float = 0.0):
    """MFCCs of audio x [samples] (numpy array or float32 CUDA tensor): mel_spectrogram_db -> mfcc (orthonormal DCT), on the GPU with
    nothing returned to the host in between -> float32 [frames, n_mfcc], the same kind.  Differs from librosa.feature.mfcc on purpose:
    the mel dB plane is 10 log10(power + 1e-11) without top_db clipping, the frames start at t * hop (no centring), they lie along axis
    -2, and the lifter is folded into the table.  Agreement with librosa was not measured."""
    import torch
    xt, was_numpy = _to_cuda(x)
    assert xt.dim() == 1, "mfcc_audio: x is one channel [samples]"
    with torch.cuda.device(_device_index(xt)):
        out = mfcc(mel_spectrogram_db(xt, sr, n_fft, hop, n_mels, fmin, fmax), n_mfcc, "ortho", lifter)
    return out.cpu().numpy() if was_numpy else out


# --------------------------------------------------------------------------------------------------
# spectral shape descriptors (include/jsg.h, section 2l)
# --------------------------------------------------------------------------------------------------
_SHAPE_OUTPUTS = ("energy", "centroid", "spread", "rolloff", "rolloff_bin", "flatness_db", "crest")
_shape_plan_cache: dict = {}


def _spectral_args(d_S, d_freqs, outs: dict, roll_percent: float) -> capi.SpectralArgs:
    import torch
    s = _plane(d_S, "d_S")
    R, T, K = s.shape
    assert d_freqs.is_cuda and d_freqs.dtype == torch.float32 and d_freqs.dim() == 1 and d_freqs.stride(0) == 1 and d_freqs.shape[0] >= K, \
        "d_freqs: float32 CUDA [>= bins]"
    ptrs, pitch = {}, None
    for name in _SHAPE_OUTPUTS:
        o = outs.get(name)
        if o is None:
            ptrs[name] = None
            continue
        o = o[None] if o.dim() == 1 else o
        want = torch.int32 if name == "rolloff_bin" else torch.float32
        assert o.is_cuda and o.dtype == want and o.dim() == 2 and o.stride(1) == 1 and o.shape[0] == R and o.shape[1] >= T, \
            f"d_{name}: {'int32' if name == 'rolloff_bin' else 'float32'} CUDA [rows][>= frames]"
        assert R == 1 or pitch is None or pitch == o.stride(0), "the outputs share one row pitch"
        pitch = o.stride(0)
        ptrs[name] = o.data_ptr()
    return capi.SpectralArgs(s.data_ptr(), s.stride(1), s.stride(0), R, K, T, d_freqs.data_ptr(), float(roll_percent), 0, ptrs["energy"], ptrs["centroid"],
                             ptrs["spread"], ptrs["rolloff"], ptrs["rolloff_bin"], ptrs["flatness_db"], ptrs["crest"], pitch or 0)


def spectral_shape_launch(d_S, d_freqs, *, d_energy=None, d_centroid=None, d_spread=None, d_rolloff=None, d_rolloff_bin=None, d_flatness_db=None,
                          d_crest=None, roll_percent: float = 0.85, stream: int | None = None):
    """jsg_spectral_shape_launch: d_S float32 [rows][frames][bins] (or one [frames][bins] plane; views with pitches), non-negative, and
    d_freqs float32 [bins] -> per frame, each output float32 [rows][>= frames] (d_rolloff_bin: int32) or None, with one shared row pitch:
    the energy (sum over the bins), the centroid (sum f S / sum S), the spread (sqrt of sum (f - centroid)^2 S / sum S), the rolloff (f at
    the first bin whose prefix sum reaches roll_percent of the total) and its bin, flatness_db (10 log10 of geometric over arithmetic
    mean, 1e-11 inside each logarithm) and the crest (largest bin over the mean).  One kernel that reads the plane once; an output that
    is None does not cost its separable work.  The summation orders are those of include/jsg.h section 2l."""
    outs = dict(energy=d_energy, centroid=d_centroid, spread=d_spread, rolloff=d_rolloff, rolloff_bin=d_rolloff_bin, flatness_db=d_flatness_db, crest=d_crest)
    a = _spectral_args(d_S, d_freqs, outs, roll_percent)
    check(lib().jsg_spectral_shape_launch(C.byref(a), _stream_handle(stream, d_S)))


def spectral_shape_kernel_name(d_S, d_freqs, *, roll_percent: float = 0.85, **outs) -> str:
    """The path spectral_shape_launch takes for these arguments (d_energy= ... as there): "spectral_regs1" ... "spectral_regs65" (a
    lane keeps its share of a frame in registers between the passes) or "spectral_stream", by the number of bins alone."""
    a = _spectral_args(d_S, d_freqs, {k[2:]: v for k, v in outs.items()}, roll_percent)
    return _kernel_name(lib().jsg_spectral_shape_kernel_name, C.byref(a))


def spectral_shape_plan(d_S, d_freqs, *, roll_percent: float = 0.85, **outs):
    """jsg_spectral_shape_plan: (path, lanes per frame, frames a group of lanes has in flight, bytes of LDS per workgroup) of
    spectral_shape_launch for these arguments (d_energy= ... as there).  A workgroup takes frames * 256 / lanes consecutive frames per
    step.  Needs no device."""
    a = _spectral_args(d_S, d_freqs, {k[2:]: v for k, v in outs.items()}, roll_percent)
    name, lanes, frames, lds = C.create_string_buffer(32), C.c_int32(), C.c_int32(), C.c_int32()
    check(lib().jsg_spectral_shape_plan(C.byref(a), name, 32, C.byref(lanes), C.byref(frames), C.byref(lds)))
    return name.value.decode(), lanes.value, frames.value, lds.value


def fft_frequencies(sr: float, n_fft: int) -> np.ndarray:
    """The centre frequencies k * sr / n_fft of the n_fft / 2 + 1 bins of an n_fft-point transform (librosa.fft_frequencies), computed
    in double and rounded to float32 once."""
    n = int(n_fft)
    return (np.arange(n // 2 + 1, dtype=np.float64) * float(sr) / n).astype(np.float32)


def _shape_freqs(s, freqs, sr):
    """The frequency table of a plane s [..., frames, bins] on its device: `freqs` (any array of bins floats), else the FFT bins of sr."""
    import torch
    K = s.shape[-1]
    if freqs is None:
        if sr is None:
            raise JsgError(capi.JSG_ERR_INVALID, "spectral_shape: give freqs (one frequency per bin) or sr (the plane is then taken as FFT bins)")
        return _cepstral_table(s.device, ("fft_frequencies", float(sr), 2 * (K - 1)), lambda: fft_frequencies(sr, 2 * (K - 1)) if K > 1 else np.zeros(1, np.float32))
    f = freqs if hasattr(freqs, "is_cuda") else torch.from_numpy(np.ascontiguousarray(freqs, dtype=np.float32))
    f = f.to(device=s.device, dtype=torch.float32).contiguous()
    assert f.dim() == 1 and f.shape[0] == K, "freqs: one frequency per bin"
    return f


def _shape(S, freqs, sr, roll_percent, names):
    """The outputs `names` of one launch over S [..., frames, bins]: a dict of [..., frames] arrays of the kind of S."""
    import torch
    s, was_numpy = _to_cuda(S)
    assert s.dim() >= 2, "expected [..., frames, bins]"
    batch = tuple(s.shape[:-2])
    sr3 = s.reshape(-1, s.shape[-2], s.shape[-1])
    sr3 = sr3 if sr3.stride(2) == 1 else sr3.contiguous()
    f = _shape_freqs(s, freqs, sr)
    outs = {n: torch.empty((sr3.shape[0], sr3.shape[1]), dtype=torch.int32 if n == "rolloff_bin" else torch.float32, device=s.device) for n in names}
    with torch.cuda.device(_device_index(s)):
        spectral_shape_launch(sr3, f, roll_percent=roll_percent, **{"d_" + n: o for n, o in outs.items()})
    outs = {n: o.reshape(*batch, sr3.shape[1]) for n, o in outs.items()}
    if "flatness_db" in outs:
        outs["flatness"] = torch.pow(10.0, outs["flatness_db"] / 10.0)
    return {n: (o.cpu().numpy() if was_numpy else o) for n, o in outs.items()}


def spectral_shape(S, freqs=None, sr=None, roll_percent: float = 0.85):
    """The spectral shape descriptors of every frame of S [..., frames, bins] (numpy array or float32 CUDA tensor, non-negative: the power
    plane of stft_db(..., linear_out=True), a mel plane, a cqt(..., power=True) plane) in one launch -> a dict of [..., frames] arrays
    of the same kind: energy, centroid, spread, rolloff, rolloff_bin (int32), flatness_db, crest, and flatness = 10^(flatness_db / 10).
    freqs: one frequency per bin (mel or CQT centres, anything); None: fft_frequencies(sr, 2 * (bins - 1)).  Differs from
    librosa.feature.spectral_centroid / spectral_bandwidth / spectral_rolloff / spectral_flatness on purpose: the plane is taken as it is,
    and it is power by default here where librosa's default is magnitude; the frames lie along axis -2; the floor inside the logarithms is
    1e-11 where librosa uses amin = 1e-10; no centring of frames.  Agreement with librosa was not measured."""
    return _shape(S, freqs, sr, roll_percent, _SHAPE_OUTPUTS)


def spectral_centroid(S, freqs=None, sr=None):
    """The centroid sum f S / sum S of every frame of S [..., frames, bins] -> [..., frames], the same kind; a launch with this output
    alone, the same bits as spectral_shape(...)["centroid"].  As there: power rather than magnitude as the plane's default, frames along
    axis -2, no centring, where librosa.feature.spectral_centroid differs; agreement with librosa was not measured."""
    return _shape(S, freqs, sr, 0.85, ("centroid",))["centroid"]


def spectral_bandwidth(S, freqs=None, sr=None):
    """The spread sqrt(sum (f - centroid)^2 S / sum S) of every frame of S [..., frames, bins] -> [..., frames], the same kind
    (librosa.feature.spectral_bandwidth with p = 2 and S as the weights); a launch with this output alone, the same bits as
    spectral_shape(...)["spread"].  Power rather than magnitude as the plane's default, frames along axis -2, no centring; agreement with
    librosa was not measured."""
    return _shape(S, freqs, sr, 0.85, ("spread",))["spread"]


def spectral_rolloff(S, freqs=None, sr=None, roll_percent: float = 0.85):
    """The frequency of the first bin of every frame of S [..., frames, bins] whose prefix sum reaches roll_percent of the frame's total
    -> [..., frames], the same kind; a launch with this output alone, the same bits as spectral_shape(...)["rolloff"].  Power rather than
    magnitude as the plane's default, frames along axis -2, no centring, where librosa.feature.spectral_rolloff differs; agreement with
    librosa was not measured."""
    return _shape(S, freqs, sr, roll_percent, ("rolloff",))["rolloff"]


def spectral_flatness(S):
    """The flatness (geometric over arithmetic mean, linear) of every frame of S [..., frames, bins] -> [..., frames], the same kind; a
    launch with flatness_db alone, then 10^(flatness_db / 10) as in spectral_shape(...)["flatness"].  Power rather than magnitude as the
    plane's default (librosa.feature.spectral_flatness squares a magnitude itself), frames along axis -2, the floor 1e-11 inside the
    logarithms where librosa uses amin = 1e-10, no centring; agreement with librosa was not measured."""
    return _shape(S, np.zeros(S.shape[-1], np.float32), None, 0.85, ("flatness_db",))["flatness"]          # the table is not read


def spectral_crest(S):
    """The crest (largest bin over the mean of the bins) of every frame of S [..., frames, bins] -> [..., frames], the same kind; a launch
    with this output alone, the same bits as spectral_shape(...)["crest"].  librosa has no counterpart; as for the others, the plane is
    power by default, the frames lie along axis -2, there is no centring, and agreement with librosa was not measured."""
    return _shape(S, np.zeros(S.shape[-1], np.float32), None, 0.85, ("crest",))["crest"]                   # the table is not read


def spectral_shape_audio(x, sr: float, n_fft: int = 2048, hop: int = 512, roll_percent: float = 0.85):
    """The spectral shape descriptors of audio x [samples] (numpy array or float32 CUDA tensor): Plan (the library's Hann window) ->
    stft_db(..., linear_out=True) -> spectral_shape on the power plane with the FFT bin frequencies of sr, on the GPU with nothing
    returned to the host in between -> the dict of spectral_shape, [frames] each, frames = 1 + (samples - n_fft) // hop.  n_fft is one
    of the engine's sizes (512 .. 8192) and hop divides it.  Differs from librosa on purpose: power rather than magnitude as the plane,
    the frames start at t * hop (no centring) and lie along axis -2 of the plane, the floor 1e-11 inside the logarithms where librosa uses
    amin = 1e-10.  Agreement with librosa was not measured."""
    import torch
    xt, was_numpy = _to_cuda(x)
    assert xt.dim() == 1, "spectral_shape_audio: x is one channel [samples]"
    n_fft, hop = int(n_fft), int(hop)
    if hop <= 0 or hop > n_fft or n_fft % hop:
        raise JsgError(capi.JSG_ERR_INVALID, f"spectral_shape_audio: hop {hop} must divide n_fft {n_fft} (frames at t * hop)")
    frames = 1 + (xt.shape[0] - n_fft) // hop
    if frames < 1:
        raise JsgError(capi.JSG_ERR_INVALID, f"spectral_shape_audio: {xt.shape[0]} samples hold no frame of {n_fft}")
    dev = _device_index(xt)
    with torch.cuda.device(dev):
        if (dev, n_fft) not in _shape_plan_cache:
            _shape_plan_cache[(dev, n_fft)] = Plan(n_fft, window(capi.WIN_HANN, n_fft))
        power = torch.empty((frames, n_fft // 2 + 1), dtype=torch.float32, device=xt.device)
        stft_db(_shape_plan_cache[(dev, n_fft)], xt[None, :].contiguous(), hop, frames, power, feedblocks=n_fft // hop, linear_out=True)
        out = spectral_shape(power, sr=sr, roll_percent=roll_percent)
    return {n: o.cpu().numpy() for n, o in out.items()} if was_numpy else out

"""The argument blocks the Python binding hands to libjsg.so, built from stand-in tensors (no GPU): every field of every block against
the value include/jsg.h documents for it, and the refusals of the builders."""
import types

import pytest
import torch

PLAN = types.SimpleNamespace(n=1024, _p=None)      # the builders read nothing of a plan but its FFT size
BINS = PLAN.n // 2 + 1


class FakeTensor:
    """What the builders read of a torch tensor: geometry, dtype, device and address, with torch's indexing rules for t[i] and t[None]."""

    def __init__(self, shape, dtype=torch.float32, strides=None, ptr=0x7F0000001000, is_cuda=True):
        self.shape, self.dtype, self.is_cuda, self._ptr = tuple(shape), dtype, is_cuda, ptr
        self.device = torch.device("cuda", 0) if is_cuda else torch.device("cpu")
        self._strides = self._dense() if strides is None else tuple(strides)

    def _dense(self):
        out, step = [], 1
        for s in reversed(self.shape):
            out.insert(0, step)
            step *= s
        return tuple(out)

    def stride(self, i=None): return self._strides if i is None else self._strides[i]
    def dim(self): return len(self.shape)
    def data_ptr(self): return self._ptr
    def element_size(self): return self.dtype.itemsize
    def is_contiguous(self): return self._strides == self._dense()

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def __getitem__(self, i):
        if i is None:
            return FakeTensor((1,) + self.shape, self.dtype, (self.shape[0] * self._strides[0],) + self._strides, self._ptr, self.is_cuda)
        return FakeTensor(self.shape[1:], self.dtype, self._strides[1:], self._ptr + i * self._strides[0] * self.element_size(), self.is_cuda)


def fields(block) -> dict:
    return {name: getattr(block, name) for name, *_ in block._fields_}


def expect(block, **want):
    """Every field of the block: those named in `want`, zero for all the others."""
    full = dict.fromkeys(fields(block), 0)
    assert set(want) <= set(full)
    full.update(want)
    got = {k: (v or 0) for k, v in fields(block).items()}       # a null pointer reads as None
    assert got == full


D_IN = FakeTensor((2, 5000), strides=(5120, 1), ptr=0x7F0000100000)
D_OUT = FakeTensor((64, 520), ptr=0x7F0000200000)


def test_stft_args_mixed(jsg):
    S, capi = jsg.spectrogram, jsg.capi
    a = S._stft_args(PLAN, D_IN, 256, 10, D_OUT)
    base = dict(in_=D_IN.data_ptr(), in_pitch=5120, channels=2, hop=256, feedblocks=4, n_frames=10, out_db=D_OUT.data_ptr(), out_pitch=520,
                ring_width=64, in_samples=5000)
    expect(a, **base)                                                 # out_channel_pitch 0 for a two-dimensional output, out_tail NULL
    a = S._stft_args(PLAN, D_IN, 256, 10, D_OUT, feedblocks=3, mix_mode=capi.MIX_MAX, first_frame=7, ring_pos=5, linear_out=True, blocks_per_cu=2,
                     plan_select=2, exact_log=True)
    expect(a, **dict(base, feedblocks=3, mix_mode=capi.MIX_MAX, first_frame=7, ring_pos=5, linear_out=1, blocks_per_cu=2, plan_select=2, exact_log=1))
    a = S._stft_args(PLAN, D_IN, 2048, 1, D_OUT)
    expect(a, **dict(base, hop=2048, feedblocks=1, n_frames=1))        # feedblocks never falls below 1
    mono = FakeTensor((1, 5000), strides=(77, 1), ptr=0x7F0000100000)
    expect(S._stft_args(PLAN, mono, 256, 10, D_OUT), **dict(base, channels=1, in_pitch=5000))     # one channel: the row length
    padded = FakeTensor((64, 520), strides=(640, 1), ptr=0x7F0000200000)
    expect(S._stft_args(PLAN, D_IN, 256, 10, padded), **dict(base, out_pitch=640))


def test_stft_args_per_channel(jsg):
    S, capi = jsg.spectrogram, jsg.capi
    out = FakeTensor((2, 48, 520), strides=(48 * 576, 576, 1), ptr=0x7F0000300000)
    a = S._stft_args(PLAN, D_IN, 512, 6, out, mix_mode=capi.MIX_PER_CHANNEL)
    expect(a, in_=D_IN.data_ptr(), in_pitch=5120, channels=2, hop=512, feedblocks=2, mix_mode=capi.MIX_PER_CHANNEL, n_frames=6,
           out_db=out.data_ptr(), out_pitch=576, out_channel_pitch=48 * 576, ring_width=48, in_samples=5000)


def test_stft_args_tail_plane_and_column_height(jsg):
    S = jsg.spectrogram
    out = FakeTensor((64, 512), ptr=0x7F0000200000)                   # n/2 floats per column: only with the tail plane
    tail = FakeTensor((64,), ptr=0x7F0000400000)
    base = dict(in_=D_IN.data_ptr(), in_pitch=5120, channels=2, hop=256, feedblocks=4, n_frames=10, out_db=out.data_ptr(), out_pitch=512,
                ring_width=64, in_samples=5000)
    expect(S._stft_args(PLAN, D_IN, 256, 10, out, d_tail=tail), **dict(base, out_tail=tail.data_ptr()))
    with pytest.raises(jsg.JsgError) as e:
        S._stft_args(PLAN, D_IN, 256, 10, out)
    assert e.value.code == jsg.capi.JSG_ERR_INVALID and "a column needs 513" in str(e.value)
    with pytest.raises(AssertionError):
        S._stft_args(PLAN, D_IN, 256, 10, out, d_tail=FakeTensor((63,)))          # one float per ring column
    bands = FakeTensor((64, 40), ptr=0x7F0000200000)
    expect(S._stft_args(PLAN, D_IN, 256, 10, bands, col_height=40), **dict(base, out_pitch=40))
    with pytest.raises(jsg.JsgError) as e:
        S._stft_args(PLAN, D_IN, 256, 10, bands, col_height=41)
    assert e.value.code == jsg.capi.JSG_ERR_INVALID and "a column needs 41" in str(e.value)


def test_stft_args_refusals(jsg):
    S, capi = jsg.spectrogram, jsg.capi
    with pytest.raises(jsg.JsgError) as e:                                         # rows shorter than a column
        S._stft_args(PLAN, D_IN, 256, 10, FakeTensor((64, 512)))
    assert e.value.code == capi.JSG_ERR_INVALID and str(e.value).endswith("output rows hold 512 floats, a column needs 513")
    for out in (D_OUT, FakeTensor((3, 64, 520)), FakeTensor((1, 2, 64, 520))):      # per-channel output of the wrong rank or channel count
        with pytest.raises(jsg.JsgError) as e:
            S._stft_args(PLAN, D_IN, 256, 10, out, mix_mode=capi.MIX_PER_CHANNEL)
        assert e.value.code == capi.JSG_ERR_INVALID and str(e.value).endswith("per-channel mode needs an output of [channels][W][pitch]")
    for bad in (FakeTensor((2, 5000), torch.float64), FakeTensor((2, 5000), strides=(1, 2)), FakeTensor((5000,)), FakeTensor((2, 5000), is_cuda=False)):
        with pytest.raises(AssertionError):
            S._stft_args(PLAN, bad, 256, 10, D_OUT)
    for bad in (FakeTensor((64, 520), torch.float64), FakeTensor((64, 520), strides=(1, 64)), FakeTensor((64, 520), is_cuda=False)):
        with pytest.raises(AssertionError):
            S._stft_args(PLAN, D_IN, 256, 10, bad)


def test_strided_split(jsg):
    S = jsg.spectrogram
    d_in = FakeTensor((3, 2, 5000), strides=(16384, 5120, 1), ptr=0x7F0000100000)
    d_out = FakeTensor((3, 64, 520), strides=(40000, 520, 1), ptr=0x7F0000200000)
    batch0 = dict(in_=d_in.data_ptr(), in_pitch=5120, channels=2, hop=256, feedblocks=4, n_frames=10, out_db=d_out.data_ptr(), out_pitch=520,
                  ring_width=64, in_samples=5000)
    a, k, s_in, s_out = S._strided_args(PLAN, d_in, 256, 10, d_out, ring_pos=3)
    expect(a, **dict(batch0, ring_pos=3))                             # `args` describes batch 0
    assert (k, s_in, s_out) == (3, 16384, 40000)
    fb = types.SimpleNamespace(n_bands=40)                            # the filterbank calls: the same split, columns of n_bands floats
    d_bands = FakeTensor((3, 64, 40), ptr=0x7F0000200000)
    a, k, s_in, s_out = S._fb_args(PLAN, fb, d_in, 256, 10, d_bands, True)
    expect(a, **dict(batch0, out_pitch=40))
    assert (k, s_in, s_out) == (3, 16384, 64 * 40)
    a, k, s_in, s_out = S._fb_args(PLAN, fb, d_in[1], 256, 10, d_bands[1], False)
    expect(a, **dict(batch0, in_=d_in.data_ptr() + 4 * 16384, out_db=d_bands.data_ptr() + 4 * 64 * 40, out_pitch=40))
    assert (k, s_in, s_out) == (1, 0, 0)
    per_channel = FakeTensor((3, 2, 64, 520), ptr=0x7F0000200000)
    a, k, s_in, s_out = S._strided_args(PLAN, d_in, 256, 10, per_channel, mix_mode=jsg.capi.MIX_PER_CHANNEL)
    expect(a, **dict(batch0, mix_mode=jsg.capi.MIX_PER_CHANNEL, out_channel_pitch=64 * 520))
    assert (k, s_in, s_out) == (3, 16384, 2 * 64 * 520)
    with pytest.raises(AssertionError):
        S._strided_args(PLAN, d_in, 256, 10, FakeTensor((2, 64, 520)))             # one ring per batch
    with pytest.raises(AssertionError):
        S._strided_args(PLAN, d_in[0], 256, 10, d_out)


def test_colormap_args(jsg):
    S = jsg.spectrogram
    d_db = FakeTensor((64, 513), strides=(520, 1), ptr=0x7F0000200000)
    lut = FakeTensor((200,), torch.int32, ptr=0x7F0000500000)
    argb = FakeTensor((513, 100), torch.int32, strides=(128, 1), ptr=0x7F0000600000)
    index = FakeTensor((513, 90), torch.uint8, strides=(96, 1), ptr=0x7F0000700000)
    vmin, vmax, mult = (float(v) for v in jsg.colormap_range(200, -70.0, 10.0))
    assert (vmin, vmax) == (-70.0, 10.0) and mult == 200 / 80.0
    base = dict(db=d_db.data_ptr(), db_pitch=520, ring_width=64, lut=lut.data_ptr(), n_colors=200, vmin=vmin, vmax=vmax, access_mult=mult)
    a = S._colormap_args(d_db, lut, -70.0, 10.0, argb, None, 0, None, 0, None)
    expect(a, **dict(base, height=513, n_cols=64, x_wrap=100, argb_out=argb.data_ptr(), argb_pitch=128))      # defaults: the whole ring
    a = S._colormap_args(d_db, lut, -70.0, 10.0, None, index, 60, 9, 17, 257)
    expect(a, **dict(base, height=257, col_first=60, n_cols=9, x_first=17, x_wrap=90, index_out=index.data_ptr(), index_pitch=96))
    a = S._colormap_args(d_db, lut, -70.0, 10.0, argb, index, 60, 9, 17, 257)
    expect(a, **dict(base, height=257, col_first=60, n_cols=9, x_first=17, x_wrap=90, argb_out=argb.data_ptr(), argb_pitch=128,
                     index_out=index.data_ptr(), index_pitch=96))


def image_blocks(a):
    assert [name for name, *_ in a._fields_] == ["stft", "colour", "index_scratch", "index_scratch_pitch"]
    return a.stft, a.colour, a.index_scratch or 0, a.index_scratch_pitch


def test_stft_image_args(jsg):
    S, capi = jsg.spectrogram, jsg.capi
    lut = FakeTensor((256,), torch.int32, ptr=0x7F0000500000)
    argb = FakeTensor((BINS, 100), torch.int32, strides=(128, 1), ptr=0x7F0000600000)
    vmin, vmax, mult = (float(v) for v in jsg.colormap_range(256, -50.0, 50.0))
    stft = dict(in_=D_IN.data_ptr(), in_pitch=5120, channels=2, hop=256, feedblocks=4, n_frames=10, ring_width=10, in_samples=5000)
    colour = dict(ring_width=10, height=BINS, n_cols=10, x_wrap=100, lut=lut.data_ptr(), n_colors=256, vmin=vmin, vmax=vmax, access_mult=mult,
                  argb_out=argb.data_ptr(), argb_pitch=128)
    # without index scratch: the ring is the launch; out_db, out_tail and colour.db stay NULL (no dB column is written)
    st, co, scratch, pitch = image_blocks(S._stft_image_args(PLAN, D_IN, 256, 10, lut, -50.0, 50.0, argb, None))
    expect(st, **stft)
    expect(co, **colour)
    assert (scratch, pitch) == (0, 0)
    # with index scratch: its columns are the ring
    sc = FakeTensor((32, 576), torch.uint8, ptr=0x7F0000800000)
    st, co, scratch, pitch = image_blocks(S._stft_image_args(PLAN, D_IN, 256, 10, lut, -50.0, 50.0, argb, sc, ring_pos=30, mix_mode=capi.MIX_LEFT,
                                                             first_frame=2, feedblocks=5, plan_select=1, exact_log=True, blocks_per_cu=3))
    expect(st, **dict(stft, ring_width=32, ring_pos=30, mix_mode=capi.MIX_LEFT, first_frame=2, feedblocks=5, plan_select=1, exact_log=1, blocks_per_cu=3))
    expect(co, **dict(colour, ring_width=32, col_first=30, x_first=30))            # colour covers exactly the columns of the launch
    assert co.col_first == st.ring_pos and co.n_cols == st.n_frames and co.ring_width == st.ring_width
    assert (scratch, pitch) == (sc.data_ptr(), 576)
    # ring_width and x_first named by the caller
    st, co, scratch, pitch = image_blocks(S._stft_image_args(PLAN, D_IN, 256, 10, lut, -50.0, 50.0, argb, sc, ring_width=20, ring_pos=4, x_first=50))
    expect(st, **dict(stft, ring_width=20, ring_pos=4))
    expect(co, **dict(colour, ring_width=20, col_first=4, x_first=50))
    assert (scratch, pitch) == (sc.data_ptr(), 576)


@pytest.mark.parametrize("bad", [FakeTensor((2, 5000), torch.float64), FakeTensor((2, 5000), strides=(1, 2)), FakeTensor((2, 5000), is_cuda=False)],
                         ids=["float64", "inner_stride", "host"])
def test_stft_image_args_refuses_what_stft_args_refuses(jsg, bad):
    """The image path reads d_in through the same pointer geometry as the dB path: it takes float32 CUDA rows of unit stride only."""
    S = jsg.spectrogram
    lut = FakeTensor((256,), torch.int32)
    argb = FakeTensor((BINS, 100), torch.int32)
    with pytest.raises(AssertionError):
        S._stft_args(PLAN, bad, 256, 10, D_OUT)
    with pytest.raises(AssertionError):
        S._stft_image_args(PLAN, bad, 256, 10, lut, -50.0, 50.0, argb, None)
    with pytest.raises(AssertionError):
        S._stft_image_args(PLAN, D_IN, 256, 10, lut, -50.0, 50.0, FakeTensor((BINS, 100), torch.int32, strides=(1, BINS)), None)
    with pytest.raises(AssertionError):
        S._stft_image_args(PLAN, D_IN, 256, 10, lut, -50.0, 50.0, argb, FakeTensor((32, 576), torch.int32))


def test_cstft_args(jsg):
    S = jsg.spectrogram
    x = FakeTensor((3, 4000), strides=(4096, 1), ptr=0x7F0000100000)
    X = FakeTensor((3, 14, BINS), torch.complex64, strides=(14 * 520, 520, 1), ptr=0x7F0000900000)
    a = S._cstft_args(PLAN, x, 300, 14, X, None)
    expect(a, in_=x.data_ptr(), in_pitch=4096, rows=3, hop=300, n_frames=14, in_samples=4000, out=X.data_ptr(), out_frame_pitch=520,
           out_row_pitch=14 * 520)
    a = S._cstft_args(PLAN, x[2], 300, 14, X[2], 3900)                # one row: a 1-dimensional input, a 2-dimensional output
    expect(a, in_=x.data_ptr() + 2 * 4096 * 4, in_pitch=4000, rows=1, hop=300, n_frames=14, in_samples=3900, out=X.data_ptr() + 2 * 14 * 520 * 8,
           out_frame_pitch=520, out_row_pitch=14 * 520)
    expect(S._cstft_args(PLAN, x, 300, 14, X, 0), in_=x.data_ptr(), in_pitch=4096, rows=3, hop=300, n_frames=14, in_samples=0, out=X.data_ptr(),
           out_frame_pitch=520, out_row_pitch=14 * 520)                # 0: not checked
    for bad_x, bad_X in ((FakeTensor((3, 4000), torch.float64), X), (x, FakeTensor((3, 14, BINS))), (x, FakeTensor((2, 14, BINS), torch.complex64)),
                         (x, FakeTensor((3, 14, BINS), torch.complex64, strides=(1, 3, 42)))):
        with pytest.raises(AssertionError):
            S._cstft_args(PLAN, bad_x, 300, 14, bad_X, None)


def test_istft_args(jsg):
    S = jsg.spectrogram
    X = FakeTensor((3, 14, BINS), torch.complex64, strides=(14 * 520, 520, 1), ptr=0x7F0000900000)
    y = FakeTensor((3, 4900), strides=(5000, 1), ptr=0x7F0000A00000)
    a = S._istft_args(PLAN, X, 300, 14, y, None)
    expect(a, in_=X.data_ptr(), in_frame_pitch=520, in_row_pitch=14 * 520, rows=3, hop=300, n_frames=14, out=y.data_ptr(), out_pitch=5000,
           out_samples=4900)
    a = S._istft_args(PLAN, X[1], 300, 14, y[1], 4000)
    expect(a, in_=X.data_ptr() + 14 * 520 * 8, in_frame_pitch=520, in_row_pitch=14 * 520, rows=1, hop=300, n_frames=14, out=y.data_ptr() + 5000 * 4,
           out_pitch=4900, out_samples=4000)
    for bad_X, bad_y in ((FakeTensor((3, 14, BINS)), y), (X, FakeTensor((3, 4900), torch.float64)), (X, FakeTensor((2, 4900))), (X[0][0], y)):
        with pytest.raises(AssertionError):
            S._istft_args(PLAN, bad_X, 300, 14, bad_y, None)


def test_pvoc_args(jsg):
    S = jsg.spectrogram
    X = FakeTensor((3, 14, BINS), torch.complex64, strides=(14 * 520, 520, 1), ptr=0x7F0000900000)
    Y = FakeTensor((3, 11, BINS), torch.complex64, strides=(11 * 576, 576, 1), ptr=0x7F0000B00000)
    a = S._pvoc_args(X, 1.3, 256, 1024, Y, 4)
    expect(a, in_=X.data_ptr(), in_frame_pitch=520, in_row_pitch=14 * 520, rows=3, n=1024, hop=256, n_frames_in=14, rate=1.3, out=Y.data_ptr(),
           out_frame_pitch=576, out_row_pitch=11 * 576, n_frames_out=11, chunk_frames=4)
    a = S._pvoc_args(X[2], 0.5, 256, 1024, Y[2], 0)
    expect(a, in_=X.data_ptr() + 2 * 14 * 520 * 8, in_frame_pitch=520, in_row_pitch=14 * 520, rows=1, n=1024, hop=256, n_frames_in=14, rate=0.5,
           out=Y.data_ptr() + 2 * 11 * 576 * 8, out_frame_pitch=576, out_row_pitch=11 * 576, n_frames_out=11)
    for bad_X, bad_Y in ((FakeTensor((3, 14, BINS)), Y), (X, FakeTensor((2, 11, BINS), torch.complex64)), (X, FakeTensor((3, 11, BINS), torch.complex64, strides=(1, 3, 33)))):
        with pytest.raises(AssertionError):
            S._pvoc_args(bad_X, 1.3, 256, 1024, bad_Y, 0)

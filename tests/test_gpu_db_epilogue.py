"""jsg_db_from_power_launch_ex -- the dB tail of the cross-GPU AbsMean (sharded.py) and of every exact_log launch -- on EVERY finite
non-negative float32 input, bit patterns 0x00000000 .. 0x7f7fffff (2^31 - 2^23 values), with both logarithms.

Reference: float32(10 * log10(float64(float32(p / div) + 1e-11f))), computed in float64 on the GPU.  The patterns are made on the GPU
(an int32 arange viewed as float32) in chunks of 2^27.

  * exact path (exact_log = 1, csrc/jsg_exact_math.h): within 2 ulp of the reference everywhere, and bit-identical to the CPU mirror
    (oracle/mirror.py exact_db) on a fixed subset of 2^27 - 2^19 values, one in 16, that covers every binade and every residue of the
    low mantissa bits;
  * hardware path (v_log_f32): within HW_ULP_BOUND = 2 ulp everywhere, and within parity_util.DB_SLACK of the float64 dB value on every
    input whose dB lies in [-110, 180] -- the assumption every dB parity test rests on;
  * divisors 3 and 6 (the non-power-of-two AbsMean) on a fixed strided subset;
  * non-finite inputs: +inf gives +inf and NaN gives NaN on both paths; count 0 and bad arguments return the documented codes.

Measured on an MI355X over all 2^31 - 2^23 inputs (worst ulp against the float32 reference / worst absolute error against the float64
dB value, per group of 16 binades of p; binade b holds p in [2^(b-127), 2^(b-126)), dB = 3.0103 * (b - 127) roughly; the binades below
64 all give the -110 dB of the 1e-11 floor):
  binades    0- 63:  exact 0 ulp 1.7e-08 dB | hardware 0 ulp 1.7e-08 dB
  binades   64- 95:  exact 1 ulp 4.1e-06 dB | hardware 2 ulp 1.4e-05 dB
  binades   96-127:  exact 2 ulp 4.1e-06 dB | hardware 2 ulp 8.8e-06 dB
  binades  128-159:  exact 1 ulp 4.1e-06 dB | hardware 2 ulp 1.7e-05 dB
  binades  160-191:  exact 1 ulp 7.9e-06 dB | hardware 2 ulp 3.3e-05 dB   (p = 2^33 .. 2^65: 100 .. 195 dB)
  binades  192-223:  exact 1 ulp 1.6e-05 dB | hardware 2 ulp 4.2e-05 dB   (195 .. 290 dB)
  binades  224-254:  exact 1 ulp 1.6e-05 dB | hardware 1 ulp 4.3e-05 dB   (290 .. 385 dB)
  hardware path, every input whose dB lies in [-110, 180]: at most 2.12e-05 dB from the float64 value -- inside DB_SLACK = 3e-5.
"""
import ctypes as C

import numpy as np
import pytest

from parity_util import DB_SLACK

pytestmark = pytest.mark.gpu

CHUNK = 1 << 27
END = 0x7f800000                      # first non-finite pattern
EXACT_ULP_BOUND = 2
HW_ULP_BOUND = 2                      # measured: 2 ulp (module docstring)
SUB = 16                              # mirror comparison: one pattern in 16
SLICE = 1 << 25                       # float64 comparison slices (four binades)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def _ordered(torch, f):
    """float32 -> int64 that is monotonic in the float value (ulp distance = difference)."""
    i = f.view(torch.int32).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7fffffff), i)


def _reference(torch, p, div):
    q = p if div == 1.0 else (p.double() / div).float()            # float32(p / div), correctly rounded (exact quotient in double)
    y = (q + np.float32(1e-11)).double()                           # float32 add, then the reference's double log10
    return 10.0 * torch.log10(y)


def test_db_epilogue_on_every_finite_input(jsg, torch_cuda):
    torch = torch_cuda
    from oracle import mirror
    mir = mirror.load()
    lib = jsg.capi.lib()
    st = torch.cuda.current_stream().cuda_stream
    per = 1 << 23                                                   # patterns per binade: a chunk holds 16 whole binades
    worst_ulp = {0: np.zeros(255, np.int64), 1: np.zeros(255, np.int64)}
    worst_abs = {0: np.zeros(255), 1: np.zeros(255)}
    slack_worst = 0.0
    mirror_checked = 0
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    for start in range(0, END, CHUNK):
        cnt = min(CHUNK, END - start)
        p = torch.arange(start, start + cnt, dtype=torch.int32, device="cuda").view(torch.float32)
        outs = {}
        for xl in (0, 1):
            outs[xl] = torch.empty_like(p)
            jsg.capi.check(lib.jsg_db_from_power_launch_ex(p.data_ptr(), outs[xl].data_ptr(), cnt, 1.0, xl, C.c_void_p(st)))
        for h in range(0, cnt, SLICE):                              # the float64 comparison a quarter chunk at a time (peak memory)
            b0 = (start + h) // per
            ps = p[h:h + SLICE]
            m = ps.numel()                                          # (the last chunk holds 15 binades: its last slice three)
            ref64 = _reference(torch, ps, 1.0)
            ord_ref = _ordered(torch, ref64.float())
            band = (ref64 >= -110.0) & (ref64 <= 180.0)
            for xl in (0, 1):
                out = outs[xl][h:h + m]
                ulp = (_ordered(torch, out) - ord_ref).abs_()
                worst_ulp[xl][b0:b0 + m // per] = ulp.view(-1, per).amax(dim=1).cpu().numpy()
                del ulp
                err = (out.double() - ref64).abs_()
                worst_abs[xl][b0:b0 + m // per] = err.view(-1, per).amax(dim=1).cpu().numpy()
                if xl == 0:
                    if bool(band.any()):
                        slack_worst = max(slack_worst, float(err[band].max()))
                else:
                    # the same bits as the CPU mirror on one pattern in 16 (every residue of the low mantissa bits comes round)
                    k = torch.arange(m // SUB, device="cuda", dtype=torch.int64)
                    sel = k * SUB + (k * 5) % SUB
                    p_cpu = ps[sel].cpu().numpy()
                    got = out[sel].cpu().numpy()
                    want = mir.exact_db(p_cpu)
                    bad = got.view(np.uint32) != want.view(np.uint32)
                    assert not bad.any(), f"exact path differs from the mirror at p = {p_cpu[bad][:4]} ({int(bad.sum())} values)"
                    mirror_checked += sel.numel()
                    del k, sel
                del err
            del ref64, ord_ref, band
        del p, outs
    peak_gib = torch.cuda.max_memory_allocated() / 2 ** 30
    wu, wa = worst_ulp, worst_abs
    print(f"\nmirror-checked values: {mirror_checked}; peak device memory {peak_gib:.2f} GiB; hw worst |err| for dB in [-110, 180]: "
          f"{slack_worst:.3g} dB")
    for b in range(0, 255, 1):
        print(f"binade {b:3d}: exact {int(wu[1][b])} ulp {wa[1][b]:.3g} dB | hw {int(wu[0][b])} ulp {wa[0][b]:.3g} dB")
    assert mirror_checked >= 10 ** 8
    assert peak_gib <= 6.0, peak_gib
    assert wu[1].max() <= EXACT_ULP_BOUND, f"exact path: {int(wu[1].max())} ulp in binade {int(wu[1].argmax())}"
    assert wu[0].max() <= HW_ULP_BOUND, f"hardware path: {int(wu[0].max())} ulp in binade {int(wu[0].argmax())}"
    assert slack_worst <= DB_SLACK, f"hardware log: {slack_worst:.3g} dB > DB_SLACK = {DB_SLACK} on a dB value in [-110, 180]"


@pytest.mark.parametrize("div", [3.0, 6.0])
def test_db_epilogue_with_a_non_power_of_two_divisor(jsg, torch_cuda, div):
    """The AbsMean divisor of 3 and 6 channels: the GPU's float32 division is the correctly rounded one (the exact path then equals
    the mirror applied to numpy's float32 quotient bit for bit), and both paths keep their bounds."""
    torch = torch_cuda
    from oracle import mirror
    mir = mirror.load()
    lib = jsg.capi.lib()
    st = torch.cuda.current_stream().cuda_stream
    bits = torch.arange(0, END, 97, dtype=torch.int64, device="cuda").to(torch.int32)      # 22 million patterns, every binade
    p = bits.view(torch.float32)
    ref64 = _reference(torch, p, div)
    ref32 = ref64.float()
    for xl in (0, 1):
        out = torch.empty_like(p)
        jsg.capi.check(lib.jsg_db_from_power_launch_ex(p.data_ptr(), out.data_ptr(), p.numel(), div, xl, C.c_void_p(st)))
        ulp = (_ordered(torch, out) - _ordered(torch, ref32)).abs()
        assert int(ulp.max()) <= (EXACT_ULP_BOUND if xl else HW_ULP_BOUND), (xl, int(ulp.max()))
        if xl:
            q = (p.cpu().numpy() / np.float32(div)).astype(np.float32)
            want = mir.exact_db(q)
            assert (out.cpu().numpy().view(np.uint32) == want.view(np.uint32)).all(), "exact path with a divisor differs from the mirror"
        else:
            err = (out.double() - ref64).abs()
            band = (ref64 >= -110.0) & (ref64 <= 180.0)
            assert float(err[band].max()) <= DB_SLACK


def test_db_epilogue_non_finite_and_arguments(jsg, torch_cuda):
    torch = torch_cuda
    lib = jsg.capi.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = torch.tensor([float("inf"), float("nan"), 0.0, 1.0, 3.4028234663852886e38], dtype=torch.float32, device="cuda")
    for xl in (0, 1):
        out = torch.full_like(p, -7.0)
        jsg.capi.check(lib.jsg_db_from_power_launch_ex(p.data_ptr(), out.data_ptr(), p.numel(), 1.0, xl, st))
        o = out.cpu().numpy()
        assert np.isposinf(o[0]), (xl, o[0])
        assert np.isnan(o[1]), (xl, o[1])
        assert np.isfinite(o[2:]).all() and o[2] == np.float32(-110.0), (xl, o)
        jsg.spectrogram.db_from_power(p, out, exact_log=bool(xl))                # the Python entry point reaches both paths
        o2 = out.cpu().numpy()
        assert np.isposinf(o2[0]) and np.isnan(o2[1]) and (o2[2:] == o[2:]).all()
    out = torch.full_like(p, -7.0)
    assert lib.jsg_db_from_power_launch_ex(p.data_ptr(), out.data_ptr(), 0, 1.0, 1, st) == jsg.capi.JSG_OK   # count 0: nothing to do
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == np.float32(-7.0)).all()
    for div in (0.0, -1.0, float("nan")):
        assert lib.jsg_db_from_power_launch_ex(p.data_ptr(), out.data_ptr(), p.numel(), div, 1, st) == jsg.capi.JSG_ERR_INVALID
    assert lib.jsg_db_from_power_launch_ex(p.data_ptr(), out.data_ptr(), -1, 1.0, 0, st) == jsg.capi.JSG_ERR_INVALID
    assert lib.jsg_db_from_power_launch_ex(None, out.data_ptr(), p.numel(), 1.0, 0, st) == jsg.capi.JSG_ERR_INVALID

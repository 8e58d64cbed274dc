"""Build-time guard for the table and load side of the 1024-point "runs" kernel (stft_db_kernel STREAM == 2; DESIGN.md section 6, "Runs
tables").  Its two instantiations must stay inside the 96 VGPRs that five waves per SIMD allow, without spills or scratch -- with
__launch_bounds__(256, 5) the compiler spills beyond that --, its loop must not read more lane-table values from LDS than it did when the
guard was written, exactly the loads of the hop that nobody re-reads carry the non-temporal hint, and the LDS-DMA pieces match the table block.
CPU only: reads the code object's metadata and disassembles it, as the other two ISA guards do."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
OBJ = os.path.join(ROOT, "jadespectrogram_amd", "build", "jsg_stft_a.o")     # the unit that holds the 1024-point kernels

# Counted in the loop body (one run = two columns) of the product build this guard was written with, both logarithms alike:
#   ds_read_b128: per column four reads of the window and four of the stage-2 twiddles = 16, as in the change's parent (16): holding half of
#       the window in registers (JSG_X_RUNS_WINREG=4: 12 reads, 90 / 92 VGPRs, no spill) did not separate in the A/B and is not in the product.
#       The stage-1 and post-pass tables have been in registers since RTAB.
#   global_load_dwordx2 with the nt modifier: 4 of the loop's 12 -- the hop that no other run reads, the upper half of a run's first frame,
#       loaded in the last round of the run before (JSG_X_RUNS_NT1, the product's; parent: 0).  The hops shared with the neighbours stay plain.
#   global_load_lds_dwordx4 in the whole function: 3 pieces per thread -- the full table block of 10 880 bytes over 256 threads; the smaller
#       block of JSG_X_RUNS_ONCETAB (2 pieces, 8 320 bytes) is a variant switch, not in the product
MAX_B128_IN_LOOP = 16
NT_LOADS_IN_LOOP = 4
TABLE_PIECES = 3


def _code_object(tmp_path):
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump", "llvm-readelf"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip(f"{tool} not found under {LLVM}")
    if not os.path.exists(OBJ):
        from jadespectrogram_amd import _build
        _build.build_lib()
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", OBJ, str(tmp_path / "scratch.o")])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"])
    return co


RUNS = re.compile(r"stft_db_kernelINS_3CfgI(?:Li\d+E)+EELi3ELi0ELi2ELi(\d)EEEv")   # one channel per column, float columns, STREAM 2, XLOG


def _functions(text):
    """name -> [(address, instruction text)]"""
    cur, body = None, []
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            if cur:
                yield cur, body
            cur, body = m.group(1), []
            continue
        m = re.match(r"^\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if cur and m:
            body.append((int(m.group(2), 16), m.group(1).strip()))
    if cur:
        yield cur, body


def _loop_body(body):
    """the instructions of the function's largest loop: from the target of the backward branch that spans the most code up to that branch"""
    best = None
    for addr, ins in body:
        m = re.match(r"s_c?branch\w*\s+(\d+)$", ins)
        if not m or int(m.group(1)) < 32768:
            continue
        target = addr + 4 + (int(m.group(1)) - 65536) * 4
        if best is None or addr - target > best[1] - best[0]:
            best = (target, addr)
    assert best, "no backward branch found"
    return [ins for addr, ins in body if best[0] <= addr <= best[1]]


def test_the_runs_kernels_keep_five_waves_per_simd_without_spills(tmp_path):
    co = _code_object(tmp_path)
    notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co]).decode()
    seen = []
    for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = RUNS.search(name)
        if not m:
            continue
        get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", blk).group(1))
        vgpr, spill, scratch = get("vgpr_count"), get("vgpr_spill_count"), get("private_segment_fixed_size")
        print(f"XLOG {m.group(1)}: {vgpr} VGPRs, {spill} spilled, {scratch} bytes of scratch")
        assert vgpr <= 96, f"{name}: {vgpr} VGPRs, five waves per SIMD allow 96"
        assert spill == 0 and scratch == 0, f"{name}: {spill} VGPRs spilled, {scratch} bytes of scratch"
        seen.append(int(m.group(1)))
    assert sorted(seen) == [0, 1], f"runs instantiations found: {sorted(seen)} (Cfg1024, one channel per column, the two logarithms)"


def test_the_runs_loop_keeps_its_table_reads_and_hints_only_the_read_once_hop(tmp_path):
    co = _code_object(tmp_path)
    text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co]).decode()
    seen = []
    for name, body in _functions(text):
        m = RUNS.search(name)
        if not m:
            continue
        loop = _loop_body(body)
        loads = [i for i in loop if i.startswith("global_load_dwordx2")]
        assert len(loads) == 12, f"{name}: the loop found holds {len(loads)} frame loads, a run of two columns has 4 + 8"
        b128 = [i for i in loop if i.startswith("ds_read_b128")]
        hinted = [i for i in loads if re.search(r"\bnt\b", i)]
        pieces = [i for _, i in body if i.startswith("global_load_lds_dwordx4")]
        print(f"XLOG {m.group(1)}: loop of {len(loop)} instructions, ds_read_b128 {len(b128)}, hinted frame loads {len(hinted)}, table pieces {len(pieces)}")
        assert len(b128) <= MAX_B128_IN_LOOP, f"{name}: {len(b128)} ds_read_b128 in the loop, {MAX_B128_IN_LOOP} when the guard was written"
        assert len(hinted) == NT_LOADS_IN_LOOP, f"{name}: {len(hinted)} of the loop's frame loads carry the nt modifier, expected {NT_LOADS_IN_LOOP}"
        # ... and they are the four of the frame's upper half (lane + 64 m float pairs, m = 4 .. 7: byte offsets 2048 .. 3584 from the frame)
        offs = sorted(int(re.search(r"offset:(\d+)", i).group(1)) if "offset:" in i else 0 for i in hinted)
        assert offs == [2048, 2560, 3072, 3584][:NT_LOADS_IN_LOOP], f"{name}: hinted loads at byte offsets {offs}"
        assert len(pieces) == TABLE_PIECES, f"{name}: {len(pieces)} LDS-DMA table pieces, the table block has {TABLE_PIECES} per thread"
        seen.append(int(m.group(1)))
    assert sorted(seen) == [0, 1], f"runs instantiations found: {sorted(seen)}"

"""Build-time guard for the bookkeeping of the 1024-point "runs" kernel (stft_db_kernel STREAM == 2; DESIGN.md section 6, "Runs bookkeeping").

Its steady-state loop (one iteration = one run = two columns) forms no 64-bit vector address -- every column store is scalar base + a lane
offset held for the whole wave + an immediate -- and selects lane 0's exceptions of the mirrored half with one v_cndmask each instead of exec
regions with duplicated stores.  A toolchain or source change that brings the per-column address arithmetic or the exec regions back shows up
here as a count.  CPU only: disassembles the device code object."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
OBJ = os.path.join(ROOT, "jadespectrogram_amd", "build", "jsg_stft_a.o")     # the unit that holds the 1024-point kernels

# Counted in the loop body (one run = two columns) of the build this guard was written with, per function (XLOG 0: v_log, 1: jsg_exact_db):
#   v_cndmask + v_cmp: 8 lane-0 selects (four mirrored stores x two columns) + two leftover pairs that rebuild the inverse of a uniform
#       flag (linear output, tail plane) once per iteration = 12; the exact-log function has the selects and compares of jsg_exact_db on
#       top = 78.  (The change's parent had 6 and 72: it branched where this build selects -- 4 s_andn2_saveexec, 4 more store
#       instructions, 4 v_lshl_add_u64 and 8 v_lshlrev per iteration.)
#   s_and_saveexec + s_andn2_saveexec: per column the lane-0 write of the post-pass exchange and bin n (tail plane / inside the column: two
#       static regions, one executed) = 6 + 0; jsg_exact_db's special-value branches bring the exact-log function to 22 + 0 (parent: 10, 26)
MAX_SELECTS = {0: 12, 1: 78}
MAX_SAVEEXEC = {0: 6, 1: 22}


def _disassemble(tmp_path):
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip(f"{tool} not found under {LLVM}")
    if not os.path.exists(OBJ):
        from jadespectrogram_amd import _build
        _build.build_lib()
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", OBJ, str(tmp_path / "scratch.o")])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"])
    return subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co]).decode()


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


def _runs_functions(text):
    out = {}
    for name, body in _functions(text):
        m = re.search(r"stft_db_kernelINS_3CfgI(?:Li\d+E)+EELi\dELi\dELi2ELi(\d)EEEv", name)
        if m:
            out[int(m.group(1))] = (name, body)
    assert sorted(out) == [0, 1], f"runs instantiations found: {sorted(out)} (Cfg1024, one channel per column, the two logarithms)"
    return out


def test_the_runs_loop_keeps_its_bookkeeping_off_the_vector_pipe(tmp_path):
    funcs = _runs_functions(_disassemble(tmp_path))
    for xlog, (name, body) in funcs.items():
        loop = _loop_body(body)
        loads = [i for i in loop if i.startswith("global_load_dwordx2")]
        assert len(loads) == 12, f"{name}: the loop found holds {len(loads)} frame loads, a run of two columns has 4 + 8"
        wide = [i for i in loop if i.startswith("v_lshl_add_u64")]
        assert not wide, f"{name}: {len(wide)} 64-bit vector address additions in the loop, e.g. {wide[0]}"
        stores = [i for i in loop if i.startswith("global_store_dword")]
        assert stores and all(re.search(r"\bs\[\d+:\d+\]", i) for i in stores), f"{name}: column stores without a scalar base: {[i for i in stores if ' off' in i][:2]}"
        selects = len([i for i in loop if i.startswith(("v_cndmask", "v_cmp"))])
        saveexec = len([i for i in loop if i.startswith(("s_and_saveexec", "s_andn2_saveexec"))])
        print(f"{name[:40]}... XLOG {xlog}: loop of {len(loop)} instructions, v_cndmask + v_cmp {selects}, saveexec {saveexec}, stores {len(stores)}")
        assert not any(i.startswith(("scratch_", "buffer_load", "buffer_store")) for _, i in body), f"{name}: scratch / buffer accesses"
        assert saveexec <= MAX_SAVEEXEC[xlog], f"{name}: {saveexec} exec regions in the loop, {MAX_SAVEEXEC[xlog]} when the guard was written"
        assert selects <= MAX_SELECTS[xlog], f"{name}: {selects} v_cndmask + v_cmp in the loop, {MAX_SELECTS[xlog]} when the guard was written"

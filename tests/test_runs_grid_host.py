"""The two-population grid of the 1024-point runs kernel (csrc/jsg_runs_grid.h, DESIGN.md section 6 "Two populations"): a stand-alone C++
program walks every (block, step) of the partition with the kernel's index arithmetic.  CPU only."""
import json
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_step_of_the_two_population_grid_lands_on_its_group():
    exe = os.path.join(tempfile.gettempdir(), "jsg_runs_grid_test")
    src = os.path.join(ROOT, "tests", "cpp", "runs_grid_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "jadespectrogram_amd", "csrc"), src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["bad"] == 0 and info["cases"] >= 300, info

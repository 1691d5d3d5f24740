"""pick() of csrc/kernel_pick.hpp, the compile-time selection behind the launchers of the *_kernels.hip units, without a device: a
stand-alone program built with plain g++, ASan and UBSan (tests/kernel_pick_host.cpp) walks every combination of two flags, a
refusing list and a list with a fallback, values outside the lists included."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pyisingmontecarlo_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pick_calls_once_with_the_matching_tags(tmp_path):
    exe = str(tmp_path / "kernel_pick_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "kernel_pick_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if out.returncode != 0 and ("cannot find -lasan" in out.stderr or "cannot find -lubsan" in out.stderr or "libasan" in out.stderr):
        pytest.skip("sanitizer runtimes are not installed with this g++")
    assert out.returncode == 0, out.stderr[-3000:]
    assert "warning" not in out.stderr, out.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "kernel_pick_host: 331 cases, 0 failures" in run.stdout and "runtime error" not in run.stderr

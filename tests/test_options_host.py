"""The options block of a graph or a container (csrc/options.hpp), without a device: `tests/options_host.cpp` drives `Options::set`
and `Options::from_env` under AddressSanitizer + UndefinedBehaviorSanitizer, as an executable of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pyisingmontecarlo_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_options_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "options_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-I" + CSRC,
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "options_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and ("cannot find -lasan" in build.stderr or "cannot find -lubsan" in build.stderr or "libasan" in build.stderr):
        pytest.skip("sanitizer runtimes are not installed with this g++")
    assert build.returncode == 0, build.stderr[-3000:]
    assert "warning" not in build.stderr, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "options_host: ok" in out.stdout and "runtime error" not in out.stderr and "Sanitizer" not in out.stderr

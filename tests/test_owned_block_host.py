"""The one owner of device and pinned blocks, and of pooled streams and events (csrc/owned_block.hpp), without a device:
`tests/owned_block_host.cpp` drives the handles with counting free functions under AddressSanitizer + UndefinedBehaviorSanitizer, as an executable of its own; and the
host sources are read to see that nothing but the handle and the caches themselves hands a block back."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pyisingmontecarlo_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_owned_block_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "owned_block_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-I" + CSRC,
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "owned_block_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and ("cannot find -lasan" in build.stderr or "cannot find -lubsan" in build.stderr or "libasan" in build.stderr):
        pytest.skip("sanitizer runtimes are not installed with this g++")
    assert build.returncode == 0, build.stderr[-3000:]
    assert "warning" not in build.stderr, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "owned_block_host: ok" in out.stdout and "runtime error" not in out.stderr and "Sanitizer" not in out.stderr


def _host_sources():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".hpp", ".cpp", ".inc")):
            with open(os.path.join(CSRC, name)) as f:
                yield name, f.read()


def test_only_the_handle_frees_blocks():
    sources = dict(_host_sources())
    assert {"core.hip", "owned_block.hpp", "internal.hpp", "isingmc.hip", "tempering.hip"} <= set(sources)
    for call in ("cached_free(", "cached_host_free("):
        users = {name for name, text in sources.items() if call in text}
        assert users == {"core.hip", "owned_block.hpp"}, (call, sorted(users))
    # ... and pooled streams and events go back through their handle alone
    for call in ("pooled_stream_destroy(", "pooled_event_destroy("):
        users = {name for name, text in sources.items() if call in text}
        assert users == {"core.hip", "owned_block.hpp"}, (call, sorted(users))
    for name, text in sources.items():
        assert not re.search(r"\bstruct\s+Undo\b", text), name

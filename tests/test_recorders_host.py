"""The periodic recorders without a device: Periodic (csrc/host_logic.hpp) -- sample points, stretches and the replay guard of a
repeated call -- against a brute-force walk over timesteps in a stand-alone program built with ASan and UBSan
(tests/recorders_host.cpp), and the surface the two series keep: the methods of the binding's classes and the library's symbols."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pyisingmontecarlo_amd", "csrc")
SERIES_SYMBOLS = ["isingmc_%s_series_%s" % (kind, s) for kind in ("overlap", "observable")
                  for s in ("create", "record", "set_every", "count", "get", "reset", "destroy")]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_periodic_against_a_brute_force_walk(tmp_path):
    exe = str(tmp_path / "recorders_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "recorders_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if out.returncode != 0 and ("cannot find -lasan" in out.stderr or "cannot find -lubsan" in out.stderr or "libasan" in out.stderr):
        pytest.skip("sanitizer runtimes are not installed with this g++")
    assert out.returncode == 0, out.stderr[-3000:]
    assert "warning" not in out.stderr, out.stderr[-3000:]
    for seed in (1, 2):
        run = subprocess.run([exe, "400", str(seed)], capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
        assert "recorders_host: 400 cases, 0 failures" in run.stdout and "runtime error" not in run.stderr


def test_series_surface_is_unchanged():
    from pyisingmontecarlo_amd import _capi
    assert len(SERIES_SYMBOLS) == 14
    assert sorted(s for s in _capi.EXPORTED_SYMBOLS if "_series_" in s) == sorted(SERIES_SYMBOLS)
    assert os.path.exists(_capi.LIB_PATH), "libisingmc.so is not built"
    so = ctypes.CDLL(_capi.LIB_PATH)
    for sym in SERIES_SYMBOLS:
        assert hasattr(so, sym), sym
    for cls in (_capi.OverlapSeries, _capi.ObservableSeries):
        for name in ("record", "set_every", "count", "capacity", "get", "reset", "close"):
            assert hasattr(cls, name), (cls.__name__, name)
        for name in ("record", "set_every", "get", "reset"):
            assert getattr(cls, name).__doc__, (cls.__name__, name)
        assert isinstance(cls.count, property) and isinstance(cls.capacity, property)

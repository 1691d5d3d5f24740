"""The host side of the moment sums, without a device: the bit-sliced vertical counter as an executable of its own,
plain and under AddressSanitizer + UndefinedBehaviorSanitizer; the numpy restatement the GPU tests compare against, on values
worked out by hand; and the surface -- header, library exports, Python methods."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import moments_reference as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pyisingmontecarlo_amd", "csrc")
SYMBOLS = ("isingmc_states_set_moments_every", "isingmc_states_moments_every", "isingmc_moments_accumulate", "isingmc_moments_get",
           "isingmc_moments_reset", "isingmc_run_sampling_moments")


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-I" + CSRC] + extra +
                           [os.path.join(ROOT, "tests", "vertical_counter_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and ("cannot find -lasan" in build.stderr or "cannot find -lubsan" in build.stderr or "libasan" in build.stderr):
        pytest.skip("sanitizer runtimes are not installed with this g++")
    assert build.returncode == 0, build.stderr[-3000:]
    assert "warning" not in build.stderr, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "vertical_counter_host: ok" in out.stdout and "runtime error" not in out.stderr and "Sanitizer" not in out.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_vertical_counter_plain(tmp_path):
    _build_and_run(tmp_path, "vertical_counter_host", [])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_vertical_counter_under_asan_and_ubsan(tmp_path):
    _build_and_run(tmp_path, "vertical_counter_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_reference_on_a_three_site_chain():
    """Sites 0 - 1 - 2; entries: (0, 1), (1, 2), (0, 1) again, (0, 2) with J = 0 (no coupling is read: it counts all the same) and
    (2, 2).  Two samples of two replicas, True = +1."""
    ea, eb = [0, 1, 0, 0, 2], [1, 2, 1, 2, 2]
    samples = np.array([[[1, 1, 0], [0, 1, 0]],      # s = (+ + -), (- + -)
                        [[1, 0, 0], [1, 1, 1]]],     # s = (+ - -), (+ + +)
                       dtype=bool)
    # site 0: + - + + = 2; site 1: + + - + = 2; site 2: - - - + = -2
    assert MR.site_sums(samples).tolist() == [2, 2, -2]
    assert MR.site_sums(samples, per_replica=True).tolist() == [[2, 0, -2], [0, 2, 0]]
    # s0 s1: + - - + = 0; s1 s2: - - + + = 0; s0 s2: - + - + = 0; s2 s2 = +1 four times
    assert MR.bond_sums(samples, ea, eb).tolist() == [0, 0, 0, 0, 4]
    one = samples[0]   # a single sample [R, N]: s0 s1 = + -, s1 s2 = - -, s0 s2 = - +
    assert MR.site_sums(one).tolist() == [0, 2, -2] and MR.bond_sums(one, ea, eb).tolist() == [0, -2, 0, 0, 2]
    acc = MR.Accumulator(ea, eb)
    for s in samples:
        acc.add(s)
    assert acc.n == 2 and acc.site.tolist() == [2, 2, -2] and acc.bond.tolist() == [0, 0, 0, 0, 4]
    acc = MR.Accumulator(ea, eb, per_replica=True)
    for s in samples:
        acc.add(s)
    assert acc.site.tolist() == [[2, 0, -2], [0, 2, 0]]


def test_surface():
    """The C ABI, the binding and both Python classes carry the moment sums."""
    with open(os.path.join(ROOT, "include", "isingmc.h")) as f:
        header = f.read()
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), sym
    assert "ISINGMC_MOMENTS_PER_REPLICA" in header and "ISINGMC_MOMENTS_BONDS" in header
    from pyisingmontecarlo_amd import _capi
    so = ctypes.CDLL(_capi.LIB_PATH) if os.path.exists(_capi.LIB_PATH) else None
    assert so is not None, "libisingmc.so is not built"
    for sym in SYMBOLS:
        assert hasattr(so, sym), sym
        assert sym in _capi.EXPORTED_SYMBOLS
    for name in ("set_moments_every", "accumulate_moments", "moments", "reset_moments"):
        assert callable(getattr(_capi.States, name))
    import py_monte_carlo
    sig = py_monte_carlo.Lattice.run_monte_carlo_and_measure_spins.__doc__.splitlines()[0]
    idx = [sig.index(n + ":") for n in ("beta", "timesteps", "num_experiments", "thermalization_time", "sampling_freq", "per_experiment", "bonds")]
    assert idx == sorted(idx)
    for name in ("set_measure_spins_every", "get_measured_spins", "reset_measured_spins"):
        assert hasattr(py_monte_carlo.ClassicIsing, name)
    lat = py_monte_carlo.Lattice([((0, 1), 1.0), ((1, 2), -1.0)])
    with pytest.raises(ValueError, match="per_experiment=False"):
        lat.run_monte_carlo_and_measure_spins(1.0, 10, 2, bonds=True)
    with pytest.raises(ValueError, match="sampling_freq"):
        lat.run_monte_carlo_and_measure_spins(1.0, 10, 2, sampling_freq=0)

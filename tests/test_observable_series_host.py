"""The observable series without a device: the surface -- header, binding and library carry the same new symbols --,
NULL handles, the numpy reference against brute-force sums, and magnetisation_moments / structure_factor against closed forms."""
import ctypes
import os
import re

import numpy as np
import pytest

import observable_series_reference as XR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["isingmc_observable_series_" + s for s in ("create", "record", "set_every", "count", "get", "reset", "destroy")]


def test_surface():
    """The header declares every new symbol the binding binds, and the library exports them."""
    with open(os.path.join(ROOT, "include", "isingmc.h")) as f:
        header = f.read()
    from pyisingmontecarlo_amd import _capi
    bound = [s for s in _capi.EXPORTED_SYMBOLS if s.startswith("isingmc_observable_series_")]
    assert sorted(bound) == sorted(SYMBOLS)
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), sym
    for name, value in (("ENERGY", 1), ("MAGNETISATION", 2), ("BY_RUNG", 4)):
        assert re.search(r"#define\s+ISINGMC_OBS_%s\s+%du" % (name, value), header)
        assert getattr(_capi, "OBS_" + name) == value
    assert re.search(r"#define\s+ISINGMC_ABI_VERSION\s+4\b", header)
    assert os.path.exists(_capi.LIB_PATH), "libisingmc.so is not built"
    so = ctypes.CDLL(_capi.LIB_PATH)
    for sym in SYMBOLS:
        assert hasattr(so, sym), sym
    for name in ("record", "set_every", "count", "capacity", "get", "reset", "close"):
        assert hasattr(_capi.ObservableSeries, name)
    assert callable(_capi.States.observable_series)
    import py_monte_carlo
    from pyisingmontecarlo_amd.tempering import ClassicalTempering
    for cls in (py_monte_carlo.ClassicIsing, ClassicalTempering):
        for name in ("set_measure_observables_every", "get_measured_observables", "reset_measured_observables"):
            assert hasattr(cls, name)
    assert hasattr(py_monte_carlo.Lattice, "run_monte_carlo_and_measure_observables")


def test_null_handles_are_refused_without_a_device():
    from pyisingmontecarlo_amd import _capi
    L = _capi.lib()
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    assert L.isingmc_observable_series_create(None, None, 3, 4, ctypes.byref(out)) == _capi.ERR_INVALID and not out
    assert b"NULL" in L.isingmc_last_error()
    assert L.isingmc_observable_series_record(None) == _capi.ERR_INVALID
    assert L.isingmc_observable_series_set_every(None, 2) == _capi.ERR_INVALID
    assert L.isingmc_observable_series_count(None, ctypes.byref(n), None) == _capi.ERR_INVALID
    assert L.isingmc_observable_series_get(None, 0, 0, None, None, None, None) == _capi.ERR_INVALID
    assert L.isingmc_observable_series_reset(None) == _capi.ERR_INVALID
    assert b"NULL series" in L.isingmc_last_error()
    assert L.isingmc_observable_series_destroy(None) == _capi.OK     # like free(NULL)


def test_reference_against_brute_force():
    from pyisingmontecarlo_amd.correlation import plane_classes

    rng = np.random.default_rng(4)
    A = rng.integers(0, 2, (5, 12)).astype(bool)
    tables = plane_classes((3, 4)).astype(np.int64)
    tables[1, 7] = XR.NO_CLASS
    n_classes = 6                                        # classes 4 and 5 (and 3 of table 0) are empty
    s = 2 * A.astype(np.int64) - 1
    mag = XR.magnetisation(A)
    assert mag.dtype == np.int64 and mag.tolist() == [sum(int(v) for v in row) for row in s]
    got = XR.class_sums(A, tables, n_classes)
    assert got.dtype == np.int64 and got.shape == (5, 2, 6)
    for r in range(5):
        for t in range(2):
            for c in range(n_classes):
                assert got[r, t, c] == sum(int(s[r, i]) for i in range(12) if tables[t, i] == c)
    assert np.array_equal(got[:, 0].sum(axis=1), mag)                      # a table without NO_CLASS adds up to the magnetisation
    assert np.array_equal(got[:, 1].sum(axis=1), mag - s[:, 7])            # ... and the site without a class counts nowhere
    assert (got[:, :, 4:] == 0).all()
    assert XR.sample_points(2, 3, 2, 12) == [5, 8, 11]
    # ... and in the form the series returns them -- [samples, columns] and [samples, columns, x] -- the reference's rows feed the new
    # helpers: <m> is the mean of the rows, and S(0) of a table without NO_CLASS is M^2 / N
    from pyisingmontecarlo_amd.correlation import magnetisation_moments, structure_factor
    m1 = magnetisation_moments(mag[:, None], 12)[0]
    assert m1.shape == (1,) and abs(m1[0] - mag.mean() / 12) < 1e-15
    assert np.allclose(structure_factor(got[:, 0, :3], 12)[:, 0], mag.astype(np.float64) ** 2 / 12, rtol=0, atol=1e-12)


def test_magnetisation_moments_equal_plain_numpy():
    from pyisingmontecarlo_amd.correlation import magnetisation_moments

    N = 64
    m1, ma, m2, m4, u4 = magnetisation_moments(np.array([[N, -N], [-N, -N], [N, -N], [-N, -N]]), N)   # all m = +-1
    assert m1.tolist() == [0.0, -1.0] and ma.tolist() == [1.0, 1.0] and m2.tolist() == [1.0, 1.0] and m4.tolist() == [1.0, 1.0]
    assert u4.tolist() == [2 / 3, 2 / 3]                                   # exactly
    # m in {-1/2 (twice), +1/2 (twice), -1, +1}: <m> = 0, <|m|> = 2/3, <m^2> = 1/2, <m^4> = 3/8, U4 = 1 - (3/8) / (3/4) = 1/2
    m1, ma, m2, m4, u4 = magnetisation_moments(np.array([-32, -32, 32, 32, -64, 64])[:, None], N)
    assert (m1[0], m2[0], m4[0], u4[0]) == (0.0, 0.5, 0.375, 0.5) and ma[0] == pytest.approx(2 / 3, abs=1e-15)
    # a hand-made integer series against the definitions written out
    rng = np.random.default_rng(8)
    mag = rng.integers(-N, N + 1, (50, 3, 2))
    got = magnetisation_moments(mag, N)
    m = mag / N
    want = (m.mean(0), np.abs(m).mean(0), (m ** 2).mean(0), (m ** 4).mean(0), 1 - (m ** 4).mean(0) / (3 * (m ** 2).mean(0) ** 2))
    for g, w in zip(got, want):
        assert g.shape == (3, 2) and np.allclose(g, w, rtol=0, atol=1e-14)
    assert np.isnan(magnetisation_moments(np.zeros((3, 2)), N)[4]).all()   # no cumulant where <m^2> = 0


def test_structure_factor_closed_forms():
    from pyisingmontecarlo_amd.correlation import correlation_length, plane_classes, structure_factor

    L = 8
    N = L * L
    up = np.ones((1, N), dtype=bool)
    planes = XR.class_sums(up, plane_classes((L, L)), L)[0]             # [2 axes, L]: every plane sum is L
    S = structure_factor(planes, N)
    assert S.shape == (2, L) and np.allclose(S[:, 0], N, rtol=0, atol=1e-12) and np.allclose(S[:, 1:], 0, rtol=0, atol=1e-12)
    # a single cosine profile M_x = a cos(2 pi 2 x / L) lands in its own wave number (and its mirror): |a L / 2|^2 / N each
    a = 3.0
    x = np.arange(L)
    S = structure_factor(a * np.cos(2 * np.pi * 2 * x / L), N)
    want = np.zeros(L)
    want[[2, L - 2]] = (a * L / 2) ** 2 / N
    assert np.allclose(S, want, rtol=0, atol=1e-12)
    # leading axes are kept, and the rows averaged over samples feed correlation_length unchanged
    rng = np.random.default_rng(3)
    rows = rng.integers(-L, L + 1, (20, 5, L)) + 2 * L                   # [samples, replicas, x], a clear k = 0 peak
    S = structure_factor(rows, N)
    assert S.shape == (20, 5, L)
    mean = S.mean(axis=0)
    xi = correlation_length(mean[:, 0], mean[:, 1], L)
    assert xi.shape == (5,) and np.array_equal(xi, np.sqrt(mean[:, 0] / mean[:, 1] - 1.0) / (2.0 * np.sin(np.pi / L))) and (xi > 0).all()

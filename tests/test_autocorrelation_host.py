"""The lag ring without a device: the ring bookkeeping the launch uses (isingmc_host_autocorr_plan) against the
numpy restatement, correlation.autocorrelation / integrated_time on exact geometric input, and the Python surface."""
import inspect

import numpy as np
import pytest

import autocorrelation_reference as AR


@pytest.mark.parametrize("L", [1, 3, 4])
def test_plan_against_the_reference(capi, L):
    """an empty ring, a partly filled one, the first wrap and the second"""
    ring = AR.LagRing(L, 1)
    for taken in range(0, 2 * L + 2):
        assert ring.samples == taken
        slots, live, write, counts = capi.autocorr_plan(taken, L)
        r_slots, r_live, r_write, r_counts = ring.plan()
        assert slots.dtype == np.uint32 and counts.dtype == np.uint64
        assert (live, write) == (r_live, r_write) == (min(taken, L), taken % L)
        assert np.array_equal(slots, r_slots) and np.array_equal(counts, r_counts)
        # the slot that is written holds the oldest lag once the ring is full, and no live lag before
        assert (slots[L] == write) if taken >= L else (write not in slots[1:live + 1])
        assert len(set(slots[1:live + 1].tolist())) == live
        ring.add(np.zeros((1, 2), dtype=np.uint8))


def test_plan_refuses_lag_counts_out_of_range(capi):
    for L in (0, 257):
        with pytest.raises(ValueError, match="1 .. 256"):
            capi.autocorr_plan(3, L)
    assert capi.autocorr_plan(2 ** 40 + 5, 256)[3][256] == 2 ** 40 + 5 - 256


@pytest.mark.parametrize("rho", [0.0, 0.5, 0.9])
def test_integrated_time_on_geometric_input(rho):
    from pyisingmontecarlo_amd import correlation as K
    N, n = 1000, 10 ** 6
    corr = rho ** np.arange(257, dtype=np.float64)   # lags 0 .. 256
    tau, window = K.integrated_time(np.stack([corr, corr]))
    r_tau, r_window = AR.integrated_time(corr)
    assert r_window > 0 and window.dtype == np.int64 and list(window) == [r_window, r_window]
    assert np.all(np.abs(tau - r_tau) <= 1e-12 * abs(r_tau))
    t1, w1 = K.integrated_time(corr)   # one row, no leading axis
    assert int(w1) == r_window and abs(float(t1) - r_tau) <= 1e-12 * abs(r_tau)
    # the window rule itself, on the closed form tau(W) = 1/2 + rho (1 - rho^W) / (1 - rho)
    closed = [0.5 + rho * (1 - rho ** W) / (1 - rho) for W in range(1, 257)]
    assert r_window == next(W for W, t in zip(range(1, 257), closed) if W >= 6.0 * t)
    # autocorrelation(): integer sums back to C, NaN where a lag has no term
    counts = np.array([n - l if l < 200 else 0 for l in range(257)], dtype=np.uint64)
    diff = np.zeros((2, 257), dtype=np.uint64)
    diff[:, 1:200] = np.rint((1 - corr[1:200]) / 2 * N * counts[1:200].astype(np.float64)).astype(np.uint64)
    C = K.autocorrelation(diff, counts, N)
    assert C.shape == (2, 257) and np.all(C[:, 0] == 1.0) and np.all(np.isnan(C[:, 200:]))
    assert np.array_equal(C[:, 1:200], 1.0 - 2.0 * diff[:, 1:200].astype(np.float64) / (counts[1:200].astype(np.float64) * N))
    assert np.all(np.abs(C[:, 1:200] - corr[1:200]) <= 2.0 / (N * counts[1:200].astype(np.float64)) + 1e-15)


def test_integrated_time_without_a_window():
    from pyisingmontecarlo_amd import correlation as K
    corr = 0.99 ** np.arange(17, dtype=np.float64)   # 16 lags: tau(16) ~ 15.2, 16 < 6 tau
    tau, window = K.integrated_time(corr)
    r_tau, r_window = AR.integrated_time(corr)
    assert r_window == -1 and int(window) == -1
    assert abs(float(tau) - r_tau) <= 1e-12 * r_tau and abs(r_tau - (0.5 + corr[1:].sum())) < 1e-12
    rows = np.stack([corr, 0.5 ** np.arange(17.0)])   # a row with a window beside one without
    tau2, window2 = K.integrated_time(rows)
    assert list(window2) == [-1, AR.integrated_time(rows[1])[1]] and abs(tau2[1] - AR.integrated_time(rows[1])[0]) <= 1e-12


def test_python_surface(capi):
    import py_monte_carlo
    from pyisingmontecarlo_amd import correlation as K
    sig = py_monte_carlo.Lattice.run_monte_carlo_and_measure_variable_autocorrelation.__doc__.splitlines()[0]
    order = [sig.index(n + ":") for n in ("beta", "timesteps", "num_experiments", "sampling_wait_buffer", "sampling_freq", "max_lag", "connected")]
    assert order == sorted(order)
    assert "sampling_wait_buffer: " in sig and "None = None" in sig and "= 32" in sig and "connected: bool = False" in sig
    C = py_monte_carlo.ClassicIsing
    sig = C.set_measure_autocorrelation_every.__doc__.splitlines()[0]
    assert sig.index("k:") < sig.index("max_lag:") and "= 32" in sig
    assert hasattr(C, "get_measured_autocorrelation") and hasattr(C, "reset_measured_autocorrelation")
    lat = py_monte_carlo.Lattice([((0, 1), 1.0)])
    with pytest.raises(NotImplementedError, match="quantum"):   # the quantum name stays refused as it is
        lat.run_quantum_monte_carlo_and_measure_variable_autocorrelation(1.0, 10, 2)
    with pytest.raises(ValueError, match="max_lag"):
        lat.run_monte_carlo_and_measure_variable_autocorrelation(1.0, 10, 2, max_lag=0)
    with pytest.raises(ValueError, match="two samples"):
        lat.run_monte_carlo_and_measure_variable_autocorrelation(1.0, 1, 2)
    assert list(inspect.signature(capi.States.autocorrelation).parameters) == ["self", "n_lags"]
    for name in ("set_every", "sample", "get", "reset", "samples", "n_lags"):
        assert hasattr(capi.Autocorrelation, name), name
    assert isinstance(capi.Autocorrelation.samples, property) and isinstance(capi.Autocorrelation.n_lags, property)
    assert list(inspect.signature(K.autocorrelation).parameters) == ["diff", "counts", "nvars"]
    assert list(inspect.signature(K.integrated_time).parameters) == ["corr", "c"] and inspect.signature(K.integrated_time).parameters["c"].default == 6.0
    for sym in ("create", "set_every", "sample", "count", "get", "reset", "destroy"):
        assert "isingmc_autocorr_" + sym in capi.EXPORTED_SYMBOLS
    assert "isingmc_host_autocorr_plan" in capi.EXPORTED_SYMBOLS

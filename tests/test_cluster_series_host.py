"""The cluster series without a device: the 128-bit split of tests/cluster_series_reference.py, the restated rows
against the steps they restate, the counting rule of the room check against a brute-force walk, the float64 estimators, and the
improved-estimator identities on the restatement alone against exact enumeration."""
import numpy as np
import pytest

import cluster_reference as CR
import cluster_series_reference as SR
import icm_reference as IR
import packed_cluster_reference as PR
import packed_icm_reference as PIR

SERIES_SYMBOLS = ["isingmc_cluster_series_" + s for s in ("create", "count", "get", "reset", "destroy")]


def test_split_and_join_of_128_bit_sums():
    for x in (0, 1, SR.M64, SR.M64 + 1, (1 << 128) - 1, 65537 ** 4 + 65535 ** 4, (2 ** 32 - 2) ** 4):
        lo, hi = SR.split128(x)
        assert 0 <= lo <= SR.M64 and 0 <= hi <= SR.M64 and SR.join128(lo, hi) == x
    # the carry case of the device test: the low words of the two fourth powers add up to more than 2^64
    a, b = 65537 ** 4, 65535 ** 4
    assert (a & SR.M64) + (b & SR.M64) > SR.M64
    assert SR.row_of_sizes([65537, 0, 65535]) == (2, 65537, 131072, 8589934594, 51539607554, 2)
    assert SR.row_of_sizes([]) == (0, 0, 0, 0, 0, 0) and SR.row_of_sizes(np.ones(16, dtype=np.int64)) == (16, 1, 16, 16, 16, 0)
    with pytest.raises(AssertionError):
        SR.split128(1 << 128)


def test_room_rule_against_a_brute_force_count(capi):
    for k in (0, 1, 2, 3, 7, 10):
        for t0 in list(range(0, 23)) + [2 ** 32 - 2, 2 ** 40 + 5]:
            for n in (0, 1, 2, 3, 9, 10, 11, 41):
                want = sum(1 for t in range(t0, t0 + n) if k and t % k == k - 1)
                assert capi.nonlocal_steps(t0, n, k) == want, (t0, n, k)
    with pytest.raises(ValueError, match="2\\^64"):
        capi.nonlocal_steps(2 ** 64 - 1, 2, 1)


def test_surface(capi):
    """The entry points stand in include/isingmc_cluster_series.h, which isingmc.h includes: what that header declares is what the
    binding's table of it holds and what the library exports."""
    import ctypes
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "isingmc_cluster_series.h")).read()
    assert set(re.findall(r"\b(isingmc_[a-z0-9_]+)\s*\(", header)) == set(SERIES_SYMBOLS) == set(capi.CLUSTER_SERIES_SYMBOLS)
    assert '#include "isingmc_cluster_series.h"' in open(os.path.join(root, "include", "isingmc.h")).read()
    assert "isingmc_host_nonlocal_steps" in capi.EXPORTED_SYMBOLS
    so, bound = ctypes.CDLL(capi.LIB_PATH), capi.lib()
    for name in SERIES_SYMBOLS + ["isingmc_host_nonlocal_steps"]:
        assert hasattr(so, name), name
        assert getattr(bound, name).argtypes is not None, name
    for name in ("get", "count", "capacity", "reset", "close"):
        assert hasattr(capi.ClusterSeries, name)
    assert capi.ClusterSeries.get.__doc__ and capi.States.cluster_series.__doc__


def test_lattice_rows_restate_the_steps():
    rng = np.random.default_rng(3)
    for J in (-1.0, 1.0):
        spins = rng.integers(0, 2, (4, 64)).astype(np.uint8)
        for t, beta in ((0, 0.0), (5, 0.3), ((7 << 32) + 1, 0.6), (9, 50.0)):
            new, row = SR.sw_row(spins, 0xABCDEF0123, t, beta, J)
            want, n, largest = CR.sw_step(spins, 0xABCDEF0123, t, beta, J)
            assert np.array_equal(new, want) and row[:3] == (n, largest, 256)
            assert SR.join128(row[4], row[5]) >= row[3] and row[3] >= 256
    a, b = rng.integers(0, 2, (2, 4, 64)).astype(np.uint8)
    assert SR.icm_row(a, b)[:3] == IR.icm_step(a, b, 1, 0)[2]
    assert SR.icm_row(a, a) == (0, 0, 0, 0, 0, 0)
    assert SR.icm_row(a, 1 - a) == (1, 256, 256, 256 ** 2, 256 ** 4, 0)


def test_packed_rows_restate_the_steps():
    rng = np.random.default_rng(4)
    G = PR.Graph(*PR.triangular_lattice_edges(5, 5), 25)
    spins = rng.integers(0, 2, (32, 25)).astype(np.uint8)
    thr = [CR.bond_threshold(b, 1.0) for b in np.linspace(0.0, 0.6, 32)]
    new, rows = SR.pk_sw_step(G, spins, 11, 5, thr)
    want, clusters, largest = PR.sw_step(G, spins, 11, 5, thr)
    assert np.array_equal(new, want)
    assert [r[0] for r in rows] == clusters.tolist() and [r[1] for r in rows] == largest.tolist() and all(r[2] == 25 for r in rows)
    for bit in (0, 9, 31):
        assert SR.pk_sw_row(G, spins[bit], bit, 11, 5, thr[bit]) == rows[bit]
    assert rows[0] == (25, 1, 25, 25, 25, 0)   # beta = 0
    _, c, l, m = PIR.icm_step(G, spins, 11, 5, [True] * 16)
    for j in (0, 7, 15):
        assert SR.pk_icm_row(G, spins[2 * j], spins[2 * j + 1])[:3] == (c[j], l[j], m[j])


def test_cluster_estimators_in_float64():
    from pyisingmontecarlo_amd.correlation import cluster_estimators

    N = 2 ** 20
    sizes = [[N], [N // 2, N // 2], [1] * 16 + [N - 16]]
    rows = np.array([SR.row_of_sizes(s) for s in sizes], dtype=np.uint64)[:, None, :]   # [n = 3, C = 1, 6]
    chi, m2, m4, u4 = cluster_estimators(rows[..., 3], rows[..., 4], rows[..., 5], N)
    s2 = [sum(x * x for x in s) for s in sizes]
    s4 = [sum(x ** 4 for x in s) for s in sizes]
    assert chi.shape == (1,)
    assert chi[0] == pytest.approx(sum(s2) / 3 / N, rel=1e-14) and m2[0] == pytest.approx(sum(s2) / 3 / N ** 2, rel=1e-14)
    assert m4[0] == pytest.approx(sum(3 * a * a - 2 * b for a, b in zip(s2, s4)) / 3 / N ** 4, rel=1e-14)
    assert u4[0] == pytest.approx(1 - m4[0] / (3 * m2[0] ** 2), rel=1e-12)
    one = np.array([SR.row_of_sizes([N])], dtype=np.uint64)
    assert cluster_estimators(one[:, 3], one[:, 4], one[:, 5], N)[3] == pytest.approx(2 / 3)   # |m| = 1: U4 = 2/3


def tri_chain_moments(oracle, rows_of_step):
    """The chains of the estimator check: per chain the means of S2 and of 3 S2^2 - 2 S4 over the measured steps.  rows_of_step(t)
    -> (s2[chains], s4[chains]) as Python integers of the cluster step at timestep t."""
    a = np.zeros(PR.TRI_CHAINS)
    b = np.zeros(PR.TRI_CHAINS)
    for t in range(PR.TRI_THERM, PR.TRI_THERM + PR.TRI_STEPS):
        s2, s4 = rows_of_step(t)
        a += np.array([float(x) for x in s2])
        b += np.array([float(3 * x * x - 2 * y) for x, y in zip(s2, s4)])   # (exact integers below 2^53 on 16 sites)
    return a / PR.TRI_STEPS, b / PR.TRI_STEPS


def tri_z_values(exact, mean_s2, mean_m4):
    ea, eb, ej = PR.triangular_lattice_edges(4, 4, -1.0)
    ex = exact.enumerate_graph(ea, eb, ej, 16, PR.TRI_BETA)
    want_m4 = float((ex["probs"] * ex["mag"].astype(np.float64) ** 4).sum())
    z2 = (mean_s2.mean() - ex["M2"]) / (mean_s2.std(ddof=1) / np.sqrt(len(mean_s2)))
    z4 = (mean_m4.mean() - want_m4) / (mean_m4.std(ddof=1) / np.sqrt(len(mean_m4)))
    print(f"<S2> {mean_s2.mean():.4f} exact <M^2> {ex['M2']:.4f} z {z2:+.2f};  <3 S2^2 - 2 S4> {mean_m4.mean():.2f} exact <M^4> {want_m4:.2f} z {z4:+.2f}")
    return z2, z4


TRI_SERIES_SEED = PR.TRI_SEED + 0x5E


def test_improved_estimators_against_exact_enumeration(exact, oracle):
    """Periodic 4 x 4 triangular ferromagnet, beta = PR.TRI_BETA, a cluster step at every timestep (k = 1), PR.TRI_CHAINS seeded
    chains from the random start, on the restatement alone: per chain the means of S2 and of 3 S2^2 - 2 S4 over PR.TRI_STEPS steps
    after PR.TRI_THERM; <S2> against <M^2> and <3 S2^2 - 2 S4> against <M^4> of exact enumeration, standard errors from the spread
    across the chains, |z| <= 5.  Observed: z = +1.80 and z = +2.21 (tests/test_gpu_cluster_series.py repeats it on the device)."""
    ea, eb, ej = PR.triangular_lattice_edges(4, 4, -1.0)
    G = PR.Graph(ea, eb, ej, 16)
    seeds = oracle.make_seeds(TRI_SERIES_SEED, PR.TRI_CHAINS)
    _, states = oracle.pk_run(ea, eb, ej, 16, seeds, 0, betas=[])
    states = np.array(states, dtype=np.uint8)
    thr = [CR.bond_threshold(PR.TRI_BETA, G.jabs)] * 32
    groups = PR.TRI_CHAINS // 32
    series = {}
    for t in range(PR.TRI_THERM + PR.TRI_STEPS):
        s2, s4 = [], []
        for g in range(groups):
            rows_g = slice(32 * g, 32 * g + 32)
            states[rows_g], rows = SR.pk_sw_step(G, states[rows_g], int(seeds[32 * g]), t, thr)
            s2 += [r[3] for r in rows]
            s4 += [SR.join128(r[4], r[5]) for r in rows]
        series[t] = (s2, s4)
    z2, z4 = tri_z_values(exact, *tri_chain_moments(oracle, series.__getitem__))
    assert abs(z2) <= 5.0 and abs(z4) <= 5.0

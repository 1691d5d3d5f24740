"""The cluster series on the device: the rows of every non-local step bit for bit against the numpy restatement of
tests/cluster_series_reference.py on the checkerboard path and on both replica-packed families, for Swendsen-Wang steps and for
isoenergetic cluster moves; agreement with cluster_stats() / icm_stats(); a twin container without a series; invariance under how
a run is cut; degenerate cases with the 128-bit carry; the improved estimators against exact enumeration and against the
observable series; the refusals; the Python surface.

The reference rows are computed from the configurations a twin container WITHOUT a series holds right before each non-local step
(it runs the same timesteps one at a time); that the two containers walk the same trajectory is checked in every case, and that
the trajectory is the restatement's is what tests/test_gpu_cluster.py, test_gpu_packed_cluster.py, test_gpu_icm.py and
test_gpu_packed_icm.py pin."""
import numpy as np
import pytest

import cluster_reference as CR
import cluster_series_reference as SR
import packed_cluster_reference as PR
import packed_icm_reference as PIR
from test_cluster_series_host import TRI_SERIES_SEED, tri_chain_moments, tri_z_values

pytestmark = pytest.mark.gpu

BETA_C = 0.4407
CARRY_ROW = (2, 65537, 131072, 8589934594, 51539607554, 2)


@pytest.fixture
def force_packed(monkeypatch):
    monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")


def _got(series):
    """(timesteps, rows uint64[n, C, 6]) of the whole log."""
    out = series.get()
    return out[0], np.stack(out[1:], axis=-1)


def _walk(twin, T, beta, row_of_step, is_step):
    """The twin container through T timesteps, one at a time: (timesteps of the non-local steps, their reference rows [n, C, 6]);
    row_of_step(t, states before the step) -> the rows of all columns."""
    ts, rows = [], []
    for _ in range(T):
        t = twin.timestep
        if is_step(t):
            ts.append(t)
            rows.append(SR.rows_array(row_of_step(t, twin.states().astype(np.uint8))))
        twin.do_time_steps(1, beta)
    return np.array(ts, dtype=np.uint64), np.array(rows, dtype=np.uint64).reshape(len(ts), -1, 6)


def _same_trajectory(st, twin):
    assert st.timestep == twin.timestep
    assert np.array_equal(st.packed(), twin.packed()) and np.array_equal(st.energies(), twin.energies())


def _check_sw_stats(st, twin, rows):
    n, largest = st.cluster_stats()
    assert np.array_equal(n, rows[-1, :, 0]) and np.array_equal(largest, rows[-1, :, 1])
    n2, largest2 = twin.cluster_stats()
    assert np.array_equal(n, n2) and np.array_equal(largest, largest2)


def _check_icm_stats(st, twin, rows):
    got = st.icm_stats()
    for i in range(3):   # n_clusters, largest, and the sites column = minus_sites
        assert np.array_equal(got[i], rows[-1, :, i]), SR.COLUMNS[i]
    for a, b in zip(got, twin.icm_stats()):
        assert np.array_equal(a, b)


# ---- rows bit for bit, lattice ----------------------------------------------------------------------------------------------
def _lattice_pair(capi, exact, W, H, J, seeds, k, t0=0, betas=None, rng=None):
    ea, eb, ej = exact.square_lattice_edges(W, H, J, rng)
    g = capi.Graph(ea, eb, ej, W * H)
    out = []
    for _ in range(2):
        st = capi.States(g, seeds)
        st.timestep = t0
        if betas is not None:
            st.set_betas(betas)
        st.set_cluster_every(k)
        out.append(st)
    return out


def _lattice_sw_rows(W, H, J, seeds, beta_of):
    return lambda t, spins: [SR.sw_row(spins[r].reshape(H, W), int(s), t, beta_of(r), J)[1] for r, s in enumerate(seeds)]


@pytest.mark.parametrize("J", [-1.0, 1.0])
@pytest.mark.parametrize("beta", [0.2, BETA_C, 0.7])
@pytest.mark.parametrize("W,H", [(64, 4), (128, 64), (1024, 128)])
def test_lattice_rows_are_bit_exact(capi, exact, W, H, J, beta):
    """k = 1 from t = 0 (a row per timestep) and k = 3 from t0 = 1 (rows at t = 2 and 5 only, the timesteps column says so)."""
    seeds = capi.make_seeds(2000 + W + H, 2)
    for k, t0, T in ((1, 0, 2), (3, 1, 6)):
        st, twin = _lattice_pair(capi, exact, W, H, J, seeds, k, t0)
        series = st.cluster_series("sw", capacity=4)
        assert series.count == 0 and series.capacity == 4 and series.n_columns == 2
        st.do_time_steps(T, beta)
        ts_ref, ref = _walk(twin, T, beta, _lattice_sw_rows(W, H, J, seeds, lambda r: beta), lambda t: t % k == k - 1)
        ts, rows = _got(series)
        assert ts.tolist() == ts_ref.tolist() == ([0, 1] if k == 1 else [2, 5])
        assert np.array_equal(rows, ref)
        assert (rows[:, :, 2] == W * H).all()
        _same_trajectory(st, twin)
        _check_sw_stats(st, twin, rows)
        series.close()


def test_lattice_rows_with_per_replica_betas(capi, exact):
    W, H, J = 256, 64, -1.0
    betas = [0.2, BETA_C, 0.7]
    seeds = capi.make_seeds(77, 3)
    st, twin = _lattice_pair(capi, exact, W, H, J, seeds, 2, betas=betas)
    series = st.cluster_series()
    st.do_time_steps(4, None)
    ts_ref, ref = _walk(twin, 4, None, _lattice_sw_rows(W, H, J, seeds, lambda r: betas[r]), lambda t: t % 2 == 1)
    ts, rows = _got(series)
    assert ts.tolist() == [1, 3] and np.array_equal(rows, ref)
    assert rows[0, 0, 0] > rows[0, 2, 0]   # the hot replica has more clusters than the cold one
    _same_trajectory(st, twin)
    _check_sw_stats(st, twin, rows)


# ---- rows bit for bit, packed -------------------------------------------------------------------------------------------------
def _packed_pair(capi, G, seeds, k, kind="sw", replica_range=None, real=False):
    if real:
        g = capi.Graph(G.ea, G.eb, G.ej, nvars=G.nvars, stable_path=True)
    else:
        g = capi.Graph(G.ea, G.eb, G.ej, nvars=G.nvars, force_general=True)
    out = []
    for _ in range(2):
        st = capi.States(g, seeds, replica_range=replica_range)
        assert st.family == ("packed_real" if real else "packed_bitsliced")
        (st.set_cluster_every if kind == "sw" else st.set_icm_every)(k)
        out.append(st)
    return out


def _packed_sw_rows(G, seeds, beta, first=0):
    thr = CR.bond_threshold(beta, G.jabs)

    def rows(t, spins):
        return [SR.pk_sw_row(G, spins[r], (first + r) % 32, int(seeds[32 * ((first + r) // 32)]), t, thr) for r in range(len(spins))]
    return rows


@pytest.mark.parametrize("case", ["6^3 x 40", "8^3 J=+1 x 33", "6^3 shard [10, 52) of 70"])
def test_packed_rows_are_bit_exact(capi, exact, force_packed, case):
    """Cubic 6^3 with 40 replicas: padded colour classes and a partial group; 8^3 antiferromagnet: full classes; a replica_range
    shard that starts inside a group: the bits it does not own have no column and add nothing to the others."""
    L, J, R, rr = {"6^3 x 40": (6, -1.0, 40, None), "8^3 J=+1 x 33": (8, 1.0, 33, None), "6^3 shard [10, 52) of 70": (6, -1.0, 70, (10, 52))}[case]
    G = PR.Graph(*exact.cubic_lattice_edges(L, J), L ** 3)
    seeds = capi.make_seeds(91, R)
    beta, k, T = 0.2216, 2, 4
    st, twin = _packed_pair(capi, G, seeds, k, replica_range=rr)
    first, C = (rr[0], rr[1] - rr[0]) if rr else (0, R)
    series = st.cluster_series("sw")
    assert series.n_columns == C
    st.do_time_steps(T, beta)
    ts_ref, ref = _walk(twin, T, beta, _packed_sw_rows(G, seeds, beta, first), lambda t: t % k == k - 1)
    ts, rows = _got(series)
    assert ts.tolist() == [1, 3] and np.array_equal(rows, ref)
    assert (rows[:, :, 2] == L ** 3).all()
    _same_trajectory(st, twin)
    _check_sw_stats(st, twin, rows)


# ---- rows bit for bit, isoenergetic ---------------------------------------------------------------------------------------------
def test_lattice_icm_rows_are_bit_exact(capi, exact):
    """128 x 64 +-J, five replicas: two pairs and a last replica without a partner (no column)."""
    W, H, k, T, beta = 128, 64, 2, 4, 0.8
    ea, eb, ej = exact.square_lattice_edges(W, H, -1.0, np.random.default_rng(5))
    g = capi.Graph(ea, eb, ej, W * H)
    seeds = capi.make_seeds(12, 5)
    st, twin = capi.States(g, seeds), capi.States(g, seeds)
    for s in (st, twin):
        s.set_icm_every(k)
    series = st.cluster_series("icm")
    assert series.n_columns == 2
    st.do_time_steps(T, beta)
    ts_ref, ref = _walk(twin, T, beta, lambda t, sp: [SR.icm_row(sp[2 * p].reshape(H, W), sp[2 * p + 1].reshape(H, W)) for p in range(2)],
                        lambda t: t % k == k - 1)
    ts, rows = _got(series)
    assert ts.tolist() == [1, 3] and np.array_equal(rows, ref)
    assert (rows[:, :, 2] > 0).all() and (rows[:, :, 2] < W * H).all()
    _same_trajectory(st, twin)
    _check_icm_stats(st, twin, rows)


@pytest.mark.parametrize("family", ["bitsliced", "real"])
def test_packed_icm_rows_are_bit_exact(capi, exact, force_packed, family):
    """Cubic 6^3 +-J on the bit-sliced family (40 experiments: 16 pairs of a full group, 4 of a partial one); a Gaussian glass on
    cubic 4^3 on the real-coupling family."""
    if family == "bitsliced":
        G = PIR.Graph(*PIR.cubic_glass(exact, 6), 216)
    else:
        ea, eb, _ = exact.cubic_lattice_edges(4, -1.0)
        G = PIR.Graph(ea, eb, np.random.default_rng(8).normal(size=len(ea)), 64)
    R, k, T, beta = 40, 2, 4, 0.6
    seeds = capi.make_seeds(13, R)
    st, twin = _packed_pair(capi, G, seeds, k, kind="icm", real=family == "real")
    series = st.cluster_series("icm")
    assert series.n_columns == R // 2
    st.do_time_steps(T, beta)
    ts_ref, ref = _walk(twin, T, beta, lambda t, sp: [SR.pk_icm_row(G, sp[2 * p], sp[2 * p + 1]) for p in range(R // 2)], lambda t: t % k == k - 1)
    ts, rows = _got(series)
    assert ts.tolist() == [1, 3] and np.array_equal(rows, ref)
    _same_trajectory(st, twin)
    _check_icm_stats(st, twin, rows)


# ---- cut invariance ---------------------------------------------------------------------------------------------------------------
def _cuts(make, T, beta, kind, small_workspace):
    """One call, the same run in pieces, and the same run with a workspace that holds one or two items per batch."""
    logs = []
    for pieces, workspace in (((T,), None), ((3, T - 3), None), ((T,), small_workspace)):
        st = make()
        if workspace:
            st.set_option("cluster_workspace_bytes", workspace)
        series = st.cluster_series(kind)
        for n in pieces:
            st.do_time_steps(n, beta)
        logs.append(_got(series) + (st.packed(),))
    for ts, rows, packed in logs[1:]:
        assert np.array_equal(ts, logs[0][0]) and np.array_equal(rows, logs[0][1]) and np.array_equal(packed, logs[0][2])
    assert len(logs[0][0]) == T // 2
    return logs[0]


def test_rows_do_not_depend_on_how_the_run_is_cut_lattice(capi, exact):
    W, H = 128, 64
    seeds = capi.make_seeds(31, 6)
    g = capi.Graph(*exact.square_lattice_edges(W, H, -1.0), W * H)

    def make(kind):
        def f():
            st = capi.States(g, seeds)
            (st.set_cluster_every if kind == "sw" else st.set_icm_every)(2)
            return st
        return f
    words = 2 * W * H + W * H // 16 + W * H // 32   # labels, sizes, bonds, flip table of one replica or pair
    _cuts(make("sw"), 8, BETA_C, "sw", 2 * 4 * words)    # three batches of two replicas
    _cuts(make("icm"), 8, BETA_C, "icm", 4 * words)      # three batches of one pair


def test_rows_do_not_depend_on_how_the_run_is_cut_packed(capi, exact, force_packed):
    G = PIR.Graph(*PIR.cubic_glass(exact, 6), 216)
    seeds = capi.make_seeds(32, 70)   # three groups
    _cuts(lambda: _packed_pair(capi, G, seeds, 2)[0], 6, 0.5, "sw", 1)                 # a group per batch
    _cuts(lambda: _packed_pair(capi, G, seeds, 2, kind="icm")[0], 6, 0.5, "icm", 1)


# ---- degenerate cases -------------------------------------------------------------------------------------------------------------
def test_beta_zero_every_site_is_a_cluster(capi, exact, force_packed):
    W, H = 64, 4
    st = capi.States(capi.Graph(*exact.square_lattice_edges(W, H, -1.0), W * H), capi.make_seeds(1, 3))
    st.set_cluster_every(1)
    series = st.cluster_series()
    st.do_time_steps(2, 0.0)
    assert (_got(series)[1] == np.array([256, 1, 256, 256, 256, 0], dtype=np.uint64)).all()
    G = PR.Graph(*exact.cubic_lattice_edges(6, -1.0), 216)
    st = _packed_pair(capi, G, capi.make_seeds(2, 40), 1)[0]
    series = st.cluster_series()
    st.do_time_steps(2, 0.0)
    assert (_got(series)[1] == np.array([216, 1, 216, 216, 216, 0], dtype=np.uint64)).all()


def _two_clusters():
    """1024 x 128: flat site index i < 65535 or i >= 131070 up, the rest down -- with every satisfied bond active, two clusters of
    65537 and 65535 sites (the two last sites join the up cluster through the periodic wrap)."""
    i = np.arange(1024 * 128)
    return ((i < 65535) | (i >= 131070)).astype(np.uint8)


def test_the_carry_into_the_high_word_lattice(capi, exact):
    """Ferromagnet, beta = 50: 65537^4 + 65535^4 -- the low words of the two fourth powers add up to more than 2^64."""
    W, H = 1024, 128
    st = capi.States(capi.Graph(*exact.square_lattice_edges(W, H, -1.0), W * H), capi.make_seeds(3, 2), initial_state=_two_clusters())
    st.set_cluster_every(1)
    series = st.cluster_series()
    st.do_time_steps(1, 50.0)
    rows = _got(series)[1]
    assert rows.shape == (1, 2, 6) and (rows == np.array(CARRY_ROW, dtype=np.uint64)).all()
    assert SR.row_of_sizes([65537, 65535]) == CARRY_ROW


def test_the_carry_into_the_high_word_packed(capi, exact, force_packed):
    """The same configuration on the same lattice as a general graph on the replica-packed path."""
    W, H = 1024, 128
    ea, eb, ej = exact.square_lattice_edges(W, H, -1.0)
    g = capi.Graph(ea, eb, ej, nvars=W * H, force_general=True)
    st = capi.States(g, capi.make_seeds(3, 2), initial_state=_two_clusters())
    assert st.family == "packed_bitsliced"
    st.set_cluster_every(1)
    series = st.cluster_series()
    st.do_time_steps(1, 50.0)
    rows = _got(series)[1]
    assert rows.shape == (1, 2, 6) and (rows == np.array(CARRY_ROW, dtype=np.uint64)).all()
    n, largest = st.cluster_stats()
    assert n.tolist() == [2, 2] and largest.tolist() == [65537, 65537]


# ---- physics ----------------------------------------------------------------------------------------------------------------------
def test_improved_estimators_against_exact_enumeration(capi, exact, oracle, force_packed):
    """The chains of tests/test_cluster_series_host.py::test_improved_estimators_against_exact_enumeration on the device, one
    enqueue-only run and one read: periodic 4 x 4 triangular ferromagnet, beta = PR.TRI_BETA, k = 1, PR.TRI_CHAINS chains; <S2>
    against <M^2> and <3 S2^2 - 2 S4> against <M^4> of exact enumeration, |z| <= 5.  On the CPU restatement: z = +1.80 and
    z = +2.21; a bit-exact device gives the same."""
    ea, eb, ej = PR.triangular_lattice_edges(4, 4, -1.0)
    G = PR.Graph(ea, eb, ej, 16)
    T = PR.TRI_THERM + PR.TRI_STEPS
    st = _packed_pair(capi, G, capi.make_seeds(TRI_SERIES_SEED, PR.TRI_CHAINS), 1)[0]
    series = st.cluster_series(capacity=T)
    st.do_time_steps(T, PR.TRI_BETA)
    ts, _, _, _, s2, s4_lo, s4_hi = series.get()
    assert ts.tolist() == list(range(T))
    z2, z4 = tri_z_values(exact, *tri_chain_moments(oracle, lambda t: ([int(x) for x in s2[t]], [SR.join128(a, b) for a, b in zip(s4_lo[t], s4_hi[t])])))
    assert abs(z2) <= 5.0 and abs(z4) <= 5.0
    assert abs(z2 - 1.80) < 0.01 and abs(z4 - 2.21) < 0.01   # the restatement's chains, bit for bit


def test_s2_agrees_with_m2_of_the_observable_series(capi, exact):
    """64 x 16 torus at beta_c, k = 1, 32 chains, 50 + 400 steps: per chain <S2> from the cluster series and <M^2> from an observable
    series of the same run (a row behind every step); the difference of the two means over the chains against the combined
    standard error, |z| <= 5."""
    W, H, R, therm, T = 64, 16, 32, 50, 450
    st = capi.States(capi.Graph(*exact.square_lattice_edges(W, H, -1.0), W * H), capi.make_seeds(41, R))
    st.set_cluster_every(1)
    clusters = st.cluster_series(capacity=T)
    obs = st.observable_series(energy=False, capacity=T)
    obs.set_every(1)
    st.do_time_steps(T, BETA_C)
    s2 = clusters.get()[4][therm:].astype(np.float64).mean(axis=0)
    m2 = (obs.get()[2][therm:].astype(np.float64) ** 2).mean(axis=0)
    se = np.sqrt(s2.var(ddof=1) / R + m2.var(ddof=1) / R)
    z = (s2.mean() - m2.mean()) / se
    print(f"<S2> {s2.mean():.1f} +- {s2.std(ddof=1) / np.sqrt(R):.1f}   <M^2> {m2.mean():.1f} +- {m2.std(ddof=1) / np.sqrt(R):.1f}   z {z:+.2f}")
    assert abs(z) <= 5.0
    from pyisingmontecarlo_amd.correlation import cluster_estimators
    got = clusters.get()
    chi = cluster_estimators(got[4][therm:], got[5][therm:], got[6][therm:], W * H)[0]
    assert np.allclose(chi, s2 / (W * H), rtol=1e-13)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_container_and_the_log_as_they_were(capi, exact, monkeypatch):
    W, H = 64, 4
    g = capi.Graph(*exact.square_lattice_edges(W, H, -1.0), W * H)
    st = capi.States(g, capi.make_seeds(5, 4))
    st.set_cluster_every(1)
    series = st.cluster_series(capacity=2)
    with pytest.raises(ValueError, match="one cluster series per container"):
        st.cluster_series()
    with pytest.raises(ValueError, match="kind must be"):
        st.cluster_series("wolff")
    # a full log: refused before anything is enqueued
    before = st.packed()
    with pytest.raises(ValueError, match="would run full: the call takes 3 non-local steps and the log has room for 2"):
        st.do_time_steps(3, 0.3)
    assert st.timestep == 0 and series.count == 0 and np.array_equal(st.packed(), before)
    st.do_time_steps(2, 0.3)
    assert series.count == 2
    with pytest.raises(ValueError, match="would run full"):
        st.do_time_steps(1, 0.3)
    ts, rows = _got(series)
    assert ts.tolist() == [0, 1] and st.timestep == 2
    # append, population annealing, ladder attach
    with pytest.raises(ValueError, match="a cluster series is live"):
        st.append(99)
    st.set_cluster_every(0)   # (so that the sentences below are the series' own)
    with pytest.raises(ValueError, match="a cluster series is live"):
        st.pa_resample(0.1, 1, 0)
    with pytest.raises(ValueError, match="a cluster series is live"):
        st.pa_run([0.1, 0.2], 1, 1)
    with pytest.raises(ValueError, match="a cluster series is live"):
        st.pt_attach(np.linspace(0.1, 0.4, 4), 0, 4, 1, 7)
    assert st.count == 4 and st.timestep == 2
    ts2, rows2 = _got(series)
    assert np.array_equal(ts, ts2) and np.array_equal(rows, rows2)
    # the container goes on: reset, run, read; and without the series everything is allowed again
    st.set_cluster_every(1)
    series.reset()
    assert series.count == 0
    st.do_time_steps(2, 0.3)
    assert _got(series)[0].tolist() == [2, 3]
    series.close()
    st.append(99)
    assert st.count == 5
    with pytest.raises(ValueError, match="one non-local move at a time"):   # Swendsen-Wang steps are on: no isoenergetic moves here
        st.cluster_series("icm")
    again = st.cluster_series()
    assert again.n_columns == 5
    # kinds the container cannot take
    monkeypatch.setenv("ISINGMC_DISABLE_PACKED", "1")
    monkeypatch.setenv("ISINGMC_DISABLE_REAL", "1")
    csr = capi.States(capi.Graph(*exact.cubic_lattice_edges(4, -1.0), nvars=64, force_general=True), capi.make_seeds(1, 2))
    with pytest.raises(ValueError, match="cluster updates need a container"):
        csr.cluster_series("sw")
    with pytest.raises(ValueError, match="isoenergetic cluster moves need a container"):
        csr.cluster_series("icm")
    glass = capi.States(capi.Graph(*exact.square_lattice_edges(W, H, -1.0, np.random.default_rng(1)), W * H), capi.make_seeds(1, 3))
    with pytest.raises(ValueError, match="one coupling sign only"):
        glass.cluster_series("sw")
    glass.cluster_series("icm").close()
    with pytest.raises(ValueError, match="larger than the option cluster_series_bytes"):
        glass.cluster_series("icm", capacity=2 ** 40)


# ---- Python surface -----------------------------------------------------------------------------------------------------------------
def test_python_surface(capi, exact):
    import py_monte_carlo
    from pyisingmontecarlo_amd.correlation import cluster_estimators

    W, H, beta, R, T = 64, 16, BETA_C, 4, 12
    ea, eb, ej = exact.square_lattice_edges(W, H, -1.0)
    # Lattice: one enqueue-only run with the Lattice's cluster period, one read
    lat = py_monte_carlo.Lattice.from_arrays(ea, eb, ej, seed_gen=5)
    with pytest.raises(ValueError, match="cluster"):
        lat.run_monte_carlo_and_measure_clusters(beta, T, R)
    lat.set_cluster_update_every(2)
    out = lat.run_monte_carlo_and_measure_clusters(beta, T - 4, R, thermalization_time=4)   # 4 + 8 timesteps, the rows from t = 4 on
    st = capi.States(capi.Graph(ea, eb, ej, W * H), lat.make_seeds(R))
    st.set_cluster_every(2)
    series = st.cluster_series()
    st.do_time_steps(T, beta)
    want = series.get()
    keep = want[0] >= 4
    assert len(out) == 7 and out[0].tolist() == want[0][keep].tolist() == [5, 7, 9, 11]
    for a, b in zip(out[1:], want[1:]):
        assert a.dtype == np.uint64 and a.shape == (4, R) and np.array_equal(a, b[keep])
    # ClassicIsing: persistent replicas; the kind follows whichever period is on
    edges = [((int(a), int(b)), float(j)) for a, b, j in zip(ea, eb, ej)]
    ci = py_monte_carlo.ClassicIsing(edges, None, R, 9)
    with pytest.raises(ValueError, match="neither"):
        ci.set_measure_clusters()
    ci.set_cluster_update_every(1)
    ci.set_measure_clusters(capacity=8)
    ci.run_monte_carlo(beta, 3)
    got = ci.get_measured_clusters()
    assert len(got) == 7 and got[0].tolist() == [0, 1, 2] and got[4].shape == (3, R) and (got[3] == W * H).all()
    chi, m2, m4, u4 = cluster_estimators(got[4], got[5], got[6], W * H)
    assert chi.shape == (R,) and np.allclose(m2, got[4].astype(np.float64).mean(axis=0) / (W * H) ** 2) and (u4 <= 2 / 3 + 1e-12).all()
    ci.reset_measured_clusters()
    assert ci.get_measured_clusters()[0].size == 0
    ci.run_monte_carlo(beta, 2)
    assert ci.get_measured_clusters()[0].tolist() == [3, 4]

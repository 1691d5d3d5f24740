"""Swendsen-Wang cluster steps on the device against the numpy restatement of tests/cluster_reference.py
(bit-exact: packed words, energies, cluster statistics), their invariances, degenerate cases, refusals, and the physics at
beta_c against Kaufman's exact energy."""
import numpy as np
import pytest

import cluster_reference as CR

pytestmark = pytest.mark.gpu

BETA_C = 0.4407


def _graph(capi, exact, W, H, J=-1.0, **kw):
    ea, eb, ej = exact.square_lattice_edges(W, H, J)
    return capi.Graph(ea, eb, ej, W * H, **kw)


def _check_against_reference(capi, oracle, st, W, H, J, seeds, start, t0, betas, k, per_replica_betas=None, energies=None):
    """st has run len(betas) timesteps from `start` (bool[R, N]) at t0: compare everything with the restatement."""
    lat = oracle.Lat(W, H, abs(J), 1 if J > 0 else 0)
    packed, e_now = st.packed(), st.energies()
    stats = st.cluster_stats() if k and any((t0 + n) % k == k - 1 for n in range(len(betas))) else None
    for r, seed in enumerate(seeds):
        b = betas if per_replica_betas is None else [per_replica_betas[r]] * len(betas)
        spins, e_ref, ref_stats = CR.run(W, H, J, int(seed), start[r].astype(np.uint8), t0, b, k)
        assert np.array_equal(packed[r], lat.pack(spins.ravel())), f"replica {r}: configurations differ"
        assert e_now[r] == e_ref[-1]
        if energies is not None:
            assert np.array_equal(energies[r], e_ref), f"replica {r}: per-step energies differ"
        if stats is not None:
            assert (int(stats[0][r]), int(stats[1][r])) == ref_stats, f"replica {r}: cluster statistics differ"


@pytest.mark.parametrize("J", [-1.0, 1.0])
@pytest.mark.parametrize("beta", [0.2, BETA_C, 0.7])
@pytest.mark.parametrize("W,H", [(64, 4), (128, 64), (256, 64), (1024, 128)])
def test_cluster_steps_are_bit_exact(capi, oracle, exact, W, H, J, beta):
    """k = 1 for 6 steps and k = 3 for 9 timesteps (Metropolis sweeps and cluster steps interleaved), 3 replicas, random starts;
    1024 x 128 has several tiles in both directions."""
    g = _graph(capi, exact, W, H, J)
    seeds = capi.make_seeds(1000 + W + H, 3)
    for k, T in ((1, 6), (3, 9)):
        st = capi.States(g, seeds)
        st.set_cluster_every(k)
        assert st.cluster_every == k
        start = st.states()
        e = st.do_time_steps(T, beta, per_step_energies=True)
        assert st.timestep == T
        _check_against_reference(capi, oracle, st, W, H, J, seeds, start, 0, [beta] * T, k, energies=e)


def test_cluster_steps_with_per_replica_betas_and_a_schedule(capi, oracle, exact):
    W, H, J = 256, 64, -1.0
    g = _graph(capi, exact, W, H, J)
    seeds = capi.make_seeds(77, 3)
    st = capi.States(g, seeds)
    st.set_cluster_every(2)
    start = st.states()
    per_replica = [0.2, BETA_C, 0.7]
    st.set_betas(per_replica)
    st.do_time_steps(6, None)
    _check_against_reference(capi, oracle, st, W, H, J, seeds, start, 0, [0.0] * 6, 2, per_replica_betas=per_replica)
    st.set_betas(None)
    mid = st.states()
    schedule = list(np.linspace(0.1, 0.8, 5))   # an annealing schedule: every timestep its own beta
    e = st.do_time_steps(5, schedule, per_step_energies=True)
    _check_against_reference(capi, oracle, st, W, H, J, seeds, mid, 6, schedule, 2, energies=e)


def test_cluster_steps_through_run_sampling(capi, oracle, exact):
    W, H, J, beta = 128, 64, -1.0, BETA_C
    g = _graph(capi, exact, W, H, J)
    seeds = capi.make_seeds(78, 3)
    st = capi.States(g, seeds)
    st.set_cluster_every(3)
    start = st.states()
    energies, states = st.run_sampling(beta, 2, 2, 4)   # thermalise 2, then 4 samples 2 timesteps apart: t = 4, 6, 8, 10
    for r, seed in enumerate(seeds):
        for n, T in enumerate((4, 6, 8, 10)):
            spins, e_ref, _ = CR.run(W, H, J, int(seed), start[r].astype(np.uint8), 0, [beta] * T, 3)
            assert np.array_equal(states[r, n], spins.ravel().astype(bool)) and energies[r, n] == e_ref[-1]
    assert st.timestep == 10


def test_cluster_steps_through_the_python_lattice(capi, oracle, exact):
    import py_monte_carlo

    W, H, J, beta, R, T = 128, 64, -1.0, BETA_C, 3, 6
    ea, eb, ej = exact.square_lattice_edges(W, H, J)
    lat = py_monte_carlo.Lattice.from_arrays(ea, eb, ej, seed_gen=5)
    start = np.random.default_rng(3).random(W * H) < 0.5
    lat.set_initial_state([bool(b) for b in start])
    assert lat.engine_info()["cluster_update_every"] == 0
    lat.set_cluster_update_every(2)
    assert lat.engine_info()["cluster_update_every"] == 2
    energies, states = lat.run_monte_carlo(beta, T, R)
    for r, seed in enumerate(lat.make_seeds(R)):
        spins, e_ref, _ = CR.run(W, H, J, int(seed), start.astype(np.uint8), 0, [beta] * T, 2)
        assert np.array_equal(states[r], spins.ravel().astype(bool)) and energies[r] == e_ref[-1]
    plain = py_monte_carlo.Lattice.from_arrays(ea, eb, ej, seed_gen=5)
    plain.set_initial_state([bool(b) for b in start])
    assert not np.array_equal(plain.run_monte_carlo(beta, T, R)[1], states)   # the default chain has no cluster steps
    ci = py_monte_carlo.ClassicIsing([((int(a), int(b)), float(j)) for a, b, j in zip(ea, eb, ej)], None, 2, 9)
    ci.set_cluster_update_every(1)
    ci.run_monte_carlo(beta, 3)
    cubic = py_monte_carlo.ClassicIsing([((int(a), int(b)), float(j)) for a, b, j in zip(*exact.cubic_lattice_edges(6))], None, 2, 9)
    with pytest.raises(ValueError, match="general-graph"):
        cubic.set_cluster_update_every(1)


def test_results_do_not_depend_on_how_the_run_is_cut(capi, exact, monkeypatch):
    W, H, J, beta, T = 1024, 128, -1.0, BETA_C, 6
    g = _graph(capi, exact, W, H, J)
    seeds = capi.make_seeds(31, 40)

    def fresh(n=40, k=3):
        st = capi.States(g, seeds[:n])
        st.set_cluster_every(k)
        return st

    whole = fresh()
    e_whole = whole.do_time_steps(T, beta, per_step_energies=True)
    ref, ref_stats = whole.packed(), whole.cluster_stats()
    # 6 timesteps in one call against 2 + 4
    split = fresh()
    e_split = np.concatenate([split.do_time_steps(2, beta, per_step_energies=True), split.do_time_steps(4, beta, per_step_energies=True)], axis=1)
    assert np.array_equal(split.packed(), ref) and np.array_equal(e_split, e_whole)
    # stop after 3 timesteps; a new container takes the configurations and the clock and resumes
    first = fresh()
    first.do_time_steps(3, beta)
    resumed = fresh()
    for r, spins in enumerate(first.states()):
        resumed.set_state(r, spins)
    resumed.timestep = 3
    resumed.do_time_steps(3, beta)
    assert np.array_equal(resumed.packed(), ref)
    # one replica alone is replica 0 of the forty
    alone = fresh(1)
    alone.do_time_steps(T, beta)
    assert np.array_equal(alone.packed()[0], ref[0])
    assert [int(a[0]) for a in alone.cluster_stats()] == [int(a[0]) for a in ref_stats]
    # one replica per batch of the cluster step's workspace against the default budget
    small = fresh()
    small.set_option("cluster_workspace_bytes", 1)
    small.do_time_steps(T, beta)
    assert np.array_equal(small.packed(), ref)
    assert all(np.array_equal(a, b) for a, b in zip(small.cluster_stats(), ref_stats))
    # the device fan-out of the Python Lattice
    import py_monte_carlo
    ea, eb, ej = exact.square_lattice_edges(256, 64, J)
    one = py_monte_carlo.Lattice.from_arrays(ea, eb, ej, seed_gen=4)
    one.set_cluster_update_every(2)
    monkeypatch.setenv("ISINGMC_DEVICES", "0,0")
    two = py_monte_carlo.Lattice.from_arrays(ea, eb, ej, seed_gen=4)
    two.set_cluster_update_every(2)
    assert two.get_devices() == [0, 0]
    a, b = one.run_monte_carlo(beta, T, 40), two.run_monte_carlo(beta, T, 40)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_degenerate_cases_span_every_tile_border(capi, exact):
    W, H = 1024, 128
    N = W * H
    seeds = capi.make_seeds(8, 3)
    ferro = _graph(capi, exact, W, H, -1.0)
    # beta = 0: no bond is active, every site is its own cluster
    st = capi.States(ferro, seeds)
    st.set_cluster_every(1)
    with pytest.raises(ValueError, match="no cluster step"):
        st.cluster_stats()
    st.do_time_steps(1, 0.0)
    n, largest = st.cluster_stats()
    assert n.tolist() == [N] * 3 and largest.tolist() == [1] * 3
    # beta = 20 from all-up: every bond is active, one cluster across every tile border and both wraps
    st = capi.States(ferro, seeds, initial_state=np.ones(N, np.uint8))
    st.set_cluster_every(1)
    st.do_time_steps(3, 20.0)
    n, largest = st.cluster_stats()
    assert n.tolist() == [1] * 3 and largest.tolist() == [N] * 3
    s = st.states()
    assert all(row.all() or not row.any() for row in s)
    # the antiferromagnet from the Neel state
    y, x = np.divmod(np.arange(N), W)
    anti = _graph(capi, exact, W, H, 1.0)
    st = capi.States(anti, seeds, initial_state=((x + y) & 1).astype(np.uint8))
    st.set_cluster_every(1)
    st.do_time_steps(3, 20.0)
    n, largest = st.cluster_stats()
    assert n.tolist() == [1] * 3 and largest.tolist() == [N] * 3
    neel = ((x + y) & 1).astype(bool)
    assert all(np.array_equal(row, neel) or np.array_equal(row, ~neel) for row in st.states())
    assert st.energies().tolist() == [-2.0 * N] * 3


@pytest.mark.parametrize("k", [1, 5])
def test_energy_at_the_critical_point_against_kaufman(capi, exact, k):
    """256^2 ferromagnet at beta = 0.4407, 64 seeded replicas from the all-up state, cluster_every = k: the lengths of the CPU
    check on 64 x 4 (cluster_reference.SAMPLING_THERM / SAMPLING_STEPS timesteps, unscaled); <E> per replica over the measured
    steps against Kaufman's exact finite-torus energy, standard error across the replicas, |z| <= 4."""
    L, R = 256, 64
    g = _graph(capi, exact, L, L, -1.0)
    st = capi.States(g, capi.make_seeds(2024 + k, R), initial_state=np.ones(L * L, np.uint8))
    st.set_cluster_every(k)
    st.do_time_steps(CR.SAMPLING_THERM, BETA_C)
    e = st.do_time_steps(CR.SAMPLING_STEPS, BETA_C, per_step_energies=True)
    means = e.mean(axis=1)
    want = exact.kaufman_energy(L, L, BETA_C)
    z = (means.mean() - want) / (means.std(ddof=1) / np.sqrt(R))
    print(f"k = {k}: <E>/N {means.mean() / L ** 2:.6f} exact {want / L ** 2:.6f} z {z:+.2f}")
    assert abs(z) <= 4.0


def test_unsupported_containers_are_refused_and_stay_usable(capi, exact):
    W, H = 256, 64
    N = W * H
    ea, eb, ej = exact.square_lattice_edges(W, H, -1.0)
    y, x = np.divmod(np.arange(N), W)
    right = np.arange(len(ea)) % 2 == 0
    cases = {
        "field": capi.Graph(ea, eb, ej, N, biases=np.full(N, 0.5)),
        "open": capi.Graph(*[a[~(right & (np.repeat(x, 2) == W - 1))] for a in (ea, eb, ej)], N),
        "sign": capi.Graph(*exact.square_lattice_edges(W, H, -1.0, np.random.default_rng(1)), N),
        "anisotropic": capi.Graph(ea, eb, np.where(right, -1.0, -2.0), N),
        "general-graph": capi.Graph(*exact.cubic_lattice_edges(8), 512),
    }
    seeds = capi.make_seeds(3, 2)
    for reason, g in cases.items():
        st = capi.States(g, seeds)
        with pytest.raises(ValueError, match=reason):
            st.set_cluster_every(2)
        assert st.cluster_every == 0
        st.do_time_steps(2, 0.4)   # still usable
        assert st.timestep == 2
    g = capi.Graph(ea, eb, ej, N)
    st = capi.States(g, seeds)
    st.set_cluster_every(4)
    assert not st.pt_can_attach(2, 0, 2, 1)
    with pytest.raises(ValueError, match="cluster"):
        st.pt_attach([0.3, 0.5], 0, 2, 1, 7)
    st.set_cluster_every(0)
    st.pt_attach([0.3, 0.5], 0, 2, 1, 7)
    with pytest.raises(ValueError, match="ladder"):
        st.set_cluster_every(3)
    assert st.cluster_every == 0
    st.pt_detach()
    st.set_cluster_every(3)
    assert st.cluster_every == 3
    st.do_time_steps(3, 0.4)
    assert int(st.cluster_stats()[1][0]) >= 1


def test_full_size_cluster_steps(capi, exact):
    """4096^2 x 8 at beta_c, two cluster steps: energies against the f64 Hamiltonian of the returned configurations (exact for
    integer J), the statistics within their bounds, and the number of clusters of replica 0's first step against the restatement."""
    L, R = 4096, 8
    N = L * L
    g = _graph(capi, exact, L, L, -1.0)
    seeds = capi.make_seeds(99, R)
    st = capi.States(g, seeds)
    st.set_cluster_every(1)
    start0 = st.states()[0].astype(np.uint8).reshape(L, L)
    st.do_time_steps(1, BETA_C)
    n1, _ = st.cluster_stats()
    ref_spins, ref_n, ref_largest = CR.sw_step(start0, int(seeds[0]), 0, BETA_C, -1.0)
    assert int(n1[0]) == ref_n
    assert np.array_equal(st.states()[0], ref_spins.ravel().astype(bool))
    e = st.do_time_steps(1, BETA_C, per_step_energies=True)
    n, largest = st.cluster_stats()
    assert all(1 <= int(v) <= N for v in largest) and all(1 <= int(v) <= N for v in n)
    for r, spins in enumerate(st.states()):
        assert e[r, 0] == CR.energy(spins.astype(np.uint8).reshape(L, L), -1.0)
    assert np.array_equal(st.energies(), e[:, 0])

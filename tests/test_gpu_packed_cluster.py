"""Swendsen-Wang cluster steps on replica-packed bit-sliced containers on the device against the numpy
restatement of tests/packed_cluster_reference.py (bit-exact: packed words with their cleared padding, energies after every
timestep, cluster statistics), their invariances, the refusals, and the physics against exact enumeration and against
Metropolis-only chains."""
import numpy as np
import pytest

import packed_cluster_reference as PR

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _force_packed(monkeypatch):
    monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")


def _states(capi, G, seeds, k, replica_range=None, initial=None):
    g = capi.Graph(G.ea, G.eb, G.ej, nvars=G.nvars, force_general=True)
    st = capi.States(g, seeds, initial_state=initial, replica_range=replica_range)
    assert st.family == "packed_bitsliced"
    st.set_cluster_every(k)
    assert st.cluster_every == k
    return st


def _check(capi, G, R, T, k, beta=None, beta_replica=None, seed=77):
    """R experiments from the random start, T timesteps with cluster_every = k, against the restatement."""
    seeds = capi.make_seeds(seed, R)
    st = _states(capi, G, seeds, k)
    if beta_replica is not None:
        st.set_betas(beta_replica)
        eps = st.do_time_steps(T, None, per_step_energies=True)
        ref, e_ref, stats_ref = PR.run(G, seeds, T, k, beta_replica=beta_replica)
    else:
        betas = [beta] * T if np.ndim(beta) == 0 else list(beta)
        eps = st.do_time_steps(T, beta, per_step_energies=True)
        ref, e_ref, stats_ref = PR.run(G, seeds, T, k, betas=betas)
    assert st.timestep == T
    _compare(st, G, ref, e_ref, stats_ref, eps)
    return st


def _compare(st, G, ref, e_ref, stats_ref, eps=None, first=0):
    R = st.count
    packed = st.packed()
    assert packed.shape[1] == G.n_pos // 32
    for r in range(R):
        assert np.array_equal(packed[r], G.pack(ref[first + r])), f"replica {r}: configurations differ"
    assert np.array_equal(st.states().astype(np.uint8), ref[first:first + R])
    assert np.array_equal(st.energies(), e_ref[first:first + R, -1])
    if eps is not None:
        assert np.array_equal(eps, e_ref[first:first + R]), "per-step energies differ"
    if stats_ref is not None:
        n, largest = st.cluster_stats()
        assert np.array_equal(n.astype(np.int64), stats_ref[0][first:first + R]), "numbers of clusters differ"
        assert np.array_equal(largest.astype(np.int64), stats_ref[1][first:first + R]), "largest clusters differ"


def _cubic(exact, L, J=-1.0):
    ea, eb, ej = exact.cubic_lattice_edges(L, J)
    return PR.Graph(ea, eb, ej, L ** 3)


def test_padded_classes(capi, exact):
    """Cubic 6^3: two colour classes of 108 sites padded to 256; one full replica group and a partial one."""
    G = _cubic(exact, 6)
    assert G.n_pos == 512
    _check(capi, G, R=40, T=6, k=2, beta=0.2216)
    _check(capi, G, R=40, T=5, k=1, beta=np.linspace(0.05, 0.6, 5))   # a schedule: every cluster step its own threshold


def test_full_classes_antiferromagnet(capi, exact):
    """Cubic 8^3, J = +1: classes of exactly 256 positions, no padding -- the one-degree sweep kernel runs between the steps."""
    G = _cubic(exact, 8, 1.0)
    assert G.n_pos == 512
    st = _check(capi, G, R=33, T=6, k=2, beta=0.3)
    assert st.graph.info.packed_degree == 6


def _mixed_graph():
    """300 sites in scrambled id order, degrees 0..6, an isolated site, a parallel edge, +-J, odd cycles."""
    rng = np.random.default_rng(2024)
    n = 300
    ids = rng.permutation(n)
    deg = np.zeros(n, dtype=int)
    edges = [(0, 1), (1, 2), (2, 0), (0, 1)]   # a triangle and a second bond between its first two sites
    for a, b in edges:
        deg[a] += 1
        deg[b] += 1
    while len(edges) < 520:
        a, b = (int(x) for x in rng.integers(0, n - 1, 2))   # site n - 1 stays isolated
        if a != b and deg[a] < 6 and deg[b] < 6 and (a, b) not in edges and (b, a) not in edges:
            edges.append((a, b))
            deg[a] += 1
            deg[b] += 1
    ea = ids[[e[0] for e in edges]].astype(np.uint64)
    eb = ids[[e[1] for e in edges]].astype(np.uint64)
    return PR.Graph(ea, eb, 0.75 * rng.choice([-1.0, 1.0], len(edges)), n), deg


def test_mixed_degrees(capi):
    G, deg = _mixed_graph()
    assert G.n_colours >= 3 and deg.min() == 0 and deg.max() == 6
    _check(capi, G, R=35, T=7, k=3, beta=0.5)
    _check(capi, G, R=35, T=4, k=1, beta=1.1)


def test_non_bipartite_triangular_lattice(capi):
    G = PR.Graph(*PR.triangular_lattice_edges(5, 5), 25)
    assert G.n_colours >= 3
    _check(capi, G, R=32, T=6, k=2, beta=0.25)
    _check(capi, G, R=3, T=4, k=1, beta=0.35)


def test_deep_chases_on_a_scrambled_ring(capi, oracle):
    """A ring of 2000 sites whose ids are a random permutation, all up (set_state): at beta = 20 the threshold is 2^32 and every
    replica is one cluster of 2000 sites whose labels chase through the whole ring; at beta = 0 every site is its own cluster."""
    n, R = 2000, 3
    order = np.random.default_rng(9).permutation(n).astype(np.uint64)
    G = PR.Graph(order, np.roll(order, -1), np.full(n, -1.0), n)
    seeds = capi.make_seeds(5, R)
    for beta, clusters, largest in ((20.0, 1, n), (0.0, n, 1)):
        st = _states(capi, G, seeds, 1)
        _, ref = oracle.pk_run(G.ea, G.eb, G.ej, n, seeds, 0, betas=[])   # the bits nobody owns keep their random start
        for r in range(R):
            st.set_state(r, np.ones(n, np.uint8))
            ref[r] = 1
        eps = st.do_time_steps(2, beta, per_step_energies=True)
        got_n, got_largest = st.cluster_stats()
        assert got_n.tolist() == [clusters] * R and got_largest.tolist() == [largest] * R
        ref, e_ref, stats_ref = PR.run(G, seeds, 2, 1, betas=[beta] * 2, states=ref)
        _compare(st, G, ref, e_ref, stats_ref, eps)
        if beta > 0:
            assert all(row.all() or not row.any() for row in st.states())


def test_per_replica_betas(capi, exact):
    G = _cubic(exact, 6)
    _check(capi, G, R=40, T=4, k=2, beta_replica=np.linspace(0.0, 0.6, 40))
    _check(capi, G, R=64, T=3, k=1, beta_replica=np.tile([0.1, 0.2216, 0.5, 20.0], 16))


@pytest.mark.parametrize("L", [6, 8])
def test_calls_that_begin_with_a_cluster_step(capi, oracle, exact, L):
    """A call with ONE beta whose first timestep is a cluster step: the Metropolis sweeps behind it need that call's acceptance
    table, not the previous call's.  6^3 (general packed kernel) and 8^3 (one-degree kernel)."""
    G = _cubic(exact, L)
    seeds = capi.make_seeds(41, 40)
    # k = 2: one sweep at one beta, then five timesteps at another, starting on the cluster step t = 1
    st = _states(capi, G, seeds, 2)
    eps = np.concatenate([st.do_time_steps(1, 0.15, per_step_energies=True), st.do_time_steps(5, 0.4, per_step_energies=True)], axis=1)
    ref, e_ref, stats_ref = PR.run(G, seeds, 6, 2, betas=[0.15] + [0.4] * 5)
    _compare(st, G, ref, e_ref, stats_ref, eps)
    # a fresh container whose clock is put on a cluster step
    st = _states(capi, G, seeds, 3)
    st.timestep = 2
    eps = st.do_time_steps(5, 0.3, per_step_energies=True)
    _, start = oracle.pk_run(G.ea, G.eb, G.ej, G.nvars, seeds, 0, betas=[])
    ref, e_ref, stats_ref = PR.run(G, seeds, 5, 3, betas=[0.3] * 5, states=start, t0=2)
    assert st.timestep == 7
    _compare(st, G, ref, e_ref, stats_ref, eps)


def test_results_do_not_depend_on_how_the_run_is_cut(capi, exact):
    G = _cubic(exact, 6)
    beta, T, R = 0.2216, 6, 64
    seeds = capi.make_seeds(31, R)

    def fresh(n=R, k=3, **kw):
        return _states(capi, G, seeds[:n], k, **kw)

    whole = fresh()
    e_whole = whole.do_time_steps(T, beta, per_step_energies=True)
    ref, ref_stats = whole.packed(), whole.cluster_stats()
    ref_e = whole.energies()
    # 6 timesteps in one call against 2 + 4
    split = fresh()
    e_split = np.concatenate([split.do_time_steps(2, beta, per_step_energies=True), split.do_time_steps(4, beta, per_step_energies=True)], axis=1)
    assert np.array_equal(split.packed(), ref) and np.array_equal(e_split, e_whole)
    # stop after 3 timesteps (the first cluster step); a new container takes the configurations and the clock and resumes
    first = fresh()
    first.do_time_steps(3, beta)
    resumed = fresh()
    for r, spins in enumerate(first.states()):
        resumed.set_state(r, spins)
    resumed.timestep = 3
    resumed.do_time_steps(3, beta)
    assert np.array_equal(resumed.packed(), ref)
    assert all(np.array_equal(a, b) for a, b in zip(resumed.cluster_stats(), ref_stats))
    # one replica alone is replica 0 of the sixty-four
    alone = fresh(1)
    alone.do_time_steps(T, beta)
    assert np.array_equal(alone.packed()[0], ref[0])
    assert [int(a[0]) for a in alone.cluster_stats()] == [int(a[0]) for a in ref_stats]
    # one replica group per batch of the cluster step's workspace against the default budget
    small = fresh()
    small.set_option("cluster_workspace_bytes", 1)
    small.do_time_steps(T, beta)
    assert np.array_equal(small.packed(), ref)
    assert all(np.array_equal(a, b) for a, b in zip(small.cluster_stats(), ref_stats))
    # shards of 5 + 32 + 27 experiments: cuts inside both groups
    parts = [fresh(replica_range=cut) for cut in ((0, 5), (5, 37), (37, 64))]
    eps = [p.do_time_steps(T, beta, per_step_energies=True) for p in parts]
    assert np.array_equal(np.concatenate([p.packed() for p in parts]), ref)
    assert np.array_equal(np.concatenate(eps), e_whole)
    assert np.array_equal(np.concatenate([p.energies() for p in parts]), ref_e)
    for i in range(2):
        assert np.array_equal(np.concatenate([p.cluster_stats()[i] for p in parts]), ref_stats[i])


def test_python_surface_gives_the_same_arrays(capi, exact):
    import py_monte_carlo

    G = _cubic(exact, 6)
    beta, T, R = 0.2216, 6, 40
    lat = py_monte_carlo.Lattice.from_arrays(G.ea, G.eb, G.ej, seed_gen=5)
    lat.set_cluster_update_every(2)
    assert lat.engine_info()["cluster_update_every"] == 2
    energies, states = lat.run_monte_carlo(beta, T, R)
    seeds = np.array(lat.make_seeds(R), dtype=np.uint64)
    st = _states(capi, G, seeds, 2)
    st.do_time_steps(T, beta)
    assert np.array_equal(states, st.states()) and np.array_equal(energies, st.energies())
    ref, e_ref, _ = PR.run(G, seeds, T, 2, betas=[beta] * T)
    assert np.array_equal(states, ref[:R].astype(bool)) and np.array_equal(energies, e_ref[:, -1])
    plain = py_monte_carlo.Lattice.from_arrays(G.ea, G.eb, G.ej, seed_gen=5)
    assert not np.array_equal(plain.run_monte_carlo(beta, T, R)[1], states)   # the default chain has no cluster steps
    ci = py_monte_carlo.ClassicIsing([((int(a), int(b)), float(j)) for a, b, j in zip(G.ea, G.eb, G.ej)], None, R, 9)
    ci.set_cluster_update_every(2)
    ci.run_monte_carlo(beta, T)
    st9 = _states(capi, G, capi.make_seeds(9, R), 2)
    st9.do_time_steps(T, beta)
    assert np.array_equal(ci.get_states(), st9.states()) and np.array_equal(ci.get_energies(), st9.energies())


@pytest.mark.parametrize("k", [1, 2])
def test_triangular_energy_against_exact_enumeration(capi, exact, k):
    """The seeded check of tests/test_packed_cluster_host.py on the device: same lattice, beta, seeds, chains and lengths; the
    restatement gives z = +0.21 (k = 1) and -0.66 (k = 2), and a bit-exact device gives the same.  |z| <= 5."""
    ea, eb, ej = PR.triangular_lattice_edges(4, 4, -1.0)
    G = PR.Graph(ea, eb, ej, 16)
    st = _states(capi, G, capi.make_seeds(PR.TRI_SEED + k, PR.TRI_CHAINS), k)
    st.do_time_steps(PR.TRI_THERM, PR.TRI_BETA)
    means = st.do_time_steps(PR.TRI_STEPS, PR.TRI_BETA, per_step_energies=True).mean(axis=1)
    want = exact.enumerate_graph(ea, eb, ej, 16, PR.TRI_BETA)["E"]
    z = (means.mean() - want) / (means.std(ddof=1) / np.sqrt(PR.TRI_CHAINS))
    print(f"k = {k}: <E> {means.mean():.4f} exact {want:.4f} z {z:+.2f}")
    assert abs(z) <= 5.0


def test_cubic_cluster_chains_agree_with_metropolis_chains(capi, exact):
    """Cubic 8^3 at the bulk critical coupling: PR.CUBIC_CHAINS chains with a cluster step at every timestep against as many
    Metropolis-only chains of the same container type (other seeds); <E> within 5 combined standard errors, each from the
    spread across its chains."""
    G = _cubic(exact, 8)
    out = []
    for k, seed in ((1, 0xC0B1C000), (0, 0xC0B1C001)):
        st = _states(capi, G, capi.make_seeds(seed, PR.CUBIC_CHAINS), k)
        st.do_time_steps(PR.CUBIC_THERM, PR.CUBIC_BETA)
        means = st.do_time_steps(PR.CUBIC_STEPS, PR.CUBIC_BETA, per_step_energies=True).mean(axis=1)
        out.append((means.mean(), means.std(ddof=1) / np.sqrt(len(means))))
    z = (out[0][0] - out[1][0]) / np.hypot(out[0][1], out[1][1])
    print(f"cluster <E> {out[0][0]:.2f} +- {out[0][1]:.2f}, Metropolis <E> {out[1][0]:.2f} +- {out[1][1]:.2f}, z {z:+.2f}")
    assert abs(z) <= 5.0


def test_refusals_leave_the_container_usable(capi, exact):
    G = _cubic(exact, 6)
    seeds = capi.make_seeds(3, 32)
    # the real-coupling packed family
    ej = np.random.default_rng(2).normal(size=len(G.ea))
    real = capi.States(capi.Graph(G.ea, G.eb, ej, nvars=G.nvars, stable_path=True), seeds)
    assert real.family == "packed_real"
    with pytest.raises(ValueError, match="real-coupling"):
        real.set_cluster_every(2)
    assert real.cluster_every == 0
    real.do_time_steps(2, 0.4)
    assert real.timestep == 2
    # a ladder attached, and the other way round
    st = _states(capi, G, seeds, 0)
    st.pt_attach(np.linspace(0.1, 0.4, 32), 0, 32, 1, 7)
    with pytest.raises(ValueError, match="ladder"):
        st.set_cluster_every(3)
    assert st.cluster_every == 0
    st.pt_detach()
    st.set_cluster_every(3)
    assert not st.pt_can_attach(32, 0, 32, 1)
    with pytest.raises(ValueError, match="cluster"):
        st.pt_attach(np.linspace(0.1, 0.4, 32), 0, 32, 1, 7)
    # isoenergetic moves stay a checkerboard feature
    with pytest.raises(ValueError, match="general-graph"):
        st.set_icm_every(2)
    st.do_time_steps(3, 0.2216)
    assert st.timestep == 3 and int(st.cluster_stats()[1][0]) >= 1
    with pytest.raises(ValueError, match="no cluster step"):
        _states(capi, G, seeds, 1).cluster_stats()

"""Isoenergetic cluster moves on replica-packed containers of both families on the device against the numpy
restatement of tests/packed_icm_reference.py (bit-exact: packed words with their cleared padding, states(), energies after every
timestep, the three statistics), their invariants and invariances, the Python surface, the refusals, and the physics against
exact enumeration and against Metropolis-only chains."""
import numpy as np
import pytest

import packed_icm_reference as IR

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _force_packed(monkeypatch):
    monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")


def _states(capi, G, seeds, k, replica_range=None, biases=None, real=False):
    if real:
        g = capi.Graph(G.ea, G.eb, G.ej, nvars=G.nvars, biases=biases, stable_path=True)
    else:
        g = capi.Graph(G.ea, G.eb, G.ej, nvars=G.nvars, force_general=True)
    st = capi.States(g, seeds, replica_range=replica_range)
    assert st.family == ("packed_real" if real else "packed_bitsliced")
    st.set_icm_every(k)
    assert st.icm_every == k
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
        got = st.icm_stats()
        for name, a, b in zip(("clusters", "largest", "minus sites"), got, stats_ref):
            assert np.array_equal(a.astype(np.int64), b[first // 2:first // 2 + R // 2]), name


def _check(capi, G, R, T, k, beta=None, beta_replica=None, seed=77, biases=None, real=False):
    """R experiments from the random start, T timesteps with icm_every = k, against the restatement."""
    seeds = capi.make_seeds(seed, R)
    st = _states(capi, G, seeds, k, biases=biases, real=real)
    if beta_replica is not None:
        st.set_betas(beta_replica)
        eps = st.do_time_steps(T, None, per_step_energies=True)
        ref, e_ref, stats_ref = IR.run(G, seeds, T, k, beta_replica=beta_replica, biases=biases, real=real)
    else:
        betas = [beta] * T if np.ndim(beta) == 0 else list(beta)
        eps = st.do_time_steps(T, beta, per_step_energies=True)
        ref, e_ref, stats_ref = IR.run(G, seeds, T, k, betas=betas, biases=biases, real=real)
    assert st.timestep == T
    _compare(st, G, ref, e_ref, stats_ref, eps)
    return st, eps


def _cubic(exact, L):
    ea, eb, ej = IR.cubic_glass(exact, L)
    return IR.Graph(ea, eb, ej, L ** 3)


# ---- bit-sliced family ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,k,T", [(40, 2, 6), (40, 1, 4), (33, 2, 6)])
def test_padded_classes(capi, exact, R, k, T):
    """Cubic 6^3 +-J: two colour classes of 108 sites padded to 256.  R = 40: a full group and a partial one; R = 33: the last
    experiment has no partner and its neighbouring bit is nobody's."""
    G = _cubic(exact, 6)
    assert G.n_pos == 512
    _, eps = _check(capi, G, R=R, T=T, k=k, beta=0.6)
    if k == 1:   # moves alone: E_a + E_b of every pair is constant, exactly -- and the configurations change
        pair_sum = eps[0::2] + eps[1::2]
        assert np.array_equal(pair_sum, np.repeat(pair_sum[:, :1], T, axis=1))
        assert (eps[:, 1:] != eps[:, :-1]).any()


def test_full_classes_and_the_one_degree_sweep_kernel(capi, exact):
    """Cubic 8^3 +-J: classes of exactly 256 positions, no padding; the one-degree sweep kernel runs between the moves."""
    G = _cubic(exact, 8)
    assert G.n_pos == 512
    st, _ = _check(capi, G, R=34, T=7, k=3, beta=0.5)
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
    return IR.Graph(ea, eb, 0.75 * rng.choice([-1.0, 1.0], len(edges)), n), deg


def test_mixed_degrees(capi):
    G, deg = _mixed_graph()
    assert G.n_colours >= 3 and deg.min() == 0 and deg.max() == 6
    _check(capi, G, R=35, T=7, k=3, beta=0.5)
    _check(capi, G, R=35, T=4, k=1, beta=1.1)


def test_non_bipartite_triangular_lattice(capi):
    ea, eb, _ = IR.triangular_lattice_edges(5, 5)
    G = IR.Graph(ea, eb, np.random.default_rng(4).choice([-1.0, 1.0], len(ea)), 25)
    assert G.n_colours >= 3
    _check(capi, G, R=3, T=6, k=2, beta=0.4)


def test_deep_chases_on_a_scrambled_ring(capi, oracle):
    """A ring of 2000 sites whose ids are a random permutation.  Replica 0 all up and replica 1 all down: one cluster of 2000
    positions whose labels chase through the whole ring.  Replicas 2 and 3 equal: no d = 1 position, nothing moves."""
    n, R = 2000, 4
    order = np.random.default_rng(9).permutation(n).astype(np.uint64)
    G = IR.Graph(order, np.roll(order, -1), np.full(n, -1.0), n)
    seeds = capi.make_seeds(5, R)
    st = _states(capi, G, seeds, 1)
    _, ref = oracle.pk_run(G.ea, G.eb, G.ej, n, seeds, 0, betas=[])   # the bits nobody owns keep their random start
    same = (np.random.default_rng(1).random(n) < 0.5).astype(np.uint8)
    for r, spins in enumerate((np.ones(n, np.uint8), np.zeros(n, np.uint8), same, same)):
        st.set_state(r, spins)
        ref[r] = spins
    eps = st.do_time_steps(3, 0.3, per_step_energies=True)
    clusters, largest, minus = st.icm_stats()
    assert clusters.tolist() == [1, 0] and largest.tolist() == [n, 0] and minus.tolist() == [n, 0]
    ref, e_ref, stats_ref = IR.run(G, seeds, 3, 1, betas=[0.3] * 3, states=ref)
    _compare(st, G, ref, e_ref, stats_ref, eps)
    got = st.states()
    assert (got[0].all() and not got[1].any()) or (got[1].all() and not got[0].any())   # uniform and opposite
    assert np.array_equal(got[2], same.astype(bool)) and np.array_equal(got[3], same.astype(bool))


# ---- real-coupling family ------------------------------------------------------------------------------------------------
def _terms(G, biases):
    return np.abs(G.ej).sum() + (0.0 if biases is None else np.abs(biases).sum())


def test_real_couplings_and_biases_on_a_cubic_lattice(capi, exact):
    """Gaussian J and Gaussian biases on cubic 6^3 (slots = 7): energies bit-equal to the oracle's two-level energy, as in
    tests/test_gpu_real.py."""
    ea, eb, _ = exact.cubic_lattice_edges(6, 1.0)
    rng = np.random.default_rng(2024)
    G = IR.Graph(ea, eb, rng.normal(size=len(ea)), 216)
    h = rng.normal(size=216)
    st, _ = _check(capi, G, R=40, T=6, k=2, beta=0.8, biases=h, real=True)
    assert st.graph.info.real_slots == 7
    # moves alone: E_a + E_b within 4e-13 sum |terms| (four energies, each inside the 1e-13 bound of tests/test_gpu_real_k1.py)
    _, eps = _check(capi, G, R=40, T=4, k=1, beta=0.8, biases=h, real=True)
    pair_sum = eps[0::2] + eps[1::2]
    assert np.abs(pair_sum - pair_sum[:, :1]).max() <= 4e-13 * _terms(G, h)
    assert (eps[:, 1:] != eps[:, :-1]).any()


def test_real_couplings_on_a_degree_15_random_graph(capi):
    """About 300 sites, degrees up to 15 (slots = 15), a zero coupling among the Gaussian ones: a stored bond like any other."""
    rng = np.random.default_rng(15)
    n, pairs, deg = 300, set(), np.zeros(300, dtype=int)
    while len(pairs) < 2000:
        a, b = (int(v) for v in rng.integers(0, n, 2))
        if a != b and deg[a] < 15 and deg[b] < 15 and (min(a, b), max(a, b)) not in pairs:
            pairs.add((min(a, b), max(a, b)))
            deg[a] += 1
            deg[b] += 1
    pairs = sorted(pairs)
    rng.shuffle(pairs)
    ea, eb = np.array([p[0] for p in pairs], dtype=np.uint64), np.array([p[1] for p in pairs], dtype=np.uint64)
    ej = rng.normal(size=len(ea))
    ej[3] = 0.0
    G = IR.Graph(ea, eb, ej, n)
    assert deg.max() == 15
    st, _ = _check(capi, G, R=34, T=5, k=2, beta=0.7, real=True)
    assert st.graph.info.real_slots == 15


# ---- results do not depend on the cut ------------------------------------------------------------------------------------
def test_results_do_not_depend_on_how_the_run_is_cut(capi, exact):
    G = _cubic(exact, 6)
    beta, T, R = 0.6, 6, 64
    seeds = capi.make_seeds(31, R)

    def fresh(n=R, k=3, **kw):
        return _states(capi, G, seeds[:n], k, **kw)

    whole = fresh()
    e_whole = whole.do_time_steps(T, beta, per_step_energies=True)
    ref, ref_stats, ref_e = whole.packed(), whole.icm_stats(), whole.energies()
    # 6 timesteps in one call against 2 + 4
    split = fresh()
    e_split = np.concatenate([split.do_time_steps(2, beta, per_step_energies=True), split.do_time_steps(4, beta, per_step_energies=True)], axis=1)
    assert np.array_equal(split.packed(), ref) and np.array_equal(e_split, e_whole)
    # stop after 3 timesteps (the first move); a new container takes the configurations and the clock and resumes
    first = fresh()
    first.do_time_steps(3, beta)
    resumed = fresh()
    for r, spins in enumerate(first.states()):
        resumed.set_state(r, spins)
    resumed.timestep = 3
    resumed.do_time_steps(3, beta)
    assert np.array_equal(resumed.packed(), ref)
    assert all(np.array_equal(a, b) for a, b in zip(resumed.icm_stats(), ref_stats))
    # one replica group per batch of the move's workspace against the default budget
    small = fresh()
    small.set_option("cluster_workspace_bytes", 1)
    small.do_time_steps(T, beta)
    assert np.array_equal(small.packed(), ref)
    assert all(np.array_equal(a, b) for a, b in zip(small.icm_stats(), ref_stats))
    # even-aligned shards that cut inside both groups
    parts = [fresh(replica_range=cut) for cut in ((0, 6), (6, 38), (38, 64))]
    eps = [p.do_time_steps(T, beta, per_step_energies=True) for p in parts]
    assert np.array_equal(np.concatenate([p.packed() for p in parts]), ref)
    assert np.array_equal(np.concatenate(eps), e_whole)
    assert np.array_equal(np.concatenate([p.energies() for p in parts]), ref_e)
    for i in range(3):
        assert np.array_equal(np.concatenate([p.icm_stats()[i] for p in parts]), ref_stats[i])
    # odd cuts would split a pair
    g = whole.graph
    for cut, why in (((5, 37), "odd experiment index"), ((6, 37), "ends inside a pair")):
        shard = capi.States(g, seeds, replica_range=cut)
        with pytest.raises(ValueError, match=why):
            shard.set_icm_every(3)
        assert shard.icm_every == 0
    capi.States(g, seeds[:63], replica_range=(38, 63)).set_icm_every(3)   # ends at the last experiment: fine


def test_per_replica_betas_and_a_schedule(capi, exact):
    G = _cubic(exact, 6)
    _check(capi, G, R=40, T=4, k=2, beta_replica=np.repeat(np.linspace(0.1, 1.0, 20), 2))
    _check(capi, G, R=40, T=5, k=2, beta=np.linspace(0.1, 0.9, 5))
    st = _states(capi, G, capi.make_seeds(1, 4), 2)
    with pytest.raises(ValueError, match="equal betas"):
        st.set_betas([0.1, 0.2, 0.3, 0.3])
    st.set_icm_every(0)
    st.set_betas([0.1, 0.2, 0.3, 0.3])
    with pytest.raises(ValueError, match="betas differ inside a pair"):
        st.set_icm_every(2)


@pytest.mark.parametrize("L", [6, 8])
def test_calls_that_begin_with_a_move(capi, oracle, exact, L):
    """A call with ONE beta whose first timestep is a move: the Metropolis sweeps behind it need that call's acceptance table."""
    G = _cubic(exact, L)
    seeds = capi.make_seeds(41, 40)
    st = _states(capi, G, seeds, 2)
    eps = np.concatenate([st.do_time_steps(1, 0.15, per_step_energies=True), st.do_time_steps(5, 0.7, per_step_energies=True)], axis=1)
    ref, e_ref, stats_ref = IR.run(G, seeds, 6, 2, betas=[0.15] + [0.7] * 5)
    _compare(st, G, ref, e_ref, stats_ref, eps)
    # a fresh container whose clock is put on a move
    st = _states(capi, G, seeds, 3)
    st.timestep = 2
    eps = st.do_time_steps(5, 0.5, per_step_energies=True)
    _, start = oracle.pk_run(G.ea, G.eb, G.ej, G.nvars, seeds, 0, betas=[])
    ref, e_ref, stats_ref = IR.run(G, seeds, 5, 3, betas=[0.5] * 5, states=start, t0=2)
    assert st.timestep == 7
    _compare(st, G, ref, e_ref, stats_ref, eps)


def test_run_sampling(capi, exact):
    G = _cubic(exact, 6)
    seeds = capi.make_seeds(8, 40)
    st = _states(capi, G, seeds, 3)
    energies, states = st.run_sampling(0.6, 2, 2, 3)   # thermalise 2, then 3 samples 2 timesteps apart: after t = 4, 6, 8 timesteps
    ref, t0 = None, 0
    for n, T in enumerate((4, 6, 8)):
        ref, e_ref, _ = IR.run(G, seeds, T - t0, 3, betas=[0.6] * (T - t0), states=ref, t0=t0)
        t0 = T
        assert np.array_equal(states[:, n].astype(np.uint8), ref[:40]) and np.array_equal(energies[:, n], e_ref[:, -1])
    assert st.timestep == 8


# ---- Python surface ------------------------------------------------------------------------------------------------------
def test_python_surface_gives_the_same_arrays(capi, exact):
    import py_monte_carlo

    G = _cubic(exact, 6)
    beta, T, R = 0.6, 6, 40
    lat = py_monte_carlo.Lattice.from_arrays(G.ea, G.eb, G.ej, seed_gen=5)
    assert lat.engine_info()["replica_cluster_update_every"] == 0
    lat.set_replica_cluster_update_every(2)
    assert lat.engine_info()["replica_cluster_update_every"] == 2
    energies, states = lat.run_monte_carlo(beta, T, R)
    seeds = np.array(lat.make_seeds(R), dtype=np.uint64)
    st = _states(capi, G, seeds, 2)
    st.do_time_steps(T, beta)
    assert np.array_equal(states, st.states()) and np.array_equal(energies, st.energies())
    ref, e_ref, _ = IR.run(G, seeds, T, 2, betas=[beta] * T)
    assert np.array_equal(states, ref[:R].astype(bool)) and np.array_equal(energies, e_ref[:, -1])
    plain = py_monte_carlo.Lattice.from_arrays(G.ea, G.eb, G.ej, seed_gen=5)
    assert not np.array_equal(plain.run_monte_carlo(beta, T, R)[1], states)   # the default chain has no moves
    ci = py_monte_carlo.ClassicIsing([((int(a), int(b)), float(j)) for a, b, j in zip(G.ea, G.eb, G.ej)], None, R, 9)
    ci.set_replica_cluster_update_every(2)
    ci.run_monte_carlo(beta, T)
    st9 = _states(capi, G, capi.make_seeds(9, R), 2)
    st9.do_time_steps(T, beta)
    assert np.array_equal(ci.get_states(), st9.states()) and np.array_equal(ci.get_energies(), st9.energies())


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_container_usable(capi, exact, monkeypatch):
    G = _cubic(exact, 6)
    seeds = capi.make_seeds(3, 32)
    # the f64 CSR family
    monkeypatch.delenv("ISINGMC_FORCE_PACKED")
    csr = capi.States(capi.Graph(G.ea, G.eb, G.ej, nvars=G.nvars), seeds[:2])
    assert csr.family == "csr_f64"
    with pytest.raises(ValueError, match="general-graph"):
        csr.set_icm_every(2)
    assert csr.icm_every == 0
    csr.do_time_steps(2, 0.4)
    assert csr.timestep == 2
    monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
    # a ladder attached, and the other way round
    st = _states(capi, G, seeds, 0)
    st.pt_attach(np.linspace(0.1, 0.4, 32), 0, 32, 1, 7)
    with pytest.raises(ValueError, match="ladder"):
        st.set_icm_every(3)
    assert st.icm_every == 0
    st.pt_detach()
    st.set_icm_every(3)
    with pytest.raises(ValueError, match="isoenergetic"):
        st.pt_attach(np.linspace(0.1, 0.4, 32), 0, 32, 1, 7)
    # Swendsen-Wang steps and isoenergetic moves exclude each other, in both orders
    with pytest.raises(ValueError, match="isoenergetic"):
        st.set_cluster_every(2)
    assert st.cluster_every == 0 and st.icm_every == 3
    st.set_icm_every(0)
    st.set_cluster_every(2)
    with pytest.raises(ValueError, match="Swendsen-Wang"):
        st.set_icm_every(3)
    assert st.icm_every == 0 and st.cluster_every == 2
    st.set_cluster_every(0)
    st.set_icm_every(3)
    st.do_time_steps(3, 0.6)
    assert st.timestep == 3 and int(st.icm_stats()[2][0]) >= 1
    with pytest.raises(ValueError, match="no isoenergetic cluster move"):
        _states(capi, G, seeds, 1).icm_stats()


# ---- physics -------------------------------------------------------------------------------------------------------------
def test_triangular_glass_energy_against_exact_enumeration(capi, exact):
    """The seeded check of tests/test_packed_icm_host.py on the device: same graph, beta, seeds, chains and lengths; a bit-exact
    device reproduces the z recorded in tests/packed_icm_reference.py.  |z| <= 5."""
    ea, eb, ej = IR.tri_glass()
    G = IR.Graph(ea, eb, ej, 16)
    st = _states(capi, G, capi.make_seeds(IR.TRI_SEED, IR.TRI_CHAINS), 2)
    st.do_time_steps(IR.TRI_THERM, IR.TRI_BETA)
    means = st.do_time_steps(IR.TRI_STEPS, IR.TRI_BETA, per_step_energies=True).mean(axis=1)
    want = exact.enumerate_graph(ea, eb, ej, 16, IR.TRI_BETA)["E"]
    z = (means.mean() - want) / (means.std(ddof=1) / np.sqrt(IR.TRI_CHAINS))
    print(f"<E> {means.mean():.4f} exact {want:.4f} z {z:+.2f}")
    assert abs(z) <= 5.0
    assert round(z, 2) == IR.TRI_Z


def test_cubic_glass_chains_agree_with_metropolis_chains(capi, exact):
    """Cubic 6^3 +-J at IR.CUBIC_BETA: IR.CUBIC_CHAINS chains with a move at every second timestep against as many
    Metropolis-only chains (other seeds); <E> within 5 combined standard errors, each from the spread across its chains; the z
    is the one the restatement gave (IR.CUBIC_Z)."""
    G = _cubic(exact, 6)
    out = []
    for k, seed in zip((2, 0), IR.CUBIC_SEEDS):
        st = _states(capi, G, capi.make_seeds(seed, IR.CUBIC_CHAINS), k)
        st.do_time_steps(IR.CUBIC_THERM, IR.CUBIC_BETA)
        means = st.do_time_steps(IR.CUBIC_STEPS, IR.CUBIC_BETA, per_step_energies=True).mean(axis=1)
        out.append((means.mean(), means.std(ddof=1) / np.sqrt(len(means))))
    z = (out[0][0] - out[1][0]) / np.hypot(out[0][1], out[1][1])
    print(f"moves <E> {out[0][0]:.2f} +- {out[0][1]:.2f}, Metropolis <E> {out[1][0]:.2f} +- {out[1][1]:.2f}, z {z:+.2f}")
    assert abs(z) <= 5.0
    assert round(z, 2) == IR.CUBIC_Z

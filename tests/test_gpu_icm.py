"""Isoenergetic cluster moves between replica pairs on the device against the numpy restatement of
tests/icm_reference.py (bit-exact: packed words, energies, per-step energies, pair statistics), their invariances, the exact
invariants at 2048^2, every refusal, and the physics on a +-J sample against a Metropolis-only chain."""
import numpy as np
import pytest

import icm_reference as IR

pytestmark = pytest.mark.gpu


def _edges(exact, W, H, J):
    """J = -1.0 / +1.0: uniform; J = "glass": a seeded +-J pattern."""
    if J == "glass":
        return exact.square_lattice_edges(W, H, -1.0, np.random.default_rng(W + 7 * H))
    return exact.square_lattice_edges(W, H, J)


def _graph(capi, exact, W, H, J, **kw):
    ea, eb, ej = _edges(exact, W, H, J)
    return capi.Graph(ea, eb, ej, W * H, **kw), IR.couplings(W, H, ej)


def _check_against_reference(st, W, H, jr, jd, seeds, start, t0, betas, k, energies=None):
    """st has run the timesteps of `betas` ([T] or [R][T]) from `start` (bool[R, N]) at t0: compare everything with the restatement."""
    lat = IR.make_lat(W, H, jr, jd)
    T = np.asarray(betas).shape[-1]
    spins, e_ref, ref_stats = IR.run_replicas(W, H, jr, jd, [int(s) for s in seeds], [s.astype(np.uint8) for s in start], t0, betas, k)
    packed, e_now = st.packed(), st.energies()
    for r in range(len(seeds)):
        assert np.array_equal(packed[r], lat.pack(spins[r].ravel())), f"replica {r}: configurations differ"
        assert e_now[r] == e_ref[r, -1]
        if energies is not None:
            assert np.array_equal(energies[r], e_ref[r]), f"replica {r}: per-step energies differ"
    if k and any((t0 + n) % k == k - 1 for n in range(T)):
        got = st.icm_stats()
        assert [tuple(int(a[p]) for a in got) for p in range(len(seeds) // 2)] == ref_stats
    return spins


@pytest.mark.parametrize("J", [-1.0, 1.0, "glass"])
@pytest.mark.parametrize("W,H", [(64, 4), (128, 64), (256, 64), (1024, 128)])
def test_icm_steps_are_bit_exact(capi, oracle, exact, W, H, J):
    """k = 1 for 6 timesteps on 4 replicas and k = 3 for 9 timesteps on 5 replicas (Metropolis sweeps and cluster moves interleaved;
    the fifth replica has no partner), random starts; 1024 x 128 has several tiles in both directions."""
    g, (jr, jd) = _graph(capi, exact, W, H, J)
    seeds = capi.make_seeds(2000 + W + H, 5)
    beta = 0.6
    for k, T, R in ((1, 6, 4), (3, 9, 5)):
        st = capi.States(g, seeds[:R])
        st.set_icm_every(k)
        assert st.icm_every == k
        start = st.states()
        e = st.do_time_steps(T, beta, per_step_energies=True)
        assert st.timestep == T
        _check_against_reference(st, W, H, jr, jd, seeds[:R], start, 0, [beta] * T, k, energies=e)
        if R % 2:   # the replica without a partner: its Metropolis-only trajectory with the ICM timesteps skipped
            lat = IR.make_lat(W, H, jr, jd)
            ref = lat.pack(start[R - 1].astype(np.uint8))
            for t in range(T):
                if t % k != k - 1:
                    lat.sweep(ref, int(seeds[R - 1]), t, beta)
            assert np.array_equal(st.packed()[R - 1], ref)


def test_icm_with_per_replica_betas_and_a_schedule(capi, oracle, exact):
    W, H = 256, 64
    g, (jr, jd) = _graph(capi, exact, W, H, "glass")
    seeds = capi.make_seeds(177, 4)
    st = capi.States(g, seeds)
    st.set_icm_every(2)
    start = st.states()
    with pytest.raises(ValueError, match="equal betas"):
        st.set_betas([0.3, 0.3, 0.8, 0.7])
    per_replica = [0.3, 0.3, 0.8, 0.8]   # equal inside the pairs
    st.set_betas(per_replica)
    st.do_time_steps(6, None)
    _check_against_reference(st, W, H, jr, jd, seeds, start, 0, np.repeat(np.array(per_replica)[:, None], 6, axis=1), 2)
    st.set_betas(None)
    mid = st.states()
    schedule = list(np.linspace(0.1, 1.2, 5))   # an annealing schedule: every timestep its own beta
    e = st.do_time_steps(5, schedule, per_step_energies=True)
    _check_against_reference(st, W, H, jr, jd, seeds, mid, 6, schedule, 2, energies=e)
    # switching it on while unequal pair betas are set
    other = capi.States(g, seeds)
    other.set_betas([0.3, 0.4, 0.8, 0.8])
    with pytest.raises(ValueError, match="differ inside a pair"):
        other.set_icm_every(2)
    assert other.icm_every == 0
    other.set_betas(per_replica)
    other.set_icm_every(2)
    assert other.icm_every == 2


def test_icm_through_run_sampling(capi, oracle, exact):
    W, H, beta = 128, 64, 0.7
    g, (jr, jd) = _graph(capi, exact, W, H, "glass")
    seeds = capi.make_seeds(178, 4)
    st = capi.States(g, seeds)
    st.set_icm_every(3)
    start = [s.astype(np.uint8) for s in st.states()]
    energies, states = st.run_sampling(beta, 2, 2, 4)   # thermalise 2, then 4 samples 2 timesteps apart: t = 4, 6, 8, 10
    spins, t0 = start, 0
    for n, T in enumerate((4, 6, 8, 10)):
        spins, e_ref, _ = IR.run_replicas(W, H, jr, jd, [int(s) for s in seeds], spins, t0, [beta] * (T - t0), 3)
        t0 = T
        for r in range(4):
            assert np.array_equal(states[r, n], spins[r].ravel().astype(bool)) and energies[r, n] == e_ref[r, -1]
    assert st.timestep == 10


def test_icm_through_the_python_classes(capi, oracle, exact):
    import py_monte_carlo

    W, H, beta, R, T = 128, 64, 0.7, 5, 6
    ea, eb, ej = _edges(exact, W, H, "glass")
    jr, jd = IR.couplings(W, H, ej)
    lat = py_monte_carlo.Lattice.from_arrays(ea, eb, ej, seed_gen=5)
    start = np.random.default_rng(3).random(W * H) < 0.5
    lat.set_initial_state([bool(b) for b in start])
    assert lat.engine_info()["replica_cluster_update_every"] == 0
    lat.set_replica_cluster_update_every(2)
    assert lat.engine_info()["replica_cluster_update_every"] == 2
    energies, states = lat.run_monte_carlo(beta, T, R)
    spins, e_ref, _ = IR.run_replicas(W, H, jr, jd, [int(s) for s in lat.make_seeds(R)], [start.astype(np.uint8)] * R, 0, [beta] * T, 2)
    for r in range(R):
        assert np.array_equal(states[r], spins[r].ravel().astype(bool)) and energies[r] == e_ref[r, -1]
    plain = py_monte_carlo.Lattice.from_arrays(ea, eb, ej, seed_gen=5)
    plain.set_initial_state([bool(b) for b in start])
    assert plain.engine_info()["replica_cluster_update_every"] == 0
    assert not np.array_equal(plain.run_monte_carlo(beta, T, R)[1], states)   # the default chain has no cluster moves
    # replica ranges: an even lower bound gives the rows of the whole call, an odd one would split a pair
    part = lat.run_monte_carlo(beta, T, R, replica_range=(2, 5))
    assert np.array_equal(part[1], states[2:5]) and np.array_equal(part[0], energies[2:5])
    with pytest.raises(ValueError, match="even"):
        lat.run_monte_carlo(beta, T, R, replica_range=(1, 5))
    ci = py_monte_carlo.ClassicIsing([((int(a), int(b)), float(j)) for a, b, j in zip(ea, eb, ej)], None, 2, 9)
    before = np.array(ci.get_energies())
    ci.set_replica_cluster_update_every(1)
    ci.run_monte_carlo(beta, 3)
    assert np.array(ci.get_energies()).sum() == before.sum()   # three cluster moves alone: E_a + E_b stays
    cubic = py_monte_carlo.ClassicIsing([((int(a), int(b)), float(j)) for a, b, j in zip(*exact.cubic_lattice_edges(6))], None, 2, 9)
    with pytest.raises(ValueError, match="general-graph"):
        cubic.set_replica_cluster_update_every(1)


def test_results_do_not_depend_on_how_the_run_is_cut(capi, exact, monkeypatch):
    W, H, beta, T = 1024, 128, 0.7, 6
    g, _ = _graph(capi, exact, W, H, "glass")
    seeds = capi.make_seeds(31, 10)

    def fresh(n=10, k=3, **kw):
        st = capi.States(g, seeds[:n], **kw)
        st.set_icm_every(k)
        return st

    whole = fresh()
    e_whole = whole.do_time_steps(T, beta, per_step_energies=True)
    ref, ref_stats = whole.packed(), whole.icm_stats()
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
    # one pair alone is pair 0 of the five; a shard of whole pairs is its pairs of the ten
    alone = fresh(2)
    alone.do_time_steps(T, beta)
    assert np.array_equal(alone.packed(), ref[:2])
    assert [int(a[0]) for a in alone.icm_stats()] == [int(a[0]) for a in ref_stats]
    shard = capi.States(g, seeds, replica_range=(4, 8))
    shard.set_icm_every(3)
    shard.do_time_steps(T, beta)
    assert np.array_equal(shard.packed(), ref[4:8])
    assert all(np.array_equal(a, b[2:4]) for a, b in zip(shard.icm_stats(), ref_stats))
    # one pair per batch of the workspace against the default budget
    small = fresh()
    small.set_option("cluster_workspace_bytes", 1)
    small.do_time_steps(T, beta)
    assert np.array_equal(small.packed(), ref)
    assert all(np.array_equal(a, b) for a, b in zip(small.icm_stats(), ref_stats))
    # the device fan-out of the Python Lattice: 10 experiments on two blocks = 5 + 5 rounded to 6 + 4, no pair is split
    import py_monte_carlo
    ea, eb, ej = _edges(exact, 256, 64, "glass")
    one = py_monte_carlo.Lattice.from_arrays(ea, eb, ej, seed_gen=4)
    one.set_replica_cluster_update_every(2)
    monkeypatch.setenv("ISINGMC_DEVICES", "0,0")
    two = py_monte_carlo.Lattice.from_arrays(ea, eb, ej, seed_gen=4)
    two.set_replica_cluster_update_every(2)
    assert two.get_devices() == [0, 0]
    a, b = one.run_monte_carlo(beta, T, 10), two.run_monte_carlo(beta, T, 10)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_degenerate_pairs_span_every_tile_border(capi, exact):
    W, H = 1024, 128
    N = W * H
    g, _ = _graph(capi, exact, W, H, "glass")
    seeds = capi.make_seeds(8, 4)
    st = capi.States(g, seeds)
    st.set_icm_every(1)
    with pytest.raises(ValueError, match="no isoenergetic cluster move"):
        st.icm_stats()
    # pair 0: identical replicas; pair 1: opposite replicas (one cluster across every tile border and both wraps)
    a = np.random.default_rng(5).random(N) < 0.5
    for r, spins in enumerate((a, a, a, ~a)):
        st.set_state(r, spins.astype(np.uint8))
    outcomes = set()
    for _ in range(6):
        st.do_time_steps(1, 0.5)
        n, largest, minus = st.icm_stats()
        assert (int(n[0]), int(largest[0]), int(minus[0])) == (0, 0, 0)
        assert (int(n[1]), int(largest[1]), int(minus[1])) == (1, N, N)
        s = st.states()
        assert np.array_equal(s[0], a) and np.array_equal(s[1], a)
        assert np.array_equal(s[3], ~s[2]) and (np.array_equal(s[2], a) or np.array_equal(s[2], ~a))
        outcomes.add(bool(np.array_equal(s[2], a)))
    assert outcomes == {False, True}


def test_invariants_at_full_glass_size(capi, exact):
    """2048^2 +-J x 8 replicas, icm_every = 1: E_a + E_b is conserved exactly across a step, a XOR b is unchanged, the reported
    q = -1 sites are the set bits of a XOR b, and about half of the clusters move."""
    L, R = 2048, 8
    g, _ = _graph(capi, exact, L, L, "glass")
    st = capi.States(g, capi.make_seeds(99, R))
    st.do_time_steps(2, 0.8)   # Metropolis first: icm_every is still 0
    st.set_icm_every(1)
    for _ in range(2):
        e0, p0 = st.energies(), st.packed()
        e = st.do_time_steps(1, 0.8, per_step_energies=True)
        e1, p1 = st.energies(), st.packed()
        assert np.array_equal(e[:, 0], e1)
        assert np.array_equal(e0[0::2] + e0[1::2], e1[0::2] + e1[1::2])   # |J| = 1: integers in f64, exactly
        assert np.array_equal(p0[0::2] ^ p0[1::2], p1[0::2] ^ p1[1::2])
        assert np.array_equal(p0[0::2] ^ p1[0::2], p0[1::2] ^ p1[1::2])   # the same sites flip in both replicas
        n, largest, minus = st.icm_stats()
        q = p0[0::2] ^ p0[1::2]
        assert [int(m) for m in minus] == [int(np.unpackbits(row.view(np.uint8)).sum()) for row in q]
        moved = p0[0::2] ^ p1[0::2]
        assert all((row & ~qrow).max() == 0 for row, qrow in zip(moved, q))   # only q = -1 sites move
        assert all(0.3 * int(m) < int(np.unpackbits(row.view(np.uint8)).sum()) < 0.7 * int(m) for row, m in zip(moved, minus))
        assert all(1 <= int(b) <= int(m) and 1 <= int(c) <= int(m) for b, c, m in zip(largest, n, minus))
        assert not np.array_equal(e0, e1)


def test_unsupported_containers_are_refused_and_stay_usable(capi, exact):
    W, H = 256, 64
    N = W * H
    ea, eb, ej = exact.square_lattice_edges(W, H, -1.0)
    y, x = np.divmod(np.arange(N), W)
    right = np.arange(len(ea)) % 2 == 0
    cases = {
        "field": capi.Graph(ea, eb, ej, N, biases=np.full(N, 0.5)),
        "open": capi.Graph(*[a[~(right & (np.repeat(x, 2) == W - 1))] for a in (ea, eb, ej)], N),
        "anisotropic": capi.Graph(ea, eb, np.where(right, -1.0, -2.0), N),
        "general-graph": capi.Graph(*exact.cubic_lattice_edges(8), 512),
    }
    seeds = capi.make_seeds(3, 2)
    for reason, g in cases.items():
        st = capi.States(g, seeds)
        with pytest.raises(ValueError, match=reason):
            st.set_icm_every(2)
        assert st.icm_every == 0
        st.do_time_steps(2, 0.4)   # still usable
        assert st.timestep == 2
    g = capi.Graph(ea, eb, ej, N)
    # Swendsen-Wang steps and isoenergetic cluster moves exclude each other, in both orders
    st = capi.States(g, seeds)
    st.set_cluster_every(2)
    with pytest.raises(ValueError, match="Swendsen-Wang"):
        st.set_icm_every(2)
    assert st.icm_every == 0 and st.cluster_every == 2
    st.set_cluster_every(0)
    st.set_icm_every(4)
    with pytest.raises(ValueError, match="isoenergetic"):
        st.set_cluster_every(2)
    assert st.icm_every == 4 and st.cluster_every == 0
    # tempering ladders
    assert not st.pt_can_attach(2, 0, 2, 1)
    with pytest.raises(ValueError, match="isoenergetic"):
        st.pt_attach([0.3, 0.5], 0, 2, 1, 7)
    st.set_icm_every(0)
    assert st.pt_can_attach(2, 0, 2, 1)
    st.pt_attach([0.3, 0.5], 0, 2, 1, 7)
    with pytest.raises(ValueError, match="ladder"):
        st.set_icm_every(3)
    assert st.icm_every == 0
    st.pt_detach()
    st.set_icm_every(3)
    assert st.icm_every == 3
    st.do_time_steps(3, 0.4)
    assert int(st.icm_stats()[2][0]) >= 1
    # shards: pairs follow the global experiment index
    six = capi.make_seeds(4, 6)
    for rng, reason in (((1, 4), "odd experiment index"), ((0, 3), "ends inside a pair"), ((3, 6), "odd experiment index")):
        shard = capi.States(g, six, replica_range=rng)
        with pytest.raises(ValueError, match=reason):
            shard.set_icm_every(1)
        assert shard.icm_every == 0
    for rng, n_total in (((2, 6), 6), ((0, 4), 6), ((4, 5), 5)):   # (4, 5) of 5: the last experiment has no partner anywhere
        shard = capi.States(g, six[:n_total], replica_range=rng)
        shard.set_icm_every(1)
        shard.do_time_steps(1, 0.4)


def test_energy_of_a_glass_against_metropolis(capi, exact):
    """128 x 64 +-J at beta = 0.5 (well above the glassy regime: the energy decorrelates in O(10) sweeps), 64 seeded replicas =
    32 pairs from random starts, 200 timesteps discarded and 400 used, per-step energies: icm_every = 2 against icm_every = 0
    with the same seeds; the pair means are the samples, |z| <= 4.  Measured with these seeds: z = +1.43."""
    W, H, R, beta = 128, 64, 64, 0.5
    g, _ = _graph(capi, exact, W, H, "glass")
    means = []
    for k in (2, 0):
        st = capi.States(g, capi.make_seeds(4242, R))
        st.set_icm_every(k)
        st.do_time_steps(200, beta)
        e = st.do_time_steps(400, beta, per_step_energies=True)
        means.append(e.mean(axis=1).reshape(R // 2, 2).mean(axis=1))
    icm, met = means
    z = (icm.mean() - met.mean()) / np.sqrt(icm.var(ddof=1) / len(icm) + met.var(ddof=1) / len(met))
    print(f"<E>/N ICM {icm.mean() / (W * H):.6f} Metropolis {met.mean() / (W * H):.6f} z {z:+.2f}")
    assert abs(z) <= 4.0

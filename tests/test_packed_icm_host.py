"""Isoenergetic cluster moves on the replica-packed general-graph paths: the numpy restatement the GPU tests
compare against, checked on its own -- exact conservation of E_a + E_b, the partnerless last experiment, the flip-table
indexing against single Philox calls, its step against a scalar reading of the spec, its chain against exact enumeration and
against Metropolis-only chains.  No GPU."""
import numpy as np

import packed_icm_reference as IR


def _random_graph(rng, n, n_edges):
    """Degree <= 6, +-J, a few isolated sites (the last three ids), one parallel edge."""
    deg = np.zeros(n, dtype=int)
    edges = []
    while len(edges) < n_edges:
        repeat = len(edges) == 5   # the sixth edge repeats the first
        a, b = edges[0] if repeat else (int(x) for x in rng.integers(0, n - 3, 2))
        if a != b and deg[a] < 6 and deg[b] < 6 and (repeat or ((a, b) not in edges and (b, a) not in edges)):
            edges.append((a, b))
            deg[a] += 1
            deg[b] += 1
    ea, eb = np.array([e[0] for e in edges], dtype=np.uint64), np.array([e[1] for e in edges], dtype=np.uint64)
    return ea, eb, rng.choice([-1.5, 1.5], len(edges))


def test_flip_table_indexing_against_single_philox_calls(oracle):
    """Root r: call r >> 3 with counter (uint32(t), call, "PKIF", ctr2(t, 0, 0)) and the group's key; word (r & 7) >> 1; half
    r & 1 (the low 16 bits are half 0); bit j of that half."""
    assert IR.DOM_FLIP == 0x504B4946
    seed, t = 0x0123456789ABCDEF, (5 << 32) + 7
    key = [seed & 0xFFFFFFFF, seed >> 32]
    hi = ((t >> 32) & 0xFFFF) << 16   # ctr2(t, 0, 0)
    words = IR.flip_words(256, seed, t)
    assert words.shape == (32, 4)
    for r, j in ((0, 0), (1, 0), (6, 15), (7, 3), (8, 9), (13, 15), (254, 1), (255, 14)):
        call = oracle.philox([t & 0xFFFFFFFF, r >> 3, 0x504B4946, hi], key)
        half = (int(call[(r & 7) >> 1]) >> (16 * (r & 1))) & 0xFFFF
        assert int(IR.flip_bit(words, r, j)) == (half >> j) & 1, (r, j)
    # hand-computed: position 13 is the HIGH half of word 2 of call 1
    call = oracle.philox([7, 1, 0x504B4946, 5 << 16], key)
    assert [int(IR.flip_bit(words, 13, j)) for j in range(16)] == [(int(call[2]) >> (16 + j)) & 1 for j in range(16)]


def test_step_equals_a_scalar_reading_of_the_spec(oracle):
    rng = np.random.default_rng(11)
    n, seed, t = 30, 0xFEDCBA9876543210, 3
    ea, eb, ej = _random_graph(rng, n, 50)
    G = IR.Graph(ea, eb, ej, n)
    spins = rng.integers(0, 2, (32, n)).astype(np.uint8)
    spins[9] = spins[8]                       # pair 4: nothing differs
    spins[11] = 1 - spins[10]                 # pair 5: everything differs
    moving = [True] * 15 + [False]
    new, clusters, largest, minus = IR.icm_step(G, spins, seed, t, moving)
    key = [seed & 0xFFFFFFFF, seed >> 32]
    adj = [[] for _ in range(n)]
    for a, b in zip(ea.astype(int), eb.astype(int)):
        adj[a].append(b)
        adj[b].append(a)
    for j in range(16):
        a, b = spins[2 * j], spins[2 * j + 1]
        want_a, want_b = a.copy(), b.copy()
        d = (a != b) & moving[j]
        seen, sizes = set(), []
        for s0 in range(n):
            if not d[s0] or s0 in seen:
                continue
            comp, queue = {s0}, [s0]
            while queue:
                x = queue.pop()
                for y in adj[x]:
                    if d[y] and y not in comp:
                        comp.add(y)
                        queue.append(y)
            seen |= comp
            sizes.append(len(comp))
            r = min(int(G.pos[i]) for i in comp)
            call = oracle.philox([t, r >> 3, 0x504B4946, 0], key)
            if (int(call[(r & 7) >> 1]) >> (16 * (r & 1) + j)) & 1:
                for i in comp:   # the two replicas swap their spins on the cluster
                    want_a[i], want_b[i] = b[i], a[i]
        assert np.array_equal(new[2 * j], want_a) and np.array_equal(new[2 * j + 1], want_b), j
        assert (clusters[j], largest[j], minus[j]) == (len(sizes), max(sizes, default=0), int(d.sum())), j
    assert minus[4] == 0 and clusters[4] == 0 and minus[5] == n
    assert np.array_equal(new[30:], spins[30:])      # a pair that does not move
    assert not np.array_equal(new[:30], spins[:30])


def test_energy_sum_of_a_pair_is_conserved_exactly(oracle, exact):
    """+-J: E_a + E_b of every pair is the same number before and after a move, and the configurations do change."""
    ea, eb, ej = IR.cubic_glass(exact)
    G = IR.Graph(ea, eb, ej, 216)
    seeds = oracle.make_seeds(5, 40)
    _, start, _ = oracle.pk_run(ea, eb, ej, 216, seeds, 3, betas=[0.6] * 3, per_step=True)
    e0 = np.array([G.energy(s) for s in start[:40]])
    states, e, stats = IR.run(G, seeds, 4, 1, betas=[0.6] * 4, states=start, t0=3)
    assert np.array_equal(e[0::2] + e[1::2], np.repeat((e0[0::2] + e0[1::2])[:, None], 4, axis=1))
    assert (states[:40] != start[:40]).any(axis=1).sum() >= 20 and (e[:, -1] != e0).any()   # (a cluster flipped twice is back)
    assert (stats[2] > 0).all() and (stats[0] >= 1).all() and (stats[1] <= stats[2]).all()
    # real couplings and biases: the same, within rounding of the sums
    rng = np.random.default_rng(1)
    ej_g, h = rng.normal(size=len(ea)), rng.normal(size=216)
    Gg = IR.Graph(ea, eb, ej_g, 216)
    e0 = np.array([oracle.energy(ea, eb, ej_g, 216, s, h) for s in start[:40]])
    new = IR.run(Gg, seeds, 1, 1, betas=[0.6], states=start, t0=0, biases=h, real=True)[0]
    e1 = np.array([oracle.energy(ea, eb, ej_g, 216, s, h) for s in new[:40]])
    bound = 4e-13 * (np.abs(ej_g).sum() + np.abs(h).sum())
    assert np.abs((e1[0::2] + e1[1::2]) - (e0[0::2] + e0[1::2])).max() <= bound and (e1 != e0).any()


def test_the_partnerless_last_experiment_follows_its_metropolis_trajectory(oracle):
    ea, eb, ej = _random_graph(np.random.default_rng(2), 40, 70)
    G = IR.Graph(ea, eb, ej, 40)
    seeds = oracle.make_seeds(9, 33)
    T = 6
    states, e, stats = IR.run(G, seeds, T, 2, betas=[0.5] * T)
    # a move takes the place of its timestep's sweep: the experiment without a partner (and the bits nobody owns) see the sweeps of
    # timesteps 0, 2, 4 alone and stay as they are at timesteps 1, 3, 5
    _, s_ref = oracle.pk_run(ea, eb, ej, 40, seeds, 0, betas=[])
    eps_ref = np.zeros(T)
    for t in range(T):
        if t % 2 == 0:
            _, s_ref = oracle.pk_run(ea, eb, ej, 40, seeds, 1, betas=[0.5], states=s_ref, t0=t)
        eps_ref[t] = G.energy(s_ref[32])
    assert np.array_equal(states[32:], s_ref[32:]) and np.array_equal(e[32], eps_ref)
    assert not np.array_equal(states[:32], s_ref[:32])
    assert all(len(x) == 16 for x in stats)
    # k = 2 in one call equals 3 + 3 timesteps in two; k = 0 is the oracle
    first = IR.run(G, seeds, 3, 2, betas=[0.5] * 3)
    second = IR.run(G, seeds, 3, 2, betas=[0.5] * 3, states=first[0], t0=3)
    assert np.array_equal(states, second[0]) and np.array_equal(e, np.concatenate([first[1], second[1]], axis=1))
    plain = IR.run(G, seeds, T, 0, betas=[0.5] * T)
    e_ref, s_ref, eps_ref = oracle.pk_run(ea, eb, ej, 40, seeds, T, betas=[0.5] * T, per_step=True)
    assert plain[2] is None and np.array_equal(plain[0], s_ref) and np.array_equal(plain[1], eps_ref)


def test_restatement_samples_the_boltzmann_distribution(exact, oracle):
    ea, eb, ej = IR.tri_glass()
    G = IR.Graph(ea, eb, ej, 16)
    T = IR.TRI_THERM + IR.TRI_STEPS
    _, e, _ = IR.run(G, oracle.make_seeds(IR.TRI_SEED, IR.TRI_CHAINS), T, 2, betas=[IR.TRI_BETA] * T)
    means = e[:, IR.TRI_THERM:].mean(axis=1)
    want = exact.enumerate_graph(ea, eb, ej, 16, IR.TRI_BETA)["E"]
    z = (means.mean() - want) / (means.std(ddof=1) / np.sqrt(IR.TRI_CHAINS))
    tau = IR.integrated_autocorrelation_time(e[:, IR.TRI_THERM:])
    print(f"<E> {means.mean():.4f} exact {want:.4f} z {z:+.2f} tau_int {tau:.2f}")
    assert abs(z) <= 5.0
    assert round(z, 2) == IR.TRI_Z and round(tau, 1) == IR.TRI_TAU   # the recorded figures are these


def test_restatement_agrees_with_metropolis_chains_on_a_cubic_glass(exact, oracle):
    G = IR.Graph(*IR.cubic_glass(exact), 216)
    T = IR.CUBIC_THERM + IR.CUBIC_STEPS
    out, taus = [], []
    for k, seed in zip((2, 0), IR.CUBIC_SEEDS):
        _, e, _ = IR.run(G, oracle.make_seeds(seed, IR.CUBIC_CHAINS), T, k, betas=[IR.CUBIC_BETA] * T)
        means = e[:, IR.CUBIC_THERM:].mean(axis=1)
        out.append((means.mean(), means.std(ddof=1) / np.sqrt(len(means))))
        taus.append(IR.integrated_autocorrelation_time(e[:, IR.CUBIC_THERM:]))
    z = (out[0][0] - out[1][0]) / np.hypot(out[0][1], out[1][1])
    print(f"moves <E> {out[0][0]:.2f} +- {out[0][1]:.2f}, Metropolis <E> {out[1][0]:.2f} +- {out[1][1]:.2f}, z {z:+.2f}, tau_int {taus}")
    assert abs(z) <= 5.0
    assert round(z, 2) == IR.CUBIC_Z and [round(t, 1) for t in taus] == [IR.CUBIC_TAU, IR.CUBIC_TAU_METROPOLIS]

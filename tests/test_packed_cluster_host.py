"""Swendsen-Wang cluster steps on the replica-packed general-graph path: the numpy restatement the GPU tests
compare against, checked on its own -- its labelling against a breadth-first search, its vectorised step against a scalar
reading of the spec, its chain against exact enumeration.  No GPU."""
import numpy as np
import pytest

import packed_cluster_reference as PR
from cluster_reference import bond_threshold


def _random_graph(rng, n, n_edges, parallel=True):
    """Degree <= 6, +-J, a few isolated sites (the last three ids), optionally one parallel edge."""
    deg = np.zeros(n, dtype=int)
    edges = []
    while len(edges) < n_edges:
        repeat = parallel and len(edges) == 5   # the sixth edge repeats the first
        a, b = edges[0] if repeat else (int(x) for x in rng.integers(0, n - 3, 2))
        if a != b and deg[a] < 6 and deg[b] < 6 and (repeat or ((a, b) not in edges and (b, a) not in edges)):
            edges.append((a, b))
            deg[a] += 1
            deg[b] += 1
    ea, eb = np.array([e[0] for e in edges], dtype=np.uint64), np.array([e[1] for e in edges], dtype=np.uint64)
    return ea, eb, rng.choice([-1.5, 1.5], len(edges))


def _bfs_labels(n, a, b):
    adj = [[] for _ in range(n)]
    for x, y in zip(a, b):
        adj[x].append(y)
        adj[y].append(x)
    lab = -np.ones(n, dtype=np.int64)
    for start in range(n):  # scanned in order: the first member of a cluster is its smallest
        if lab[start] >= 0:
            continue
        lab[start] = start
        queue = [start]
        while queue:
            x = queue.pop()
            for y in adj[x]:
                if lab[y] < 0:
                    lab[y] = start
                    queue.append(y)
    return lab


@pytest.mark.parametrize("p", [0.1, 0.4, 0.8, 1.0])
def test_labelling_equals_breadth_first_search(p):
    rng = np.random.default_rng(int(100 * p))
    for n, n_edges in ((12, 14), (40, 70), (300, 500)):
        ea, eb, _ = _random_graph(rng, n, n_edges)
        keep = rng.random(len(ea)) < p
        a, b = ea[keep].astype(np.int64), eb[keep].astype(np.int64)
        assert np.array_equal(PR.labels_from_bonds(n, a, b), _bfs_labels(n, a, b))
    ring = np.random.default_rng(1).permutation(500)   # one long chain in scrambled order: deep pointer chases
    assert not PR.labels_from_bonds(500, ring[:-1], ring[1:]).any()


def test_bond_ownership_and_positions(oracle):
    ea, eb, ej = _random_graph(np.random.default_rng(3), 60, 120)
    G = PR.Graph(ea, eb, ej, 60)
    assert len(G.owner) == len(ea) and G.n_pos % 256 == 0 and G.n_pos == 256 * G.n_colours
    assert (G.pos[G.owner] < G.pos[G.other]).all()
    # the slot is the bond's place in its owner's adjacency (edge-list order): (owner, slot) pairs are unique, parallel edges too
    assert len({(int(o), int(k)) for o, k in zip(G.owner, G.slot)}) == len(ea)
    assert G.slot.max() <= 5
    spins = np.random.default_rng(4).integers(0, 2, 60).astype(np.uint8)
    assert G.energy(spins) == oracle.energy(G.ea, G.eb, G.ej, 60, spins)
    words = G.pack(spins)
    assert sum(bin(int(w)).count("1") for w in words) == int(spins.sum())


def test_step_equals_a_scalar_reading_of_the_spec(oracle):
    """One group on a 30-site graph: every (bond, replica bit) uniform, label and flip bit drawn one Philox call at a time."""
    rng = np.random.default_rng(11)
    n, seed, t = 30, 0x0123456789ABCDEF, (5 << 32) + 7
    ea, eb, ej = _random_graph(rng, n, 50)
    G = PR.Graph(ea, eb, ej, n)
    spins = rng.integers(0, 2, (32, n)).astype(np.uint8)
    betas = np.linspace(0.0, 1.2, 32)
    thr = [bond_threshold(b, G.jabs) for b in betas]
    new, clusters, largest = PR.sw_step(G, spins, seed, t, thr)
    key = [seed & 0xFFFFFFFF, seed >> 32]
    hi = ((t >> 32) & 0xFFFF) << 16
    site_of = {int(p): i for i, p in enumerate(G.pos)}
    for b in (0, 5, 17, 31):
        a_pos, b_pos = [], []
        for own, oth, k, jpos in zip(G.owner, G.other, G.slot, G.jpos):
            satisfied = (spins[b, own] != spins[b, oth]) if jpos else (spins[b, own] == spins[b, oth])
            u = oracle.philox([t & 0xFFFFFFFF, int(G.pos[own]), PR.DOM_BOND, hi | (int(k) << 8) | (b >> 2)], key)[b & 3]
            if satisfied and int(u) < thr[b]:
                a_pos.append(int(G.pos[own]))
                b_pos.append(int(G.pos[oth]))
        lab = _bfs_labels(G.n_pos, a_pos, b_pos)
        want = spins[b].copy()
        for i in range(n):
            r = int(lab[G.pos[i]])
            want[i] ^= (int(oracle.philox([t & 0xFFFFFFFF, r >> 2, PR.DOM_FLIP, hi], key)[r & 3]) >> b) & 1
        assert np.array_equal(new[b], want), b
        roots = [int(lab[p]) for p in G.pos]
        assert clusters[b] == len(set(roots)) and largest[b] == max(roots.count(r) for r in set(roots))
        assert all(r in site_of for r in roots)   # a root is a real site: padding owns no bonds
    assert clusters[0] == n and largest[0] == 1   # beta = 0: no bond is active


def test_step_depends_on_seed_and_time_only():
    ea, eb, ej = PR.triangular_lattice_edges(5, 5)
    G = PR.Graph(ea, eb, ej, 25)
    spins = np.random.default_rng(1).integers(0, 2, (32, 25)).astype(np.uint8)
    thr = [bond_threshold(0.25, 1.0)] * 32
    a = PR.sw_step(G, spins, 11, 5, thr)[0]
    assert np.array_equal(a, PR.sw_step(G, spins.copy(), 11, 5, thr)[0])
    assert not np.array_equal(a, PR.sw_step(G, spins, 12, 5, thr)[0])
    assert not np.array_equal(a, PR.sw_step(G, spins, 11, 6, thr)[0])


def test_run_without_cluster_steps_is_the_oracle(oracle):
    ea, eb, ej = PR.triangular_lattice_edges(5, 5)
    G = PR.Graph(ea, eb, ej, 25)
    seeds = oracle.make_seeds(3, 40)
    states, energies, stats = PR.run(G, seeds, 5, 0, betas=[0.3] * 5)
    e_ref, s_ref, eps_ref = oracle.pk_run(ea, eb, ej, 25, seeds, 5, betas=[0.3] * 5, per_step=True)
    assert stats is None and np.array_equal(states, s_ref) and np.array_equal(energies, eps_ref)
    # k = 2 in one call equals 3 + 4 timesteps in two
    whole = PR.run(G, seeds, 7, 2, betas=[0.3] * 7)
    first = PR.run(G, seeds, 3, 2, betas=[0.3] * 3)
    second = PR.run(G, seeds, 4, 2, betas=[0.3] * 4, states=first[0], t0=3)
    assert np.array_equal(whole[0], second[0]) and np.array_equal(whole[1], np.concatenate([first[1], second[1]], axis=1))


@pytest.mark.parametrize("k", [1, 2])
def test_restatement_samples_the_boltzmann_distribution(exact, oracle, k):
    """Periodic 4 x 4 triangular ferromagnet, cluster_every = k, PR.TRI_CHAINS seeded chains from the random start: per-chain
    time averages of E after thermalisation against exact enumeration; standard error across the chains; |z| <= 5."""
    ea, eb, ej = PR.triangular_lattice_edges(4, 4, -1.0)
    G = PR.Graph(ea, eb, ej, 16)
    T = PR.TRI_THERM + PR.TRI_STEPS
    _, e, _ = PR.run(G, oracle.make_seeds(PR.TRI_SEED + k, PR.TRI_CHAINS), T, k, betas=[PR.TRI_BETA] * T)
    means = e[:, PR.TRI_THERM:].mean(axis=1)
    want = exact.enumerate_graph(ea, eb, ej, 16, PR.TRI_BETA)["E"]
    z = (means.mean() - want) / (means.std(ddof=1) / np.sqrt(PR.TRI_CHAINS))
    print(f"k = {k}: <E> {means.mean():.4f} exact {want:.4f} z {z:+.2f}")
    assert abs(z) <= 5.0


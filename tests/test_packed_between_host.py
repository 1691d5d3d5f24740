"""The numpy restatement of the isoenergetic cluster move between two replica-packed containers (DESIGN.md S13,
tests/packed_between_reference.py) on the CPU: labels against a breadth-first search, conservation of E_a + E_b, the move as
an involution, what does not move, the order of the pairs, a pinned flip bit, and the seeded physics of a copies=2 ladder on the
oracle-backed engine against exact enumeration."""
import numpy as np

import packed_between_reference as BR
import packed_icm_reference as IR
from packed_ladder_icm_engine import OraclePackedIcmEngine


def _cubic(exact, L=6):
    ea, eb, ej = IR.cubic_glass(exact, L)
    return BR.Graph(ea, eb, ej, L ** 3)


def _bfs_labels(G, d):
    """Smallest position of every d = 1 site's component, by breadth-first search over the edge list."""
    nbrs = [[] for _ in range(G.nvars)]
    for a, b in zip(G.ea.astype(int), G.eb.astype(int)):
        if a != b:
            nbrs[a].append(b)
            nbrs[b].append(a)
    lab = np.full(G.nvars, -1, dtype=np.int64)
    for s in np.nonzero(d)[0]:
        if lab[s] >= 0:
            continue
        comp, queue = [s], [s]
        lab[s] = 0
        while queue:
            x = queue.pop()
            for y in nbrs[x]:
                if d[y] and lab[y] < 0:
                    lab[y] = 0
                    comp.append(y)
                    queue.append(y)
        lab[comp] = G.pos[comp].min()
    return lab


def _random_states(rng, R, n, p=0.5):
    return (rng.random((R, n)) < p).astype(np.uint8)


def test_labels_against_a_breadth_first_search(oracle, exact):
    rng = np.random.default_rng(1)
    for G in (_cubic(exact), BR.Graph(*IR.tri_glass(), 16)):
        for p in (0.2, 0.5, 0.8):
            d = rng.random(G.nvars) < p
            lab = BR.cluster_labels(G, d)
            want = _bfs_labels(G, d)
            sites = np.nonzero(d)[0]
            assert np.array_equal(lab[G.pos[sites]], want[sites])


def test_energy_sum_is_conserved_and_the_move_is_an_involution(oracle, exact):
    G = _cubic(exact)
    rng = np.random.default_rng(2)
    A, B = _random_states(rng, 5, G.nvars), _random_states(rng, 6, G.nvars)
    seeds = oracle.make_seeds(9, 40)
    sa, sb = np.array([4, 0, 2]), np.array([1, 5, 3])
    A1, B1, stats = BR.move(G, A, B, sa, sb, seeds, 8, 3)
    assert not np.array_equal(A1, A) and all(s[2] > 0 and s[0] >= 1 and s[1] >= 1 for s in stats)
    for a, b in zip(sa, sb):
        assert G.energy(A[a]) + G.energy(B[b]) == G.energy(A1[a]) + G.energy(B1[b])   # integer energies: exactly
        assert np.array_equal(A1[a] ^ B1[b], A[a] ^ B[b])                             # the overlap does not move
    # d, the clusters and the flip bits are unchanged by the move: the same call again undoes it
    A2, B2, stats2 = BR.move(G, A1, B1, sa, sb, seeds, 8, 3)
    assert np.array_equal(A2, A) and np.array_equal(B2, B) and stats2 == stats
    # slots in no pair stay as they were
    for r in (1, 3):
        assert np.array_equal(A1[r], A[r])
    for r in (0, 2, 4):
        assert np.array_equal(B1[r], B[r])


def test_real_couplings_with_biases_conserve_the_sum(oracle, exact):
    ea, eb, _ = exact.cubic_lattice_edges(4, 1.0)
    rng = np.random.default_rng(3)
    ej, h = rng.normal(size=len(ea)), rng.normal(size=64)
    ej[5] = 0.0                                                   # a zero coupling joins clusters like any other stored edge
    G = BR.Graph(ea, eb, ej, 64)
    A, B = _random_states(rng, 3, 64), _random_states(rng, 3, 64)
    A1, B1, _ = BR.move(G, A, B, [0, 1, 2], [2, 0, 1], oracle.make_seeds(4, 3), 0, 7)
    energy = lambda s: oracle.rj_energy(G.ea, G.eb, G.ej, 64, s, h)
    bound = 4 * np.finfo(float).eps * (np.abs(ej).sum() + np.abs(h).sum())
    for a, b in zip([0, 1, 2], [2, 0, 1]):
        assert abs(energy(A[a]) + energy(B[b]) - energy(A1[a]) - energy(B1[b])) <= bound
    # the zero coupling's two ends, both d = 1, share a label although no other d = 1 path joins them
    d = np.zeros(64, dtype=bool)
    d[[int(ea[5]), int(eb[5])]] = True
    lab = BR.cluster_labels(G, d)
    assert lab[G.pos[int(ea[5])]] == lab[G.pos[int(eb[5])]]


def test_order_of_the_pairs_and_the_key_of_a(oracle, exact):
    G = _cubic(exact)
    rng = np.random.default_rng(4)
    A, B = _random_states(rng, 40, G.nvars), _random_states(rng, 37, G.nvars)
    seeds = oracle.make_seeds(11, 40)
    sa, sb = rng.permutation(40)[:37], rng.permutation(37)
    one = BR.move(G, A, B, sa, sb, seeds, 0, 5)
    order = rng.permutation(37)
    two = BR.move(G, A, B, sa[order], sb[order], seeds, 0, 5)
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])
    assert [one[2][i] for i in order] == two[2]
    # the flip bits are a's: slot 33 of a container that starts at experiment 0 is bit 1 of the group keyed by seed 32
    assert BR.slot_key(seeds, 0, 33) == (int(seeds[32]), 1)
    assert BR.slot_key(seeds, 8, 30) == (int(seeds[32]), 6)


def test_pinned_flip_bits(oracle):
    """Known answers of the "PKBF" flip table (key 0x0123456789ABCDEF, t = 2^32 + 5, global bit 9)."""
    assert BR.DOM_FLIP == 0x504B4246
    bits = BR.flip_bits(512, 0x0123456789ABCDEF, (1 << 32) + 5, 9)
    assert len(bits) == 512
    packed = np.packbits(bits, bitorder="little").view(np.uint32)
    assert [int(w) for w in packed[:4]] == PINNED_WORDS and int(bits.sum()) == PINNED_ONES
    # roots 0..127 are the four words of call 0, as the oracle's C Philox gives them from the counter and key written out by hand
    call0 = oracle.philox([5, 0, 0x504B4246, (1 << 16) | (9 << 8)], [0x89ABCDEF, 0x01234567])
    assert [int(w) for w in call0] == PINNED_WORDS
    other = BR.flip_bits(512, 0x0123456789ABCDEF, (1 << 32) + 5, 10)   # the replica's bit goes into the counter
    assert not np.array_equal(other, bits)


PINNED_WORDS = [0x2CADB0EE, 0x2B9F075D, 0x6C38CEFC, 0x81A019C6]
PINNED_ONES = 247


def _ladder(edges, factory):
    from pyisingmontecarlo_amd.tempering import ClassicalTempering

    pt = ClassicalTempering(edges, seed=BR.LADDER_SEED, engine_factory=factory, copies=2)
    for b in BR.LADDER_BETAS:
        pt.add_graph(b)
    pt.set_replica_cluster_update_every(BR.LADDER_K)
    return pt


def test_ladder_energies_against_exact_enumeration(oracle, exact):
    """ClassicalTempering(copies=2) on the oracle-backed engine, periodic 4 x 4 triangular +-J: <E> per rung and copy."""
    ea, eb, ej = IR.tri_glass()
    pt = _ladder((ea, eb, ej), lambda: OraclePackedIcmEngine(ea, eb, ej, 16, bit_sliced=True))
    pt.timesteps(BR.LADDER_THERM, BR.LADDER_ROUND_EVERY)
    means = np.array([pt.timesteps_sample(BR.LADDER_BATCH, BR.LADDER_ROUND_EVERY, BR.LADDER_BATCH)[1] for _ in range(BR.LADDER_BATCHES)])
    assert means.shape == (BR.LADDER_BATCHES, 2, len(BR.LADDER_BETAS))
    assert pt.get_total_swaps() > 0 and pt.get_replica_cluster_stats() is not None
    want = np.array([exact.enumerate_graph(ea, eb, ej, 16, b)["E"] for b in BR.LADDER_BETAS])
    z = (means.mean(axis=0) - want) / (means.std(axis=0, ddof=1) / np.sqrt(len(means)))
    print("z per copy and rung\n", np.round(z, 2))
    assert np.abs(z).max() < 3.5
    assert round(float(np.abs(z).max()), 2) == BR.LADDER_MAX_ABS_Z

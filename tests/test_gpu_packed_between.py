"""Isoenergetic cluster moves between two replica-packed containers of one family, and inside tempering ladders on them
(DESIGN.md S13), on the device against the numpy restatement of tests/packed_between_reference.py -- bit-exact: packed words with
their cleared padding, states(), energies() and the three statistics -- on both families, across pair blocks, batches, pair
orders, shards and the ladders' own permutations; the whole ClassicalTempering(copies=2) loop against the oracle-backed engine of
tests/packed_ladder_icm_engine.py on the on-stream and the host swap path; and every refusal."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _packed_between_worker as W
import packed_between_reference as BR
import packed_icm_reference as IR
from packed_ladder_icm_engine import OraclePackedIcmEngine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = float(np.finfo(np.float64).eps)


@pytest.fixture(autouse=True)
def _force_packed(monkeypatch):
    monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")


def _graph(capi, G, real=False, biases=None):
    if real:
        return capi.Graph(G.ea, G.eb, G.ej, nvars=G.nvars, biases=biases, stable_path=True)
    return capi.Graph(G.ea, G.eb, G.ej, nvars=G.nvars, force_general=True)


def _container(capi, g, seeds, real=False, replica_range=None):
    st = capi.States(g, seeds, replica_range=replica_range)
    assert st.family == ("packed_real" if real else "packed_bitsliced")
    return st


def _energies(oracle, G, spins, real, biases):
    if real:
        return np.array([oracle.rj_energy(G.ea, G.eb, G.ej, G.nvars, s, biases) for s in spins])
    return np.array([G.energy(s) for s in spins])


def _assert_is(oracle, G, st, want, real=False, biases=None):
    packed = st.packed()
    assert packed.shape == (st.count, G.n_pos // 32)
    for r in range(st.count):
        assert np.array_equal(packed[r], G.pack(want[r])), f"slot {r}: configurations differ"
    assert np.array_equal(st.states().astype(np.uint8), want)
    assert np.array_equal(st.energies(), _energies(oracle, G, want, real, biases))


def _stats(st, n):
    got = st.icm_between_stats()
    return [tuple(int(a[p]) for a in got) for p in range(n)]


def _move(oracle, G, a, b, sa, sb, seeds_a, first_a=0, real=False, biases=None):
    """a.icm_between(b, sa, sb) against the restatement; returns (A before, B before, A after, B after, statistics)."""
    A, B, t = a.states().astype(np.uint8), b.states().astype(np.uint8), a.timestep
    assert b.timestep == t
    a.icm_between(b, sa, sb)
    A1, B1, stats = BR.move(G, A, B, sa, sb, seeds_a, first_a, t)
    assert a.timestep == b.timestep == t + 1
    _assert_is(oracle, G, a, A1, real, biases)
    _assert_is(oracle, G, b, B1, real, biases)
    assert _stats(a, len(sa)) == stats
    return A, B, A1, B1, stats


def _cubic(exact, L):
    ea, eb, ej = IR.cubic_glass(exact, L)
    return BR.Graph(ea, eb, ej, L ** 3)


# ---- bit-sliced family ---------------------------------------------------------------------------------------------------
def test_two_pair_blocks_batches_and_the_order_of_the_pairs(capi, oracle, exact):
    """Cubic 6^3 +-J (n_pos = 512, padded classes), containers of 40 and 37 slots, 37 pairs through two different permutations:
    two pair blocks, the second with 5 pairs; pairs cross the group boundary in both containers; slots 37-39 of a stay
    unpaired.  Then one block per batch and the pairs in another order: the same words."""
    G = _cubic(exact, 6)
    assert G.n_pos == 512
    g = _graph(capi, G)
    seeds_a, seeds_b = capi.make_seeds(501, 40), capi.make_seeds(502, 37)
    rng = np.random.default_rng(6)
    sa, sb = rng.permutation(37), rng.permutation(37)
    assert not np.array_equal(sa, sb)
    out = []
    for workspace, order in ((None, np.arange(37)), (1, rng.permutation(37))):
        a, b = _container(capi, g, seeds_a), _container(capi, g, seeds_b)
        if workspace:
            a.set_option("cluster_workspace_bytes", workspace)
        for st in (a, b):
            st.do_time_steps(2, 0.6)
        with pytest.raises(ValueError, match="between containers"):
            a.icm_between_stats()
        A, B, A1, B1, stats = _move(oracle, G, a, b, sa[order], sb[order], seeds_a)
        assert np.array_equal(A1[37:], A[37:]) and not np.array_equal(A1[:37], A[:37])
        assert all(s[2] > 0 for s in stats)
        # integer energies: E_a + E_b of every pair exactly
        ea0, eb0, ea1, eb1 = (_energies(oracle, G, X, False, None) for X in (A, B, A1, B1))
        assert np.array_equal(ea0[sa] + eb0[sb], ea1[sa] + eb1[sb]) and not np.array_equal(ea0, ea1)
        inverse = np.argsort(order)
        out.append((a.packed(), b.packed(), [stats[i] for i in inverse]))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


def test_full_classes_with_sweeps_between_two_moves(capi, oracle, exact):
    """Cubic 8^3 +-J: classes of exactly 256 positions; the one-degree sweep kernel runs between two moves, and numbers its ties
    over all 32 bits of a group: the bits nobody owns must have stayed as the oracle has them."""
    G = _cubic(exact, 8)
    assert G.n_pos == 512
    g = _graph(capi, G)
    seeds = [capi.make_seeds(503, 34), capi.make_seeds(504, 33)]
    a, b = _container(capi, g, seeds[0]), _container(capi, g, seeds[1])
    assert a.graph.info.packed_degree == 6
    full = [oracle.pk_run(G.ea, G.eb, G.ej, G.nvars, s, 0, betas=[])[1] for s in seeds]   # uint8[64, nvars]: spare bits included
    rng = np.random.default_rng(8)
    t = 0
    for sweeps in (2, 2, 1):
        for st in (a, b):
            st.do_time_steps(sweeps, 0.5)
        full = [oracle.pk_run(G.ea, G.eb, G.ej, G.nvars, s, sweeps, betas=[0.5] * sweeps, states=f, t0=t)[1] for s, f in zip(seeds, full)]
        t += sweeps
        assert np.array_equal(a.states().astype(np.uint8), full[0][:34]) and np.array_equal(b.states().astype(np.uint8), full[1][:33])
        if sweeps == 1:
            break
        sa, sb = rng.permutation(34)[:33], rng.permutation(33)
        _, _, A1, B1, _ = _move(oracle, G, a, b, sa, sb, seeds[0])
        full[0][:34], full[1][:33] = A1, B1
        t += 1
        assert a.timestep == b.timestep == t
    assert a.timestep == b.timestep == 7


def _mixed_graph():
    """300 sites in scrambled id order, degrees 0..6, an isolated site, a parallel edge, +-J, odd cycles (the recipe of
    tests/test_gpu_packed_icm.py)."""
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
    return BR.Graph(ea, eb, 0.75 * rng.choice([-1.0, 1.0], len(edges)), n), deg


def test_mixed_degrees(capi, oracle):
    G, deg = _mixed_graph()
    assert G.n_colours >= 3 and deg.min() == 0 and deg.max() == 6
    g = _graph(capi, G)
    seeds_a, seeds_b = capi.make_seeds(505, 35), capi.make_seeds(506, 33)
    a, b = _container(capi, g, seeds_a), _container(capi, g, seeds_b)
    rng = np.random.default_rng(3)
    _move(oracle, G, a, b, rng.permutation(35)[:33], rng.permutation(33), seeds_a)   # from the random starts
    for st in (a, b):
        st.do_time_steps(2, 1.1)
    _move(oracle, G, a, b, rng.permutation(35)[:20], rng.permutation(33)[:20], seeds_a)


def test_scrambled_ring_one_cluster_and_no_cluster(capi, oracle):
    """A ring of 2000 sites whose ids are a random permutation.  Pair 0: a's slot all up, b's all down -- one cluster of 2000
    positions whose labels chase through the whole ring.  Pair 1: equal configurations -- nothing moves."""
    n = 2000
    order = np.random.default_rng(9).permutation(n).astype(np.uint64)
    G = BR.Graph(order, np.roll(order, -1), np.full(n, -1.0), n)
    g = _graph(capi, G)
    seeds_a, seeds_b = capi.make_seeds(507, 2), capi.make_seeds(508, 2)
    a, b = _container(capi, g, seeds_a), _container(capi, g, seeds_b)
    same = (np.random.default_rng(1).random(n) < 0.5).astype(np.uint8)
    a.set_state(0, np.ones(n, np.uint8))
    b.set_state(1, np.zeros(n, np.uint8))
    a.set_state(1, same)
    b.set_state(0, same)
    _, _, A1, B1, stats = _move(oracle, G, a, b, [0, 1], [1, 0], seeds_a)
    assert stats == [(1, n, n), (0, 0, 0)]
    assert (A1[0].all() and not B1[1].any()) or (B1[1].all() and not A1[0].any())   # uniform and opposite
    assert np.array_equal(A1[1], same) and np.array_equal(B1[0], same)


# ---- real-coupling family ------------------------------------------------------------------------------------------------
def _sum_bound(G, biases):
    """Four two-level energies, each rounded once at the scale of the sum of its terms' magnitudes: 4 ulp of sum |terms|."""
    return 4 * ULP * (np.abs(G.ej).sum() + (0.0 if biases is None else np.abs(biases).sum()))


def _check_pair_sums(oracle, G, biases, A, B, A1, B1, sa, sb):
    ea0, eb0, ea1, eb1 = (_energies(oracle, G, X, True, biases) for X in (A, B, A1, B1))
    drift = np.abs((ea0[sa] + eb0[sb]) - (ea1[sa] + eb1[sb])).max()
    print(f"largest |change of E_a + E_b| {drift:.3e}, bound {_sum_bound(G, biases):.3e}")
    assert drift <= _sum_bound(G, biases) and not np.array_equal(ea0, ea1)


def test_gaussian_glass_with_biases(capi, oracle, exact):
    """Gaussian J and Gaussian biases on cubic 6^3 (7 slots), 40 and 37 slots, after two sweeps."""
    ea, eb, _ = exact.cubic_lattice_edges(6, 1.0)
    rng = np.random.default_rng(2024)
    G = BR.Graph(ea, eb, rng.normal(size=len(ea)), 216)
    h = rng.normal(size=216)
    g = _graph(capi, G, real=True, biases=h)
    seeds_a, seeds_b = capi.make_seeds(509, 40), capi.make_seeds(510, 37)
    a, b = _container(capi, g, seeds_a, real=True), _container(capi, g, seeds_b, real=True)
    assert a.graph.info.real_slots == 7
    for st in (a, b):
        st.do_time_steps(2, 0.8)
    sa, sb = rng.permutation(37), rng.permutation(37)
    A, B, A1, B1, _ = _move(oracle, G, a, b, sa, sb, seeds_a, real=True, biases=h)
    _check_pair_sums(oracle, G, h, A, B, A1, B1, sa, sb)


def _degree_10_graph():
    rng = np.random.default_rng(10)
    n, pairs, deg = 300, set(), np.zeros(300, dtype=int)
    while len(pairs) < 1300:
        a, b = (int(v) for v in rng.integers(0, n, 2))
        if a != b and deg[a] < 10 and deg[b] < 10 and (min(a, b), max(a, b)) not in pairs:
            pairs.add((min(a, b), max(a, b)))
            deg[a] += 1
            deg[b] += 1
    pairs = sorted(pairs)
    rng.shuffle(pairs)
    ea, eb = np.array([p[0] for p in pairs], dtype=np.uint64), np.array([p[1] for p in pairs], dtype=np.uint64)
    ej = rng.normal(size=len(ea))
    ej[::40] = 0.0   # zero couplings: stored bonds like any other, they join clusters
    return BR.Graph(ea, eb, ej, n), deg


def test_degree_10_random_graph_with_zero_couplings(capi, oracle):
    G, deg = _degree_10_graph()
    assert deg.max() == 10 and (G.ej == 0.0).sum() >= 30
    g = _graph(capi, G, real=True)
    seeds_a, seeds_b = capi.make_seeds(511, 34), capi.make_seeds(512, 34)
    a, b = _container(capi, g, seeds_a, real=True), _container(capi, g, seeds_b, real=True)
    assert a.graph.info.real_slots == 11
    for st in (a, b):
        st.do_time_steps(1, 0.7)
    rng = np.random.default_rng(5)
    sa, sb = rng.permutation(34), rng.permutation(34)
    A, B, A1, B1, _ = _move(oracle, G, a, b, sa, sb, seeds_a, real=True)
    _check_pair_sums(oracle, G, None, A, B, A1, B1, sa, sb)


def test_a_shard_that_starts_at_experiment_8(capi, oracle, exact):
    """pk_bit0 = 8 on the real family, paired with an unsharded container, on either side of the call: slot s of the shard is bit
    8 + s of its group, and as `a` its flip bits are those of GLOBAL bit 8 + s of the group keyed by experiment 0's seed."""
    ea, eb, _ = exact.cubic_lattice_edges(6, 1.0)
    rng = np.random.default_rng(88)
    G = BR.Graph(ea, eb, rng.normal(size=len(ea)), 216)
    g = _graph(capi, G, real=True)
    seeds_all, seeds_b = capi.make_seeds(513, 30), capi.make_seeds(514, 20)
    shard, whole = _container(capi, g, seeds_all, real=True, replica_range=(8, 30)), _container(capi, g, seeds_b, real=True)
    assert shard.count == 22
    for st in (shard, whole):
        st.do_time_steps(2, 0.6)
    sa, sb = rng.permutation(22)[:20], rng.permutation(20)
    _move(oracle, G, shard, whole, sa, sb, seeds_all, first_a=8, real=True)
    _move(oracle, G, whole, shard, sb[:15], sa[:15], seeds_b, real=True)


# ---- the ladders' own permutations ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("real", [False, True])
def test_null_form_reads_the_permutations_on_the_device(capi, oracle, exact, real):
    """Two 12-rung ladders after exchange rounds: the move without tables == the restatement with the permutations read back;
    the exchange round right after it decides on the energies of the new configurations."""
    R = 12
    ea, eb, _ = exact.cubic_lattice_edges(6, 1.0)
    rng = np.random.default_rng(12)
    G = BR.Graph(ea, eb, rng.normal(size=len(ea)) if real else rng.choice([-1.0, 1.0], len(ea)), 216)
    g = _graph(capi, G, real=real)
    betas = np.linspace(0.5, 0.72, R)
    seeds_a, seeds_b = capi.make_seeds(515, R), capi.make_seeds(516, R)
    a, b = _container(capi, g, seeds_a, real=real), _container(capi, g, seeds_b, real=real)
    a.pt_attach(betas, 0, R, 1, 101)
    b.pt_attach(betas, 0, R, 1, 202)
    for st in (a, b):
        st.pt_run(12, 2)
    (pa, rounds_a, swaps_a), pb = a.pt_state(), b.pt_state()[0]
    assert not np.array_equal(pa, np.arange(R)) and not np.array_equal(pb, np.arange(R)) and not np.array_equal(pa, pb)
    A, B = a.states().astype(np.uint8), b.states().astype(np.uint8)
    a.icm_between(b)
    A1, B1, stats = BR.move(G, A, B, pa, pb, seeds_a, 0, 12)
    assert a.timestep == b.timestep == 13
    assert _stats(a, R) == stats and any(s[2] > 0 for s in stats)
    # a round at once: the host twin of the exchange step on the energies after the move
    for st, seed, perm, want, rounds, swaps in ((a, 101, pa, A1, rounds_a, swaps_a), (b, 202, pb, B1, *b.pt_state()[1:])):
        st.pt_measure()
        st.pt_swap()
        ref = np.array(perm, dtype=np.uint32)
        swaps += capi.pt_swap_round(seed, rounds, betas, _energies(oracle, G, want, real, None), ref)
        got = st.pt_state()
        assert np.array_equal(got[0], ref) and got[1] == rounds + 1 and got[2] == swaps
        _assert_is(oracle, G, st, want, real)


# ---- whole ladders -------------------------------------------------------------------------------------------------------
def _oracle_factory(family):
    ea, eb, ej = W.edges(family)
    return lambda: OraclePackedIcmEngine(ea, eb, ej, 216, bit_sliced=family == "pm")


@pytest.mark.parametrize("family", ["pm", "gauss"])
def test_whole_ladder_on_stream_equals_the_oracle_engine(capi, oracle, monkeypatch, family):
    """ClassicalTempering(copies=2) on 6^3, 8 rungs, a move every 3rd timestep, a round every 2nd: timesteps and
    timesteps_sample on the HIP engine (exchange rounds and moves on the stream) == the oracle-backed engine, bit for bit."""
    for name, value in W.ENV[family].items():
        monkeypatch.setenv(name, value)
    hip = W.ladder(family)
    got = W.run(hip)
    assert hip._on_stream and hip._pair[0]._states.family == W.FAMILY[family] and hip.get_total_swaps() > 0
    want = W.run(W.ladder(family, _oracle_factory(family)))
    assert len(got) == len(want)
    for n, (x, y) in enumerate(zip(got, want)):
        assert x.shape == y.shape and np.array_equal(x, y), f"array {n} differs"


@pytest.fixture(scope="module")
def host_path_child():
    """Both families' ladders on the host swap path, from a child process started with ISINGMC_PT_HOST=1."""
    env = dict(os.environ, ISINGMC_PT_HOST="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_packed_between_worker.py")], env=env, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("family", ["pm", "gauss"])
def test_whole_ladder_on_the_host_swap_path_equals_the_oracle_engine(oracle, host_path_child, family):
    child = host_path_child[family]
    assert not child["on_stream"] and child["family"] == W.FAMILY[family]
    assert child["digests"] == W.digests(W.run(W.ladder(family, _oracle_factory(family))))


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_both_containers_unchanged(capi, oracle, exact, monkeypatch):
    G = _cubic(exact, 6)
    g = _graph(capi, G)
    seeds_a, seeds_b = capi.make_seeds(517, 4), capi.make_seeds(518, 4)
    a, b = _container(capi, g, seeds_a), _container(capi, g, seeds_b)
    start = [a.packed(), b.packed()]
    ident = np.arange(4)

    def refused(match, x, y, *tables):
        before = [x.packed(), y.packed(), x.timestep, y.timestep]
        with pytest.raises(ValueError, match=match):
            x.icm_between(y, *tables)
        assert "" != capi.last_error()
        assert np.array_equal(x.packed(), before[0]) and np.array_equal(y.packed(), before[1]) and [x.timestep, y.timestep] == before[2:]

    # the f64 CSR family, on either side
    monkeypatch.delenv("ISINGMC_FORCE_PACKED")
    csr = capi.States(g, seeds_b)
    assert csr.family == "csr_f64"
    refused("general-graph", a, csr, ident, ident)
    refused("general-graph", csr, a, ident, ident)
    refused("general-graph", csr, capi.States(g, seeds_a), ident, ident)
    # one graph handle, two packed families: a graph created under ISINGMC_FORCE_REAL=1 carries both layouts, and a container
    # takes the family its own creation finds switched on
    monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
    monkeypatch.setenv("ISINGMC_FORCE_REAL", "1")
    both = _graph(capi, G)
    real = capi.States(both, seeds_b)
    monkeypatch.delenv("ISINGMC_FORCE_REAL")
    sliced = capi.States(both, seeds_a)
    assert real.family == "packed_real" and sliced.family == "packed_bitsliced"
    refused("bit-sliced.*real-coupling", sliced, real, ident, ident)
    refused("bit-sliced.*real-coupling", real, sliced, ident, ident)
    # timesteps, switches, tables
    late = _container(capi, g, seeds_b)
    late.do_time_steps(1, 0.5)
    refused("unequal timesteps", a, late, ident, ident)
    b.set_icm_every(2)
    refused("one non-local move at a time", a, b, ident, ident)
    b.set_icm_every(0)
    a.set_cluster_every(2)
    refused("one non-local move at a time", a, b, ident, ident)
    a.set_cluster_every(0)
    refused("duplicate slot", a, b, [0, 1, 1], [0, 1, 2])
    refused("duplicate slot", a, b, [0, 1, 2], [3, 1, 3])
    refused("out of range", a, b, [0, 4], [0, 1])
    refused("two different containers", a, a, ident, ident)
    # betas
    a.set_betas([0.3, 0.4, 0.5, 0.6])
    refused("one container only", a, b, ident, ident)
    b.set_betas([0.3, 0.4, 0.5, 0.7])
    refused("differ inside a pair", a, b, ident, ident)
    a.set_betas(None)
    b.set_betas(None)
    # ladders that do not match
    refused("ladder", a, b)
    betas = [0.3, 0.5, 0.7, 0.9]
    a.pt_attach(betas, 0, 4, 1, 7)
    refused("ladder", a, b)
    b.pt_attach([0.3, 0.5, 0.7, 0.95], 0, 4, 1, 8)
    refused("differ in their betas", a, b)
    five = _container(capi, g, capi.make_seeds(5, 5))
    five.pt_attach(betas + [1.0], 0, 5, 1, 9)
    refused("number of rungs", a, five)
    a.pt_detach()
    b.pt_detach()
    a.set_betas(None)
    b.set_betas(None)
    assert a.timestep == b.timestep == 0 and np.array_equal(a.packed(), start[0]) and np.array_equal(b.packed(), start[1])
    # after all of it: a move and sweeps as the restatement and the oracle do them
    _, _, A1, B1, _ = _move(oracle, G, a, b, ident, ident[::-1].copy(), seeds_a)
    for st, seeds, X in ((a, seeds_a, A1), (b, seeds_b, B1)):
        full = oracle.pk_run(G.ea, G.eb, G.ej, G.nvars, seeds, 0, betas=[])[1]
        full[:4] = X
        st.do_time_steps(2, 0.6)
        want = oracle.pk_run(G.ea, G.eb, G.ej, G.nvars, seeds, 2, betas=[0.6] * 2, states=full, t0=1)[1]
        assert np.array_equal(st.states().astype(np.uint8), want[:4])

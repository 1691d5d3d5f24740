"""Isoenergetic cluster moves between two containers and inside tempering ladders on the device: the move
against tests/icm_reference.py bit for bit (host slot tables, the ladders' own permutations), the whole ClassicalTempering(copies=2)
loop against the oracle-backed engine on every exchange path, cached measurements, the physics and every refusal.

A 4 x 4 sample cannot live on the device path of the move (the checkerboard kernels need W to be a multiple of 64): the exact
enumeration check of the ladder runs through the same ClassicalTempering code in tests/test_ladder_icm_host.py; here the glass is
compared with the ladder without moves instead, and the ferromagnet with Kaufman."""
import numpy as np
import pytest

import icm_reference as IR
from ladder_icm_engine import LadderRestatement, OracleIcmEngine

pytestmark = pytest.mark.gpu


def _edges(exact, W, H, J):
    if J == "glass":
        return exact.square_lattice_edges(W, H, -1.0, np.random.default_rng(W + 7 * H))
    return exact.square_lattice_edges(W, H, J)


def _reference_move(W, H, sa, sb, seeds_a, A, B, t):
    """A, B: bool[R, N] -> the same after the move of the pairs (sa[p], sb[p]) at timestep t, and the pairs' statistics."""
    A, B, stats = A.copy(), B.copy(), []
    for pa, pb in zip(sa, sb):
        a, b, st = IR.icm_step(A[pa].astype(np.uint8).reshape(H, W), B[pb].astype(np.uint8).reshape(H, W), int(seeds_a[pa]), t)
        A[pa], B[pb] = a.ravel().astype(bool), b.ravel().astype(bool)
        stats.append(st)
    return A, B, stats


def _stats(st, n):
    got = st.icm_between_stats()
    return [tuple(int(a[p]) for a in got) for p in range(n)]


@pytest.mark.parametrize("J", [-1.0, 1.0, "glass"])
@pytest.mark.parametrize("W,H", [(64, 4), (128, 64), (256, 64), (1024, 128)])
def test_moves_with_host_tables_are_bit_exact(capi, exact, W, H, J):
    """Identity, a random permutation and a proper subset of the slots, 5 and 6 replicas, after two sweeps; then the same with
    a workspace of one pair per batch."""
    ea, eb, ej = _edges(exact, W, H, J)
    g = capi.Graph(ea, eb, ej, W * H)
    seeds_a, seeds_b = capi.make_seeds(3000 + W + H, 5), capi.make_seeds(4000 + W + H, 6)
    rng = np.random.default_rng(W * H)
    tables = [(np.arange(5), np.arange(5)), (rng.permutation(5), rng.permutation(6)[:5]), (np.array([4, 1, 2]), np.array([0, 5, 1]))]
    for workspace in (None, 1):
        a, b = capi.States(g, seeds_a), capi.States(g, seeds_b)
        if workspace:
            a.set_option("cluster_workspace_bytes", workspace)
        for st in (a, b):
            st.do_time_steps(2, 0.6)
        with pytest.raises(ValueError, match="between containers"):
            a.icm_between_stats()
        for n, (sa, sb) in enumerate(tables):
            A, B = a.states(), b.states()
            a.icm_between(b, sa, sb)
            wantA, wantB, want_stats = _reference_move(W, H, sa, sb, seeds_a, A, B, 2 + n)
            assert np.array_equal(a.states(), wantA) and np.array_equal(b.states(), wantB)
            assert a.timestep == b.timestep == 3 + n
            assert _stats(a, len(sa)) == want_stats
            assert any(s[2] > 0 for s in want_stats) and not np.array_equal(wantA, A)


def test_move_with_equal_per_replica_betas_and_order_of_the_pairs(capi, exact):
    W, H = 256, 64
    g = capi.Graph(*_edges(exact, W, H, "glass"), W * H)
    seeds_a, seeds_b = capi.make_seeds(1, 4), capi.make_seeds(2, 4)
    out = []
    for order in ([0, 1, 2, 3], [2, 0, 3, 1]):
        a, b = capi.States(g, seeds_a), capi.States(g, seeds_b)
        a.set_betas([0.3, 0.5, 0.7, 0.9])
        b.set_betas([0.9, 0.7, 0.5, 0.3])
        sa, sb = np.array([0, 1, 2, 3])[order], np.array([3, 2, 1, 0])[order]
        a.icm_between(b, sa, sb)
        out.append((a.packed(), b.packed()))
        stats = _stats(a, 4)
        out.append([stats[order.index(p)] for p in range(4)])
    assert np.array_equal(out[0][0], out[2][0]) and np.array_equal(out[0][1], out[2][1]) and out[1] == out[3]


def test_ladder_form_reads_the_permutations_on_the_device(capi, exact):
    """Two ladders after exchange rounds: the move without tables == the move with the permutations read back."""
    W, H, G = 256, 64, 6
    g = capi.Graph(*_edges(exact, W, H, "glass"), W * H)
    betas = list(np.linspace(0.5, 0.503, G))
    runs = []
    for tables in (False, True):
        a, b = capi.States(g, capi.make_seeds(11, G)), capi.States(g, capi.make_seeds(12, G))
        a.pt_attach(betas, 0, G, 1, 101)
        b.pt_attach(betas, 0, G, 1, 202)
        for st in (a, b):
            st.pt_run(12, 2)
        pa, pb = a.pt_state()[0], b.pt_state()[0]
        A, B = a.states(), b.states()
        if tables:
            a.icm_between(b, pa, pb)
        else:
            a.icm_between(b)
        want = _reference_move(W, H, pa, pb, capi.make_seeds(11, G), A, B, 12)
        assert np.array_equal(a.states(), want[0]) and np.array_equal(b.states(), want[1]) and _stats(a, G) == want[2]
        assert a.timestep == b.timestep == 13
        for st in (a, b):   # the ladders go on
            st.pt_run(4, 2)
        runs.append((pa, pb, a.packed(), b.packed(), a.pt_state()[0], b.pt_state()[0]))
    assert not np.array_equal(runs[0][0], np.arange(G)) and not np.array_equal(runs[0][0], runs[0][1])
    for x, y in zip(*runs):
        assert np.array_equal(x, y)


def _ladder(edges, betas, seed, k, factory=None):
    from pyisingmontecarlo_amd.tempering import ClassicalTempering

    pt = ClassicalTempering(edges, seed=seed, engine_factory=factory, copies=2)
    for b in betas:
        pt.add_graph(float(b))
    pt.set_replica_cluster_update_every(k)
    return pt


def _snapshot(pt):
    return (pt.get_permutation(), pt.get_total_swaps(), [c._states.states() for c in pt._pair], [c._states.energies() for c in pt._pair],
            pt.get_replica_cluster_stats())


def _assert_equal_runs(x, y):
    assert np.array_equal(x[0], y[0]) and x[1] == y[1]
    for c in range(2):
        assert np.array_equal(x[2][c], y[2][c]) and np.array_equal(x[3][c], y[3][c])
    assert all(np.array_equal(p, q) for p, q in zip(x[4], y[4]))


@pytest.mark.parametrize("path", ["rounds", "in-kernel", "host"])
def test_whole_ladder_equals_the_oracle_engine(capi, oracle, exact, monkeypatch, path):
    """ClassicalTempering(copies=2) on the HIP engine == the same code on the oracle-backed engine: one library call per
    round, exchange rounds inside the strip launch (the 1024 x 128 x 8-rung shape), and the host swap step; one timesteps
    call == the same timesteps in several calls."""
    W, H, G = (1024, 128, 8) if path == "in-kernel" else (256, 64, 6)
    if path == "in-kernel":
        monkeypatch.setenv("ISINGMC_STRIP", "1")
        monkeypatch.setenv("ISINGMC_PT_IN_KERNEL", "1")
        k, f, calls = 9, 2, (20, 8)      # stretches of 8 sweeps = 4 rounds inside one launch between the moves
        betas = np.linspace(0.7, 0.728, G)
    else:
        k, f, calls = 3, 2, (6, 4, 12)
        betas = np.linspace(0.5, 0.503, G)
    if path == "host":
        monkeypatch.setenv("ISINGMC_PT_HOST", "1")
    edges = _edges(exact, W, H, "glass")
    jr, jd = IR.couplings(W, H, edges[2])
    hip, ref = _ladder(edges, betas, 77, k), _ladder(edges, betas, 77, k, lambda: OracleIcmEngine(W, H, jr, jd))
    for T in calls:
        hip.timesteps(T, f)
        ref.timesteps(T, f)
        _assert_equal_runs(_snapshot(hip), _snapshot(ref))
    assert hip._on_stream == (path != "host") and hip.get_total_swaps() > 0
    whole = _ladder(edges, betas, 77, k)   # every call above is a whole number of rounds: one call does the same
    whole.timesteps(sum(calls), f)
    _assert_equal_runs(_snapshot(whole), _snapshot(hip))


def test_sampling_loop_equals_the_oracle_engine(capi, oracle, exact):
    W, H, G = 128, 64, 4
    edges = _edges(exact, W, H, "glass")
    jr, jd = IR.couplings(W, H, edges[2])
    betas = np.linspace(0.5, 0.504, G)
    hip, ref = _ladder(edges, betas, 5, 3), _ladder(edges, betas, 5, 3, lambda: OracleIcmEngine(W, H, jr, jd))
    s1, e1 = hip.timesteps_sample(12, 4, 3)
    s2, e2 = ref.timesteps_sample(12, 4, 3)
    assert s1.shape == (2, G, 4, W * H) and np.array_equal(s1, s2) and np.array_equal(e1, e2)
    _assert_equal_runs(_snapshot(hip), _snapshot(ref))


class _StaleRestatement(LadderRestatement):
    """What a ladder would do that kept the energies measured BEFORE a move for the round after it."""

    def step(self):
        move = self.k and self.t % self.k == self.k - 1
        before = [self.energies(c) for c in range(2)]
        out = super().step()
        self.cached = before if move else None
        return out

    def energies(self, c):
        cached = getattr(self, "cached", None)
        if cached is not None and getattr(self, "_in_exchange", False):
            return cached[c]
        return super().energies(c)

    def exchange(self):
        self._in_exchange = True
        super().exchange()
        self._in_exchange = False


def test_a_round_right_after_a_move_uses_the_new_energies(capi, oracle, exact, monkeypatch):
    """1024 x 128 x 8 rungs on the strip kernel, whose last launch leaves the energies of the final sweep in the exchange buffer:
    a move every 3rd timestep and a round every 3rd, so that every round follows a move directly.  The swap decisions equal the
    restatement's; a restatement that keeps the energies from before the move decides differently on this sample."""
    W, H, G = 1024, 128, 8
    monkeypatch.setenv("ISINGMC_STRIP", "1")
    edges = _edges(exact, W, H, "glass")
    jr, jd = IR.couplings(W, H, edges[2])
    betas = np.linspace(0.7, 0.728, G)
    hip = _ladder(edges, betas, 2468, 3)
    ref, stale = LadderRestatement(capi, W, H, jr, jd, betas, 2468, 3), _StaleRestatement(capi, W, H, jr, jd, betas, 2468, 3)
    for T in (6, 3):
        hip.timesteps(T, 3)
        ref.timesteps(T, 3)
        stale.timesteps(T, 3)
    perm = hip.get_permutation()
    assert np.array_equal(perm[0], ref.perm[0]) and np.array_equal(perm[1], ref.perm[1]) and hip.get_total_swaps() == sum(ref.swaps)
    assert not (np.array_equal(stale.perm[0], ref.perm[0]) and np.array_equal(stale.perm[1], ref.perm[1]))
    for c in range(2):
        assert np.array_equal(hip._pair[c]._states.energies(), ref.energies(c))


def _batch_means(pt, therm, batches, length, f):
    pt.timesteps(therm, f)
    return np.array([pt.timesteps_sample(length, f, length)[1].mean(axis=0) for _ in range(batches)])


def test_ferromagnet_ladder_with_moves_against_kaufman(capi, exact):
    """64^2 ferromagnet, 2 copies x 6 rungs around beta_c, a move every 2nd timestep, a round every 2nd; 1000 timesteps
    discarded, 20 batches of 500: <E> per rung (both copies) against Kaufman, standard error from the batch means, |z| <= 4."""
    L, betas = 64, np.linspace(0.40, 0.48, 6)
    pt = _ladder(exact.square_lattice_edges(L, L, -1.0), betas, 31337, 2)
    means = _batch_means(pt, 1000, 20, 500, 2)
    for r, beta in enumerate(betas):
        want = exact.kaufman_energy(L, L, float(beta))
        z = (means[:, r].mean() - want) / (means[:, r].std(ddof=1) / np.sqrt(len(means)))
        print(f"beta {beta:.3f}: <E>/N {means[:, r].mean() / L ** 2:.5f} Kaufman {want / L ** 2:.5f} z {z:+.2f}")
    for r, beta in enumerate(betas):
        want = exact.kaufman_energy(L, L, float(beta))
        assert abs((means[:, r].mean() - want) / (means[:, r].std(ddof=1) / np.sqrt(len(means)))) <= 4.0


def test_glass_ladder_with_moves_against_the_ladder_without(capi, exact):
    """128 x 64 +-J, 2 copies x 6 rungs from beta 0.4 to 0.9, a round every 2nd timestep: a move every 2nd timestep against no
    moves, same seeds; 300 timesteps discarded, 16 batches of 200; the batch means are the samples, |z| <= 4 on every rung."""
    W, H, betas = 128, 64, np.linspace(0.4, 0.9, 6)
    edges = _edges(exact, W, H, "glass")
    icm = _batch_means(_ladder(edges, betas, 99, 2), 300, 16, 200, 2)
    met = _batch_means(_ladder(edges, betas, 99, 0), 300, 16, 200, 2)
    zs = (icm.mean(axis=0) - met.mean(axis=0)) / np.sqrt(icm.var(axis=0, ddof=1) / len(icm) + met.var(axis=0, ddof=1) / len(met))
    print("z per rung", np.round(zs, 2))
    assert np.all(np.abs(zs) <= 4.0)


def test_refusals_leave_both_containers_usable(capi, oracle, exact):
    W, H = 256, 64
    N = W * H
    ea, eb, ej = _edges(exact, W, H, "glass")
    g, g2 = capi.Graph(ea, eb, ej, N), capi.Graph(ea, eb, ej, N)
    seeds = capi.make_seeds(3, 4)
    a, b, other = capi.States(g, seeds), capi.States(g, capi.make_seeds(4, 4)), capi.States(g2, seeds)
    start = [a.packed(), b.packed()]
    ident = np.arange(4)

    def refused(match, x, y, *tables):
        with pytest.raises(ValueError, match=match):
            x.icm_between(y, *tables)
        assert "" != capi.last_error()

    refused("two different containers", a, a, ident, ident)
    refused("graph handles", a, other, ident, ident)
    refused("duplicate slot", a, b, [0, 1, 1], [0, 1, 2])
    refused("duplicate slot", a, b, [0, 1, 2], [3, 1, 3])
    refused("out of range", a, b, [0, 4], [0, 1])
    refused("ladder", a, b)
    late = capi.States(g, seeds)
    late.do_time_steps(1, 0.5)
    refused("unequal timesteps", a, late, ident, ident)
    a.set_betas([0.3, 0.4, 0.5, 0.6])
    b.set_betas([0.3, 0.4, 0.5, 0.7])
    refused("differ inside a pair", a, b, ident, ident)
    a.set_betas(None)
    b.set_betas(None)
    b.set_icm_every(2)
    refused("one non-local move at a time", a, b, ident, ident)
    b.set_icm_every(0)
    # ladders that do not match
    betas = [0.3, 0.5, 0.7, 0.9]
    a.pt_attach(betas, 0, 4, 1, 7)
    refused("ladder", a, b)
    b.pt_attach([0.3, 0.5, 0.7, 0.95], 0, 4, 1, 8)
    refused("differ in their betas", a, b)
    five = capi.States(g, capi.make_seeds(5, 5))
    five.pt_attach(betas + [1.0], 0, 5, 1, 9)
    refused("number of rungs", a, five)
    a.pt_detach()
    b.pt_detach()
    assert a.timestep == b.timestep == 0
    # graphs the move does not serve
    y, x = np.divmod(np.arange(N), W)
    for reason, graph in (("field", capi.Graph(ea, eb, ej, N, biases=np.full(N, 0.5))),
                          ("general-graph", capi.Graph(*exact.cubic_lattice_edges(8), 512))):
        u, v = capi.States(graph, capi.make_seeds(1, 64)), capi.States(graph, capi.make_seeds(2, 64))
        refused(reason, u, v, [0], [0])
        u.do_time_steps(2, 0.4)
        assert u.timestep == 2 and v.timestep == 0
    # after all of it: sweeps as the oracle does them
    lat = IR.make_lat(W, H, *IR.couplings(W, H, ej))
    for st, sd, p0 in ((a, seeds, start[0]), (b, capi.make_seeds(4, 4), start[1])):
        st.do_time_steps(3, 0.6)
        for r in range(4):
            want = p0[r].copy()
            for t in range(3):
                lat.sweep(want, int(sd[r]), t, 0.6)
            assert np.array_equal(st.packed()[r], want)

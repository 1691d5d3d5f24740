"""Spin and link overlaps between replica pairs on the device against the numpy rule of tests/overlap_reference.py,
which works from states() and the edge list alone -- integer equality everywhere: the checkerboard path and both replica-packed
families, the default pairing and arbitrary tables inside one container and between two, the cross-checks against the statistics
of the isoenergetic move and the magnetisation, purity, ladders, population annealing and every refusal."""
import numpy as np
import pytest

import overlap_reference as OR
import packed_icm_reference as IR

pytestmark = pytest.mark.gpu


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def _check(st, ea, eb, other=None, sa=None, sb=None):
    """st.overlaps(other, sa, sb) with and without the link overlap == the numpy rule; returns (spin, link)."""
    A = st.states()
    B = A if other is None else other.states()
    if sa is None:
        pa, pb = OR.default_pairs(st.count) if other is None else (np.arange(min(st.count, other.count)),) * 2
    else:
        pa, pb = sa, sb
    want_spin, want_link = OR.overlaps(A, B, ea, eb, pa, pb)
    spin, link = st.overlaps(other, sa, sb)
    assert spin.dtype == np.int64 and link.dtype == np.int64
    assert np.array_equal(spin, want_spin), (spin, want_spin)
    assert np.array_equal(link, want_link), (link, want_link)
    spin_only, none = st.overlaps(other, sa, sb, link=False)
    assert none is None and np.array_equal(spin_only, want_spin)
    return spin, link


def _tables(rng, n, count_a, count_b):
    """n pairs of slots: pair 0 = (r, r), a replica used twice, and -- from 33 pairs on -- pairs that cross the 32-bit words."""
    sa, sb = rng.integers(0, count_a, n), rng.integers(0, count_b, n)
    sa[0] = sb[0] = min(count_a, count_b) - 1
    if n >= 3:
        sa[2] = sa[1]
        sa[n - 1], sb[n - 1] = 1, count_b - 1
        sa[n - 2], sb[n - 2] = count_a - 1, 0
    return sa.astype(np.uint32), sb.astype(np.uint32)


def _check_tables(st, ea, eb, n_edges, rng, other=None):
    """Arbitrary tables of 1, 33 and 70 pairs: a partial pair block, one pair more than a block, three blocks."""
    b = st if other is None else other
    for n in (1, 33, 70):
        sa, sb = _tables(rng, n, st.count, b.count)
        spin, link = _check(st, ea, eb, other, sa, sb)
        if other is None:
            assert spin[0] == st.graph.nvars and link[0] == n_edges          # the pair (r, r)
            swapped = st.overlaps(None, sb, sa)
            assert np.array_equal(swapped[0], spin) and np.array_equal(swapped[1], link)
        else:
            swapped = other.overlaps(st, sb, sa)
            assert np.array_equal(swapped[0], spin) and np.array_equal(swapped[1], link)


def _lattice(capi, exact, W, H, glass):
    ea, eb, ej = exact.square_lattice_edges(W, H, -1.0, np.random.default_rng(5) if glass else None)
    g = capi.Graph(ea, eb, ej)
    assert g.kind == capi.KIND_LATTICE2D and g.info.fast_path == 0
    return g, ea, eb


# ---- 1. the checkerboard path ---------------------------------------------------------------------------------------------
# 64 x 4: the smallest lattice the recogniser serves (4 words per plane: one partial workgroup, tail threads); 256 x 64; and
# 192 x 344 (wpr = 3, 1032 words per plane: two workgroups per pair as the kernel is written -- a workgroup covers 1024 words --
# the second with 8 words)
@pytest.mark.parametrize("glass", [False, True])
@pytest.mark.parametrize("W,H", [(64, 4), (256, 64), (192, 344)])
def test_checkerboard_default_pairing(capi, exact, W, H, glass):
    g, ea, eb = _lattice(capi, exact, W, H, glass)
    for R in (2, 7, 40):   # 7: the last replica is unpaired
        st = capi.States(g, capi.make_seeds(100 + R, R))
        assert st.family == "checkerboard"
        st.do_time_steps(3, 0.5)
        spin, link = _check(st, ea, eb)
        assert len(spin) == R // 2 and np.all(np.abs(spin) < W * H)


@pytest.mark.parametrize("W,H", [(64, 4), (192, 344)])
def test_checkerboard_tables_and_two_containers(capi, exact, W, H):
    g, ea, eb = _lattice(capi, exact, W, H, True)
    a, b = capi.States(g, capi.make_seeds(11, 40)), capi.States(g, capi.make_seeds(12, 37))
    a.do_time_steps(3, 0.5)
    b.do_time_steps(2, 0.5)   # unequal timesteps are fine
    rng = np.random.default_rng(W)
    _check_tables(a, ea, eb, len(ea), rng)
    _check(a, ea, eb, b)                                   # identity pairing: 37 pairs
    assert len(a.overlaps(b)[0]) == 37
    _check(a, ea, eb, b, rng.permutation(40)[:37].astype(np.uint32), rng.permutation(37).astype(np.uint32))
    _check_tables(a, ea, eb, len(ea), rng, other=b)


# ---- 2. the bit-sliced packed family ------------------------------------------------------------------------------------------
@pytest.fixture
def force_packed(monkeypatch):
    monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")


def _diluted_graph():
    """300 sites in scrambled id order, degrees 0..6 (unused adjacency slots), an isolated site, a parallel edge, an entry
    a_e == b_e, +-J, odd cycles."""
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
    edges.insert(100, (7, 7))                   # graph creation accepts it: the constant term +1 of every link overlap
    ea = ids[[e[0] for e in edges]].astype(np.uint64)
    eb = ids[[e[1] for e in edges]].astype(np.uint64)
    assert deg.min() == 0 and deg.max() == 6
    return ea, eb, 0.75 * rng.choice([-1.0, 1.0], len(edges)), n


def test_bit_sliced_cubic_glass(capi, exact, force_packed):
    """Cubic 6^3 +-J: n_pos = 512 with padded classes.  40 and 33 replicas (a second group with 8 bits and with one, the last
    replica of 33 unpaired), then a shard whose bits start at bit 20 of a word and cross into the next."""
    ea, eb, ej = IR.cubic_glass(exact, 6)
    g = capi.Graph(ea, eb, ej, nvars=216, force_general=True)
    rng = np.random.default_rng(6)
    for R in (40, 33):
        st = capi.States(g, capi.make_seeds(200 + R, R))
        assert st.family == "packed_bitsliced"
        st.do_time_steps(3, 0.5)
        assert len(_check(st, ea, eb)[0]) == R // 2
        _check_tables(st, ea, eb, len(ea), rng)
    shard = capi.States(g, capi.make_seeds(207, 70), replica_range=(20, 50))
    assert shard.count == 30
    shard.do_time_steps(3, 0.5)
    assert len(_check(shard, ea, eb)[0]) == 15
    _check_tables(shard, ea, eb, len(ea), rng)
    whole = capi.States(g, capi.make_seeds(208, 37))
    whole.do_time_steps(2, 0.5)
    _check(shard, ea, eb, whole)
    _check_tables(shard, ea, eb, len(ea), rng, other=whole)
    _check_tables(whole, ea, eb, len(ea), rng, other=shard)


def test_bit_sliced_diluted_graph(capi, force_packed):
    ea, eb, ej, n = _diluted_graph()
    g = capi.Graph(ea, eb, ej, nvars=n, force_general=True)
    a, b = capi.States(g, capi.make_seeds(210, 40)), capi.States(g, capi.make_seeds(211, 37))
    assert a.family == "packed_bitsliced"
    a.do_time_steps(3, 0.5)
    b.do_time_steps(3, 0.5)
    rng = np.random.default_rng(7)
    _check(a, ea, eb)
    _check_tables(a, ea, eb, len(ea), rng)
    _check(a, ea, eb, b)
    _check_tables(a, ea, eb, len(ea), rng, other=b)


# ---- 3. the real-coupling packed family ---------------------------------------------------------------------------------------
def _degree_15_graph():
    """300 sites, degrees up to 15 (15 adjacency slots), Gaussian couplings with zeros among them, one duplicated entry and one
    entry a_e == b_e."""
    rng = np.random.default_rng(15)
    n, pairs, deg = 300, set(), np.zeros(300, dtype=int)
    while len(pairs) < 1900:
        a, b = (int(v) for v in rng.integers(0, n, 2))
        if a != b and deg[a] < 14 and deg[b] < 14 and (min(a, b), max(a, b)) not in pairs:
            pairs.add((min(a, b), max(a, b)))
            deg[a] += 1
            deg[b] += 1
    pairs = sorted(pairs)
    rng.shuffle(pairs)
    full = [p for p in pairs if deg[p[0]] == 14 and deg[p[1]] == 14]
    assert full, "no bond between two sites of degree 14 to duplicate"
    pairs.append((full[0][1], full[0][0]))   # the duplicate, the other way round: both ends get degree 15
    pairs.append((5, 5))
    ea, eb = np.array([p[0] for p in pairs], dtype=np.uint64), np.array([p[1] for p in pairs], dtype=np.uint64)
    ej = rng.normal(size=len(ea))
    ej[:-2:40] = 0.0   # zero couplings: stored bonds like any other
    return ea, eb, ej, n


def test_real_coupling_gaussian_glass_with_biases(capi, exact):
    ea, eb, _ = exact.cubic_lattice_edges(6, 1.0)
    rng = np.random.default_rng(2024)
    g = capi.Graph(ea, eb, rng.normal(size=len(ea)), nvars=216, biases=rng.normal(size=216), stable_path=True)
    a, b = capi.States(g, capi.make_seeds(300, 40)), capi.States(g, capi.make_seeds(301, 37))
    assert a.family == "packed_real" and g.info.real_slots == 7
    a.do_time_steps(3, 0.5)
    b.do_time_steps(3, 0.5)
    _check(a, ea, eb)
    _check_tables(a, ea, eb, len(ea), rng)
    _check(a, ea, eb, b)
    _check_tables(a, ea, eb, len(ea), rng, other=b)


def test_real_coupling_degree_15_zero_couplings_and_a_duplicate(capi):
    ea, eb, ej, n = _degree_15_graph()
    assert (ej == 0.0).sum() >= 30
    g = capi.Graph(ea, eb, ej, nvars=n, stable_path=True)
    st = capi.States(g, capi.make_seeds(302, 33))
    assert st.family == "packed_real" and g.info.real_slots == 15
    st.do_time_steps(3, 0.5)
    rng = np.random.default_rng(8)
    spin, link = _check(st, ea, eb)
    # the zeros and the duplicate show in the link overlap: without them the rule gives other numbers
    keep = ej != 0.0
    keep[-2] = False
    assert not np.array_equal(OR.overlaps(st.states(), st.states(), ea[keep], eb[keep], *OR.default_pairs(33))[1], link)
    _check_tables(st, ea, eb, len(ea), rng)
    shard = capi.States(g, capi.make_seeds(303, 60), replica_range=(8, 50))   # pk_bit0 = 8, 42 slots across two words
    shard.do_time_steps(2, 0.5)
    _check(shard, ea, eb)
    _check_tables(shard, ea, eb, len(ea), rng, other=st)


# ---- the arbitrary-pair form of both packed families in batches ---------------------------------------------------------------
@pytest.mark.parametrize("family", ["packed_bitsliced", "packed_real"])
def test_packed_tables_in_batches(capi, exact, force_packed, family):
    """70 pairs = three pair blocks, the last partly filled, inside one container and between two (40 and 37 replicas) of the 6^3
    cube: cluster_workspace_bytes = 1 cuts one block per batch, 1 << 30 takes all three in one.  Both against the numpy rule --
    the one anchor of the batches that shares no plan with the library (the series and the class form compare with this call)."""
    if family == "packed_bitsliced":
        ea, eb, ej = IR.cubic_glass(exact, 6)
        g = capi.Graph(ea, eb, ej, nvars=216, force_general=True)
    else:   # Gaussian couplings: the neighbour table of the real-coupling family
        ea, eb, _ = exact.cubic_lattice_edges(6, 1.0)
        g = capi.Graph(ea, eb, np.random.default_rng(2024).normal(size=len(ea)), nvars=216, stable_path=True)
    a, b = capi.States(g, capi.make_seeds(220, 40)), capi.States(g, capi.make_seeds(221, 37))
    assert a.family == family
    a.do_time_steps(3, 0.5)
    b.do_time_steps(2, 0.5)
    rng = np.random.default_rng(70)
    for other in (None, b):
        sa, sb = _tables(rng, 70, 40, 40 if other is None else 37)
        assert sa[2] == sa[1]   # a slot used twice
        got = []
        for workspace in (1, 1 << 30):
            a.set_option("cluster_workspace_bytes", workspace)
            got.append(_check(a, ea, eb, other, sa, sb))
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


# ---- 6. cross-checks against code that exists ------------------------------------------------------------------------------
def _three_paths(capi, exact, monkeypatch):
    """(graph, ea, eb) on the checkerboard path, then -- under ISINGMC_FORCE_PACKED=1 -- on the bit-sliced and the real-coupling
    family; a generator: the caller creates its containers before the next graph is made."""
    yield _lattice(capi, exact, 64, 4, True)
    monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
    ea, eb, ej = IR.cubic_glass(exact, 6)
    yield capi.Graph(ea, eb, ej, nvars=216, force_general=True), ea, eb
    rng = np.random.default_rng(31)
    yield capi.Graph(ea, eb, rng.normal(size=len(ea)), nvars=216, stable_path=True), ea, eb


def test_minus_sites_of_the_isoenergetic_move_and_the_magnetisation(capi, exact, monkeypatch):
    families = []
    for g, ea, eb in _three_paths(capi, exact, monkeypatch):
        st = capi.States(g, capi.make_seeds(400, 38))
        families.append(st.family)
        st.set_icm_every(4)
        st.do_time_steps(4, 0.5)                      # timestep 3 is the move: it flips both replicas, so d stays as it was
        minus = st.icm_stats()[2].astype(np.int64)
        spin, _ = _check(st, ea, eb)
        assert np.array_equal(g.nvars - spin, 2 * minus) and minus.max() > 0
        st.set_icm_every(0)
        st.set_state(5, np.ones(g.nvars, dtype=np.uint8))
        r = np.arange(38, dtype=np.uint32)
        spin, _ = _check(st, ea, eb, None, np.full(38, 5, dtype=np.uint32), r)
        assert np.array_equal(spin, st.magnetisations()) and spin[5] == g.nvars
    assert families == ["checkerboard", "packed_bitsliced", "packed_real"]


# ---- 7. purity -------------------------------------------------------------------------------------------------------------
def test_a_measurement_changes_nothing(capi, exact, monkeypatch):
    for g, ea, eb in _three_paths(capi, exact, monkeypatch):
        seeds = capi.make_seeds(500, 35)
        st, twin, other = capi.States(g, seeds), capi.States(g, seeds), capi.States(g, capi.make_seeds(501, 35))
        for c in (st, twin, other):
            c.do_time_steps(2, 0.5)
        before = [st.raw_state(), st.timestep, st.energies(), other.raw_state(), other.timestep]
        tables = np.random.default_rng(1).permutation(35).astype(np.uint32), np.arange(35, dtype=np.uint32)
        st.overlaps()
        st.overlaps(None, *tables)
        st.overlaps(other)
        st.overlaps(other, *tables, link=False)
        after = [st.raw_state(), st.timestep, st.energies(), other.raw_state(), other.timestep]
        for x, y in zip(before, after):
            assert np.array_equal(x, y)
        st.do_time_steps(2, 0.5)
        twin.do_time_steps(2, 0.5)
        assert np.array_equal(st.raw_state(), twin.raw_state()) and st.timestep == twin.timestep == 4


# ---- 8. ladders ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["lattice", "lattice_host_swaps", "bit_sliced", "real_coupling"])
def test_ladder_overlaps_in_rung_order(capi, exact, monkeypatch, case):
    from pyisingmontecarlo_amd.tempering import ClassicalTempering

    if case.startswith("lattice"):
        ea, eb, ej = exact.square_lattice_edges(64, 4, -1.0, np.random.default_rng(9))
        betas, family = np.linspace(0.3, 0.44, 8), "checkerboard"
        if case == "lattice_host_swaps":
            monkeypatch.setenv("ISINGMC_PT_HOST", "1")
    else:
        monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
        monkeypatch.setenv("ISINGMC_FORCE_REAL", "1" if case == "real_coupling" else "0")
        ea, eb, _ = exact.cubic_lattice_edges(6, 1.0)
        rng = np.random.default_rng(77)
        ej = rng.normal(size=len(ea)) if case == "real_coupling" else rng.choice([-1.0, 1.0], len(ea))
        betas, family = np.linspace(0.4, 0.61, 8), "packed_real" if case == "real_coupling" else "packed_bitsliced"
    pt = ClassicalTempering((ea, eb, ej), seed=4711, copies=2)
    for beta in betas:
        pt.add_graph(float(beta))
    pt.timesteps(24, 2)
    assert pt._on_stream == (case != "lattice_host_swaps") and pt._pair[0]._states.family == family
    perm = pt.get_permutation()
    assert pt.get_total_swaps() > 0 and not np.array_equal(perm[0], np.arange(8)) and not np.array_equal(perm[1], np.arange(8))
    A, B = (c._states.states()[perm[i]] for i, c in enumerate(pt._pair))   # the two copies' configurations in rung order
    want = OR.overlaps(A, B, ea, eb, np.arange(8), np.arange(8))
    spin, link = pt.get_overlaps()
    assert np.array_equal(spin, want[0]) and np.array_equal(link, want[1])
    spin_only, none = pt.get_overlaps(link=False)
    assert none is None and np.array_equal(spin_only, want[0])
    assert np.array_equal(pt.get_permutation(), perm)
    single = ClassicalTempering((ea, eb, ej), seed=4711)
    single.add_graph(0.4)
    with pytest.raises(ValueError, match="copies=2"):
        single.get_overlaps()


# ---- the persistent replicas of ClassicIsing, and 9. population annealing ---------------------------------------------------
def _edge_list(ea, eb, ej):
    return [((int(a), int(b)), float(j)) for a, b, j in zip(ea, eb, ej)]


def test_classic_ising_get_overlaps(exact):
    import py_monte_carlo

    ea, eb, ej = exact.square_lattice_edges(64, 4, -1.0, np.random.default_rng(3))
    ci = py_monte_carlo.ClassicIsing(_edge_list(ea, eb, ej), None, 7, 21)
    ci.run_monte_carlo(0.5, 3)
    states = np.array(ci.get_states())
    spin, link = ci.get_overlaps()
    want = OR.overlaps(states, states, ea, eb, *OR.default_pairs(7))
    assert spin.dtype == np.int64 and np.array_equal(spin, want[0]) and np.array_equal(link, want[1])
    pairs = np.array([[6, 0], [3, 3], [0, 6], [2, 5]])
    spin, link = ci.get_overlaps(pairs)
    want = OR.overlaps(states, states, ea, eb, pairs[:, 0], pairs[:, 1])
    assert np.array_equal(spin, want[0]) and np.array_equal(link, want[1]) and spin[1] == 256 and link[1] == 512
    spin_only, none = ci.get_overlaps(pairs=pairs, link=False)
    assert none is None and np.array_equal(spin_only, want[0])
    assert np.array_equal(np.array(ci.get_states()), states)
    with pytest.raises(ValueError, match="out of range"):
        ci.get_overlaps([[0, 7]])
    with pytest.raises(ValueError, match=r"\[n, 2\]"):
        ci.get_overlaps([0, 1, 2])
    wide = exact.square_lattice_edges(256, 4, -1.0)   # (a lattice with a field stays on the checkerboard path from 256 columns on)
    field = py_monte_carlo.ClassicIsing(_edge_list(*wide), 0.5, 4, 21)
    with pytest.raises(ValueError, match="field"):
        field.get_overlaps()


def test_population_annealing_overlaps_of_the_final_population(exact):
    import py_monte_carlo

    ea, eb, ej = exact.square_lattice_edges(64, 4, -1.0, np.random.default_rng(4))
    betas, R = [0.1, 0.3, 0.5], 21

    def run(**kw):
        return py_monte_carlo.Lattice(_edge_list(ea, eb, ej), seed_gen=77).run_population_annealing(betas, 3, R, **kw)

    res = run(measure_overlaps=True)
    pairs = np.stack([np.arange(10), np.arange(10) + 10], axis=1)
    assert res.overlap_pairs.dtype == np.int64 and np.array_equal(res.overlap_pairs, pairs)
    want = OR.overlaps(res.states, res.states, ea, eb, pairs[:, 0], pairs[:, 1])
    assert res.spin_overlaps.dtype == np.int64 and np.array_equal(res.spin_overlaps, want[0])
    assert res.link_overlaps.dtype == np.int64 and np.array_equal(res.link_overlaps, want[1])
    plain, again = vars(run()), vars(run())
    assert sorted(plain) == sorted(again) == sorted(set(vars(res)) - {"overlap_pairs", "spin_overlaps", "link_overlaps"})
    for key, value in plain.items():   # the measurement changed nothing else, and without the argument nothing changed at all
        for other in (again[key], vars(res)[key]):
            assert np.array_equal(np.asarray(value), np.asarray(other)), key


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals(capi, exact):
    W, H = 256, 4   # (fields, open boundaries and anisotropy stay on the checkerboard path from 256 columns on)
    N = W * H
    ea, eb, ej = exact.square_lattice_edges(W, H, -1.0)
    x = np.arange(N) % W
    right = np.arange(len(ea)) % 2 == 0
    seeds = capi.make_seeds(3, 6)
    one = np.zeros(1, dtype=np.uint32)
    cases = {
        "f64 CSR": capi.Graph(*exact.cubic_lattice_edges(6), 216),   # a small graph without the force flag
        "field": capi.Graph(ea, eb, ej, N, biases=np.full(N, 0.5)),
        "open": capi.Graph(*[a[~(right & (np.repeat(x, 2) == W - 1))] for a in (ea, eb, ej)], N),
        "anisotropic": capi.Graph(ea, eb, np.where(right, -1.0, -2.0), N),
    }
    for reason, g in cases.items():
        st = capi.States(g, seeds[:2])
        for args in ((), (None, one, one + 1), (capi.States(g, seeds[:2]),)):
            with pytest.raises(ValueError, match=reason):
                st.overlaps(*args)
        st.do_time_steps(2, 0.4)   # still usable
        assert st.timestep == 2
    assert capi.States(cases["f64 CSR"], seeds[:2]).family == "csr_f64"
    g = capi.Graph(ea, eb, ej)
    st = capi.States(g, seeds)
    with pytest.raises(ValueError, match="out of range"):
        st.overlaps(None, [0, 6], [1, 2])          # a slot equal to count
    with pytest.raises(ValueError, match="out of range"):
        st.overlaps(capi.States(g, capi.make_seeds(4, 3)), [0, 1], [1, 3])
    with pytest.raises(ValueError, match="different graph handles"):
        st.overlaps(capi.States(capi.Graph(ea, eb, ej), seeds))
    with pytest.raises(ValueError, match="odd experiment index"):
        capi.States(g, seeds, replica_range=(1, 5)).overlaps()
    with pytest.raises(ValueError, match="n_pairs is 0"):
        capi.States(g, seeds[:1]).overlaps()
    with pytest.raises(ValueError, match="n_pairs is 0"):
        st.overlaps(None, np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32))
    with pytest.raises(ValueError, match="both slot tables or neither"):
        st.overlaps(None, [0, 1], None)
    assert capi.last_error() != ""
    # an even lower bound is served, and tables on a shard with an odd one are too
    assert np.array_equal(capi.States(g, seeds, replica_range=(2, 6)).overlaps()[0], st.overlaps()[0][1:])
    odd = capi.States(g, seeds, replica_range=(1, 5))
    assert np.array_equal(odd.overlaps(None, [1, 0], [2, 3])[0], st.overlaps(None, [2, 1], [3, 4])[0])   # slot s = experiment 1 + s

"""The spin overlap resolved by a class label per site on the device against the numpy rule of
tests/class_overlap_reference.py, which works from states() alone -- integer equality everywhere: the checkerboard path (words
whose sites share a class and words that do not, the LDS limit), both replica-packed families (classes of one site, empty classes,
classes that span segments), the default pairing and arbitrary tables inside one container and between two, the invariants, purity,
ladders, ClassicIsing, population annealing, the normalisation of chi_SG end to end and every refusal."""
import numpy as np
import pytest

import class_overlap_reference as CR
import overlap_reference as OR
import packed_icm_reference as IR
from pyisingmontecarlo_amd import correlation as K

pytestmark = pytest.mark.gpu

NO_CLASS = CR.NO_CLASS


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def _pairs(st, other, sa, sb):
    if sa is not None:
        return sa, sb
    return OR.default_pairs(st.count) if other is None else (np.arange(min(st.count, other.count)),) * 2


def _check(st, cs, tables, other=None, sa=None, sb=None):
    """st.overlaps_by_class(cs, other, sa, sb) == the numpy rule; a second call and the two sides swapped return the same array;
    the classes of a table without NO_CLASS add up to the spin overlap.  Returns the array."""
    A = st.states()
    B = A if other is None else other.states()
    pa, pb = _pairs(st, other, sa, sb)
    want = CR.overlaps_by_class(A, B, tables, cs.n_classes, pa, pb)
    got = st.overlaps_by_class(cs, other, sa, sb)
    assert got.dtype == np.int64 and got.shape == (len(pa), cs.n_tables, cs.n_classes)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert np.array_equal(st.overlaps_by_class(cs, other, sa, sb), got)
    spin = st.overlaps(other, sa, sb, link=False)[0]
    for t, table in enumerate(np.atleast_2d(tables)):
        if not np.any(table == NO_CLASS):
            assert np.array_equal(got[:, t].sum(-1), spin)
    if sa is not None:
        swapped = (st if other is None else other).overlaps_by_class(cs, None if other is None else st, sb, sa)
        assert np.array_equal(swapped, got)
    return got


def _tables(rng, n, count_a, count_b):
    """n pairs of slots: pair 0 = (r, r), a replica used twice, and -- from 33 pairs on -- pairs that cross the 32-bit words."""
    sa, sb = rng.integers(0, count_a, n), rng.integers(0, count_b, n)
    sa[0] = sb[0] = min(count_a, count_b) - 1
    if n >= 3:
        sa[2] = sa[1]
        sa[n - 1], sb[n - 1] = 1, count_b - 1
        sa[n - 2], sb[n - 2] = count_a - 1, 0
    return sa.astype(np.uint32), sb.astype(np.uint32)


def _check_tables(st, cs, tables, rng, other=None):
    """Arbitrary tables of 1, 33 and 70 pairs: a partial pair block, one pair more than a block, three blocks."""
    b = st if other is None else other
    for n in (1, 33, 70):
        sa, sb = _tables(rng, n, st.count, b.count)
        got = _check(st, cs, tables, other, sa, sb)
        if other is None:
            assert np.array_equal(got[0], cs.sizes.astype(np.int64))   # the pair (r, r)


def _random_table(rng, nvars, n_classes, no_class=0.0):
    t = rng.integers(0, n_classes, nvars).astype(np.uint32)
    t[rng.random(nvars) < no_class] = NO_CLASS
    return t


def _lattice(capi, exact, W, H):
    ea, eb, ej = exact.square_lattice_edges(W, H, -1.0, np.random.default_rng(5))
    g = capi.Graph(ea, eb, ej)
    assert g.kind == capi.KIND_LATTICE2D and g.info.fast_path == 0
    return g


def _lattice_class_sets(capi, g, W, H):
    """(name, SiteClasses, tables): rows and columns (site y W + x: every word lies in one row, so the row table is served word by
    word and the column table bit by bit); five random classes with a tenth of the sites in none; at 192 x 344 two tables of 4096
    classes, n_tables * n_classes = 8192: the 32 KiB of LDS the limit states."""
    rng = np.random.default_rng(W + H)
    rows_cols = K.plane_classes((H, W))
    assert np.array_equal(rows_cols[0], np.arange(W * H) // W) and np.array_equal(rows_cols[1], np.arange(W * H) % W)
    sets = [("rows_cols", rows_cols, max(W, H)), ("random5", _random_table(rng, W * H, 5, 0.1)[None], 5)]
    if W * H > 8192:
        sets.append(("lds_limit", np.stack([_random_table(rng, W * H, 4096), _random_table(rng, W * H, 4096, 0.05)]), 4096))
    return [(name, capi.SiteClasses(g, t, n), t) for name, t, n in sets]


# ---- 1. the checkerboard path ---------------------------------------------------------------------------------------------
# 64 x 4: 4 words per plane (one partial workgroup, tail threads); 192 x 344: 1032 words per plane, so a second workgroup with 8
@pytest.mark.parametrize("W,H", [(64, 4), (192, 344)])
def test_checkerboard(capi, exact, W, H):
    g = _lattice(capi, exact, W, H)
    sets = _lattice_class_sets(capi, g, W, H)
    name, cs, tables = sets[0]
    assert cs.n_tables == 2 and cs.n_classes == max(W, H)
    assert np.array_equal(cs.sizes[0, :H], np.full(H, W)) and np.array_equal(cs.sizes[1, :W], np.full(W, H)) and cs.sizes.sum() == 2 * W * H
    for R in (2, 7, 40):   # 7: the last replica is unpaired
        st = capi.States(g, capi.make_seeds(100 + R, R))
        assert st.family == "checkerboard"
        st.do_time_steps(3, 0.5)
        for name, cs, tables in sets:
            got = _check(st, cs, tables)
            assert len(got) == R // 2 and np.any(got != cs.sizes.astype(np.int64)[None])
    a, b = st, capi.States(g, capi.make_seeds(12, 37))
    b.do_time_steps(2, 0.5)   # unequal timesteps are fine
    rng = np.random.default_rng(W)
    for name, cs, tables in sets:
        _check_tables(a, cs, tables, rng)
        assert len(_check(a, cs, tables, b)) == 37          # identity pairing
        _check_tables(a, cs, tables, rng, other=b)


def test_checkerboard_batches_under_the_workspace_option(capi, exact):
    """8 bytes per (pair, table, class): a workspace of 1000 bytes holds the 12 pairs' 2 x 64 accumulators in no fewer than 12 batches."""
    g = _lattice(capi, exact, 64, 4)
    cs, tables = capi.SiteClasses(g, K.plane_classes((4, 64))), K.plane_classes((4, 64))
    st = capi.States(g, capi.make_seeds(3, 25))
    st.do_time_steps(3, 0.5)
    whole = _check(st, cs, tables)
    st.set_option("cluster_workspace_bytes", 1000)
    assert np.array_equal(_check(st, cs, tables), whole)
    _check_tables(st, cs, tables, np.random.default_rng(2))


# ---- 2. the bit-sliced packed family ------------------------------------------------------------------------------------------
@pytest.fixture
def force_packed(monkeypatch):
    monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")


def _cubic_tables(L):
    """The three axis tables of a cubic lattice with site (z L + y) L + x, and a table with a class of one site (3), an empty class
    (1) and sites in no class."""
    axes = K.plane_classes((L, L, L))
    odd = np.zeros(L ** 3, dtype=np.uint32)
    odd[1::3] = 2
    odd[2::7] = NO_CLASS
    odd[100] = 3
    assert (odd == 3).sum() == 1 and not (odd == 1).any() and (odd == NO_CLASS).any() and L > 3
    return np.concatenate([axes, odd[None]])


@pytest.mark.parametrize("L", [6, 12])
def test_bit_sliced_cubic_glass(capi, exact, force_packed, L):
    """6^3: n_pos = 512 with padded classes.  12^3: 1728 sites, so the single class of the one-class table spans two segments of
    at most 1024 positions.  40 and 33 replicas (a second group with 8 bits and with one, the last replica of 33 unpaired), a
    shard whose bits start at bit 20 of a word and cross into the next, two containers."""
    ea, eb, ej = IR.cubic_glass(exact, L)
    g = capi.Graph(ea, eb, ej, nvars=L ** 3, force_general=True)
    tables = _cubic_tables(L)
    one = np.zeros((1, L ** 3), dtype=np.uint32)
    sets = [(capi.SiteClasses(g, tables), tables), (capi.SiteClasses(g, one), one)]
    assert sets[0][0].n_classes == L and sets[0][0].sizes[0, 0] == L * L and sets[0][0].sizes[3, 3] == 1 and sets[0][0].sizes[3, 1] == 0
    assert sets[1][0].sizes.tolist() == [[L ** 3]]
    rng = np.random.default_rng(6)
    for R in (40, 33):
        st = capi.States(g, capi.make_seeds(200 + R, R))
        assert st.family == "packed_bitsliced"
        st.do_time_steps(3, 0.5)
        for cs, t in sets:
            assert len(_check(st, cs, t)) == R // 2
            _check_tables(st, cs, t, rng)
    shard = capi.States(g, capi.make_seeds(207, 70), replica_range=(20, 50))
    whole = capi.States(g, capi.make_seeds(208, 37))
    shard.do_time_steps(3, 0.5)
    whole.do_time_steps(2, 0.5)
    for cs, t in sets:
        assert len(_check(shard, cs, t)) == 15
        _check_tables(shard, cs, t, rng)
        _check(shard, cs, t, whole)
        _check_tables(shard, cs, t, rng, other=whole)
        _check_tables(whole, cs, t, rng, other=shard)


def test_packed_batches_under_the_workspace_option(capi, exact, force_packed):
    ea, eb, ej = IR.cubic_glass(exact, 6)
    g = capi.Graph(ea, eb, ej, nvars=216, force_general=True)
    tables = _cubic_tables(6)
    cs = capi.SiteClasses(g, tables)
    st = capi.States(g, capi.make_seeds(9, 70))   # three replica groups, three pair blocks of the tabled form
    st.do_time_steps(3, 0.5)
    whole = _check(st, cs, tables)
    st.set_option("cluster_workspace_bytes", 1)   # one group / one pair block per batch
    assert np.array_equal(_check(st, cs, tables), whole)
    _check_tables(st, cs, tables, np.random.default_rng(4))


# ---- 3. the real-coupling packed family ---------------------------------------------------------------------------------------
def test_real_coupling_gaussian_glass_with_biases(capi):
    ea, eb, ej, n, biases = CR.gaussian_glass_2d()
    g = capi.Graph(ea, eb, ej, nvars=n, biases=biases, stable_path=True)
    rng = np.random.default_rng(31)
    tables = np.stack([_random_table(rng, n, 9), _random_table(rng, n, 9, 0.2), K.plane_classes((10, 12))[0]])
    cs = capi.SiteClasses(g, tables)
    a, b = capi.States(g, capi.make_seeds(300, 40)), capi.States(g, capi.make_seeds(301, 37))
    assert a.family == "packed_real"
    a.do_time_steps(3, 0.5)
    b.do_time_steps(3, 0.5)
    _check(a, cs, tables)
    _check_tables(a, cs, tables, rng)
    _check(a, cs, tables, b)
    _check_tables(a, cs, tables, rng, other=b)


def test_real_coupling_degree_15(capi):
    ea, eb, ej, n = CR.degree_15_graph()
    g = capi.Graph(ea, eb, ej, nvars=n, stable_path=True)
    rng = np.random.default_rng(8)
    tables = np.stack([_random_table(rng, n, 40), _random_table(rng, n, 3, 0.3)])
    cs = capi.SiteClasses(g, tables, 40)
    st = capi.States(g, capi.make_seeds(302, 33))
    assert st.family == "packed_real" and g.info.real_slots == 15
    st.do_time_steps(3, 0.5)
    _check(st, cs, tables)
    _check_tables(st, cs, tables, rng)
    shard = capi.States(g, capi.make_seeds(303, 60), replica_range=(8, 50))   # pk_bit0 = 8, 42 slots across two words
    shard.do_time_steps(2, 0.5)
    _check(shard, cs, tables)
    _check_tables(shard, cs, tables, rng, other=st)


# ---- 4. purity on all three paths ------------------------------------------------------------------------------------------
def _three_paths(capi, exact, monkeypatch):
    """(graph, tables) on the checkerboard path, then -- under ISINGMC_FORCE_PACKED=1 -- on the bit-sliced and the real-coupling
    family; a generator: the caller creates its containers before the next graph is made."""
    yield _lattice(capi, exact, 64, 4), K.plane_classes((4, 64))
    monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
    ea, eb, ej = IR.cubic_glass(exact, 6)
    yield capi.Graph(ea, eb, ej, nvars=216, force_general=True), _cubic_tables(6)
    rng = np.random.default_rng(31)
    yield capi.Graph(ea, eb, rng.normal(size=len(ea)), nvars=216, stable_path=True), _cubic_tables(6)


def test_a_measurement_changes_nothing(capi, exact, monkeypatch):
    families = []
    for g, tables in _three_paths(capi, exact, monkeypatch):
        cs = capi.SiteClasses(g, tables)
        seeds = capi.make_seeds(500, 35)
        st, twin, other = capi.States(g, seeds), capi.States(g, seeds), capi.States(g, capi.make_seeds(501, 35))
        families.append(st.family)
        for c in (st, twin, other):
            c.do_time_steps(2, 0.5)
        before = [st.raw_state(), st.states(), st.timestep, st.energies(), other.raw_state(), other.timestep]
        slots = np.random.default_rng(1).permutation(35).astype(np.uint32), np.arange(35, dtype=np.uint32)
        st.overlaps_by_class(cs)
        st.overlaps_by_class(cs, None, *slots)
        st.overlaps_by_class(cs, other)
        st.overlaps_by_class(cs, other, *slots)
        after = [st.raw_state(), st.states(), st.timestep, st.energies(), other.raw_state(), other.timestep]
        for x, y in zip(before, after):
            assert np.array_equal(x, y)
        st.do_time_steps(3, 0.5)
        twin.do_time_steps(3, 0.5)
        assert np.array_equal(st.raw_state(), twin.raw_state()) and st.timestep == twin.timestep == 5
    assert families == ["checkerboard", "packed_bitsliced", "packed_real"]


# ---- 5. ladders ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["lattice", "bit_sliced"])
def test_ladder_overlaps_by_class_in_rung_order(capi, exact, monkeypatch, case):
    from pyisingmontecarlo_amd.tempering import ClassicalTempering

    if case == "lattice":
        ea, eb, ej = exact.square_lattice_edges(64, 4, -1.0, np.random.default_rng(9))
        betas, family, tables = np.linspace(0.3, 0.44, 8), "checkerboard", K.plane_classes((4, 64))
    else:
        monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
        monkeypatch.setenv("ISINGMC_FORCE_REAL", "0")
        ea, eb, _ = exact.cubic_lattice_edges(6, 1.0)
        ej = np.random.default_rng(77).choice([-1.0, 1.0], len(ea))
        betas, family, tables = np.linspace(0.4, 0.61, 8), "packed_bitsliced", _cubic_tables(6)
    pt = ClassicalTempering((ea, eb, ej), seed=4711, copies=2)
    for beta in betas:
        pt.add_graph(float(beta))
    pt.timesteps(24, 2)
    assert pt._pair[0]._states.family == family
    perm = pt.get_permutation()
    assert pt.get_total_swaps() > 0 and not np.array_equal(perm[0], np.arange(8)) and not np.array_equal(perm[1], np.arange(8))
    A, B = (c._states.states()[perm[i]] for i, c in enumerate(pt._pair))   # the two copies' configurations in rung order
    n_classes = int(tables[tables != NO_CLASS].max()) + 1
    want = CR.overlaps_by_class(A, B, tables, n_classes, np.arange(8), np.arange(8))
    got = pt.get_overlaps_by_class(tables)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    cs = pt.site_classes(tables, n_classes + 2)   # a class set built once; two empty classes more
    again = pt.get_overlaps_by_class(cs)
    assert again.shape == (8, len(tables), n_classes + 2) and np.array_equal(again[..., :n_classes], want) and not again[..., n_classes:].any()
    assert np.array_equal(got[:, 0].sum(-1), pt.get_overlaps(link=False)[0]) and np.array_equal(pt.get_permutation(), perm)
    single = ClassicalTempering((ea, eb, ej), seed=4711)
    single.add_graph(0.4)
    with pytest.raises(ValueError, match="copies=2"):
        single.get_overlaps_by_class(tables)


# ---- 6. the persistent replicas of ClassicIsing, and population annealing ---------------------------------------------------
def _edge_list(ea, eb, ej):
    return [((int(a), int(b)), float(j)) for a, b, j in zip(ea, eb, ej)]


def test_classic_ising_get_overlaps_by_class(exact):
    import py_monte_carlo

    ea, eb, ej = exact.square_lattice_edges(64, 4, -1.0, np.random.default_rng(3))
    ci = py_monte_carlo.ClassicIsing(_edge_list(ea, eb, ej), None, 7, 21)
    ci.run_monte_carlo(0.5, 3)
    states = np.array(ci.get_states())
    tables = K.plane_classes((4, 64))
    got = ci.get_overlaps_by_class(tables)
    assert got.dtype == np.int64 and np.array_equal(got, CR.overlaps_by_class(states, states, tables, 64, *OR.default_pairs(7)))
    pairs = np.array([[6, 0], [3, 3], [0, 6], [2, 5]])
    one = np.where(np.arange(256) % 5 == 0, NO_CLASS, np.arange(256) % 3)   # a single table, given as a 1-d array
    got = ci.get_overlaps_by_class(one, n_classes=4, pairs=pairs)
    assert got.shape == (4, 1, 4) and np.array_equal(got, CR.overlaps_by_class(states, states, one, 4, pairs[:, 0], pairs[:, 1]))
    assert np.array_equal(got[1, 0], CR.class_sizes(one, 4)[0].astype(np.int64)) and np.array_equal(got[0], got[2])
    assert np.array_equal(ci.get_overlaps_by_class(tables, pairs=pairs).sum(-1)[:, 0], ci.get_overlaps(pairs, link=False)[0])
    assert np.array_equal(np.array(ci.get_states()), states)
    with pytest.raises(ValueError, match="out of range"):
        ci.get_overlaps_by_class(tables, pairs=[[0, 7]])
    with pytest.raises(ValueError, match="class value out of range"):
        ci.get_overlaps_by_class(tables, n_classes=63)
    with pytest.raises(ValueError, match="nvars entries"):
        ci.get_overlaps_by_class(tables[:, :-1])


def test_population_annealing_overlaps_by_class(exact):
    import py_monte_carlo

    ea, eb, ej = exact.square_lattice_edges(64, 4, -1.0, np.random.default_rng(4))
    betas, R, tables = [0.1, 0.3, 0.5], 21, K.plane_classes((4, 64))

    def run(**kw):
        return py_monte_carlo.Lattice(_edge_list(ea, eb, ej), seed_gen=77).run_population_annealing(betas, 3, R, **kw)

    res = run(measure_overlaps=True, overlap_classes=tables)
    pairs = res.overlap_pairs
    assert np.array_equal(pairs, np.stack([np.arange(10), np.arange(10) + 10], axis=1))
    want = CR.overlaps_by_class(res.states, res.states, tables, 64, pairs[:, 0], pairs[:, 1])
    assert res.overlaps_by_class.dtype == np.int64 and np.array_equal(res.overlaps_by_class, want)
    assert np.array_equal(res.overlaps_by_class[:, 1].sum(-1), res.spin_overlaps)
    plain = vars(run(measure_overlaps=True))
    assert sorted(plain) == sorted(set(vars(res)) - {"overlaps_by_class"})
    for key, value in plain.items():   # the measurement changed nothing else
        assert np.array_equal(np.asarray(value), np.asarray(vars(res)[key])), key
    with pytest.raises(ValueError, match="needs measure_overlaps"):
        run(overlap_classes=tables)


# ---- 7. the normalisation, end to end --------------------------------------------------------------------------------------
def test_chi_sg_of_independent_spins_is_one(capi, exact):
    """At beta = 0 the overlap q_i of two replicas is an independent fair sign per site, so |q_hat(k_1)|^2 / N is exponentially
    distributed with mean 1 for every pair: the mean over 128 pairs has standard error 1 / sqrt(128)."""
    W = H = 64
    g = _lattice(capi, exact, W, H)
    tables = K.plane_classes((H, W))
    cs = capi.SiteClasses(g, tables)
    st = capi.States(g, capi.make_seeds(2718, 256))
    st.do_time_steps(2, 0.0)
    planes = st.overlaps_by_class(cs)
    assert planes.shape == (128, 2, 64)
    chi = K.chi_sg(planes, W * H)
    S = st.states()
    ref = K.chi_sg(CR.overlaps_by_class(S, S, tables, 64, *OR.default_pairs(256)), W * H)
    for axis in range(2):
        mean = chi[:, axis, 1].mean()
        print(f"axis {axis}: mean chi_SG(k_1) over 128 pairs = {mean:.6f}")
        assert mean == ref[:, axis, 1].mean()
        assert abs(mean - 1.0) < 5.0 / np.sqrt(128)
    spin2 = st.overlaps(link=False)[0].astype(np.float64) ** 2 / (W * H)   # k = 0 is the spin overlap squared, whatever the axis
    assert np.allclose(chi[:, 0, 0], spin2, rtol=1e-12, atol=0.0) and np.allclose(chi[:, 1, 0], spin2, rtol=1e-12, atol=0.0)


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(capi, exact):
    W, H = 256, 4   # (a field stays on the checkerboard path from 256 columns on)
    N = W * H
    ea, eb, ej = exact.square_lattice_edges(W, H, -1.0)
    seeds = capi.make_seeds(3, 6)
    one = np.zeros(1, dtype=np.uint32)
    cubic = exact.cubic_lattice_edges(6)
    cases = {
        "f64 CSR": (capi.Graph(*cubic, 216), np.zeros(216, dtype=np.uint32)),   # a small graph without the force flag
        "field": (capi.Graph(ea, eb, ej, N, biases=np.full(N, 0.5)), np.zeros(N, dtype=np.uint32)),
    }
    for reason, (graph, table) in cases.items():
        cs = capi.SiteClasses(graph, table)          # the tables alone are fine: the containers are refused
        assert cs.sizes.tolist() == [[graph.nvars]]
        st = capi.States(graph, seeds[:2])
        for args in ((), (None, one, one + 1), (capi.States(graph, seeds[:2]),)):
            with pytest.raises(ValueError, match=reason):
                st.overlaps_by_class(cs, *args)
        st.do_time_steps(2, 0.4)   # still usable
        assert st.timestep == 2
    assert capi.States(cases["f64 CSR"][0], seeds[:2]).family == "csr_f64"
    g = capi.Graph(ea, eb, ej)
    st = capi.States(g, seeds)
    table = np.arange(N, dtype=np.uint32) % 7
    cs = capi.SiteClasses(g, table)
    assert cs.n_tables == 1 and cs.n_classes == 7
    with pytest.raises(ValueError, match="another graph handle"):
        capi.States(capi.Graph(ea, eb, ej), seeds).overlaps_by_class(cs)
    with pytest.raises(ValueError, match="class value out of range"):
        capi.SiteClasses(g, table, 6)
    for tables, n_classes, message in ((np.zeros((0, N), dtype=np.uint32), 1, r"n_tables must be 1 \.\. 8"),
                                       (np.zeros((9, N), dtype=np.uint32), 1, r"n_tables must be 1 \.\. 8"),
                                       (table, 0, r"n_classes must be 1 \.\. 4096"), (table, 4097, r"n_classes must be 1 \.\. 4096"),
                                       (np.zeros((3, N), dtype=np.uint32), 4096, "must not exceed 8192")):
        with pytest.raises(ValueError, match=message):
            capi.SiteClasses(g, tables, n_classes)
    capi.SiteClasses(g, np.zeros((2, N), dtype=np.uint32), 4096)   # 2 x 4096 is the limit itself
    with pytest.raises(ValueError, match="both slot tables or neither"):
        st.overlaps_by_class(cs, None, [0, 1], None)
    with pytest.raises(ValueError, match="out of range"):
        st.overlaps_by_class(cs, None, [0, 6], [1, 2])          # a slot equal to count
    with pytest.raises(ValueError, match="out of range"):
        st.overlaps_by_class(cs, capi.States(g, capi.make_seeds(4, 3)), [0, 1], [1, 3])
    with pytest.raises(ValueError, match="odd experiment index"):
        capi.States(g, seeds, replica_range=(1, 5)).overlaps_by_class(cs)
    with pytest.raises(ValueError, match="n_pairs is 0"):
        capi.States(g, seeds[:1]).overlaps_by_class(cs)
    lib = capi.lib()
    out = np.zeros((3, 1, 7), dtype=np.int64)
    assert lib.isingmc_overlaps_by_class(st._h, None, None, None, 3, None, out.ctypes.data) == capi.ERR_INVALID and "NULL" in capi.last_error()
    assert lib.isingmc_overlaps_by_class(st._h, None, None, None, 3, cs._h, None) == capi.ERR_INVALID and "NULL" in capi.last_error()
    assert np.array_equal(st.overlaps_by_class(cs).sum(-1)[:, 0], st.overlaps(link=False)[0])   # and the container still measures

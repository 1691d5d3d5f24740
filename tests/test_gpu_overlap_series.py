"""The overlap series on the device: every row against the synchronising calls isingmc_overlaps and
isingmc_overlaps_by_class at the same timesteps of a twin with equal seeds -- integer equality everywhere.  The checkerboard path
(64 x 4 and 192 x 344 +-J lattices), the bit-sliced family (6^3 +-J cube) and the real-coupling family (6^3 Gaussian cube);
periodic records inside the step loop, explicit records with tables and between two containers, ladders by rung, purity,
bookkeeping and every refusal."""
import numpy as np
import pytest

import class_overlap_reference as CR
import overlap_series_reference as SR
import packed_icm_reference as IR
from pyisingmontecarlo_amd.correlation import plane_classes

pytestmark = pytest.mark.gpu

FAMILIES = ["lattice_64x4", "lattice_192x344", "bit_sliced", "real_coupling"]


def _graph(capi, exact, monkeypatch, name):
    """(graph, ea, eb, tables, family): the tables are the row and column (plane) classes of the shape."""
    if name.startswith("lattice"):
        W, H = (64, 4) if name == "lattice_64x4" else (192, 344)
        ea, eb, ej = exact.square_lattice_edges(W, H, -1.0, np.random.default_rng(5))
        g = capi.Graph(ea, eb, ej)
        assert g.kind == capi.KIND_LATTICE2D and g.info.fast_path == 0
        return g, ea, eb, plane_classes((H, W)), "checkerboard"
    if name == "bit_sliced":
        monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
        ea, eb, ej = IR.cubic_glass(exact, 6)
        return capi.Graph(ea, eb, ej, nvars=216, force_general=True), ea, eb, plane_classes((6, 6, 6)), "packed_bitsliced"
    ea, eb, _ = exact.cubic_lattice_edges(6, 1.0)
    g = capi.Graph(ea, eb, np.random.default_rng(31).normal(size=len(ea)), nvars=216, stable_path=True)
    return g, ea, eb, plane_classes((6, 6, 6)), "packed_real"


def _sync_row(st, classes, other=None, sa=None, sb=None, link=True):
    """One row through the synchronising calls: int64[P, entries]."""
    spin, lnk = st.overlaps(other, sa, sb, link=link)
    parts = [spin[:, None]] + ([lnk[:, None]] if link else [])
    if classes is not None:
        parts.append(st.overlaps_by_class(classes, other, sa, sb).reshape(len(spin), -1))
    return np.concatenate(parts, axis=1)


def _rows(series):
    """(timesteps, int64[n, P, entries]) of the whole log, put together again from what get() returns."""
    t, spin, lnk, by_class = series.get()
    parts = [spin[:, :, None]] + ([lnk[:, :, None]] if lnk is not None else [])
    if by_class is not None:
        parts.append(by_class.reshape(by_class.shape[0], by_class.shape[1], -1))
    return t, np.concatenate(parts, axis=2)


# ---- 1. rows against the synchronising calls, single container -----------------------------------------------------------------
@pytest.mark.parametrize("name", FAMILIES)
def test_periodic_rows_equal_the_synchronising_calls(capi, exact, monkeypatch, name):
    """A period of 3 over calls of 5, 1, 7 and 6 timesteps with an isoenergetic move every 4th (timestep 11 is a move and 12 a
    sample point): 37 replicas -- the last one unpaired, the second group partly used -- and the shard [20, 57) of 57 experiments (bit 20 of a word on)."""
    g, ea, eb, tables, family = _graph(capi, exact, monkeypatch, name)
    classes = capi.SiteClasses(g, tables)
    for seeds, rng_ in ((capi.make_seeds(600, 37), None), (capi.make_seeds(601, 57), (20, 57))):
        st, twin = capi.States(g, seeds, replica_range=rng_), capi.States(g, seeds, replica_range=rng_)
        assert st.family == family and st.count == 37
        for c in (st, twin):
            c.set_icm_every(4)
        series = st.overlap_series(classes=classes, capacity=16)
        assert series.n_pairs == 18 and series.capacity == 16 and series.count == 0
        series.set_every(3)
        want_t, want = [], []
        for n in (5, 1, 7, 6):
            st.do_time_steps(n, 0.5)
            for t in SR.sample_points(0, 3, twin.timestep, twin.timestep + n):
                twin.do_time_steps(t - twin.timestep, 0.5)
                want_t.append(t)
                want.append(_sync_row(twin, classes))
            twin.do_time_steps(st.timestep - twin.timestep, 0.5)
        assert want_t == [3, 6, 9, 12, 15, 18] and st.timestep == twin.timestep == 19
        got_t, got = _rows(series)
        assert series.count == 6 and got_t.dtype == np.uint64 and got_t.tolist() == want_t
        assert got.dtype == np.int64 and np.array_equal(got, np.stack(want))
        assert np.abs(got[:, :, 0]).max() < g.nvars            # no trivial pair: the comparison can see a wrong pairing
        # the numpy rule on the configurations as they are now: one explicit record without tables
        series.set_every(0)
        series.record()
        A = st.states()
        pa, pb = SR.OR.default_pairs(37)
        assert np.array_equal(_rows(series)[1][6], SR.row(A, A, ea, eb, pa, pb, True, tables, classes.n_classes))
        # purity: the twin carried no series
        assert np.array_equal(st.raw_state(), twin.raw_state()) and np.array_equal(st.energies(), twin.energies())
        series.close()


# ---- 2. tables and two containers, 3. by class ---------------------------------------------------------------------------------
def _tables(rng, n, count_a, count_b, same):
    """n pairs of slots: shuffled, a slot repeated, and inside one container the pair (r, r) first."""
    sa, sb = rng.integers(0, count_a, n), rng.integers(0, count_b, n)
    sa[2] = sa[1]
    if same:
        sa[0] = sb[0] = count_a - 1
    sa[n - 1], sb[n - 1] = 1, count_b - 1
    return sa.astype(np.uint32), sb.astype(np.uint32)


@pytest.mark.parametrize("name", ["lattice_64x4", "bit_sliced", "real_coupling"])
def test_explicit_records_with_tables_and_between_two_containers(capi, exact, monkeypatch, name):
    g, ea, eb, tables, family = _graph(capi, exact, monkeypatch, name)
    tables = tables.astype(np.int64)
    tables[0, 3] = tables[1, 7] = CR.NO_CLASS            # sites counted nowhere
    classes = capi.SiteClasses(g, tables, n_classes=int(tables[tables != CR.NO_CLASS].max()) + 3)   # the last two classes are empty
    assert (classes.sizes[:, -2:] == 0).all()
    a, b = capi.States(g, capi.make_seeds(11, 40)), capi.States(g, capi.make_seeds(12, 37))
    a.do_time_steps(3, 0.5)
    b.do_time_steps(2, 0.5)
    rng = np.random.default_rng(8)
    n = 70                                               # three pair blocks of a packed container
    # three records with three tables and nothing read in between (the expected rows come from twins with equal seeds): b goes on
    # at once behind every record, and the caller's tables are free again when record returns
    a2, b2 = capi.States(g, capi.make_seeds(11, 40)), capi.States(g, capi.make_seeds(12, 37))
    a2.do_time_steps(3, 0.5)
    b2.do_time_steps(2, 0.5)
    for other, other2 in ((None, None), (b, b2)):
        series = a.overlap_series(other, n_pairs=n, classes=classes, capacity=4)
        want, want_t = [], []
        for k in range(3):
            sa, sb = _tables(rng, n, 40, 37 if other is not None else 40, other is None)
            series.record(sa, sb)
            want_t.append(a.timestep)
            for c in (a, b):
                c.do_time_steps(1 + k, 0.5)
            want.append(_sync_row(a2, classes, other2, sa, sb))
            sa[:] = 0
            sb[:] = 0
            for c in (a2, b2):
                c.do_time_steps(1 + k, 0.5)
        got_t, got = _rows(series)
        assert got_t.tolist() == want_t and np.array_equal(got, np.stack(want))
        series.close()
    # with the synchronising calls between the records, with and without the link overlap, and in batches
    for other in (None, b):
        for link in (True, False):
            series = a.overlap_series(other, n_pairs=n, classes=classes, link=link, capacity=5)
            want, want_t = [], []
            for k in range(3):
                sa, sb = _tables(rng, n, 40, 37 if other is not None else 40, other is None)
                want.append(_sync_row(a, classes, other, sa, sb, link=link))
                want_t.append(a.timestep)
                series.record(sa, sb)
                for c in (a, b):
                    c.do_time_steps(1 + k, 0.5)
            got_t, got = _rows(series)
            assert got_t.tolist() == want_t and np.array_equal(got, np.stack(want))
            if other is None:                            # the pair (r, r): the sizes themselves
                assert (got[:, 0, 0] == g.nvars).all()
                if link:
                    assert (got[:, 0, 1] == len(ea)).all()
                assert np.array_equal(got[0, 0, 2 if link else 1:], classes.sizes.astype(np.int64).ravel())
            # cluster_workspace_bytes small enough for one item per batch: 70 batches of pairs on the lattice, 3 of pair blocks
            # on a packed container -- the same row as in one batch
            a.set_option("cluster_workspace_bytes", 1)
            series.record(sa, sb)
            a.set_option("cluster_workspace_bytes", 1 << 30)
            series.record(sa, sb)
            got = _rows(series)[1]
            assert np.array_equal(got[3], got[4]) and np.array_equal(got[4], _sync_row(a, classes, other, sa, sb, link=link))
            # ... and the numpy rule on the configurations as they are: the synchronising calls cut their batches by the plan
            # of the series, so that the comparison above would not see a plan that is wrong
            A, B = a.states(), (a if other is None else other).states()
            assert np.array_equal(got[3], SR.row(A, B, ea, eb, sa, sb, link, tables, classes.n_classes))
            series.close()
    # two containers without tables: (slot p, slot p)
    series = a.overlap_series(b, classes=classes, capacity=2)
    assert series.n_pairs == 37
    series.record()
    assert np.array_equal(_rows(series)[1][0], _sync_row(a, classes, b))
    A, B = a.states(), b.states()
    assert np.array_equal(_rows(series)[1][0], SR.row(A, B, ea, eb, np.arange(37), np.arange(37), True, tables, classes.n_classes))
    series.close()


# ---- 4. ladders, and 5. purity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["lattice", "lattice_host_swaps", "bit_sliced", "real_coupling"])
def test_ladder_rows_in_rung_order(capi, exact, monkeypatch, case):
    from pyisingmontecarlo_amd.tempering import ClassicalTempering

    if case.startswith("lattice"):
        ea, eb, ej = exact.square_lattice_edges(64, 4, -1.0, np.random.default_rng(9))
        betas, family, tables = np.linspace(0.3, 0.44, 8), "checkerboard", plane_classes((4, 64))
        if case == "lattice_host_swaps":
            monkeypatch.setenv("ISINGMC_PT_HOST", "1")
    else:
        monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
        monkeypatch.setenv("ISINGMC_FORCE_REAL", "1" if case == "real_coupling" else "0")
        ea, eb, _ = exact.cubic_lattice_edges(6, 1.0)
        rng = np.random.default_rng(77)
        ej = rng.normal(size=len(ea)) if case == "real_coupling" else rng.choice([-1.0, 1.0], len(ea))
        betas, family, tables = np.linspace(0.4, 0.61, 8), "packed_real" if case == "real_coupling" else "packed_bitsliced", plane_classes((6, 6, 6))

    def ladder():
        pt = ClassicalTempering((ea, eb, ej), seed=4711, copies=2)
        for beta in betas:
            pt.add_graph(float(beta))
        pt.set_replica_cluster_update_every(4)
        return pt

    pt, twin, plain = ladder(), ladder(), ladder()
    pt.set_measure_overlaps_every(3, classes=tables)
    pt.timesteps(24, 2)
    plain.timesteps(24, 2)
    assert pt._on_stream == (case != "lattice_host_swaps") and pt._pair[0]._states.family == family
    assert pt._ovl_series.by_rung == pt._on_stream
    # the twin, one timestep at a time: the timestep, then the sample, then the exchange round
    twin_classes = twin.site_classes(tables)
    want, left_identity = [], False
    for t in range(1, 25):
        twin.timesteps(1, 0)
        if t % 3 == 0:
            left_identity = left_identity or not np.array_equal(twin.get_permutation()[0], np.arange(8))
            spin, lnk = twin.get_overlaps()
            want.append(np.concatenate([spin[:, None], lnk[:, None], twin.get_overlaps_by_class(twin_classes).reshape(8, -1)], axis=1))
        if t % 2 == 0:
            for c in twin._pair:
                c._swap_step()
    assert left_identity, "the permutation was the identity at every sample: a wrong pairing would not show"
    ts, spin, lnk, by_class = pt.get_measured_overlaps()
    assert ts.tolist() == list(range(3, 25, 3)) and spin.shape == (8, 8) and by_class.shape == (8, 8, len(tables), twin_classes.n_classes)
    got = np.concatenate([spin[:, :, None], lnk[:, :, None], by_class.reshape(8, 8, -1)], axis=2)
    assert np.array_equal(got, np.stack(want))
    assert np.abs(spin).max() < pt.nvars
    # purity: the same run without a series, and the twin's piecewise run
    for other in (plain, twin):
        assert np.array_equal(pt.get_permutation(), other.get_permutation()) and pt.get_total_swaps() == other.get_total_swaps() > 0
        for c, d in zip(pt._pair, other._pair):
            assert np.array_equal(c._states.raw_state(), d._states.raw_state()) and c._states.timestep == d._states.timestep == 24
            assert np.array_equal(c._states.energies(), d._states.energies())
    # reset keeps the period; the next rows start at 0
    pt.reset_measured_overlaps()
    pt.timesteps(3, 2)
    ts, spin, _, _ = pt.get_measured_overlaps()
    assert ts.tolist() == [27] and np.array_equal(spin[0], pt.get_overlaps(link=False)[0])
    pt.set_measure_overlaps_every(0)
    pt.timesteps(3, 2)
    assert pt.get_measured_overlaps()[0].tolist() == [27]


def test_a_series_changes_nothing_in_one_container(capi, exact, monkeypatch):
    for name in ("lattice_64x4", "bit_sliced", "real_coupling"):
        g, ea, eb, tables, _ = _graph(capi, exact, monkeypatch, name)
        seeds = capi.make_seeds(500, 35)
        st, plain, other = capi.States(g, seeds), capi.States(g, seeds), capi.States(g, capi.make_seeds(501, 35))
        classes = capi.SiteClasses(g, tables)
        periodic, between = st.overlap_series(classes=classes, capacity=8), st.overlap_series(other, capacity=8)
        periodic.set_every(2)
        other.do_time_steps(2, 0.5)
        for n in (3, 4):
            st.do_time_steps(n, 0.5)
            plain.do_time_steps(n, 0.5)
            between.record()
        assert periodic.count == 3 and between.count == 2
        before = [st.raw_state(), st.timestep, st.energies(), other.raw_state(), other.timestep]
        periodic.get()
        between.get()
        after = [st.raw_state(), st.timestep, st.energies(), other.raw_state(), other.timestep]
        for x, y in zip(before, after):
            assert np.array_equal(x, y)
        assert np.array_equal(st.raw_state(), plain.raw_state()) and st.timestep == plain.timestep == 7
        assert np.array_equal(st.energies(), plain.energies())


# ---- 6. bookkeeping --------------------------------------------------------------------------------------------------------------
def test_bookkeeping(capi, exact, monkeypatch):
    g, ea, eb, tables, _ = _graph(capi, exact, monkeypatch, "lattice_64x4")
    st = capi.States(g, capi.make_seeds(700, 6))
    series = st.overlap_series(capacity=4)
    series.set_every(2)
    st.do_time_steps(8, 0.5)                              # rows at 2, 4, 6, 8: exactly the capacity
    assert series.count == series.capacity == 4
    full = series.get()
    assert full[0].tolist() == [2, 4, 6, 8] and np.array_equal(full[1][3], st.overlaps()[0]) and full[3] is None
    with pytest.raises(ValueError, match="full"):
        series.record()
    with pytest.raises(ValueError, match="run full"):
        st.do_time_steps(2, 0.5)                          # would take a sample: refused before anything moves
    with pytest.raises(ValueError, match="run full"):
        st.run_sampling_moments(0.5, 1, 1, 1)
    assert st.timestep == 8 and series.count == 4
    again = series.get()
    for x, y in zip(full[:3], again[:3]):
        assert np.array_equal(x, y)
    st.do_time_steps(1, 0.5)                              # no sample point in it: served
    assert st.timestep == 9
    window = series.get(1, 2)
    assert window[0].tolist() == [4, 6] and np.array_equal(window[1], full[1][1:3]) and np.array_equal(window[2], full[2][1:3])
    assert series.get(4)[0].size == 0 and series.get(3)[0].tolist() == [8]
    with pytest.raises(ValueError, match="out of range"):
        series.get(3, 2)
    series.reset()
    assert series.count == 0
    st.do_time_steps(1, 0.5)                              # the period stays: timestep 10 is a sample point, now row 0
    t, spin, lnk, _ = series.get()
    assert t.tolist() == [10] and np.array_equal(spin[0], st.overlaps()[0]) and np.array_equal(lnk[0], st.overlaps()[1])
    st.timestep = 101                                     # the sample points are counted from here
    st.do_time_steps(4, 0.5)
    assert series.get()[0].tolist() == [10, 103, 105]
    series.set_every(0)                                   # off: the rows stay, no more come
    st.do_time_steps(4, 0.5)
    assert series.count == 3 and series.get()[0].tolist() == [10, 103, 105]
    # the sampling run with device sums takes its rows too: 2 + 5 x 2 timesteps from 0, a row every 3rd, the last at the end
    fresh = capi.States(g, capi.make_seeds(701, 6))
    log = fresh.overlap_series(link=False, capacity=4)
    log.set_every(3)
    fresh.run_sampling_moments(0.5, 2, 2, 5)
    t, spin, lnk, _ = log.get()
    assert t.tolist() == [3, 6, 9, 12] and lnk is None and np.array_equal(spin[3], fresh.overlaps(link=False)[0])


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(capi, exact, monkeypatch):
    from pyisingmontecarlo_amd import tempering as T

    W, H = 256, 4   # (a field stays on the checkerboard path from 256 columns on)
    N = W * H
    ea, eb, ej = exact.square_lattice_edges(W, H, -1.0)
    seeds = capi.make_seeds(3, 6)
    for reason, g in {"f64 CSR": capi.Graph(*exact.cubic_lattice_edges(6), 216),
                      "field": capi.Graph(ea, eb, ej, N, biases=np.full(N, 0.5))}.items():
        st = capi.States(g, seeds[:2])
        for other in (None, capi.States(g, seeds[:2])):
            with pytest.raises(ValueError, match=reason):
                st.overlap_series(other)
    g = capi.Graph(ea, eb, ej)
    st, st2 = capi.States(g, seeds), capi.States(g, seeds)
    with pytest.raises(ValueError, match="different graph handles"):
        st.overlap_series(capi.States(capi.Graph(ea, eb, ej), seeds))
    with pytest.raises(ValueError, match="n_pairs is 0"):
        capi.States(g, seeds[:1]).overlap_series()
    with pytest.raises(ValueError, match="capacity is 0"):
        st.overlap_series(capacity=0)
    with pytest.raises(ValueError, match="attached tempering ladder"):
        st.overlap_series(st2, by_rung=True)
    with pytest.raises(ValueError, match="two different containers"):
        st.overlap_series(by_rung=True)
    between = st.overlap_series(st2)
    with pytest.raises(ValueError, match="inside one container"):
        between.set_every(2)
    with pytest.raises(ValueError, match="out of range"):
        between.record(np.full(6, 6, dtype=np.uint32), np.zeros(6, dtype=np.uint32))
    with pytest.raises(ValueError, match="both slot tables or neither"):
        between.record(np.zeros(6, dtype=np.uint32), None)
    assert between.count == 0
    with pytest.raises(ValueError, match="count / 2"):
        st.overlap_series(n_pairs=2).record()             # tables may follow, so creation serves it; a record without tables does not
    first, second = st.overlap_series(), st.overlap_series()
    first.set_every(2)
    with pytest.raises(ValueError, match="one periodic series per container"):
        second.set_every(2)
    with pytest.raises(ValueError, match="overlap series records on a period"):
        st.append(int(seeds[0]))
    first.set_every(0)
    second.set_every(2)                                   # the period is free again
    second.set_every(0)
    st.append(int(seeds[0]))
    st.set_option("overlap_series_bytes", 3 * 8 * 100)
    assert st.overlap_series(link=False, capacity=100).capacity == 100
    with pytest.raises(ValueError, match="overlap_series_bytes"):
        st.overlap_series(link=False, capacity=101)
    with pytest.raises(ValueError, match="overlap_series_bytes"):
        st.overlap_series(link=True, capacity=100)
    # ladders: one engine (one graph handle), three ladders, the third over other betas
    eng = T.HipEngine(ea, eb, ej, N)
    ladders = []
    for betas in ([0.3, 0.35, 0.4, 0.45], [0.3, 0.35, 0.4, 0.45], [0.3, 0.35, 0.4, 0.46]):
        pt = T.ClassicalTempering((ea, eb, ej), seed=9, engine_factory=lambda: eng)
        for beta in betas:
            pt.add_graph(beta)
        pt._materialise()
        assert pt._on_stream
        ladders.append(pt._states)
    with pytest.raises(ValueError, match="differ in their betas"):
        ladders[0].overlap_series(ladders[2], by_rung=True)
    with pytest.raises(ValueError, match="number of rungs"):
        ladders[0].overlap_series(ladders[1], n_pairs=3, by_rung=True)
    by_rung = ladders[0].overlap_series(ladders[1], by_rung=True)
    with pytest.raises(ValueError, match="takes no slot tables"):
        by_rung.record(np.arange(4, dtype=np.uint32), np.arange(4, dtype=np.uint32))
    with pytest.raises(ValueError, match="inside one container"):
        by_rung.set_every(2)
    for s in ladders[:2]:
        with pytest.raises(ValueError, match="ISINGMC_SERIES_BY_RUNG"):
            s.pt_detach()
    by_rung.record()
    assert np.array_equal(by_rung.get()[1][0], ladders[0].overlaps(ladders[1], ladders[0].pt_state()[0], ladders[1].pt_state()[0])[0])
    by_rung.close()
    ladders[1].pt_detach()                                # nothing reads the permutation any more


# ---- 8. ClassicIsing -------------------------------------------------------------------------------------------------------------
def test_classic_ising_round_trip(exact):
    import py_monte_carlo

    ea, eb, ej = exact.square_lattice_edges(64, 4, -1.0, np.random.default_rng(3))
    edges = [((int(a), int(b)), float(j)) for a, b, j in zip(ea, eb, ej)]
    ci, twin = (py_monte_carlo.ClassicIsing(edges, None, 7, 21) for _ in range(2))
    with pytest.raises(ValueError, match="set_measure_overlaps_every"):
        ci.get_measured_overlaps()
    tables = plane_classes((4, 64))
    ci.set_measure_overlaps_every(2, classes=tables, capacity=8)
    with pytest.raises(ValueError, match="overlap series records on a period"):
        ci.add_graph()
    ci.run_monte_carlo(0.5, 3)
    ci.run_monte_carlo(0.5, 3)
    want = []
    for _ in range(3):
        twin.run_monte_carlo(0.5, 2)
        spin, lnk = twin.get_overlaps()
        want.append((spin, lnk, twin.get_overlaps_by_class(tables)))
    t, spin, lnk, by_class = ci.get_measured_overlaps()
    assert t.dtype == np.uint64 and t.tolist() == [2, 4, 6] and spin.dtype == np.int64 and by_class.shape == (3, 3, 2, 64)
    for k in range(3):
        assert np.array_equal(spin[k], want[k][0]) and np.array_equal(lnk[k], want[k][1]) and np.array_equal(by_class[k], want[k][2])
    assert np.array_equal(np.array(ci.get_states()), np.array(twin.get_states()))
    ci.reset_measured_overlaps()
    assert ci.get_measured_overlaps()[0].size == 0
    ci.set_measure_overlaps_every(0)
    ci.run_monte_carlo(0.5, 2)
    assert ci.get_measured_overlaps()[0].size == 0
    ci.set_measure_overlaps_every(1, link=False)           # a new log: no link overlaps, no classes
    ci.run_monte_carlo(0.5, 2)
    t, spin, lnk, by_class = ci.get_measured_overlaps()
    assert t.tolist() == [9, 10] and lnk is None and by_class is None and np.array_equal(spin[1], ci.get_overlaps(link=False)[0])

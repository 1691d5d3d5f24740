"""The observable series on the device: every row against a twin container with equal seeds, driven to the same
timesteps and read with the synchronising calls -- energies() on the float64 bits, magnetisations(), and the class sums of
tests/observable_series_reference.py from states().  The checkerboard path (64 x 4 and 192 x 344 +-J lattices), the bit-sliced
family (6^3 +-J cube) and the real-coupling family (6^3 Gaussian cube); periodic and explicit records, ladders by rung, purity,
bookkeeping, every refusal, the shim, and Kaufman's exact energy."""
import ctypes
import json
import os

import numpy as np
import pytest

import observable_series_reference as XR
import packed_icm_reference as IR
from ladder_icm_engine import ladder_seeds
from pyisingmontecarlo_amd.correlation import plane_classes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ["lattice_64x4", "lattice_192x344", "bit_sliced", "real_coupling"]


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _graph(capi, exact, monkeypatch, name):
    """(graph, tables, family): the tables are the row and column (plane) classes of the shape."""
    if name.startswith("lattice"):
        W, H = (64, 4) if name == "lattice_64x4" else (192, 344)
        ea, eb, ej = exact.square_lattice_edges(W, H, -1.0, np.random.default_rng(5))
        g = capi.Graph(ea, eb, ej)
        assert g.kind == capi.KIND_LATTICE2D and g.info.fast_path == 0
        return g, plane_classes((H, W)), "checkerboard"
    if name == "bit_sliced":
        monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
        ea, eb, ej = IR.cubic_glass(exact, 6)
        return capi.Graph(ea, eb, ej, nvars=216, force_general=True), plane_classes((6, 6, 6)), "packed_bitsliced"
    ea, eb, _ = exact.cubic_lattice_edges(6, 1.0)
    g = capi.Graph(ea, eb, np.random.default_rng(31).normal(size=len(ea)), nvars=216, stable_path=True)
    return g, plane_classes((6, 6, 6)), "packed_real"


def _holes(tables):
    """One more table: the first one with two sites counted nowhere; the set gets two empty classes behind the largest."""
    tables = tables.astype(np.int64)
    holes = tables[0].copy()
    holes[[3, 7]] = XR.NO_CLASS
    return np.concatenate([tables, holes[None]]), int(tables.max()) + 3


def _sync_row(st, tables, n_classes):
    """(energy bits, magnetisation, class sums) of the configurations as they are, through the synchronising calls."""
    return _bits(st.energies()), st.magnetisations(), XR.class_sums(st.states(), tables, n_classes)


def _assert_rows(series, want_t, want):
    t, e, m, c = series.get()
    assert t.dtype == np.uint64 and t.tolist() == want_t
    assert e.dtype == np.float64 and np.array_equal(_bits(e), np.stack([w[0] for w in want]))
    assert m.dtype == np.int64 and np.array_equal(m, np.stack([w[1] for w in want]))
    assert c.dtype == np.int64 and np.array_equal(c, np.stack([w[2] for w in want]))
    return e, m, c


# ---- 1. periodic rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FAMILIES)
def test_periodic_rows_equal_the_synchronising_calls(capi, exact, monkeypatch, name):
    """A period of 3 over calls of 5, 1, 7 and 6 timesteps with an isoenergetic move every 4th (timestep 11 is a move and 12 a
    sample point): 37 replicas -- the second group partly used -- and the shard [20, 57) of 57 experiments (bit 20 of a word on)."""
    g, tables, family = _graph(capi, exact, monkeypatch, name)
    tables, n_classes = _holes(tables)
    classes = capi.SiteClasses(g, tables, n_classes=n_classes)
    assert (classes.sizes[:, -2:] == 0).all()
    for seeds, rng_ in ((capi.make_seeds(600, 37), None), (capi.make_seeds(601, 57), (20, 57))):
        st, twin = capi.States(g, seeds, replica_range=rng_), capi.States(g, seeds, replica_range=rng_)
        assert st.family == family and st.count == 37
        for c in (st, twin):
            c.set_icm_every(4)
        series = st.observable_series(classes=classes, capacity=16)
        assert series.n_columns == 37 and series.capacity == 16 and series.count == 0
        series.set_every(3)
        want_t, want = [], []
        for n in (5, 1, 7, 6):
            st.do_time_steps(n, 0.5)
            for t in XR.sample_points(0, 3, twin.timestep, twin.timestep + n):
                twin.do_time_steps(t - twin.timestep, 0.5)
                want_t.append(t)
                want.append(_sync_row(twin, tables, n_classes))
            twin.do_time_steps(st.timestep - twin.timestep, 0.5)
        assert want_t == [3, 6, 9, 12, 15, 18] and st.timestep == twin.timestep == 19
        e, m, c = _assert_rows(series, want_t, want)
        assert series.count == 6 and np.abs(m).max() < g.nvars and len(set(m[0].tolist())) > 4   # no trivial column
        # the rule itself: tables without NO_CLASS add up to the magnetisation, the holes are missing from the third, empty classes give 0
        assert np.array_equal(c[:, :, :-1].sum(axis=3), np.repeat(m[:, :, None], len(tables) - 1, axis=2))
        assert (c[:, :, :, -2:] == 0).all() and not np.array_equal(c[:, :, -1].sum(axis=2), m)
        # purity: the twin carried no series
        assert np.array_equal(st.raw_state(), twin.raw_state()) and np.array_equal(_bits(st.energies()), _bits(twin.energies()))
        series.close()


def test_periodic_rows_with_swendsen_wang_steps(capi, exact):
    """A ferromagnetic 64 x 4 lattice with a cluster step every 2nd timestep: rows behind Metropolis sweeps and behind cluster steps."""
    ea, eb, ej = exact.square_lattice_edges(64, 4, -1.0)
    g = capi.Graph(ea, eb, ej)
    tables = plane_classes((4, 64))
    classes = capi.SiteClasses(g, tables)
    seeds = capi.make_seeds(610, 37)
    st, twin = capi.States(g, seeds), capi.States(g, seeds)
    for c in (st, twin):
        c.set_cluster_every(2)
    series = st.observable_series(classes=classes, capacity=8)
    series.set_every(3)
    want_t, want = [], []
    for n in (5, 1, 7, 6):
        st.do_time_steps(n, 0.4)
        for t in XR.sample_points(0, 3, twin.timestep, twin.timestep + n):
            twin.do_time_steps(t - twin.timestep, 0.4)
            want_t.append(t)
            want.append(_sync_row(twin, tables, classes.n_classes))
        twin.do_time_steps(st.timestep - twin.timestep, 0.4)
    assert want_t == [3, 6, 9, 12, 15, 18]            # the rows at 6, 12 and 18 follow cluster steps (timestep t - 1 = 5, 11, 17 is one)
    _assert_rows(series, want_t, want)
    assert np.array_equal(st.raw_state(), twin.raw_state())


# ---- 2. explicit records -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lattice_64x4", "bit_sliced", "real_coupling"])
def test_explicit_records_and_partial_series(capi, exact, monkeypatch, name):
    g, tables, _ = _graph(capi, exact, monkeypatch, name)
    tables, n_classes = _holes(tables)
    classes = capi.SiteClasses(g, tables, n_classes=n_classes)
    seeds = capi.make_seeds(620, 35)
    st, twin = capi.States(g, seeds), capi.States(g, seeds)
    full = st.observable_series(classes=classes, capacity=8)
    e_only = st.observable_series(magnetisation=False, capacity=8)
    m_only = st.observable_series(energy=False, capacity=8)
    c_only = st.observable_series(classes=classes, energy=False, magnetisation=False, capacity=8)
    full.set_every(2)                                     # explicit records come between the periodic ones, whatever the period
    want_t, want = [], []
    for n in (1, 2, 3):
        st.do_time_steps(n, 0.5)
        for s in (full, e_only, m_only, c_only):
            s.record()
        for t in XR.sample_points(0, 2, twin.timestep, twin.timestep + n):
            twin.do_time_steps(t - twin.timestep, 0.5)
            want_t.append(t)
            want.append(_sync_row(twin, tables, n_classes))
        twin.do_time_steps(st.timestep - twin.timestep, 0.5)
        want_t.append(twin.timestep)                      # (a record at a sample point gives the row twice: timestep 6)
        want.append(_sync_row(twin, tables, n_classes))
    assert want_t == [1, 2, 3, 4, 6, 6]
    _assert_rows(full, want_t, want)
    explicit = [w for t, w, first in zip(want_t, want, [True, False, True, False, False, True]) if first]
    t, e, m, c = e_only.get()
    assert t.tolist() == [1, 3, 6] and m is None and c is None and np.array_equal(_bits(e), np.stack([w[0] for w in explicit]))
    t, e, m, c = m_only.get()
    assert e is None and c is None and np.array_equal(m, np.stack([w[1] for w in explicit]))
    t, e, m, c = c_only.get()
    assert e is None and m is None and np.array_equal(c, np.stack([w[2] for w in explicit]))
    # cluster_workspace_bytes small enough for one item per batch of the class counters: the same row as in one batch
    st.set_option("cluster_workspace_bytes", 1)
    c_only.record()
    st.set_option("cluster_workspace_bytes", 1 << 30)
    c_only.record()
    c = c_only.get()[3]
    assert np.array_equal(c[3], c[4]) and np.array_equal(c[4], want[-1][2])
    assert np.array_equal(st.raw_state(), twin.raw_state())


# ---- 3. ladders by rung --------------------------------------------------------------------------------------------------------
def _ladder(capi, g, betas, seed):
    st = capi.States(g, np.array(ladder_seeds(capi, seed, len(betas))[0][0], dtype=np.uint64))
    st.pt_attach(betas, 0, len(betas), 1, seed)
    return st


def _drive_twin(twin, rows, T, f, every, tables, n_classes):
    """pt_run(T, f) in pieces: a row after every timestep t with t % every == 0, between the timestep and that timestep's round."""
    done, rounds = 0, (T // f) * f
    while done < T:
        m = min(T - done, every - twin.timestep % every)
        if done < rounds:
            m = min(m, f - done % f)
        twin.pt_time_steps(m)
        done += m
        if twin.timestep % every == 0:
            perm = twin.pt_state()[0]
            e, mag, cls = _sync_row(twin, tables, n_classes)
            rows.append((twin.timestep, perm.copy(), (e[perm], mag[perm], cls[perm])))
        if done <= rounds and done % f == 0:
            twin.pt_measure()
            twin.pt_swap()


@pytest.mark.parametrize("case", ["lattice", "bit_sliced", "real_coupling"])
def test_ladder_rows_in_rung_order(capi, exact, monkeypatch, case):
    if case == "lattice":
        ea, eb, ej = exact.square_lattice_edges(128, 6, -1.0, np.random.default_rng(5))
        g, betas, tables, calls = capi.Graph(ea, eb, ej), 0.40 + 0.02 * np.arange(5), plane_classes((6, 128)), [(13, 3), (4, 3)]
    elif case == "bit_sliced":
        monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
        ea, eb, ej = IR.cubic_glass(exact, 6)
        g = capi.Graph(ea, eb, ej, nvars=216, force_general=True)
        betas, tables, calls = 0.30 + 0.005 * np.arange(40), plane_classes((6, 6, 6)), [(12, 1), (3, 2)]
    else:
        monkeypatch.setenv("ISINGMC_FORCE_REAL", "1")
        ea, eb, _ = exact.square_lattice_edges(12, 12, -1.0)
        rng = np.random.default_rng(2024)
        g = capi.Graph(ea, eb, rng.normal(size=len(ea)), nvars=144, biases=rng.normal(size=144), force_general=True)
        betas, tables, calls = 0.30 + 0.005 * np.arange(33), plane_classes((12, 12)), [(12, 1), (3, 2)]
    classes = capi.SiteClasses(g, tables)
    st, twin, plain = (_ladder(capi, g, betas, 71) for _ in range(3))
    for c in (st, twin, plain):
        c.pt_set_statistics(True)
    series = st.observable_series(classes=classes, by_rung=True, capacity=16)
    series.set_every(2)
    rows = []
    for T, f in calls:
        st.pt_run(T, f)
        plain.pt_run(T, f)
        _drive_twin(twin, rows, T, f, 2, tables, classes.n_classes)
    assert len(rows) == sum(T for T, _ in calls) // 2
    assert any(not np.array_equal(p, np.arange(len(betas))) for _, p, _ in rows), "the identity at every sample: a wrong routing would not show"
    _assert_rows(series, [t for t, _, _ in rows], [w for _, _, w in rows])
    # purity: the same run without a series (its rounds inside persistent launches where they fit), and the twin in pieces
    for other in (plain, twin):
        assert st.timestep == other.timestep and np.array_equal(st.raw_state(), other.raw_state())
        assert np.array_equal(_bits(st.energies()), _bits(other.energies()))
        pa, pb = st.pt_state(), other.pt_state()
        assert np.array_equal(pa[0], pb[0]) and pa[1:] == pb[1:] and pa[2] > 0
        sa, sb = st.pt_statistics(), other.pt_statistics()
        for k in sa:
            if k != "in_kernel_rounds":                   # (which path the rounds took: the series keeps them at kernel boundaries)
                assert np.array_equal(sa[k], sb[k]), k
    with pytest.raises(ValueError, match="ISINGMC_OBS_BY_RUNG"):
        st.pt_detach()
    # without the flag an attached ladder is allowed: the columns are slots
    slots = st.observable_series(capacity=1)
    slots.record()
    assert np.array_equal(_bits(slots.get()[1][0]), _bits(st.energies())) and np.array_equal(slots.get()[2][0], st.magnetisations())
    series.close()
    st.pt_detach()


def test_tempering_two_copies_with_moves_between_them(capi, exact):
    from pyisingmontecarlo_amd.tempering import ClassicalTempering

    ea, eb, ej = exact.square_lattice_edges(64, 4, -1.0, np.random.default_rng(9))
    betas, tables = np.linspace(0.3, 0.44, 8), plane_classes((4, 64))

    def ladder():
        pt = ClassicalTempering((ea, eb, ej), seed=4711, copies=2)
        for beta in betas:
            pt.add_graph(float(beta))
        pt.set_replica_cluster_update_every(4)
        return pt

    pt, twin, plain = ladder(), ladder(), ladder()
    with pytest.raises(ValueError, match="set_measure_observables_every"):
        pt.get_measured_observables()
    pt.set_measure_observables_every(3, classes=tables)
    pt.timesteps(12, 2)                                   # (the moves are timesteps 3, 7 and 11: the row at 12 is taken behind one)
    plain.timesteps(12, 2)
    assert pt._on_stream
    want = []
    for t in range(1, 13):                                # the twin, one timestep at a time: timestep, sample, exchange round
        twin.timesteps(1, 0)
        if t % 3 == 0:
            per_copy = []
            for c, perm in zip(twin._pair, twin.get_permutation()):
                e, m, cls = _sync_row(c._states, tables, 64)
                per_copy.append((e[perm], m[perm], cls[perm]))
            want.append(per_copy)
        if t % 2 == 0:
            for c in twin._pair:
                c._swap_step()
    ts, e, m, cls = pt.get_measured_observables()
    assert ts.tolist() == [3, 6, 9, 12] and e.shape == (2, 4, 8) and m.shape == (2, 4, 8) and cls.shape == (2, 4, 8, 2, 64)
    for copy in range(2):
        assert np.array_equal(_bits(e[copy]), np.stack([w[copy][0] for w in want]))
        assert np.array_equal(m[copy], np.stack([w[copy][1] for w in want]))
        assert np.array_equal(cls[copy], np.stack([w[copy][2] for w in want]))
    for other in (plain, twin):
        assert np.array_equal(pt.get_permutation(), other.get_permutation()) and pt.get_total_swaps() == other.get_total_swaps() > 0
        for c, d in zip(pt._pair, other._pair):
            assert np.array_equal(c._states.raw_state(), d._states.raw_state()) and c._states.timestep == d._states.timestep == 12
    pt.reset_measured_observables()
    pt.timesteps(3, 2)
    assert pt.get_measured_observables()[0].tolist() == [15]
    pt.set_measure_observables_every(0)
    pt.timesteps(3, 2)
    assert pt.get_measured_observables()[0].tolist() == [15]


def test_tempering_one_copy_and_its_refusals(capi, exact):
    from pyisingmontecarlo_amd.tempering import ClassicalTempering

    ea, eb, ej = exact.square_lattice_edges(64, 4, -1.0, np.random.default_rng(9))
    single = ClassicalTempering((ea, eb, ej), seed=5)     # one copy: no leading axis
    for beta in np.linspace(0.3, 0.44, 8):
        single.add_graph(float(beta))
    single.set_measure_observables_every(2)
    single.timesteps(4, 3)                                # rows at 2 and 4, the one exchange round behind timestep 3
    ts, e, m, cls = single.get_measured_observables()
    assert ts.tolist() == [2, 4] and e.shape == (2, 8) and m.shape == (2, 8) and cls is None
    perm = single.get_permutation()
    assert np.array_equal(_bits(e[1]), _bits(single._states.energies()[perm])) and np.array_equal(m[1], single._states.magnetisations()[perm])
    sharded = ClassicalTempering((ea, eb, ej), seed=5, devices=[0, 0])
    with pytest.raises(ValueError, match="one device"):
        sharded.set_measure_observables_every(2)
    ranks = ClassicalTempering((ea, eb, ej), seed=5)
    ranks._world = 2                                      # (what a torch.distributed group of two ranks sets)
    with pytest.raises(ValueError, match="one process: not inside a torch.distributed group of several ranks"):
        ranks.set_measure_observables_every(2)


def test_a_full_log_refuses_a_ladder_call_before_anything_moves(capi, exact):
    """pt_run, isingmc_icm_between and ClassicalTempering.timesteps are several rounds, a move, several library calls: the rows of
    the WHOLE call are counted first, and a refused call leaves timestep, permutation, swap count and configurations as they were."""
    from pyisingmontecarlo_amd.tempering import ClassicalTempering

    ea, eb, ej = exact.square_lattice_edges(128, 6, -1.0, np.random.default_rng(5))
    g, betas = capi.Graph(ea, eb, ej), 0.40 + 0.02 * np.arange(5)
    st, other = _ladder(capi, g, betas, 71), _ladder(capi, g, betas, 72)
    series = st.observable_series(by_rung=True, capacity=3)
    series.set_every(2)
    st.pt_run(4, 2)                                       # rows at 2 and 4: room for one more
    other.pt_run(4, 2)
    start = (st.pt_state(), st.raw_state())
    with pytest.raises(ValueError, match="run full: the call takes 3 samples and the log has room for 1 of its 3"):
        st.pt_run(6, 2)                                   # its first round would fit: none is run
    assert st.timestep == 4 and np.array_equal(start[0][0], st.pt_state()[0]) and start[0][1:] == st.pt_state()[1:]
    assert np.array_equal(start[1], st.raw_state())
    st.pt_run(2, 2)                                       # the row at 6: the log is full
    assert series.count == 3
    before = (st.timestep, st.pt_state(), st.raw_state())
    with pytest.raises(ValueError, match="run full"):
        st.pt_run(2, 1)
    st.pt_time_steps(1)                                   # timestep 7: no sample point in it
    other.pt_time_steps(3)
    assert st.timestep == other.timestep == 7
    mid = (st.pt_state(), st.raw_state(), other.raw_state())
    for a, b in ((st, other), (other, st)):               # the move would be timestep 7 and the row at 8 behind it: refused before its launches
        with pytest.raises(ValueError, match="run full"):
            a.icm_between(b)
    assert st.timestep == other.timestep == 7 and series.count == 3
    now = (st.pt_state(), st.raw_state(), other.raw_state())
    assert np.array_equal(mid[0][0], now[0][0]) and mid[0][1:] == now[0][1:] and np.array_equal(mid[1], now[1]) and np.array_equal(mid[2], now[2])
    assert before[0] == 6 and np.array_equal(before[1][0], st.pt_state()[0]) and before[1][1:] == st.pt_state()[1:]
    series.reset()
    st.icm_between(other)                                 # with room again: the move, and the row behind it
    assert st.timestep == 8 and series.get()[0].tolist() == [8]
    # the Python ladder: both copies or neither
    pt = ClassicalTempering((exact.square_lattice_edges(64, 4, -1.0, np.random.default_rng(9))), seed=4711, copies=2)
    for beta in np.linspace(0.3, 0.44, 8):
        pt.add_graph(float(beta))
    pt.set_replica_cluster_update_every(4)
    pt.set_measure_observables_every(3, capacity=2)
    pt.timesteps(6, 2)
    state = [(c._states.timestep, c._states.raw_state()) for c in pt._pair]
    perm, swaps = pt.get_permutation(), pt.get_total_swaps()
    with pytest.raises(ValueError, match="would run full: the call takes 2 samples and the log has room for 0 of its 2"):
        pt.timesteps(8, 2)                                # (its first library calls hold no sample point)
    assert np.array_equal(pt.get_permutation(), perm) and pt.get_total_swaps() == swaps
    for c, (t, raw) in zip(pt._pair, state):
        assert c._states.timestep == t == 6 and np.array_equal(c._states.raw_state(), raw)
    pt.timesteps(2, 2)                                    # no sample point: served
    assert pt.get_measured_observables()[0].tolist() == [3, 6]


def test_tempering_refuses_the_host_swap_path(capi, exact, monkeypatch):
    from pyisingmontecarlo_amd.tempering import ClassicalTempering

    monkeypatch.setenv("ISINGMC_PT_HOST", "1")
    ea, eb, ej = exact.square_lattice_edges(64, 4, -1.0)
    pt = ClassicalTempering((ea, eb, ej), seed=1)
    for beta in (0.3, 0.4):
        pt.add_graph(beta)
    with pytest.raises(ValueError, match="host swap step"):
        pt.set_measure_observables_every(2)


# ---- 4. purity -----------------------------------------------------------------------------------------------------------------
def test_a_series_changes_nothing(capi, exact, monkeypatch):
    for name in ("lattice_64x4", "bit_sliced", "real_coupling"):
        g, tables, _ = _graph(capi, exact, monkeypatch, name)
        seeds = capi.make_seeds(500, 35)
        classes = capi.SiteClasses(g, tables)
        st, plain = capi.States(g, seeds), capi.States(g, seeds)
        series = st.observable_series(classes=classes, capacity=16)
        series.set_every(2)
        for n in (3, 4):
            st.do_time_steps(n, 0.5)
            plain.do_time_steps(n, 0.5)
            series.record()
        out = [c.run_sampling(0.5, 1, 2, 3) for c in (st, plain)]       # timesteps 8 .. 14: rows at 8, 10, 12, 14 inside the sampling run
        assert series.count == 9 and series.get()[0].tolist() == [2, 3, 4, 6, 7, 8, 10, 12, 14]
        for x, y in zip(*out):
            assert np.array_equal(x, y)
        before = [st.raw_state(), st.timestep, st.energies()]
        series.get()
        for x, y in zip(before, [st.raw_state(), st.timestep, st.energies()]):
            assert np.array_equal(x, y)
        assert np.array_equal(st.raw_state(), plain.raw_state()) and st.timestep == plain.timestep == 14
        assert np.array_equal(_bits(st.energies()), _bits(plain.energies()))


# ---- 5. bookkeeping ------------------------------------------------------------------------------------------------------------
def test_bookkeeping(capi, exact, monkeypatch):
    g, tables, _ = _graph(capi, exact, monkeypatch, "lattice_64x4")
    st = capi.States(g, capi.make_seeds(700, 6))
    series = st.observable_series(capacity=4)
    series.set_every(2)
    st.do_time_steps(8, 0.5)                              # rows at 2, 4, 6, 8: exactly the capacity
    assert series.count == series.capacity == 4
    full = series.get()
    assert full[0].tolist() == [2, 4, 6, 8] and np.array_equal(_bits(full[1][3]), _bits(st.energies())) and full[3] is None
    with pytest.raises(ValueError, match="full"):
        series.record()
    with pytest.raises(ValueError, match="run full"):
        st.do_time_steps(2, 0.5)                          # would take a sample: refused before anything moves
    with pytest.raises(ValueError, match="run full"):
        st.run_sampling_moments(0.5, 1, 1, 1)
    with pytest.raises(ValueError, match="run full"):
        st.run_sampling(0.5, 1, 1, 1)
    assert st.timestep == 8 and series.count == 4
    for x, y in zip(full[:3], series.get()[:3]):
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
    t, e, m, _ = series.get()
    assert t.tolist() == [10] and np.array_equal(_bits(e[0]), _bits(st.energies())) and np.array_equal(m[0], st.magnetisations())
    st.timestep = 101                                     # the sample points are counted from here
    st.do_time_steps(4, 0.5)
    assert series.get()[0].tolist() == [10, 103, 105]
    series.set_every(0)                                   # off: the rows stay, no more come
    st.do_time_steps(4, 0.5)
    assert series.count == 3 and series.get()[0].tolist() == [10, 103, 105]
    # one periodic series per container
    second = st.observable_series(capacity=2)
    series.set_every(2)
    with pytest.raises(ValueError, match="one periodic series per container"):
        second.set_every(2)
    with pytest.raises(ValueError, match="observable series records on a period"):
        st.append(int(capi.make_seeds(1, 1)[0]))
    with pytest.raises(ValueError, match="observable series records on a period"):
        st.pa_resample(0.1, 1, 0)
    with pytest.raises(ValueError, match="observable series records on a period"):
        st.pa_run([0.1, 0.2], 1, 1)
    assert st.timestep == 109 and st.count == 6
    series.set_every(0)
    second.set_every(2)                                   # the period is free again
    second.set_every(0)
    # the byte budget: 6 columns x (E + M) x 8 bytes a row
    st.set_option("observable_series_bytes", 6 * 2 * 8 * 100)
    assert st.observable_series(capacity=100).capacity == 100
    with pytest.raises(ValueError, match="observable_series_bytes"):
        st.observable_series(capacity=101)
    assert st.observable_series(energy=False, capacity=200).capacity == 200
    # asking for a part the series does not hold
    m_only = st.observable_series(energy=False, capacity=1)
    m_only.record()
    L = capi.lib()
    buf = np.zeros(6)
    assert L.isingmc_observable_series_get(m_only._h, 0, 1, None, buf.ctypes.data, None, None) == capi.ERR_INVALID
    assert b"no energies are held" in L.isingmc_last_error()
    ibuf = np.zeros(6, dtype=np.int64)
    assert L.isingmc_observable_series_get(m_only._h, 0, 1, None, None, None, ibuf.ctypes.data) == capi.ERR_INVALID
    assert b"by class" in L.isingmc_last_error()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(capi, exact):
    W, H = 256, 4   # (a field stays on the checkerboard path from 256 columns on)
    N = W * H
    ea, eb, ej = exact.square_lattice_edges(W, H, -1.0)
    seeds = capi.make_seeds(3, 6)
    x = np.arange(N) % W
    right = np.arange(len(ea)) % 2 == 0
    for reason, g in {"f64 CSR": capi.Graph(*exact.cubic_lattice_edges(6), 216),   # a small graph without the force flag
                      "field": capi.Graph(ea, eb, ej, N, biases=np.full(N, 0.5)),
                      "open": capi.Graph(*[a[~(right & (np.repeat(x, 2) == W - 1))] for a in (ea, eb, ej)], N),
                      "anisotropic": capi.Graph(ea, eb, np.where(right, -1.0, -2.0), N)}.items():
        st = capi.States(g, seeds[:2])
        with pytest.raises(ValueError, match=reason):
            st.observable_series()
        st.do_time_steps(2, 0.4)   # still usable
        assert st.timestep == 2
    g = capi.Graph(ea, eb, ej)
    st = capi.States(g, seeds)
    L = capi.lib()
    out = ctypes.c_void_p()
    assert L.isingmc_observable_series_create(st._h, None, 8 | 1, 4, ctypes.byref(out)) == capi.ERR_INVALID and not out
    assert b"unknown flag" in L.isingmc_last_error()
    with pytest.raises(ValueError, match="nothing to log"):
        st.observable_series(energy=False, magnetisation=False)
    with pytest.raises(ValueError, match="capacity is 0"):
        st.observable_series(capacity=0)
    other = capi.Graph(ea, eb, ej)
    with pytest.raises(ValueError, match="another graph handle"):
        st.observable_series(classes=capi.SiteClasses(other, plane_classes((H, W))))
    with pytest.raises(ValueError, match="needs a tempering ladder"):
        st.observable_series(by_rung=True)
    # a shard of a larger ladder
    shard = capi.States(g, seeds[:3])
    shard.pt_attach(np.linspace(0.3, 0.5, 6), 0, 3, 2, 9)
    with pytest.raises(ValueError, match="whole ladder on this container"):
        shard.observable_series(by_rung=True)
    assert shard.observable_series(capacity=1).n_columns == 3      # by slot: allowed
    assert st.timestep == 0 and st.count == 6


# ---- 7. the shim ---------------------------------------------------------------------------------------------------------------
def test_classic_ising_round_trip(exact):
    import py_monte_carlo

    ea, eb, ej = exact.square_lattice_edges(64, 4, -1.0, np.random.default_rng(3))
    edges = [((int(a), int(b)), float(j)) for a, b, j in zip(ea, eb, ej)]
    ci, twin = (py_monte_carlo.ClassicIsing(edges, None, 7, 21) for _ in range(2))
    with pytest.raises(ValueError, match="set_measure_observables_every"):
        ci.get_measured_observables()
    tables = plane_classes((4, 64))
    ci.set_measure_observables_every(2, classes=tables, capacity=8)
    with pytest.raises(ValueError, match="observable series records on a period"):
        ci.add_graph()
    ci.run_monte_carlo(0.5, 3)
    ci.run_monte_carlo(0.5, 3)
    want = []
    for _ in range(3):
        twin.run_monte_carlo(0.5, 2)
        A = np.array(twin.get_states())
        want.append((_bits(twin.get_energies()), XR.magnetisation(A), XR.class_sums(A, tables, 64)))
    t, e, m, by_class = ci.get_measured_observables()
    assert t.dtype == np.uint64 and t.tolist() == [2, 4, 6] and e.dtype == np.float64 and m.dtype == np.int64
    assert e.shape == m.shape == (3, 7) and by_class.shape == (3, 7, 2, 64)
    for k in range(3):
        assert np.array_equal(_bits(e[k]), want[k][0]) and np.array_equal(m[k], want[k][1]) and np.array_equal(by_class[k], want[k][2])
    assert np.array_equal(np.array(ci.get_states()), np.array(twin.get_states()))
    ci.reset_measured_observables()
    assert ci.get_measured_observables()[0].size == 0
    ci.set_measure_observables_every(0)
    ci.run_monte_carlo(0.5, 2)
    assert ci.get_measured_observables()[0].size == 0
    ci.set_measure_observables_every(1)                   # a new log, no classes
    ci.run_monte_carlo(0.5, 2)
    t, e, m, by_class = ci.get_measured_observables()
    assert t.tolist() == [9, 10] and by_class is None and np.array_equal(_bits(e[1]), _bits(ci.get_energies()))


def test_lattice_run_and_measure_observables(exact):
    import py_monte_carlo

    ea, eb, ej = exact.square_lattice_edges(64, 4, -1.0, np.random.default_rng(3))
    edges = [((int(a), int(b)), float(j)) for a, b, j in zip(ea, eb, ej)]
    tables = plane_classes((4, 64))
    for cluster in (0, 2):
        a, b = (py_monte_carlo.Lattice(edges, 17) for _ in range(2))
        for lat in (a, b):
            lat.set_replica_cluster_update_every(cluster)
        e, m, by_class = a.run_monte_carlo_and_measure_observables(0.5, 11, 6, thermalization_time=3, sampling_freq=2, classes=tables)
        e2, states = b.run_monte_carlo_sampling(0.5, 11, 6, thermalization_time=3, sampling_freq=2)
        assert e.shape == (6, 5) and m.shape == (6, 5) and m.dtype == np.int64 and by_class.shape == (6, 5, 2, 64)
        assert np.array_equal(_bits(e), _bits(e2))
        for r in range(6):
            assert np.array_equal(m[r], XR.magnetisation(states[r])) and np.array_equal(by_class[r], XR.class_sums(states[r], tables, 64))
    e, m = a.run_monte_carlo_and_measure_observables(0.5, 4, 3)
    assert e.shape == (3, 4) and m.shape == (3, 4)


# ---- 8. Kaufman ----------------------------------------------------------------------------------------------------------------
def test_kaufman_energy_from_the_series(capi, exact):
    """A 64 x 16 ferromagnetic torus at the critical beta of tests/golden/kaufman.json, 64 replicas, a Swendsen-Wang step every 2nd
    timestep: 2000 thermalising timesteps, then 2000 with a row every 10th.  The mean energy per site from the series against
    Kaufman's exact value, within 5 standard errors; the standard error from the spread of the per-replica means (the rule and
    margin of test_kaufman_energy_from_the_bond_sums).  Seeded: deterministic."""
    with open(os.path.join(ROOT, "tests", "golden", "kaufman.json")) as f:
        beta = [c["beta"] for c in json.load(f)["cases"] if c["W"] == 64][-1]
    assert beta == 0.4407
    W, H, R, every, T = 64, 16, 64, 10, 2000
    N = W * H
    ea, eb, ej = exact.square_lattice_edges(W, H, -1.0)
    st = capi.States(capi.Graph(ea, eb, ej), capi.make_seeds(41, R))
    st.set_cluster_every(2)
    st.do_time_steps(2000, beta)   # thermalised
    series = st.observable_series(capacity=T // every)
    series.set_every(every)
    st.do_time_steps(T, beta)
    t, e, m, _ = series.get()
    assert t.tolist() == list(range(2000 + every, 2000 + T + 1, every)) and e.shape == (T // every, R)
    means = e.mean(axis=0) / N                                          # per replica
    got, stderr = means.mean(), means.std(ddof=1) / np.sqrt(R)
    want = exact.kaufman_energy(W, H, beta) / N
    print(f"energy per site {got:.6f}, exact {want:.6f}, standard error {stderr:.6f}, z {(got - want) / stderr:+.2f}")
    assert np.array_equal(_bits(e[-1]), _bits(st.energies())) and np.array_equal(m[-1], st.magnetisations())
    assert abs(got - want) < 5 * stderr

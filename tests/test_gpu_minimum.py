"""Minimum tracking on the device against the twin rule: a container with the same seeds is stepped through the
existing calls, its energies and configurations are read after every update point, and tests/minimum_reference.py forms the
records from them.  Everything is compared exactly: energies bit for bit as f64, configurations, timesteps, the count."""
import numpy as np
import pytest

import minimum_reference as MR
import packed_icm_reference as IR

pytestmark = pytest.mark.gpu

# hot -> cold -> hot: the records are set mid-run
SCHEDULE = np.concatenate([np.linspace(0.1, 1.2, 12), np.linspace(1.2, 0.05, 12)])


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _slice(beta, k0, n):
    return beta if np.ndim(beta) == 0 else np.asarray(beta)[k0:k0 + n]


def _twin_records(twin, calls, every, rec=None, raws=None, by_hand=()):
    """Steps `twin` through calls = [(timesteps, beta)], cut at the update points t % every == 0 (every = 0: none), reads it there
    and after the calls whose index is in `by_hand`; returns (records, update timesteps)."""
    rec = rec or MR.Records(twin.count, twin.graph.nvars)
    points = []

    def read():
        rec.update(twin.timestep, twin.energies(), twin.states())
        points.append(twin.timestep)
        if raws is not None:
            raws.append(twin.raw_state())

    for i, (n, beta) in enumerate(calls):
        k = 0
        while k < n:
            m = n - k if not every else min(n - k, every - twin.timestep % every)
            twin.do_time_steps(m, _slice(beta, k, m))
            k += m
            if every and twin.timestep % every == 0:
                read()
        if i in by_hand:
            read()
    return rec, points


def _assert_equal(st, rec):
    e, s, t, n = st.best()
    assert np.array_equal(_bits(e), _bits(rec.energy))
    assert np.array_equal(s, rec.state)
    assert t.dtype == np.uint64 and np.array_equal(t, rec.timestep)
    assert n == rec.improvements


def _assert_same_container(a, b):
    assert a.timestep == b.timestep
    assert np.array_equal(_bits(a.energies()), _bits(b.energies()))
    assert np.array_equal(a.raw_state(), b.raw_state())


def _anneal_and_compare(capi, make, bit0=0):
    """The schedule with every = 1 on a tracked container, its twin and an untracked container run in one call; the conditions the
    schedule is chosen for are asserted on the reference's own output."""
    st, twin, plain = make(), make(), make()
    st.set_track_best(1)
    assert st.track_best == 1 and twin.track_best == 0
    T = len(SCHEDULE)
    st.do_time_steps(T, SCHEDULE)
    plain.do_time_steps(T, SCHEDULE)
    raws = []
    rec, points = _twin_records(twin, [(T, SCHEDULE)], 1, raws=raws)
    assert points == list(range(1, T + 1))
    mid = (rec.timestep != points[0]) & (rec.timestep != points[-1])
    assert 2 * int(mid.sum()) >= st.count, "the schedule sets too few records mid-run"
    assert rec.improved[0].all(), "the first update must improve every replica (the plain-copy branch)"
    _assert_equal(st, rec)
    _assert_same_container(st, twin)
    _assert_same_container(st, plain)
    if st.family != "checkerboard":
        groups = (bit0 + st.count + 31) // 32
        own = MR.owned_masks(st.count, bit0, groups)
        masks = np.array([MR.improved_masks(b, bit0, groups) for b in rec.improved])   # [update][group]
        assert np.array_equal(masks[0], own)
        assert (masks == 0).any(), "no update leaves a whole group unimproved (the m == 0 branch)"
        assert ((masks != 0) & (masks != own)).any(), "no update improves part of a group (the merge branch)"
        want = MR.merge_words(raws, rec.improved, bit0, groups)
        got = st.best_raw().reshape(groups, -1)
        assert np.array_equal(got & own[:, None], want & own[:, None])
    else:
        assert any(not b.all() for b in rec.improved[1:]), "every update improves every replica: no row is ever skipped"
        if st.count >= 32:   # (a few replicas of a large ferromagnet cool and heat together: only a population mixes)
            assert any(b.any() and not b.all() for b in rec.improved[1:]), "no update keeps some rows and skips others"
    return st, twin


# ---- shapes: the smallest at which each kernel can go wrong (those of tests/test_gpu_overlaps.py) ----------------------------
@pytest.mark.parametrize("glass", [False, True])
@pytest.mark.parametrize("W,H,R", [(64, 4, 40), (192, 344, 5)])
def test_checkerboard(capi, exact, W, H, R, glass):
    ea, eb, ej = exact.square_lattice_edges(W, H, -1.0, np.random.default_rng(5) if glass else None)
    g = capi.Graph(ea, eb, ej)
    assert g.kind == capi.KIND_LATTICE2D and g.info.fast_path == 0
    st, _ = _anneal_and_compare(capi, lambda: capi.States(g, capi.make_seeds(100 + R, R)))
    assert st.family == "checkerboard"


@pytest.fixture
def force_packed(monkeypatch):
    monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")


def _diluted_graph():
    from test_gpu_overlaps import _diluted_graph as make
    return make()


def test_bit_sliced_cubic_glass_and_a_shard(capi, exact, force_packed):
    ea, eb, ej = IR.cubic_glass(exact, 6)
    g = capi.Graph(ea, eb, ej, nvars=216, force_general=True)
    st, _ = _anneal_and_compare(capi, lambda: capi.States(g, capi.make_seeds(207, 70)))   # a partial last group
    assert st.family == "packed_bitsliced"
    shard, _ = _anneal_and_compare(capi, lambda: capi.States(g, capi.make_seeds(207, 70), replica_range=(20, 50)), bit0=20)
    assert shard.count == 30
    # the shard's records are the whole container's records of the same experiments
    for a, b in zip(shard.best()[:3], st.best()[:3]):
        assert np.array_equal(a, b[20:50])


def test_bit_sliced_diluted_graph(capi, force_packed):
    ea, eb, ej, n = _diluted_graph()
    g = capi.Graph(ea, eb, ej, nvars=n, force_general=True)
    st, _ = _anneal_and_compare(capi, lambda: capi.States(g, capi.make_seeds(210, 70)))
    assert st.family == "packed_bitsliced"


def test_real_coupling_gaussian_glass_with_biases_and_a_shard(capi, exact):
    ea, eb, _ = exact.cubic_lattice_edges(6, 1.0)
    rng = np.random.default_rng(2024)
    g = capi.Graph(ea, eb, rng.normal(size=len(ea)), nvars=216, biases=rng.normal(size=216), stable_path=True)
    st, _ = _anneal_and_compare(capi, lambda: capi.States(g, capi.make_seeds(300, 60)))
    assert st.family == "packed_real"
    shard, _ = _anneal_and_compare(capi, lambda: capi.States(g, capi.make_seeds(300, 60), replica_range=(8, 50)), bit0=8)   # slots across two words
    assert shard.count == 42


# ---- periods, several calls, updates by hand, reset --------------------------------------------------------------------------
def _three_paths(capi, exact, monkeypatch):
    ea, eb, ej = exact.square_lattice_edges(64, 4, -1.0, np.random.default_rng(9))
    yield capi.Graph(ea, eb, ej)
    monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
    ea, eb, ej = IR.cubic_glass(exact, 6)
    yield capi.Graph(ea, eb, ej, nvars=216, force_general=True)
    rng = np.random.default_rng(31)
    yield capi.Graph(ea, eb, rng.normal(size=len(ea)), nvars=216, stable_path=True)


@pytest.mark.parametrize("every", [1, 3, 100])
def test_periods_across_calls(capi, exact, monkeypatch, every):
    calls = [(4, 0.9), (5, np.linspace(1.0, 0.2, 5)), (7, 0.1), (2, 1.5)]
    families = []
    for g in _three_paths(capi, exact, monkeypatch):
        seeds = capi.make_seeds(600, 38)
        st, twin = capi.States(g, seeds), capi.States(g, seeds)
        families.append(st.family)
        st.set_track_best(every)
        for n, beta in calls:
            st.do_time_steps(n, beta)
        rec, points = _twin_records(twin, calls, every)
        assert points == [t for t in range(1, 19) if t % every == 0]
        _assert_equal(st, rec)
        _assert_same_container(st, twin)
        if every == 100:   # larger than every call: nothing recorded
            assert np.all(np.isinf(st.best()[0])) and st.best()[3] == 0 and not st.best()[1].any()
    assert families == ["checkerboard", "packed_bitsliced", "packed_real"]


def test_updates_by_hand_and_reset(capi, exact, monkeypatch):
    calls = [(3, 0.2), (4, 1.0), (2, 0.05)]
    for g in _three_paths(capi, exact, monkeypatch):
        seeds = capi.make_seeds(601, 35)
        st, twin = capi.States(g, seeds), capi.States(g, seeds)
        assert st.track_best == 0
        with pytest.raises(ValueError, match="keeps no records"):
            st.best()
        for n, beta in calls:   # every = 0: the updates are the caller's
            st.do_time_steps(n, beta)
            st.best_update()
        rec, points = _twin_records(twin, calls, 0, by_hand=(0, 1, 2))
        assert points == [3, 7, 9]
        _assert_equal(st, rec)
        kept = st.best_raw()
        st.best_reset()
        rec.reset()
        e, s, t, n = st.best()
        assert np.all(np.isinf(e)) and not t.any() and n == 0 and np.array_equal(s, rec.state) and np.array_equal(st.best_raw(), kept)
        st.do_time_steps(2, 0.05)   # hot: worse than the records before the reset, recorded all the same
        st.best_update()
        rec, _ = _twin_records(twin, [(2, 0.05)], 0, rec=rec, by_hand=(0,))
        assert rec.improved[-1].all()
        _assert_equal(st, rec)
        st.set_state(0, np.ones(g.nvars, dtype=np.uint8))   # leaves the records alone
        _assert_equal(st, rec)


# ---- tracking changes nothing ------------------------------------------------------------------------------------------------
def _same_with_and_without(make, prepare=lambda st: None, per_step=False):
    a, b = make(), make()
    for st in (a, b):
        prepare(st)
    a.set_track_best(2)
    betas = np.linspace(0.2, 0.9, 9)
    ea_, eb_ = a.do_time_steps(9, betas, per_step_energies=per_step), b.do_time_steps(9, betas, per_step_energies=per_step)
    if per_step:
        assert np.array_equal(_bits(ea_), _bits(eb_))
    a.do_time_steps(4, 0.6)
    b.do_time_steps(4, 0.6)
    _assert_same_container(a, b)
    assert a.best()[3] >= a.count and set(a.best()[2].tolist()) <= {2, 4, 6, 8, 10, 12}
    return a


def test_tracking_changes_nothing(capi, exact, monkeypatch):
    for g in _three_paths(capi, exact, monkeypatch):
        make = lambda: capi.States(g, capi.make_seeds(700, 36))
        family = _same_with_and_without(make).family
        _same_with_and_without(make, per_step=True)
        _same_with_and_without(make, lambda st: st.set_icm_every(3))
        if family == "packed_bitsliced":   # (cluster steps: one coupling size; the +-J lattice above has none)
            _same_with_and_without(make, lambda st: st.set_cluster_every(2))
    ea, eb, ej = exact.square_lattice_edges(64, 4, -1.0)
    g = capi.Graph(ea, eb, ej)
    _same_with_and_without(lambda: capi.States(g, capi.make_seeds(701, 8)), lambda st: st.set_cluster_every(2))


def test_tracking_changes_nothing_on_the_forced_strip_path(capi, exact):
    ea, eb, ej = exact.square_lattice_edges(1024, 128, -1.0, np.random.default_rng(3))
    g = capi.Graph(ea, eb, ej)

    def strips(st):
        st.set_option("strip", 1)
        st.set_option("disable_resident", 1)

    st = _same_with_and_without(lambda: capi.States(g, capi.make_seeds(702, 8)), strips)
    twin = capi.States(g, capi.make_seeds(702, 8))   # on the default path, read at the update points
    rec, _ = _twin_records(twin, [(9, np.linspace(0.2, 0.9, 9)), (4, 0.6)], 2)
    _assert_equal(st, rec)


# ---- ladders -----------------------------------------------------------------------------------------------------------------
def _ladder(case, exact, monkeypatch):
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
    return (ea, eb, ej), betas, family


def _run_ladders(edges, betas, copies, icm_every=0):
    """(tracked ladder run in one call, twin driven round by round with host read-outs, untracked ladder run in one call)."""
    from pyisingmontecarlo_amd.tempering import ClassicalTempering

    def make(track):
        pt = ClassicalTempering(edges, seed=4711, copies=copies)
        for beta in betas:
            pt.add_graph(float(beta))
        if icm_every:
            pt.set_replica_cluster_update_every(icm_every)
        if track:
            pt.set_track_minimum(True)
        return pt

    tracked, twin, plain = make(True), make(False), make(False)
    tracked.timesteps(24, 2)
    plain.timesteps(24, 2)
    containers = lambda pt: [c._states for c in pt._pair] if copies == 2 else [pt._states]
    recs = None
    for k in range(1, 13):   # a round swaps temperatures, never configurations: the configurations it measured are still there
        twin.timesteps(2, 2)
        sts = containers(twin)
        recs = recs or [MR.Records(st.count, st.graph.nvars) for st in sts]
        for rec, st in zip(recs, sts):
            assert st.timestep == 2 * k
            rec.update(2 * k, st.energies(), st.states())
    for other in (twin, plain):
        assert tracked.get_total_swaps() == other.get_total_swaps() > 0
        assert np.array_equal(tracked.get_permutation(), other.get_permutation())
        for a, b in zip(containers(tracked), containers(other)):
            _assert_same_container(a, b)
    for rec, st in zip(recs, containers(tracked)):
        _assert_equal(st, rec)
        assert len(set(rec.timestep.tolist())) > 1
    return tracked, recs


@pytest.mark.parametrize("case", ["lattice", "lattice_host_swaps", "bit_sliced", "real_coupling"])
def test_ladder_records_per_slot(capi, exact, monkeypatch, case):
    edges, betas, family = _ladder(case, exact, monkeypatch)
    tracked, recs = _run_ladders(edges, betas, 1)
    assert tracked._on_stream == (case != "lattice_host_swaps") and tracked._states.family == family
    e, s, t, rungs = tracked.get_minimum()
    assert np.array_equal(_bits(e), _bits(recs[0].energy)) and np.array_equal(s, recs[0].state) and np.array_equal(t, recs[0].timestep)
    assert np.array_equal(tracked.get_permutation()[rungs], np.arange(8))   # the rung each slot holds now


def test_ladder_of_two_copies_with_cluster_moves(capi, exact, monkeypatch):
    edges, betas, _ = _ladder("lattice", exact, monkeypatch)
    tracked, recs = _run_ladders(edges, betas, 2, icm_every=3)
    e, s, t, rungs = tracked.get_minimum()
    assert e.shape == (2, 8) and s.shape == (2, 8, 256) and rungs.shape == (2, 8)
    for i in range(2):
        assert np.array_equal(_bits(e[i]), _bits(recs[i].energy)) and np.array_equal(s[i], recs[i].state)


def test_ladder_refusals(exact):
    from pyisingmontecarlo_amd.tempering import ClassicalTempering

    edges = exact.square_lattice_edges(64, 4, -1.0)
    with pytest.raises(ValueError, match="one process and one device"):
        ClassicalTempering(edges, seed=1, devices=[0]).set_track_minimum(True)
    pt = ClassicalTempering(edges, seed=1)
    pt.add_graph(0.4)
    with pytest.raises(ValueError, match="set_track_minimum"):
        pt.get_minimum()


# ---- population annealing ----------------------------------------------------------------------------------------------------
def _population(capi, g, seeds, betas, sweeps):
    """A tracked pa_run against a twin driven step by step: the sources of tests/pa_reference.py from the energies read on the
    host, applied with pa_apply_sources."""
    import pa_reference as PR

    R = len(seeds) - 1
    st, twin = capi.States(g, seeds[:R]), capi.States(g, seeds[:R])
    st.set_track_best(1 << 62)   # the update points are the resamplings and the end of the run
    log = st.pa_run(betas, sweeps, int(seeds[R]))
    rec = MR.Records(R, g.nvars)
    for k, beta in enumerate(betas):
        if k:
            e = twin.energies()
            rec.update(twin.timestep, e, twin.states())
            ref = PR.sources(int(seeds[R]), k, e, betas[k] - betas[k - 1])
            assert ref["sum"] == int(log["sum"][k - 1])
            twin.pa_apply_sources(ref["src"])
        twin.do_time_steps(sweeps, float(beta))
    rec.update(twin.timestep, twin.energies(), twin.states())
    _assert_equal(st, rec)
    _assert_same_container(st, twin)
    assert len(set(rec.timestep.tolist())) > 1
    return rec


def _edge_list(ea, eb, ej):
    return [((int(a), int(b)), float(j)) for a, b, j in zip(ea, eb, ej)]


def test_population_annealing(capi, exact, monkeypatch):
    import py_monte_carlo

    ea, eb, ej = exact.square_lattice_edges(64, 4, -1.0, np.random.default_rng(4))
    betas, R, sweeps = [0.1, 0.5, 0.9, 1.3], 21, 3
    L = py_monte_carlo.Lattice(_edge_list(ea, eb, ej), seed_gen=77)
    seeds = np.array(L.make_seeds(R + 1), dtype=np.uint64)
    rec = _population(capi, capi.Graph(ea, eb, ej), seeds, betas, sweeps)
    res = L.run_population_annealing(betas, sweeps, R, track_minimum=True)
    arg = int(np.argmin(rec.energy))
    assert res.min_energy == rec.energy[arg] and np.array_equal(res.min_state, rec.state[arg])
    t = int(rec.timestep[arg])
    assert res.min_beta_index == (t + sweeps - 1) // sweeps - 1 and 0 <= res.min_beta_index < len(betas)
    plain = vars(py_monte_carlo.Lattice(_edge_list(ea, eb, ej), seed_gen=77).run_population_annealing(betas, sweeps, R))
    assert sorted(plain) == sorted(set(vars(res)) - {"min_energy", "min_state", "min_beta_index"})
    for key, value in plain.items():
        assert np.array_equal(np.asarray(value), np.asarray(vars(res)[key])), key
    monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
    ea, eb, ej = IR.cubic_glass(exact, 6)
    _population(capi, capi.Graph(ea, eb, ej, nvars=216, force_general=True), capi.make_seeds(78, 41), betas, sweeps)


# ---- the Python surface ------------------------------------------------------------------------------------------------------
def test_lattice_annealing_and_get_minimum(exact):
    import py_monte_carlo

    ea, eb, ej = exact.square_lattice_edges(64, 4, -1.0, np.random.default_rng(3))
    stops = [(0, 0.1), (12, 1.2), (24, 0.05)]
    T, R = 24, 9
    for every in (1, 4):
        L = py_monte_carlo.Lattice(_edge_list(ea, eb, ej), seed_gen=5)
        series, _ = L.run_monte_carlo_annealing_and_get_energies(stops, T, R)
        e, s, t = L.run_monte_carlo_annealing_and_get_minimum(stops, T, R, every=every)
        at = np.arange(every, T + 1, every)   # the update points; series[:, k] is the energy after timestep k + 1
        seen = series[:, at - 1]
        assert e.dtype == np.float64 and np.array_equal(_bits(e), _bits(seen.min(axis=1)))
        assert t.dtype == np.uint64 and np.array_equal(t, at[seen.argmin(axis=1)])   # argmin: the first of equals
        assert s.dtype == np.bool_ and s.shape == (R, 256)
    L.set_devices([0, 0])
    with pytest.raises(ValueError, match="one device"):
        L.run_monte_carlo_annealing_and_get_minimum(stops, T, R)
    L.set_devices([0])
    with pytest.raises(ValueError, match="every must be positive"):
        L.run_monte_carlo_annealing_and_get_minimum(stops, T, R, every=0)


def test_classic_ising_get_minimum(exact):
    import py_monte_carlo

    ea, eb, ej = exact.square_lattice_edges(64, 4, -1.0, np.random.default_rng(3))
    ci, twin = (py_monte_carlo.ClassicIsing(_edge_list(ea, eb, ej), None, 7, 21) for _ in range(2))
    ci.set_track_minimum(2)
    rec, t = MR.Records(7, 256), 0
    for beta, n in ((1.0, 6), (0.1, 4)):
        ci.run_monte_carlo(beta, n)
        for _ in range(n // 2):
            twin.run_monte_carlo(beta, 2)
            t += 2
            rec.update(t, twin.get_energies(), twin.get_states())
    e, s, t, n = ci.get_minimum()
    assert np.array_equal(_bits(e), _bits(rec.energy)) and np.array_equal(s, rec.state) and np.array_equal(t, rec.timestep) and n == rec.improvements
    assert np.array_equal(np.array(ci.get_states()), np.array(twin.get_states()))
    with pytest.raises(ValueError, match="minimum tracking is switched on"):
        ci.add_graph()
    assert ci.get_num_graphs() == 7
    ci.reset_minimum()
    assert np.all(np.isinf(ci.get_minimum()[0]))
    ci.set_track_minimum(0)
    ci.add_graph()
    assert ci.get_num_graphs() == 8


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(capi, exact):
    W, H = 256, 4   # (fields, open boundaries and anisotropy stay on the checkerboard path from 256 columns on)
    N = W * H
    ea, eb, ej = exact.square_lattice_edges(W, H, -1.0)
    x = np.arange(N) % W
    right = np.arange(len(ea)) % 2 == 0
    seeds = capi.make_seeds(3, 6)
    cases = {
        "f64 CSR": capi.Graph(*exact.cubic_lattice_edges(6), 216),   # a small graph without the force flag
        "field": capi.Graph(ea, eb, ej, N, biases=np.full(N, 0.5)),
        "open": capi.Graph(*[a[~(right & (np.repeat(x, 2) == W - 1))] for a in (ea, eb, ej)], N),
        "anisotropic": capi.Graph(ea, eb, np.where(right, -1.0, -2.0), N),
    }
    for reason, g in cases.items():
        st, twin = capi.States(g, seeds[:2]), capi.States(g, seeds[:2])
        with pytest.raises(ValueError, match=reason):
            st.set_track_best(1)
        with pytest.raises(ValueError, match=reason):
            st.best_update()
        assert st.track_best == 0
        st.do_time_steps(2, 0.4)   # unchanged and still usable
        twin.do_time_steps(2, 0.4)
        _assert_same_container(st, twin)
    assert capi.States(cases["f64 CSR"], seeds[:2]).family == "csr_f64"
    st = capi.States(capi.Graph(ea, eb, ej), seeds)
    st.set_track_best(3)
    with pytest.raises(ValueError, match="minimum tracking is switched on"):
        st.append(99)
    assert st.count == 6 and st.track_best == 3 and capi.last_error() != ""
    st.set_track_best(0)
    st.append(99)
    assert st.count == 7

"""Ladder statistics on the device.  The reference of every case is a TWIN ladder: the same graph, seeds and betas,
driven one round at a time; before each of its rounds the permutation, the round number and the energies are read on the host, and
the recorded rounds go through the numpy rule of tests/ladder_statistics_reference.py.  The counted ladder runs whole calls
(pt_run: one launch per round, or the rounds inside the persistent strip launch).  Round count, the eight arrays (the f64 sums bit
for bit) and in_kernel_rounds must be equal, and permutation, swap count, raw state words and energies must equal the same run with
statistics off."""
import numpy as np
import pytest

import ladder_statistics_reference as SR
import packed_icm_reference as IR
from ladder_icm_engine import ladder_seeds

pytestmark = pytest.mark.gpu


# ---- containers with the whole ladder attached -----------------------------------------------------------------------------------
def _states(capi, g, betas, seed):
    st = capi.States(g, np.array(ladder_seeds(capi, seed, len(betas))[0][0], dtype=np.uint64))
    st.pt_attach(betas, 0, len(betas), 1, seed)
    return st


def _twin_round(st, ref):
    """one exchange round of an on-stream ladder, recorded: what the round reads goes to the numpy rule"""
    energies = st.energies()
    st.pt_measure()
    before, rnd, _ = st.pt_state()
    st.pt_swap()
    ref.round(rnd, before, st.pt_state()[0], energies)


def _twin_run(twin, ref, T, f):
    """pt_run(T, f) in pieces"""
    for _ in range(T // f):
        twin.pt_time_steps(f)
        _twin_round(twin, ref)
    if T % f:
        twin.pt_time_steps(T % f)


def _same_ladder(a, b):
    assert a.timestep == b.timestep and np.array_equal(a.raw_state(), b.raw_state())
    assert np.array_equal(SR.bits(a.energies()), SR.bits(b.energies()))
    pa, pb = a.pt_state(), b.pt_state()
    assert np.array_equal(pa[0], pb[0]) and pa[1:] == pb[1:]


def _counted_against_twin(capi, g, betas, seed, calls, in_kernel_rounds=0):
    st, twin, plain = (_states(capi, g, betas, seed) for _ in range(3))
    st.pt_set_statistics(True)
    ref = SR.Statistics(len(betas))
    for T, f in calls:
        st.pt_run(T, f)
        plain.pt_run(T, f)
        _twin_run(twin, ref, T, f)
        SR.assert_equal(st.pt_statistics(), ref)
        _same_ladder(st, twin)
        _same_ladder(st, plain)
    got = st.pt_statistics()
    assert got["in_kernel_rounds"] == in_kernel_rounds and ref.rounds == sum(T // f for T, f in calls)
    assert ref.accepts.sum() == st.pt_state()[2] > 0   # rounds that exchange: the routing by permutation is under test
    return st, twin, ref


# ---- 1. one launch per round ------------------------------------------------------------------------------------------------------
CALLS_1 = [(41, 1), (40, 1)]           # an odd first call: the round parity carries over into the second
BETAS_1 = 0.40 + 0.01 * np.arange(6)   # 1024 spins near the transition, chosen with the CPU oracle engines: 81 rounds hold pairs
                                       # that are sometimes refused, labelled visits of both kinds and completed round trips


def _assert_not_vacuous(ref):
    assert ((ref.accepts > 0) & (ref.accepts < ref.attempts)).any() and ref.n_down.any() and ref.round_trips.sum() >= 1


def test_checkerboard_one_launch_per_round(capi, exact):
    """64 x 16: the smallest periodic lattice of 1024 spins that the checkerboard kernels serve (rows of whole 64-bit words)"""
    g = capi.Graph(*exact.square_lattice_edges(64, 16, -1.0))
    st, _, ref = _counted_against_twin(capi, g, BETAS_1, 71, CALLS_1)
    assert st.family == "checkerboard" and ref.rounds == 81
    _assert_not_vacuous(ref)
    assert ref.attempts[0] == 41 and ref.attempts[1] == 40


def test_32x32_ferromagnet_through_the_class(capi, exact):
    """32 x 32, 6 rungs, one round per timestep, two calls.  Rows of 32 spins are not served by the checkerboard kernels: the
    class attaches no ladder and keeps the statistics through the host twin -- on a GPU engine, against the numpy rule."""
    from pyisingmontecarlo_amd.tempering import ClassicalTempering

    def ladder():
        pt = ClassicalTempering(exact.square_lattice_edges(32, 32, -1.0), seed=71)
        for b in BETAS_1:
            pt.add_graph(float(b))
        return pt
    pt, twin, plain = ladder(), ladder(), ladder()
    pt.set_ladder_statistics()
    ref = SR.Statistics(6)
    for T, f in CALLS_1:
        pt.timesteps(T, f)
        plain.timesteps(T, f)
        for _ in range(T):
            twin.timesteps(f)
            before, energies, rnd = twin._perm.copy(), twin._states.energies(), twin._round
            twin._swap_step()
            ref.round(rnd, before, twin._perm, energies)
    assert not pt._on_stream
    SR.assert_equal(pt.get_ladder_statistics(), ref, in_kernel_rounds=0)
    _assert_not_vacuous(ref)
    for other in (twin, plain):
        assert np.array_equal(pt.get_permutation(), other.get_permutation()) and pt.get_total_swaps() == other.get_total_swaps()
        assert np.array_equal(pt._states.raw_state(), other._states.raw_state())
        assert np.array_equal(SR.bits(pt._states.energies()), SR.bits(other._states.energies()))


# ---- 2. the rounds inside the persistent strip launch -------------------------------------------------------------------------------
def test_inside_the_persistent_launch(capi, exact, monkeypatch):
    """1024 x 128 x 8 rungs, the shape of test_in_kernel_exchange_against_the_oracle_engine: pt_run(26, 4) holds 5 of its 6
    rounds inside the launch, pt_run(9, 3) 2 of 3; the last round of a block goes through the exchange kernel"""
    monkeypatch.setenv("ISINGMC_STRIP", "1")
    W, H, G = 1024, 128, 8
    g = capi.Graph(*exact.square_lattice_edges(W, H, -1.0))
    betas = np.linspace(0.4400, 0.4403, G)
    runs = {}
    for in_kernel in ("1", "0"):
        monkeypatch.setenv("ISINGMC_PT_IN_KERNEL", in_kernel)
        st = _states(capi, g, betas, 77)
        st.pt_time_steps(3)
        st.pt_set_statistics(True)
        st.pt_run(26, 4)
        st.pt_run(9, 3)
        runs[in_kernel] = st
    monkeypatch.setenv("ISINGMC_PT_IN_KERNEL", "1")
    twin, plain = _states(capi, g, betas, 77), _states(capi, g, betas, 77)
    ref = SR.Statistics(G)
    for c in (twin, plain):
        c.pt_time_steps(3)
    plain.pt_run(26, 4)
    plain.pt_run(9, 3)
    _twin_run(twin, ref, 26, 4)
    _twin_run(twin, ref, 9, 3)
    assert ref.rounds == 9 and ref.accepts.sum() == twin.pt_state()[2] > 0
    for in_kernel, inside in (("1", 7), ("0", 0)):
        got = runs[in_kernel].pt_statistics()
        SR.assert_equal(got, ref, in_kernel_rounds=inside)
        _same_ladder(runs[in_kernel], twin)
        _same_ladder(runs[in_kernel], plain)


# ---- 3. replica-packed families -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rungs", [5, 33])   # 33: a ladder across two replica groups
def test_packed_bit_sliced(capi, exact, monkeypatch, n_rungs):
    monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
    g = capi.Graph(*IR.cubic_glass(exact, 4), nvars=64, force_general=True)
    betas = 0.30 + (0.10 if n_rungs == 5 else 0.02) * np.arange(n_rungs)
    st, _, ref = _counted_against_twin(capi, g, betas, 81, [(21, 1), (12, 2)])
    assert st.family == "packed_bitsliced" and st.count == n_rungs and ref.rounds == 27 and ref.n_down.any()


def test_packed_real(capi, exact, monkeypatch):
    monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
    monkeypatch.setenv("ISINGMC_FORCE_REAL", "1")   # (a graph of 36 sites takes the real-coupling family only when it is told to)
    ea, eb, _ = exact.square_lattice_edges(6, 6, -1.0)
    rng = np.random.default_rng(2024)
    g = capi.Graph(ea, eb, rng.normal(size=len(ea)), nvars=36, biases=rng.normal(size=36), force_general=True)
    st, _, ref = _counted_against_twin(capi, g, 0.30 + 0.10 * np.arange(5), 91, [(21, 1), (12, 2)])
    assert st.family == "packed_real" and ref.rounds == 27 and ref.n_down.any()


# ---- 4. two copies with cluster moves between them -----------------------------------------------------------------------------------
def test_two_copies_with_cluster_moves(capi, exact):
    """copies=2, every 3rd timestep a move, a round after every 2nd: one set of statistics per copy, and a move counts nothing"""
    from pyisingmontecarlo_amd.tempering import ClassicalTempering
    edges = exact.square_lattice_edges(64, 16, -1.0)
    T, f = 24, 2

    def ladder():
        pt = ClassicalTempering(edges, seed=71, copies=2)
        for b in BETAS_1:
            pt.add_graph(float(b))
        pt.set_replica_cluster_update_every(3)
        return pt
    pt, twin, plain = ladder(), ladder(), ladder()
    pt.set_ladder_statistics()   # before the first timestep
    pt.timesteps(T, f)
    plain.timesteps(T, f)
    refs = [SR.Statistics(6), SR.Statistics(6)]
    for t in range(1, T + 1):
        twin.timesteps(1)
        if t % f == 0:
            for c, ref in zip(twin._pair, refs):
                _twin_round(c._states, ref)
    d = pt.get_ladder_statistics()
    assert pt._on_stream and np.array_equal(d["rounds"], [T // f] * 2) and not d["in_kernel_rounds"].any()
    for c, ref in enumerate(refs):
        SR.assert_equal({k: v[c] for k, v in d.items()}, ref)
        SR.assert_equal(pt._pair[c]._states.pt_statistics(), ref)
        for other in (twin, plain):
            _same_ladder(pt._pair[c]._states, other._pair[c]._states)
    assert not np.array_equal(d["accepts"][0], d["accepts"][1]) or not np.array_equal(SR.bits(refs[0].sum_e), SR.bits(refs[1].sum_e))
    assert pt.get_replica_cluster_stats() is not None and pt.get_total_swaps() == d["accepts"].sum() > 0
    # a move timestep alone (the 27th: t % 3 == 2) updates nothing
    pt.timesteps(2)
    before = pt.get_ladder_statistics()
    pt.timesteps(1)
    after = pt.get_ladder_statistics()
    assert pt._t == 27 and all(np.array_equal(before[k], after[k], equal_nan=True) for k in before)


# ---- 5. the in-process ladder over two shards of one device ------------------------------------------------------------------------
def test_two_shards_hold_the_whole_ladders_statistics(capi, exact):
    from pyisingmontecarlo_amd.tempering import ClassicalTempering
    edges = exact.square_lattice_edges(64, 16, -1.0)

    def ladder(**kw):
        pt = ClassicalTempering(edges, seed=71, **kw)
        for b in BETAS_1:
            pt.add_graph(float(b))
        pt.set_ladder_statistics()
        return pt
    solo, group = ladder(), ladder(devices=[0, 0])
    for pt in (solo, group):
        pt.timesteps(41, 1)
        pt.timesteps(20, 2)
    assert group.group_backend() == "copy" and len(group._shards) == 2
    want = solo._states.pt_statistics()
    assert want["rounds"] == 51 and want["accepts"].sum() == solo.get_total_swaps() == group.get_total_swaps() > 0
    for shard in group._shards:
        got = shard.pt_statistics()
        assert got["rounds"] == want["rounds"] and got["in_kernel_rounds"] == 0
        for k in SR.ARRAYS:
            assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k
    assert np.array_equal(group.get_permutation(), solo.get_permutation())
    d, s = group.get_ladder_statistics(), solo.get_ladder_statistics()
    assert all(np.array_equal(d[k], s[k], equal_nan=True) for k in s)
    # the solo ladder against the rule
    twin, ref = _states(capi, solo._states.graph, BETAS_1, 71), SR.Statistics(6)
    _twin_run(twin, ref, 41, 1)
    _twin_run(twin, ref, 20, 2)
    SR.assert_equal(want, ref)


# ---- 6. lifecycle --------------------------------------------------------------------------------------------------------------
def test_lifecycle(capi, exact):
    g = capi.Graph(*exact.square_lattice_edges(64, 16, -1.0))
    seeds = np.array(ladder_seeds(capi, 71, 6)[0][0], dtype=np.uint64)
    bare = capi.States(g, seeds)
    for call in (bare.pt_statistics, bare.pt_reset_statistics, lambda: bare.pt_set_statistics(True)):
        with pytest.raises(ValueError, match="no ladder attached"):
            call()
    st, twin, ref = _counted_against_twin(capi, g, BETAS_1, 71, [(7, 1)])
    # off: the ladder runs on, the values stay; on again: counting continues where the ladder now stands
    st.pt_set_statistics(False)
    st.pt_run(4, 1)
    for _ in range(4):
        twin.pt_time_steps(1)
        twin.pt_measure()
        twin.pt_swap()
    SR.assert_equal(st.pt_statistics(), ref)
    st.pt_set_statistics(True)
    st.pt_run(6, 2)
    _twin_run(twin, ref, 6, 2)
    SR.assert_equal(st.pt_statistics(), ref)
    assert ref.rounds == 10 and st.pt_state()[1] == 14
    _same_ladder(st, twin)
    # reset: zeros, the setting stays
    st.pt_reset_statistics()
    ref.reset()
    SR.assert_equal(st.pt_statistics(), ref, in_kernel_rounds=0)
    st.pt_run(3, 1)
    _twin_run(twin, ref, 3, 1)
    SR.assert_equal(st.pt_statistics(), ref)
    assert ref.rounds == 3
    # detach discards them; a new ladder on the container starts clean and switched off
    st.pt_detach()
    with pytest.raises(ValueError, match="no ladder attached"):
        st.pt_statistics()
    st.pt_attach(BETAS_1, 0, 6, 1, 71)
    for call in (st.pt_statistics, st.pt_reset_statistics):
        with pytest.raises(ValueError, match="holds no statistics"):
            call()
    st.pt_run(2, 1)
    st.pt_set_statistics(True)
    SR.assert_equal(st.pt_statistics(), SR.Statistics(6), in_kernel_rounds=0)
    st.pt_run(2, 1)
    got = st.pt_statistics()
    assert got["rounds"] == 2 and np.array_equal(got["attempts"], [1, 1, 1, 1, 1]) and st.pt_state()[1] == 4

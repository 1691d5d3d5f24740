"""Ladder statistics without a GPU: the library's host twin against the numpy rule of
tests/ladder_statistics_reference.py, the rule's invariants, ClassicalTempering on the host swap path with the oracle-backed
engine injected, the refusals, and betas_from_flow on an analytic flow."""
import ctypes as C

import numpy as np
import pytest

import ladder_statistics_reference as SR
from helpers import OracleLatEngine


def _drive(capi, n, round0, n_rounds, seed, on_round=None):
    """n_rounds exchange rounds from round number round0 on random energies: (library statistics, reference, swaps)"""
    rng = np.random.default_rng(seed)
    betas = 0.5 + 0.01 * np.arange(n)
    perm = rng.permutation(n).astype(np.uint32)
    got, want, swaps = capi.pt_statistics_zeros(n), SR.Statistics(n), 0
    for k in range(n_rounds):
        rnd = round0 + k
        energies = rng.normal(scale=60.0, size=n)   # |d beta d E| of order one: accepted and refused pairs alike
        before = perm.copy()
        swaps += capi.pt_swap_round(1234, rnd, betas, energies, perm)
        capi.pt_statistics_round(got, rnd, before, perm, energies)
        want.round(rnd, before, perm, energies)
        if on_round:
            on_round(rnd, before, perm.copy(), got)
    return got, want, swaps


@pytest.mark.parametrize("n", [1, 2, 3, 8, 33])
@pytest.mark.parametrize("round0", [0, 1, (1 << 32) - 3])   # both parities first; round numbers across 2^32
def test_host_twin_against_the_rule(capi, n, round0):
    got, want, swaps = _drive(capi, n, round0, 40, 100 * n + (round0 & 7))
    SR.assert_equal(got, want)
    assert got["rounds"] == 40 and int(got["accepts"].sum()) == swaps
    if n >= 3:
        assert ((got["accepts"] > 0) & (got["accepts"] < got["attempts"])).any() and got["n_down"].any()
    if n == 1:
        assert not got["n_up"].any() and not got["labels"].any() and got["sum_e"][0] != 0.0


def test_invariants(capi):
    n, round0, T = 8, 5, 400
    trips_before = [np.zeros(n, dtype=np.uint64)]

    def on_round(rnd, before, after, got):
        changed = np.flatnonzero(got["round_trips"] != trips_before[0])
        assert set(changed) <= {int(after[0])}   # a round trip completes only at rung 0
        trips_before[0] = got["round_trips"].copy()
        assert ((got["n_up"] + got["n_down"]) <= got["rounds"]).all()
    got, want, swaps = _drive(capi, n, round0, T, 7, on_round)
    SR.assert_equal(got, want)
    rounds_of_parity = [sum(1 for k in range(T) if (round0 + k) % 2 == par) for par in (0, 1)]
    assert np.array_equal(got["attempts"], [rounds_of_parity[i % 2] for i in range(n - 1)])
    assert int(got["accepts"].sum()) == swaps and (got["accepts"] <= got["attempts"]).all()
    assert got["round_trips"].sum() > 0 and got["n_up"][0] == got["rounds"] and got["n_down"][-1] == got["rounds"]
    assert got["n_down"][0] == 0 and got["n_up"][-1] == 0


def test_host_twin_refuses_bad_arguments(capi):
    stats = capi.pt_statistics_zeros(3)
    with pytest.raises(ValueError, match="not a permutation"):
        capi.pt_statistics_round(stats, 0, np.array([0, 1, 7], dtype=np.uint32), np.arange(3, dtype=np.uint32), np.zeros(3))
    with pytest.raises(ValueError, match="cover the ladder"):
        capi.pt_statistics_round(stats, 0, np.arange(2, dtype=np.uint32), np.arange(3, dtype=np.uint32), np.zeros(3))
    assert stats["rounds"] == 0 and not stats["sum_e"].any()


# ---- ClassicalTempering on the host swap path ----------------------------------------------------------------------------------
BETAS = (0.30, 0.34, 0.38, 0.42)


def _ladder(exact, **kw):
    from pyisingmontecarlo_amd.tempering import ClassicalTempering
    pt = ClassicalTempering(exact.square_lattice_edges(64, 4, -1.0), seed=5, engine_factory=lambda: OracleLatEngine(64, 4), **kw)
    for b in BETAS:
        pt.add_graph(b)
    return pt


def _replay(twin, refs, n_rounds, f):
    """the twin ladder one round at a time: the recorded (permutation, energies) of every copy go through the numpy rule"""
    copies = twin._pair if twin._pair is not None else [twin]
    for _ in range(n_rounds):
        twin.timesteps(f)
        for c, ref in zip(copies, refs):
            before, energies, rnd = c._perm.copy(), c._states.energies(), c._round
            c._swap_step()
            ref.round(rnd, before, c._perm, energies)


@pytest.mark.parametrize("copies", [1, 2])
def test_class_on_the_host_swap_path(capi, oracle, exact, copies):
    kw = {"copies": 2} if copies == 2 else {}
    pt, twin, plain = _ladder(exact, **kw), _ladder(exact, **kw), _ladder(exact, **kw)
    refs = [SR.Statistics(len(BETAS)) for _ in range(copies)]
    pt.set_ladder_statistics()   # before the first timestep
    pt.timesteps(2 * 30, 2)
    plain.timesteps(2 * 30, 2)
    _replay(twin, refs, 30, 2)
    assert not pt._on_stream

    def check(d):
        assert list(d) == ["rounds", "in_kernel_rounds", "attempts", "accepts", "acceptance", "n_up", "n_down", "flow", "mean_energy",
                           "var_energy", "round_trips", "labels"]
        for c, ref in enumerate(refs):
            one = {k: v[c] for k, v in d.items()} if copies == 2 else d
            SR.assert_equal(one, ref, in_kernel_rounds=0)
            with np.errstate(divide="ignore", invalid="ignore"):
                acc = ref.accepts / ref.attempts.astype(np.float64)
                flow = ref.n_up / (ref.n_up + ref.n_down).astype(np.float64)
            assert one["acceptance"].dtype == np.float64 and np.array_equal(one["acceptance"], acc, equal_nan=True)
            assert np.array_equal(one["flow"], flow, equal_nan=True)
        if copies == 2:
            assert all(np.asarray(v).shape[0] == 2 for v in d.values())
    check(pt.get_ladder_statistics())
    assert all(r.accepts.sum() > 0 for r in refs) and pt.get_total_swaps() == sum(int(r.accepts.sum()) for r in refs)
    # counting changes nothing
    assert np.array_equal(pt.get_permutation(), plain.get_permutation()) and np.array_equal(pt.get_permutation(), twin.get_permutation())
    assert np.array_equal(pt._states.states(), plain._states.states())
    # off: the values stay; on again: counting goes on
    pt.set_ladder_statistics(False)
    pt.timesteps(4, 2)
    twin.timesteps(4, 2)
    check(pt.get_ladder_statistics())
    pt.set_ladder_statistics(True)
    pt.timesteps(6, 2)
    _replay(twin, refs, 3, 2)
    check(pt.get_ladder_statistics())
    # reset: zeros, NaN ratios, the setting stays
    pt.reset_ladder_statistics()
    for r in refs:
        r.reset()
    d = pt.get_ladder_statistics()
    check(d)
    assert not np.asarray(d["rounds"]).any() and np.isnan(d["acceptance"]).all() and np.isnan(d["flow"]).all() and np.isnan(d["mean_energy"]).all()
    pt.timesteps(4, 2)
    _replay(twin, refs, 2, 2)
    check(pt.get_ladder_statistics())


def test_switched_on_after_the_first_timesteps(capi, oracle, exact):
    pt, twin = _ladder(exact), _ladder(exact)
    pt.timesteps(6, 2)
    twin.timesteps(6, 2)
    pt.set_ladder_statistics()
    ref = SR.Statistics(len(BETAS))
    pt.timesteps(10, 2)
    _replay(twin, [ref], 5, 2)   # rounds 3 .. 7: the parity carries over
    SR.assert_equal(pt.get_ladder_statistics(), ref, in_kernel_rounds=0)
    assert ref.attempts[0] == 2 and ref.attempts[1] == 3


# ---- refusals, before any device is touched ------------------------------------------------------------------------------------
def test_refusals(capi, exact):
    from pyisingmontecarlo_amd.tempering import ClassicalTempering
    for kw in ({}, {"copies": 2}, {"devices": [0, 1]}):
        pt = ClassicalTempering(exact.square_lattice_edges(64, 4, -1.0), seed=5, **kw)   # the HIP engine: never built here
        for b in BETAS:
            pt.add_graph(b)
        for call in (pt.get_ladder_statistics, pt.reset_ladder_statistics):
            with pytest.raises(ValueError, match="holds no statistics"):
                call()
        assert pt._states is None
    L = capi.lib()
    for rc in (L.isingmc_pt_set_statistics(None, 1), L.isingmc_pt_statistics_reset(None),
               L.isingmc_pt_statistics_get(None, None, None, *([None] * 8))):
        assert rc == capi.ERR_INVALID and "no ladder attached" in capi.last_error()
    assert L.isingmc_host_pt_statistics_round(C.c_uint64(0), 2, *([None] * 11), None) == capi.ERR_INVALID
    assert L.isingmc_abi_version() == 4


# ---- the helper ----------------------------------------------------------------------------------------------------------------
def test_betas_from_flow():
    from pyisingmontecarlo_amd.tempering import betas_from_flow
    betas = np.array([0.2, 0.25, 0.45, 0.5, 0.9, 1.0])
    n = len(betas)
    up, down = (n - 1 - np.arange(n)) * 7, np.arange(n) * 7   # f linear in the rung index: nothing to move
    assert np.array_equal(betas_from_flow(betas, up, down), betas)
    # a bottleneck between rungs 2 and 3 (f falls from 0.9 to 0.1 there): the new rungs crowd into that interval, ends kept
    f = np.array([1.0, 0.95, 0.9, 0.1, 0.05, 0.0])
    new = betas_from_flow(betas, np.round(1000 * f), np.round(1000 * (1 - f)))
    assert new[0] == betas[0] and new[-1] == betas[-1] and (np.diff(new) > 0).all()
    assert ((new > betas[2]) & (new < betas[3])).sum() == 4
    # f = 0.5 + ... : piecewise-linear inversion by hand; a non-monotone measurement is flattened from the last rung on
    got = betas_from_flow([1.0, 2.0, 3.0], [10, 2, 0], [0, 8, 10], n_rungs=5)   # f = 1, 0.2, 0
    assert np.allclose(got, [1.0, 1.0 + 0.25 / 0.8, 1.0 + 0.5 / 0.8, 1.0 + 0.75 / 0.8, 3.0])
    bumpy = betas_from_flow([1.0, 2.0, 3.0, 4.0], [9, 2, 4, 0], [0, 8, 6, 9])   # f = 1, .2, .4, 0 -> 1, .4, .4, 0
    assert bumpy[0] == 1.0 and bumpy[-1] == 4.0 and (np.diff(bumpy) >= 0).all()
    unvisited = betas_from_flow(betas, [5, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 5])   # f known at the ends only: linear -> unchanged
    assert np.allclose(unvisited, betas)
    with pytest.raises(ValueError):
        betas_from_flow([1.0], [1], [0])

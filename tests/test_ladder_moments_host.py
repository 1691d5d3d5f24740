"""Per-site spin sums by rung without a GPU: the reference accumulator of the device tests against a loop over
samples, rungs and sites, and what ClassicalTempering refuses, with the oracle-backed engine injected."""
import numpy as np
import pytest

import ladder_moments_reference as LR
from helpers import OracleLatEngine, OracleLatStates


def test_accumulator_against_a_loop():
    rng = np.random.default_rng(3)
    G, N, S = 7, 11, 5
    acc = LR.Accumulator(G, N)
    want = np.zeros((G, N), dtype=np.int64)
    assert not acc.saw_a_permutation()
    for k in range(S):
        states = rng.random((G, N)) < 0.5
        perm = np.arange(G, dtype=np.uint32) if k == 0 else rng.permutation(G).astype(np.uint32)
        acc.add(states, perm)
        for i in range(G):
            for v in range(N):
                want[i, v] += 1 if states[perm[i], v] else -1
        assert acc.saw_a_permutation() == (k > 0)
    assert acc.n == S and acc.site.dtype == np.int64 and np.array_equal(acc.site, want)
    assert (np.abs(acc.site) <= S).all() and ((acc.site + S) % 2 == 0).all()
    with pytest.raises(AssertionError):
        acc.add(states, np.zeros(G, dtype=np.uint32))   # no permutation
    acc.reset()
    assert acc.n == 0 and not acc.site.any() and not acc.perms


def _ladder(exact, factory, **kw):
    from pyisingmontecarlo_amd.tempering import ClassicalTempering
    pt = ClassicalTempering(exact.square_lattice_edges(64, 4, -1.0), seed=5, engine_factory=factory, **kw)
    for b in (0.3, 0.4, 0.5):
        pt.add_graph(b)
    return pt


class _StatesWithSums(OracleLatStates):
    """an engine that does keep sums, on a ladder that takes the host swap step"""

    def set_moments_every(self, every, per_replica=False, bonds=False, per_rung=False):
        raise AssertionError("the ladder must refuse before it reaches the container")


class _EngineWithSums(OracleLatEngine):
    def make_states(self, seeds, replica_range=None):
        lo, hi = replica_range if replica_range is not None else (0, len(seeds))
        return _StatesWithSums(self.lat, seeds[lo:hi])


def _calls(pt):
    return (lambda: pt.set_measure_spins_every(2), pt.get_measured_spins, pt.reset_measured_spins)


def test_refused_by_the_ladder_class(capi, oracle, exact):
    engine = lambda: OracleLatEngine(64, 4)   # noqa: E731
    for call in _calls(_ladder(exact, engine)):
        with pytest.raises(ValueError, match="this engine keeps no spin sums"):
            call()
    for copies in (1, 2):
        for call in _calls(_ladder(exact, lambda: _EngineWithSums(64, 4), copies=copies)):
            with pytest.raises(ValueError, match="host swap step"):
                call()
    for call in _calls(_ladder(exact, None, devices=[0, 1])):   # (refused before any device is touched)
        with pytest.raises(ValueError, match=r"devices=\[\.\.\.\]"):
            call()
    pt = _ladder(exact, engine)
    pt._world = 2   # what a torch.distributed group of two ranks leaves behind
    for call in _calls(pt):
        with pytest.raises(ValueError, match="several ranks"):
            call()
    with pytest.raises(ValueError, match="must not be negative"):
        _ladder(exact, engine).set_measure_spins_every(-1)
    # a refusal leaves the ladder usable: it runs and exchanges as before
    pt, ref = _ladder(exact, engine), _ladder(exact, engine)
    with pytest.raises(ValueError):
        pt.set_measure_spins_every(2)
    pt.timesteps(4, 2)
    ref.timesteps(4, 2)
    assert np.array_equal(pt._states.states(), ref._states.states()) and np.array_equal(pt.get_permutation(), ref.get_permutation())

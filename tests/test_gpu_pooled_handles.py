"""Every pooled stream and event of a container is created, released with the container and used again by the next one.

A container's streams and events are held in handles (csrc/owned_block.hpp) that hand them back to the pools of core.hip when
the container goes.  One pass creates all of them on two small containers -- the main stream and the timing events at
creation, two forced replica lanes with their events and the fork event, the copy stream and slab events of the sampling
pipeline, the two events of `icm_between`, the two events of an overlap series -- and destroys the containers.  The second
pass does the same on fresh containers, which draw the recycled streams and events out of the pools (destroyed in the other
order, so that the pools hand them out differently), and everything it computes must equal the first pass BIT FOR BIT: which
stream or event carries a launch is no part of a result.  No tolerance: every compared value is an integer or an f64
produced by the same arithmetic.

Shape: the 64 x 4 +-J lattice with 4 replicas, the smallest the checkerboard kernels serve (a row is a multiple of 64 sites);
two lanes of two replicas each."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BETA = 0.5
R = 4


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _one_pass(capi, exact, a_goes_first):
    ea, eb, ej = exact.square_lattice_edges(64, 4, -1.0, np.random.default_rng(64))
    g = capi.Graph(ea, eb, ej)
    a, b = capi.States(g, capi.make_seeds(101, R)), capi.States(g, capi.make_seeds(202, R))
    out = {}
    for name, st in (("a", a), ("b", b)):
        assert st.family == "checkerboard"
        st.set_option("disable_resident", 1)   # the streaming kernels: the ones that take replica lanes
        st.set_option("strip", 0)
        st.set_option("streams", 2)
        st.do_time_steps(5, BETA)
        energies, states = st.run_sampling(BETA, 2, 2, 2)   # (both containers: the move below needs equal timesteps)
        assert energies.shape == (R, 2) and states.shape == (R, 2, g.nvars)
        out[name + ".sample_energies"], out[name + ".samples"] = _bits(energies), states.copy()
    slots = np.arange(R, dtype=np.uint32)
    a.icm_between(b, slots, slots[::-1].copy())
    out["between_stats"] = np.stack(a.icm_between_stats())
    series = a.overlap_series(b, capacity=2)
    series.record()
    t, spin, link, _ = series.get()
    out["series"] = np.concatenate([t.astype(np.int64), spin.ravel(), link.ravel()])
    series.close()
    for name, st in (("a", a), ("b", b)):
        st.do_time_steps(3, BETA)   # on the lanes again, behind the move
        out[name + ".energies"], out[name + ".raw"], out[name + ".t"] = _bits(st.energies()), st.raw_state(), st.timestep
    for st in ((a, b) if a_goes_first else (b, a)):
        st.close()
    g.close()
    return out


def test_recycled_streams_and_events_change_nothing(capi, exact):
    first = _one_pass(capi, exact, True)
    second = _one_pass(capi, exact, False)
    assert first.keys() == second.keys()
    for key in first:
        assert np.array_equal(first[key], second[key]), key
    assert first["a.t"] == first["b.t"] >= 5 + 1 + 3
    assert not np.array_equal(first["a.raw"], first["b.raw"])   # (two different containers were compared)

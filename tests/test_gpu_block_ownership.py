"""Every device block and pinned block a graph or a container takes comes back when it is destroyed.

A container's blocks are held in handles (csrc/owned_block.hpp) that hand them back to the block caches on destruction, on
reset() and when another block is assigned over them; `isingmc_debug_live_blocks` counts the blocks that owners hold at the
moment.  Every case reads the two counts, builds a graph and a container, exercises one feature, destroys both and reads the
counts again: they must be back where they were.  The allocation cache is on (the default; with ISINGMC_NO_ALLOC_CACHE=1 nothing is
counted, and the cases say so).  No case provokes a failure: assignment over a block left by a failed call is the matter of
tests/owned_block_host.cpp.

Shapes, the smallest that reach each owner: the checkerboard family on 64 x 4 (a row of the lattice kernels is a multiple of 64
sites: a 16 x 16 lattice is served by the f64 CSR family, and is a case of that family here), uniform for the Swendsen-Wang steps
and +-J otherwise; the strip kernel on 1024 x 128, the smallest geometry of tests/test_gpu_strip.py; the multi-class kernels on
256 x 4 with a field and with an open boundary (whole quads per row); a general graph of 240 sites forced onto the f64 CSR, the
bit-sliced packed and the real-coupling family with the switches of the variant tests."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BETA = 0.5


# ---- graphs ---------------------------------------------------------------------------------------------------------------------
def _general_edges(exact):
    """240 sites: the bonds of a periodic 20 x 12 grid with +-1 couplings (20 is no multiple of 64: no lattice kernel takes it)."""
    return exact.square_lattice_edges(20, 12, 1.0, np.random.default_rng(2012))


def _graph(spec, capi, exact, monkeypatch):
    """(graph, family): the switches are read when graphs and containers are created."""
    if spec in ("board", "glass"):
        ea, eb, ej = exact.square_lattice_edges(64, 4, -1.0, np.random.default_rng(64) if spec == "glass" else None)
        return capi.Graph(ea, eb, ej), "checkerboard"
    if spec == "lattice16":   # periodic 16 x 16: no lattice kernel, the LDS-resident CSR kernel
        ea, eb, ej = exact.square_lattice_edges(16, 16, -1.0)
        return capi.Graph(ea, eb, ej), "csr_f64"
    if spec == "strip":
        monkeypatch.setenv("ISINGMC_STRIP", "1")
        monkeypatch.setenv("ISINGMC_DISABLE_RESIDENT", "1")
        ea, eb, ej = exact.square_lattice_edges(1024, 128, -1.0)
        return capi.Graph(ea, eb, ej), "checkerboard"
    if spec in ("field", "open"):
        W, H = 256, 4
        ea, eb, ej = exact.square_lattice_edges(W, H, -1.0)
        biases = None
        if spec == "field":
            biases = np.full(W * H, 0.25)
        else:
            keep = ~((ea % W == W - 1) & (eb % W == 0))   # the right bonds of the last column
            ea, eb, ej = ea[keep], eb[keep], ej[keep]
        g = capi.Graph(ea, eb, ej, nvars=W * H, biases=biases)
        assert g.kind == capi.KIND_LATTICE2D and g.info.fast_path == (1 if spec == "field" else 2)
        return g, "checkerboard"
    family = {"csr": "csr_f64", "packed": "packed_bitsliced", "real": "packed_real"}[spec]
    for name in {"csr": ("DISABLE_REAL", "DISABLE_PACKED"), "packed": ("FORCE_PACKED",), "real": ("FORCE_REAL",)}[spec]:
        monkeypatch.setenv("ISINGMC_" + name, "1")
    ea, eb, ej = _general_edges(exact)
    return capi.Graph(ea, eb, ej, nvars=240, force_general=True), family


# ---- features: each takes the graph and returns the containers it made ---------------------------------------------------------
def _states(capi, g, family, R, tag=0):
    st = capi.States(g, capi.make_seeds(77 + tag, R))
    assert st.family == family
    return st


def _append(capi, g, family):
    """Across a reserve() growth (2 -> 3 -> 4 -> 6 replicas' room), or into a second replica group (experiment 33)."""
    packed = family.startswith("packed")
    st = _states(capi, g, family, 31 if packed else 2)
    st.do_time_steps(2, BETA)
    for k in range(3):
        st.append(1000 + k, np.ones(g.nvars, dtype=np.uint8) if k == 1 else None)
    assert st.count == (34 if packed else 5)
    st.do_time_steps(3, BETA)
    assert np.isfinite(st.energies()).all()
    return [st]


def _betas(capi, g, family):
    """Per-replica betas set, used, cleared; a packed container then opens a new group, which drops its per-group tables, and
    takes betas again."""
    packed = family.startswith("packed")
    st = _states(capi, g, family, 32 if packed else 4)
    for _ in range(2):
        st.set_betas(np.linspace(0.3, 0.6, st.count))
        st.do_time_steps(3)
        st.set_betas(None)
        st.do_time_steps(2, BETA)
        st.append(2000 + st.count)
    st.set_betas(np.linspace(0.3, 0.6, st.count))   # destroyed with the tables set
    st.do_time_steps(2)
    return [st]


def _ladder_round_trip(st, R, seed):
    st.pt_attach(np.linspace(0.3, 0.6, R), 0, R, 1, seed)
    st.pt_run(15, 5)   # three exchange rounds
    st.synchronize()


def _ladder(capi, g, family):
    """Attach, a few rounds, detach, attach again; destroyed with the ladder attached."""
    R = 40 if family == "packed_bitsliced" else 8
    st = _states(capi, g, family, R)
    _ladder_round_trip(st, R, 5)
    st.pt_detach()
    st.do_time_steps(2, BETA)
    _ladder_round_trip(st, R, 6)
    assert st.pt_state()[1] >= 3
    return [st]


def _cluster(capi, g, family):
    st = _states(capi, g, family, 6)
    st.set_cluster_every(2)
    st.do_time_steps(6, 0.42)
    assert (st.cluster_stats()[0] > 0).all()
    return [st]


def _icm_inside(capi, g, family):
    st = _states(capi, g, family, 6)
    st.set_icm_every(2)
    st.do_time_steps(6, BETA)
    st.icm_stats()
    return [st]


def _icm_between(capi, g, family):
    a, b = _states(capi, g, family, 6, 1), _states(capi, g, family, 6, 2)
    for st in (a, b):
        st.do_time_steps(3, BETA)
    slots = np.arange(6, dtype=np.uint32)
    a.icm_between(b, slots[:4], slots[:4][::-1].copy())
    a.icm_between(b, slots, slots)   # more pairs than the call before
    a.icm_between_stats()
    assert a.timestep == b.timestep == 5
    return [a, b]


def _track_best(capi, g, family):
    st = _states(capi, g, family, 6)
    st.set_track_best(2)
    st.do_time_steps(6, BETA)
    assert st.best()[3] >= 6
    return [st]


def _pa_resample(capi, g, family):
    st = _states(capi, g, family, 6)
    st.do_time_steps(4, 0.2)
    st.pa_resample(0.1, 99, 1)
    assert len(st.pa_last()["src"]) == 6
    st.append(3000)              # the population grows: the next resampling regrows its tables
    st.pa_resample(0.1, 99, 2)
    assert (st.pa_last()["src"] < 7).all()
    return [st]


def _sampling(capi, g, family):
    st = _states(capi, g, family, 3)
    energies, states = st.run_sampling(BETA, 2, 2, 3)
    assert energies.shape == (3, 3) and states.shape == (3, 3, g.nvars)
    st.states()
    return [st]


def _step_energies(capi, g, family):
    st = _states(capi, g, family, 3)
    eps = st.do_time_steps(4, np.linspace(0.3, 0.6, 4), per_step_energies=True)
    assert eps.shape == (3, 4) and np.isfinite(eps).all()
    return [st]


def _strip(capi, g, family):
    """Halo granules, error word and snapshot of the strip kernel; the mailboxes and final counters of its in-kernel ladder."""
    st = _states(capi, g, family, 8)
    st.do_time_steps(3, np.linspace(0.3, 0.6, 3), per_step_energies=True)
    st.do_time_steps(2, 0.4407)
    _ladder_round_trip(st, 8, 7)
    st.pt_detach()
    st.do_time_steps(2, 0.4407)
    return [st]


FEATURES = {"append": _append, "betas": _betas, "ladder": _ladder, "cluster": _cluster, "icm_inside": _icm_inside,
            "icm_between": _icm_between, "track_best": _track_best, "pa_resample": _pa_resample, "sampling": _sampling,
            "step_energies": _step_energies, "strip": _strip}
PLAIN = ["append", "betas", "sampling", "step_energies"]   # what every family offers
MOVES = ["ladder", "icm_inside", "icm_between", "track_best", "pa_resample"]
CASES = ([("glass", f) for f in PLAIN + MOVES] + [("board", f) for f in ("cluster", "append")] + [("strip", "strip")] +
         [(spec, f) for spec in ("field", "open", "lattice16", "csr") for f in PLAIN] +
         [("packed", f) for f in PLAIN + MOVES + ["cluster"]] + [("real", f) for f in PLAIN + MOVES])


def _live(capi):
    gc.collect()   # containers of earlier tests that wait in a reference cycle go now, not between the two readings
    return capi.debug_live_blocks()


@pytest.mark.parametrize("spec,feature", CASES, ids=[f"{s}-{f}" for s, f in CASES])
def test_every_block_comes_back(capi, exact, monkeypatch, spec, feature):
    before = _live(capi)
    g, family = _graph(spec, capi, exact, monkeypatch)
    containers = FEATURES[feature](capi, g, family)
    held = capi.debug_live_blocks()
    assert held[0] > before[0], "no device block is counted: is the allocation cache switched off?"
    if feature == "sampling":
        assert held[1] > before[1], "the sampling pipeline holds pinned blocks"
    for st in containers:
        st.close()
    g.close()
    del containers, g
    assert _live(capi) == before


def test_twenty_ladders_on_one_container(capi, exact, monkeypatch):
    before = _live(capi)
    g, family = _graph("glass", capi, exact, monkeypatch)
    st = _states(capi, g, family, 8)
    after_detach = []
    for k in range(20):
        _ladder_round_trip(st, 8, 100 + k)
        st.pt_detach()
        after_detach.append(capi.debug_live_blocks())
    assert after_detach[-1] == after_detach[0] and len(set(after_detach)) == 1
    st.close()
    g.close()
    assert _live(capi) == before

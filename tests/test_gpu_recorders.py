"""The four periodic recorders of the step loop together -- minimum tracking, moment sums (S18), the overlap series
(S21) and the observable series (S22): all of them on one container against each of them alone, what isingmc_states_set_timestep
restarts, who refuses replicas to come and go while a recorder is on, the repeat of a call after a strip launch gave up with
recorders switched on, and a ladder call whose periodic overlap series would run full."""
import numpy as np
import pytest

import packed_icm_reference as IR

pytestmark = pytest.mark.gpu

BETA = 0.44
ALL = ("best", "moments", "overlaps", "observables")


def _ferromagnet(capi, exact, W=64, H=16):
    return capi.Graph(*exact.square_lattice_edges(W, H, -1.0))


def _switch_on(st, which, periods, capacity=16):
    """The recorders named in `which` with their periods; the two series come back (None where off)."""
    osr = obs = None
    if "best" in which:
        st.set_track_best(periods["best"])
    if "moments" in which:
        st.set_moments_every(periods["moments"])
    if "overlaps" in which:
        osr = st.overlap_series(capacity=capacity)
        osr.set_every(periods["overlaps"])
    if "observables" in which:
        obs = st.observable_series(capacity=capacity)
        obs.set_every(periods["observables"])
    return osr, obs


def _equal(a, b):
    """Tuples of arrays, scalars and None, bit for bit (float64 on its bits)."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if x is None or y is None:
            assert x is None and y is None
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape
            assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y)
        else:
            assert x == y


# ---- (a) all four at once against one at a time -------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["checkerboard", "packed_bitsliced"])
def test_all_recorders_at_once_equal_each_alone(capi, exact, monkeypatch, family):
    """Minimum tracking every 2, moment sums every 3, an overlap series every 2 and an observable series every 5, switched on at
    t = 0, over calls of 11 and 4 timesteps: what each recorder holds does not depend on the other three, and none of them changes
    the configurations.  A 64 x 16 ferromagnet and the 6^3 +-J cube on forced replica lanes, 8 replicas each."""
    if family == "checkerboard":
        g = _ferromagnet(capi, exact)
    else:
        monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
        g = capi.Graph(*IR.cubic_glass(exact, 6), nvars=216, force_general=True)
    seeds = capi.make_seeds(900, 8)
    periods = dict(best=2, moments=3, overlaps=2, observables=5)

    def run(which):
        st = capi.States(g, seeds)
        assert st.family == family
        osr, obs = _switch_on(st, which, periods)
        st.do_time_steps(11, BETA)
        st.do_time_steps(4, BETA)
        return st, osr, obs

    A, A_osr, A_obs = run(ALL)
    plain = run(())[0]
    assert np.array_equal(A.packed(), plain.packed()) and np.array_equal(A.raw_state(), plain.raw_state())
    assert np.array_equal(A.states(), plain.states())
    B, _, _ = run(("best",))
    e, s, t, n = A.best()
    assert n > 0 and set(t.tolist()) <= {2, 4, 6, 8, 10, 12, 14}
    _equal(A.best(), B.best())
    B, _, _ = run(("moments",))
    assert A.moments()[0] == 5                       # 3, 6, 9, 12, 15
    _equal(A.moments(), B.moments())
    B, B_osr, _ = run(("overlaps",))
    assert A_osr.get()[0].tolist() == [2, 4, 6, 8, 10, 12, 14]
    _equal(A_osr.get(), B_osr.get())
    B, _, B_obs = run(("observables",))
    assert A_obs.get()[0].tolist() == [5, 10, 15]
    _equal(A_obs.get(), B_obs.get())


# ---- (b) set_timestep and the refusals ----------------------------------------------------------------------------------------------
def test_set_timestep_restarts_all_but_minimum_tracking(capi, exact):
    """All four with period 3, then the clock goes to 100: the sample points of the moment sums and of both series are counted
    from 100 (103, 106), those of minimum tracking stay the multiples of 3 (102, 105).  The twin takes the same samples by hand."""
    g = _ferromagnet(capi, exact)
    seeds = capi.make_seeds(901, 8)
    st, twin = capi.States(g, seeds), capi.States(g, seeds)
    osr, obs = _switch_on(st, ALL, dict(best=3, moments=3, overlaps=3, observables=3))
    st.timestep = 100
    twin.timestep = 100
    st.do_time_steps(6, BETA)
    for _ in range(2):
        twin.do_time_steps(2, BETA)
        twin.best_update()                            # 102, 105
        twin.do_time_steps(1, BETA)
        twin.accumulate_moments()                     # 103, 106
    assert st.timestep == twin.timestep == 106
    assert osr.get()[0].tolist() == [103, 106] and obs.get()[0].tolist() == [103, 106]
    e, _, t, n = st.best()
    assert n > 0 and set(t.tolist()) <= {102, 105}
    _equal(st.best(), twin.best())
    assert st.moments()[0] == 2
    _equal(st.moments(), twin.moments())
    assert np.array_equal(st.packed(), twin.packed())


APPEND_SENTENCE = dict(best="minimum tracking is switched on", moments="moment sums are switched on",
                       overlaps="an overlap series records on a period", observables="an observable series records on a period")


def test_refusals_while_a_recorder_is_on(capi, exact):
    """Appending a replica is refused with each recorder's own sentence, a resampling (both population-annealing entry points) with
    those of the three recorders that follow replicas; where several are on, the first in the order best, moments, overlap
    series, observable series speaks."""
    g = _ferromagnet(capi, exact)
    seeds = capi.make_seeds(902, 8)
    periods = dict(best=2, moments=2, overlaps=2, observables=2)

    def refused(which, sentence, pa_sentence):
        st = capi.States(g, seeds)
        series = _switch_on(st, which, periods)
        with pytest.raises(ValueError, match=sentence + ".*after the graphs are added"):
            st.append(5)
        if pa_sentence:
            with pytest.raises(ValueError, match=pa_sentence + ".*a resampling replaces"):
                st.pa_resample(0.1, 1, 1)
            with pytest.raises(ValueError, match=pa_sentence + ".*a resampling replaces"):
                st.pa_run([0.1, 0.2], 1, 1)
        assert st.count == 8 and st.timestep == 0
        del series

    for name in ALL:
        refused((name,), APPEND_SENTENCE[name], None if name == "best" else APPEND_SENTENCE[name])
    refused(("overlaps", "observables"), APPEND_SENTENCE["overlaps"], APPEND_SENTENCE["overlaps"])
    refused(ALL, APPEND_SENTENCE["best"], APPEND_SENTENCE["moments"])
    # minimum tracking alone does not keep a population from being resampled
    st = capi.States(g, seeds)
    st.set_track_best(2)
    st.pa_resample(0.1, 1, 1)
    assert st.pa_run([0.1, 0.2], 1, 1)["sum"].shape == (1,)


# ---- (c) the strip retry with recorders on ------------------------------------------------------------------------------------------
def test_strip_retry_takes_no_sample_twice(capi, exact, monkeypatch):
    """The shape of test_strip_timeout_is_recovered with moment sums and an overlap series every 4 and an observable series every 2
    switched on, against the per-colour launches.  The hook fails the object's first strip launch.  To make the replay guard
    matter, a sample must precede that launch inside the call that is repeated: Swendsen-Wang steps every 4 (timesteps 3, 7,
    ...) and three calls of one timestep, which never launch strips, bring the clock to 3; the call of 6 timesteps then starts
    with the cluster step (no strip launch), takes the samples of all three recorders at t = 4, and only then launches its first
    strips for the stretch 4 .. 6.  The sample point t = 6 waits for that launch, finds it failed and the call is repeated from
    t = 3: without the guard the repeat would add the sample at t = 4 to the sums and to both logs a second time."""
    W, H, R = 1024, 256, 12
    g = _ferromagnet(capi, exact, W, H)
    seeds = capi.make_seeds(21, R)

    def run(strip, hook):
        monkeypatch.setenv("ISINGMC_STRIP", strip)
        monkeypatch.setenv("ISINGMC_STRIP_TEST_FAIL_ONCE", hook)
        st = capi.States(g, seeds)
        st.set_cluster_every(4)
        osr, obs = _switch_on(st, ("moments", "overlaps", "observables"), dict(moments=4, overlaps=4, observables=2), capacity=8)
        for _ in range(3):
            st.do_time_steps(1, 0.45)
        st.do_time_steps(6, 0.45)
        assert st.timestep == 9
        return st, osr, obs

    ref, ref_osr, ref_obs = run("0", "0")
    st, osr, obs = run("1", "1")
    assert st.moments()[0] == 2
    _equal(st.moments(), ref.moments())
    assert osr.get()[0].tolist() == [4, 8] and obs.get()[0].tolist() == [2, 4, 6, 8]
    _equal(osr.get(), ref_osr.get())
    _equal(obs.get(), ref_obs.get())
    assert np.array_equal(st.packed(), ref.packed())


# ---- (d) a ladder call and a full overlap series ------------------------------------------------------------------------------------
def test_pt_run_refuses_a_full_overlap_series_before_any_round(capi, exact):
    """A ladder of 4 rungs with a periodic overlap series of capacity 1 and period 2: pt_run(4, 2) would take two rows.  The call
    is refused before its first round is enqueued -- clock, planes and permutation are as they were, the log is empty."""
    g = _ferromagnet(capi, exact)
    st = capi.States(g, capi.make_seeds(903, 4))
    st.pt_attach(np.linspace(0.3, 0.6, 4), 0, 4, 1, 77)
    st.pt_run(3, 1)                                   # a permutation that is not the identity any more, most likely
    osr = st.overlap_series(capacity=1)
    osr.set_every(2)
    t0, planes, perm = st.timestep, st.packed(), st.pt_state()
    with pytest.raises(ValueError, match="would run full: the call takes 2 samples and the log has room for 1 of its 1"):
        st.pt_run(4, 2)
    assert st.timestep == t0 == 3 and osr.count == 0
    assert np.array_equal(st.packed(), planes)
    after = st.pt_state()
    assert np.array_equal(after[0], perm[0]) and after[1:] == perm[1:]
    st.pt_run(2, 2)                                   # what fits still runs
    assert osr.get()[0].tolist() == [5]

"""The step chooser of population annealing on the device: isingmc_pa_choose_step against the restatement of
tests/pa_adaptive_reference.py applied to the energies the library returns (k, the bits of dbeta, S, N), on the three served
families and across the workgroup, grid-stride and 2^64 borders; that a choice reads only; isingmc_pa_run_adaptive against the
blocking loop and against isingmc_pa_run on the schedule it took; and Lattice.run_population_annealing_adaptive against Kaufman's
exact partition function."""
import struct
from fractions import Fraction

import numpy as np
import pytest

import pa_adaptive_reference as PAA
import packed_icm_reference as IR

pytestmark = pytest.mark.gpu

SEED = 0x0123456789ABCDEF
TARGET = 0.85
FAMILIES = ("board", "cubic", "real")


def _bits(x):
    return struct.pack("<d", float(x))


def _container(capi, exact, monkeypatch, family, R, seed_gen=21):
    """A population on the 64 x 16 torus (checkerboard), the 4^3 +-J cubic lattice (bit-sliced) or the 64 x 8 lattice with Gaussian
    couplings and fields (real-coupling), built as tests/test_gpu_population_annealing.py builds them."""
    seeds = capi.make_seeds(seed_gen, R)
    if family == "board":
        ea, eb, ej = exact.square_lattice_edges(64, 16, -1.0)
        st = capi.States(capi.Graph(ea, eb, ej, device=0), seeds)
        assert st.family == "checkerboard"
        return st
    monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
    if family == "cubic":
        ea, eb, ej = IR.cubic_glass(exact, 4)
        st = capi.States(capi.Graph(ea, eb, ej, nvars=64, force_general=True), seeds)
        assert st.family == "packed_bitsliced"
        return st
    ea, eb, _ = exact.square_lattice_edges(64, 8, -1.0)
    rng = np.random.default_rng(648)
    ej, h = rng.normal(size=len(ea)), rng.normal(size=512)
    st = capi.States(capi.Graph(ea, eb, ej, nvars=512, biases=h, stable_path=True), seeds)
    assert st.family == "packed_real"
    return st


def _compare(st, e, dbeta_max, target=TARGET):
    want = PAA.choose_step(e, dbeta_max, target)
    got = st.pa_choose_step(dbeta_max, target)
    assert got["k"] == want["k"], (got, {k: want[k] for k in ("k", "dbeta", "sum", "num")})
    assert _bits(got["dbeta"]) == _bits(want["dbeta"])
    assert got["sum"] == want["sum"]
    assert got["num"] & (2 ** 64 - 1) == want["num"] & (2 ** 64 - 1) and got["num"] >> 64 == want["num"] >> 64
    return want


def _three_steps(e):
    """dbeta_max that the whole of holds / that is cut inside the grid / whose 65536th part is already too large, from the
    spread of the energies: the overlap of two temperatures falls to the target where dbeta is a fraction of 1 / spread."""
    spread = float(e.max() - e.min()) or 1.0
    return 1e-3 / spread, 8.0 / spread, 1e7 / spread


@pytest.mark.parametrize("R", (1, 33, 257, 1025, 4099))
@pytest.mark.parametrize("family", FAMILIES)
def test_choice_equals_the_restatement(capi, exact, monkeypatch, family, R):
    st = _container(capi, exact, monkeypatch, family, R)
    st.do_time_steps(3, 0.1)
    e = st.energies()
    ks = [_compare(st, e, dbeta_max)["k"] for dbeta_max in _three_steps(e)]
    print(f"{family} R {R}: k = {ks}")
    if R == 1:
        assert ks == [65536] * 3   # one replica overlaps with itself
    else:
        assert ks[0] == 65536 and 1 < ks[1] < 65536 and ks[2] == 1
    assert np.array_equal(st.energies(), e)


@pytest.mark.parametrize("family", FAMILIES)
def test_a_degenerate_population_takes_the_whole_step(capi, exact, monkeypatch, family):
    R = 70
    st = _container(capi, exact, monkeypatch, family, R)
    st.do_time_steps(2, 0.1)
    st.pa_apply_sources(np.zeros(R, dtype=np.uint32))   # every slot holds the configuration of slot 0
    e = st.energies()
    assert (e == e[0]).all()
    for dbeta_max in (1e-3, 0.7, 1e6):
        want = _compare(st, e, dbeta_max)
        assert want["k"] == 65536 and want["dbeta"] == dbeta_max and want["sum"] == R << 32 and want["num"] == R * (R << 32)


def test_the_numerator_carries_into_its_high_word(capi, exact, monkeypatch):
    """2^17 + 33 replicas on the 4^3 lattice: 513 workgroups of 256 (the last one with 33 live threads) below the grid cap, so
    every thread holds at most one element; N is about R S ~ 2^66."""
    R = (1 << 17) + 33
    st = _container(capi, exact, monkeypatch, "cubic", R)
    st.do_time_steps(2, 0.1)
    e = st.energies()
    for dbeta_max in _three_steps(e)[:2]:
        want = _compare(st, e, dbeta_max)
        highs = [c["num"] >> 64 for c in want["evaluated"]]
        print(f"dbeta_max {dbeta_max:.3e}: k {want['k']}, {sum(h != 0 for h in highs)} of {len(highs)} evaluated candidates with a high word")
        assert any(h != 0 for h in highs)


def test_a_population_beyond_the_grid_cap(capi, exact, monkeypatch):
    """2048 workgroups of 256 threads cover 2^19 elements: at 2^19 + 2^18 + 77 replicas the threads of the first workgroups walk
    two elements, the others one."""
    R = (1 << 19) + (1 << 18) + 77
    st = _container(capi, exact, monkeypatch, "cubic", R)
    st.do_time_steps(1, 0.1)
    e = st.energies()
    _compare(st, e, _three_steps(e)[1])


def _observe(st):
    return dict(raw=st.raw_state(), e=st.energies(), t=st.timestep, fam=st.pa_families(), last=st.pa_last())


def _same(a, b):
    assert np.array_equal(a["raw"], b["raw"]) and np.array_equal(a["e"], b["e"]) and a["t"] == b["t"]
    assert np.array_equal(a["fam"], b["fam"])
    for name in ("sum", "eref", "distinct", "mean_energy"):
        assert a["last"][name] == b["last"][name], name
    assert np.array_equal(a["last"]["src"], b["last"]["src"])


@pytest.mark.parametrize("family", FAMILIES)
def test_a_choice_reads_only_and_agrees_with_the_resampling(capi, exact, monkeypatch, family):
    R = 257
    P, Q = (_container(capi, exact, monkeypatch, family, R) for _ in range(2))
    for st in (P, Q):
        st.do_time_steps(3, 0.1)
        st.pa_resample(0.01, SEED, 1)   # a record and families that are not the identity
        st.do_time_steps(2, 0.11)
    before = _observe(P)
    e = before["e"]
    choice = P.pa_choose_step(_three_steps(e)[1], TARGET)
    P.pa_choose_step(_three_steps(e)[0], 0.5)   # (a second search reuses the chooser's blocks)
    _same(_observe(P), before)
    _same(_observe(P), _observe(Q))
    for st in (P, Q):   # the twin never chose: both continue alike, and the resampling forms the chooser's weights
        st.pa_resample(choice["dbeta"], SEED, 2)
        st.do_time_steps(2, 0.11 + choice["dbeta"])
    _same(_observe(P), _observe(Q))
    assert 1 < choice["k"] < 65536
    assert P.pa_last()["sum"] == choice["sum"]


# beta_start, beta_end and the cap are dyadic and the cap is a power of two near the steps the rule takes here, so every chosen
# dbeta and every beta + dbeta is exact in f64 (multiples of 2^-54 below 1/2) and betas[k] - betas[k-1] gives the dbeta back: the
# condition under which isingmc_pa_run on the reported schedule repeats the run.  The test checks that condition before it uses it.
ADAPTIVE = {"board": (0.0, 0.25, 2.0 ** -6), "cubic": (0.0, 0.25, 2.0 ** -5), "real": (0.0, 0.25, 2.0 ** -6)}
SWEEPS = 2


def _blocking_loop(st, b0, b1, cap, max_steps=10 ** 6):
    """the loop the header states, with blocking calls: (betas, choices, records)"""
    beta, betas, choices, recs = b0, [b0], [], []
    st.do_time_steps(SWEEPS, beta)
    while beta < b1 and len(choices) < max_steps:
        dbeta_max = min(cap, b1 - beta)
        c = st.pa_choose_step(dbeta_max, TARGET)
        reaches = not (cap < b1 - beta) or beta + dbeta_max >= b1
        beta = b1 if c["k"] == 65536 and reaches else beta + c["dbeta"]
        choices.append(c)
        st.pa_resample(c["dbeta"], SEED, len(choices))
        recs.append(st.pa_last())
        st.do_time_steps(SWEEPS, beta)
        betas.append(beta)
    return np.array(betas), choices, recs


def _records_equal(log, recs):
    for name in ("sum", "eref", "distinct", "mean_energy"):
        assert np.array_equal(log[name], [r[name] for r in recs]), name


@pytest.mark.parametrize("family", FAMILIES)
def test_adaptive_run_equals_the_blocking_loop_and_replays(capi, exact, monkeypatch, family):
    R = 257
    b0, b1, cap = ADAPTIVE[family]
    P, Q, Z = (_container(capi, exact, monkeypatch, family, R) for _ in range(3))
    log = P.pa_run_adaptive(b0, b1, SWEEPS, SEED, TARGET, dbeta_cap=cap)
    betas, choices, recs = _blocking_loop(Q, b0, b1, cap)
    ks = [c["k"] for c in choices]
    print(f"{family}: {len(ks)} steps, k = {ks}")
    assert any(1 < k < 65536 for k in ks), "no step was cut by the rule: choose a larger cap"
    assert log["betas"].tobytes() == betas.tobytes() and betas[0] == b0 and betas[-1] == b1
    _records_equal(log, recs)
    assert [r["sum"] for r in recs] == [c["sum"] for c in choices]
    assert P.timestep == Q.timestep == SWEEPS * len(betas)
    assert np.array_equal(P.raw_state(), Q.raw_state()) and np.array_equal(P.pa_families(), Q.pa_families())
    _same(_observe(P), _observe(Q))
    for c in choices:   # a step the rule cut kept the overlap it promises
        if c["k"] < 65536:
            assert TARGET <= Fraction(c["num"], R * c["sum"]) <= 1
    # the schedule that was taken, as a fixed one
    assert all(betas[k + 1] - betas[k] == c["dbeta"] for k, c in enumerate(choices)), "the parameters do not keep the arithmetic exact"
    fixed = Z.pa_run(betas, SWEEPS, SEED)
    _records_equal(fixed, recs)
    assert np.array_equal(Z.raw_state(), P.raw_state()) and np.array_equal(Z.pa_families(), P.pa_families())


def test_max_steps_that_do_not_reach_the_end(capi, exact, monkeypatch):
    R = 257
    b0, b1, cap = ADAPTIVE["board"]
    P, Q = (_container(capi, exact, monkeypatch, "board", R) for _ in range(2))
    with pytest.raises(ValueError, match="max_steps") as err:
        P.pa_run_adaptive(b0, b1, SWEEPS, SEED, TARGET, dbeta_cap=cap, max_steps=3)
    betas, _, recs = _blocking_loop(Q, b0, b1, cap, max_steps=3)
    part = err.value.partial
    assert len(betas) == 4 and betas[-1] < b1
    assert part["betas"].tobytes() == betas.tobytes()
    _records_equal(part, recs)
    _same(_observe(P), _observe(Q))


def test_refusals_leave_the_container_untouched(capi, exact, monkeypatch):
    st = _container(capi, exact, monkeypatch, "board", 33)
    st.do_time_steps(2, 0.2)
    st.pa_resample(0.01, SEED, 1)
    before = _observe(st)
    for dbeta_max in (0.0, -0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="dbeta_max"):
            st.pa_choose_step(dbeta_max, TARGET)
    for target in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="target"):
            st.pa_choose_step(0.1, target)
        with pytest.raises(ValueError, match="target"):
            st.pa_run_adaptive(0.0, 0.1, 1, SEED, target)
    with pytest.raises(ValueError, match="beta_start"):
        st.pa_run_adaptive(0.2, 0.1, 1, SEED, TARGET)
    with pytest.raises(ValueError, match="dbeta_cap"):
        st.pa_run_adaptive(0.1, 0.2, 1, SEED, TARGET, dbeta_cap=0.0)
    st.set_betas(np.full(33, 0.2))   # an obstacle of pa_obstacle: a population shares one beta
    with pytest.raises(ValueError, match="per-replica betas"):
        st.pa_choose_step(0.1, TARGET)
    with pytest.raises(ValueError, match="per-replica betas"):
        st.pa_run_adaptive(0.1, 0.2, 1, SEED, TARGET)
    _same(_observe(st), before)


# ---- physics and the Python entry point ------------------------------------------------------------------------------------
PA_W, PA_H, PA_POP, PA_SWEEPS = 64, 16, 1024, 4
PA_SEED_GENS = (101, 202, 303, 404, 505, 606, 707, 808)


def _lattice(exact, seed_gen):
    import py_monte_carlo
    ea, eb, ej = exact.square_lattice_edges(PA_W, PA_H, -1.0)
    return py_monte_carlo.Lattice.from_arrays(ea, eb, ej, seed_gen=seed_gen)


def test_free_energy_of_the_adaptive_schedule_against_kaufman(capi, exact):
    """The adaptive schedule from 0 to 0.3 on the 64 x 16 torus over eight seeds: N ln 2 + log_z_ratio[-1] against the exact
    ln Z(0.3) and the final mean energy against the exact energy, both within 4 standard errors of the eight runs (the bound of
    test_free_energy_against_kaufman); then one schedule through the C ABI: every step the rule cut kept an overlap in [target, 1]."""
    N = PA_W * PA_H
    runs = [_lattice(exact, sg).run_population_annealing_adaptive(0.0, 0.3, PA_SWEEPS, PA_POP, return_states=False) for sg in PA_SEED_GENS]
    lnz = np.array([N * np.log(2.0) + r.log_z_ratio[-1] for r in runs])
    want = exact.kaufman_lnZ(PA_W, PA_H, 0.3)
    std = lnz.std(ddof=1)
    print(f"ln Z {lnz.mean():.4f} +- {std / np.sqrt(8):.4f} (std {std:.4f}) exact {want:.4f}; steps {[len(r.betas) - 1 for r in runs]}")
    assert abs(lnz.mean() - want) <= 4 * std / np.sqrt(8)
    e = np.array([r.mean_energy[-1] for r in runs])
    e_want = exact.kaufman_energy(PA_W, PA_H, 0.3)
    print(f"<E> {e.mean():.3f} +- {e.std(ddof=1) / np.sqrt(8):.3f} exact {e_want:.3f}")
    assert abs(e.mean() - e_want) <= 4 * e.std(ddof=1) / np.sqrt(8)
    ea, eb, ej = exact.square_lattice_edges(PA_W, PA_H, -1.0)
    st = capi.States(capi.Graph(ea, eb, ej, device=0), capi.make_seeds(101, PA_POP))
    beta, cut = 0.0, 0
    st.do_time_steps(PA_SWEEPS, beta)
    for step in range(1, 200):
        c = st.pa_choose_step(0.3 - beta, 0.85)
        if c["k"] == 65536:
            break
        cut += 1
        assert 0.85 <= Fraction(c["num"], PA_POP * c["sum"]) <= 1
        beta += c["dbeta"]
        st.pa_resample(c["dbeta"], SEED, step)
        st.do_time_steps(PA_SWEEPS, beta)
    assert cut >= 5 and c["k"] == 65536


def test_python_result_and_refusals(exact):
    lat = _lattice(exact, 42)
    r = lat.run_population_annealing_adaptive(0.05, 0.3, 2, 256)
    n = len(r.betas)
    assert n >= 3 and r.betas[0] == 0.05 and r.betas[-1] == 0.3 and (np.diff(r.betas) > 0).all()
    assert r.log_z_ratio.shape == (n,) and r.mean_energy.shape == (n,) and r.distinct_sources.shape == (n - 1,)
    assert r.log_z_ratio[0] == 0.0 and (r.distinct_sources <= 256).all() and (r.distinct_sources >= 1).all()
    assert r.energies.shape == (256,) and r.states.shape == (256, PA_W * PA_H) and r.families.shape == (256,) and r.rho_t >= 1.0
    again = _lattice(exact, 42).run_population_annealing_adaptive(0.05, 0.3, 2, 256)
    for name in ("betas", "energies", "states", "log_z_ratio", "mean_energy", "distinct_sources", "families"):
        assert np.array_equal(getattr(r, name), getattr(again, name)), name
    capped = _lattice(exact, 42).run_population_annealing_adaptive(0.05, 0.3, 2, 256, max_dbeta=0.004)
    assert np.diff(capped.betas).max() <= 0.004 * (1 + 1e-12) and len(capped.betas) > n
    loose = _lattice(exact, 42).run_population_annealing_adaptive(0.05, 0.3, 2, 256, target_overlap=0.5, track_minimum=True, measure_overlaps=True)
    assert len(loose.betas) < n and loose.min_energy <= loose.energies.min() and loose.spin_overlaps.shape == (128,)
    one = lat.run_population_annealing_adaptive(0.2, 0.2, 1, 4)   # nowhere to go: no resampling at all
    assert one.betas.tolist() == [0.2] and one.log_z_ratio.tolist() == [0.0] and one.distinct_sources.shape == (0,)
    for kw in (dict(target_overlap=0.0), dict(target_overlap=1.5), dict(max_dbeta=0.0), dict(max_dbeta=-1.0), dict(max_steps=1)):
        with pytest.raises(ValueError):
            lat.run_population_annealing_adaptive(0.05, 0.3, 2, 16, **kw)
    for b0, b1, sweeps, pop in ((0.3, 0.1, 1, 4), (float("nan"), 0.1, 1, 4), (0.1, 0.2, 0, 4), (0.1, 0.2, 1, 0)):
        with pytest.raises(ValueError):
            lat.run_population_annealing_adaptive(b0, b1, sweeps, pop)
    with pytest.raises(ValueError, match="needs measure_overlaps"):
        lat.run_population_annealing_adaptive(0.1, 0.2, 1, 4, overlap_classes=np.zeros(PA_W * PA_H, dtype=np.uint32))
    lat.set_devices([0, 0])
    with pytest.raises(ValueError, match="one device"):
        lat.run_population_annealing_adaptive(0.1, 0.2, 1, 4)
    lat.set_devices([0])
    lat.set_global_bias(0.5)
    with pytest.raises(ValueError):   # a field: no family this graph can run on is served
        lat.run_population_annealing_adaptive(0.1, 0.2, 1, 4)

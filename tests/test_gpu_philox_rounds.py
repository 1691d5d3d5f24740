"""The option "philox_rounds" = 7 on every kernel that draws the sweeps of the periodic, field-free, one-|J|
checkerboard lattices, bit for bit against tests/philox_rounds_reference.py (pinned at ten rounds by
tests/test_philox_rounds_host.py): one test per kernel on the shapes that force it (tests/lat_variants_reference.py,
tests/strip_ladder_reference.py), three couplings, uniform then per-replica betas; the ladder inside the strip launch against a
twin driven call by call; switching between the round counts; the default untouched; the refusals; the Python surface; and the
exact finite-torus energy as the physics control of both round counts.  No number in this module is a tolerance but the sigma
rule of the Kaufman check, which is the one tests/test_gpu_moments.py uses on the same torus."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lat_variants_reference as LV
import mc_variants_reference as MV
import philox_rounds_reference as PR
import strip_ladder_reference as SL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUPLINGS = pytest.mark.parametrize("coupling", LV.COUPLINGS)
STREAM = dict(LV.STREAM)                                   # disable_resident, strip off, one quad per thread
N_UNIFORM, N_REPLICA = len(PR.UNIFORM), len(PR.PER_REPLICA)


def _container(capi, shape, coupling, seeds, options, rounds=7):
    case = LV.make_case(shape[0], shape[1], coupling)
    g = capi.Graph(case.ea, case.eb, case.ej)
    assert g.kind == capi.KIND_LATTICE2D
    st = capi.States(g, seeds)
    assert st.family == "checkerboard" and st.philox_rounds == 10
    for name, value in options.items():
        st.set_option(name, value)
    if rounds is not None:
        st.set_option("philox_rounds", rounds)
        assert st.philox_rounds == rounds
    return case, st


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _check_case(capi, oracle, group, shape, coupling, options, per_step=False):
    """UNIFORM in one call, then PER_REPLICA under per-replica betas: configurations (and energies) against the reference"""
    seeds = PR.case_seeds(group, coupling)
    traj = PR.case_run(oracle, group, shape, coupling)
    case, st = _container(capi, shape, coupling, seeds, options)
    assert np.array_equal(st.packed(), traj.start)       # the initial configurations are ten rounds whatever the option says
    e = st.do_time_steps(N_UNIFORM, np.array(PR.UNIFORM), per_step_energies=per_step)
    assert np.array_equal(st.packed(), traj.steps[N_UNIFORM - 1].words)
    assert np.array_equal(_bits(st.energies()), _bits(PR.energies(case, traj.steps[N_UNIFORM - 1].words)))
    if per_step:
        for k in range(N_UNIFORM):
            assert np.array_equal(_bits(e[:, k]), _bits(PR.energies(case, traj.steps[k].words))), k
    st.set_betas(PR.PER_REPLICA[0])
    e = st.do_time_steps(N_REPLICA, per_step_energies=per_step)
    assert np.array_equal(st.packed(), traj.steps[-1].words)
    if per_step:
        for k in range(N_REPLICA):
            assert np.array_equal(_bits(e[:, k]), _bits(PR.energies(case, traj.steps[N_UNIFORM + k].words))), k
    assert st.timestep == N_UNIFORM + N_REPLICA and st.philox_rounds == 7
    return st


# ---- one test per kernel ---------------------------------------------------------------------------------------------------------
@COUPLINGS
@pytest.mark.parametrize("shape", PR.GROUPS["resident"], ids=lambda s: f"{s[0]}x{s[1]}")
def test_lat_resident_kernel(capi, oracle, shape, coupling):
    _check_case(capi, oracle, "resident", shape, coupling, {"resident_spread": 0})
    _check_case(capi, oracle, "resident", shape, coupling, {"resident_spread": 0}, per_step=True)


@COUPLINGS
@pytest.mark.parametrize("lpq", [8, 4, 2])
@pytest.mark.parametrize("shape", PR.GROUPS["resident"], ids=lambda s: f"{s[0]}x{s[1]}")
def test_lat_resident_spread_kernel(capi, oracle, shape, lpq, coupling):
    options = {"resident_spread": 2, "resident_lpq": 0 if lpq == 8 else lpq}
    assert LV.resident_launch(shape[0], shape[1], options)[:2] == (True, lpq)
    _check_case(capi, oracle, "resident", shape, coupling, options)
    _check_case(capi, oracle, "resident", shape, coupling, options, per_step=True)


@COUPLINGS
@pytest.mark.parametrize("shape", PR.GROUPS["stream"], ids=lambda s: f"{s[0]}x{s[1]}")
def test_lat_sweep_kernel(capi, oracle, shape, coupling):
    assert LV.by_name(LV.FUSED, f"{shape[0]}x{shape[1]}").options == LV.STREAM
    _check_case(capi, oracle, "stream", shape, coupling, STREAM)


@COUPLINGS
@pytest.mark.parametrize("iters", [2, 4])
def test_lat_sweep_loop_kernel(capi, oracle, iters, coupling):
    """512 x 512: 1024 quads in rows of two -- 2 and 4 quads per thread fit (nquads % (256 k) == 0, H % (2 k) == 0), 8 do not"""
    (shape,) = PR.GROUPS["loop"]
    nquads = MV.geometry(*shape)[2]
    assert LV.uni(*shape) and nquads % (256 * 4) == 0 and nquads % (256 * 8) != 0
    _check_case(capi, oracle, "loop", shape, coupling, dict(STREAM, sweep_iters=iters))


@COUPLINGS
@pytest.mark.parametrize("shape", PR.GROUPS["stream"], ids=lambda s: f"{s[0]}x{s[1]}")
def test_lat_sweep_measure_kernel(capi, oracle, shape, coupling):
    _check_case(capi, oracle, "stream", shape, coupling, STREAM, per_step=True)


@COUPLINGS
@pytest.mark.parametrize("nw", [1, 4])
def test_lat_strip_kernel(capi, oracle, nw, coupling):
    shape = PR.GROUPS["strip"][0 if nw == 1 else 1]
    assert SL.strip_plan(shape[0], shape[1], nw)[2] == 2    # the smallest two-strip geometry of that NW
    options = {"disable_resident": 1, "strip": 1, "strip_nw": nw}
    _check_case(capi, oracle, "strip", shape, coupling, options)
    _check_case(capi, oracle, "strip", shape, coupling, options, per_step=True)


# ---- the strip kernel with a ladder ----------------------------------------------------------------------------------------------
LADDERS = [SL.BY_NAME["nw1-256x128-glass-2rungs-A"], SL.BY_NAME["nw4-8192x16-fm-2rungs-A"]]   # the smallest ladders with a pair, NW = 1 and 4


def _ladder(capi, case, in_kernel):
    g = capi.Graph(*SL.edges(case))
    st = capi.States(g, np.array(SL.twin(case).slot_seeds, dtype=np.uint64))
    for name, value in (("strip", 1), ("strip_nw", case.nw), ("pt_in_kernel", int(in_kernel)), ("philox_rounds", 7)):
        st.set_option(name, value)
    st.pt_attach(np.array(case.betas), 0, len(case.betas), 1, case.seed)
    st.pt_set_statistics(True)
    return st


@pytest.mark.parametrize("case", LADDERS, ids=[c.name for c in LADDERS])
def test_ladder_inside_the_strip_launch(capi, oracle, case):
    """pt_run at seven rounds against a twin driven call by call (pt_time_steps / pt_measure / pt_swap, pt_in_kernel = 0), whose
    sweeps of the first round are the reference's: the rounds inside the launch still draw their exchange words with ten rounds --
    the twin's come from pt_swap_kernel, which never sees the option."""
    inside, twin = _ladder(capi, case, True), _ladder(capi, case, False)
    G = len(case.betas)
    coupling = {"fm": "ferro", "afm": "antiferro"}.get(case.coupling)
    first = True
    for T, f in SL.calls(case):
        inside.pt_run(T, f)
        for _ in range(T // f):
            twin.pt_time_steps(f)
            if first and coupling:   # (the glass of the ladder cases is seeded otherwise than LV's: the uniform couplings carry this check)
                ref = PR.run(oracle, case.W, case.H, coupling, np.array(SL.twin(case).slot_seeds, dtype=np.uint64), [np.array(case.betas)] * f, 7)
                assert np.array_equal(twin.packed(), ref.steps[-1].words)
            first = False
            twin.pt_measure()
            twin.pt_swap()
        if T % f:
            twin.pt_time_steps(T % f)
        a, b = inside.pt_state(), twin.pt_state()
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
        assert np.array_equal(inside.packed(), twin.packed()) and inside.timestep == twin.timestep
    stats = inside.pt_statistics()
    assert stats["in_kernel_rounds"] == sum(T // f for T, f in SL.calls(case)) - 2 > 0 == twin.pt_statistics()["in_kernel_rounds"]
    assert G == 1 or stats["attempts"].sum() > 0


# ---- switching, the default, the refusals ---------------------------------------------------------------------------------------
@COUPLINGS
@pytest.mark.parametrize("options", [{}, STREAM], ids=["resident", "stream"])
def test_switching_between_the_round_counts(capi, oracle, options, coupling):
    shape, seeds = (256, 8), LV.SEEDS
    case, st = _container(capi, shape, coupling, seeds, options, rounds=None)
    ref = PR.run(oracle, shape[0], shape[1], coupling, seeds, [0.4407] * 9, [10] * 3 + [7] * 3 + [10] * 3)
    for k, rounds in enumerate((10, 7, 10)):
        st.set_option("philox_rounds", rounds)
        st.do_time_steps(3, 0.4407)
        assert np.array_equal(st.packed(), ref.steps[3 * k + 2].words), rounds
        assert st.timestep == 3 * (k + 1)
    lat = LV.oracle_lat(oracle, case)
    plain = PR.run(oracle, shape[0], shape[1], coupling, seeds, [0.4407] * 3, 10)
    assert np.array_equal(plain.steps[2].words, ref.steps[2].words) and not np.array_equal(plain.start, ref.steps[8].words)
    assert lat.energy_mag(ref.steps[8].words[0])[0] == st.energies()[0]


_CHILD = """
import sys, numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
from pyisingmontecarlo_amd import _capi
import lat_variants_reference as LV
case = LV.make_case(256, 8, "pmj")
st = _capi.States(_capi.Graph(case.ea, case.eb, case.ej), LV.SEEDS)
assert st.philox_rounds == 7
st.do_time_steps(3, 0.4407)
np.save(sys.argv[1], st.packed())
field = _capi.Graph(case.ea, case.eb, case.ej, nvars=256 * 8, biases=np.full(256 * 8, 0.25))
assert _capi.States(field, LV.SEEDS).philox_rounds == 10
"""


@COUPLINGS
def test_the_default_is_untouched(capi, oracle, coupling, tmp_path):
    """a container that sets 10 explicitly equals the C oracle, as one that never sets the option does (the existing suites);
    ISINGMC_PHILOX_ROUNDS=7 is read at creation -- in a fresh child process -- and only there"""
    shape, seeds = (256, 8), LV.SEEDS
    case, st = _container(capi, shape, coupling, seeds, {}, rounds=10)
    lat = LV.oracle_lat(oracle, case)
    st.do_time_steps(len(MV.BETAS), MV.BETAS)
    for r, seed in enumerate(seeds):
        ref = lat.init(seed)
        for t, beta in enumerate(MV.BETAS):
            lat.sweep(ref, seed, t, beta)
        assert np.array_equal(st.packed()[r], ref) and st.energies()[r] == lat.energy_mag(ref)[0]
    if coupling != "pmj":
        return
    out = str(tmp_path / "child.npy")
    env = dict(os.environ, ISINGMC_PHILOX_ROUNDS="7")
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    done = subprocess.run([sys.executable, "-c", code, out], env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    want = PR.run(oracle, 256, 8, "pmj", seeds, [0.4407] * 3, 7)
    assert np.array_equal(np.load(out), want.steps[2].words)
    assert _container(capi, shape, coupling, seeds, {}, rounds=None)[1].philox_rounds == 10   # this process never had the variable


def _unserved(capi, exact, monkeypatch, which):
    if which in ("field", "open", "aniso"):
        case = MV.make_case(256, 8, {"field": "field+", "open": "open_x", "aniso": "aniso"}[which], False)
        g = capi.Graph(case.ea, case.eb, case.ej, nvars=case.nvars, biases=case.biases)
        return g, "checkerboard"
    family = {"csr": "csr_f64", "packed": "packed_bitsliced", "real": "packed_real"}[which]
    for name in {"csr": ("DISABLE_REAL", "DISABLE_PACKED"), "packed": ("FORCE_PACKED",), "real": ("FORCE_REAL",)}[which]:
        monkeypatch.setenv("ISINGMC_" + name, "1")
    if which == "packed":   # a +-J cubic lattice
        ea, eb, ej = exact.cubic_lattice_edges(4, -1.0)
        ej = ej * np.random.default_rng(4).choice([-1.0, 1.0], size=len(ej))
        return capi.Graph(ea, eb, ej, nvars=64, force_general=True), family
    ea, eb, ej = exact.square_lattice_edges(20, 12, 1.0, np.random.default_rng(2012))
    if which == "real":
        ej = ej * np.random.default_rng(5).uniform(0.5, 1.5, size=len(ej))
    return capi.Graph(ea, eb, ej, nvars=240, force_general=True), family


@pytest.mark.parametrize("which", ["field", "open", "aniso", "packed", "real", "csr"])
def test_refusals(capi, exact, monkeypatch, which):
    g, family = _unserved(capi, exact, monkeypatch, which)
    seeds = capi.make_seeds(5, 33 if family.startswith("packed") else 3)
    st, twin = capi.States(g, seeds), capi.States(g, seeds)
    assert st.family == family and st.philox_rounds == 10
    for value in (7, 0, 8, 11):
        with pytest.raises(ValueError, match="philox_rounds|Philox"):
            st.set_option("philox_rounds", value)
        assert st.philox_rounds == 10
    st.set_option("philox_rounds", 10)
    st.do_time_steps(4, 0.5)
    twin.do_time_steps(4, 0.5)
    assert np.array_equal(st.states(), twin.states()) and np.array_equal(_bits(st.energies()), _bits(twin.energies()))


def test_other_values_are_refused_on_a_served_container(capi, oracle):
    _, st = _container(capi, (256, 8), "ferro", LV.SEEDS, {}, rounds=7)
    for value in (0, 8, 11, -7):
        with pytest.raises(ValueError, match="7 or 10"):
            st.set_option("philox_rounds", value)
        assert st.philox_rounds == 7


# ---- the Python surface ---------------------------------------------------------------------------------------------------------
def _edge_list(case):
    return [((int(a), int(b)), float(j)) for a, b, j in zip(case.ea, case.eb, case.ej)]


def test_lattice_set_rng_rounds(capi, oracle):
    import py_monte_carlo
    case = LV.make_case(256, 8, "pmj")
    lat = py_monte_carlo.Lattice(_edge_list(case), seed_gen=99)
    assert lat.engine_info()["rng_rounds"] == 10
    energies, states = lat.set_rng_rounds(7).run_monte_carlo(0.4407, 5, 3)
    assert lat.engine_info()["rng_rounds"] == 7
    seeds = np.array(lat.make_seeds(3), dtype=np.uint64)
    ref = PR.run(oracle, 256, 8, "pmj", seeds, [0.4407] * 5, 7)
    olat = LV.oracle_lat(oracle, case)
    for r in range(3):
        assert np.array_equal(states[r], olat.unpack(ref.steps[-1].words[r]).astype(bool))
        assert energies[r] == PR.energy(case, ref.steps[-1].words[r])
    with pytest.raises(ValueError):
        lat.set_rng_rounds(8)
    field = py_monte_carlo.Lattice(_edge_list(case))
    field.set_global_bias(0.25)
    with pytest.raises(ValueError, match="philox_rounds"):   # no run with ten rounds instead
        field.set_rng_rounds(7).run_monte_carlo(0.4407, 2, 2)
    field.set_rng_rounds(10).run_monte_carlo(0.4407, 2, 2)


def test_classic_ising_and_tempering_equal_their_states_level_twins(capi, oracle):
    import py_monte_carlo
    from pyisingmontecarlo_amd.tempering import ClassicalTempering
    case = LV.make_case(256, 8, "ferro")
    ci = py_monte_carlo.ClassicIsing(_edge_list(case), num_experiments=3, seed=5)
    twin = py_monte_carlo.ClassicIsing(_edge_list(case), num_experiments=3, seed=5)
    assert ci.set_rng_rounds(7).get_rng_rounds() == 7 and twin.get_rng_rounds() == 10
    ci.run_monte_carlo(0.4407, 4)
    twin.run_monte_carlo(0.4407, 4)
    assert not np.array_equal(ci.get_states(), twin.get_states())
    # the States-level twin: the experiments' seeds are the draws of the master seed (classicising.rs:62-79), the option set by hand
    st = capi.States(capi.Graph(case.ea, case.eb, case.ej), capi.make_seeds(5, 3))
    st.set_option("philox_rounds", 7)
    st.do_time_steps(4, 0.4407)
    assert np.array_equal(ci.get_states(), st.states()) and np.array_equal(_bits(ci.get_energies()), _bits(st.energies()))
    betas = [0.43, 0.44, 0.45]
    for copies in (1, 2):
        pt = ClassicalTempering((case.ea, case.eb, case.ej), seed=21, copies=copies, rng_rounds=7)
        plain = ClassicalTempering((case.ea, case.eb, case.ej), seed=21, copies=copies)
        for b in betas:
            pt.add_graph(b)
            plain.add_graph(b)
        pt.timesteps(6)
        plain.timesteps(6)
        lads = pt._pair if copies == 2 else [pt]
        for lad, lad10 in zip(lads, plain._pair if copies == 2 else [plain]):
            assert lad._states.philox_rounds == 7 and lad10._states.philox_rounds == 10
            ref = PR.run(oracle, 256, 8, "ferro", np.array(lad._slot_seeds, dtype=np.uint64), [np.array(betas)] * 6, 7)
            assert np.array_equal(lad._states.packed(), ref.steps[-1].words)
    with pytest.raises(ValueError):
        ClassicalTempering((case.ea, case.eb, case.ej), seed=21, rng_rounds=8)
    with pytest.raises(ValueError, match="one process and one device"):
        ClassicalTempering((case.ea, case.eb, case.ej), seed=21, devices=[0], rng_rounds=7)


# ---- the physics control --------------------------------------------------------------------------------------------------------
def test_both_round_counts_meet_the_exact_torus_energy(capi, exact):
    """The exact value is the yardstick, not the ten-round run: shape, beta, run length and sigma rule of the Kaufman check of
    tests/test_gpu_moments.py on the 64 x 16 torus, once per round count, the same bound for both."""
    beta = 0.4407
    W, H, R, every, T = 64, 16, 64, 10, 2000
    N = W * H
    ea, eb, ej = exact.square_lattice_edges(W, H, -1.0)
    g = capi.Graph(ea, eb, ej)
    want = exact.kaufman_energy(W, H, beta) / N
    for rounds in (7, 10):
        st = capi.States(g, capi.make_seeds(41, R))
        st.set_option("philox_rounds", rounds)
        st.do_time_steps(2000, beta)   # thermalised
        e = st.do_time_steps(T, beta, per_step_energies=True)
        means = e[:, every - 1::every].mean(axis=1) / N
        got, stderr = means.mean(), means.std(ddof=1) / np.sqrt(R)
        print(f"rounds {rounds}: energy per site {got:.6f}, exact {want:.6f}, standard error {stderr:.6f}, z {(got - want) / stderr:+.2f}")
        assert abs(got - want) < 5 * stderr, rounds

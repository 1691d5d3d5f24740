"""Every kernel variant of the f64 CSR family on forced shapes: gen_resident_kernel<float|double, STAGE 0|1|2> (`gen_stage`),
gen_sweep_kernel<float|double, RB 1|2|4|8> (`gen_rb`, `disable_resident`), gen_measure_kernel / gen_reduce_kernel, the cuts of the
replica range at 32768 grid rows, the batched row fetch.  Spins bit for bit against oracle engine C, energies against the exact
Hamiltonian (tests/csr_reference.py) within its derived rounding bound, every forced configuration bit-equal to the default one.
tests/test_csr_reference_host.py shows on the host that each graph has the shape its test is named for.

Two shapes the layout rules out, so no graph reaches them: colour classes are padded to 256 positions, hence a workgroup of
the resident kernel never has fewer than 256 threads (tiny_class_graph runs whole waves of padding instead), and the
`p >= class_end` exit of gen_sweep_kernel is never taken (the ring of 640 sites gives classes of 320 sites = 512 positions:
a block of 256 sites, then one wave of sites and three of padding)."""
import math
from fractions import Fraction

import numpy as np
import pytest

import csr_reference as CR

pytestmark = pytest.mark.gpu

SCHEDULE = [0.0, -0.3, 30.0, 0.7]                    # per step: infinite temperature, a negative beta, a frozen step
REPLICA_BETAS = [0.0, -0.3, 30.0, 0.5, 1.2]
RATIOS = {}                                          # kernel -> largest |E_gpu - E_exact| / energy_bound seen
_TRAJ = {}


@pytest.fixture(scope="module", autouse=True)
def report_ratios():
    yield
    for kernel, ratio in sorted(RATIOS.items()):
        print(f"\n[csr] largest |E_gpu - E_exact| / energy_bound, {kernel}: {ratio:.4f}")


@pytest.fixture(autouse=True)
def csr_family(monkeypatch):
    monkeypatch.setenv("ISINGMC_DISABLE_REAL", "1")
    monkeypatch.setenv("ISINGMC_DISABLE_PACKED", "1")


def replica_betas(R):
    return np.resize(np.array(REPLICA_BETAS), R) + 0.01 * (np.arange(R) // len(REPLICA_BETAS) % 50)


def trajectory(oracle, g, seed, betas):
    """the oracle's configuration after every step, computed once per (graph, seed, betas)"""
    key = (g.name, int(seed), tuple(float(b) for b in betas))
    if key not in _TRAJ:
        _TRAJ[key] = CR.oracle_trajectory(oracle, g, seed, betas)
        _TRAJ[key].setflags(write=False)
    return _TRAJ[key]


def check_energy(kernel, g, e_gpu, spins, bound):
    assert math.isfinite(e_gpu)
    err = abs(Fraction(float(e_gpu)) - CR.exact_energy(g.ea, g.eb, g.ej, g.nvars, spins, g.biases))
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), float(err / bound))
    assert err <= bound, (kernel, g.name, float(err), float(bound))


class Run:
    """one container: T steps under `options`, with a schedule (betas per step) or per-replica betas"""

    def __init__(self, capi, g, seeds, options, T, schedule=None, per_replica=None, per_step=False):
        graph = capi.Graph(g.ea, g.eb, g.ej, nvars=g.nvars, biases=g.biases)
        st = capi.States(graph, seeds)
        assert st.family == "csr_f64"
        self.step_kernel = ("gen_measure_kernel + gen_reduce_kernel, per step" if options.get("disable_resident")
                            else "gen_resident_kernel, per step")
        for name, value in options.items():
            st.set_option(name, value)
        if per_replica is not None:
            st.set_betas(per_replica)
            self.eps = st.do_time_steps(T, per_step_energies=per_step)
        else:
            self.eps = st.do_time_steps(T, schedule, per_step_energies=per_step)
        self.spins = st.states().astype(np.uint8)
        self.energies = st.energies()
        self.mags = st.magnetisations()
        st.close()
        graph.close()

    def same_as(self, other, eps=True):
        """eps: the two runs' per-step energies come from the same kernel family (resident or streaming) -- same order, same bits"""
        assert np.array_equal(self.spins, other.spins)
        assert np.array_equal(self.energies.view(np.uint64), other.energies.view(np.uint64))
        assert np.array_equal(self.mags, other.mags)
        if eps and self.eps is not None and other.eps is not None:
            assert np.array_equal(self.eps.view(np.uint64), other.eps.view(np.uint64))


def check_against_oracle(oracle, g, seeds, run, replicas, step_betas):
    """step_betas(r): the betas replica r saw.  Spins, final energy, magnetisation and (when asked for) every step's energy."""
    bound = CR.energy_bound(g.ej, g.biases, g.nvars, CR.max_degree(g))
    for r in replicas:
        traj = trajectory(oracle, g, seeds[r], step_betas(r))
        assert np.array_equal(run.spins[r], traj[-1]), (g.name, r)
        check_energy("gen_measure_kernel + gen_reduce_kernel, final", g, run.energies[r], traj[-1], bound)
        assert run.mags[r] == 2 * int(np.count_nonzero(run.spins[r])) - g.nvars
        if run.eps is not None:
            for t in range(len(traj)):
                check_energy(run.step_kernel, g, run.eps[r, t], traj[t], bound)


def both_beta_modes(capi, oracle, g, seeds, options, T, replicas=None, per_step=True, default_options=None):
    """the configuration and the default-heuristic run of the same inputs, under a schedule and under per-replica betas"""
    R = len(seeds)
    replicas = range(R) if replicas is None else replicas
    default_options = {} if default_options is None else default_options
    for mode in ("schedule", "per_replica"):
        kw = dict(schedule=SCHEDULE[:T]) if mode == "schedule" else dict(per_replica=replica_betas(R))
        run = Run(capi, g, seeds, options, T, per_step=per_step, **kw)
        step_betas = (lambda r: SCHEDULE[:T]) if mode == "schedule" else (lambda r: [replica_betas(R)[r]] * T)
        check_against_oracle(oracle, g, seeds, run, replicas, step_betas)
        if options != default_options:
            run.same_as(Run(capi, g, seeds, default_options, T, per_step=per_step, **kw), eps="disable_resident" not in options)


# ---- resident kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("kind", ["float", "extreme"])
@pytest.mark.parametrize("stage", [0, 1, 2, -1])
def test_resident_instantiations(capi, oracle, stage, kind, bias):
    """gen_resident_kernel<float|double, 0|1|2> on 300 sites, R = 5, T = 4, energies of every step"""
    g = CR.random_graph(kind, bias)
    both_beta_modes(capi, oracle, g, capi.make_seeds(101, 5), {"gen_stage": stage}, 4,
                    default_options={"gen_stage": -1})


@pytest.mark.parametrize("stage", [1, 2])
@pytest.mark.parametrize("window", ["small", "mid", "big"])
def test_resident_lds_windows(capi, oracle, window, stage):
    """staged bytes within 64 KB, between 64 KB and the 150 KB cap (hipFuncSetAttribute), and beyond the cap with STAGE 1 (a
    forced 1 falls back to 0) while STAGE 2 fits with more than 64 KB"""
    g = CR.lds_graph(window)
    both_beta_modes(capi, oracle, g, capi.make_seeds(102, 3), {"gen_stage": stage}, 3)


@pytest.mark.parametrize("stage", [0, 1, 2])
@pytest.mark.parametrize("shape", ["big_class", "tiny_class"])
def test_resident_class_sizes(capi, oracle, shape, stage):
    """classes of 1300 sites (1536 positions on 1024 threads: the `p += nthreads` loop) and classes of fewer than 64 sites"""
    g = CR.big_class_graph() if shape == "big_class" else CR.tiny_class_graph()
    both_beta_modes(capi, oracle, g, capi.make_seeds(103, 3), {"gen_stage": stage}, 3)


# ---- row batching -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["float", "double"])
@pytest.mark.parametrize("kernel", ["resident0", "resident1", "streaming"])
def test_row_batching(capi, oracle, kernel, kind):
    """rows of 0, 1, 7, 8, 9, 15, 16, 17 and 40 directed edges, duplicate bonds and self-loops: every row length's energy term
    against the exact Hamiltonian, on both resident loops (edge by edge) and the streaming kernel (batches of 8, clamped)"""
    g = CR.degree_mix_graph(kind)
    options = {"resident0": {"gen_stage": 0}, "resident1": {"gen_stage": 1}, "streaming": {"disable_resident": 1}}[kernel]
    both_beta_modes(capi, oracle, g, capi.make_seeds(104, 5), options, 4)


# ---- streaming kernel, every RB -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 3, 8, 13])
@pytest.mark.parametrize("kind", ["float", "double"])
@pytest.mark.parametrize("shape", ["ring640", "multi_class"])
def test_streaming_every_rb(capi, oracle, shape, kind, R):
    """gen_sweep_kernel<float|double, 1|2|4|8>: R below RB, not a multiple of RB, exactly RB; all four widths give the same
    spins and the same energy bits; RB = 1 against the oracle for every replica"""
    g = CR.ring_graph(640, kind) if shape == "ring640" else CR.multi_class_graph(kind)
    seeds = capi.make_seeds(105, R)
    for mode in ("schedule", "per_replica"):
        kw = dict(schedule=SCHEDULE) if mode == "schedule" else dict(per_replica=replica_betas(R))
        step_betas = (lambda r: SCHEDULE) if mode == "schedule" else (lambda r: [replica_betas(R)[r]] * 4)
        one = Run(capi, g, seeds, {"disable_resident": 1, "gen_rb": 1}, 4, per_step=True, **kw)
        check_against_oracle(oracle, g, seeds, one, range(R), step_betas)
        for rb in (2, 4, 8, 0):
            Run(capi, g, seeds, {"disable_resident": 1, "gen_rb": rb}, 4, per_step=True, **kw).same_as(one)
        Run(capi, g, seeds, {}, 4, per_step=False, **kw).same_as(one)      # the default choice for this size: the resident kernel


# ---- the rule that picks RB, and the cut of the replica range ---------------------------------------------------------------------
@pytest.mark.parametrize("shape,R,replicas", [("one_block", 16387, [0, 7, 8, 16383, 16384, 16386]),
                                              ("multi_class", 8003, [0, 7, 8, 7999, 8000, 8002])])
def test_rb_rule(capi, oracle, shape, R, replicas):
    """One 256-position block per class and 16387 replicas: the rule keeps RB = 8, the last thread row holds 3 replicas.
    Classes of three blocks and of one with 8003 replicas: RB = 8 and RB = 2 within one timestep (test_rb_rule_shapes on the
    host).  The default run equals the RB = 1 run on every replica; the listed ones against the oracle."""
    g = CR.one_block_graph() if shape == "one_block" else CR.multi_class_graph("double")
    seeds = capi.make_seeds(106, R)
    for kw, step_betas in ((dict(schedule=SCHEDULE[:3]), lambda r: SCHEDULE[:3]),
                           (dict(per_replica=replica_betas(R)), lambda r: [replica_betas(R)[r]] * 3)):
        default = Run(capi, g, seeds, {"disable_resident": 1}, 3, **kw)
        check_against_oracle(oracle, g, seeds, default, replicas, step_betas)
        default.same_as(Run(capi, g, seeds, {"disable_resident": 1, "gen_rb": 1}, 3, **kw))


def test_grid_cut(capi, oracle):
    """32768 + 5 replicas at RB = 1: launch_gen_timestep and the measurement cut the replica range at 32768 grid rows and offset
    keys, betas, states and partial sums; per-replica betas.  Every replica equals the RB = 8 run (one launch)."""
    g = CR.one_block_graph()
    R = 32768 + 5
    seeds = capi.make_seeds(107, R)
    betas = replica_betas(R)
    one = Run(capi, g, seeds, {"disable_resident": 1, "gen_rb": 1}, 3, per_replica=betas)
    check_against_oracle(oracle, g, seeds, one, [0, 32767, 32768, 32772], lambda r: [betas[r]] * 3)
    one.same_as(Run(capi, g, seeds, {"disable_resident": 1, "gen_rb": 8}, 3, per_replica=betas))
    assert np.array_equal(one.mags, 2 * one.spins.sum(axis=1, dtype=np.int64) - g.nvars)


# ---- per-step energies on the streaming path ------------------------------------------------------------------------------------
def test_streaming_per_step_energies(capi, oracle):
    """6 steps on the degree-mix graph: every column within the bound of the exact energy of the oracle's configuration after
    that step; the last column is the same kernels in the same order as energies(): equal bits"""
    g = CR.degree_mix_graph("double")
    seeds = capi.make_seeds(108, 5)
    betas = SCHEDULE + [1.5, 0.2]
    run = Run(capi, g, seeds, {"disable_resident": 1}, 6, schedule=betas, per_step=True)
    check_against_oracle(oracle, g, seeds, run, range(5), lambda r: betas)
    assert np.array_equal(run.eps[:, -1].view(np.uint64), run.energies.view(np.uint64))

"""Every instantiation of the plain two-class checkerboard kernels (`mc_mode == MC_NONE`) outside the streaming sweep, on forced
shapes, bit for bit against oracle engine B: lat_resident_kernel, lat_sweep_measure_kernel, lat_measure_kernel
(csrc/lattice_kernels.hpp) and lat_resident_spread_kernel (csrc/spread_kernels.hpp) -- spins after every call, energies after
every timestep, energies() and magnetisations(), and the K1 recomputation of the energy from the returned spins over the edge
list (`oracle.energy`; J = +-1, so that sum is an exact integer and equality is asked for).  tests/lat_variants_reference.py
holds the shapes, the couplings (ferro: J = -1, antiferro: J = +1, pmj: +-1 from sign planes) and the selection rules restated;
tests/test_lat_variants_host.py proves without a GPU that each shape selects the kernel named below and that the oracle alone
keeps K1 on these shapes.

Census.  "before": what compared the kernel with the oracle before this module (ties = test_gpu_ties.py:
test_lat_resident_kernels_64x64 at 64 x 64, 16 quads, `resident_spread` 0 / 1, one beta, three steps, and
test_lat_sweep_measure_kernel at 1024 x 256, 16 workgroups; full = test_gpu_fullsize.py at 4096^2; par = test_gpu_parity.py,
one beta per call, `resident_spread` left at 1 so that the occupancy query picks the kernel: 64 x 64, 128 x 32, 64 x 4, 256 x 64,
512 x 16, 256 x 32 and 256 x 16 spread at LPQ 8 when it says yes, 16384 x 16 and 8192 x 6 are lat_resident_kernel by their
size, 16384 x 64 streams with per-step energies; "-" = never; "(eq)" = test_resident_kernel_equals_per_colour_launches, which
compares with the streaming launches, not with the oracle).  "now": R = test_resident_instantiations[shape-spread.lpq-coupling],
F = test_fused_instantiations[shape-coupling], M = test_measure_instantiations[shape-coupling]; one_sign = the couplings ferro
and antiferro.  Every R and F case runs a
schedule in one call and per-replica betas, each with and without per-step energies.

 lat_resident_kernel<VEC, PMJ>              before          now
  false false                               ties            R[64x4|192x12|128x32|64x512 - 0.0 - one_sign]
  false true                                ties            R[the same - 0.0 - pmj]
  true  false                               par             R[256x8|768x4|256x128|256x256|512x256|512x512 - 0.0 - one_sign], R[256x132 - 2.0 - one_sign]
  true  true                                (eq)            R[the same - pmj]
  and, all four, test_resident_chunk_border[0-*]
 lat_resident_spread_kernel<VEC, PMJ, LPQ>  before          now
  false false 8                             ties, par       R[64x4|192x12|128x32|64x512 - 2.0 - one_sign], test_three_hundred_replicas
  false true  8                             ties            R[the same - 2.0 - pmj], test_three_hundred_replicas[pmj]
  true  false 8                             par             R[256x8|768x4|256x128 - 2.0 - one_sign]
  true  true  8                             par             R[the same - 2.0 - pmj]
  false false 4                             - (never run)   R[64x4|192x12|128x32|64x512 - 2.4 - one_sign]
  false true  4                             - (never run)   R[the same - 2.4 - pmj]
  true  false 4                             - (never run)   R[256x8|768x4|256x128|256x132|256x256 - 2.4 - one_sign]
  true  true  4                             - (never run)   R[the same - 2.4 - pmj]
  false false 2                             - (never run)   R[64x4|192x12|128x32|64x512 - 2.2 - one_sign]
  false true  2                             - (never run)   R[the same - 2.2 - pmj]
  true  false 2                             - (never run)   R[256x8|768x4|256x128|256x132|256x256|512x256 - 2.2 - one_sign]
  true  true  2                             - (never run)   R[the same - 2.2 - pmj]
  and <false, *, 8> in test_resident_chunk_border[2-*]
 lat_sweep_measure_kernel<VEC, PMJ, UNI>    before          now
  false false false                         -               F[192x12|64x16416 - one_sign]
  false true  false                         -               F[192x12|64x16416 - pmj]
  true  false false                         -               F[768x12|768x172|256x4104 - one_sign]
  true  true  false                         -               F[768x12|768x172|256x4104 - pmj]
  true  false true                          ties, full      F[1024x32|1024x96|256x4224 - one_sign]
  true  true  true                          ties, par       F[1024x32|1024x96|256x4224 - pmj]
 lat_measure_kernel<VEC, PMJ>               before          now
  false false                               side effect     M[192x12|192x688|64x16416 - one_sign]
  false true                                side effect     M[192x12|192x688|64x16416 - pmj]
  true  false                               side effect     M[768x12|768x172|256x4104 - one_sign]
  true  true                                side effect     M[768x12|768x172|256x4104 - pmj]
  ("side effect": read through energies() behind sweeps everywhere, never on a hand-built configuration.)  Every R and F case
  reads energies() and magnetisations() -- this kernel -- after each of its calls too.

Corrections to what the shapes were chosen for, from the code.  (1) test_gpu_ties.py::test_lat_sweep_measure_kernel does compare
lat_sweep_measure_kernel<true, *, true> with the oracle at a moderate size (1024 x 256: 4096 quads, exactly MEASURE_SLOTS = 16
workgroups in x, so the slots do not wrap there).  (2) The comment "whole waves" on the deciding lanes of the spread kernel holds
for `tid < nquads` only up to the last wave: 132 quads at LPQ 4 are two waves and four lanes, and on every small shape a part of
one wave decides; idle lanes (`quad >= nquads`, up to 63 of them by the rounding of the threads) only pass the barriers.  (3) At
LPQ 2 and 512 quads the launch asks for 16 KB of planes and 64 KB of random words, 80 KB of dynamic LDS: more than the 64 KB
LDS_RESIDENT_MAX_BYTES speaks of, which bounds the planes alone.  (4) lat_resident_fits admits at most 1024 quads and the one-lane
kernel gets a thread per quad up to 1024 threads: `gid += nthreads` runs once on every lattice the host sends there.  (5) 256 x
132 with `resident_spread` = 2 and no `resident_lpq` is the rule's refusal (8 * 132 > 1024): that variant IS lat_resident_kernel,
so the shape carries no separate `resident_spread` = 0 variant.  (6) No earlier test crosses the chunk border of 65536
timesteps on the resident path: test_resident_chunk_border stays.  (7) The oracle takes 35 ms, not a second, per million-spin
sweep here; the large fused shapes still run two replicas and two timesteps per run.  (8) lat_sweep_measure_kernel counts no up
spins (quad_measure): magnetisations() behind a fused call is lat_measure_kernel's.

So the 8 LPQ = 4 / LPQ = 2 kernels ran under no test, 4 of the 6 fused kernels and lat_resident_kernel<true, true> had no oracle
comparison, no resident kernel had one under a schedule or per-replica betas, and no measuring kernel was named by a test.  None
of the 26 disagrees with the oracle on these shapes."""
from fractions import Fraction

import numpy as np
import pytest

import lat_variants_reference as LV

pytestmark = pytest.mark.gpu

COUPLING = [pytest.param(c, id=c) for c in LV.COUPLINGS]


def make_graph(capi, case):
    """the graph of a case, with everything isingmc_graph_info shows of the selection checked against the restatement"""
    g = capi.Graph(case.ea, case.eb, case.ej, nvars=case.nvars)
    info = g.info
    assert g.kind == capi.KIND_LATTICE2D and info.fast_path == 0 == LV.MV.mc_mode(case)
    assert (info.width, info.height) == (case.W, case.H) and bool(info.uniform_sign) == (not case.pmj)
    assert not info.field_signs and not info.open_x and not info.open_y and info.jabs == 1.0 and info.field == 0.0
    assert info.state_words == 2 * LV.geometry(case.W, case.H)[1]
    return g


class Twin:
    """a container beside the oracle's trajectory of its lattice (LV.trajectory: computed once, shared, read-only)"""

    def __init__(self, capi, oracle, shape, coupling, seeds, options, rows=None, large=False):
        self.oracle, self.case, self.seeds, self.large = oracle, LV.make_case(shape.W, shape.H, coupling), seeds, large
        self.rows = list(range(len(seeds))) if rows is None else rows      # the replicas the oracle follows
        self.start, self.runs = LV.trajectory(oracle, shape, coupling, seeds, self.rows, large)
        self.g = make_graph(capi, self.case)
        self.st = capi.States(self.g, seeds)
        assert self.st.family == "checkerboard"
        for name, value in options.items():
            self.st.set_option(name, value)
        self.same_spins(self.start, "the start")

    def close(self):
        self.st.close()
        self.g.close()

    def same_spins(self, want, what):
        packed = self.st.packed()
        for r in self.rows:
            assert np.array_equal(packed[r], want[r]), (what, f"replica {r}", f"{int((packed[r] != want[r]).sum())} words differ")

    def same_measurements(self, step, what):
        e, m = self.st.energies(), self.st.magnetisations()
        for r in self.rows:
            assert (e[r], m[r]) == (step.energy[r], step.mag[r]), (what, r)

    def same_step_energies(self, eps, steps, what):
        assert eps.shape == (len(self.seeds), len(steps))
        for r in self.rows:
            assert eps[r].tolist() == [s.energy[r] for s in steps], (what, r)

    def k1(self, what):
        """the energy and the magnetisation recomputed from the returned spins: independent of the kernel's counters"""
        c = self.case
        spins, e, m = self.st.states(), self.st.energies(), self.st.magnetisations()
        for r in self.rows:
            assert e[r] == self.oracle.energy(c.ea, c.eb, c.ej, c.nvars, spins[r]), (what, r)
            assert m[r] == 2 * int(spins[r].sum()) - c.nvars, (what, r)

    def four_runs(self):
        """LV.four_runs: all steps in one call with the energy of every timestep (`thr_stride` = 1, `steps_out`); the same betas as
        separate calls without; per-replica betas without; per-replica betas with"""
        st, R = self.st, len(self.seeds)
        plan = LV.four_runs(R, self.large)
        (sched, _), steps = plan[0], self.runs[0]
        eps = st.do_time_steps(len(sched), np.array(sched), per_step_energies=True)
        self.same_step_energies(eps, steps, "per-step energies of one call")
        self.same_spins(steps[-1].packed, "one call of all steps")
        self.same_measurements(steps[-1], "one call of all steps")
        self.k1("one call of all steps")
        for step in self.runs[1]:
            st.do_time_steps(1, float(step.beta))
            self.same_spins(step.packed, f"a call of one step at beta {step.beta}")
            self.same_measurements(step, f"a call of one step at beta {step.beta}")
        (betas, _), steps = plan[2], self.runs[2]
        st.set_betas(betas[0])
        st.do_time_steps(len(betas))
        self.same_spins(steps[-1].packed, "per-replica betas")
        self.same_measurements(steps[-1], "per-replica betas")
        (betas, _), steps = plan[3], self.runs[3]
        st.set_betas(betas[0])
        eps = st.do_time_steps(len(betas), per_step_energies=True)
        self.same_step_energies(eps, steps, "per-step energies under per-replica betas")
        self.same_spins(steps[-1].packed, "per-replica betas, per-step energies")
        self.same_measurements(steps[-1], "per-replica betas, per-step energies")
        self.k1("the end")
        assert st.timestep == sum(len(r) for r in self.runs)


# ---- resident kernels -------------------------------------------------------------------------------------------------------------
RESIDENT_CASES = [pytest.param(s, spread, lpq, id=f"{s.name}-{spread}.{lpq}") for s in LV.RESIDENT for spread, lpq in LV.resident_variants(s)]


@pytest.mark.parametrize("coupling", COUPLING)
@pytest.mark.parametrize("shape,spread,lpq", RESIDENT_CASES)
def test_resident_instantiations(capi, oracle, shape, spread, lpq, coupling):
    """lat_resident_kernel<VEC, PMJ> / lat_resident_spread_kernel<VEC, PMJ, LPQ> as LV.resident_kernel names them, three seeds"""
    options = LV.variant_options(shape, spread, lpq)
    print(f"[lat resident] {LV.resident_kernel(shape._replace(options=options), coupling == 'pmj')} "
          f"(spread, lpq, threads, lds) = {LV.resident_launch(shape.W, shape.H, options)}")
    twin = Twin(capi, oracle, shape, coupling, LV.SEEDS, options)
    try:
        twin.four_runs()
    finally:
        twin.close()


@pytest.mark.parametrize("coupling", [pytest.param("antiferro", id="antiferro"), pytest.param("pmj", id="pmj")])
def test_three_hundred_replicas(capi, oracle, coupling):
    """64 x 4 with `resident_spread` = 2 and 300 replicas: more workgroups than compute units, `keys[r]`, `thr_replica[r]` and
    `steps_out[(k * n_replicas + r) * 2]` at r up to 299.  The oracle follows the first, a middle and the last replica."""
    shape = LV.by_name(LV.RESIDENT, "64x4")
    seeds = capi.make_seeds(300, 300)
    betas = LV.replica_betas(300)
    assert betas[0] == 0.0 and betas[149] > 0.4 and betas[299] > 1.0
    twin = Twin(capi, oracle, shape, coupling, seeds, LV.variant_options(shape, 2, 0), rows=[0, 149, 299])
    try:
        twin.four_runs()
    finally:
        twin.close()


_BORDER = {}


def _border_reference(oracle, coupling, seeds, betas):
    """the oracle over 65536 + 3 timesteps of 64 x 4, once per coupling: (packed spins at the end, the last three energies)"""
    if coupling not in _BORDER:
        lat = LV.oracle_lat(oracle, LV.make_case(64, 4, coupling))
        packed, last = [], []
        for seed in seeds:
            ref, e = lat.init(seed), []
            for t, beta in enumerate(betas):
                lat.sweep(ref, seed, t, beta)
                if t >= len(betas) - 3:
                    e.append(lat.energy_mag(ref)[0])
            packed.append(ref)
            last.append(e)
        _BORDER[coupling] = (np.stack(packed), last)
    return _BORDER[coupling]


@pytest.mark.parametrize("per_step", [True, False], ids=["per_step", "plain"])
@pytest.mark.parametrize("coupling", [pytest.param("ferro", id="ferro"), pytest.param("pmj", id="pmj")])
@pytest.mark.parametrize("spread", [0, 2])
def test_resident_chunk_border(capi, oracle, spread, coupling, per_step):
    """64 x 4, two replicas, one call of 65536 + 3 timesteps over a schedule: plan_steps caps a resident chunk at 65536 timesteps, so
    the call is two launches; the second starts at k = 0 of its own threshold table (`h_thr`, refilled behind a stream
    synchronisation or the read-back of the first chunk's counters) and of its own `steps_out`, at t0 = 65536.  The last three
    per-step energies -- all of the second launch -- and the final spins against the oracle.  (No other test crosses this border
    on the resident path.)"""
    T = LV.RESIDENT_CHUNK + 3
    # the schedule repeats with period 5 and 65536 % 5 = 1: a second launch that read the table from the call's start, or the
    # first chunk's table again, would run the wrong betas
    betas = np.resize(LV.BETAS, T)
    assert not np.array_equal(betas[LV.RESIDENT_CHUNK:], betas[:3])
    seeds = LV.SEEDS[:2]
    want_packed, want_last = _border_reference(oracle, coupling, seeds, betas)
    shape = LV.by_name(LV.RESIDENT, "64x4")
    case = LV.make_case(shape.W, shape.H, coupling)
    g = make_graph(capi, case)
    st = capi.States(g, seeds)
    try:
        st.set_option("resident_spread", spread)
        eps = st.do_time_steps(T, betas, per_step_energies=per_step)
        assert st.timestep == T
        assert np.array_equal(st.packed(), want_packed)
        e = st.energies()
        for r in range(2):
            assert e[r] == want_last[r][-1]
            if per_step:
                assert eps[r, -3:].tolist() == want_last[r]
        spins = st.states()
        assert e[0] == oracle.energy(case.ea, case.eb, case.ej, case.nvars, spins[0])
    finally:
        st.close()
        g.close()


# ---- the fused kernel -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coupling", COUPLING)
@pytest.mark.parametrize("shape", LV.FUSED, ids=[s.name for s in LV.FUSED])
def test_fused_instantiations(capi, oracle, shape, coupling):
    """lat_sweep_measure_kernel<VEC, PMJ, UNI> as LV.step_measure_kernel names it (`disable_resident`, `strip` = 0, `sweep_iters`
    = 1: run_lat_stream, colour 0 by lat_sweep_kernel and colour 1 fused with the counting).  The runs without per-step energies
    are the twin on the same container: both colours by lat_sweep_kernel, the same spins asked of both.  Three seeds; two seeds
    and two timesteps on the shapes of 17 workgroups (a million spins)."""
    large = LV.is_large(shape)
    print(f"[lat fused] {LV.step_measure_kernel(shape, coupling == 'pmj')} (workgroups, quads of the last) = {LV.fused_grid(shape.W, shape.H)}")
    twin = Twin(capi, oracle, shape, coupling, LV.SEEDS[:2] if large else LV.SEEDS, shape.options, large=large)
    try:
        twin.four_runs()
    finally:
        twin.close()


# ---- the measuring kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coupling", COUPLING)
@pytest.mark.parametrize("shape", LV.MEASURE, ids=[s.name for s in LV.MEASURE])
def test_measure_instantiations(capi, oracle, shape, coupling):
    """lat_measure_kernel<VEC, PMJ> as LV.measure_kernel names it: energies() and magnetisations() of nine hand-built
    configurations (set_state) against the exact Hamiltonian in integers, against the closed forms of the one-sign lattices, and
    against engine B.  One trip; three trips, the third of 4 lanes; two workgroups, 16 trips and 8 quads."""
    W, H = shape.W, shape.H
    case = LV.make_case(W, H, coupling)
    configs = LV.hand_configurations(W, H)
    g = make_graph(capi, case)
    st = capi.States(g, capi.make_seeds(11, len(configs)))
    try:
        for r, spins in enumerate(configs.values()):
            st.set_state(r, spins)
        e, m = st.energies(), st.magnetisations()
        lat = LV.oracle_lat(oracle, case)
        assert np.array_equal(st.packed(), np.stack([lat.pack(spins) for spins in configs.values()]))
        N, j = W * H, {"ferro": -1, "antiferro": 1, "pmj": 0}[coupling]
        closed = {"up": (2 * N * j, N), "down": (2 * N * j, -N), "checkerboard": (-2 * N * j, 0), "rows": (0, 0)}
        closed.update({name: (2 * N * j - 8 * j, N - 2) for name in configs if name.startswith("corner")})
        for r, (name, spins) in enumerate(configs.items()):
            want_e, want_m = LV.exact_energy_mag(case, spins)
            print(f"[lat measure] {LV.measure_kernel(shape, case.pmj)} {shape.name} {name}: E = {e[r]!r} (exact {float(want_e)!r}), M = {m[r]} (exact {want_m})")
            assert Fraction(float(e[r])) == want_e and int(m[r]) == want_m, name
            assert (e[r], m[r]) == lat.energy_mag(lat.pack(spins)), name
            if name in closed:
                assert int(m[r]) == closed[name][1] and (case.pmj or e[r] == closed[name][0]), name
    finally:
        st.close()
        g.close()

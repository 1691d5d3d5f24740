"""Every instantiation of the multi-class checkerboard kernels (csrc/mc_kernels.hpp, mc_quad_body.inc; launchers and the runtime
switchboard in mc_kernels.hip) on forced shapes, bit for bit against oracle engine B: spins after every call, energies after
every timestep, magnetisations, and the K1 recomputation of the energy from the returned spins over the edge list
(`oracle.energy`, rtol = 1e-12 as tests/test_gpu_field_open.py::_check; every |J| and h here is dyadic, so that sum is exact).
tests/mc_variants_reference.py holds the shapes, the lattices and the selection rules restated; tests/test_mc_variants_host.py
proves without a GPU that each shape selects the kernel named below and that the oracle alone keeps K1 on these shapes.

Census.  T = template arguments; "before": what reached the kernel with an oracle comparison before this module (ties =
test_gpu_ties.py::test_multi_class_kernels, one workgroup, 256 x 16 streaming / 256 x 8 resident; fo = test_gpu_field_open.py;
wide = its streaming test at 4096 x 8 / 16384 x 4 / 2048 x 16, +-J only; load = test_gpu_underload.py at 2048^2; ctr =
test_gpu_counters.py; lanes = test_gpu_lanes.py at 256 x 4; rnd = the hypothesis draws of test_gpu_random.py, W in {256, 512, 768},
H <= 34: resident spread whenever drawn, so not counted as reached); "-" = never.  "now": the shapes of this module
(s12 = stream-768x12, s172 = stream-768x172, u32 = stream-1024x32, u128 = stream-256x128, u96 = stream-1024x96; r136 =
resident-256x136, r44 = resident-768x44, r8n = resident-256x8-nospread; p8 = resident-256x8, p4 = resident-768x4) in
test_sweep_instantiations[shape-mode-one_sign|pmj]; modes: F+ F- = field+ field-, FS = field_signs, OX OY OXY = open_x open_y
open_xy, OF OF- = open_field open_field-, OFS = open_field_signs, A = aniso.

 lat_mc_sweep_kernel<MODE, PMJ, UNI, FS>                 before                      now
  MC_FIELD       false false false                       ties, lanes (1 workgroup)   s12 s172 x F+ F-
  MC_FIELD       false false true                        -                           s12 s172 x FS
  MC_FIELD       false true  false                       load, ctr                   u32 u128 u96 x F+ F-
  MC_FIELD       false true  true                        load                        u32 u128 u96 x FS
  MC_FIELD       true  false false                       -                           s12 s172 x F+ F-
  MC_FIELD       true  false true                        ties (gauged, 1 workgroup)  s12 s172 x FS
  MC_FIELD       true  true  false                       wide, load                  u32 u128 u96 x F+ F-
  MC_FIELD       true  true  true                        -                           u32 u128 u96 x FS
  MC_FIELD_OPEN  false false false                       ties                        s12 s172 x OF OF-
  MC_FIELD_OPEN  false false true                        -                           s12 s172 x OFS
  MC_FIELD_OPEN  false true  false                       -                           u32 u128 u96 x OF OF-
  MC_FIELD_OPEN  false true  true                        -                           u32 u128 u96 x OFS
  MC_FIELD_OPEN  true  false false                       -                           s12 s172 x OF OF-
  MC_FIELD_OPEN  true  false true                        -                           s12 s172 x OFS
  MC_FIELD_OPEN  true  true  false                       wide, load                  u32 u128 u96 x OF OF-
  MC_FIELD_OPEN  true  true  true                        -                           u32 u128 u96 x OFS
  MC_OPEN        false false -                           ties, lanes                 s12 s172 x OX OY OXY
  MC_OPEN        false true  -                           load                        u32 u128 u96 x OX OY OXY
  MC_OPEN        true  false -                           -                           s12 s172 x OX OY OXY
  MC_OPEN        true  true  -                           -                           u32 u128 u96 x OX OY OXY
  MC_ANISO       false false -                           ties                        s12 s172 x A
  MC_ANISO       false true  -                           load                        u32 u128 u96 x A
  MC_ANISO       true  false -                           -                           s12 s172 x A
  MC_ANISO       true  true  -                           wide                        u32 u128 u96 x A
 (the equality test of fo at 512 x 64 compares streaming UNI = true with the resident kernel, not with the oracle.)

 lat_mc_resident_kernel<MODE, PMJ, FS, SPREAD>           before                      now
  MC_FIELD       false false false                       ties (option, 8 quads)      r136 r44 r8n x F+ F-
  MC_FIELD       false false true                        fo, ctr, ties               p8 p4 x F+ F-
  MC_FIELD       false true  false                       -                           r136 r44 r8n x FS
  MC_FIELD       false true  true                        fo                          p8 p4 x FS
  MC_FIELD       true  false false                       -                           r136 r44 r8n x F+ F-
  MC_FIELD       true  false true                        fo                          p8 p4 x F+ F-
  MC_FIELD       true  true  false                       ties (option, gauged)       r136 r44 r8n x FS
  MC_FIELD       true  true  true                        fo, ties                    p8 p4 x FS
  MC_FIELD_OPEN  false false false                       ties (option)               r136 r44 r8n x OF OF-
  MC_FIELD_OPEN  false false true                        fo, ties                    p8 p4 x OF OF-
  MC_FIELD_OPEN  false true  false                       -                           r136 r44 r8n x OFS
  MC_FIELD_OPEN  false true  true                        fo                          p8 p4 x OFS
  MC_FIELD_OPEN  true  false false                       -                           r136 r44 r8n x OF OF-
  MC_FIELD_OPEN  true  false true                        fo                          p8 p4 x OF OF-
  MC_FIELD_OPEN  true  true  false                       -                           r136 r44 r8n x OFS
  MC_FIELD_OPEN  true  true  true                        fo                          p8 p4 x OFS
  MC_OPEN        false -     false                       ties (option)               r136 r44 r8n x OX OY OXY
  MC_OPEN        false -     true                        fo, ties                    p8 p4 x OX OY OXY
  MC_OPEN        true  -     false                       -                           r136 r44 r8n x OX OY OXY
  MC_OPEN        true  -     true                        fo                          p8 p4 x OX OY OXY
  MC_ANISO       false -     false                       ties (option)               r136 r44 r8n x A
  MC_ANISO       false -     true                        fo, ties                    p8 p4 x A
  MC_ANISO       true  -     false                       -                           r136 r44 r8n x A
  MC_ANISO       true  -     true                        fo                          p8 p4 x A

 measurement kernels                                     before                      now
  lat_mc_measure_aniso_kernel<false>                     fo, load (through sweeps)   test_measure_instantiations[*-aniso-one_sign]
  lat_mc_measure_aniso_kernel<true>                      fo, wide                    test_measure_instantiations[*-aniso-pmj]
  lat_mc_measure_open_kernel<false>, no sign planes      fo, load                    ...[*-open_xy-one_sign] [*-open_field-one_sign]
  lat_mc_measure_open_kernel<false>, sign planes         fo, load                    ...[*-field_signs-one_sign] [*-open_field_signs-one_sign]
  lat_mc_measure_open_kernel<true>, no sign planes       fo, wide, load              ...[*-open_xy-pmj] [*-open_field-pmj]
  lat_mc_measure_open_kernel<true>, sign planes          fo                          ...[*-field_signs-pmj] [*-open_field_signs-pmj]
 and every case of test_sweep_instantiations reads energies() (a measurement pass) after each of its separate calls, on the
 streaming shapes also behind every timestep of the call with per-step energies (measure_enqueue in run_mc_stream).

So 12 of the 24 streaming and 7 of the 24 resident instantiations had no oracle comparison before, and every UNI = false streaming
kernel that had one had it on a single workgroup; none of the measurement kernels was named by a test or run on a hand-built
configuration.  None of the 52 disagrees with the oracle on these shapes.

Corrections to what the shapes were chosen for, from the code.  (1) 1024 x 32 and 256 x 128 hold 128 quads per colour: ONE workgroup
in x, half full -- the replicas are the grid's y; 1024 x 96 (384 quads: two workgroups in x, the second cut at 128) is added for a
UNI = true grid that is wider than one workgroup.  (2) lat_resident_fits admits at most 1024 quads and run_mc_resident starts a
wave per 64 quads up to 1024 threads, so no thread of the resident kernel ever owns a second quad: `gid += nthreads` runs once on
every lattice the host sends there; 256 x 136 and 768 x 44 run 192 threads of which 136 / 132 hold a quad.  (3) The streaming
shapes all fit the resident kernel (768 x 172 is 516 quads, 16.5 KB): they carry `disable_resident`.  (4) The measurement kernels
have no grid-stride loop: a workgroup walks MEASURE_QUADS_PER_THREAD = 16 trips of 256 quads and the grid has ceil(nquads / 4096)
workgroups in x.  768 x 172 takes three trips, the last cut after 4 lanes; 256 x 4104 (1.05e6 spins, about a second per case) fills
the 16 trips of a first workgroup and leaves 8 quads to a second."""
from fractions import Fraction

import numpy as np
import pytest

import mc_variants_reference as MV

pytestmark = pytest.mark.gpu

SEEDS = np.array([0x0123456789ABCDEF, 42, 2 ** 64 - 1], dtype=np.uint64)
PMJ = [pytest.param(False, id="one_sign"), pytest.param(True, id="pmj")]
FAST_PATH = {MV.MC_FIELD: 1, MV.MC_OPEN: 2, MV.MC_ANISO: 3, MV.MC_FIELD_OPEN: 4}


def make_graph(capi, case):
    """the graph of a case, with everything isingmc_graph_info shows of the selection checked against the restatement"""
    g = capi.Graph(case.ea, case.eb, case.ej, nvars=case.nvars, biases=case.biases)
    info = g.info
    assert g.kind == capi.KIND_LATTICE2D and info.fast_path == FAST_PATH[MV.mc_mode(case)] == MV.mc_mode(case)
    assert (info.width, info.height) == (case.W, case.H) and bool(info.uniform_sign) == (not case.pmj)
    assert bool(info.field_signs) == case.signs and (bool(info.open_x), bool(info.open_y)) == (case.open_x, case.open_y)
    assert (info.jabs, info.jabs_y) == (case.jx, case.jy) and info.field == (abs(case.h) if case.signs else case.h)
    assert info.state_words == 2 * MV.geometry(case.W, case.H)[1]
    return g


class Twin:
    """a container and engine B side by side"""

    def __init__(self, capi, oracle, case, shape, seeds, rows=None):
        self.oracle, self.case, self.seeds = oracle, case, seeds
        self.g = make_graph(capi, case)
        self.st = capi.States(self.g, seeds)
        assert self.st.family == "checkerboard"
        for name, value in shape.options.items():
            self.st.set_option(name, value)
        self.lat = MV.oracle_lat(oracle, case)
        self.rows = list(range(len(seeds))) if rows is None else rows      # the replicas the oracle follows
        self.ref = {r: self.lat.init(seeds[r]) for r in self.rows}
        self.t = 0
        self.same_spins("the start")

    def close(self):
        self.st.close()
        self.g.close()

    def same_spins(self, what):
        packed = self.st.packed()
        for r in self.rows:
            assert np.array_equal(packed[r], self.ref[r]), (what, f"replica {r}", f"{int((packed[r] != self.ref[r]).sum())} words differ")

    def reference_steps(self, betas):
        """betas[step] or betas[step][replica]; returns the oracle's energies [row, step]"""
        out = np.zeros((len(self.rows), len(betas)))
        for k, beta in enumerate(betas):
            for i, r in enumerate(self.rows):
                self.lat.sweep(self.ref[r], self.seeds[r], self.t, beta[r] if np.ndim(beta) else beta)
                out[i, k] = self.lat.energy_mag(self.ref[r])[0]
            self.t += 1
        return out

    def same_measurements(self, what):
        e, m = self.st.energies(), self.st.magnetisations()
        for r in self.rows:
            assert (e[r], m[r]) == self.lat.energy_mag(self.ref[r]), (what, r)
        return e

    def k1(self, what):
        """the energy and the magnetisation recomputed from the returned spins: independent of the kernel's counters"""
        c = self.case
        spins, e, m = self.st.states(), self.st.energies(), self.st.magnetisations()
        for r in self.rows:
            np.testing.assert_allclose(e[r], self.oracle.energy(c.ea, c.eb, c.ej, c.nvars, spins[r], biases=c.biases), rtol=1e-12, atol=1e-9,
                                       err_msg=f"{what}, replica {r}")
            assert m[r] == 2 * int(spins[r].sum()) - c.nvars

    def schedule(self):
        """section 4 of the plan: one call with the energy of every timestep, the same betas as separate calls without, then
        per-replica betas without and with"""
        st, T, R = self.st, len(MV.BETAS), len(self.seeds)
        eps = st.do_time_steps(T, MV.BETAS, per_step_energies=True)
        want = self.reference_steps(MV.BETAS)
        for i, r in enumerate(self.rows):
            assert eps[r].tolist() == want[i].tolist(), ("per-step energies of one call", r)
        self.same_spins("one call of all steps")
        e = self.same_measurements("one call of all steps")
        assert np.array_equal(e, eps[:, -1])
        self.k1("one call of all steps")
        for beta in MV.BETAS:
            st.do_time_steps(1, float(beta))
            self.reference_steps([beta])
            self.same_spins(f"a call of one step at beta {beta}")
            self.same_measurements(f"a call of one step at beta {beta}")
        betas = MV.replica_betas(R)
        assert 0.0 in betas and betas.min() < 0.0
        st.set_betas(betas)
        st.do_time_steps(3)
        self.reference_steps([betas] * 3)
        self.same_spins("per-replica betas")
        self.same_measurements("per-replica betas")
        eps = st.do_time_steps(2, per_step_energies=True)
        want = self.reference_steps([betas] * 2)
        for i, r in enumerate(self.rows):
            assert eps[r].tolist() == want[i].tolist(), ("per-step energies under per-replica betas", r)
        self.same_spins("per-replica betas, per-step energies")
        self.k1("the end")
        assert st.timestep == self.t == 2 * T + 5


@pytest.mark.parametrize("pmj", PMJ)
@pytest.mark.parametrize("mode", list(MV.MODES))
@pytest.mark.parametrize("shape", MV.SHAPES, ids=[s.name for s in MV.SHAPES])
def test_sweep_instantiations(capi, oracle, shape, mode, pmj):
    """lat_mc_sweep_kernel / lat_mc_resident_kernel as the docstring's table names them (MV.sweep_kernel(case, shape)), 3 replicas"""
    case = MV.make_case(shape.W, shape.H, mode, pmj)
    twin = Twin(capi, oracle, case, shape, SEEDS)
    try:
        twin.schedule()
    finally:
        twin.close()


@pytest.mark.parametrize("mode,pmj", [("field_signs", True), ("open_field", False), ("open_xy", True), ("aniso", False)])
def test_seventy_replicas_on_two_lanes(capi, oracle, mode, pmj):
    """768 x 12 streaming (UNI = false) with `streams` = 2: the calls without per-step energies put replicas 0 .. 34 and 35 .. 69 on
    two streams (`per_lane` = 35 in run_mc_stream), `keys + r0` / `d_thr_mc + r0` / the state offset of the second lane.  Every
    replica against the oracle."""
    shape = MV.SHAPE["stream-768x12"]
    shape = shape._replace(options=dict(shape.options, streams=2))
    case = MV.make_case(shape.W, shape.H, mode, pmj)
    twin = Twin(capi, oracle, case, shape, capi.make_seeds(70, 70))
    try:
        twin.schedule()
    finally:
        twin.close()


# ---- measurement kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pmj", PMJ)
@pytest.mark.parametrize("mode", list(MV.MEASURE_MODES))
@pytest.mark.parametrize("W,H", [(768, 172), (256, 4104)])
def test_measure_instantiations(capi, oracle, W, H, mode, pmj):
    """lat_mc_measure_aniso_kernel<PMJ> (aniso) and lat_mc_measure_open_kernel<PMJ> without (open_xy, open_field) and with sign
    planes (field_signs: no open edge; open_field_signs), as MV.measure_kernel names them: energies() and magnetisations() of nine
    hand-built configurations against the exact Hamiltonian in integers (equality: every size is dyadic), and against engine B.
    768 x 172: three trips of the one workgroup, the last of 4 lanes; 256 x 4104: two workgroups, 16 trips and 8 quads.
    |Jx| = 0.75, |Jy| = 1.25: with the two packed bond counters swapped the energy of `rows` and `random` (and of every
    configuration on the +-J lattice) would differ."""
    case = MV.make_case(W, H, mode, pmj, MV.MEASURE_MODES)
    configs = MV.hand_configurations(W, H)
    g = make_graph(capi, case)
    st = capi.States(g, capi.make_seeds(11, len(configs)))
    try:
        st.set_option("disable_resident", 1)
        for r, spins in enumerate(configs.values()):
            st.set_state(r, spins)
        e, m = st.energies(), st.magnetisations()
        lat = MV.oracle_lat(oracle, case)
        assert np.array_equal(st.packed(), np.stack([lat.pack(spins) for spins in configs.values()]))
        swapped = 0
        for r, (name, spins) in enumerate(configs.items()):
            want_e, want_m = MV.exact_energy_mag(case, spins)
            print(f"[mc measure] {MV.measure_kernel(case)} {W}x{H} {name}: E = {e[r]!r} (exact {float(want_e)!r}), M = {m[r]} (exact {want_m})")
            assert Fraction(float(e[r])) == want_e and int(m[r]) == want_m, name
            assert (e[r], m[r]) == lat.energy_mag(lat.pack(spins)), name
            sx, sy, _, _ = MV.bond_sums(case, spins)
            swapped += Fraction(case.jx) * sy + Fraction(case.jy) * sx != want_e
        assert mode != "aniso" or swapped >= 2
        # one timestep behind it, measured again: the counters of a configuration the sweep kernel wrote
        eps = st.do_time_steps(1, 0.4407, per_step_energies=True)
        spins = st.states()
        for r in (0, 2, len(configs) - 1):
            want_e, want_m = MV.exact_energy_mag(case, spins[r])
            assert Fraction(float(eps[r, 0])) == want_e and Fraction(float(st.energies()[r])) == want_e and int(st.magnetisations()[r]) == want_m
    finally:
        st.close()
        g.close()

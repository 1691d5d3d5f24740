"""Shapes, lattices and selection rules of the plain two-class checkerboard kernels (`mc_mode == MC_NONE`: periodic, no field,
one |J|) outside the streaming sweep: lat_resident_kernel, lat_sweep_measure_kernel, lat_measure_kernel
(csrc/lattice_kernels.hpp) and lat_resident_spread_kernel (csrc/spread_kernels.hpp).  Shared by tests/test_gpu_lat_variants.py
and its host companion tests/test_lat_variants_host.py; the helpers that fit come from tests/mc_variants_reference.py
(`geometry`, `cols_log2`, `resident_fits`, `sign_plane`, `edge_lines`, the hand configurations, the exact Hamiltonian).

Three things live here:
 * the shape tables RESIDENT / FUSED / MEASURE and the three couplings run on each shape;
 * the predicates that decide which of the 26 instantiations a container runs, restated from the library's host code (each
   function quotes the lines it mirrors);
 * the oracle's trajectory of a case over the four runs of the GPU tests, computed once per (shape, coupling) and shared by
   every (spread, lpq) variant of the shape.

Nothing here is taken from what a kernel returns."""
from collections import namedtuple

import numpy as np

import mc_variants_reference as MV
from mc_variants_reference import cols_log2, edge_lines, exact_energy_mag, geometry, hand_configurations, resident_fits  # noqa: F401

MEASURE_SLOTS = 16                        # lattice_types.hpp
MEASURE_QUADS_PER_THREAD = 16             # lattice_types.hpp
RESIDENT_CHUNK = 65536                    # step_policy.hpp, plan_steps: P.chunk = std::min<size_t>(P.chunk, 65536) on the resident paths
LDS_PER_CU = 160 * 1024                   # gfx950

# beta 0 and a negative beta: every spin of both classes flips outright; 0.4407: both classes are costly; 3.0: the top threshold
# planes are all zero; 0.9 in between
BETAS = MV.BETAS
BETAS_LARGE = np.array([0.4407, -0.3])    # the fused shapes of 4104 and more quads: two timesteps
SEEDS = np.array([0x0123456789ABCDEF, 42, 2 ** 64 - 1], dtype=np.uint64)

COUPLINGS = ["ferro", "antiferro", "pmj"]  # J = -1 on every bond, J = +1 on every bond, +-1 from two sign planes


def replica_betas(R, run=0):
    """per-replica betas with 0 and a negative one among them.  Two replicas cannot hold 0, a negative and a costly beta at once:
    the two runs under per-replica betas (run = 0, 1) take one of the two outright betas each, beside a costly one"""
    if R == 2:
        return np.array([[0.0, 0.7], [0.55, -0.25]][run])
    return MV.replica_betas(R)


# ---- shapes -----------------------------------------------------------------------------------------------------------------------
Shape = namedtuple("Shape", "name W H options what")
STREAM = {"disable_resident": 1, "strip": 0, "sweep_iters": 1}

RESIDENT = [
    Shape("64x4", 64, 4, {}, "1 quad, non-VEC: 64 threads of which 8, 4 or 2 draw"),
    Shape("192x12", 192, 12, {}, "9 quads, non-VEC: three words per row, quads straddle rows"),
    Shape("128x32", 128, 32, {}, "16 quads, non-VEC"),
    Shape("256x8", 256, 8, {}, "8 quads, VEC: one quad per row"),
    Shape("768x4", 768, 4, {}, "12 quads, VEC: three quads per row; 128 threads at LPQ 8, of which 96 draw"),
    Shape("256x128", 256, 128, {}, "128 quads: LPQ 8 at exactly 1024 threads"),
    Shape("64x512", 64, 512, {}, "128 quads, non-VEC: the same border"),
    Shape("256x132", 256, 132, {}, "132 quads: LPQ 8 falls back to lat_resident_kernel on 192 threads; LPQ 4 spreads on 576 threads"),
    Shape("256x256", 256, 256, {}, "256 quads: LPQ 4 at 1024 threads"),
    Shape("512x256", 512, 256, {}, "512 quads: LPQ 2 at 1024 threads"),
    Shape("512x512", 512, 512, {}, "1024 quads: the largest resident lattice, lat_resident_kernel on 1024 threads"),
]
HOST_ONLY = Shape("256x1028", 256, 1028, {}, "1028 quads: does not fit the resident path")

FUSED = [
    Shape("192x12", 192, 12, STREAM, "<F,*,F>: 9 quads, one cut workgroup"),
    Shape("64x16416", 64, 16416, STREAM, "<F,*,F>: 4104 quads, 17 workgroups: the slots wrap"),
    Shape("768x12", 768, 12, STREAM, "<T,*,F>: 36 quads"),
    Shape("768x172", 768, 172, STREAM, "<T,*,F>: 516 quads, three workgroups, the last with 4 quads"),
    Shape("256x4104", 256, 4104, STREAM, "<T,*,F>: 4104 quads, 17 workgroups, the last with 8 quads"),
    Shape("1024x32", 1024, 32, STREAM, "<T,*,T>: 128 quads"),
    Shape("1024x96", 1024, 96, STREAM, "<T,*,T>: 384 quads, two workgroups"),
    Shape("256x4224", 256, 4224, STREAM, "<T,*,T>: 4224 quads, 17 workgroups, the last half full"),
]

MEASURE = [
    Shape("192x12", 192, 12, {}, "non-VEC, one trip"),
    Shape("768x12", 768, 12, {}, "VEC, one trip"),
    Shape("192x688", 192, 688, {}, "non-VEC, 516 quads: three trips, the third cut after 4 lanes"),
    Shape("768x172", 768, 172, {}, "VEC, 516 quads: three trips, the third cut after 4 lanes"),
    Shape("64x16416", 64, 16416, {}, "non-VEC, 4104 quads: a full first workgroup, a second with 8 quads"),
    Shape("256x4104", 256, 4104, {}, "VEC, 4104 quads: a full first workgroup, a second with 8 quads"),
]


def by_name(table, name):
    return next(s for s in table if s.name == name)


def is_large(shape):
    """the fused shapes the GPU test runs with two replicas and two timesteps"""
    return geometry(shape.W, shape.H)[2] >= 4104


# ---- lattices ---------------------------------------------------------------------------------------------------------------------
def make_case(W, H, coupling):
    """a periodic W x H lattice with |J| = 1 as an MV.Case (so MV.bond_sums / MV.exact_energy_mag read it): edge list in the order
    right(0), down(0), right(1), ...; jright / jdown: 1 where J > 0"""
    assert coupling in COUPLINGS
    pmj = coupling == "pmj"
    seed = 1000 * W + H
    if pmj:
        jright, jdown = MV.sign_plane(W, H, seed + 1, 0), MV.sign_plane(W, H, seed + 2, 1)
    else:
        jright = jdown = np.full((H, W), coupling == "antiferro", dtype=np.uint8)
    ids = np.arange(W * H, dtype=np.uint64).reshape(H, W)
    ea = np.stack([ids, ids], axis=-1).reshape(-1)
    eb = np.stack([np.roll(ids, -1, axis=1), np.roll(ids, -1, axis=0)], axis=-1).reshape(-1)
    ej = np.stack([2.0 * jright - 1.0, 2.0 * jdown - 1.0], axis=-1).reshape(-1)
    c = np.ascontiguousarray
    return MV.Case(W, H, coupling, pmj, 0.0, False, False, False, 1.0, 1.0, jright, jdown, None, c(ea), c(eb), c(ej), None, W * H)


def oracle_lat(O, case):
    """oracle engine B of the case"""
    if case.pmj:
        return O.Lat(case.W, case.H, 1.0, 0, case.jright.ravel(), case.jdown.ravel())
    return O.Lat(case.W, case.H, 1.0, int(case.mode == "antiferro"))


# ---- the library's selection rules, restated ---------------------------------------------------------------------------------------
def vec(W, H):
    """step_policy.hpp, lattice_shape (which graph.hip builds the lattice from):  G.vec = G.wpr % 4 == 0;   (`cols_log2` is only looked for `if (g->vec)`: MV.cols_log2 divides
    wpr by four first, so it is asked behind `vec` here too)"""
    return geometry(W, H)[0] % 4 == 0


def uni(W, H):
    """lattice_kernels.hip, lat_launch_sweep_measure:  pick(vec, pmj, vec && g.cols_log2 >= 0, ...) -> lat_sweep_measure_kernel<VEC, PMJ, UNI>"""
    return vec(W, H) and cols_log2(W, H) >= 0


def fast_path_ok(W, H):
    """graph.hip, lattice_fast_path_ok, what it asks of the shape of a periodic field-free lattice:
        if (!L.ok || L.W % 64 != 0) return false;   ...   return wpp % 4 == 0 && 2 * wpp * sizeof(uint32_t) < (uint64_t(1) << 31);"""
    wpp = geometry(W, H)[1]
    return W % 64 == 0 and H % 2 == 0 and wpp % 4 == 0 and 2 * wpp * 4 < 2 ** 31


def resident_launch(W, H, options):
    """(spread, lpq, threads, lds_bytes) of step_policy.hpp, lat_resident_launch (lpq = 0 without the spread form;
    tests/test_step_policy_host.py holds this restatement against it):
        const int lpq = lpq_forced == 4 || lpq_forced == 2 ? lpq_forced : 8;
        bool spread = spread_mode != 0 && size_t(g.nquads) * size_t(lpq) <= 1024;
        const unsigned spread_threads = unsigned((size_t(g.nquads) * size_t(lpq) + 63) / 64 * 64);
        const size_t spread_lds = g.state_words * sizeof(uint32_t) + size_t(g.nquads) * 8 * 16;
        if (spread && spread_mode != 2) { ... the occupancy query: not restated, the tests force mode 0 or 2 ... }
        const unsigned threads = spread ? spread_threads : unsigned(std::min<size_t>(1024, (g.nquads + 63) / 64 * 64));
        const size_t lds = spread ? spread_lds : g.state_words * sizeof(uint32_t);"""
    _, wpp, nquads = geometry(W, H)
    mode, forced = options.get("resident_spread", 1), options.get("resident_lpq", 0)
    assert mode in (0, 2), "mode 1 asks the runtime's occupancy calculation"
    lpq = forced if forced in (4, 2) else 8
    spread = mode != 0 and nquads * lpq <= 1024
    if spread:
        return True, lpq, (nquads * lpq + 63) // 64 * 64, 2 * wpp * 4 + nquads * 8 * 16
    return False, 0, min(1024, (nquads + 63) // 64 * 64), 2 * wpp * 4


def resident_variants(shape):
    """the (resident_spread, resident_lpq) options a resident shape is run with: the one-lane kernel, every spread form the rule
    admits there, and -- where the rule says no just beyond a border (132 quads at LPQ 8) -- the request it turns down"""
    nquads = geometry(shape.W, shape.H)[2]
    out = [(0, 0)] if shape.name != "256x132" else [(2, 0)]
    out += [(2, f) for f in (0, 4, 2) if nquads * (f or 8) <= 1024]
    return out


def variant_options(shape, spread, lpq):
    return dict(shape.options, resident_spread=spread, resident_lpq=lpq)


def measure_grid(W, H):
    """(workgroups in x, trips of the fullest thread) of lattice_kernels.hip, lat_launch_measure:
        const uint32_t blocks = (g.nquads + 256 * MEASURE_QUADS_PER_THREAD - 1) / (256 * MEASURE_QUADS_PER_THREAD);
    and lat_measure_kernel:  gid = (blockIdx.x * MEASURE_QUADS_PER_THREAD + i) * 256 + threadIdx.x;  if (gid >= g.nquads) break;"""
    nquads = geometry(W, H)[2]
    per = 256 * MEASURE_QUADS_PER_THREAD
    return (nquads + per - 1) // per, min(MEASURE_QUADS_PER_THREAD, (nquads + 255) // 256)


def fused_grid(W, H):
    """(workgroups in x, quads of the last one) of lattice_kernels.hip, lat_grid:  dim3((quads + 255) / 256, n_replicas, 1)"""
    nquads = geometry(W, H)[2]
    blocks = (nquads + 255) // 256
    return blocks, nquads - 256 * (blocks - 1)


def _b(flag):
    return "true" if flag else "false"


def resident_kernel(shape, pmj):
    """what one call runs on a resident shape (lattice_kernels.hip: lat_launch_resident; spread_kernels.hip: spread_pick)"""
    assert resident_fits(shape.W, shape.H, shape.options)
    spread, lpq, _, _ = resident_launch(shape.W, shape.H, shape.options)
    if spread:
        return f"lat_resident_spread_kernel<{_b(vec(shape.W, shape.H))}, {_b(pmj)}, {lpq}>"
    return f"lat_resident_kernel<{_b(vec(shape.W, shape.H))}, {_b(pmj)}>"


def step_measure_kernel(shape, pmj):
    """the colour-1 launch of a timestep whose energy is wanted, on the streaming path (isingmc.hip, run_lat_stream)"""
    assert not resident_fits(shape.W, shape.H, shape.options)
    v = vec(shape.W, shape.H)
    return f"lat_sweep_measure_kernel<{_b(v)}, {_b(pmj)}, {_b(uni(shape.W, shape.H))}>"


def measure_kernel(shape, pmj):
    """energies() / magnetisations() of a two-class container (isingmc.hip, lat_measure_enqueue -> lat_launch_measure)"""
    return f"lat_measure_kernel<{_b(vec(shape.W, shape.H))}, {_b(pmj)}>"


def all_instantiations():
    """4 + 12 + 6 + 4 = 26: lat_sweep_measure_kernel<false, *, true> is not instantiated (UNI implies VEC)"""
    out = []
    for v in (False, True):
        for pmj in (False, True):
            out.append(f"lat_resident_kernel<{_b(v)}, {_b(pmj)}>")
            out += [f"lat_resident_spread_kernel<{_b(v)}, {_b(pmj)}, {lpq}>" for lpq in (8, 4, 2)]
            out += [f"lat_sweep_measure_kernel<{_b(v)}, {_b(pmj)}, {_b(u)}>" for u in ((False, True) if v else (False,))]
            out.append(f"lat_measure_kernel<{_b(v)}, {_b(pmj)}>")
    return out


# ---- the oracle's trajectory over the four runs ------------------------------------------------------------------------------------
Step = namedtuple("Step", "beta packed energy mag")


def four_runs(R, large=False):
    """[(betas of the run's timesteps, per-replica?)]: all steps of the schedule (one call), the same betas again (separate calls),
    per-replica betas twice (without and with per-step energies).  betas[k] is a float or an array of R"""
    sched = BETAS_LARGE if large else BETAS
    n3, n4 = (1, 1) if large else (3, 2)
    return [(list(sched), False), (list(sched), False), ([replica_betas(R, 0)] * n3, True), ([replica_betas(R, 1)] * n4, True)]


_TRAJECTORIES = {}


def trajectory(O, shape, coupling, seeds, rows=None, large=False):
    """the oracle over four_runs, once per (lattice, seeds): (the start, four lists of Step): one Step per timestep, with the packed
    spins, the energy and the magnetisation of the followed replicas `rows` after that timestep.  Read-only for its users."""
    rows = tuple(range(len(seeds))) if rows is None else tuple(rows)
    key = (shape.W, shape.H, coupling, tuple(int(s) for s in seeds), rows, large)
    if key not in _TRAJECTORIES:
        lat = oracle_lat(O, make_case(shape.W, shape.H, coupling))
        ref = {r: lat.init(seeds[r]) for r in rows}
        start = {r: ref[r].copy() for r in rows}
        t, out = 0, []
        for betas, per_replica in four_runs(len(seeds), large):
            steps = []
            for beta in betas:
                for r in rows:
                    lat.sweep(ref[r], seeds[r], t, beta[r] if per_replica else beta)
                t += 1
                em = {r: lat.energy_mag(ref[r]) for r in rows}
                steps.append(Step(beta, {r: ref[r].copy() for r in rows}, {r: em[r][0] for r in rows}, {r: em[r][1] for r in rows}))
            out.append(steps)
        for steps in out:
            for s in steps:
                for a in s.packed.values():
                    a.setflags(write=False)
        _TRAJECTORIES[key] = (start, out)
    return _TRAJECTORIES[key]

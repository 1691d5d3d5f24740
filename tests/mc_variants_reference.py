"""Shapes, lattices and selection rules of the multi-class checkerboard kernels (csrc/mc_kernels.hpp), shared by
tests/test_gpu_mc_variants.py and its host companion tests/test_mc_variants_host.py.

Three things live here and nowhere else:
 * SHAPES / MODES: the forced shapes and the lattices (couplings, fields, boundaries) run on each of them;
 * the four predicates that decide which of the 52 instantiations a container runs, restated from the library's host code
   (each function quotes the lines it mirrors) -- `cols_log2` is not readable from isingmc_graph_info, so this restatement is the
   one statement of the UNI rule outside graph.hip;
 * the exact Hamiltonian E = sum_bonds J s s - sum_i h_i s_i of a configuration in Python integers and Fractions, from the sign
   planes themselves (not from an edge list, not from the oracle).

Nothing here is taken from what a kernel returns."""
from collections import namedtuple
from fractions import Fraction

import numpy as np

MC_NONE, MC_FIELD, MC_OPEN, MC_ANISO, MC_FIELD_OPEN = 0, 1, 2, 3, 4
MODE_NAME = {MC_FIELD: "MC_FIELD", MC_OPEN: "MC_OPEN", MC_ANISO: "MC_ANISO", MC_FIELD_OPEN: "MC_FIELD_OPEN"}
LDS_RESIDENT_MAX_BYTES = 64 * 1024        # lattice_types.hpp
MEASURE_QUADS_PER_THREAD = 16             # lattice_types.hpp
N_CU = 256                                # internal.hpp: isingmc_graph::n_cu (the MI355X has 256 compute units)

# ---- the schedule of every case ---------------------------------------------------------------------------------------------------
# beta 0 and a negative beta: every class flips outright (`costly` = 0, no random number is compared); 0.4407: every class is
# costly; 3.0: the top threshold planes of the expensive classes are all zero; 0.9 in between
BETAS = np.array([0.0, -0.3, 0.4407, 3.0, 0.9])


def replica_betas(R):
    """per-replica betas with 0 at replica 0 and a negative one at replica 1 (and again at the last but one of a long container)"""
    betas = np.linspace(0.2, 1.3, R)
    betas[0], betas[1] = 0.0, -0.25
    if R > 4:
        betas[R - 2] = -0.4
        betas[R // 2] = 0.0
    return betas


# ---- shapes -----------------------------------------------------------------------------------------------------------------------
Shape = namedtuple("Shape", "name W H options path uni spread")
SHAPES = [
    # streaming (resident off), UNI = false: W / 256 = 3 is no power of two; 36 quads: one workgroup in x, cut after 36 lanes
    Shape("stream-768x12", 768, 12, {"disable_resident": 1}, "stream", False, None),
    # ... 516 quads: three workgroups in x, the last holds 4 quads (a wave cut mid-row)
    Shape("stream-768x172", 768, 172, {"disable_resident": 1}, "stream", False, None),
    # streaming, UNI = true: cl = 2 (32 rows per pair of waves, 128 quads), cl = 0 (128 rows per pair, 128 quads); at both the one
    # workgroup in x is half full, the replicas are the grid's y.  1024 x 96 (384 quads) adds a second workgroup in x, cut at 128
    Shape("stream-1024x32", 1024, 32, {"disable_resident": 1}, "stream", True, None),
    Shape("stream-256x128", 256, 128, {"disable_resident": 1}, "stream", True, None),
    Shape("stream-1024x96", 1024, 96, {"disable_resident": 1}, "stream", True, None),
    # resident, SPREAD = false by the shape: 136 and 132 quads per colour (8 * nquads > 1024), 192 threads
    Shape("resident-256x136", 256, 136, {}, "resident", False, False),
    Shape("resident-768x44", 768, 44, {}, "resident", False, False),
    # resident, SPREAD = false by the option
    Shape("resident-256x8-nospread", 256, 8, {"resident_spread": 0}, "resident", False, False),
    # resident, SPREAD = true: 8 quads on 64 threads, 12 quads on 128 threads (96 of them draw)
    Shape("resident-256x8", 256, 8, {}, "resident", False, True),
    Shape("resident-768x4", 768, 4, {}, "resident", False, True),
]
SHAPE = {s.name: s for s in SHAPES}
# the shapes beside the table that tests/test_mc_variants_host.py asks `resident_launch` about, and tests/test_step_policy_host.py
# the library's rule: ((W, H, R, options), expected (spread, threads))
LAUNCH_CASES = (((256, 136, 3, {}), (False, 192)), ((768, 44, 3, {}), (False, 192)),     # more than 128 quads: every thread has at most one
                ((256, 1024, 3, {}), (False, 1024)),                                     # 1024 quads: no resident thread loops
                ((256, 8, 3, {"resident_spread": 0}), (False, 64)), ((256, 8, 3, {}), (True, 64)), ((768, 4, 3, {}), (True, 128)),
                ((256, 128, 3, {}), (True, 1024)), ((256, 132, 3, {}), (False, 192)),
                # a container too large for every replica to be resident at once leaves the spread form: n_cu * (1024 / threads) replicas
                ((256, 128, 256, {}), (True, 1024)), ((256, 128, 257, {}), (False, 128)), ((256, 128, 257, {"resident_spread": 2}), (True, 1024)))

# ---- lattices ---------------------------------------------------------------------------------------------------------------------
# name: (h, field signs, open_x, open_y, |Jx|, |Jy|); |h| <= 2|J| periodic, <= |J| on an open lattice (lattice_fast_path_ok).
# Every size is dyadic: the K1 recomputation (oracle.energy, a running f64 sum over the edge list and the biases) is then exact
# at the 4e5 terms of 768 x 172, and the rtol = 1e-12 it is asserted at says something about the kernel's counters -- with
# h = 0.8 the reference's own summation error was 2.4e-12 of the energy there (the oracle against itself, no GPU involved)
MODES = {
    "field+":           (0.75, False, False, False, 1.0, 1.0),
    "field-":           (-1.5, False, False, False, 1.0, 1.0),
    "field_signs":      (1.25, True,  False, False, 1.0, 1.0),
    "open_x":           (0.0,  False, True,  False, 1.0, 1.0),
    "open_y":           (0.0,  False, False, True,  1.0, 1.0),
    "open_xy":          (0.0,  False, True,  True,  1.0, 1.0),
    "open_field":       (0.5,  False, True,  True,  1.0, 1.0),
    "open_field-":      (-0.75, False, False, True, 1.0, 1.0),   # fneg_uniform of McOpen
    "open_field_signs": (0.875, True, True,  True,  1.0, 1.0),
    "aniso":            (0.0,  False, False, False, 0.75, 1.75),
}
# the measurement tests: the library's f64 expression of the energy is exact too and equality is asked for;
# |Jx| != |Jy| with both bond sums differing (asserted per configuration): a swap of the two bond counters changes the energy
MEASURE_MODES = {
    "aniso":            (0.0,  False, False, False, 0.75, 1.25),
    "open_xy":          (0.0,  False, True,  True,  1.0, 1.0),
    "open_field":       (0.5,  False, True,  False, 1.0, 1.0),
    "field_signs":      (0.5,  True,  False, False, 1.0, 1.0),
    "open_field_signs": (0.5,  True,  True,  True,  1.0, 1.0),
}

Case = namedtuple("Case", "W H mode pmj h signs open_x open_y jx jy jright jdown fneg ea eb ej biases nvars")


def edge_lines(plane):
    """the 8 (line, colour) selections of an [H, W] plane: first and last column, first and last row, sites of each colour"""
    H, W = plane.shape
    y, x = np.mgrid[0:H, 0:W]
    out = {}
    for colour in (0, 1):
        mine = (x + y) % 2 == colour
        for name, line in (("col0", x == 0), ("colW", x == W - 1), ("row0", y == 0), ("rowH", y == H - 1)):
            out[(name, colour)] = plane[mine & line]
    return out


def sign_plane(W, H, seed, flip=0):
    """uint8[H, W], random inside; along the first and last row the value alternates every second site, along the first and last
    column every second row (the columns win at the corners): each colour's sites of those four lines -- every second site of a
    line -- carry both values whatever H >= 4 and the seed are (tests/test_mc_variants_host.py asserts it)"""
    plane = np.random.default_rng(seed).integers(0, 2, (H, W)).astype(np.uint8)
    xs, ys = np.arange(W), np.arange(H)
    for row in (0, H - 1):
        plane[row, :] = ((xs // 2) + flip) % 2
    for col in (0, W - 1):
        plane[:, col] = ((ys // 2) + flip) % 2
    return plane


def make_case(W, H, mode, pmj, modes=MODES):
    """edge list in the order right(0), down(0), right(1), ... without the bonds across an open boundary; J = -|J| on every bond
    (one coupling sign, PMJ = false) or +-|J| from two sign planes (jright / jdown: 1 where J > 0)"""
    h, signs, open_x, open_y, jx, jy = modes[mode]
    seed = 1000 * W + H
    jright = sign_plane(W, H, seed + 1, 0) if pmj else np.zeros((H, W), dtype=np.uint8)
    jdown = sign_plane(W, H, seed + 2, 1) if pmj else np.zeros((H, W), dtype=np.uint8)
    fneg = sign_plane(W, H, seed + 3, 1) if signs else None
    ids = np.arange(W * H, dtype=np.uint64).reshape(H, W)
    ea = np.stack([ids, ids], axis=-1).reshape(-1)
    eb = np.stack([np.roll(ids, -1, axis=1), np.roll(ids, -1, axis=0)], axis=-1).reshape(-1)
    ej = np.stack([jx * (2.0 * jright - 1.0), jy * (2.0 * jdown - 1.0)], axis=-1).reshape(-1)
    keep = np.ones(len(ea), dtype=bool)
    if open_x:
        keep &= ~((ea % W == W - 1) & (eb % W == 0))
    if open_y:
        keep &= ~((ea // W == H - 1) & (eb // W == 0))
    biases = None
    if h != 0.0:
        biases = np.full(W * H, h) if not signs else np.where(fneg.ravel() == 1, -h, h)
    c = np.ascontiguousarray
    return Case(W, H, mode, pmj, h, signs, open_x, open_y, jx, jy, jright, jdown, fneg, c(ea[keep]), c(eb[keep]), c(ej[keep]), biases, W * H)


def oracle_lat(O, case):
    """oracle engine B of the case"""
    planes = (case.jright.ravel(), case.jdown.ravel()) if case.pmj else (None, None)
    return O.Lat(case.W, case.H, case.jx, 0, planes[0], planes[1], field=case.h, open_x=case.open_x, open_y=case.open_y,
                 jabs_y=case.jy if case.jy != case.jx else None, field_neg=case.fneg.ravel() if case.signs else None)


# ---- the library's selection rules, restated ---------------------------------------------------------------------------------------
def mc_mode(case):
    """graph.hip, build_lattice:
        g->mc_mode = h != 0.0 ? (open ? MC_FIELD_OPEN : MC_FIELD) : open ? MC_OPEN : L.jabs != L.jabs_y ? MC_ANISO : MC_NONE;"""
    opn = case.open_x or case.open_y
    return (MC_FIELD_OPEN if opn else MC_FIELD) if case.h != 0.0 else MC_OPEN if opn else MC_ANISO if case.jx != case.jy else MC_NONE


def geometry(W, H):
    """step_policy.hpp, lattice_shape (which graph.hip builds the lattice from):  G.wpr = W / 64;  G.wpp = H * G.wpr;  G.nquads = G.wpp / 4;"""
    wpr = W // 64
    return wpr, H * wpr, H * wpr // 4


def fast_path_ok(W, H):
    """graph.hip, lattice_fast_path_ok, what it asks of the shape of a multi-class lattice:
        if ((open || h != 0.0 || aniso) && (L.W / 64) % 4 != 0) return false;   ...   return wpp % 4 == 0 && ...;"""
    wpr, wpp, _ = geometry(W, H)
    return W % 256 == 0 and wpr % 4 == 0 and wpp % 4 == 0 and H % 2 == 0


def cols_log2(W, H):
    """step_policy.hpp, lattice_shape (tests/test_step_policy_host.py holds this restatement against it):
        const uint32_t cols = G.wpr / 4;
        if ((cols & (cols - 1)) == 0) {
            int cl = 0;
            while ((1u << cl) < cols) cl++;
            const uint32_t rows_per_pair = cl >= 6 ? 1 : 2 * (64u >> cl);
            if (H % rows_per_pair == 0 && G.nquads % 64 == 0) G.cols_log2 = cl;
        }
    -1 otherwise; mc_kernels.hip, mc_launch_sweep:  const bool uni = g.cols_log2 >= 0;"""
    wpr, _, nquads = geometry(W, H)
    cols = wpr // 4
    if cols & (cols - 1):
        return -1
    cl = cols.bit_length() - 1
    rows_per_pair = 1 if cl >= 6 else 2 * (64 >> cl)
    return cl if H % rows_per_pair == 0 and nquads % 64 == 0 else -1


def resident_fits(W, H, options):
    """step_policy.hpp, lat_resident_fits (tests/test_step_policy_host.py holds this restatement against it):
        return g.state_words * sizeof(uint32_t) <= LAT_RESIDENT_BYTES && g.nquads <= 1024 && o.disable_resident == 0;"""
    _, wpp, nquads = geometry(W, H)
    return 2 * wpp * 4 <= LDS_RESIDENT_MAX_BYTES and nquads <= 1024 and not options.get("disable_resident", 0)


def resident_launch(W, H, R, options):
    """(spread, threads) of step_policy.hpp, mc_resident_launch (tests/test_step_policy_host.py holds this restatement against it):
        const size_t spread_threads = (size_t(g.nquads) * 8 + 63) / 64 * 64;
        const bool mc_spread = mc_spread_mode != 0 && spread_threads <= 1024 &&
                               (mc_spread_mode == 2 || R <= size_t(g.n_cu) * std::max<size_t>(1, 1024 / spread_threads));
        const unsigned threads = mc_spread ? unsigned(spread_threads) : unsigned(std::min<size_t>(1024, (g.nquads + 63) / 64 * 64));"""
    nquads = geometry(W, H)[2]
    mode = options.get("resident_spread", 1)
    spread_threads = (nquads * 8 + 63) // 64 * 64
    spread = mode != 0 and spread_threads <= 1024 and (mode == 2 or R <= N_CU * max(1, 1024 // spread_threads))
    return spread, spread_threads if spread else min(1024, (nquads + 63) // 64 * 64)


def _b(flag):
    return "true" if flag else "false"


def sweep_kernel(case, shape, R=3):
    """the instantiation one timestep of the case runs on the shape (mc_kernels.hip: mc_launch_sweep, mc_launch_resident)"""
    mode = mc_mode(case)
    if resident_fits(shape.W, shape.H, shape.options):
        spread, _ = resident_launch(shape.W, shape.H, R, shape.options)
        return f"lat_mc_resident_kernel<{MODE_NAME[mode]}, {_b(case.pmj)}, {_b(case.signs)}, {_b(spread)}>"
    return f"lat_mc_sweep_kernel<{MODE_NAME[mode]}, {_b(case.pmj)}, {_b(cols_log2(shape.W, shape.H) >= 0)}, {_b(case.signs)}>"


def measure_kernel(case):
    """isingmc.hip, lat_measure_enqueue:
        if (g->mc_mode == MC_ANISO) { mc_launch_measure_aniso(pmj, ...
        if (g->mc_mode == MC_OPEN || g->mc_mode == MC_FIELD_OPEN || g->d_fneg) { mc_launch_measure_open(pmj, ..., g->d_fneg, ...
        lat_launch_measure(...)                                      (a uniform field on a periodic lattice: the two-class kernel)"""
    mode = mc_mode(case)
    if mode == MC_ANISO:
        return f"lat_mc_measure_aniso_kernel<{_b(case.pmj)}>"
    if mode in (MC_OPEN, MC_FIELD_OPEN) or case.signs:
        return f"lat_mc_measure_open_kernel<{_b(case.pmj)}>" + (" fneg" if case.signs else "")
    return "lat_measure_kernel"


def measure_trips(W, H):
    """(workgroups in x, trips of the fullest thread) of a measurement: MEASURE_QUADS_PER_THREAD x 256 quads per workgroup
        const uint32_t blocks = (g->geom.nquads + 256 * MEASURE_QUADS_PER_THREAD - 1) / (256 * MEASURE_QUADS_PER_THREAD);"""
    nquads = geometry(W, H)[2]
    per = 256 * MEASURE_QUADS_PER_THREAD
    return (nquads + per - 1) // per, min(MEASURE_QUADS_PER_THREAD, (nquads + 255) // 256)


def all_instantiations():
    """the 24 + 24 + 4 kernels of mc_kernels.hip; the open measurement kernel is listed with and without sign planes (6 names)"""
    out = []
    for mode in (MC_FIELD, MC_FIELD_OPEN, MC_OPEN, MC_ANISO):
        for pmj in (False, True):
            for fs in ((False, True) if mode in (MC_FIELD, MC_FIELD_OPEN) else (False,)):
                for other in (False, True):
                    out.append(f"lat_mc_sweep_kernel<{MODE_NAME[mode]}, {_b(pmj)}, {_b(other)}, {_b(fs)}>")
                    out.append(f"lat_mc_resident_kernel<{MODE_NAME[mode]}, {_b(pmj)}, {_b(fs)}, {_b(other)}>")
    for pmj in (False, True):
        out += [f"lat_mc_measure_aniso_kernel<{_b(pmj)}>", f"lat_mc_measure_open_kernel<{_b(pmj)}>", f"lat_mc_measure_open_kernel<{_b(pmj)}> fneg"]
    return out


# ---- the exact Hamiltonian --------------------------------------------------------------------------------------------------------
def bond_sums(case, spins):
    """(Sx, Sy, F, M): sums of sign(J) s s over the existing horizontal / vertical bonds, of sign(h_i) s_i and of s_i: integers"""
    W, H = case.W, case.H
    s = 2 * np.asarray(spins, dtype=np.int64).reshape(H, W) - 1
    hx = s * np.roll(s, -1, axis=1) * (2 * case.jright.astype(np.int64) - 1)
    vy = s * np.roll(s, -1, axis=0) * (2 * case.jdown.astype(np.int64) - 1)
    if case.open_x:
        hx[:, W - 1] = 0
    if case.open_y:
        vy[H - 1, :] = 0
    fsign = 1 - 2 * case.fneg.astype(np.int64) if case.signs else (1 if case.h >= 0 else -1)
    return int(hx.sum()), int(vy.sum()), int((s * fsign).sum()), int(s.sum())


def exact_energy_mag(case, spins):
    """E = |Jx| Sx + |Jy| Sy - |h| F as a Fraction of the f64 sizes, and M"""
    sx, sy, f, m = bond_sums(case, spins)
    return Fraction(case.jx) * sx + Fraction(case.jy) * sy - Fraction(abs(case.h)) * f, m


def hand_configurations(W, H, seed=5):
    """all up, all down, the checkerboard, rows alternating, one flipped spin in each corner of the all-up lattice, a random one"""
    y, x = np.mgrid[0:H, 0:W]
    out = {"up": np.ones((H, W), dtype=np.uint8), "down": np.zeros((H, W), dtype=np.uint8),
           "checkerboard": ((x + y) % 2).astype(np.uint8), "rows": (y % 2).astype(np.uint8)}
    for name, (cy, cx) in (("corner00", (0, 0)), ("corner0W", (0, W - 1)), ("cornerH0", (H - 1, 0)), ("cornerHW", (H - 1, W - 1))):
        spins = np.ones((H, W), dtype=np.uint8)
        spins[cy, cx] = 0
        out[name] = spins
    out["random"] = np.random.default_rng(seed).integers(0, 2, (H, W)).astype(np.uint8)
    return {k: v.ravel() for k, v in out.items()}

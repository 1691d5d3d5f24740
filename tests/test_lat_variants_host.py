"""Host side of tests/test_gpu_lat_variants.py, no GPU: every shape of tests/lat_variants_reference.py selects the instantiation
its GPU test is named for (`vec` and `cols_log2` of build_lattice, lat_resident_fits, the spread rule of run_lat_resident, the UNI
rule of lat_launch_sweep_measure, the grid of lat_launch_measure, all restated there), with the borders of those rules asserted
on both sides; the shapes together name all 26 kernels, each on at least two shapes; the +-J planes carry both signs on the first
and last row and column of both colours; the library's host-side recogniser reads the lattices as built; and the oracle alone
keeps K1 on these shapes: `lat.energy_mag` equals `oracle.energy` of the unpacked spins and the exact Hamiltonian in integers,
so a failure on the GPU points at the kernel and not at the reference."""
from fractions import Fraction

import numpy as np
import pytest

import lat_variants_reference as LV

PMJ = [False, True]
EVERY = {(s.W, s.H): s for s in LV.RESIDENT + LV.FUSED + LV.MEASURE}.values()      # each lattice once
SMALL = [s for s in EVERY if s.W * s.H <= 2 ** 18]


def _launch(W, H, spread, lpq):
    return LV.resident_launch(W, H, {"resident_spread": spread, "resident_lpq": lpq})


def test_resident_shapes_select_what_they_are_named_for():
    q = lambda name: LV.geometry(*map(int, name.split("x")))[2]
    assert [q(s.name) for s in LV.RESIDENT] == [1, 9, 16, 8, 12, 128, 128, 132, 256, 512, 1024]
    assert [LV.vec(s.W, s.H) for s in LV.RESIDENT] == [False, False, False, True, True, True, False, True, True, True, True]
    for s in LV.RESIDENT:
        assert LV.fast_path_ok(s.W, s.H) and LV.resident_fits(s.W, s.H, s.options), s.name
        for spread, lpq in LV.resident_variants(s):
            on, l, threads, lds = _launch(s.W, s.H, spread, lpq)
            assert threads % 64 == 0 and 64 <= threads <= 1024 and lds <= LV.LDS_PER_CU, (s.name, spread, lpq)
            assert not on or threads >= l * q(s.name) > threads - 64, (s.name, spread, lpq)   # blockDim.x >= LPQ * nquads (spread_kernels.hpp)
            assert on or threads >= min(1024, q(s.name)), s.name     # one quad per thread: `gid += nthreads` never runs twice
    # mode 0 never spreads, whatever lpq says
    assert _launch(256, 8, 0, 4) == (False, 0, 64, 2 * 32 * 4)
    # 64 x 4: one quad on a wave, 8 / 4 / 2 lanes of it draw; 768 x 4: 96 of 128 threads draw at LPQ 8
    assert [_launch(64, 4, 2, f)[:3] for f in (0, 4, 2)] == [(True, 8, 64), (True, 4, 64), (True, 2, 64)]
    assert _launch(768, 4, 2, 0)[:3] == (True, 8, 128) and 8 * 12 == 96
    # wpr = 3: the words of a quad span two rows (word 4 Q + q lies in row (4 Q + q) / 3)
    assert LV.geometry(192, 12) == (3, 36, 9) and {(4 * Q + 0) // 3 != (4 * Q + 3) // 3 for Q in range(9)} == {True}
    # border 128 / 132 quads at LPQ 8, VEC and not: 1024 threads, then no spread form and 192 threads of which 132 hold a quad
    assert _launch(256, 128, 2, 0) == (True, 8, 1024, 2 * 128 * 4 * 4 + 128 * 128) == _launch(64, 512, 2, 0)
    assert _launch(256, 132, 2, 0) == (False, 0, 192, 2 * 132 * 4 * 4)
    # ... where LPQ 4 spreads on 576 threads = 9 waves: 528 lanes draw, 132 decide (two waves and four lanes)
    assert _launch(256, 132, 2, 4)[:3] == (True, 4, 576) and 132 * 4 == 528 and 132 == 2 * 64 + 4
    assert _launch(256, 132, 2, 2)[:3] == (True, 2, 320)
    # border 256 / 260 quads at LPQ 4
    assert _launch(256, 256, 2, 4)[:3] == (True, 4, 1024) and _launch(256, 260, 2, 4)[:3] == (False, 0, 320)
    assert _launch(256, 256, 2, 0)[0] is False and _launch(256, 256, 2, 2)[:3] == (True, 2, 512)
    # border 512 / 516 quads at LPQ 2: 16 KB of planes and 64 KB of random words
    assert _launch(512, 256, 2, 2) == (True, 2, 1024, 16384 + 65536) and _launch(256, 516, 2, 2)[:3] == (False, 0, 576)
    assert _launch(512, 256, 2, 4)[0] is False and _launch(512, 256, 2, 0)[0] is False
    # border 1024 / 1028 quads of lat_resident_fits: 1024 threads, one quad each; 1028 quads go to the streaming path
    assert _launch(512, 512, 2, 2) == (False, 0, 1024, 32768) == _launch(512, 512, 0, 0)
    assert LV.resident_fits(512, 512, {}) and LV.geometry(256, 1028)[2] == 1028 and not LV.resident_fits(LV.HOST_ONLY.W, LV.HOST_ONLY.H, {})
    assert LV.fast_path_ok(256, 1028)
    # the variants of the GPU test: every spread form the rule admits, and the request it turns down at 132 quads
    v = {s.name: LV.resident_variants(s) for s in LV.RESIDENT}
    assert v["64x4"] == v["64x512"] == v["256x128"] == [(0, 0), (2, 0), (2, 4), (2, 2)]
    assert v["256x132"] == [(2, 0), (2, 4), (2, 2)] and v["256x256"] == [(0, 0), (2, 4), (2, 2)]
    assert v["512x256"] == [(0, 0), (2, 2)] and v["512x512"] == [(0, 0)]


def test_fused_and_measure_shapes_select_what_they_are_named_for():
    for s in LV.FUSED:
        assert LV.fast_path_ok(s.W, s.H) and not LV.resident_fits(s.W, s.H, s.options), s.name
        assert s.options == {"disable_resident": 1, "strip": 0, "sweep_iters": 1}
        assert LV.step_measure_kernel(s, False).split("<")[1][:-1].replace("true", "T").replace("false", "F").replace(" ", "") == \
            s.what[1:6].replace("*", "F"), s.name
    g = {s.name: LV.fused_grid(s.W, s.H) for s in LV.FUSED}
    assert g == {"192x12": (1, 9), "64x16416": (17, 8), "768x12": (1, 36), "768x172": (3, 4), "256x4104": (17, 8), "1024x32": (1, 128),
                 "1024x96": (2, 128), "256x4224": (17, 128)}
    # border 16 / 17 workgroups: workgroup 16 adds into slot 16 % MEASURE_SLOTS = 0 again
    assert LV.MEASURE_SLOTS == 16 and LV.fused_grid(256, 4096) == (16, 256) and LV.fused_grid(256, 4100)[0] == 17
    assert [s.name for s in LV.FUSED if LV.is_large(s)] == ["64x16416", "256x4104", "256x4224"]
    # UNI: a power of two of quads per row, H a multiple of the rows of a pair of waves, whole waves
    assert LV.cols_log2(1024, 32) == LV.cols_log2(1024, 96) == 2 and LV.cols_log2(256, 4224) == 0 and 4224 % 128 == 0 and 4224 % 64 == 0
    assert LV.cols_log2(256, 4104) == -1 and 4104 % 128 == 8 and LV.cols_log2(768, 172) == -1
    assert not LV.uni(64, 16416) and not LV.vec(192, 12)
    # the measuring kernel: MEASURE_QUADS_PER_THREAD x 256 quads per workgroup
    m = {s.name: LV.measure_grid(s.W, s.H) for s in LV.MEASURE}
    assert m == {"192x12": (1, 1), "768x12": (1, 1), "192x688": (1, 3), "768x172": (1, 3), "64x16416": (2, 16), "256x4104": (2, 16)}
    assert LV.geometry(192, 688)[2] == LV.geometry(768, 172)[2] == 516 == 2 * 256 + 4
    assert LV.geometry(64, 16416)[2] == LV.geometry(256, 4104)[2] == 4096 + 8
    assert LV.measure_grid(256, 4096) == (1, 16)
    for s in LV.MEASURE:
        assert LV.fast_path_ok(s.W, s.H), s.name


def _seen():
    seen = {}
    for pmj in PMJ:
        for s in LV.RESIDENT:
            for spread, lpq in LV.resident_variants(s):
                variant = s._replace(options=LV.variant_options(s, spread, lpq))
                seen.setdefault(LV.resident_kernel(variant, pmj), set()).add(s.name)
        for s in LV.FUSED:
            seen.setdefault(LV.step_measure_kernel(s, pmj), set()).add(s.name)
        for s in LV.MEASURE:
            seen.setdefault(LV.measure_kernel(s, pmj), set()).add(s.name)
    return seen


def test_shapes_cover_every_instantiation():
    want = LV.all_instantiations()
    assert len(want) == 26 == len(set(want))
    seen = _seen()
    assert sorted(seen) == sorted(want)
    for name, shapes in seen.items():
        assert len(shapes) >= 2, name
    # all 8 LPQ = 4 / LPQ = 2 kernels and all six fused kernels on a launch of more than one workgroup in x (fused), resp. on a
    # lattice of more than one deciding wave (spread)
    for pmj in PMJ:
        wide = {LV.step_measure_kernel(s, pmj) for s in LV.FUSED if LV.fused_grid(s.W, s.H)[0] >= 17}
        assert len(wide) == 3
        for lpq in (4, 2):
            big = {LV.resident_kernel(s._replace(options=LV.variant_options(s, 2, lpq)), pmj) for s in LV.RESIDENT
                   if 64 < LV.geometry(s.W, s.H)[2] <= 1024 // lpq}
            assert big == {f"lat_resident_spread_kernel<{v}, {'true' if pmj else 'false'}, {lpq}>" for v in ("false", "true")}


def test_coverage_test_fails_when_a_kernel_loses_its_shapes(monkeypatch):
    monkeypatch.setattr(LV, "RESIDENT", [s for s in LV.RESIDENT if s.name != "512x256"] + [])
    seen = _seen()
    assert sorted(seen) == sorted(LV.all_instantiations())            # 256 x 256 still names the LPQ 2 kernels ...
    monkeypatch.setattr(LV, "RESIDENT", [s for s in LV.RESIDENT if LV.vec(s.W, s.H)])
    lost = set(LV.all_instantiations()) - set(_seen())                # ... but without the narrow lattices eight names are gone
    assert lost == {n for n in LV.all_instantiations() if n.startswith("lat_resident") and "<false" in n} and len(lost) == 8


@pytest.mark.parametrize("shape", EVERY, ids=[s.name for s in EVERY])
def test_sign_planes_carry_both_signs_on_every_edge_line(shape):
    case = LV.make_case(shape.W, shape.H, "pmj")
    for plane in (case.jright, case.jdown):
        lines = LV.edge_lines(plane)
        assert len(lines) == 8
        for key, values in lines.items():
            assert len(values) >= 2 and set(values.tolist()) == {0, 1}, (shape.name, key)
        assert 0.3 < plane.mean() < 0.7
    assert not np.array_equal(case.jright, case.jdown)
    ferro, anti = LV.make_case(shape.W, shape.H, "ferro"), LV.make_case(shape.W, shape.H, "antiferro")
    assert np.all(ferro.ej == -1.0) and np.all(anti.ej == 1.0) and set(case.ej) == {-1.0, 1.0}
    assert len(case.ea) == 2 * shape.W * shape.H


@pytest.mark.parametrize("coupling", LV.COUPLINGS)
@pytest.mark.parametrize("shape", EVERY, ids=[s.name for s in EVERY])
def test_recogniser_reads_the_lattices_as_built(capi, shape, coupling):
    """isingmc_host_recognise_lattice2d on the shuffled edge list: a periodic lattice of this size, one |J|, no open edge and no
    anisotropy -- with no biases that is `mc_mode == MC_NONE` (graph.hip, build_lattice), `fast_path == 0`; the GPU test reads
    kind, fast_path and uniform_sign back from isingmc_graph_info"""
    case = LV.make_case(shape.W, shape.H, coupling)
    perm = np.random.default_rng(1).permutation(len(case.ea))
    r = capi.recognise_lattice2d(case.ea[perm], case.eb[perm], case.ej[perm], case.nvars)
    assert r["is_lattice"] and (r["width"], r["height"]) == (shape.W, shape.H) and r["jabs"] == 1.0
    assert r["uniform_sign"] == (coupling != "pmj")
    assert not r.get("open_x", False) and not r.get("open_y", False) and not r.get("anisotropic", False)
    assert LV.MV.mc_mode(case) == LV.MV.MC_NONE == 0 and case.biases is None
    assert LV.fast_path_ok(shape.W, shape.H)


@pytest.mark.parametrize("coupling", LV.COUPLINGS)
@pytest.mark.parametrize("shape", EVERY, ids=[s.name for s in EVERY])
def test_oracle_alone_keeps_k1(oracle, shape, coupling):
    """engine B over the GPU tests' schedule (two timesteps on the lattices of a million spins): after every timestep its energy
    and magnetisation equal the edge-list energy of the unpacked spins and the exact Hamiltonian in integers"""
    case = LV.make_case(shape.W, shape.H, coupling)
    lat = LV.oracle_lat(oracle, case)
    seed = 0x0123456789ABCDEF
    ref = lat.init(seed)
    assert np.array_equal(lat.pack(lat.unpack(ref)), ref)
    for t, beta in enumerate(LV.BETAS_LARGE if LV.is_large(shape) else LV.BETAS):
        lat.sweep(ref, seed, t, beta)
        e, m = lat.energy_mag(ref)
        spins = lat.unpack(ref)
        assert e == oracle.energy(case.ea, case.eb, case.ej, case.nvars, spins)      # integers below 2^53: the f64 sum is exact
        want, m_want = LV.exact_energy_mag(case, spins)
        assert m == m_want == 2 * int(spins.sum()) - case.nvars
        assert Fraction(e) == want
    assert 0 < spins.sum() < case.nvars


def test_trajectory_is_shared_and_read_only(oracle):
    shape = LV.by_name(LV.RESIDENT, "192x12")
    start, runs = LV.trajectory(oracle, shape, "pmj", LV.SEEDS)
    assert LV.trajectory(oracle, shape, "pmj", LV.SEEDS)[1] is runs
    assert [len(r) for r in runs] == [5, 5, 3, 2] and sorted(start) == [0, 1, 2]
    with pytest.raises(ValueError):
        runs[0][0].packed[0][0] = 0
    betas = LV.replica_betas(3)
    assert 0.0 in betas and betas.min() < 0.0 and betas.max() > 0.4
    for run in (0, 1):
        b = LV.replica_betas(2, run)
        assert min(b) <= 0.0 < 0.4 < max(b)
    assert {min(LV.replica_betas(2, 0)), min(LV.replica_betas(2, 1))} == {0.0, -0.25}
    # replicas differ and the schedule moves them
    last = runs[3][-1]
    assert not np.array_equal(last.packed[0], last.packed[1]) and not np.array_equal(last.packed[0], start[0])


@pytest.mark.parametrize("coupling", LV.COUPLINGS)
def test_hand_configurations_by_hand(oracle, coupling):
    """the exact Hamiltonian of the measurement test's configurations: closed forms on the one-sign lattices, the oracle everywhere"""
    W, H = 192, 12
    case = LV.make_case(W, H, coupling)
    lat = LV.oracle_lat(oracle, case)
    N, j = W * H, {"ferro": -1, "antiferro": 1, "pmj": None}[coupling]
    configs = LV.hand_configurations(W, H)
    assert list(configs) == ["up", "down", "checkerboard", "rows", "corner00", "corner0W", "cornerH0", "cornerHW", "random"]
    for name, spins in configs.items():
        e, m = LV.exact_energy_mag(case, spins)
        assert (Fraction(lat.energy_mag(lat.pack(spins))[0]), lat.energy_mag(lat.pack(spins))[1]) == (e, m), name
        assert e == closed_form(name, j, N)[0] or j is None or name == "random"
        assert m == closed_form(name, 1, N)[1] or name == "random"


def closed_form(name, j, N):
    """(E, M) on a periodic lattice with J = j on all 2 N bonds"""
    if j is None:
        return None, None
    if name in ("up", "down"):
        return 2 * N * j, N if name == "up" else -N
    if name == "checkerboard":
        return -2 * N * j, 0
    if name == "rows":
        return 0, 0                  # the horizontal bonds at +j, the vertical ones at -j
    if name.startswith("corner"):
        return 2 * N * j - 8 * j, N - 2   # four bonds change sign
    return None, None

"""Host side of tests/test_gpu_mc_variants.py, no GPU: every shape of tests/mc_variants_reference.py selects the instantiation
its GPU test is named for (the four predicates restated there: UNI from build_lattice, lat_resident_fits, the spread rule of
run_mc_resident, mc_mode), the cases together name all 52 kernels of csrc/mc_kernels.hip, the sign planes carry both signs on
the first and last column and row of both colours, the library's host-side recogniser reads the lattices as built, and the
oracle alone keeps K1 on these shapes: `lat.energy_mag` equals `oracle.energy` of the unpacked spins and the exact Hamiltonian
in integers, so a failure on the GPU points at the kernel and not at the reference."""
from fractions import Fraction

import numpy as np
import pytest

import mc_variants_reference as MV

PMJ = [False, True]
SMALL = [s for s in MV.SHAPES if "nospread" not in s.name]   # (the same lattice as resident-256x8)
MODE_OF = {"field+": MV.MC_FIELD, "field-": MV.MC_FIELD, "field_signs": MV.MC_FIELD, "open_x": MV.MC_OPEN, "open_y": MV.MC_OPEN,
           "open_xy": MV.MC_OPEN, "open_field": MV.MC_FIELD_OPEN, "open_field-": MV.MC_FIELD_OPEN, "open_field_signs": MV.MC_FIELD_OPEN,
           "aniso": MV.MC_ANISO}


def test_shapes_select_what_they_are_named_for():
    by = MV.SHAPE
    for s in MV.SHAPES:
        assert MV.fast_path_ok(s.W, s.H), s.name
        assert MV.resident_fits(s.W, s.H, s.options) == (s.path == "resident"), s.name
        assert (MV.cols_log2(s.W, s.H) >= 0) == s.uni or s.path == "resident", s.name
        if s.path == "resident":
            assert MV.resident_launch(s.W, s.H, 3, s.options)[0] == s.spread, s.name
    # the streaming shapes would all be resident without the option: that is why they carry it
    assert all(MV.resident_fits(s.W, s.H, {}) for s in MV.SHAPES)
    # UNI = false: three quads per row; 36 quads: one workgroup, cut; 516 = 2 * 256 + 4: three workgroups, the last holds 4 quads
    assert MV.cols_log2(768, 12) == MV.cols_log2(768, 172) == -1 and (768 // 256) & (768 // 256 - 1)
    assert MV.geometry(768, 12)[2] == 36 and MV.geometry(768, 172)[2] == 516 == 2 * 256 + 4
    # UNI = true
    assert MV.cols_log2(1024, 32) == 2 and MV.cols_log2(256, 128) == 0 and MV.cols_log2(1024, 96) == 2
    assert MV.geometry(1024, 32)[2] == MV.geometry(256, 128)[2] == 128 and MV.geometry(1024, 96)[2] == 384
    # ... and the rule's other ways out: a power of two whose H is no multiple of the rows per pair of waves, quads no multiple of 64
    assert MV.cols_log2(256, 136) == -1 and MV.cols_log2(256, 16) == -1 and MV.cols_log2(1024, 16) == -1 and MV.cols_log2(4096, 8) == 4
    assert MV.cols_log2(16384, 4) == 6 and MV.cols_log2(2048, 16) == 3 and MV.cols_log2(2048, 2048) == 3
    # resident without the spread form by the shape: more than 128 quads; 192 threads, so every thread has at most one quad
    assert MV.geometry(256, 136)[2] == 136 and MV.geometry(768, 44)[2] == 132
    for args, want in MV.LAUNCH_CASES:
        assert MV.resident_launch(*args) == want, args
    # lat_resident_fits admits at most 1024 quads and run_mc_resident gives every 64 quads a wave: no resident thread loops
    assert MV.resident_launch(256, 1024, 3, {}) == (False, 1024) and not MV.resident_fits(256, 1028, {})
    assert MV.resident_launch(256, 8, 3, by["resident-256x8-nospread"].options) == (False, 64)
    assert MV.resident_launch(256, 8, 3, {}) == (True, 64) and MV.resident_launch(768, 4, 3, {}) == (True, 128)
    assert MV.resident_launch(256, 128, 3, {}) == (True, 1024) and MV.resident_launch(256, 132, 3, {})[0] is False
    # a container too large for every replica to be resident at once leaves the spread form: n_cu * (1024 / threads) replicas
    assert MV.resident_launch(256, 128, 257, {})[0] is False and MV.resident_launch(256, 128, 257, {"resident_spread": 2})[0] is True


def test_cases_cover_every_instantiation():
    seen = {}
    for s in MV.SHAPES:
        for mode in MV.MODES:
            for pmj in PMJ:
                case = MV.make_case(256, 4, mode, pmj)                 # the names depend on the mode, not on the size
                seen.setdefault(MV.sweep_kernel(case, s), []).append((s.name, mode))
                seen.setdefault(MV.measure_kernel(case), []).append((s.name, mode))
    seen.pop("lat_measure_kernel")                                     # a uniform field on a periodic lattice: the two-class kernel
    want = MV.all_instantiations()
    assert len(want) == 54 and len(set(want)) == 54                    # 24 + 24 + 2 + 2, the open measurement with and without planes
    assert sorted(seen) == sorted(want)
    # every kernel on at least two shapes of its kind
    for name, where in seen.items():
        assert len({shape for shape, _ in where}) >= 2, name
    for mode in MV.MEASURE_MODES:                                      # the measurement tests name the same kernels
        for pmj in PMJ:
            assert MV.measure_kernel(MV.make_case(256, 4, mode, pmj, MV.MEASURE_MODES)) in want


@pytest.mark.parametrize("shape", MV.SHAPES, ids=[s.name for s in MV.SHAPES])
def test_sign_planes_carry_both_signs_on_every_edge_line(shape):
    """+-J planes (right and down bonds) and the field-sign plane: both values among each colour's sites of the first and last
    column and the first and last row -- the words in which the thread-to-quad mapping and the compact layout of the planes can
    disagree without the bulk noticing"""
    case = MV.make_case(shape.W, shape.H, "open_field_signs", True)
    for plane in (case.jright, case.jdown, case.fneg):
        lines = MV.edge_lines(plane)
        assert len(lines) == 8
        for key, values in lines.items():
            assert len(values) >= 2 and set(values.tolist()) == {0, 1}, (shape.name, key)
        assert 0.3 < plane.mean() < 0.7
    assert not np.array_equal(case.jright, case.jdown) and not np.array_equal(case.jright, case.fneg)
    uniform = MV.make_case(shape.W, shape.H, "field+", False)
    assert not uniform.jright.any() and not uniform.jdown.any() and uniform.fneg is None and np.all(uniform.ej == -1.0)


@pytest.mark.parametrize("pmj", PMJ, ids=["one_sign", "pmj"])
@pytest.mark.parametrize("mode", list(MV.MODES))
@pytest.mark.parametrize("shape", SMALL, ids=[s.name for s in SMALL])
def test_recogniser_reads_the_lattices_as_built(capi, shape, mode, pmj):
    case = MV.make_case(shape.W, shape.H, mode, pmj)
    perm = np.random.default_rng(1).permutation(len(case.ea))
    r = capi.recognise_lattice2d(case.ea[perm], case.eb[perm], case.ej[perm], case.nvars)
    assert r["is_lattice"] and (r["width"], r["height"]) == (shape.W, shape.H) and r["jabs"] == case.jx
    assert r["uniform_sign"] == (not pmj)
    assert (r.get("open_x", False), r.get("open_y", False)) == (case.open_x, case.open_y)
    assert r.get("anisotropic", False) == (mode == "aniso")
    assert MV.mc_mode(case) == MODE_OF[mode]
    if case.biases is not None:                                        # one size; both signs exactly with sign planes
        assert set(np.abs(case.biases)) == {abs(case.h)} and (len(set(case.biases)) == 2) == case.signs
        assert abs(case.h) <= (case.jx if case.open_x or case.open_y else 2 * case.jx)


@pytest.mark.parametrize("pmj", PMJ, ids=["one_sign", "pmj"])
@pytest.mark.parametrize("mode", list(MV.MODES))
@pytest.mark.parametrize("shape", SMALL, ids=[s.name for s in SMALL])
def test_oracle_alone_keeps_k1(oracle, shape, mode, pmj):
    """engine B over the GPU tests' schedule: after every timestep its energy and magnetisation equal the edge-list energy of the
    unpacked spins (f64, the tolerance of tests/test_gpu_field_open.py::_check) and the exact Hamiltonian (a Fraction; every
    size is dyadic, so all three are the same number)"""
    case = MV.make_case(shape.W, shape.H, mode, pmj)
    lat = MV.oracle_lat(oracle, case)
    seed = 0x0123456789ABCDEF
    ref = lat.init(seed)
    assert np.array_equal(lat.pack(lat.unpack(ref)), ref)
    for t, beta in enumerate(MV.BETAS):
        lat.sweep(ref, seed, t, beta)
        e, m = lat.energy_mag(ref)
        spins = lat.unpack(ref)
        np.testing.assert_allclose(e, oracle.energy(case.ea, case.eb, case.ej, case.nvars, spins, biases=case.biases), rtol=1e-12, atol=1e-9)
        want, m_want = MV.exact_energy_mag(case, spins)
        assert m == m_want == 2 * int(spins.sum()) - case.nvars
        assert Fraction(e) == want
    assert 0 < spins.sum() < case.nvars


@pytest.mark.parametrize("pmj", PMJ, ids=["one_sign", "pmj"])
@pytest.mark.parametrize("mode", list(MV.MEASURE_MODES))
def test_hand_configurations_by_hand(oracle, mode, pmj):
    """the exact Hamiltonian of the measurement tests' configurations: closed forms where one exists, the oracle's energy (exact:
    dyadic sizes) everywhere, and the anisotropic sizes tell the two bond sums apart"""
    W, H = 768, 12
    case = MV.make_case(W, H, mode, pmj, MV.MEASURE_MODES)
    lat = MV.oracle_lat(oracle, case)
    N = W * H
    bonds_x = N - (H if case.open_x else 0)
    bonds_y = N - (W if case.open_y else 0)
    configs = MV.hand_configurations(W, H)
    assert list(configs) == ["up", "down", "checkerboard", "rows", "corner00", "corner0W", "cornerH0", "cornerHW", "random"]
    swapped = 0
    for name, spins in configs.items():
        e, m = MV.exact_energy_mag(case, spins)
        e_lat, m_lat = lat.energy_mag(lat.pack(spins))
        assert Fraction(e_lat) == e and m_lat == m, name
        sx, sy, f, _ = MV.bond_sums(case, spins)
        swapped += Fraction(case.jx) * sy + Fraction(case.jy) * sx != e
        if not pmj and not case.signs:
            hm = Fraction(case.h)
            if name in ("up", "down"):
                assert e == -Fraction(case.jx) * bonds_x - Fraction(case.jy) * bonds_y - hm * m and abs(m) == N
            if name == "checkerboard":
                assert e == Fraction(case.jx) * bonds_x + Fraction(case.jy) * bonds_y and m == 0
            if name == "rows":
                assert e == -Fraction(case.jx) * bonds_x + Fraction(case.jy) * bonds_y and m == 0
            if name.startswith("corner"):                              # the corner's existing bonds turn from -|J| to +|J|
                lost = 2 * Fraction(case.jx) * (1 if case.open_x else 2) + 2 * Fraction(case.jy) * (1 if case.open_y else 2)
                assert e == configs_energy_up(case, bonds_x, bonds_y, N) + lost + 2 * hm and m == N - 2
    if mode == "aniso":
        assert case.jx != case.jy and swapped >= (1 if not pmj else 5)  # one sign: rows and random; +-J: nearly all


def configs_energy_up(case, bonds_x, bonds_y, N):
    return -Fraction(case.jx) * bonds_x - Fraction(case.jy) * bonds_y - Fraction(case.h) * N


def test_measurement_shapes_take_several_trips():
    """lat_mc_measure_*_kernel: a workgroup walks 16 x 256 quads, `gid = (blockIdx.x * 16 + i) * 256 + threadIdx.x`.  768 x 172:
    one workgroup, three trips, the third cut after 4 lanes; 256 x 4104: two workgroups, the second with 8 quads"""
    assert MV.measure_trips(768, 172) == (1, 3) and MV.geometry(768, 172)[2] % 256 == 4
    assert MV.measure_trips(256, 4104) == (2, 16) and MV.geometry(256, 4104)[2] - 4096 == 8
    assert MV.fast_path_ok(256, 4104) and not MV.resident_fits(256, 4104, {})
    assert MV.measure_trips(256, 8) == (1, 1)

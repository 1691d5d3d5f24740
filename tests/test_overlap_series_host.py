"""The overlap series without a device: its numpy row format against brute-force sums, overlap_moments against
closed forms, and the surface -- header, binding and library carry the same new symbols."""
import ctypes
import os
import re

import numpy as np
import pytest

import overlap_series_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["isingmc_overlap_series_" + s for s in ("create", "record", "set_every", "count", "get", "reset", "destroy")]


def _brute_row(A, B, ea, eb, pa, pb, link, tables, n_classes):
    """Every entry as the sum it is defined as, term by term."""
    sA, sB = 2 * A.astype(np.int64) - 1, 2 * B.astype(np.int64) - 1
    out = []
    for ra, rb in zip(pa, pb):
        e = [sum(int(sA[ra, i] * sB[rb, i]) for i in range(A.shape[1]))]
        if link:
            e.append(sum(int(sA[ra, a] * sA[ra, b] * sB[rb, a] * sB[rb, b]) for a, b in zip(ea, eb)))
        for t in ([] if tables is None else tables):
            for c in range(n_classes):
                e.append(sum(int(sA[ra, i] * sB[rb, i]) for i in range(A.shape[1]) if t[i] == c))
        out.append(e)
    return np.array(out, dtype=np.int64)


@pytest.mark.parametrize("shape", ["torus_4x4", "cube_3"])
def test_row_format_against_brute_force(exact, shape):
    from pyisingmontecarlo_amd.correlation import plane_classes

    if shape == "torus_4x4":
        ea, eb, _ = exact.square_lattice_edges(4, 4, -1.0)
        N, tables = 16, plane_classes((4, 4))
    else:
        ea, eb, _ = exact.cubic_lattice_edges(3, 1.0)
        N, tables = 27, plane_classes((3, 3, 3))
    ea, eb = np.append(ea, [2, 0]).astype(np.int64), np.append(eb, [2, 1]).astype(np.int64)   # an entry a == b and a duplicate
    tables = tables.astype(np.int64)
    tables[0, 5] = SR.CR.NO_CLASS          # a site counted nowhere in table 0
    n_classes = 5                          # class 4 (and 3 on the cube) is empty
    rng = np.random.default_rng(21)
    A, B = rng.integers(0, 2, (6, N)).astype(bool), rng.integers(0, 2, (5, N)).astype(bool)
    pa, pb = np.array([0, 3, 3, 5, 2]), np.array([4, 0, 0, 1, 2])
    for link in (True, False):
        for tb in (None, tables):
            got = SR.row(A, B, ea, eb, pa, pb, link, tb, n_classes)
            want = _brute_row(A, B, ea, eb, pa, pb, link, tb, n_classes)
            assert got.dtype == np.int64 and got.shape == (5, SR.entries(link, 0 if tb is None else len(tb), n_classes))
            assert np.array_equal(got, want)
    same = SR.row(A, A, ea, eb, [1], [1], True, tables, n_classes)[0]   # a pair (r, r): the sizes
    assert same[0] == N and same[1] == len(ea)
    assert np.array_equal(same[2:].reshape(len(tables), n_classes), SR.CR.class_sizes(tables, n_classes).astype(np.int64))
    spin, lnk, by_class = SR.split(np.stack([got, got]), False, len(tables), n_classes)
    assert lnk is None and spin.shape == (2, 5) and by_class.shape == (2, 5, len(tables), n_classes)
    assert np.array_equal(by_class[1].reshape(5, -1), got[:, 1:])
    assert SR.sample_points(2, 3, 2, 12) == [5, 8, 11] and SR.sample_points(0, 4, 4, 8) == [8]


def test_overlap_moments_closed_forms():
    from pyisingmontecarlo_amd.correlation import overlap_moments

    N = 64
    q1, q2, q4, binder = overlap_moments(np.array([[N, -N], [-N, -N], [N, -N], [-N, -N]]), N)   # all q = +-1
    assert q1.tolist() == [0.0, -1.0] and q2.tolist() == [1.0, 1.0] and q4.tolist() == [1.0, 1.0] and binder.tolist() == [1.0, 1.0]
    # q in {-1/2 (twice), +1/2 (twice), -1, +1}: <q> = 0, <q^2> = (4 / 4 + 2) / 6 = 1/2, <q^4> = (4 / 16 + 2) / 6 = 3/8,
    # binder = (3 - (3/8) / (1/4)) / 2 = 3/4 -- every value a binary fraction, so the comparison is exact
    q1, q2, q4, binder = overlap_moments(np.array([-32, -32, 32, 32, -64, 64])[:, None], N)
    assert (q1[0], q2[0], q4[0], binder[0]) == (0.0, 0.5, 0.375, 0.75)
    # leading axes are kept: [n, P, ...] gives [P, ...]; a column that is 0 throughout has no ratio
    out = overlap_moments(np.zeros((3, 2, 4)), N)
    assert all(o.shape == (2, 4) for o in out) and np.isnan(out[3]).all()


def test_surface():
    """The header declares every new symbol the binding binds, and the library exports them."""
    with open(os.path.join(ROOT, "include", "isingmc.h")) as f:
        header = f.read()
    from pyisingmontecarlo_amd import _capi
    bound = [s for s in _capi.EXPORTED_SYMBOLS if s.startswith("isingmc_overlap_series_")]
    assert sorted(bound) == sorted(SYMBOLS)
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), sym
    assert re.search(r"#define\s+ISINGMC_SERIES_LINK\s+1u", header) and re.search(r"#define\s+ISINGMC_SERIES_BY_RUNG\s+2u", header)
    assert (_capi.SERIES_LINK, _capi.SERIES_BY_RUNG) == (1, 2)
    assert re.search(r"#define\s+ISINGMC_ABI_VERSION\s+4\b", header)
    so = ctypes.CDLL(_capi.LIB_PATH) if os.path.exists(_capi.LIB_PATH) else None
    assert so is not None, "libisingmc.so is not built"
    for sym in SYMBOLS:
        assert hasattr(so, sym), sym
    for name in ("record", "set_every", "count", "capacity", "get", "reset", "close"):
        assert hasattr(_capi.OverlapSeries, name)
    assert callable(_capi.States.overlap_series)
    import py_monte_carlo
    from pyisingmontecarlo_amd.tempering import ClassicalTempering
    for cls in (py_monte_carlo.ClassicIsing, ClassicalTempering):
        for name in ("set_measure_overlaps_every", "get_measured_overlaps", "reset_measured_overlaps"):
            assert hasattr(cls, name)


def test_ladder_refusals_without_a_device():
    from pyisingmontecarlo_amd.tempering import ClassicalTempering

    edges = (np.array([0, 1], dtype=np.uint64), np.array([1, 2], dtype=np.uint64), np.array([1.0, -1.0]))
    single = ClassicalTempering(edges, seed=1)
    with pytest.raises(ValueError, match="copies=2"):
        single.set_measure_overlaps_every(3)
    with pytest.raises(ValueError, match="copies=2"):
        ClassicalTempering(edges, seed=1, devices=[0, 0]).set_measure_overlaps_every(3)
    pair = ClassicalTempering(edges, seed=1, copies=2)
    with pytest.raises(ValueError, match="negative"):
        pair.set_measure_overlaps_every(-1)
    with pytest.raises(ValueError, match="set_measure_overlaps_every"):
        pair.get_measured_overlaps()

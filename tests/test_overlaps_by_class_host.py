"""The host halves of the overlap by site class, no GPU: the segment construction the library's own
isingmc_site_classes_create calls (isingmc_host_class_segments) against its restatement in tests/class_overlap_reference.py, and
the numpy module that turns plane overlaps into chi_SG(k) and xi_L against closed forms."""
import numpy as np
import pytest

import class_overlap_reference as CR
from pyisingmontecarlo_amd import correlation as K


def _segment_case():
    """4096 positions over 3700 sites in scrambled order (396 padding positions); one table with a class of 2500 positions (three
    segments), a class of one site, an empty class, a class of 1024 positions (exactly one full segment), NO_CLASS sites and the
    rest in class 0; a second table of random classes, so that `first` carries on behind the first table's positions."""
    rng = np.random.default_rng(17)
    n_pos, nvars, n_classes = 4096, 3700, 6
    site = np.full(n_pos, CR.PAD_SITE, dtype=np.uint32)
    site[rng.permutation(n_pos)[:nvars]] = rng.permutation(nvars)
    t0 = np.zeros(nvars, dtype=np.uint32)
    ids = rng.permutation(nvars)
    t0[ids[:2500]] = 1
    t0[ids[2500]] = 2                 # one site; class 3 stays empty
    t0[ids[2501:3525]] = 4
    t0[ids[3525:3600]] = CR.NO_CLASS
    t1 = rng.integers(0, n_classes, nvars).astype(np.uint32)
    t1[rng.random(nvars) < 0.1] = CR.NO_CLASS
    return site, np.stack([t0, t1]), n_classes


def test_class_segments_against_the_restatement(capi):
    site, tables, n_classes = _segment_case()
    order, seg, sizes = capi.class_segments(site, tables, n_classes)
    want_order, want_seg = CR.class_segments(site, tables, n_classes)
    assert np.array_equal(order, want_order) and np.array_equal(seg, want_seg)
    assert np.array_equal(sizes, CR.class_sizes(tables, n_classes))
    assert [int(n) for n in sizes[0]] == [3700 - 2500 - 1 - 1024 - 75, 2500, 1, 0, 1024, 0]
    # the properties the kernel relies on, stated without the restatement
    real = np.flatnonzero(site != CR.PAD_SITE)
    for t, cls in enumerate(tables):
        mine = seg[seg[:, 0] == t]
        covered = np.concatenate([order[f:f + n] for _, _, f, n in mine])
        classed = real[cls[site[real]] != CR.NO_CLASS]
        assert np.array_equal(np.sort(covered), classed)          # every classed, non-padding position exactly once
        for _, c, f, n in mine:
            assert 1 <= n <= CR.SEGMENT_MAX and np.all(cls[site[order[f:f + n]]] == c)   # one class, at most a workgroup's positions
    assert [int(n) for t, c, f, n in seg if t == 0 and c == 1] == [1024, 1024, 452]
    assert [int(n) for t, c, f, n in seg if t == 0 and c == 4] == [1024] and not np.any((seg[:, 0] == 0) & (seg[:, 1] == 3))
    assert np.array_equal(seg[:, 2], np.concatenate([[0], np.cumsum(seg[:-1, 3])]))   # the segments tile `order`


def test_class_segments_refusals(capi):
    site = np.arange(8, dtype=np.uint32)
    ok = np.zeros((1, 8), dtype=np.uint32)
    with pytest.raises(ValueError, match="class value out of range"):
        capi.class_segments(site, np.full((1, 8), 3, dtype=np.uint32), 3)
    with pytest.raises(ValueError, match=r"n_classes must be 1 \.\. 4096"):
        capi.class_segments(site, ok, 4097)
    with pytest.raises(ValueError, match=r"n_tables must be 1 \.\. 8"):
        capi.class_segments(site, np.zeros((9, 8), dtype=np.uint32), 1)
    with pytest.raises(ValueError, match="must not exceed 8192"):
        capi.class_segments(site, np.zeros((3, 8), dtype=np.uint32), 4096)
    with pytest.raises(ValueError, match="site table entry out of range"):
        capi.class_segments(np.full(8, 8, dtype=np.uint32), ok, 1)
    order, seg, sizes = capi.class_segments(site, np.full((1, 8), CR.NO_CLASS, dtype=np.uint32), 2)   # nothing classed: nothing to count
    assert len(order) == 0 and len(seg) == 0 and not sizes.any()


def test_plane_classes_are_the_coordinates():
    got = K.plane_classes((3, 4, 5))
    assert got.dtype == np.uint32 and got.shape == (3, 60)
    assert np.array_equal(got, np.indices((3, 4, 5)).reshape(3, -1))
    site = np.ravel_multi_index((2, 1, 3), (3, 4, 5))
    assert list(got[:, site]) == [2, 1, 3]


def test_chi_sg_closed_forms():
    L, N, c, A = 12, 12 * 7, 5.0, 3.0
    x = np.arange(L)
    const = K.chi_sg(np.full(L, c), N)
    assert const[0] == pytest.approx(L * L * c * c / N, rel=1e-14) and np.allclose(const[1:], 0.0, atol=1e-12)
    delta = K.chi_sg(np.eye(L)[4], N)
    assert np.allclose(delta, 1.0 / N, rtol=1e-13, atol=0.0)
    wave = K.chi_sg(A * np.cos(2 * np.pi * x / L), N)
    assert wave[1] == pytest.approx(A * A * L * L / (4 * N), rel=1e-13) and wave[L - 1] == pytest.approx(A * A * L * L / (4 * N), rel=1e-13)
    assert np.allclose(np.delete(wave, [1, L - 1]), 0.0, atol=1e-12)
    stacked = K.chi_sg(np.stack([np.full(L, c), np.eye(L)[4]]), N)   # leading axes are kept
    assert stacked.shape == (2, L) and np.array_equal(stacked[0], const) and np.array_equal(stacked[1], delta)


@pytest.mark.parametrize("L,xi,n", [(8, 0.7, 1), (16, 3.25, 1), (64, 40.0, 1), (16, 3.25, 2)])
def test_correlation_length_inverts_ornstein_zernike(L, xi, n):
    chi0 = 37.5
    k = 2 * np.pi * n / L
    chik = chi0 / (1.0 + 4.0 * xi * xi * np.sin(k / 2) ** 2)
    assert abs(K.correlation_length(chi0, chik, L, n) - xi) < 1e-12

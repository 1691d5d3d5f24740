"""The step chooser of population annealing on the host: isingmc_host_pa_choose_step against the restatement of
tests/pa_adaptive_reference.py -- k, the f64 bits of dbeta, S and N as integers -- on synthetic energy arrays, and the refusals."""
import struct

import numpy as np
import pytest

import pa_adaptive_reference as PAA


def _bits(x):
    return struct.pack("<d", float(x))


def _check(capi, energies, dbeta_max, target):
    want = PAA.choose_step(energies, dbeta_max, target)
    got = capi.pa_choose_step(energies, dbeta_max, target)
    assert got["k"] == want["k"]
    assert _bits(got["dbeta"]) == _bits(want["dbeta"])
    assert got["sum"] == want["sum"] and got["num"] == want["num"]
    return want


def _gaussian(n, sigma, seed=5):
    """integer energies (few distinct values: the restatement takes one weight per level) with a Gaussian spread"""
    return np.rint(np.random.default_rng(seed).normal(-1000.0, sigma, n) / 4.0) * 4.0


def test_equal_energies_take_the_whole_step(capi):
    for n in (1, 2, 100):
        want = _check(capi, np.full(n, -37.5), 0.3, 0.85)
        assert want["k"] == 65536 and want["dbeta"] == 0.3 and want["sum"] == n << 32 and want["num"] == n * (n << 32)
        assert len(want["evaluated"]) == 16


def test_two_levels(capi):
    e = np.array([-10.0] * 30 + [-2.0] * 70)
    ks = set()
    for dbeta_max in (0.001, 0.1, 1.0, 1e6):   # (1e6 / 65536 times the gap of 8: the upper level has no weight left)
        for target in (0.5, 0.85, 0.99):
            ks.add(_check(capi, e, dbeta_max, target)["k"])
    assert 65536 in ks and 1 in ks and any(1 < k < 65536 for k in ks)


def test_gaussian_spread_inside_the_grid(capi):
    e = _gaussian(3000, 40.0)
    want = _check(capi, e, 0.1, 0.85)
    assert 1 < want["k"] < 65536
    # the answer is where the predicate turns: k holds, k + 1 does not (both were looked at by the search: k + 1 in the last
    # round, or as the candidate that ended an earlier one)
    by_k = {c["k"]: c for c in want["evaluated"]}
    assert by_k[want["k"]]["holds"] and not by_k[want["k"] + 1]["holds"]
    assert PAA.overlap(want, len(e)) >= 0.85


def test_a_spread_too_wide_for_any_step(capi):
    e = np.arange(4000) * 1.0e9
    want = _check(capi, e, 1.0, 0.85)
    assert want["k"] == 1
    W = want["sum"] - (1 << 32)
    assert W == 0, "every weight but the reference's is zero"
    assert want["num"] == want["sum"]   # min(S, R W) = S for the one replica with a weight


def test_one_replica(capi):
    want = _check(capi, np.array([12.0]), 2.5, 1.0)
    assert want["k"] == 65536 and want["sum"] == 1 << 32 and want["num"] == 1 << 32


def test_extreme_targets(capi):
    e = _gaussian(2000, 25.0, seed=9)
    one = _check(capi, e, 0.05, 1.0)
    assert one["k"] == 1   # only equal weights overlap completely
    assert PAA.target32(1.0) == 1 << 32
    tiny = _check(capi, e, 0.05, 1e-12)
    assert PAA.target32(1e-12) == 1 and tiny["k"] == 65536
    mid = _check(capi, e, 0.05, 0.85)
    assert one["k"] <= mid["k"] <= tiny["k"]


def test_the_numerator_on_both_sides_of_2_to_the_64(capi):
    """n = 2^17 + 33 and a small dbeta_max: R S is about 2^81 where the weights are near 2^32, so N passes 2^64 at the small
    candidates, while at the large ones of the first round almost every weight is zero and N stays below it.  Which side each
    evaluated candidate falls on is read off the restatement, not assumed."""
    n = (1 << 17) + 33
    e = _gaussian(n, 200.0, seed=17)
    want = _check(capi, e, 4.0, 0.85)
    nums = [c["num"] for c in want["evaluated"]]
    print(f"k {want['k']}, {sum(x >= 1 << 64 for x in nums)} of {len(nums)} evaluated candidates with N >= 2^64, min {min(nums):.3e}, max {max(nums):.3e}")
    assert any(x >= 1 << 64 for x in nums) and any(x < 1 << 64 for x in nums)


def test_refusals(capi):
    e = np.array([1.0, 2.0, 3.0])
    for dbeta_max in (0.0, -0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="dbeta_max"):
            capi.pa_choose_step(e, dbeta_max, 0.85)
    for target in (0.0, -0.5, 1.0000001, float("nan")):
        with pytest.raises(ValueError, match="target"):
            capi.pa_choose_step(e, 0.1, target)
    with pytest.raises(ValueError, match="at least one replica"):
        capi.pa_choose_step(np.zeros(0), 0.1, 0.85)
    with pytest.raises(ValueError, match="finite"):
        capi.pa_choose_step(np.array([1.0, float("inf")]), 0.1, 0.85)
    assert capi.pa_choose_step(e, 0.1, 1.0)["k"] >= 1   # the closed end of (0, 1]

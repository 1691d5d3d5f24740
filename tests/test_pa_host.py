"""The resampling rule of population annealing on the host: isingmc_host_pa_sources against the restatement of
tests/pa_reference.py (source table and weight sum, exactly) and the invariants of systematic resampling in exact arithmetic."""
from fractions import Fraction

import numpy as np
import pytest

import pa_reference as PA

SEED = 0x9E3779B97F4A7C15


def _check(capi, energies, dbeta, seed=SEED, step=3):
    src, total, eref = capi.pa_sources(seed, step, energies, dbeta)
    ref = PA.sources(seed, step, energies, dbeta)
    assert total == ref["sum"] and eref == ref["eref"]
    assert np.array_equal(src, ref["src"])
    # invariants, whatever the restatement says
    R = len(energies)
    W = ref["weights"]
    assert total == sum(W) and total >= 1 << 32 and max(W) == 1 << 32
    assert (np.diff(src.astype(np.int64)) >= 0).all()
    counts = np.bincount(src, minlength=R)
    assert counts.sum() == R
    # |n_r - R W_r / S| < 1 for every replica, in integers: |n_r S - R W_r| < S
    assert all(abs(int(c) * total - R * w) < total for c, w in zip(counts, W))
    r = int(np.argmax(counts))
    assert abs(int(counts[r]) - Fraction(R * W[r], total)) < 1
    return src, total


@pytest.mark.parametrize("R", [1, 2, 31, 32, 33, 1000, 100000])
@pytest.mark.parametrize("dbeta", [0.0, 1e-3, 0.05, 1.0, -0.05])
def test_random_energies(capi, oracle, R, dbeta):
    rng = np.random.default_rng(R)
    energies = -2.0 * rng.integers(0, 400, R).astype(np.float64) + (rng.normal(size=R) if R % 2 else 0.0)
    src, _ = _check(capi, energies, dbeta)
    if dbeta == 0.0:
        assert np.array_equal(src, np.arange(R))


def test_equal_energies_give_the_identity(capi, oracle):
    src, total = _check(capi, np.full(77, -123.5), 0.7)
    assert np.array_equal(src, np.arange(77)) and total == 77 << 32


def test_one_replica_far_below_takes_every_slot(capi, oracle):
    energies = np.full(100, -10.0)
    energies[41] = -1010.0
    src, total = _check(capi, energies, 1.0)
    assert (src == 41).all() and total == 1 << 32
    src, _ = _check(capi, energies, -1.0)   # heating: the reference is the maximum, the low replica alone dies out
    assert 41 not in src


def test_energies_of_the_largest_lattice_scale(capi, oracle):
    rng = np.random.default_rng(5)
    energies = -1.0e7 - 4.0 * rng.integers(0, 3000, 4096).astype(np.float64)
    _check(capi, energies, 1e-3)
    _check(capi, energies + 0.123456789, 2.5e-4)   # not representable steps: the subtraction rounds


def test_the_table_follows_seed_and_step(capi, oracle):
    energies = -2.0 * np.random.default_rng(2).integers(0, 30, 500).astype(np.float64)
    a, _ = _check(capi, energies, 0.05, step=1)
    b, _ = _check(capi, energies, 0.05, step=2)
    c, _ = _check(capi, energies, 0.05, step=1 + (1 << 32))
    d, _ = _check(capi, energies, 0.05, seed=SEED + 1, step=1)
    again, _ = _check(capi, energies, 0.05, step=1)
    assert np.array_equal(a, again)
    assert all(not np.array_equal(a, x) for x in (b, c, d))


def test_bad_arguments(capi):
    with pytest.raises(ValueError):
        capi.pa_sources(1, 0, np.zeros(0), 0.1)
    with pytest.raises(ValueError):
        capi.pa_sources(1, 0, np.zeros(4), float("nan"))
    with pytest.raises(ValueError):
        capi.pa_sources(1, 0, np.array([0.0, float("inf")]), 0.1)


def test_gathers_of_the_restatement():
    """A self-check of the test infrastructure (tests/pa_reference.py alone, no library code): the two gathers the GPU tests
    compare the device words with, against a bit-by-bit statement of what they should do."""
    rng = np.random.default_rng(0)
    rows = rng.integers(0, 1 << 32, (5, 8), dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(PA.row_gather(rows, [4, 4, 0, 1, 1]), rows[[4, 4, 0, 1, 1]])
    words = rng.integers(0, 1 << 32, (3, 64), dtype=np.uint64).astype(np.uint32)
    R = 70
    src = rng.integers(0, R, R)
    pad = np.zeros(64, dtype=bool)
    pad[60:] = True
    out = PA.bit_gather(words, src, pad)
    bits = lambda w, s: (w[s // 32] >> np.uint32(s % 32)) & 1   # noqa: E731
    for j in range(96):
        want = bits(words, src[j]) if j < R else bits(words, j)
        assert np.array_equal(bits(out, j)[:60], want[:60])
        assert np.array_equal(bits(out, j)[60:], bits(words, j)[60:])


# ---- the vectorised restatement (sources_fast, bit_gather_fast) and the host rule at the populations it makes affordable ---
def _energies(kind, R):
    rng = np.random.default_rng(R)
    if kind == "equal":
        return np.full(R, -123.5)
    if kind == "binomial":
        return -512.0 + 4.0 * rng.binomial(128, 0.3, R)
    return -300.0 + 25.0 * rng.normal(size=R)   # not integers: the subtraction and the product round


def _same_table(fast, slow):
    for name in ("sum", "eref", "distinct", "mean_energy"):
        assert fast[name] == slow[name], name
    assert np.array_equal(fast["src"], slow["src"]) and fast["src"].dtype == slow["src"].dtype
    assert fast["weights"].tolist() == slow["weights"]


@pytest.mark.parametrize("R", [1, 2, 31, 32, 33, 64, 1000, 2000])
@pytest.mark.parametrize("dbeta", [0.0, 0.05, 1.0, -0.05, -1.0])
def test_fast_sources_equal_the_definition(oracle, R, dbeta):
    for kind in ("equal", "binomial", "real"):
        e = _energies(kind, R)
        fast = PA.sources_fast(SEED, 5, e, dbeta)
        _same_table(fast, PA.sources(SEED, 5, e, dbeta))
        assert not fast["needs_high_words"] and fast["low_word_carries"] == 0


@pytest.mark.parametrize("R", [32, 33, 63, 64, 65, 95, 1000, 2000])   # the last group owns R % 32 in {0, 1, 31, 8, 16} bits
def test_fast_bit_gather_equals_the_definition(R):
    rng = np.random.default_rng(R)
    groups, n_pos = (R + 31) // 32, 24
    words = rng.integers(0, 1 << 32, (groups, n_pos), dtype=np.uint64).astype(np.uint32)
    pad = np.zeros(n_pos, dtype=bool)
    pad[[3, 20, 23]] = True
    for src in (rng.integers(0, R, R), np.sort(rng.integers(0, R, R)), np.arange(R)[::-1], (np.arange(R) * 2654435761) % R):
        assert np.array_equal(PA.bit_gather_fast(words, src, pad), PA.bit_gather(words, src, pad))
        assert np.array_equal(PA.bit_gather_fast(words, src), PA.bit_gather(words, src))
    assert np.array_equal(PA.bit_gather_fast(words, np.arange(R), pad), words)


LARGE = [(65535, "equal", 0.7), (65535, "binomial", -0.05), (65535, "real", 0.05),
         (65536, "equal", 0.7), (65536, "equal", -0.7), (65536, "binomial", 0.05), (65536, "real", -0.05),
         ((1 << 20) + 1025, "equal", -0.7), ((1 << 20) + 1025, "binomial", 0.05), ((1 << 20) + 1025, "binomial", -0.05),
         ((1 << 20) + 1025, "real", 0.002), ((1 << 20) + 1025, "real", -0.002)]


@pytest.mark.parametrize("R,kind,dbeta", LARGE)
def test_host_rule_at_the_populations_with_high_words(capi, oracle, R, kind, dbeta):
    """isingmc_host_pa_sources against sources_fast on both sides of R S = 2^64.  What the case reaches is certified by the
    restatement: below R = 65 536 no product reaches 2^64; R = 65 536 reaches it with equal energies alone (S = R 2^32, the low
    words of j S are multiples of 2^48 and never carry); at 2^20 + 1025 every case reaches it, and where the mean weight is large
    (equal energies, |dbeta| = 0.002) the low word of j S + u carries at some slots."""
    e = _energies(kind, R)
    want = PA.sources_fast(SEED, 3, e, dbeta)
    src, total, eref = capi.pa_sources(SEED, 3, e, dbeta)
    assert total == want["sum"] and eref == want["eref"] and eref == (e.min() if dbeta >= 0 else e.max())
    assert np.array_equal(src, want["src"])
    print(f"R {R} {kind} dbeta {dbeta}: S / (R 2^32) = {want['sum'] / (R << 32):.5f}, distinct {want['distinct']}, "
          f"high words {want['needs_high_words']}, low-word carries {want['low_word_carries']}")
    assert want["needs_high_words"] == (R > 65536 or (R == 65536 and kind == "equal"))
    if kind == "equal":
        assert np.array_equal(src, np.arange(R)) and total == R << 32 and want["distinct"] == R
    if R > 65536 and (kind == "equal" or abs(dbeta) == 0.002):
        assert want["low_word_carries"] > 0
    else:
        assert R > 65536 or want["low_word_carries"] == 0

"""Host side of tests/test_gpu_real_variants.py: the exact reference agrees with the oracle, every graph builder of
tests/real_reference.py has the eligibility, heavy sites, degrees, slot count and colour classes its GPU test relies on, and
oracle engine E stays within the derived energy bound of the exact Hamiltonian on exactly those graphs."""
from fractions import Fraction

import numpy as np
import pytest

import real_reference as RR

GRAPHS = {g.name: g for g in RR.all_graphs()}


def _small_graph(rng, n, m, dyadic):
    ea, eb = rng.integers(0, n, m).astype(np.uint64), rng.integers(0, n, m).astype(np.uint64)
    ea[:2], eb[:2] = [1, 2], [1, 3]                  # a self-loop for sure ...
    ea[2:4], eb[2:4] = [3, 2], [2, 3]                # ... and one bond three times, in both orientations
    ej = rng.integers(-16, 17, m) / 8.0 if dyadic else rng.normal(size=m)
    h = rng.integers(-16, 17, n) / 8.0 if dyadic else rng.normal(size=n)
    return ea, eb, ej, h


def test_exact_energy_by_hand():
    ea, eb = np.array([0, 1, 1, 2], dtype=np.uint64), np.array([1, 0, 1, 2], dtype=np.uint64)   # a doubled bond, two self-loops
    ej = np.array([0.1, 1e-50, 1e39, -0.25])
    h = np.array([0.5, -3.0, 0.0])
    want = -Fraction(0.1) - Fraction(1e-50) + Fraction(1e39) - Fraction(0.25) - (Fraction(0.5) + Fraction(3.0))
    assert RR.exact_energy(ea, eb, ej, 3, [1, 0, 1], h) == want
    assert RR.exact_energy(ea, eb, ej, 3, [1, 1, 1]) == Fraction(0.1) + Fraction(1e-50) + Fraction(1e39) - Fraction(0.25)


def test_exact_energy_against_the_oracle(oracle):
    """<= 16 spins, self-loops and repeated bonds: equal to oracle.energy when every partial sum is exact in f64 (multiples of
    1/8), within (terms) u sum|terms| of it on Gaussian couplings; the sign convention is the project's"""
    rng = np.random.default_rng(2)
    for trial in range(8):
        n = int(rng.integers(2, 17))
        m = int(rng.integers(4, 40))
        for dyadic in (True, False):
            ea, eb, ej, h = _small_graph(rng, max(n, 4), m, dyadic)
            n_ = max(n, 4)
            for biases in (None, h):
                for _ in range(4):
                    spins = rng.integers(0, 2, n_).astype(np.uint8)
                    e = RR.exact_energy(ea, eb, ej, n_, spins, biases)
                    ref = Fraction(oracle.energy(ea, eb, ej, n_, spins, biases))
                    if dyadic:
                        assert e == ref
                    else:
                        assert abs(e - ref) <= (m + n_) * RR.U * Fraction(float(np.abs(ej).sum() + np.abs(h).sum()))


def test_energy_bound_by_hand():
    # F = (1.5 + 0.25, 1.5 + 0.75 + 3, 0.75): Fmax = 5.25, kE = 2 + 2 - 30; three terms + three sites; one self-loop
    ea, eb = np.array([0, 1, 2], dtype=np.uint64), np.array([1, 2, 2], dtype=np.uint64)
    ej, h = np.array([1.5, -0.75, 0.3]), np.array([0.25, -3.0, 0.0])
    assert RR.energy_log2(ea, eb, ej, 3, h) == -26
    q, u = Fraction(1, 2 ** 51), RR.U
    assert RR.energy_bound(ea, eb, ej, 3, h) == 5 * q + (2 * u + u * u) * (Fraction(5.5) + 5 * q) + u / (1 - u) * Fraction(0.3)
    assert RR.energy_log2(ea, eb, ej, 3) == -27                      # Fmax = 2.25
    assert RR.energy_bound(ea[:2], eb[:2], ej[:2], 3) == 2 * q / 2 + (2 * u + u * u) * (Fraction(2.25) + 2 * q / 2)


def test_energy_levels_are_what_the_bound_assumes(capi, oracle):
    """kE as derived here equals the library's and the oracle's; both levels rebuild every term to half a lo quantum"""
    for g in GRAPHS.values():
        kE = RR.energy_log2(g.ea, g.eb, g.ej, g.nvars, g.biases)
        lev = oracle.rj_energy_levels(g.ea, g.eb, g.ej, g.nvars, g.biases)
        assert kE == lev[0] == capi.rj_energy_levels(g.ea, g.eb, g.ej, g.nvars, g.biases)[0]
        q = Fraction(2) ** (kE - 25)
        for x, hi, lo in zip(g.ej[:200], lev[1], lev[2]):
            assert abs(Fraction(float(x)) - (int(hi) * 4 * q * 2 ** 23 + int(lo) * 2 * q)) <= q
        assert np.abs(lev[2]).max() <= 2 ** 23 and np.abs(lev[2]).max() > 0     # non-dyadic couplings: the lo level is in use


@pytest.mark.parametrize("name", list(GRAPHS))
def test_builder_shapes(capi, oracle, name):
    g = GRAPHS[name]
    kind, slots, bias, heavy = name.rsplit("-", 3)
    odd, slots, bias, heavy = kind == "odd-cycle", int(slots), bias == "bias", heavy == "heavy"
    assert g.nvars == RR.N_SITES == 1302 and (g.biases is not None) == bias and g.scale == RR.SCALE
    assert not np.any(g.ea == g.eb)
    lo, hi = np.minimum(g.ea, g.eb), np.maximum(g.ea, g.eb)
    assert len(np.unique(lo * np.uint64(g.nvars) + hi)) == len(g.ea)            # no bond twice
    assert (g.ea < g.eb).any() and (g.ea > g.eb).any()
    # degrees: 0, 1, and SLOTS exactly -- the last ELL slot is in use
    deg = RR.degrees(g)
    assert deg[RR.ISOLATED] == 0 and deg[RR.LEAF_EVEN] == 1 and deg[RR.LEAF_ODD] == 1
    assert deg.max() == slots == RR.slots_for(int(deg.max())) and deg[RR.HUB] == slots
    if bias:
        assert g.biases[RR.ISOLATED] != 0.0 and np.all(g.biases != 0.0)
    # colours: by parity, or with the one equal-parity bond a third class of one site
    colours = RR.greedy_colours(g)
    nc, colours_oracle, _ = oracle.gen_colouring(g.ea, g.eb, g.ej, g.nvars)
    nc_lib, colours_lib = capi.colour_graph(g.ea, g.eb, g.nvars)
    assert np.array_equal(colours, colours_oracle) and np.array_equal(colours, colours_lib) and nc == nc_lib
    parity = (np.arange(g.nvars) % 2).astype(np.uint32)
    if odd:
        assert nc == 3 and RR.class_sizes(colours) == [651, 650, 1] and colours[RR.ODD_BOND[1]] == 2
        assert np.array_equal(np.delete(colours, RR.ODD_BOND[1]), np.delete(parity, RR.ODD_BOND[1]))
        assert RR.ODD_BOND[0] % 2 == RR.ODD_BOND[1] % 2
    else:
        assert nc == 2 and np.array_equal(colours, parity) and RR.class_sizes(colours) == [651, 651]
        assert np.all((g.ea + g.eb) % 2 == 1)
    # 768 positions per big class: 3 / 6 / 12 blocks of 256 / 128 / 64 threads; the sites end inside the 3rd / 6th / 11th
    per_block = RR.THREADS[slots]
    assert RR.blocks_per_class(colours, slots)[:2] == [768 // per_block] * 2 and 651 % per_block != 0
    assert (651 + per_block - 1) // per_block == {256: 3, 128: 6, 64: 11}[per_block]       # blocks that hold sites
    # the family takes the graph; heavy sites and their shifts
    assert oracle.rj_eligible(g.ea, g.eb, g.ej, g.nvars, g.biases)
    k, jq, hq, d = oracle.rj_quantise(g.ea, g.eb, g.ej, g.nvars, g.biases)
    k_lib, _, _, d_lib, ok = capi.rj_quantise(g.ea, g.eb, g.ej, g.nvars, g.biases)
    assert ok and k == k_lib and np.array_equal(d, d_lib)
    shifts = {int(i): int(d[i]) for i in np.flatnonzero(d)}
    if not heavy:
        assert shifts == {}
    else:
        a, b = RR.HEAVY_BOND
        c = RR.HEAVY_BOND2[1]
        want = {a, b, c} | ({RR.PIN_UP, RR.PIN_DOWN} if bias else set())
        assert set(shifts) == want
        assert shifts[b] == shifts[a] + 1 and shifts[c] < shifts[a]              # the two ends of the big bond: different shifts
        assert colours[a] != colours[b]
        if bias:
            assert colours[RR.PIN_UP] != colours[RR.PIN_DOWN] and g.biases[RR.PIN_UP] > 0 > g.biases[RR.PIN_DOWN]
            assert shifts[RR.PIN_UP] > shifts[b] > shifts[RR.PIN_DOWN]
            assert 5e5 < g.biases[RR.PIN_UP] / g.scale < 2e6 and 1e3 < -g.biases[RR.PIN_DOWN] / g.scale < 1e4
        # the betas of the GPU tests put a heavy site's shift on both sides of the acceptance scale's within one launch
        sh = [oracle.rj_beta(beta / g.scale, k)[0] for beta in (1e-7, 3.0)]
        assert sh[0] >= max(shifts.values()) and sh[1] < min(shifts.values())
    assert kind in ("bipartite", "odd-cycle")


@pytest.mark.parametrize("name", list(GRAPHS))
def test_engine_e_energies_within_bound(oracle, name):
    """the reference alone satisfies the bound on the inputs of the GPU tests: all up, all down, the parity pattern, random
    configurations, and the configurations of a run at the GPU tests' schedule"""
    g = GRAPHS[name]
    bound = RR.energy_bound(g.ea, g.eb, g.ej, g.nvars, g.biases)
    ex = RR.Exact(g.ea, g.eb, g.ej, g.nvars, g.biases)
    rng = np.random.default_rng(1)
    configs = [np.ones(g.nvars, dtype=np.uint8), np.zeros(g.nvars, dtype=np.uint8), (np.arange(g.nvars) % 2 == 0).astype(np.uint8)]
    configs += [rng.integers(0, 2, g.nvars).astype(np.uint8) for _ in range(5)]
    worst = Fraction(0)
    for spins in configs:
        worst = max(worst, abs(Fraction(oracle.rj_energy(g.ea, g.eb, g.ej, g.nvars, spins, g.biases)) - ex.energy(spins)))
    betas = [b / g.scale for b in (0.0, -0.3, 30.0, 0.7)]
    seeds = oracle.make_seeds(77, 5)
    spins, eps = RR.oracle_trajectory(oracle, g, seeds, len(betas), betas=betas)
    e_run, s_run, eps_run = oracle.rj_run(g.ea, g.eb, g.ej, g.nvars, seeds, len(betas), betas=betas, biases=g.biases, per_step=True)
    assert np.array_equal(spins[-1], s_run) and np.array_equal(eps, eps_run) and np.array_equal(eps[:, -1], e_run)
    for r in range(5):
        for t in range(len(betas)):
            worst = max(worst, abs(Fraction(float(eps[r, t])) - ex.energy(spins[t, r])))
    assert worst <= bound, (name, float(worst), float(bound))
    assert bound < Fraction(1, 10 ** 9) * Fraction(float(np.abs(g.ej).sum()))    # and the bound itself means something

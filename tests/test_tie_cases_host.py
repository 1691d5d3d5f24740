"""The searched high-tie quads (tests/golden/tie_cases.json, written by tests/golden/make_tie_cases.py) on the CPU.

A tie draws 32 more bits from call 7 + n / 4, word n % 4; random inputs reach the fifth tie of a quad a few times in a
thousand quads and the ninth about once in a million, so the refill calls 8, 9, ... of the sweeps are reached only by cases
that were searched for.  Here: every fixture record recounted with tests/tie_reference.py, the conditions the fixture must meet,
and the oracle's own tie numbering (engines B and D) against that independent restatement on the fixture's quads."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tie_cases as TC  # noqa: E402
import tie_reference as TR  # noqa: E402

LATS, PKSW = TC.load("LATS"), TC.load("PKSW")


@pytest.mark.parametrize("case", LATS + PKSW, ids=TC.case_id)
def test_fixture_record_recounted(case):
    """One class for all 128 spins at the case's beta: the same number of ties, in the same (word, bit) order, and the
    highest call is 7 + (n - 1) / 4."""
    dE = 8.0 if case["domain"] == "LATS" else 12.0
    assert case["colour"] == 0
    beta, T = TC.beta_and_threshold(case, dE)
    flips, ties, highest = TR.class_pass(case["domain"], case["seed"], case["t"], 0, case["Q"], [T], [0] * 128)
    assert len(ties) == case["n_ties"]
    assert [list(t) for t in ties] == case["ties"]
    assert highest == 7 + (case["n_ties"] - 1) // 4
    assert case["t"] + 3 < 2 ** 48 and case["Q"] < 64
    assert all(f in (0, 1) for f in flips) and len(flips) == 128


@pytest.mark.parametrize("cases", [LATS, PKSW], ids=["LATS", "PKSW"])
def test_fixture_conditions(cases):
    counts = [c["n_ties"] for c in cases]
    for n in (4, 5, 8, 9):                                             # the branch boundary and the refill boundary
        assert n in counts
    assert sum(n >= 9 for n in counts) >= 4
    assert any(c["t"] >= 2 ** 32 and (c["t"] >> 32) & 0xFFFF and c["n_ties"] >= 9 for c in cases)
    assert sum(max(0, n - 4) for n in counts) >= 40                    # ties of index >= 4: drawn from calls 8 and later
    assert sum(max(0, n - 8) for n in counts) >= 8                     # ties of index >= 8: calls 9 and later
    # the first tie beyond each boundary (the 5th: call 8, the 9th: call 9) must fall differently from what word 3 or word 0
    # of the previous call would give it, so that a kernel which stays in the previous call there cannot escape by chance
    for n in (5, 9):
        c = next(c for c in cases if c["n_ties"] == n)
        lo = TC.beta_and_threshold(c, 8.0 if cases is LATS else 12.0)[1] & 0xFFFFFFFF
        own, prev = (TR.call(c["domain"], c["seed"], c["t"], 0, c["Q"], 7 + (n - 1) // 4 - k) for k in (0, 1))
        assert (own[0] < lo) != (prev[3] < lo) and (own[0] < lo) != (prev[0] < lo)
    if cases is LATS:
        assert any(c["Q"] == 0 and c["n_ties"] >= 9 for c in cases)    # exists in 64 x 8
        assert any(c["Q"] == 1 and c["n_ties"] >= 9 for c in cases)    # ... and its second quad
        assert len(TC.load("LATS", colour=1)) >= 2                     # the second colour
        assert any(1 <= c["Q"] <= 6 and c["n_ties"] >= 10 for c in cases)  # an interior row of 256 x 8
    else:
        assert all(c["Q"] < 64 for c in cases)                         # a leader of block 0


def _lattice_oracle_quad(oracle, exact, W, H, mode, case):
    sysm = TC.LatticeSystem(exact, W, H, mode)
    beta, flips, ties, _ = sysm.first_pass(case)
    lat = sysm.oracle_lat(oracle)
    st = lat.pack(sysm.start)
    before = sysm.quad_bits(st, case["Q"])
    lat.sweep(st, case["seed"], case["t"], beta)
    after = sysm.quad_bits(st, case["Q"])                              # plane 0 is final after the colour-0 pass
    return [a ^ b for a, b in zip(before, after)], flips, ties


@pytest.mark.parametrize("mode", ["ferro", "mattis"])
@pytest.mark.parametrize("case", [c for c in LATS if c["Q"] < 2], ids=TC.case_id)
def test_oracle_lattice_sweep_against_tie_reference(oracle, exact, mode, case):
    """64 x 8 (quads 0 and 1 per plane), uniform J < 0 from the all-up start and a Mattis-gauged +-J lattice from s = eps."""
    got, flips, ties = _lattice_oracle_quad(oracle, exact, 64, 8, mode, case)
    assert [list(t) for t in ties] == case["ties"]
    assert got == flips


@pytest.mark.parametrize("mode", ["field", "field_signs", "open", "open_field", "aniso"])
@pytest.mark.parametrize("case", [c for c in LATS if 1 <= c["Q"] <= 6], ids=TC.case_id)
def test_oracle_multi_class_sweep_against_tie_reference(oracle, exact, mode, case):
    """256 x 8, the quad an interior row: the classes of the field, +-h, open, open + field and anisotropic lattices."""
    got, flips, ties = _lattice_oracle_quad(oracle, exact, 256, 8, mode, case)
    assert len(ties) >= 9
    assert got == flips


@pytest.mark.parametrize("case", PKSW, ids=TC.case_id)
def test_oracle_packed_engine_against_tie_reference(oracle, exact, case):
    """Engine D on the 8^3 cubic ferromagnet, all 32 replicas of the group started all-up, the case's seed on replica 0."""
    sysm = TC.PackedSystem(exact, oracle)
    beta, flips, ties, _ = sysm.first_pass(case)
    assert [list(t) for t in ties] == case["ties"]
    start = np.tile(sysm.start, (32, 1))
    _, after = oracle.pk_run(sysm.ea, sysm.eb, sysm.ej, sysm.nvars, TC.seeds_for(case, 32), 1, betas=[beta], states=start.copy(), t0=case["t"])
    got = [a ^ b for a, b in zip(sysm.quad_bits(start, case["Q"]), sysm.quad_bits(after, case["Q"]))]
    assert got == flips                                                # class 0's sites are final after class 0's pass


@pytest.mark.parametrize("case", TC.diluted_cases(PKSW), ids=TC.case_id)
def test_diluted_cases_keep_nine_ties_over_two_rows(oracle, exact, case):
    """The cases the diluted GPU row uses: cutting bonds at the two words with the fewest ties leaves >= 9 ties, at least
    one of them at a site of lower degree (another row of the threshold table), and engine D agrees with the reference."""
    sysm = TC.diluted(exact, oracle, case)
    beta, flips, ties, highest = sysm.first_pass(case)
    assert len(ties) >= 9 and highest >= 9
    assert len(TC.tie_rows(sysm, case, ties)) >= 2
    start = np.tile(sysm.start, (32, 1))
    _, after = oracle.pk_run(sysm.ea, sysm.eb, sysm.ej, sysm.nvars, TC.seeds_for(case, 32), 1, betas=[beta], states=start.copy(), t0=case["t"])
    assert [a ^ b for a, b in zip(sysm.quad_bits(start, case["Q"]), sysm.quad_bits(after, case["Q"]))] == flips


@pytest.mark.parametrize("W,H", [(64, 8), (1024, 256)])
@pytest.mark.parametrize("mode", ["ferro", "mattis"])
@pytest.mark.parametrize("case", TC.load("LATS", colour=1), ids=TC.case_id)
def test_oracle_second_colour_against_tie_reference(oracle, exact, W, H, mode, case):
    """The cases searched for colour 1 at the prefix value 0: the classes of the colour-1 spins come from what the colour-0
    pass left (final after the timestep).  On 1024 x 256, the shape of the GPU row, >= 9 ties must be left."""
    sysm = TC.LatticeSystem(exact, W, H, mode)
    beta = TC.beta_and_threshold(case, sysm.bulk_dE())[0]
    lat = sysm.oracle_lat(oracle)
    st = lat.pack(sysm.start)
    before = sysm.quad_bits(st, case["Q"], 1)
    lat.sweep(st, case["seed"], case["t"], beta)
    _, flips, ties, highest = sysm.second_pass(case, lat.unpack(st))
    assert W == 64 or (len(ties) >= 9 and highest >= 9)
    assert [a ^ b for a, b in zip(before, sysm.quad_bits(st, case["Q"], 1))] == flips

"""The strip-ladder census (tests/test_gpu_strip_ladder.py) without a GPU: every case of tests/strip_ladder_reference.py selects
the instantiation of lat_strip_kernel<PMJ, NW, LAD = true> it claims, by the restated strip_plan and in_kernel rules alone, and the
oracle-backed twin's rounds are not vacuous -- they hold accepted and refused pairs on both sides of d = 0 and beyond d = -40,
an accepted swap in every ladder, a refused one in every long ladder, a completed round trip.  These are conditions on the
committed betas, not measurements: the betas were chosen so that the reference alone meets them."""
import numpy as np
import pytest

import strip_ladder_reference as R

CASES = pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])


# ---- the restated rules ---------------------------------------------------------------------------------------------------------------
def test_strip_plan_restated():
    for nw, shapes in R.SHAPES.items():
        for (W, H), qpr, S, strips in shapes:
            assert R.strip_plan(W, H, nw) == (qpr, S, strips)
            assert S * qpr == 64 * nw and S * strips == H   # a strip is 64 nw quads per colour; the strips tile the lattice
            assert R.strip_plan(W, S, nw) is None           # one strip
            assert R.strip_plan(W, H + 1, nw) is None       # strips that do not divide the rows
    for args, want in R.STRIP_PLAN_CASES:
        assert R.strip_plan(*args) == want, args


def test_in_kernel_condition_restated():
    assert len(R.IN_KERNEL_CASES) == 13
    for args, want in R.IN_KERNEL_CASES:
        assert R.rounds_inside_the_launch(*args) == want, args


# ---- every case selects what it claims ----------------------------------------------------------------------------------------------
@CASES
def test_case_selects_its_instantiation(capi, case):
    shapes = {shape: rest for shape, *rest in R.SHAPES[case.nw]}
    qpr, S, strips = shapes[(case.W, case.H)]                  # no shape outside the table
    assert R.strip_plan(case.W, case.H, case.nw) == (qpr, S, strips)
    G = len(case.betas)
    assert G in (1, 2, 5, 8) and G * strips <= 8 * 3           # every workgroup of the launch is resident at once
    assert list(case.betas) == sorted(case.betas)
    # the call sequence: the first call's rounds are odd in number, one call holds >= 6 rounds inside its launch, both periods, a tail
    (T1, f1), (T2, f2) = R.calls(case)
    inside = [R.rounds_inside_the_launch(G, G, T, f) for T, f in R.calls(case)]
    assert inside == [T1 // f1 - 1, T2 // f2 - 1] and min(inside) >= 1 and max(inside) >= 6
    assert (T1 // f1) % 2 == 1 and {f1, f2} == {1, 3} and (T1 % f1 or T2 % f2) and R.warm_up(case) >= 1
    # PMJ: what the library's own recognition makes of the edge list (host code)
    J, glass = R.COUPLINGS[case.coupling]
    info = capi.recognise_lattice2d(*R.edges(case), case.W * case.H)
    assert info["is_lattice"] and (info["width"], info["height"]) == (case.W, case.H)
    assert info["jabs"] == abs(J) and info["uniform_sign"] == (not glass)
    assert R.instantiation(case) == (glass, case.nw)
    if glass:
        ej = R.edges(case)[2]
        assert (ej > 0).any() and (ej < 0).any()


def test_census_is_covered():
    """every instantiation gets every rung count, both periods, a ladder with a beta gap and a fallback case; every shape a
    ferromagnet and a glass; all four couplings occur"""
    for inst in R.INSTANTIATIONS:
        mine = [c for c in R.CASES if R.instantiation(c) == inst]
        assert {len(c.betas) for c in mine} == {1, 2, 5, 8}
        assert {f for c in mine for _, f in R.calls(c)} == {1, 3}
        assert sum(c.fallback for c in mine) >= 1
        assert any(len(c.betas) % 8 for c in mine if len(c.betas) == 5)   # 5 rungs: blocks map to strips without the XCD remap
    for nw, shapes in R.SHAPES.items():
        for shape, *_ in shapes:
            here = {c.coupling for c in R.CASES if c.nw == nw and (c.W, c.H) == shape}
            assert here & {"fm", "half"} and "glass" in here, (nw, shape)
    assert {c.coupling for c in R.CASES} == set(R.COUPLINGS)
    assert len({c.seed for c in R.CASES}) == len(R.CASES)


# ---- the twin's rounds are not vacuous ----------------------------------------------------------------------------------------------
@CASES
def test_twin_ladder(oracle, case):
    tw = R.twin(case)
    G, last = len(case.betas), tw.after[-1]
    assert R.contains(tw) == case.contains                     # the counts written above the betas
    n = R.counts(tw.pairs)
    rounds = [T // f for T, f in R.calls(case)]
    assert [a.round for a in tw.after] == [rounds[0], sum(rounds)] and last.stats.rounds == sum(rounds)
    assert n["acc"] == last.swaps == int(last.stats.accepts.sum()) and n["att"] == int(last.stats.attempts.sum())
    if G >= 2:
        assert n["acc"] >= 1
    if G >= 5:
        assert n["att"] - n["acc"] >= 1
    assert sorted(last.perm) == list(range(G))
    # K1 with the oracle alone: the energy of the returned spins over the edge list (every |J| is dyadic: equality)
    ea, eb, ej = R.edges(case)
    for r in {0, G - 1}:
        assert last.energies[r] == oracle.energy(ea, eb, ej, case.W * case.H, last.states[r].astype(np.uint8))


@pytest.mark.parametrize("pmj,nw", R.INSTANTIATIONS)
def test_every_instantiation_meets_every_branch_of_the_decision(pmj, nw):
    mine = [c for c in R.CASES if R.instantiation(c) == (pmj, nw)]
    pairs = [p for c in mine for p in R.twin(c).pairs]
    assert any(p.accepted and p.d >= 0 for p in pairs)
    assert any(p.accepted and -40 <= p.d < 0 for p in pairs)
    assert any(not p.accepted and -40 <= p.d < 0 for p in pairs)
    assert not any(not p.accepted and p.d >= 0 for p in pairs)
    # one ladder with a rung gap made large: strip_det_exp returns 0 there, and the ladder still exchanges elsewhere
    gapped = [c for c in mine if any(not p.accepted and p.d < -40 for p in R.twin(c).pairs)]
    assert gapped and all(R.counts(R.twin(c).pairs)["acc"] >= 1 for c in gapped)
    assert not any(p.accepted and p.d < -40 for p in pairs)


def test_a_five_rung_ladder_completes_a_round_trip():
    trips = {c.name: int(R.twin(c).after[-1].stats.round_trips.sum()) for c in R.CASES if len(c.betas) == 5}
    assert max(trips.values()) >= 1, trips


def test_one_rung_is_a_plain_run(oracle):
    """a ladder of one rung: no pair in any round, and the configuration of a plain oracle run at that beta"""
    singles = [c for c in R.CASES if len(c.betas) == 1]
    assert {R.instantiation(c) for c in singles} == set(R.INSTANTIATIONS)
    for case in singles:
        tw = R.twin(case)
        assert not tw.pairs and tw.after[-1].swaps == 0
        lat, seed = R.oracle_engine(case).lat, tw.slot_seeds[0]
        st, t = lat.init(seed), 0
        for k, (T, _) in enumerate(R.calls(case)):
            for _ in range(T + (R.warm_up(case) if k == 0 else 0)):
                lat.sweep(st, seed, t, case.betas[0])
                t += 1
            assert np.array_equal(tw.after[k].states[0], lat.unpack(st).astype(np.bool_))
            assert tw.after[k].energies[0] == lat.energy_mag(st)[0]

"""All four instantiations of lat_strip_kernel<PMJ, NW, LAD = true> (csrc/strip_kernels.hpp: the exchange rounds of a tempering
ladder inside the persistent strip launch -- rung-indexed mailboxes in a ring of four, an arrival counter per replica and round
parity, a release / acquire pair, strip_det_exp, relabelling of my_rung and of the thresholds) bit for bit against the host twin:
ClassicalTempering on the host swap step over the CPU oracle engine, one round at a time, its rounds recorded through the numpy rule
of tests/ladder_statistics_reference.py.  After the warm-up and each of the two pt_run calls: permutation, round number, total
swaps, spins, energies as bit patterns, all ten outputs of the ladder statistics -- and in_kernel_rounds, the proof that the
LAD = true launch ran and not one launch per round.  K1 on two rungs: the energy recomputed from the returned spins over the edge
list (`oracle.energy`; every |J| here is dyadic: equality).  No number in this module is a tolerance.
tests/strip_ladder_reference.py holds the shapes, the couplings, the ladders with their searched betas and the selection rules
restated; tests/test_strip_ladder_host.py proves without a GPU that each case selects the instantiation named below and that the
twin's rounds hold accepted and refused pairs on both sides of d = 0 and beyond d = -40.

Census.  "before": what reached the instantiation before this module -- strip = test_gpu_strip.py (test_on_stream_tempering_on_the_
strip_path, test_in_kernel_exchange_against_the_oracle_engine, test_in_kernel_exchange_at_c3_shape), stat = test_gpu_ladder_
statistics.py::test_inside_the_persistent_launch, mom = test_gpu_ladder_moments.py, icm = test_gpu_ladder_icm.py: ferromagnets of
J = -1 at width 1024 (qpr = 4), 8, 12 or 64 rungs, a round after every 3rd, 4th or 10th timestep, betas within 3e-4 of each other,
NW = 4 (no ladder test set strip_nw); "-" = never.  "now": test_ladder_inside_the_launch[case], the cases by shape, coupling
(fm: J = -1, half: J = -0.5, afm: J = +1, glass: seeded +-1) and rungs; every case runs a round after every timestep in one call
and after every 3rd in the other, starts its second call on an odd round, holds 6 or more rounds inside one launch and ends a call
on a tail; "*": also test_one_launch_per_round_gives_the_same_bits (ISINGMC_PT_IN_KERNEL=0 on the same calls).

 lat_strip_kernel<PMJ, NW, LAD>   before               now
  false 1 true                    -                    256x128 fm 1, 1024x48 half 2, 256x128 afm 5 (28 rounds: round trips),
                                                       8192x4 fm 5 (a beta gap: d < -40) *, 1024x48 afm 8
  true  1 true                    -                    8192x4 glass 1, 256x128 glass 2, 1024x48 glass 5 (gap) *, 8192x4 glass 8
  false 4 true                    strip stat mom icm   1024x192 half 1, 8192x16 fm 2, 1024x192 afm 5 (gap) *, 256x512 fm 8
  true  4 true                    -                    256x512 glass 1, 1024x192 glass 2, 8192x16 glass 5 (gap) *, 256x512 glass 8

 inside them, met for the first time: an odd ladder (5: the top or the bottom rung has no partner in a round), two rungs (every
 second round has no pair), one rung, a round after EVERY timestep (the random words of the next sweep are always drawn behind the
 post), strip_det_exp(d < -40) = 0, blocks -> strips without the XCD remap (1, 2, 5 rungs) with NW = 1 and NW = 4, |J| = 0.5 in
 lad.jabs and lad.ladder_thr, J > 0, and the strip geometries qpr = 1 (S = 64 / 256: both neighbours of a strip are the same
 strip; NW = 4: the wave-pair row mapping), qpr = 32 (S = 2: every row is a boundary row; S = 8) and three strips (qpr = 4)."""
import numpy as np
import pytest

import ladder_statistics_reference as SR
import strip_ladder_reference as R

pytestmark = pytest.mark.gpu

CASES = pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
FALLBACK = [c for c in R.CASES if c.fallback]


def _ladder(capi, monkeypatch, case, in_kernel):
    """the case's ladder attached to a container of its own, statistics on, on the strip kernel of the case's NW"""
    monkeypatch.setenv("ISINGMC_STRIP", "1")
    monkeypatch.setenv("ISINGMC_PT_IN_KERNEL", "1" if in_kernel else "0")
    monkeypatch.setenv("ISINGMC_STRIP_NW", str(case.nw))   # (the switches are read when a container is created)
    g = capi.Graph(*R.edges(case))
    assert g.kind == capi.KIND_LATTICE2D and bool(g.info.uniform_sign) == (not R.COUPLINGS[case.coupling][1])
    assert g.info.jabs == abs(R.COUPLINGS[case.coupling][0])
    st = capi.States(g, np.array(R.twin(case).slot_seeds, dtype=np.uint64))
    st.pt_attach(np.array(case.betas), 0, len(case.betas), 1, case.seed)
    st.pt_set_statistics(True)
    return st


def _run_against_the_twin(capi, oracle, monkeypatch, case, in_kernel):
    tw, G = R.twin(case), len(case.betas)
    ea, eb, ej = R.edges(case)
    st = _ladder(capi, monkeypatch, case, in_kernel)
    assert st.family == "checkerboard" and st.count == G
    st.pt_time_steps(R.warm_up(case))
    inside, t = 0, R.warm_up(case)
    for (T, f), want in zip(R.calls(case), tw.after):
        st.pt_run(T, f)
        t += T
        inside += R.rounds_inside_the_launch(G, G, T, f) if in_kernel else 0
        perm, rnd, swaps = st.pt_state()
        assert np.array_equal(perm, want.perm) and rnd == want.round and swaps == want.swaps and st.timestep == t
        states, energies = st.states(), st.energies()
        assert np.array_equal(states, want.states)
        assert np.array_equal(SR.bits(energies), SR.bits(want.energies))
        SR.assert_equal(st.pt_statistics(), want.stats, in_kernel_rounds=inside)
        for r in {int(perm[0]), int(perm[-1])}:   # K1 on the lowest and the highest rung
            assert energies[r] == oracle.energy(ea, eb, ej, case.W * case.H, states[r].astype(np.uint8))
    return st


@CASES
def test_ladder_inside_the_launch(capi, oracle, monkeypatch, case):
    st = _run_against_the_twin(capi, oracle, monkeypatch, case, in_kernel=True)
    rounds = [T // f for T, f in R.calls(case)]
    assert st.pt_statistics()["in_kernel_rounds"] == sum(rounds) - 2 >= 7   # all but the last round of each call


@pytest.mark.parametrize("case", FALLBACK, ids=[c.name for c in FALLBACK])
def test_one_launch_per_round_gives_the_same_bits(capi, oracle, monkeypatch, case):
    """ISINGMC_PT_IN_KERNEL=0: the same calls, every round at a kernel boundary (pt_swap_kernel), against the same twin -- and the
    raw state words against the ladder that held its rounds inside the launch"""
    per_round = _run_against_the_twin(capi, oracle, monkeypatch, case, in_kernel=False)
    inside = _run_against_the_twin(capi, oracle, monkeypatch, case, in_kernel=True)
    assert per_round.pt_statistics()["in_kernel_rounds"] == 0 < inside.pt_statistics()["in_kernel_rounds"]
    assert np.array_equal(per_round.raw_state(), inside.raw_state())
    assert np.array_equal(per_round.packed(), inside.packed())


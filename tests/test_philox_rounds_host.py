"""The yardstick of the option "philox_rounds" (DESIGN.md S23), pinned without a GPU: tests/philox_rounds_reference.py restates
Philox4x32-R and the checkerboard sweep in numpy; here its generator is tied to Random123's known answers at R = 7 and R = 10, its
sweep to the C oracle's trajectories at R = 10, and the searched seeds of tests/golden/philox7_tie_cases.json are recounted."""
import json
import os

import numpy as np
import pytest

import cluster_reference as CR
import lat_variants_reference as LV
import mc_variants_reference as MV
import philox_rounds_reference as PR

HERE = os.path.dirname(os.path.abspath(__file__))


def _vectors():
    with open(os.path.join(HERE, "golden", "philox_kat.json")) as f:
        kat = json.load(f)
    assert "philox4x32 10" in kat["source"]
    return [([int(x, 16) for x in v["ctr"]], [int(x, 16) for x in v["key"]], [int(x, 16) for x in v["out"]]) for v in kat["vectors"]]


def test_seven_rounds_continue_to_the_known_answers_of_ten():
    """Random123 publishes philox4x32-10 answers; three more rounds on the R = 7 output, with the key bumped 7, 8 and 9 times, must
    arrive there: that pins the seven rounds without vectors of their own."""
    vectors = _vectors()
    assert len(vectors) >= 3
    for ctr, key, out in vectors:
        seven = PR.philox4x32(7, *ctr, *key)
        assert [int(w) for w in PR.philox4x32(10, *seven, *key, first_round=7)] == out
        assert [int(w) for w in PR.philox4x32(10, *ctr, *key)] == out
        assert [int(w) for w in seven] != out


def test_ten_rounds_equal_the_cluster_reference():
    rng = np.random.default_rng(7)
    c = rng.integers(0, 2 ** 32, (4, 64), dtype=np.uint64)
    k0, k1 = 0x89ABCDEF, 0x01234567
    for a, b in zip(PR.philox4x32(10, *c, k0, k1), CR.philox4x32_10(*c, k0, k1)):
        assert np.array_equal(a, b)
    assert not np.array_equal(PR.philox4x32(7, *c, k0, k1)[0], PR.philox4x32(10, *c, k0, k1)[0])


@pytest.mark.parametrize("coupling", LV.COUPLINGS)
@pytest.mark.parametrize("shape", [(256, 8), (64, 16)], ids=["256x8", "64x16"])
def test_reference_sweep_reproduces_the_oracle_at_ten_rounds(oracle, shape, coupling):
    """configurations and energies of every timestep, bit for bit, at the betas of MV.BETAS (0 and a negative beta: both classes
    flip outright; 3.0: all-zero threshold planes) and then under per-replica betas"""
    W, H = shape
    case, seeds = LV.make_case(W, H, coupling), LV.SEEDS
    lat = LV.oracle_lat(oracle, case)
    betas = list(MV.BETAS) + [LV.replica_betas(len(seeds))] * 2
    traj = PR.run(oracle, W, H, coupling, seeds, betas, 10)
    ties = 0
    for r, seed in enumerate(seeds):
        ref = lat.init(seed)
        assert np.array_equal(ref, traj.start[r])
        for t, beta in enumerate(betas):
            lat.sweep(ref, seed, t, float(np.asarray(beta).ravel()[r % np.asarray(beta).size]))
            assert np.array_equal(ref, traj.steps[t].words[r]), (r, t)
            assert lat.energy_mag(ref)[0] == PR.energy(case, traj.steps[t].words[r])
            ties += int(traj.steps[t].ties[r].sum())
    assert ties > 0   # the tie stage was part of what was compared
    seven = PR.run(oracle, W, H, coupling, seeds, betas[2:3], 7, t0=2, start=traj.steps[1].words)
    assert not np.array_equal(seven.steps[0].words, traj.steps[2].words)   # another generator: another trajectory


@pytest.mark.parametrize("coupling", LV.COUPLINGS)
@pytest.mark.parametrize("group", list(PR.GROUPS))
def test_the_fixed_gpu_cases_reach_both_tie_calls_at_seven_rounds(oracle, group, coupling):
    """the coverage condition of the searched seeds, from the reference's own counts: a tie in each costly class, and a quad with
    five or more ties (the second tie call) -- in the seven-round trajectory the GPU tests compare against"""
    n3, n4, most = PR.coverage(oracle, group, coupling, 7)
    assert n3 >= 1 and n4 >= 1 and most >= 5, (n3, n4, most)
    want = PR.fixture()["found"][group][coupling]
    assert (n3, n4, most) == (want["class3_ties"], want["class4_ties"], want["most_ties_in_a_quad"])

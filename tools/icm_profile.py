"""Measurements for profiles/icm_update.txt: device time per isoenergetic cluster move next to a Swendsen-Wang
cluster step (S8) on HALF as many replicas of the same size -- the same number of labelling problems -- in one session (HIP events
of isingmc_do_time_steps_timed).

  python tools/icm_profile.py > profiles/icm_update.txt
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import exact  # noqa: E402
from pyisingmontecarlo_amd import _capi  # noqa: E402

BETA = 0.8      # the glass: Metropolis sweeps between the moves keep the two replicas of a pair apart (q = -1 on about half the sites)
BETA_C = 0.4407  # the ferromagnet of the Swendsen-Wang step


def timed(st, steps, beta, repeats=3):
    """Median device time per timestep in ms."""
    return float(np.median([st.do_time_steps_timed(steps, beta) / steps for _ in range(repeats)]))


def main():
    print("library sha256", hashlib.sha256(open(_capi.LIB_PATH, "rb").read()).hexdigest())
    print("\n# device time per timestep (HIP events, median of 3 runs of `steps` timesteps), random start + 20 warm-up timesteps")
    print("# ICM: +-J sample, R replicas = R / 2 pairs at beta 0.8, icm_every = 1 after 20 Metropolis sweeps (the pairs keep their overlap:")
    print("#      the move conserves q); SW: ferromagnet at beta_c, R / 2 replicas, cluster_every = 1: the same number of labelling problems")
    for L, R, steps in ((256, 64, 200), (2048, 128, 20)):
        N = L * L
        glass = _capi.Graph(*exact.square_lattice_edges(L, L, -1.0, np.random.default_rng(1)), N)
        st = _capi.States(glass, _capi.make_seeds(1, R))
        st.do_time_steps(20, BETA)
        st.set_icm_every(1)
        st.do_time_steps(20, BETA)
        icm_ms = timed(st, steps, BETA)
        n, largest, minus = st.icm_stats()
        st.close()
        glass.close()
        ferro = _capi.Graph(*exact.square_lattice_edges(L, L, -1.0), N)
        sw = _capi.States(ferro, _capi.make_seeds(1, R // 2))
        sw.set_cluster_every(1)
        sw.do_time_steps(20, BETA_C)
        sw_ms = timed(sw, steps, BETA_C)
        sw_n, sw_largest = sw.cluster_stats()
        sw.close()
        ferro.close()
        print(f"{L}^2 x {R}: ICM step {icm_ms * 1e3:10.1f} us   SW step on {R // 2} replicas {sw_ms * 1e3:10.1f} us   ICM / SW {icm_ms / sw_ms:5.2f}")
        print(f"    ICM per pair: q = -1 sites {minus.mean() / N:.3f} N, clusters {n.mean():.0f}, largest {largest.mean():.0f};   "
              f"SW per replica: clusters {sw_n.mean():.0f}, largest {sw_largest.mean():.0f}")


if __name__ == "__main__":
    main()

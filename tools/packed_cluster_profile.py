"""Measurements for profiles/packed_cluster.txt: device time of a Swendsen-Wang cluster step on the replica-packed bit-sliced
path next to a Metropolis timestep of the same container type, on the cubic lattice at its critical coupling,
and next to the checkerboard cluster step (S8) at the same number of site-replicas -- one session, one binary, HIP events of
isingmc_do_time_steps_timed, medians of five interleaved runs.

  python tools/packed_cluster_profile.py > profiles/packed_cluster.txt
  python tools/packed_cluster_profile.py --trace 64     # a short run of 64^3 x 64 alone, for rocprofv3 --kernel-trace --stats
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import exact  # noqa: E402
from pyisingmontecarlo_amd import _capi  # noqa: E402

BETA_3D = 0.2216  # cubic ferromagnet, bulk critical coupling
BETA_2D = 0.4407  # square ferromagnet
R = 64
WARMUP = 20
REPEATS = 5


def cubic_states(L, k):
    g = _capi.Graph(*exact.cubic_lattice_edges(L, -1.0), L ** 3)
    st = _capi.States(g, _capi.make_seeds(1, R))
    assert st.family == "packed_bitsliced"  # (by size: no switch is set in this process)
    st.set_cluster_every(k)
    return g, st


def interleaved(cases, steps):
    """cases: [(states, beta)]; median over REPEATS rounds of the device time per timestep in ms, the cases taking turns."""
    ms = [[] for _ in cases]
    for _ in range(REPEATS):
        for i, (st, beta) in enumerate(cases):
            ms[i].append(st.do_time_steps_timed(steps, beta) / steps)
    return [float(np.median(m)) for m in ms]


def trace(L):
    g, st = cubic_states(L, 1)
    st.do_time_steps(WARMUP, BETA_3D)
    st.do_time_steps(10, BETA_3D)
    st.synchronize()


def main():
    if "--trace" in sys.argv:
        return trace(int(sys.argv[sys.argv.index("--trace") + 1]))
    print("library sha256", hashlib.sha256(open(_capi.LIB_PATH, "rb").read()).hexdigest())
    print(f"\n# device time per timestep (HIP events, median of {REPEATS} interleaved runs of `steps` timesteps), {R} replicas, random start +")
    print(f"# {WARMUP} warm-up timesteps of the container's own kind.  Cubic ferromagnet at beta = {BETA_3D}: `cluster` = cluster_every = 1")
    print(f"# (every timestep a cluster step), `sweep` = Metropolis only; S8: square ferromagnet at beta = {BETA_2D}, cluster_every = 1")
    for L, steps, L2 in ((64, 50, 512), (256, 5, None)):
        N = L ** 3
        g, cl = cubic_states(L, 1)
        mc = _capi.States(g, _capi.make_seeds(2, R))
        cases = [(cl, BETA_3D), (mc, BETA_3D)]
        if L2:  # the same number of site-replicas on the checkerboard path
            g2 = _capi.Graph(*exact.square_lattice_edges(L2, L2, -1.0), L2 * L2)
            sw = _capi.States(g2, _capi.make_seeds(3, R))
            assert sw.family == "checkerboard"
            sw.set_cluster_every(1)
            cases.append((sw, BETA_2D))
        for st, beta in cases:
            st.do_time_steps(WARMUP if L < 256 else 5, beta)
        t = interleaved(cases, steps)
        n, largest = cl.cluster_stats()
        print(f"{L}^3 x {R} (steps = {steps}): cluster {t[0] * 1e3:10.1f} us   sweep {t[1] * 1e3:10.1f} us   cluster / sweep {t[0] / t[1]:6.2f}   "
              f"cluster step {t[0] * 1e6 / (N * R):.4f} ns per site-replica")
        print(f"    per replica: clusters {n.mean():.0f}, largest {largest.mean():.0f} of {N} sites")
        if L2:
            print(f"    S8 step on {L2}^2 x {R}: {t[2] * 1e3:10.1f} us   S11 / S8 at {N * R} site-replicas {t[0] / t[2]:6.2f}")
            cases[2][0].close()
            g2.close()
        cl.close()
        mc.close()
        g.close()


if __name__ == "__main__":
    main()

"""Measurements for profiles/packed_icm.txt: device time of an isoenergetic cluster move on the replica-packed paths (DESIGN.md
S12) next to a Swendsen-Wang cluster step (S11) and a Metropolis timestep on the same container shape -- the cubic +-J glass,
64^3 x 64 replicas -- and of the move next to a Metropolis timestep on one real-coupling shape (Gaussian couplings on the same
lattice).  One session, one binary, HIP events of isingmc_do_time_steps_timed, medians of five interleaved runs.

  python tools/packed_icm_profile.py > profiles/packed_icm.txt
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import exact  # noqa: E402
from pyisingmontecarlo_amd import _capi  # noqa: E402

BETA = 0.5  # paramagnetic side of the 3-d +-J glass (T_c near beta = 0.9): the d = 1 sites percolate, one large cluster per pair
R = 64
L = 64
WARMUP = 20
REPEATS = 5
STEPS = 50


def interleaved(cases, steps):
    """cases: [(states, beta)]; median over REPEATS rounds of the device time per timestep in ms, the cases taking turns."""
    ms = [[] for _ in cases]
    for _ in range(REPEATS):
        for i, (st, beta) in enumerate(cases):
            ms[i].append(st.do_time_steps_timed(steps, beta) / steps)
    return [float(np.median(m)) for m in ms]


def main():
    print("library sha256", hashlib.sha256(open(_capi.LIB_PATH, "rb").read()).hexdigest())
    print(f"\n# device time per timestep (HIP events, median of {REPEATS} interleaved runs of {STEPS} timesteps), {L}^3 x {R} replicas, random")
    print(f"# start + {WARMUP} warm-up timesteps of the container's own kind, beta = {BETA}.  `icm` = icm_every = 1 (every timestep a move),")
    print("# `sw` = cluster_every = 1 (every timestep an S11 step), `sweep` = Metropolis only")
    N = L ** 3
    ea, eb, _ = exact.cubic_lattice_edges(L, -1.0)
    rng = np.random.default_rng(1)
    for name, ej, family in (("+-J", rng.choice([-1.0, 1.0], len(ea)), "packed_bitsliced"), ("Gaussian J", rng.normal(size=len(ea)), "packed_real")):
        g = _capi.Graph(ea, eb, ej, N)
        cases = []
        for i, kind in enumerate(("icm", "sw", "sweep")):
            if kind == "sw" and family == "packed_real":
                continue  # (S11 does not serve the real-coupling family)
            st = _capi.States(g, _capi.make_seeds(1 + i, R))
            assert st.family == family  # (by size: no switch is set in this process)
            if kind == "icm":
                # a few sweeps first: from the random start every second site has d = 1
                st.do_time_steps(WARMUP, BETA)
                st.set_icm_every(1)
            elif kind == "sw":
                st.set_cluster_every(1)
            cases.append((kind, st))
        for _, st in cases:
            st.do_time_steps(WARMUP, BETA)
        t = dict(zip((k for k, _ in cases), interleaved([(st, BETA) for _, st in cases], STEPS)))
        clusters, largest, minus = cases[0][1].icm_stats()
        line = f"{name} {L}^3 x {R} ({family}): icm {t['icm'] * 1e3:10.1f} us   sweep {t['sweep'] * 1e3:10.1f} us   icm / sweep {t['icm'] / t['sweep']:6.2f}"
        if "sw" in t:
            line += f"   sw {t['sw'] * 1e3:10.1f} us   icm / sw {t['icm'] / t['sw']:6.2f}"
        print(line)
        print(f"    icm step {t['icm'] * 1e6 / (N * R):.4f} ns per site-replica; per pair: d = 1 sites {minus.mean():.0f} of {N}, clusters {clusters.mean():.0f}, "
              f"largest {largest.mean():.0f}")
        for _, st in cases:
            st.close()
        g.close()


if __name__ == "__main__":
    main()

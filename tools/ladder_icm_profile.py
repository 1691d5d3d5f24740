"""Measurements for profiles/ladder_icm.txt: the isoenergetic cluster move between two containers next to the move
between adjacent replicas of one container (S9) on the same number of pairs, and a tempering block with moves next to the same
ladder without, in one session on one binary.  Wall clock around enqueue + synchronise (the new call has no HIP-event variant),
runs of the variants interleaved, medians.

  python tools/ladder_icm_profile.py > profiles/ladder_icm.txt
"""
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import exact  # noqa: E402
from pyisingmontecarlo_amd import _capi  # noqa: E402
from pyisingmontecarlo_amd.tempering import ClassicalTempering  # noqa: E402

BETA = 0.8
REPEATS = 5


def wall(fn, sync):
    t0 = time.perf_counter()
    fn()
    sync()
    return time.perf_counter() - t0


def moves(L, pairs, steps):
    N = L * L
    g = _capi.Graph(*exact.square_lattice_edges(L, L, -1.0, np.random.default_rng(1)), N)
    a, b = _capi.States(g, _capi.make_seeds(1, pairs)), _capi.States(g, _capi.make_seeds(2, pairs))
    la, lb = _capi.States(g, _capi.make_seeds(1, pairs)), _capi.States(g, _capi.make_seeds(2, pairs))
    one = _capi.States(g, _capi.make_seeds(1, 2 * pairs))
    for st in (a, b, la, lb, one):
        st.do_time_steps(20, BETA)
    for st, seed in ((la, 5), (lb, 6)):
        st.pt_attach([BETA] * pairs, 0, pairs, 1, seed)   # one beta on every rung: the permutation stays a table like any other
    one.set_icm_every(1)
    ident = np.arange(pairs, dtype=np.uint32)
    variants = {
        "between, host tables": lambda: wall(lambda: [a.icm_between(b, ident, ident) for _ in range(steps)], lambda: (a.synchronize(), b.synchronize())),
        "between, ladder form": lambda: wall(lambda: [la.icm_between(lb) for _ in range(steps)], lambda: (la.synchronize(), lb.synchronize())),
        "adjacent pairs (S9)": lambda: wall(lambda: one.do_time_steps(steps, BETA), one.synchronize),
    }
    for fn in variants.values():   # warm-up: workspaces, code objects
        fn()
    times = {name: [] for name in variants}
    for _ in range(REPEATS):
        for name, fn in variants.items():
            times[name].append(fn() / steps)
    events = float(np.median([one.do_time_steps_timed(steps, BETA) / steps for _ in range(3)]))
    print(f"{L}^2 x {pairs} pairs, {steps} moves per run, {REPEATS} interleaved runs: us per move, median (min .. max)")
    for name, ts in times.items():
        print(f"    {name:22s} {np.median(ts) * 1e6:10.1f}  ({min(ts) * 1e6:.1f} .. {max(ts) * 1e6:.1f})")
    print(f"    adjacent pairs, HIP events {events * 1e3:8.1f}")
    n, largest, minus = a.icm_between_stats()
    print(f"    per pair: q = -1 sites {minus.mean() / N:.3f} N, clusters {n.mean():.0f}, largest {largest.mean():.0f}")
    for st in (a, b, la, lb, one):
        st.close()
    g.close()


def blocks(L, G, T, f, k):
    edges = exact.square_lattice_edges(L, L, -1.0, np.random.default_rng(1))
    ladders = {}
    for name, kk in (("with moves", k), ("without", 0)):
        pt = ClassicalTempering(edges, seed=1, copies=2)
        for beta in np.linspace(0.5, 1.0, G):
            pt.add_graph(float(beta))
        pt.set_replica_cluster_update_every(kk)
        pt.timesteps(T, f)   # warm-up
        ladders[name] = pt
    times = {name: [] for name in ladders}
    for _ in range(REPEATS):
        for name, pt in ladders.items():
            times[name].append(wall(lambda: pt.timesteps(T, f), lambda: None) / T)
    print(f"{L}^2 x 2 copies x {G} rungs, blocks of {T} timesteps, a round every {f}, a move every {k}: us per timestep, median (min .. max)")
    for name, ts in times.items():
        print(f"    {name:12s} {np.median(ts) * 1e6:10.1f}  ({min(ts) * 1e6:.1f} .. {max(ts) * 1e6:.1f})")


def main():
    print("library sha256", hashlib.sha256(open(_capi.LIB_PATH, "rb").read()).hexdigest())
    print()
    moves(256, 32, 200)
    moves(2048, 64, 20)
    print()
    blocks(256, 32, 120, 4, 4)
    blocks(1024, 16, 120, 4, 4)


if __name__ == "__main__":
    main()

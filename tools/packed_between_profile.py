"""Measurements for profiles/packed_between.txt: device time of an isoenergetic cluster move between two replica-packed
containers (32 slots each, 32 pairs = one pair block) next to the S12 step on one container of 64 experiments (32
pairs: the yardstick) and a Metropolis timestep of that container, on the cubic +-J glass 64^3 and on the Gaussian glass of the
same shape; and a copies=2 tempering block with and without moves.  One session, one binary, HIP events, medians of five
interleaved runs.

  python tools/packed_between_profile.py > profiles/packed_between.txt
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

BETA = 0.5  # paramagnetic side of the 3-d +-J glass (T_c near beta = 0.9): the d = 1 sites percolate, one large cluster per pair
L = 64
PAIRS = 32
WARMUP = 20
REPEATS = 5
STEPS = 30
RUNGS, ROUND_EVERY, MOVE_EVERY, BLOCK = 16, 4, 4, 120


def between_ms(a, b, steps):
    """HIP-event time per move of `steps` moves in the ladder-free table form, on a's stream (b's stream only waits)."""
    import torch

    stream = a.pt_stream()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ident = np.arange(PAIRS, dtype=np.uint32)
    a.synchronize()
    b.synchronize()
    start.record(stream)
    for _ in range(steps):
        a.icm_between(b, ident, ident)
    end.record(stream)
    a.synchronize()
    b.synchronize()
    return start.elapsed_time(end) / steps


def ladder_us_per_timestep(edges, k):
    pt = ClassicalTempering(edges, seed=9, copies=2)
    for beta in np.linspace(0.3, 1.0, RUNGS):
        pt.add_graph(float(beta))
    pt.set_replica_cluster_update_every(k)
    pt.timesteps(BLOCK, ROUND_EVERY)   # warm-up: workspace, tables
    out = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        pt.timesteps(BLOCK, ROUND_EVERY)
        out.append((time.perf_counter() - t0) / BLOCK * 1e6)
    assert pt._on_stream and pt._pair[0]._states.family.startswith("packed")
    return float(np.median(out))


def main():
    print("library sha256", hashlib.sha256(open(_capi.LIB_PATH, "rb").read()).hexdigest())
    print(f"\n# device time (HIP events, median of {REPEATS} interleaved runs of {STEPS}), {L}^3, beta = {BETA}, random start + {WARMUP} sweeps.")
    print(f"# `between` = isingmc_icm_between of two containers of {PAIRS} slots ({PAIRS} pairs, host tables); `icm` = the S12 step of one")
    print(f"# container of {2 * PAIRS} experiments ({PAIRS} pairs, icm_every = 1); `sweep` = a Metropolis timestep of that container")
    N = L ** 3
    ea, eb, _ = exact.cubic_lattice_edges(L, -1.0)
    rng = np.random.default_rng(1)
    for name, ej, family in (("+-J", rng.choice([-1.0, 1.0], len(ea)), "packed_bitsliced"), ("Gaussian J", rng.normal(size=len(ea)), "packed_real")):
        g = _capi.Graph(ea, eb, ej, N)
        a, b = _capi.States(g, _capi.make_seeds(1, PAIRS)), _capi.States(g, _capi.make_seeds(2, PAIRS))
        icm, sweep = _capi.States(g, _capi.make_seeds(3, 2 * PAIRS)), _capi.States(g, _capi.make_seeds(4, 2 * PAIRS))
        for st in (a, b, icm, sweep):
            assert st.family == family  # (by size: no switch is set in this process)
            st.do_time_steps(WARMUP, BETA)
        icm.set_icm_every(1)
        between_ms(a, b, 3)
        icm.do_time_steps(3, BETA)
        ms = {"between": [], "icm": [], "sweep": []}
        for _ in range(REPEATS):
            ms["between"].append(between_ms(a, b, STEPS))
            ms["icm"].append(icm.do_time_steps_timed(STEPS, BETA) / STEPS)
            ms["sweep"].append(sweep.do_time_steps_timed(STEPS, BETA) / STEPS)
        t = {k: float(np.median(v)) for k, v in ms.items()}
        clusters, largest, minus = a.icm_between_stats()
        print(f"{name} {L}^3 ({family}): between {t['between'] * 1e3:10.1f} us   icm {t['icm'] * 1e3:10.1f} us   sweep {t['sweep'] * 1e3:10.1f} us   "
              f"between / icm {t['between'] / t['icm']:6.2f}   between / sweep {t['between'] / t['sweep']:6.2f}")
        print(f"    per pair: d = 1 sites {minus.mean():.0f} of {N}, clusters {clusters.mean():.0f}, largest {largest.mean():.0f}")
        for st in (a, b, icm, sweep):
            st.close()
        g.close()
        with_moves, without = ladder_us_per_timestep((ea, eb, ej), MOVE_EVERY), ladder_us_per_timestep((ea, eb, ej), 0)
        print(f"    copies=2 ladder, {RUNGS} rungs, a round every {ROUND_EVERY} timesteps, {BLOCK} timesteps per call (wall clock, median of {REPEATS}): "
              f"{with_moves:.1f} us per timestep with a move every {MOVE_EVERY}, {without:.1f} us without")


if __name__ == "__main__":
    main()

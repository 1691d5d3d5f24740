"""The copies=2 ladder scenarios of tests/test_gpu_packed_between.py, shared between the test process and a child
process that runs them under another environment (ISINGMC_PT_HOST=1): run as a script it prints one JSON line of digests."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

G_RUNGS, K, ROUND_EVERY, SEED = 8, 3, 2, 4711
BETAS = {"pm": np.linspace(0.5, 0.64, G_RUNGS), "gauss": np.linspace(0.4, 0.61, G_RUNGS)}


def edges(family):
    from oracle import exact

    ea, eb, _ = exact.cubic_lattice_edges(6, 1.0)
    rng = np.random.default_rng(77)
    ej = rng.choice([-1.0, 1.0], len(ea)) if family == "pm" else rng.normal(size=len(ea))
    return ea, eb, ej


def ladder(family, factory=None):
    from pyisingmontecarlo_amd.tempering import ClassicalTempering

    pt = ClassicalTempering(edges(family), seed=SEED, engine_factory=factory, copies=2)
    for b in BETAS[family]:
        pt.add_graph(float(b))
    pt.set_replica_cluster_update_every(K)
    return pt


# the switches that put the family's graph on its replica-packed family at 8 experiments (FORCE_REAL would take the +-J glass too)
ENV = {"pm": {"ISINGMC_FORCE_PACKED": "1", "ISINGMC_FORCE_REAL": "0"}, "gauss": {"ISINGMC_FORCE_PACKED": "1", "ISINGMC_FORCE_REAL": "1"}}
FAMILY = {"pm": "packed_bitsliced", "gauss": "packed_real"}


def snapshot(pt):
    return [np.asarray(pt.get_permutation(), dtype=np.int64), np.array([pt.get_total_swaps()], dtype=np.int64),
            *[np.asarray(c._states.states(), dtype=np.uint8) for c in pt._pair],
            *[np.asarray(c._states.energies(), dtype=np.float64) for c in pt._pair],
            *[np.asarray(x, dtype=np.uint64) for x in pt.get_replica_cluster_stats()]]


def run(pt):
    """timesteps in two calls, then timesteps_sample: a list of arrays after every call."""
    out = []
    for T in (6, 4):
        pt.timesteps(T, ROUND_EVERY)
        out += snapshot(pt)
    states, energies = pt.timesteps_sample(12, 4, 3)
    return out + [np.asarray(states, dtype=np.uint8), np.asarray(energies, dtype=np.float64)] + snapshot(pt)


def digests(arrays):
    return [hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() for a in arrays]


if __name__ == "__main__":
    res = {}
    for family in ("pm", "gauss"):
        os.environ.update(ENV[family])
        pt = ladder(family)
        res[family] = {"digests": digests(run(pt)), "on_stream": bool(pt._on_stream), "family": pt._pair[0]._states.family}
    print(json.dumps(res))

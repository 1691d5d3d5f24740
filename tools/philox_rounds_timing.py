"""Device time of the sweeps at 7 against 10 Philox rounds, same binary, the two round counts alternated.

    python tools/philox_rounds_timing.py [--reps 5]

Three workloads: do_time_steps at the bench.py shape (4096^2 x 256, beta 0.4407), pt_run(200, 10) at 1024^2 x 64 rungs (host wall
clock around the synchronised call: one persistent launch per call), and the LDS-resident path at 512^2 x 256.  Prints one JSON
line per workload with the medians of both round counts, their spreads and the binary's sha256."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import exact as X  # noqa: E402
from pyisingmontecarlo_amd import _capi  # noqa: E402


def sha256_of_library():
    here = os.path.dirname(os.path.abspath(_capi.__file__))
    with open(os.path.join(here, "lib", "libisingmc.so"), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def sweeps(L, R, steps, warmup, reps):
    g = _capi.Graph(*X.square_lattice_edges(L, L, -1.0))
    st = {r: _capi.States(g, _capi.make_seeds(7, R)) for r in (10, 7)}
    out = {10: [], 7: []}
    for r, s in st.items():
        s.set_option("philox_rounds", r)
        s.do_time_steps(warmup, 0.4407)
    for _ in range(reps):
        for r in (10, 7):
            out[r].append(st[r].do_time_steps_timed(steps, 0.4407) * 1e3 / steps)   # us per timestep, device events
    return out


def ladder(L, G, reps):
    g = _capi.Graph(*X.square_lattice_edges(L, L, -1.0))
    out = {10: [], 7: []}
    st = {}
    for r in (10, 7):
        st[r] = _capi.States(g, _capi.make_seeds(11, G))
        st[r].set_option("philox_rounds", r)
        st[r].pt_attach(np.linspace(0.42, 0.46, G), 0, G, 1, 5)
        st[r].pt_run(200, 10)
        st[r].synchronize()
    for _ in range(reps):
        for r in (10, 7):
            t0 = time.perf_counter()
            st[r].pt_run(200, 10)
            st[r].synchronize()
            out[r].append((time.perf_counter() - t0) * 1e6 / 200)   # us per timestep, host wall clock
    return out


def report(name, out, sha):
    med = {r: statistics.median(v) for r, v in out.items()}
    print(json.dumps({"workload": name, "us_per_timestep_median": med, "min": {r: min(v) for r, v in out.items()},
                      "max": {r: max(v) for r, v in out.items()}, "gain_7_over_10": med[10] / med[7] - 1.0, "sha256": sha}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    sha = sha256_of_library()
    report("do_time_steps 4096^2 x 256", sweeps(4096, 256, 20, 5, a.reps), sha)
    report("pt_run(200, 10) 1024^2 x 64 rungs", ladder(1024, 64, a.reps), sha)
    report("resident 512^2 x 256", sweeps(512, 256, 200, 20, a.reps), sha)


if __name__ == "__main__":
    main()

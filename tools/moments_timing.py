"""Time of one moment-sum sample in units of one sweep of the same container, in every mode and for K = 4, 5, 6, 8
time planes, beside get_states() + numpy: 1024^2 +-J x 256 (checkerboard) and 64^3 +-J x 1024 (bit-sliced).  Wall clock of enqueued
samples and one wait, best of three.  Output kept in profiles/2026-10-19_moments.txt."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import exact as X  # noqa: E402
from pyisingmontecarlo_amd import _capi as capi  # noqa: E402


def say(*a):
    print(" ".join(str(x) for x in a), flush=True)


def sync(st):
    capi._check(capi.lib().isingmc_synchronize(st._h))


def timed_samples(st, n, reps=3):
    """best-of-reps wall time per sample of n enqueued samples (enqueue-only calls, one wait)"""
    best = 1e9
    for _ in range(reps):
        sync(st)
        t0 = time.perf_counter()
        for _ in range(n):
            st.accumulate_moments()
        sync(st)
        best = min(best, (time.perf_counter() - t0) / n)
    return best


def shape(name, make_graph, R, beta):
    g = make_graph()
    st = capi.States(g, capi.make_seeds(1, R))
    say(f"== {name} x {R}: family {st.family}")
    st.do_time_steps(20, beta)
    sweep = min(st.do_time_steps_timed(50, beta) for _ in range(3)) / 50 * 1e-3
    say(f"sweep {sweep * 1e6:.1f} us")
    for bonds in (False, True):
        st.set_moments_every(1 << 40, bonds=bonds)
        timed_samples(st, 5, 1)
        t = timed_samples(st, 40)
        say(f"summed{' + bonds' if bonds else ''}: {t * 1e6:.1f} us per sample = {t / sweep:.2f} sweeps")
        st.set_moments_every(0)
    for K in (4, 5, 6, 8):
        st.set_option("moments_planes", K)
        st.set_moments_every(1 << 40, per_replica=True)
        n = 2 * ((1 << K) - 1)
        timed_samples(st, (1 << K) - 1, 1)
        t = timed_samples(st, n)
        say(f"per replica K={K}: {t * 1e6:.1f} us per sample (flushes included, {n} samples) = {t / sweep:.2f} sweeps")
        st.set_moments_every(0)
    t0 = time.perf_counter()
    s = st.states()
    t1 = time.perf_counter()
    m = (2 * s.astype(np.int8) - 1).sum(axis=0, dtype=np.int64)
    t2 = time.perf_counter()
    say(f"get_states() {t1 - t0:.3f} s + numpy site sum {t2 - t1:.3f} s per sample = {(t2 - t0) / sweep:.0f} sweeps  (checksum {int(m.sum())})")
    t0 = time.perf_counter()
    n, site, _ = st.moments()
    say(f"moments() read-out of the per-replica totals: {time.perf_counter() - t0:.3f} s")


beta = 0.4407
shape("1024^2 +-J lattice", lambda: capi.Graph(*X.square_lattice_edges(1024, 1024, -1.0, np.random.default_rng(3))), 256, beta)
os.environ["ISINGMC_FORCE_PACKED"] = "1"
ea, eb, _ = X.cubic_lattice_edges(64, -1.0)
ej = np.random.default_rng(4).choice([-1.0, 1.0], len(ea))
shape("64^3 +-J cubic", lambda: capi.Graph(ea, eb, ej, nvars=64 ** 3, force_general=True), 1024, 0.9)
say("done")

"""Cost and gain of the cluster series:
  1. cost of a row: the device time of a Swendsen-Wang step (k = 1) with a live series against the same binary without one, at
     1024^2 x 256 on the checkerboard path and at 64^3 x 1024 on the replica-packed path, the two variants alternated; stated in
     sweeps of the same container (all three between HIP events on its stream);
  2. gain of the estimator: 256^2 at beta_c, k = 1 -- the standard error over independent chains of chi from M^2 (observable series)
     and from S2 (cluster series) over the same run, and their ratio (reported, not asserted);
  3. the untouched path (--untouched; --parent with ISINGMC_LIB_PATH naming the parent commit's library): do_time_steps with k = 1 at
     1024^2 x 256 without a series and do_time_steps at the bench.py shape -- run this script once per binary in alternating
     processes and compare the medians with the spread of the parent's own medians.
Medians of five throughout; every line names its clock.  Output kept in profiles/<date>_cluster_series.txt."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from oracle import exact as X  # noqa: E402
from pyisingmontecarlo_amd import _capi as capi  # noqa: E402

PARENT, UNTOUCHED = "--parent" in sys.argv, "--untouched" in sys.argv or "--parent" in sys.argv
if PARENT:   # the parent commit's library has no cluster series entry points
    capi._CLUSTER_SERIES_PROTOTYPES.clear()
    del capi._PROTOTYPES["isingmc_host_nonlocal_steps"]
BETA_C = 0.4407


def say(*a):
    print(" ".join(str(x) for x in a), flush=True)


def device_ms(st, fn):
    """milliseconds of what fn enqueues on the container's stream, between two events"""
    stream = st.pt_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.synchronize()
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def fmt(xs):
    return f"median {float(np.median(xs)):.3f} ms (min {min(xs):.3f}, max {max(xs):.3f})"


def row_cost(name, g, R, beta, steps=4):
    sweeps = capi.States(g, capi.make_seeds(3, R))
    sweeps.do_time_steps(4, beta)
    sweep = [device_ms(sweeps, lambda: sweeps.do_time_steps(8, beta)) / 8 for _ in range(5)]
    del sweeps
    plain, logged = capi.States(g, capi.make_seeds(3, R)), capi.States(g, capi.make_seeds(3, R))
    for st in (plain, logged):
        st.set_cluster_every(1)
    series = logged.cluster_series(capacity=64)
    for st in (plain, logged):
        st.do_time_steps(steps, beta)   # (the same trajectory: the same clusters in both)
    without, with_series = [], []
    for _ in range(5):   # alternated
        without.append(device_ms(plain, lambda: plain.do_time_steps(steps, beta)) / steps)
        with_series.append(device_ms(logged, lambda: logged.do_time_steps(steps, beta)) / steps)
    assert series.count == 6 * steps
    s, a, b = float(np.median(sweep)), float(np.median(without)), float(np.median(with_series))
    say(f"== {name} x {R} replicas: family {plain.family}")
    say(f"device: one sweep {fmt(sweep)}; one cluster step without a series {fmt(without)} = {a / s:.2f} sweeps; with a series "
        f"{fmt(with_series)} = {b / s:.2f} sweeps; a row costs {(b - a) / s:+.3f} sweeps = {100 * (b - a) / a:+.2f} % of a step")


def estimator_gain():
    L, R, therm, T = 256, 64, 200, 1200
    st = capi.States(capi.Graph(*X.square_lattice_edges(L, L, -1.0)), capi.make_seeds(9, R))
    st.set_cluster_every(1)
    clusters = st.cluster_series(capacity=T)
    obs = st.observable_series(energy=False, capacity=T)
    obs.set_every(1)
    st.do_time_steps(T, BETA_C)
    s2 = clusters.get()[4][therm:].astype(np.float64).mean(axis=0) / L ** 2
    m2 = (obs.get()[2][therm:].astype(np.float64) ** 2).mean(axis=0) / L ** 2
    se_s2, se_m2 = s2.std(ddof=1) / np.sqrt(R), m2.std(ddof=1) / np.sqrt(R)
    say(f"== {L}^2 at beta_c, k = 1, {R} chains, {T - therm} steps after {therm}: chi from S2 {s2.mean():.1f} +- {se_s2:.1f}; from M^2 "
        f"{m2.mean():.1f} +- {se_m2:.1f}; standard error M^2 / S2 = {se_m2 / se_s2:.2f}")


def untouched():
    g = capi.Graph(*X.square_lattice_edges(1024, 1024, -1.0))
    st = capi.States(g, capi.make_seeds(3, 256))
    st.set_cluster_every(1)
    st.do_time_steps(4, BETA_C)
    steps = [device_ms(st, lambda: st.do_time_steps(4, BETA_C)) / 4 for _ in range(5)]
    say(f"no series, device: one cluster step at 1024^2 x 256: {fmt(steps)}")
    del st, g
    st = capi.States(capi.Graph(*X.square_lattice_edges(4096, 4096, -1.0)), capi.make_seeds(1, 256))
    st.do_time_steps(5, 0.44)
    sweeps = [device_ms(st, lambda: st.do_time_steps(20, 0.44)) / 20 for _ in range(5)]
    say(f"no series, device: one sweep at 4096^2 x 256: {fmt(sweeps)}")


with open(capi.lib()._name, "rb") as fh:
    say("# libisingmc.so sha256", hashlib.sha256(fh.read()).hexdigest(), "(parent)" if PARENT else "")
if UNTOUCHED:
    untouched()
    say("done")
    sys.exit(0)
row_cost("1024^2 lattice", capi.Graph(*X.square_lattice_edges(1024, 1024, -1.0)), 256, BETA_C)
estimator_gain()
os.environ["ISINGMC_FORCE_PACKED"] = "1"
ea, eb, ej = X.cubic_lattice_edges(64, -1.0)
row_cost("64^3 cube", capi.Graph(ea, eb, ej, nvars=64 ** 3, force_general=True), 1024, 0.2216)
say("done")

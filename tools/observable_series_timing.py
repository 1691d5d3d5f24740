"""Cost of the observable series:
  1. 1024^2 x 256 replicas, E + M: the device time of one record in units of the device time of one sweep of the same container
     (both between HIP events on its stream); on the host, what enqueueing a record costs the calling thread, a record followed by
     a wait, and energies() + magnetisations() with their waits;
  2. the same with the row and column tables;
  3. 64^3 +-J x 1024 replicas with the three axis tables;
  4. pt_run(200, 10) at 1024^2 x 64 rungs with a row every 10th timestep against the same run without a series;
  5. the untouched path: do_time_steps at the bench.py shape and pt_run(200, 10) without a series -- run this script once per binary,
     alternating, with --untouched (and ISINGMC_LIB_PATH naming the parent commit's library, --parent), and compare medians and spreads.
Best and median of five throughout; every line says whether its clock is the device's (HIP events) or the host's (wall clock), and no
ratio mixes the two.  Output kept in profiles/<date>_observable_series.txt."""
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from oracle import exact as X  # noqa: E402
from pyisingmontecarlo_amd import _capi as capi  # noqa: E402
from pyisingmontecarlo_amd.correlation import plane_classes  # noqa: E402

PARENT, UNTOUCHED = "--parent" in sys.argv, "--untouched" in sys.argv or "--parent" in sys.argv
if PARENT:   # the parent commit's library has no series entry points
    for name in [n for n in capi._PROTOTYPES if "observable_series" in n]:
        del capi._PROTOTYPES[name]


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


def host_ms(st, fn):
    st.synchronize()
    t0 = time.perf_counter()
    fn()
    st.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def fmt(xs):
    return f"{min(xs):.3f} ms (median {float(np.median(xs)):.3f}, max {max(xs):.3f})"


def record_cost(name, g, R, beta, tables):
    """Every figure names its clock: `device` = between two HIP events on the container's stream, `host` = wall clock of the calling
    thread.  The ratios compare like with like: record / sweep on the device, synchronising route / record with a wait on the host."""
    st = capi.States(g, capi.make_seeds(3, R))
    st.set_betas(np.full(R, beta))                        # one beta, as per-replica thresholds on the device
    st.do_time_steps(10)
    say(f"== {name} x {R} replicas: family {st.family}")
    sweep = [device_ms(st, lambda: st.do_time_steps(10)) / 10 for _ in range(5)]
    classes = capi.SiteClasses(g, tables) if tables is not None else None
    series = st.observable_series(classes=classes, capacity=64)
    series.record()
    rec = [device_ms(st, series.record) for _ in range(5)]

    def enqueue_ms():                                     # the host's share of a record: the call returns, nothing is waited for
        st.synchronize()
        t0 = time.perf_counter()
        series.record()
        return 1e3 * (time.perf_counter() - t0)
    enq = [enqueue_ms() for _ in range(5)]
    rec_wall = [host_ms(st, series.record) for _ in range(5)]
    sync = [host_ms(st, lambda: (st.energies(), st.magnetisations())) for _ in range(5)]
    say(f"device: one sweep {fmt(sweep)}; one record {fmt(rec)} = {min(rec) / min(sweep):.3f} sweeps")
    say(f"host: enqueueing one record {fmt(enq)}; one record and a wait {fmt(rec_wall)}; energies() + magnetisations() with their waits "
        f"{fmt(sync)} = {min(sync) / min(rec_wall):.2f} records with a wait")


def ladder(g, betas):
    st = capi.States(g, capi.make_seeds(5, len(betas)))
    st.pt_attach(betas, 0, len(betas), 1, 17)
    st.pt_run(20, 10)
    return st


def untouched(g_bench, g_ladder, betas):
    st = capi.States(g_bench, capi.make_seeds(1, 256))
    st.do_time_steps(5, 0.44)
    steps = [host_ms(st, lambda: st.do_time_steps(20, 0.44)) for _ in range(5)]
    say(f"no series: do_time_steps(20) at 4096^2 x 256: {fmt(steps)}")
    del st
    lad = ladder(g_ladder, betas)
    runs = [host_ms(lad, lambda: lad.pt_run(200, 10)) for _ in range(5)]
    say(f"no series: pt_run(200, 10) at 1024^2 x 64 rungs: {fmt(runs)}")


with open(capi.lib()._name, "rb") as fh:
    say("# libisingmc.so sha256", hashlib.sha256(fh.read()).hexdigest(), "(parent)" if PARENT else "")
g1024 = capi.Graph(*X.square_lattice_edges(1024, 1024, -1.0))
betas = 0.4400 + 0.0003 * np.arange(64) / 64
if UNTOUCHED:
    untouched(capi.Graph(*X.square_lattice_edges(4096, 4096, -1.0)), g1024, betas)
    say("done")
    sys.exit(0)
record_cost("1024^2 lattice, E + M", g1024, 256, 0.44, None)
record_cost("1024^2 lattice, E + M + row and column tables", g1024, 256, 0.44, plane_classes((1024, 1024)))
os.environ["ISINGMC_FORCE_PACKED"] = "1"
ea, eb, _ = X.cubic_lattice_edges(64, -1.0)
ej = np.random.default_rng(4).choice([-1.0, 1.0], len(ea))
record_cost("64^3 +-J cube, E + M + three axis tables", capi.Graph(ea, eb, ej, nvars=64 ** 3, force_general=True), 1024, 0.9,
            plane_classes((64, 64, 64)))
lad = ladder(g1024, betas)
series = lad.observable_series(by_rung=True, capacity=4096)
series.set_every(10)
with_series = []
for _ in range(5):
    with_series.append(host_ms(lad, lambda: lad.pt_run(200, 10)))
    assert series.count == 20
    series.reset()
plain = ladder(g1024, betas)
without = [host_ms(plain, lambda: plain.pt_run(200, 10)) for _ in range(5)]
say(f"pt_run(200, 10) at 1024^2 x 64 rungs with a row every 10th timestep: {fmt(with_series)}; without: {fmt(without)}; "
    f"with / without = {min(with_series) / min(without):.3f}")
say("done")

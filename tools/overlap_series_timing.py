"""Cost of the overlap series on ClassicalTempering(copies=2) ladders of 64 rungs:
  1. 1024^2 lattice, spin + link: the device time of one record (HIP events on the first copy's stream) in units of one sweep of
     one ladder, and the synchronising route get_overlaps() timed on the host, waits included;
  2. 64^3 +-J cube with the three axis tables: the same, with get_overlaps() + get_overlaps_by_class() as the synchronising route;
  3. the wall time of timesteps(200, 10) with a sample every 10th timestep against the same run without a series.
--parent: the library named by ISINGMC_LIB_PATH is the parent commit's (no series entry points): the run without a series alone,
for the comparison of the two binaries (one process each).  Best and median of five throughout.
Output kept in profiles/2026-10-20_overlap_series.txt."""
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
from pyisingmontecarlo_amd.tempering import ClassicalTempering  # noqa: E402

PARENT = "--parent" in sys.argv
if PARENT:
    for name in [n for n in capi._PROTOTYPES if "overlap_series" in n]:
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


def host_ms(pt, fn):
    for c in pt._pair:
        c._states.synchronize()
    t0 = time.perf_counter()
    fn()
    for c in pt._pair:
        c._states.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def fmt(xs):
    return f"{min(xs):.3f} ms (median {float(np.median(xs)):.3f})"


def ladder(edges, betas):
    pt = ClassicalTempering(edges, seed=11, copies=2)
    for b in betas:
        pt.add_graph(float(b))
    pt.timesteps(20, 10)
    return pt


def run(name, edges, betas, tables):
    pt = ladder(edges, betas)
    a = pt._pair[0]._states
    say(f"== {name} x {len(betas)} rungs, copies=2: family {a.family}, on the device's stream: {pt._on_stream}")
    plain = [host_ms(pt, lambda: pt.timesteps(200, 10)) for _ in range(5)]
    say(f"timesteps(200, 10) without a series: {fmt(plain)}")
    if PARENT:
        return
    sweep = [device_ms(a, lambda: a.pt_time_steps(1)) for _ in range(5)]
    pt._pair[1]._states.pt_time_steps(5)   # (the two copies stand at one timestep again)
    classes = pt.site_classes(tables) if tables is not None else None
    pt.set_measure_overlaps_every(10, classes=classes, capacity=4096)
    series = pt._ovl_series
    series.record()
    rec = [device_ms(a, series.record) for _ in range(5)]
    sync = [host_ms(pt, (lambda: (pt.get_overlaps(), pt.get_overlaps_by_class(classes))) if classes else pt.get_overlaps) for _ in range(5)]
    say(f"one sweep of one ladder {fmt(sweep)}; one record {fmt(rec)} = {min(rec) / min(sweep):.3f} sweeps; "
        f"the synchronising route on the host {fmt(sync)} = {min(sync) / min(rec):.1f} records")
    series.reset()
    with_series = []
    for _ in range(5):
        with_series.append(host_ms(pt, lambda: pt.timesteps(200, 10)))
        assert series.count == 20
        series.reset()
    again = [host_ms(plain_pt, lambda: plain_pt.timesteps(200, 10)) for plain_pt in [ladder(edges, betas)] for _ in range(5)]
    say(f"timesteps(200, 10) with a sample every 10th timestep: {fmt(with_series)}; without, a fresh ladder: {fmt(again)}; "
        f"with / without = {min(with_series) / min(again):.3f}")


with open(capi.lib()._name, "rb") as fh:
    say("# libisingmc.so sha256", hashlib.sha256(fh.read()).hexdigest(), "(parent)" if PARENT else "")
run("1024^2 lattice", X.square_lattice_edges(1024, 1024, -1.0), 0.4400 + 0.0003 * np.arange(64) / 64, None)
os.environ["ISINGMC_FORCE_PACKED"] = "1"
ea, eb, _ = X.cubic_lattice_edges(64, -1.0)
ej = np.random.default_rng(4).choice([-1.0, 1.0], len(ea))
run("64^3 +-J cube, three axis tables", (ea, eb, ej), np.linspace(0.6, 1.1, 64), plane_classes((64, 64, 64)))
say("done")

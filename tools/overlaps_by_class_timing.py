"""Cost of one overlap measurement by site class (isingmc_overlaps_by_class) next to the plain spin overlap
(isingmc_overlaps without the link overlap), next to what a user does without it -- states() plus the numpy rule of
tests/class_overlap_reference.py -- and next to one sweep, all in one session on the same container.  Shapes: 64^3 +-J x 1024 with
the three axis tables on the replica-packed bit-sliced path, 1024^2 +-J x 256 with row and column tables on the checkerboard path.
Device figures are HIP events recorded on the container's stream around the call (its kernels, copies and the gaps between its
batches); wall-clock figures are the synchronising call as the caller sees it.  Prints a text block for
profiles/<date>_overlaps_by_class.txt.

    python tools/overlaps_by_class_timing.py > profiles/$(date +%F)_overlaps_by_class.txt
"""
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPS = 20


def timed(st, call, reps=REPS):
    """(device ms, wall ms) of one call, each as (median, minimum) over reps after two warm-up calls."""
    import torch

    stream = st.pt_stream()
    for _ in range(2):   # the first call takes its blocks from the allocator
        call()
    dev, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(e0.elapsed_time(e1))
    return (np.median(dev), np.min(dev)), (np.median(wall), np.min(wall))


def time_container(name, st, cs, tables, beta):
    import class_overlap_reference as CR
    import overlap_reference as OR

    st.do_time_steps(20, beta)                        # warm clocks, thermalise a little
    sweep = [st.do_time_steps_timed(4, beta) / 4 for _ in range(10)]
    st.synchronize()
    s = np.median(sweep)
    pa, pb = OR.default_pairs(st.count)
    sa, sb = pa.astype(np.uint32), pb.astype(np.uint32)
    rows = [("1. overlaps_by_class, default pairing", timed(st, lambda: st.overlaps_by_class(cs))),
            ("   overlaps_by_class, the same pairs as slot tables", timed(st, lambda: st.overlaps_by_class(cs, None, sa, sb))),
            ("2. overlaps(link=False), default pairing", timed(st, lambda: st.overlaps(link=False)))]
    t0 = time.perf_counter()
    states = st.states()
    t1 = time.perf_counter()
    want = CR.overlaps_by_class(states, states, tables, cs.n_classes, pa, pb)
    t2 = time.perf_counter()
    assert np.array_equal(st.overlaps_by_class(cs), want) and np.array_equal(st.overlaps_by_class(cs, None, sa, sb), want)
    print(f"{name}: sweep {s:.4f} ms ({np.min(sweep):.4f}; HIP events); {len(pa)} pairs, {cs.n_tables} tables x {cs.n_classes} classes")
    for label, (dev, wall) in rows:
        print(f"  {label}: device {dev[0]:.4f} ms ({dev[1]:.4f}) = {dev[0] / s:.2f} sweeps; wall {wall[0]:.4f} ms ({wall[1]:.4f}) = {wall[0] / s:.2f} sweeps")
    route = 1e3 * (t2 - t0)
    print(f"  3. states() {1e3 * (t1 - t0):.1f} ms + numpy rule {1e3 * (t2 - t1):.1f} ms = {route:.1f} ms = {route / s:.0f} sweeps = "
          f"{route / rows[0][1][1][0]:.0f} x the wall clock of (1) (equal results)")
    assert rows[0][1][1][0] < route, "the device measurement must beat states() + numpy"


def main():
    from oracle import exact as X
    from pyisingmontecarlo_amd import _capi as capi
    from pyisingmontecarlo_amd import correlation as K
    import packed_icm_reference as IR

    sha = hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()
    print(f"# overlaps by site class: one isingmc_overlaps_by_class call next to isingmc_overlaps (spin alone), states() + numpy and one sweep; medians (minima) over {REPS} repetitions")
    print(f"# libisingmc.so sha256 {sha}")
    os.environ["ISINGMC_FORCE_PACKED"] = "1"
    ea, eb, ej = IR.cubic_glass(X, 64)
    g = capi.Graph(ea, eb, ej, nvars=64 ** 3, force_general=True, device=0)
    st = capi.States(g, capi.make_seeds(2, 1024))
    assert st.family == "packed_bitsliced"
    tables = K.plane_classes((64, 64, 64))
    time_container("packed bit-sliced 64^3 +-J x 1024", st, capi.SiteClasses(g, tables), tables, 0.5)
    st.close()
    del os.environ["ISINGMC_FORCE_PACKED"]
    ea, eb, ej = X.square_lattice_edges(1024, 1024, -1.0, np.random.default_rng(1))
    g = capi.Graph(ea, eb, ej, device=0)
    st = capi.States(g, capi.make_seeds(1, 256))
    assert st.family == "checkerboard"
    tables = K.plane_classes((1024, 1024))
    time_container("checkerboard 1024^2 +-J x 256", st, capi.SiteClasses(g, tables), tables, 0.4)


if __name__ == "__main__":
    main()

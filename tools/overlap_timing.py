"""Wall-clock time of one overlap measurement (isingmc_overlaps; the call synchronises) next to one sweep of the
same container and next to the route through states() plus the numpy rule of tests/overlap_reference.py.  Shapes: 1024^2 x 256 on
the checkerboard path and 64^3 +-J x 1024 on the replica-packed bit-sliced path.  Prints a text block for
profiles/<date>_overlaps.txt.

    python tools/overlap_timing.py > profiles/$(date +%F)_overlaps.txt
"""
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def wall_ms(call, reps=10):
    call()   # the first call takes its blocks from the allocator
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        out.append((time.perf_counter() - t0) * 1e3)
    return np.median(out), np.min(out)


def time_container(name, st, ea, eb, beta):
    import overlap_reference as OR

    st.do_time_steps(20, beta)                        # warm clocks, thermalise a little
    sweep = [st.do_time_steps_timed(4, beta) / 4 for _ in range(10)]
    st.synchronize()
    pa, pb = OR.default_pairs(st.count)
    sa, sb = pa.astype(np.uint32), pb.astype(np.uint32)
    both = wall_ms(lambda: st.overlaps())
    spin = wall_ms(lambda: st.overlaps(link=False))
    tables = wall_ms(lambda: st.overlaps(None, sa, sb))
    tables_spin = wall_ms(lambda: st.overlaps(None, sa, sb, link=False))
    t0 = time.perf_counter()
    states = st.states()
    t1 = time.perf_counter()
    want = OR.overlaps(states, states, ea, eb, pa, pb)
    t2 = time.perf_counter()
    got, got_tables = st.overlaps(), st.overlaps(None, sa, sb)
    assert all(np.array_equal(x, y) for x, y in zip(got, want)) and all(np.array_equal(x, y) for x, y in zip(got_tables, want))
    s = np.median(sweep)
    print(f"{name}: sweep {s:.4f} ms ({np.min(sweep):.4f}; HIP events); {len(pa)} pairs, wall clock of one synchronising call:")
    print(f"  default pairing, spin and link {both[0]:.4f} ms ({both[1]:.4f}) = {both[0] / s:.2f} sweeps; spin alone {spin[0]:.4f} ms ({spin[1]:.4f}) = {spin[0] / s:.2f} sweeps")
    print(f"  the same pairs as slot tables, spin and link {tables[0]:.4f} ms ({tables[1]:.4f}) = {tables[0] / s:.2f} sweeps; spin alone {tables_spin[0]:.4f} ms ({tables_spin[1]:.4f})")
    print(f"  states() {1e3 * (t1 - t0):.1f} ms + numpy rule {1e3 * (t2 - t1):.1f} ms = {(t2 - t0) / (1e-3 * both[0]):.0f} x the default call (equal results)")


def main():
    from oracle import exact as X
    from pyisingmontecarlo_amd import _capi as capi
    import packed_icm_reference as IR

    sha = hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()
    print("# overlaps: one isingmc_overlaps call next to one sweep and next to states() + numpy, medians (minima) over 10 repetitions")
    print(f"# libisingmc.so sha256 {sha}")
    ea, eb, ej = X.square_lattice_edges(1024, 1024, -1.0, np.random.default_rng(1))
    st = capi.States(capi.Graph(ea, eb, ej, device=0), capi.make_seeds(1, 256))
    time_container("checkerboard 1024^2 +-J x 256", st, ea, eb, 0.4)
    st.close()
    os.environ["ISINGMC_FORCE_PACKED"] = "1"
    ea, eb, ej = IR.cubic_glass(X, 64)
    st = capi.States(capi.Graph(ea, eb, ej, nvars=64 ** 3, force_general=True, device=0), capi.make_seeds(2, 1024))
    assert st.family == "packed_bitsliced"
    time_container("packed bit-sliced 64^3 +-J x 1024", st, ea, eb, 0.5)


if __name__ == "__main__":
    main()

"""What the step chooser of population annealing costs, on one MI355X.  Shapes: 1024^2 x 256 on the checkerboard
path and 64^3 +-J x 1024 on the replica-packed bit-sliced path (those of tools/pa_timing.py), and a population of 2^20 on the 4^3
+-J lattice.  Per shape:
  1. the device time of one isingmc_pa_choose_step between HIP events, next to one sweep of the same container;
  2. the host wall time of that call, against get_energies() plus the host twin on the same energies (what a user had before);
  3. the wall time of isingmc_pa_run_adaptive, against isingmc_pa_run on the betas it chose (the price of the wait per step).
--fixed: one fixed-schedule isingmc_pa_run alone (entry points the parent commit has too: run it in alternating processes with
ISINGMC_LIB_PATH naming the parent commit's library, next to bench.py, to see that the existing paths did not move).

    python tools/pa_adaptive_timing.py > profiles/$(date +%F)_pa_adaptive.txt
"""
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TARGET = 0.85


def _wall(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return np.array(out)


def time_container(capi, make, beta, dbeta_max, sweeps, reps=10):
    import torch
    st = make()
    stream = st.pt_stream()
    st.do_time_steps(20, beta)                        # warm clocks, thermalise a little
    sweep = [st.do_time_steps_timed(4, beta) / 4 for _ in range(reps)]
    st.pa_choose_step(dbeta_max, TARGET)              # the first call allocates the chooser's blocks
    device = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        choice = st.pa_choose_step(dbeta_max, TARGET)
        e1.record(stream)
        e1.synchronize()
        device.append(e0.elapsed_time(e1))
    wall = _wall(lambda: st.pa_choose_step(dbeta_max, TARGET), reps)
    twin = {}

    def by_hand():
        twin.update(capi.pa_choose_step(st.energies(), dbeta_max, TARGET))

    hand = _wall(by_hand, 3)
    assert twin == choice, (twin, choice)
    copy = _wall(lambda: st.energies(), reps)
    print(f"  one sweep {np.median(sweep):.4f} ms ({np.min(sweep):.4f}); choose_step between events {np.median(device):.4f} ms ({np.min(device):.4f}), "
          f"{np.median(device) / np.median(sweep):.2f} sweeps; k = {choice['k']}, dbeta = {choice['dbeta']:.6g}")
    print(f"  host wall: choose_step {np.median(wall):.4f} ms ({np.min(wall):.4f}); get_energies() + host twin {np.median(hand):.3f} ms ({np.min(hand):.3f}), "
          f"of which get_energies() {np.median(copy):.4f} ms: {np.median(hand) / np.median(wall):.1f} x")
    st.close()
    # a whole schedule: adaptive, then the fixed one on the betas it chose, on fresh containers of the same seeds; three times each
    adaptive, fixed = [], []
    for _ in range(3):
        a = make()
        a.synchronize()
        t0 = time.perf_counter()
        log = a.pa_run_adaptive(beta, beta + 40 * dbeta_max / 16, sweeps, 999, TARGET, dbeta_cap=dbeta_max)
        adaptive.append((time.perf_counter() - t0) * 1e3)
        a.close()
        b = make()
        b.synchronize()
        t0 = time.perf_counter()
        b.pa_run(log["betas"], sweeps, 999)
        fixed.append((time.perf_counter() - t0) * 1e3)
        b.close()
    n = len(log["betas"]) - 1
    print(f"  schedule of {n} chosen steps x {sweeps} sweeps: pa_run_adaptive {np.median(adaptive):.2f} ms, pa_run on its betas {np.median(fixed):.2f} ms: "
          f"{(np.median(adaptive) - np.median(fixed)) / max(n, 1):.4f} ms per step more ({np.median(adaptive) / np.median(fixed):.3f} x)")


def shapes(capi):
    from oracle import exact as X
    import packed_icm_reference as IR

    def board():
        ea, eb, ej = X.square_lattice_edges(1024, 1024, -1.0)
        return capi.States(capi.Graph(ea, eb, ej, device=0), capi.make_seeds(1, 256))

    def cubic(L, R):
        def make():
            os.environ["ISINGMC_FORCE_PACKED"] = "1"
            ea, eb, ej = IR.cubic_glass(X, L)
            st = capi.States(capi.Graph(ea, eb, ej, nvars=L ** 3, force_general=True, device=0), capi.make_seeds(2, R))
            assert st.family == "packed_bitsliced"
            return st
        return make

    # dbeta_max: about four times the step the rule takes at these betas, so that the search ends inside the grid
    return (("checkerboard 1024^2 x 256", board, 0.4, 0.004, 4), ("packed bit-sliced 64^3 +-J x 1024", cubic(64, 1024), 0.5, 0.008, 4),
            ("packed bit-sliced 4^3 +-J x 2^20", cubic(4, 1 << 20), 0.5, 0.2, 4))


def main():
    from pyisingmontecarlo_amd import _capi as capi
    sha = hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()
    print(f"# libisingmc.so sha256 {sha}")
    if "--fixed" in sys.argv:
        _, make, beta, dbeta_max, sweeps = shapes(capi)[1]
        st = make()
        betas = beta + np.arange(41) * dbeta_max / 16
        st.do_time_steps(20, beta)
        runs = []
        for _ in range(5):
            st.synchronize()
            t0 = time.perf_counter()
            st.pa_run(betas, sweeps, 999)
            runs.append((time.perf_counter() - t0) * 1e3)
        print(f"fixed pa_run, 41 betas x {sweeps} sweeps, 64^3 +-J x 1024: median of five {np.median(runs):.3f} ms (min {np.min(runs):.3f})")
        return
    print("# population annealing, steps chosen on the device: HIP events and host wall clock, medians (minima) over 10 repetitions")
    for name, make, beta, dbeta_max, sweeps in shapes(capi):
        print(name)
        time_container(capi, make, beta, dbeta_max, sweeps)


if __name__ == "__main__":
    main()

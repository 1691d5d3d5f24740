"""Device time of one population-annealing resampling (isingmc_pa_resample) next to one sweep of the same container, with HIP
events on the engine's stream.  Shapes: 1024^2 x 256 on the checkerboard path and 64^3 +-J x 1024 on the
replica-packed bit-sliced path.  Prints a text block for profiles/<date>_population_annealing.txt.

    python tools/pa_timing.py > profiles/$(date +%F)_population_annealing.txt
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def time_container(capi, st, beta, reps=10):
    import torch
    stream = st.pt_stream()
    st.do_time_steps(20, beta)                        # warm clocks, thermalise a little
    sweep = [st.do_time_steps_timed(4, beta) / 4 for _ in range(reps)]
    resample = []
    for k in range(reps + 2):
        st.do_time_steps(2, beta)                     # separate the copies again
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        st.pa_resample(0.01, 12345, k + 1)
        e1.record(stream)
        e1.synchronize()
        resample.append(e0.elapsed_time(e1))
    resample = resample[2:]                           # the first call allocates the second buffer
    # behind queued work: a schedule of 41 betas x 4 sweeps in ONE enqueue-only call (isingmc_pa_run) against the same 164 sweeps alone
    import time
    betas = np.linspace(beta, beta + 0.004, 41)
    queued = []
    for _ in range(3):
        st.synchronize()
        t0 = time.perf_counter()
        log = st.pa_run(betas, 4, 999)
        t1 = time.perf_counter()
        queued.append(((t1 - t0) * 1e3 - 164 * np.median(sweep)) / 40)
    return (np.median(sweep), np.min(sweep), np.median(resample), np.min(resample), st.pa_last()["distinct"], np.median(queued),
            int(np.median(log["distinct"])))


def main():
    from oracle import exact as X
    from pyisingmontecarlo_amd import _capi as capi
    import packed_icm_reference as IR

    sha = hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()
    print(f"# population annealing: one resampling next to one sweep, HIP events, medians (minima) over 10 repetitions")
    print(f"# libisingmc.so sha256 {sha}")
    ea, eb, ej = X.square_lattice_edges(1024, 1024, -1.0)
    st = capi.States(capi.Graph(ea, eb, ej, device=0), capi.make_seeds(1, 256))
    s, smin, r, rmin, d, q, qd = time_container(capi, st, 0.4)
    print(f"checkerboard 1024^2 x 256: sweep {s:.4f} ms ({smin:.4f}), resampling on an idle stream {r:.4f} ms ({rmin:.4f}), ratio {r / s:.2f}, {d} distinct sources")
    print(f"  inside a 41-beta schedule of one call (wall clock minus the sweeps, per resampling): {q:.4f} ms, ratio {q / s:.2f}, {qd} distinct sources (median)")
    st.close()
    os.environ["ISINGMC_FORCE_PACKED"] = "1"
    ea, eb, ej = IR.cubic_glass(X, 64)
    st = capi.States(capi.Graph(ea, eb, ej, nvars=64 ** 3, force_general=True, device=0), capi.make_seeds(2, 1024))
    assert st.family == "packed_bitsliced"
    s, smin, r, rmin, d, q, qd = time_container(capi, st, 0.5)
    print(f"packed bit-sliced 64^3 +-J x 1024: sweep {s:.4f} ms ({smin:.4f}), resampling on an idle stream {r:.4f} ms ({rmin:.4f}), ratio {r / s:.2f}, {d} distinct sources")
    print(f"  inside a 41-beta schedule of one call (wall clock minus the sweeps, per resampling): {q:.4f} ms, ratio {q / s:.2f}, {qd} distinct sources (median)")


if __name__ == "__main__":
    main()

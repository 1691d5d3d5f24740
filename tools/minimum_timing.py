"""Cost of minimum tracking (isingmc_best_*), wall clock around enqueue + wait: one update when no replica
improves and when all do, next to one sweep; a 41-beta population-annealing run with and without tracking; a tempering ladder with
tracking on against the same ladder with pt_in_kernel = 0 and with the default (in-kernel rounds).  Shapes: 1024^2 x 256 on the
checkerboard path and 64^3 +-J x 1024 on the replica-packed bit-sliced path; the ladder is 1024^2 x 16 rungs.  Prints a text block
for profiles/<date>_minimum.txt.

    python tools/minimum_timing.py > profiles/$(date +%F)_minimum.txt
"""
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROUNDS_PERIOD = 1 << 62   # tracking on, no periodic update: the resamplings / exchange rounds are the update points


def wall_ms(call, before=lambda: None, reps=10):
    out = []
    for _ in range(reps + 1):   # the first repetition takes its blocks from the allocator
        before()
        t0 = time.perf_counter()
        call()
        out.append((time.perf_counter() - t0) * 1e3)
    return np.median(out[1:]), np.min(out[1:])


def time_updates(name, st, beta):
    st.do_time_steps(20, beta)
    sweep = [st.do_time_steps_timed(4, beta) / 4 for _ in range(10)]
    st.synchronize()

    def update():
        st.best_update()
        st.synchronize()

    update()
    none = wall_ms(update)                      # the configurations do not change: nobody beats the record
    assert st.best(states=False)[3] == st.count
    every = wall_ms(update, before=st.best_reset)   # records back to +inf: everybody does
    assert st.best(states=False)[3] == st.count
    energies = wall_ms(lambda: st.energies())
    s = np.median(sweep)
    print(f"{name}: sweep {s:.4f} ms ({np.min(sweep):.4f}; HIP events); one update, enqueue + wait:")
    print(f"  no replica improves {none[0]:.4f} ms ({none[1]:.4f}) = {none[0] / s:.2f} sweeps; all improve {every[0]:.4f} ms ({every[1]:.4f}) = {every[0] / s:.2f} sweeps; "
          f"get_energies alone {energies[0]:.4f} ms ({energies[1]:.4f})")


def time_population(name, make, betas, sweeps):
    res = []
    for track in (False, True):
        st = make()
        if track:
            st.set_track_best(ROUNDS_PERIOD)
        res.append(wall_ms(lambda: st.pa_run(betas, sweeps, 99), reps=3))
        st.close()
    print(f"{name}: pa_run of {len(betas)} betas x {sweeps} sweeps: {res[0][0]:.2f} ms ({res[0][1]:.2f}) without, {res[1][0]:.2f} ms ({res[1][1]:.2f}) with tracking "
          f"= +{100 * (res[1][0] / res[0][0] - 1):.1f} %")


def time_ladder(capi, g, rungs, timesteps, swap_every):
    out = {}
    for label in ("default", "pt_in_kernel = 0", "tracking on"):
        st = capi.States(g, capi.make_seeds(5, rungs))
        if label == "pt_in_kernel = 0":
            st.set_option("pt_in_kernel", 0)
        st.pt_attach(np.linspace(0.40, 0.48, rungs), 0, rungs, 1, 17)
        if label == "tracking on":
            st.set_track_best(ROUNDS_PERIOD)

        def run():
            st.pt_run(timesteps, swap_every)
            st.synchronize()

        out[label] = wall_ms(run, reps=5)
        st.close()
    base = out["default"][0]
    print(f"ladder 1024^2 x {rungs} rungs, pt_run({timesteps}, {swap_every}): " +
          "; ".join(f"{k} {v[0]:.3f} ms ({v[1]:.3f}) = {v[0] / base:.2f} x" for k, v in out.items()))


def main():
    from oracle import exact as X
    from pyisingmontecarlo_amd import _capi as capi
    import packed_icm_reference as IR

    sha = hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()
    print("# minimum tracking: wall clock of enqueue + wait, medians (minima)")
    print(f"# libisingmc.so sha256 {sha}")
    betas = np.linspace(0.1, 0.9, 41)
    ea, eb, ej = X.square_lattice_edges(1024, 1024, -1.0, np.random.default_rng(1))
    g = capi.Graph(ea, eb, ej, device=0)
    st = capi.States(g, capi.make_seeds(1, 256))
    time_updates("checkerboard 1024^2 +-J x 256", st, 0.4)
    st.close()
    time_population("checkerboard 1024^2 +-J x 256", lambda: capi.States(g, capi.make_seeds(1, 256)), betas, 10)
    time_ladder(capi, g, 16, 200, 10)
    os.environ["ISINGMC_FORCE_PACKED"] = "1"
    ea, eb, ej = IR.cubic_glass(X, 64)
    g = capi.Graph(ea, eb, ej, nvars=64 ** 3, force_general=True, device=0)
    st = capi.States(g, capi.make_seeds(2, 1024))
    time_updates("packed bit-sliced 64^3 +-J x 1024", st, 0.5)
    st.close()
    time_population("packed bit-sliced 64^3 +-J x 1024", lambda: capi.States(g, capi.make_seeds(2, 1024)), betas, 10)


if __name__ == "__main__":
    main()

"""Cluster-step measurements for profiles/cluster_update.txt: device time per Swendsen-Wang cluster step next to the Metropolis
sweep of the same container (HIP events of isingmc_do_time_steps_timed), and the integrated autocorrelation time of the energy at
512^2, beta_c for cluster_every = 0, 1, 5.

  python tools/cluster_profile.py [--skip-tau] [--tau-steps N] > profiles/cluster_update.txt
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import exact  # noqa: E402
from pyisingmontecarlo_amd import _capi  # noqa: E402

BETA_C = 0.4407


def tau_int(series):
    """Integrated autocorrelation time (in timesteps) per replica with Sokal's automatic window (c = 6), averaged over replicas;
    series[R, T].  Also returns the largest window used: an estimate close to T / 10 is a lower bound, not a measurement."""
    x = series - series.mean(axis=1, keepdims=True)
    T = x.shape[1]
    f = np.fft.rfft(x, n=2 * T, axis=1)
    acf = np.fft.irfft(f * np.conj(f), axis=1)[:, :T] / np.arange(T, 0, -1)
    rho = (acf / acf[:, :1]).mean(axis=0)  # replicas are independent and identically distributed: average the normalised ACFs
    tau, window = 0.5, T - 1
    for w in range(1, T):
        tau += rho[w]
        if w >= 6 * tau:
            window = w
            break
    return tau, window


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-tau", action="store_true")
    ap.add_argument("--tau-steps", type=int, default=4000)
    args = ap.parse_args()
    print("library sha256", hashlib.sha256(open(_capi.LIB_PATH, "rb").read()).hexdigest())
    print("\n# device time per timestep (HIP events), random start + 20 warm-up timesteps at beta_c, then `steps` timed timesteps")
    print("# bytes per cluster step and site: labels 4 W + 8 R (label, root's label), sizes 4 W + 4 R, bonds / flip table / spins ~1: 21 B")
    for L, R, steps in ((256, 64, 200), (1024, 64, 100), (4096, 256, 20)):
        g = _capi.Graph(*exact.square_lattice_edges(L, L, -1.0), L * L)
        st = _capi.States(g, _capi.make_seeds(1, R))
        st.do_time_steps(20, BETA_C)
        sweep_ms = st.do_time_steps_timed(steps, BETA_C) / steps
        st.set_cluster_every(1)
        st.do_time_steps(20, BETA_C)
        cluster_ms = st.do_time_steps_timed(steps, BETA_C) / steps
        n, largest = st.cluster_stats()
        gbs = 21.0 * L * L * R / (cluster_ms * 1e-3) / 1e9
        print(f"{L}^2 x {R}: sweep {sweep_ms * 1e3:10.1f} us   cluster step {cluster_ms * 1e3:10.1f} us   ratio {cluster_ms / sweep_ms:7.1f}   "
              f"{gbs:7.0f} GB/s = {gbs / 8000:.3f} of 8 TB/s   clusters {n.mean():.0f}  largest {largest.mean():.0f}")
        st.close()
        g.close()
    if args.skip_tau:
        return
    L, R, T = 512, 64, args.tau_steps
    print(f"\n# integrated autocorrelation time of E, {L}^2 x {R} at beta_c, all-up start, {T // 4} timesteps discarded, {T} measured")
    g = _capi.Graph(*exact.square_lattice_edges(L, L, -1.0), L * L)
    for k in (0, 1, 5):
        st = _capi.States(g, _capi.make_seeds(2, R), initial_state=np.ones(L * L, np.uint8))
        st.set_cluster_every(k)
        st.do_time_steps(T // 4, BETA_C)
        ms = st.do_time_steps_timed(T, BETA_C) / T
        e = st.do_time_steps(T, BETA_C, per_step_energies=True)
        tau, window = tau_int(e)
        bound = "  (window ~ run length: a LOWER bound)" if window > T // 20 else ""
        print(f"cluster_every {k}: tau_int {tau:9.1f} timesteps (window {window}){bound}   {ms * 1e3:9.1f} us per timestep   "
              f"tau_int x time = {tau * ms:10.3f} ms per independent sample")
        st.close()


if __name__ == "__main__":
    main()

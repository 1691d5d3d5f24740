"""The lag ring restated in numpy on states() arrays, and a plain restatement of correlation.integrated_time.

Sample j (0, 1, ... since the last reset): for every replica r and every lag l = 1 .. min(j, L), diff[r][l] += the number of sites
that differ between now and sample j - l; then the configuration is stored as snapshot j mod L.  counts[l] = max(0, samples - l)."""
import numpy as np


class LagRing:
    def __init__(self, n_lags, n_replicas):
        self.L, self.R = int(n_lags), int(n_replicas)
        self.reset()

    def reset(self):
        self.samples = 0
        self.slots = [None] * self.L
        self.diff = np.zeros((self.R, self.L + 1), dtype=np.uint64)

    def plan(self):
        """(slot_of_lag, live, write_slot, counts) before the next sample, as isingmc_host_autocorr_plan states them"""
        j, L = self.samples, self.L
        live, write = min(j, L), j % L
        slots = np.full(L + 1, 0xFFFFFFFF, dtype=np.uint32)
        slots[0] = write
        for l in range(1, live + 1):
            slots[l] = (j - l) % L
        return slots, live, write, self.counts

    def add(self, states):
        """states: bool / uint8 [R, nvars], the configurations of one sample"""
        s = np.asarray(states).astype(np.uint8)
        assert s.shape[0] == self.R
        slots, live, write, _ = self.plan()
        for l in range(1, live + 1):
            self.diff[:, l] += (s != self.slots[slots[l]]).sum(axis=1).astype(np.uint64)
        self.slots[write] = s.copy()
        self.samples += 1

    @property
    def counts(self):
        return np.array([max(0, self.samples - l) for l in range(self.L + 1)], dtype=np.uint64)


def diff_from_samples(samples, n_lags):
    """samples[R, S, nvars] (run_monte_carlo_sampling's states) -> (counts, diff) of a ring of n_lags over the S samples"""
    samples = np.asarray(samples)
    ring = LagRing(n_lags, samples.shape[0])
    for k in range(samples.shape[1]):
        ring.add(samples[:, k, :])
    return ring.counts, ring.diff


def integrated_time(corr_row, c=6.0):
    """(tau, window) of ONE row: tau(W) = 1/2 + sum_{l=1..W} C(l) added in the order of l; the smallest W >= c tau(W); without one
    the last lag and -1"""
    tau = 0.5
    for W in range(1, len(corr_row)):
        tau = tau + float(corr_row[W])
        if W >= c * tau:
            return tau, W
    return tau, -1

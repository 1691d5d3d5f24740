"""The moment sums of DESIGN.md S18 restated in numpy, from configurations as get_states() returns them (bool, True = +1).

site_sums / bond_sums take samples[S, R, N] (or one sample [R, N]); Accumulator gathers them one sample at a time, as the twin
container of tests/test_gpu_moments.py is read."""
import numpy as np


def spins(states):
    return 2 * np.asarray(states, dtype=np.int64) - 1


def site_sums(samples, per_replica=False):
    """int64[N]: the sum of s_i over samples and replicas; per_replica: int64[R, N], over the samples of each replica."""
    s = spins(samples)
    s = s.reshape((-1,) + s.shape[-2:])
    return s.sum(axis=0) if per_replica else s.sum(axis=(0, 1))


def bond_sums(samples, ea, eb):
    """int64[n_edges]: the sum of s_a s_b over samples and replicas, one term per entry of the edge list -- whatever its coupling,
    duplicated entries each on their own, +1 per sample and replica for an entry with a == b."""
    s = spins(samples)
    s = s.reshape((-1, s.shape[-1]))
    ea, eb = np.asarray(ea, dtype=np.int64), np.asarray(eb, dtype=np.int64)
    return (s[:, ea] * s[:, eb]).sum(axis=0)


class Accumulator:
    def __init__(self, ea, eb, per_replica=False):
        self.ea, self.eb, self.per_replica = ea, eb, per_replica
        self.n, self.site, self.bond = 0, 0, 0

    def add(self, states):
        self.n += 1
        self.site = self.site + site_sums(states[None], self.per_replica)
        self.bond = self.bond + bond_sums(states[None], self.ea, self.eb)

    def reset(self):
        self.n, self.site, self.bond = 0, 0, 0

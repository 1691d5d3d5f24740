"""Reference for the per-site spin sums by rung of a tempering ladder -- TEST INFRASTRUCTURE, numpy only: rung i
of a sample adds the configuration of the slot that holds it, perm[i], as +-1 spins (True = +1)."""
import numpy as np


class Accumulator:
    """site int64[G, N]: add(states bool[R, N] by slot, perm uint32[G] rung -> slot) adds 2 * states[perm[i]] - 1 into row i."""

    def __init__(self, n_rungs, nvars):
        self.site = np.zeros((int(n_rungs), int(nvars)), dtype=np.int64)
        self.n = 0
        self.perms = []   # the permutation of every sample, for the tests' own conditions

    def add(self, states, perm):
        states, perm = np.asarray(states), np.asarray(perm)
        assert states.ndim == 2 and states.shape[1] == self.site.shape[1] and perm.shape == (self.site.shape[0],)
        assert sorted(perm.tolist()) == list(range(len(perm))), "perm must be a permutation of the rungs' slots"
        self.site += 2 * states[perm.astype(np.int64)].astype(np.int64) - 1
        self.n += 1
        self.perms.append(perm.copy())

    def reset(self):
        self.site[:] = 0
        self.n = 0
        self.perms = []

    def saw_a_permutation(self):
        """was at least one sample taken under a permutation that is not the identity?"""
        return any(not np.array_equal(p, np.arange(len(p))) for p in self.perms)

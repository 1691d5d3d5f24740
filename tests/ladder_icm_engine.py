"""Test-side stand-ins for tempering ladders with isoenergetic cluster moves between two copies -- TEST
INFRASTRUCTURE, no GPU: an oracle-backed engine whose containers carry `icm_between` (sweeps by the CPU oracle, the move by
tests/icm_reference.py), and the whole ladder loop restated on its own from the S10 text."""
import numpy as np

import icm_reference as IR
from helpers import OracleLatStates

COPY_SEED_XOR = 0x9E3779B97F4A7C15   # S10: copy 1 is the ladder of seed ^ this


class OracleIcmStates(OracleLatStates):
    """OracleLatStates plus the move between two containers, host slot tables only (the oracle has no ladder on a device)."""

    def __init__(self, lat, seeds, W, H):
        super().__init__(lat, seeds)
        self.W, self.H = W, H
        self.last_stats = None

    def icm_between(self, other, slots_a=None, slots_b=None):
        assert slots_a is not None and slots_b is not None and other is not self and self.t == other.t
        stats = []
        for sa, sb in zip(slots_a, slots_b):
            a = self.lat.unpack(self.st[sa]).reshape(self.H, self.W)
            b = self.lat.unpack(other.st[sb]).reshape(self.H, self.W)
            a, b, st = IR.icm_step(a, b, self.seeds[sa], self.t)
            self.st[sa], other.st[sb] = self.lat.pack(a.ravel()), self.lat.pack(b.ravel())
            stats.append(st)
        self.last_stats = stats
        self.t += 1
        other.t += 1

    def icm_between_stats(self):
        return tuple(np.array([s[i] for s in self.last_stats], dtype=np.uint64) for i in range(3))


class OracleIcmEngine:
    def __init__(self, W, H, jr, jd):
        self.lat = IR.make_lat(W, H, jr, jd)
        self.W, self.H, self.nvars = W, H, W * H

    def make_states(self, seeds, replica_range=None):
        lo, hi = replica_range if replica_range is not None else (0, len(seeds))
        return OracleIcmStates(self.lat, seeds[lo:hi], self.W, self.H)


def ladder_seeds(capi, seed, G):
    """(slot seeds [2][G], exchange seeds [2]) of a copies=2 ladder whose rungs were added without explicit seeds."""
    ex = [int(seed), int(seed) ^ COPY_SEED_XOR]
    return [[int(capi.make_seeds(e, n)[-1]) for n in range(1, G + 1)] for e in ex], ex


class LadderRestatement:
    """Two ladders over `betas` on one +-J sample, restated: a timestep is a sweep of every slot at the beta of its rung, or -- when
    t % k == k - 1 -- a cluster move between the two configurations at every rung; an exchange round per copy after every f-th
    timestep of a call, after the timestep itself."""

    def __init__(self, capi, W, H, jr, jd, betas, seed, k):
        self.capi, self.W, self.H, self.jr, self.jd = capi, W, H, jr, jd
        self.betas, self.k, self.t = [float(b) for b in betas], int(k), 0
        G = len(self.betas)
        self.lat = IR.make_lat(W, H, jr, jd)
        self.seeds, self.exchange_seeds = ladder_seeds(capi, seed, G)
        self.spins = [[self.lat.unpack(self.lat.init(s)).reshape(H, W) for s in self.seeds[c]] for c in range(2)]
        self.perm = [np.arange(G, dtype=np.uint32) for _ in range(2)]   # rung -> slot
        self.rounds, self.swaps = [0, 0], [0, 0]
        self.stats = None
        self.icm_log = []   # (t, sum over both copies of E per rung before, after, q = -1 sites before, after)

    def energies(self, c):
        return np.array([IR.energy(s, self.jr, self.jd) for s in self.spins[c]])

    def step(self):
        """One timestep; returns the energies [2][G] by SLOT after it."""
        G = len(self.betas)
        if self.k and self.t % self.k == self.k - 1:
            before = [IR.energy(self.spins[0][self.perm[0][r]], self.jr, self.jd) + IR.energy(self.spins[1][self.perm[1][r]], self.jr, self.jd) for r in range(G)]
            q_before = [int((self.spins[0][self.perm[0][r]] ^ self.spins[1][self.perm[1][r]]).sum()) for r in range(G)]
            self.stats = []
            for r in range(G):
                sa, sb = int(self.perm[0][r]), int(self.perm[1][r])
                self.spins[0][sa], self.spins[1][sb], st = IR.icm_step(self.spins[0][sa], self.spins[1][sb], self.seeds[0][sa], self.t)
                self.stats.append(st)
            after = [IR.energy(self.spins[0][self.perm[0][r]], self.jr, self.jd) + IR.energy(self.spins[1][self.perm[1][r]], self.jr, self.jd) for r in range(G)]
            q_after = [int((self.spins[0][self.perm[0][r]] ^ self.spins[1][self.perm[1][r]]).sum()) for r in range(G)]
            self.icm_log.append((self.t, before, after, q_before, q_after))
        else:
            for c in range(2):
                beta_of_slot = np.empty(G)
                beta_of_slot[self.perm[c]] = self.betas
                for slot in range(G):
                    st = self.lat.pack(self.spins[c][slot].ravel())
                    self.lat.sweep(st, self.seeds[c][slot], self.t, beta_of_slot[slot])
                    self.spins[c][slot] = self.lat.unpack(st).reshape(self.H, self.W)
        self.t += 1
        return [self.energies(c) for c in range(2)]

    def exchange(self):
        for c in range(2):
            self.swaps[c] += self.capi.pt_swap_round(self.exchange_seeds[c], self.rounds[c], self.betas, self.energies(c), self.perm[c])
            self.rounds[c] += 1

    def timesteps(self, T, f):
        """One ClassicalTempering.timesteps(T, f) call."""
        for n in range(1, T + 1):
            self.step()
            if f and n % f == 0:
                self.exchange()

    def by_rung(self, c):
        """bool[G, N]: the configuration at every rung of copy c."""
        return np.stack([self.spins[c][int(s)].ravel().astype(bool) for s in self.perm[c]])

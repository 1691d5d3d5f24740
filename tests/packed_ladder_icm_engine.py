"""An oracle-backed engine for tempering ladders with isoenergetic cluster moves between two copies on the replica-packed
families -- TEST INFRASTRUCTURE, no GPU: sweeps by the CPU oracle's engine D (`oracle.pk_run`, bit-sliced family)
or E (`oracle.rj_run`, real-coupling family) with per-replica betas, the move by tests/packed_between_reference.py.  What
tests/ladder_icm_engine.py is for the checkerboard lattice."""
import numpy as np

import packed_between_reference as BR
from helpers import OracleRjEngine, OracleRjStates


class OraclePackedIcmStates(OracleRjStates):
    """OracleRjStates plus the move between two containers, host slot tables only (the oracle has no ladder on a device)."""

    def __init__(self, eng, seeds, lo, hi):
        super().__init__(eng, seeds, lo, hi)
        self.last_stats = None

    def _rows(self):
        if self.st is None:
            self.do_time_steps(0, 0.0)   # the random start
        return self.st

    def icm_between(self, other, slots_a=None, slots_b=None):
        assert slots_a is not None and slots_b is not None and other is not self and self.t == other.t
        A, B = self._rows(), other._rows()
        stats = []
        for sa, sb in zip(slots_a, slots_b):
            seed, bit = BR.slot_key(self.all_seeds, self.lo, sa)
            ra, rb = self.lo + int(sa), other.lo + int(sb)
            A[ra], B[rb], st = BR.move_pair(self.eng.G, A[ra], B[rb], seed, bit, self.t)
            stats.append(st)
        self.last_stats = stats
        self.t += 1
        other.t += 1

    def icm_between_stats(self):
        return tuple(np.array([s[i] for s in self.last_stats], dtype=np.uint64) for i in range(3))


class OraclePackedIcmEngine(OracleRjEngine):
    def __init__(self, ea, eb, ej, nvars, biases=None, bit_sliced=False):
        super().__init__(ea, eb, ej, nvars, biases=biases, bit_sliced=bit_sliced)
        self.G = BR.Graph(ea, eb, ej, nvars)

    def make_states(self, seeds, replica_range=None):
        lo, hi = replica_range if replica_range is not None else (0, len(seeds))
        return OraclePackedIcmStates(self, seeds, lo, hi)

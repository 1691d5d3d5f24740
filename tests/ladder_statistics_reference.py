"""The ladder statistics of DESIGN.md S20, restated in plain numpy from the rule's text -- TEST INFRASTRUCTURE, no GPU and no
library call.  One object per ladder; round(round_number, perm_before, perm_after, slot_energy) is one exchange round."""
import numpy as np

NONE, UP, DOWN = 0, 1, 2
ARRAYS = ("attempts", "accepts", "n_up", "n_down", "sum_e", "sum_e2", "round_trips", "labels")


class Statistics:
    def __init__(self, n_rungs):
        self.n = int(n_rungs)
        self.reset()

    def reset(self):
        n = self.n
        self.rounds = 0
        self.attempts = np.zeros(max(n - 1, 0), dtype=np.uint64)
        self.accepts = np.zeros(max(n - 1, 0), dtype=np.uint64)
        self.n_up = np.zeros(n, dtype=np.uint64)
        self.n_down = np.zeros(n, dtype=np.uint64)
        self.sum_e = np.zeros(n, dtype=np.float64)
        self.sum_e2 = np.zeros(n, dtype=np.float64)
        self.round_trips = np.zeros(n, dtype=np.uint64)   # by slot
        self.labels = np.zeros(n, dtype=np.uint8)         # by slot

    def round(self, rnd, perm_before, perm_after, slot_energy):
        n = self.n
        p, q = np.asarray(perm_before, dtype=np.int64), np.asarray(perm_after, dtype=np.int64)
        E = np.asarray(slot_energy, dtype=np.float64)
        assert sorted(p) == sorted(q) == list(range(n))
        # 1. energy sums: numpy rounds the product and each addition on its own
        for i in range(n):
            e = np.float64(E[p[i]])
            self.sum_e[i] = self.sum_e[i] + e
            self.sum_e2[i] = self.sum_e2[i] + e * e
        # 2. pair counts
        for i in range(int(rnd) & 1, n - 1, 2):
            self.attempts[i] += np.uint64(1)
            exchanged = p[i] != q[i]
            assert exchanged == (p[i + 1] != q[i + 1]) and (not exchanged or (q[i], q[i + 1]) == (p[i + 1], p[i]))
            if exchanged:
                self.accepts[i] += np.uint64(1)
        # 3. flow
        if n >= 2:
            s = q[0]
            if self.labels[s] == DOWN:
                self.round_trips[s] += np.uint64(1)
            self.labels[s] = UP
            self.labels[q[n - 1]] = DOWN
            for i in range(n):
                self.n_up[i] += np.uint64(self.labels[q[i]] == UP)
                self.n_down[i] += np.uint64(self.labels[q[i]] == DOWN)
        # 4.
        self.rounds += 1

    def raw(self):
        return {k: getattr(self, k).copy() for k in ARRAYS} | {"rounds": self.rounds}


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def assert_equal(got, want, in_kernel_rounds=None):
    """got: the raw dict of States.pt_statistics() / the dict of get_ladder_statistics() (one copy); want: Statistics.  All ten
    outputs: the round count, in_kernel_rounds where the caller pins it, and the eight arrays, the f64 sums bit for bit."""
    assert int(got["rounds"]) == want.rounds
    if in_kernel_rounds is not None:
        assert int(got["in_kernel_rounds"]) == in_kernel_rounds
    for k in ("attempts", "accepts", "n_up", "n_down", "round_trips"):
        assert got[k].dtype == np.uint64 and np.array_equal(got[k], getattr(want, k)), k
    assert got["labels"].dtype == np.uint8 and np.array_equal(got["labels"], want.labels)
    if "sum_e" in got:
        assert np.array_equal(bits(got["sum_e"]), bits(want.sum_e)) and np.array_equal(bits(got["sum_e2"]), bits(want.sum_e2))
    else:   # the class's dict: the moments derived from the sums by the same two operations
        r = float(want.rounds) if want.rounds else np.nan
        mean = want.sum_e / r
        assert np.array_equal(bits(got["mean_energy"]), bits(mean))
        assert np.array_equal(bits(got["var_energy"]), bits(want.sum_e2 / r - mean ** 2))

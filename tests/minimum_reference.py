"""The minimum-tracking rule of DESIGN.md S16, restated with numpy -- TEST INFRASTRUCTURE, no GPU.

An update at timestep t with energies e[r] sets, for every replica with e[r] < record[r] (strictly; records start at +inf),
record[r] = e[r], timestep[r] = t and keeps the replica's configuration.  Ties therefore keep the EARLIEST update.
"""
import numpy as np


class Records:
    def __init__(self, R, nvars):
        self.energy = np.full(R, np.inf, dtype=np.float64)
        self.timestep = np.zeros(R, dtype=np.uint64)
        self.state = np.zeros((R, nvars), dtype=np.bool_)
        self.improvements = 0
        self.improved = []   # bool[R] per update, in order

    def update(self, t, energies, states):
        e = np.asarray(energies, dtype=np.float64)
        better = e < self.energy
        self.energy[better] = e[better]
        self.timestep[better] = t
        self.state[better] = np.asarray(states, dtype=np.bool_)[better]
        self.improvements += int(better.sum())
        self.improved.append(better.copy())
        return better

    def reset(self):
        """Records back to +inf, timesteps and the count to zero; the kept configurations stay as they are."""
        self.energy[:] = np.inf
        self.timestep[:] = 0
        self.improvements = 0


def records(timesteps, energies, states):
    """timesteps[U], energies[U, R], states[U, R, N] of a run's update points -> Records."""
    energies = np.asarray(energies, dtype=np.float64)
    rec = Records(energies.shape[1], np.asarray(states[0]).shape[1])
    for t, e, s in zip(timesteps, energies, states):
        rec.update(int(t), e, s)
    return rec


def owned_masks(R, bit0, groups):
    """uint32[groups]: the bits of every 32-replica group that the slots [bit0, bit0 + R) occupy."""
    m = np.zeros(groups, dtype=np.uint32)
    for r in range(R):
        m[(r + bit0) // 32] |= np.uint32(1 << ((r + bit0) % 32))
    return m


def improved_masks(better, bit0, groups):
    """uint32[groups]: the group masks of the replicas marked in better[R]."""
    m = np.zeros(groups, dtype=np.uint32)
    for r in np.nonzero(better)[0]:
        m[(r + bit0) // 32] |= np.uint32(1 << ((r + bit0) % 32))
    return m


def merge_words(raw_per_update, improved_per_update, bit0, groups):
    """The word-level rule on a replica-packed container, u32[groups][n_pos] with replica r = bit (r + bit0) % 32 of group
    (r + bit0) / 32: after every update best = (best & ~m) | (state & m), m = the group's mask of improved replicas."""
    best = np.zeros_like(np.asarray(raw_per_update[0], dtype=np.uint32).reshape(groups, -1))
    for raw, better in zip(raw_per_update, improved_per_update):
        raw = np.asarray(raw, dtype=np.uint32).reshape(groups, -1)
        m = improved_masks(better, bit0, groups)
        best = (best & ~m[:, None]) | (raw & m[:, None])
    return best

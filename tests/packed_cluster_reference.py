"""The Swendsen-Wang cluster step of DESIGN.md S11 (replica-packed general-graph path), restated in numpy on site and position
arrays -- TEST INFRASTRUCTURE, no GPU.

Written from the S11 text alone: bonds owned by their smaller position at that end's adjacency slot, one Philox word per
(bond, replica bit), min-position labels, one flip bit per (root position, replica bit), the two statistics.  Positions come from
the CPU oracle's colouring (`oracle.gen_colouring`), Metropolis timesteps (S6) from its engine D (`oracle.pk_run`); Philox and
the bond threshold are those of tests/cluster_reference.py.
"""
import numpy as np

from cluster_reference import bond_threshold, ctr2, philox4x32_10

DOM_BOND = int.from_bytes(b"PKBD", "big")
DOM_FLIP = int.from_bytes(b"PKFL", "big")


class Graph:
    """Positions, owned bonds and padding of an edge list as S4 / S6 / S11 lay them out."""

    def __init__(self, ea, eb, ej, nvars):
        from oracle import oracle as O

        self.ea, self.eb, self.ej = (np.ascontiguousarray(a, dtype=t) for a, t in ((ea, np.uint64), (eb, np.uint64), (ej, np.float64)))
        self.nvars = int(nvars)
        self.n_colours, colours, pos = O.gen_colouring(self.ea, self.eb, self.ej, self.nvars)
        self.pos = pos.astype(np.int64)
        counts = np.bincount(colours, minlength=self.n_colours)
        self.n_pos = int(((counts + 255) // 256 * 256).sum())  # every colour class padded to a multiple of 256
        real = self.ej[self.ea != self.eb]
        self.jabs = float(abs(real[0])) if len(real) else 0.0
        # adjacency slots in edge-list order (self-loops dropped); a bond belongs to its end with the smaller position
        fill = np.zeros(self.nvars, dtype=np.int64)
        owner, other, slot, jpos = [], [], [], []
        for a, b, j in zip(self.ea.astype(np.int64), self.eb.astype(np.int64), self.ej):
            if a == b:
                continue
            ka, kb = fill[a], fill[b]
            fill[a] += 1
            fill[b] += 1
            if self.pos[a] < self.pos[b]:
                owner.append(a), other.append(b), slot.append(ka)
            else:
                owner.append(b), other.append(a), slot.append(kb)
            jpos.append(j > 0.0)
        self.owner, self.other, self.slot = (np.array(x, dtype=np.int64) for x in (owner, other, slot))
        self.jpos = np.array(jpos, dtype=bool)

    def pack(self, spins):
        """One replica's spins (site order) as the bit-packed position words `States.packed()` returns: padding cleared."""
        words = np.zeros(self.n_pos // 32, dtype=np.uint32)
        p = self.pos[np.asarray(spins, dtype=bool)]
        np.bitwise_or.at(words, p >> 5, (np.uint32(1) << (p & 31).astype(np.uint32)))
        return words

    def energy(self, spins):
        s = 2.0 * np.asarray(spins, dtype=np.float64) - 1.0
        return float((self.ej * s[self.ea.astype(np.int64)] * s[self.eb.astype(np.int64)]).sum())


def bond_uniforms(G, seed, t):
    """u[bond, replica bit]: word q of call j of the bond's (owner position, slot), replica bit 4 j + q."""
    k0, k1 = int(seed) & 0xFFFFFFFF, int(seed) >> 32
    p = G.pos[G.owner].astype(np.uint64)[:, None]
    k = G.slot.astype(np.uint64)[:, None]
    j = np.arange(8, dtype=np.uint64)[None, :]
    words = philox4x32_10(int(t) & 0xFFFFFFFF, p, DOM_BOND, ctr2(t, k, j), k0, k1)  # four [bonds, 8] arrays
    return np.stack(words, axis=-1).reshape(len(G.owner), 32)


def labels_from_bonds(n_pos, a, b):
    """Smallest position of every position's cluster; a, b: the end positions of the active bonds.  Min-label hooking on roots
    and pointer jumping, to a fixed point."""
    lab = np.arange(n_pos, dtype=np.int64)
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    while True:
        ra, rb = lab[a], lab[b]  # roots: lab is fully compressed here
        keep = ra != rb
        if not keep.any():
            return lab
        a, b, ra, rb = a[keep], b[keep], ra[keep], rb[keep]
        np.minimum.at(lab, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt


def flip_bits(G, roots, seed, t):
    """roots[32, n]: bit b of word r & 3 of the call of r >> 2, for the root r of row (replica bit) b."""
    k0, k1 = int(seed) & 0xFFFFFFFF, int(seed) >> 32
    words = np.stack(philox4x32_10(int(t) & 0xFFFFFFFF, np.arange(G.n_pos // 4, dtype=np.uint64), DOM_FLIP, ctr2(t, 0, 0), k0, k1))
    w = words[roots & 3, roots >> 2]
    return ((w >> np.arange(32, dtype=np.uint32)[:, None]) & 1).astype(np.uint8)


def sw_step(G, spins, seed, t, thresholds):
    """One S11 cluster step of a group: spins[32, nvars] (uint8, row = replica bit), the group's key, timestep t, one bond
    threshold per replica bit.  Returns (new spins, clusters[32], largest[32])."""
    spins = np.asarray(spins, dtype=np.uint8)
    T = np.array([int(x) for x in thresholds], dtype=np.uint64)
    differ = spins[:, G.owner] != spins[:, G.other]                        # [32, bonds]
    satisfied = np.where(G.jpos[None, :], differ, ~differ)                 # J s s' < 0
    active = satisfied & (bond_uniforms(G, seed, t).T.astype(np.uint64) < T[:, None])
    # the 32 replicas as one disjoint union of graphs: node b n_pos + p
    bit, bond = np.nonzero(active)
    lab = labels_from_bonds(32 * G.n_pos, bit * G.n_pos + G.pos[G.owner[bond]], bit * G.n_pos + G.pos[G.other[bond]])
    roots = lab.reshape(32, G.n_pos)[:, G.pos] - np.arange(32, dtype=np.int64)[:, None] * G.n_pos   # [32, nvars]: real sites only
    clusters, largest = np.zeros(32, dtype=np.int64), np.zeros(32, dtype=np.int64)
    for b in range(32):
        sizes = np.bincount(roots[b], minlength=G.n_pos)
        clusters[b], largest[b] = (sizes > 0).sum(), sizes.max()
    return spins ^ flip_bits(G, roots, seed, t), clusters, largest


def run(G, seeds, timesteps, k, betas=None, beta_replica=None, states=None, t0=0):
    """Timesteps t0 .. t0 + timesteps - 1 of the experiments `seeds` (whole groups are simulated, as in S6) with
    cluster_every = k (0: Metropolis only).  betas: one per timestep, or beta_replica: one per experiment.  states: None (random
    start at t0 = 0) or uint8[32 groups, nvars] from an earlier call.
    Returns (states[32 groups, nvars], energies[R, timesteps], (clusters[R], largest[R]) of the last cluster step or None)."""
    from oracle import oracle as O

    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    R, groups = len(seeds), (len(seeds) + 31) // 32
    if states is None:
        _, states = O.pk_run(G.ea, G.eb, G.ej, G.nvars, seeds, 0, betas=[])
    states = np.array(states, dtype=np.uint8)
    energies = np.zeros((R, timesteps))
    stats = None
    n = 0
    while n < timesteps:
        t = t0 + n
        if k and t % k == k - 1:
            clusters, largest = np.zeros(32 * groups, dtype=np.int64), np.zeros(32 * groups, dtype=np.int64)
            for g in range(groups):
                rows = slice(32 * g, 32 * g + 32)
                if beta_replica is None:
                    thr = [bond_threshold(betas[n], G.jabs)] * 32
                else:  # the unused bits of a last partial group run at the last experiment's beta (S6)
                    thr = [bond_threshold(beta_replica[min(R - 1, 32 * g + b)], G.jabs) for b in range(32)]
                states[rows], clusters[rows], largest[rows] = sw_step(G, states[rows], int(seeds[32 * g]), t, thr)
            stats = (clusters[:R], largest[:R])
            energies[:, n] = [G.energy(states[r]) for r in range(R)]
            n += 1
            continue
        stretch = timesteps - n if not k else min(timesteps - n, k - 1 - t % k)
        _, states, eps = O.pk_run(G.ea, G.eb, G.ej, G.nvars, seeds, stretch, betas=None if betas is None else betas[n:n + stretch],
                                  beta_replica=beta_replica, states=states, t0=t, per_step=True)
        energies[:, n:n + stretch] = eps
        n += stretch
    return states, energies, stats


def triangular_lattice_edges(W, H, J=-1.0):
    """Periodic W x H triangular lattice: site y W + x bonded to its right, lower and lower-right neighbours (degree 6)."""
    ids = np.arange(W * H, dtype=np.uint64).reshape(H, W)
    nb = [np.roll(ids, -1, axis=1), np.roll(ids, -1, axis=0), np.roll(np.roll(ids, -1, axis=0), -1, axis=1)]
    ea = np.stack([ids] * 3, axis=-1).reshape(-1)
    eb = np.stack(nb, axis=-1).reshape(-1)
    return np.ascontiguousarray(ea), np.ascontiguousarray(eb), np.full(ea.shape, float(J))


# The seeded sampling check on the periodic 4 x 4 triangular ferromagnet (tests/test_packed_cluster_host.py with this module
# alone, tests/test_gpu_packed_cluster.py on the device with the same numbers): beta = 0.2 sits a little below the bulk
# critical coupling ln(3)/4 = 0.2747, where the 16-site energy still fluctuates widely; cluster steps decorrelate it in a few
# steps, so 50 timesteps from the random start thermalise and 400 give > 50 independent values per chain, with k = 2 as with
# k = 1; 64 chains (two groups) give the standard error from the spread ACROSS independent chains.
TRI_BETA = 0.2
TRI_CHAINS = 64
TRI_THERM = 50
TRI_STEPS = 400
TRI_SEED = 0x7A1C0000
# Cubic 8^3 at beta = 0.2216 (the bulk critical coupling), cluster chains against Metropolis-only chains on the device: 64 chains
# each, 200 timesteps to thermalise from the random start, 1000 measured.  Chosen with this module alone on 32 chains each: the
# integrated autocorrelation time of E is 3.2 timesteps with a cluster step at every timestep and 5.5 with Metropolis sweeps only
# (8^3 is small), so 200 timesteps thermalise either chain and 1000 give > 90 independent values; <E> = -568.8 +- 2.0 against
# -565.6 +- 2.7, z = -0.98.
CUBIC_BETA = 0.2216
CUBIC_CHAINS = 64
CUBIC_THERM = 200
CUBIC_STEPS = 1000

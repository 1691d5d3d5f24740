"""The row of a cluster series, restated in numpy -- TEST INFRASTRUCTURE, no GPU.

Written from the S24 text alone: per column the six numbers n_clusters, largest, sites = sum s, S2 = sum s^2, S4 = sum s^4 as two
64-bit words, over the sizes s of the clusters the step built for that column.  The clusters themselves are those of S8 / S9 /
S11 / S12: bond uniforms, labelling and flip bits come from tests/cluster_reference.py, tests/packed_cluster_reference.py,
tests/icm_reference.py and tests/packed_icm_reference.py; what those modules compute inside their steps without handing it out --
the cluster sizes -- is restated here from the same pieces.  All sums are Python integers: exact at any size.
"""
import numpy as np

import cluster_reference as CR
import packed_cluster_reference as PR

M64 = (1 << 64) - 1
COLUMNS = ("n_clusters", "largest", "sites", "s2", "s4_lo", "s4_hi")


def split128(x):
    """(low, high) 64-bit words of 0 <= x < 2^128."""
    x = int(x)
    assert 0 <= x < 1 << 128
    return x & M64, x >> 64


def join128(lo, hi):
    return (int(hi) << 64) | int(lo)


def row_of_sizes(sizes):
    """The six numbers of one column from its cluster sizes (any iterable of integers; zeros are no clusters)."""
    s = [int(x) for x in np.asarray(sizes).ravel() if int(x) > 0]
    lo, hi = split128(sum(x ** 4 for x in s))
    return (len(s), max(s, default=0), sum(s), sum(x * x for x in s), lo, hi)


# ---- Swendsen-Wang step on the checkerboard lattice (S8) ----------------------------------------------------------------------
def sw_labels(spins, seed, t, beta, J):
    """Cluster label of every site of spins[H, W] for the step at timestep t: the bonds CR.sw_step activates, labelled."""
    H, W = spins.shape
    T = CR.bond_threshold(beta, J)
    u = CR.bond_uniforms(W, H, seed, t) if 0 < T < 2 ** 32 else [np.zeros((H, W), dtype=np.uint32)] * 2
    act = []
    for d, axis in ((0, 1), (1, 0)):
        equal = spins == np.roll(spins, -1, axis=axis)
        satisfied = equal if J < 0 else ~equal  # J s s' < 0
        act.append(satisfied & (u[d].astype(np.uint64) < np.uint64(T)))
    return CR.labels_from_bonds(act[0], act[1])


def sw_row(spins, seed, t, beta, J):
    """(spins after the step, row) of one replica: spins uint8[H, W] before the step at timestep t."""
    spins = np.ascontiguousarray(spins, dtype=np.uint8)
    labels = sw_labels(spins, seed, t, beta, J)
    row = row_of_sizes(np.bincount(labels.ravel()))
    return spins ^ CR.flip_bits(labels, seed, t), row


# ---- isoenergetic cluster move on the checkerboard lattice (S9) -----------------------------------------------------------------
def icm_row(a, b):
    """Row of the pair (a, b) (uint8[H, W] before the move): the clusters of the q = a XOR b = 1 sites.  No random number enters."""
    q = (np.asarray(a, dtype=np.uint8) ^ np.asarray(b, dtype=np.uint8)).astype(bool)
    labels = CR.labels_from_bonds(q & np.roll(q, -1, axis=1), q & np.roll(q, -1, axis=0))
    return row_of_sizes(np.bincount(labels[q], minlength=1))  # q = +1 sites are singleton labels that do not count


# ---- Swendsen-Wang step on the replica-packed path (S11) ----------------------------------------------------------------------
def pk_sw_step(G, spins, seed, t, thresholds):
    """PR.sw_step with the sizes handed out: spins uint8[32, nvars] of a group, its key, one threshold per replica bit.
    Returns (new spins, rows[32])."""
    spins = np.asarray(spins, dtype=np.uint8)
    T = np.array([int(x) for x in thresholds], dtype=np.uint64)
    differ = spins[:, G.owner] != spins[:, G.other]
    satisfied = np.where(G.jpos[None, :], differ, ~differ)
    active = satisfied & (PR.bond_uniforms(G, seed, t).T.astype(np.uint64) < T[:, None])
    bit, bond = np.nonzero(active)
    lab = PR.labels_from_bonds(32 * G.n_pos, bit * G.n_pos + G.pos[G.owner[bond]], bit * G.n_pos + G.pos[G.other[bond]])
    roots = lab.reshape(32, G.n_pos)[:, G.pos] - np.arange(32, dtype=np.int64)[:, None] * G.n_pos  # real sites only
    rows = [row_of_sizes(np.bincount(roots[b])) for b in range(32)]
    return spins ^ PR.flip_bits(G, roots, seed, t), rows


def pk_sw_row(G, spins, bit, seed, t, threshold):
    """Row of ONE replica of a group: its spins uint8[nvars] before the step, its replica bit, the group's key."""
    spins = np.asarray(spins, dtype=bool)
    differ = spins[G.owner] != spins[G.other]
    satisfied = np.where(G.jpos, differ, ~differ)
    active = satisfied & (PR.bond_uniforms(G, seed, t)[:, bit].astype(np.uint64) < np.uint64(int(threshold)))
    lab = PR.labels_from_bonds(G.n_pos, G.pos[G.owner[active]], G.pos[G.other[active]])
    return row_of_sizes(np.bincount(lab[G.pos]))


# ---- isoenergetic cluster move on the replica-packed paths (S12) ------------------------------------------------------------------
def pk_icm_row(G, a, b):
    """Row of the pair (a, b) (uint8[nvars] before the move): the components of the sites where they differ, along every edge of
    the list that is no self-loop."""
    d = np.asarray(a, dtype=bool) != np.asarray(b, dtype=bool)
    act = d[G.owner] & d[G.other]
    lab = PR.labels_from_bonds(G.n_pos, G.pos[G.owner[act]], G.pos[G.other[act]])
    return row_of_sizes(np.bincount(lab[G.pos[np.nonzero(d)[0]]], minlength=1))


def rows_array(rows):
    """rows[column] (tuples of six integers) -> uint64[columns, 6], as ClusterSeries.get returns one row stacked on the last axis."""
    return np.array([[int(v) for v in r] for r in rows], dtype=np.uint64).reshape(len(rows), 6)

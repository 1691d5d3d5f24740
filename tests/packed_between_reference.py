"""The isoenergetic cluster move between two replica-packed containers of DESIGN.md S13, restated in numpy on site and position
arrays -- TEST INFRASTRUCTURE, no GPU.

Written from the S13 text alone: pair n is slot slots_a[n] of container a and slot slots_b[n] of container b; d = 1 on the real
sites where the two differ; the clusters are the components of the d = 1 positions along every stored adjacency entry (every
edge of the list that is no self-loop, whatever its J); min-position labels; root position r flips iff bit r & 31 of word
(r >> 5) & 3 of P(key of a's GLOBAL group, (t_lo, r >> 7, "PKBF", ctr2(t, global bit of a's slot, 0))) is set; a flipped cluster
swaps the two replicas' spins on it; three statistics per pair.  Nothing else moves.

Graph, labels_from_bonds and Philox are those of tests/packed_cluster_reference.py / tests/cluster_reference.py; positions come
from the CPU oracle's colouring for both families (as in tests/packed_icm_reference.py).
"""
import numpy as np

from cluster_reference import ctr2, philox4x32_10
from packed_cluster_reference import Graph, labels_from_bonds, triangular_lattice_edges  # noqa: F401  (re-exported)

DOM_FLIP = int.from_bytes(b"PKBF", "big")   # 0x504B4246


def flip_bits(n_pos, seed, t, bit):
    """uint8[n_pos]: the flip bit of every possible root position for the pair whose a-side replica is global bit `bit` of the
    group keyed by `seed`."""
    k0, k1 = int(seed) & 0xFFFFFFFF, int(seed) >> 32
    calls = np.arange((n_pos + 127) // 128, dtype=np.uint64)
    words = np.stack(philox4x32_10(int(t) & 0xFFFFFFFF, calls, DOM_FLIP, ctr2(t, int(bit), 0), k0, k1), axis=-1).astype(np.uint32)   # [call, word]
    r = np.arange(n_pos)
    return ((words[r >> 7, (r >> 5) & 3] >> (r & 31).astype(np.uint32)) & 1).astype(np.uint8)


def slot_key(all_seeds, first, slot):
    """(seed of the GLOBAL group, global bit) of local slot `slot` of a container that is the shard starting at `first`."""
    n = int(first) + int(slot)
    return int(all_seeds[32 * (n // 32)]), n % 32


def cluster_labels(G, d):
    """Smallest position of every position's cluster for the overlap d[nvars] (bool)."""
    act = d[G.owner] & d[G.other]
    return labels_from_bonds(G.n_pos, G.pos[G.owner][act], G.pos[G.other][act])


def move_pair(G, sa, sb, seed, bit, t):
    """One pair: sa, sb uint8[nvars].  Returns (new sa, new sb, (clusters, largest, d = 1 positions))."""
    sa, sb = np.array(sa, dtype=np.uint8), np.array(sb, dtype=np.uint8)
    d = sa != sb
    sites = np.nonzero(d)[0]
    if not len(sites):
        return sa, sb, (0, 0, 0)
    roots = cluster_labels(G, d)[G.pos[sites]]
    sizes = np.bincount(roots, minlength=G.n_pos)
    f = flip_bits(G.n_pos, seed, t, bit)[roots]
    sa[sites] ^= f
    sb[sites] ^= f
    return sa, sb, (int((sizes > 0).sum()), int(sizes.max()), len(sites))


def move(G, A, B, slots_a, slots_b, seeds_a, first_a, t):
    """The whole call: A[R_a, nvars], B[R_b, nvars] by LOCAL slot; seeds_a: the seeds of ALL experiments of a's set, first_a: the
    global index of a's slot 0.  Returns (new A, new B, [(clusters, largest, minus)] per pair)."""
    A, B = np.array(A, dtype=np.uint8), np.array(B, dtype=np.uint8)
    stats = []
    for sa, sb in zip(slots_a, slots_b):
        seed, bit = slot_key(seeds_a, first_a, sa)
        A[sa], B[sb], st = move_pair(G, A[sa], B[sb], seed, bit, t)
        stats.append(st)
    return A, B, stats


# The seeded sampling check (tests/test_packed_between_host.py): ClassicalTempering(copies=2) on the oracle-backed engine of
# tests/packed_ladder_icm_engine.py, the periodic 4 x 4 triangular lattice with the seeded +-J signs of
# tests/packed_icm_reference.py (tri_glass), 8 rungs, a move every 2nd timestep, a round every 2nd; LADDER_THERM timesteps
# discarded, then LADDER_BATCHES batches of LADDER_BATCH timesteps whose mean energies per rung and copy are the samples; <E>
# against exact enumeration, standard error from the batch means.
LADDER_BETAS = tuple(float(b) for b in np.linspace(0.2, 0.9, 8))
LADDER_SEED = 12345
LADDER_K = 2
LADDER_ROUND_EVERY = 2
LADDER_THERM = 200
LADDER_BATCHES = 20
LADDER_BATCH = 100
# Observed with this module and the engine alone (tests/test_packed_between_host.py re-runs it and pins the figure): z per rung
#   copy 0: -1.57 -2.33 -1.20 +0.88 +0.24 +1.12 -0.44 +1.04      copy 1: -0.52 -0.64 -1.05 -0.32 +0.87 -0.23 -0.29 -0.83
# and with 160 batches instead of 20 (same seed) every |z| <= 1.23: the two low rungs of copy 0 are fluctuations, not a bias.
LADDER_MAX_ABS_Z = 2.33

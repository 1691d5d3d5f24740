"""The isoenergetic cluster move of DESIGN.md S9, restated in numpy on site-id arrays -- TEST INFRASTRUCTURE, no GPU.

Written from the S9 text alone: q = a XOR b, a bond is active iff both ends have q = -1, clusters labelled by their smallest site
id, one flip bit per possible root from Philox4x32-10 with the "ICFL" counters and the key of the pair's first replica, flips
applied to both replicas.  Philox, ctr2 and the min-label hooking come from tests/cluster_reference.py; Metropolis timesteps (S3),
packing and unpacking (S2) from the CPU oracle (`oracle.Lat`), which takes +-J sign arrays.
"""
import numpy as np

from cluster_reference import ctr2, labels_from_bonds, philox4x32_10

DOM_ICM_FLIP = int.from_bytes(b"ICFL", "big")


def icm_step(a, b, seed, t):
    """One S9 move of the pair (a, b) (uint8[H, W], 1 = up) at timestep t; seed: the seed of replica a.
    Returns (new a, new b, (number of q = -1 clusters, largest one, number of q = -1 sites))."""
    q = (a ^ b).astype(bool)
    act_right = q & np.roll(q, -1, axis=1)
    act_down = q & np.roll(q, -1, axis=0)
    labels = labels_from_bonds(act_right, act_down)
    n_calls = (q.size + 127) // 128
    k0, k1 = int(seed) & 0xFFFFFFFF, int(seed) >> 32
    words = np.stack(philox4x32_10(int(t) & 0xFFFFFFFF, np.arange(n_calls, dtype=np.uint64), DOM_ICM_FLIP, ctr2(t, 0, 0), k0, k1))
    r = labels.astype(np.int64)
    flip = (((words[(r >> 5) & 3, r >> 7] >> (r & 31).astype(np.uint32)) & 1).astype(bool) & q).astype(np.uint8)
    sizes = np.bincount(labels[q], minlength=1)  # q = +1 sites are singleton labels that do not count
    return a ^ flip, b ^ flip, (int((sizes > 0).sum()), int(sizes.max()), int(q.sum()))


def couplings(W, H, ej):
    """(jright, jdown) as float[H, W] from the edge couplings in the order of exact.square_lattice_edges."""
    ej = np.asarray(ej, dtype=np.float64)
    return ej[0::2].reshape(H, W), ej[1::2].reshape(H, W)


def energy(spins, jr, jd):
    s = 2 * spins.astype(np.int64) - 1
    return float((jr * (s * np.roll(s, -1, axis=1))).sum() + (jd * (s * np.roll(s, -1, axis=0))).sum())


def make_lat(W, H, jr, jd):
    from oracle import oracle as O

    jabs = float(abs(jr[0, 0]))
    if (jr > 0).all() and (jd > 0).all():
        return O.Lat(W, H, jabs, 1)
    if (jr < 0).all() and (jd < 0).all():
        return O.Lat(W, H, jabs, 0)
    return O.Lat(W, H, jabs, 0, (jr > 0).astype(np.uint8).ravel(), (jd > 0).astype(np.uint8).ravel())


def run_replicas(W, H, jr, jd, seeds, spins, t0, betas, k, first=0):
    """Timesteps t0 .. t0 + T - 1 of the replicas with global indices first, first + 1, ... (first even) with icm_every = k
    (0: Metropolis only).  betas: [T] (every replica) or [R][T].  Replicas (2p, 2p + 1) form a pair; a last one without a partner
    stays as it is on an ICM timestep.  Returns (spins [R][H, W], energies [R, T], stats of the last ICM step per pair or None)."""
    assert first % 2 == 0
    lat = make_lat(W, H, jr, jd)
    R = len(seeds)
    spins = [np.ascontiguousarray(s, dtype=np.uint8).reshape(H, W) for s in spins]
    betas = np.asarray(betas, dtype=np.float64)
    T = betas.shape[-1]
    energies, stats = np.zeros((R, T)), None
    for n in range(T):
        t = t0 + n
        if k and t % k == k - 1:
            stats = []
            for p in range(R // 2):
                spins[2 * p], spins[2 * p + 1], st = icm_step(spins[2 * p], spins[2 * p + 1], seeds[2 * p], t)
                stats.append(st)
        else:
            for r in range(R):
                st = lat.pack(spins[r].ravel())
                lat.sweep(st, seeds[r], t, betas[n] if betas.ndim == 1 else betas[r, n])
                spins[r] = lat.unpack(st).reshape(H, W)
        for r in range(R):
            energies[r, n] = energy(spins[r], jr, jd)
    return spins, energies, stats


def run_pair(W, H, jr, jd, seeds, a, b, t0, betas, k):
    """One pair: ((a, b), energies [2, T], stats of the last ICM step or None)."""
    spins, energies, stats = run_replicas(W, H, jr, jd, list(seeds), [a, b], t0, betas, k)
    return (spins[0], spins[1]), energies, None if stats is None else stats[0]


# Lengths of the seeded sampling checks (tests/test_icm_host.py): 16 pairs, icm_every = 2, 50 timesteps discarded, 200 used; the
# Metropolis-only chain they are compared with on the +-J sample: 100 discarded, 400 used.  The pair means are the samples.
SAMPLING_PAIRS = 16
SAMPLING_THERM, SAMPLING_STEPS = 50, 200
METROPOLIS_THERM, METROPOLIS_STEPS = 100, 400

"""The Swendsen-Wang cluster step of DESIGN.md S8, restated in numpy on site-id arrays -- TEST INFRASTRUCTURE, no GPU.

Written from the S8 text alone: the S2 index formulas for (plane, word, bit), Philox4x32-10 with the counters of S8,
`math.expm1` for the bond threshold, min-label hooking with pointer jumping run to a fixed point, flip bits and stats.
Metropolis timesteps (S3) come from the CPU oracle (`oracle.Lat.sweep`), as do packing and unpacking (S2).
"""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
DOM_BOND = int.from_bytes(b"SWBD", "big")
DOM_FLIP = int.from_bytes(b"SWFL", "big")


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10: counter words and key words broadcast against each other; four uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3)])
    k0, k1 = int(k0), int(k1)
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [c.astype(np.uint32) for c in (c0, c1, c2, c3)]


def ctr2(t, colour, call):
    return (((int(t) >> 32) & 0xFFFF) << 16) | (np.asarray(colour, dtype=np.uint64) << np.uint64(8)) | np.asarray(call, dtype=np.uint64)


def bond_threshold(beta, J):
    """T = floor((1 - exp(-2 beta |J|)) 2^32) in f64; 2^32 = always active, beta <= 0 = never."""
    if not beta > 0.0:
        return 0
    return int(math.floor(-math.expm1(-2.0 * beta * abs(J)) * 2.0 ** 32))


def site_layout(W, H):
    """(c, w, b) of every site (x, y) in the S2 layout: plane, word of the plane, bit; arrays [H, W]."""
    y, x = np.meshgrid(np.arange(H, dtype=np.uint64), np.arange(W, dtype=np.uint64), indexing="ij")
    c = (x + y) & np.uint64(1)
    i = x >> np.uint64(1)  # x = 2 i + ((y + c) & 1)
    w = y * np.uint64(W // 64) + (i >> np.uint64(5))
    return c, w, i & np.uint64(31)


def bond_uniforms(W, H, seed, t):
    """u[d][y, x]: the 32-bit uniform of the bond site (x, y) owns in direction d (0 right, 1 down)."""
    c, w, b = site_layout(W, H)
    wpp = H * (W // 64)
    k0, k1 = int(seed) & 0xFFFFFFFF, int(seed) >> 32
    out = []
    cc, ww, jj = np.meshgrid(np.arange(2, dtype=np.uint64), np.arange(wpp, dtype=np.uint64), np.arange(8, dtype=np.uint64), indexing="ij")
    for d in (0, 1):  # one call per (plane, word, quarter-byte of bits): [4][2, wpp, 8]
        words = np.stack(philox4x32_10(int(t) & 0xFFFFFFFF, ww, DOM_BOND, ctr2(t, cc, np.uint64(8 * d) + jj), k0, k1))
        out.append(words[(b & np.uint64(3)).astype(np.intp), c.astype(np.intp), w.astype(np.intp), (b >> np.uint64(2)).astype(np.intp)])
    return out


def labels_from_bonds(act_right, act_down):
    """Cluster label (smallest site id y W + x of the cluster) of every site; act_*[y, x]: the bond from (x, y) to its right /
    lower neighbour (periodic) is active.  Min-label hooking on roots + pointer jumping, to a fixed point."""
    H, W = act_right.shape
    ids = np.arange(H * W, dtype=np.int64).reshape(H, W)
    a = np.concatenate([ids[act_right], ids[act_down]])
    b = np.concatenate([np.roll(ids, -1, axis=1)[act_right], np.roll(ids, -1, axis=0)[act_down]])
    lab = np.arange(H * W, dtype=np.int64)
    while True:
        ra, rb = lab[a], lab[b]  # roots: lab is fully compressed here
        keep = ra != rb
        if not keep.any():
            break
        a, b, ra, rb = a[keep], b[keep], ra[keep], rb[keep]
        np.minimum.at(lab, np.maximum(ra, rb), np.minimum(ra, rb))  # a root hangs below the smallest root it meets
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
    return lab.reshape(H, W)


def flip_bits(labels, seed, t):
    """Flip decision of every site's cluster (bit r & 31 of word (r >> 5) & 3 of the call of r >> 7)."""
    n_calls = (labels.size + 127) // 128
    k0, k1 = int(seed) & 0xFFFFFFFF, int(seed) >> 32
    words = np.stack(philox4x32_10(int(t) & 0xFFFFFFFF, np.arange(n_calls, dtype=np.uint64), DOM_FLIP, ctr2(t, 0, 0), k0, k1))
    r = labels.astype(np.int64)
    return ((words[(r >> 5) & 3, r >> 7] >> (r & 31).astype(np.uint32)) & 1).astype(np.uint8)


def sw_step(spins, seed, t, beta, J):
    """One S8 cluster step of spins[H, W] (uint8, 1 = up) at timestep t: (new spins, number of clusters, largest cluster)."""
    H, W = spins.shape
    T = bond_threshold(beta, J)
    u = bond_uniforms(W, H, seed, t) if 0 < T < 2 ** 32 else [np.zeros((H, W), dtype=np.uint32)] * 2
    act = []
    for d, axis in ((0, 1), (1, 0)):
        equal = spins == np.roll(spins, -1, axis=axis)
        satisfied = equal if J < 0 else ~equal  # J s s' < 0
        act.append(satisfied & (u[d].astype(np.uint64) < np.uint64(T)))
    labels = labels_from_bonds(act[0], act[1])
    sizes = np.bincount(labels.ravel(), minlength=H * W)
    return spins ^ flip_bits(labels, seed, t), int((sizes > 0).sum()), int(sizes.max())


def energy(spins, J):
    s = 2 * spins.astype(np.int64) - 1
    return float(J) * float((s * np.roll(s, -1, axis=1)).sum() + (s * np.roll(s, -1, axis=0)).sum())


def run(W, H, J, seed, spins, t0, betas, k):
    """Timesteps t0 .. t0 + len(betas) - 1 of one replica with cluster_every = k (0: Metropolis only): the Metropolis sweeps from
    the CPU oracle.  Returns (spins[H, W], energy after every timestep, stats of the last cluster step or None)."""
    from oracle import oracle as O

    lat = O.Lat(W, H, abs(float(J)), 1 if J > 0 else 0)
    spins = np.ascontiguousarray(spins, dtype=np.uint8).reshape(H, W)
    energies, stats = [], None
    for n, beta in enumerate(betas):
        t = t0 + n
        if k and t % k == k - 1:
            spins, n_clusters, largest = sw_step(spins, seed, t, beta, J)
            stats = (n_clusters, largest)
        else:
            st = lat.pack(spins.ravel())
            lat.sweep(st, seed, t, beta)
            spins = lat.unpack(st).reshape(H, W)
        energies.append(energy(spins, J))
    return spins, np.array(energies), stats


# Lengths of the seeded sampling checks (tests/test_cluster_host.py on 64 x 4, tests/test_gpu_cluster.py on 256^2 with the same
# numbers): cluster steps decorrelate the energy in O(10) steps, so 50 steps from the all-up start thermalise and 200 steps give
# ~20 independent values per chain; the standard error comes from the spread ACROSS the independent chains.
SAMPLING_THERM = 50
SAMPLING_STEPS = 200

"""The isoenergetic cluster move of DESIGN.md S12 (replica-packed general-graph paths, both families), restated in numpy on site
and position arrays -- TEST INFRASTRUCTURE, no GPU.

Written from the S12 text alone: experiments (2 j, 2 j + 1) of a replica group form pair j; d = 1 where the two differ (real
sites, moving pairs); the clusters are the components of the d = 1 sites along every stored adjacency entry (every edge of the
list that is no self-loop, whatever its J); min-position labels; one flip bit per (root position, pair) -- bit j of half r & 1 of
word (r & 7) >> 1 of Philox call r >> 3; a flipped cluster swaps the two replicas' spins on it; three statistics per pair.

Positions come from the CPU oracle's colouring (`oracle.gen_colouring`) for BOTH families: the real-coupling family lays its
positions out by the same colouring of the same adjacency (zero couplings included), which the oracle's engine E uses too.
Metropolis timesteps come from the oracle's engine D (`oracle.pk_run`, one |J|) or E (`oracle.rj_run`, real couplings and
biases); Graph, labels_from_bonds and Philox are those of tests/packed_cluster_reference.py.
"""
import numpy as np

from cluster_reference import ctr2, philox4x32_10
from packed_cluster_reference import Graph, labels_from_bonds, triangular_lattice_edges  # noqa: F401  (re-exported)

DOM_FLIP = int.from_bytes(b"PKIF", "big")


def flip_words(n_pos, seed, t):
    """The flip table of a group: uint32[n_pos // 8, 4], row i = Philox call i."""
    k0, k1 = int(seed) & 0xFFFFFFFF, int(seed) >> 32
    words = philox4x32_10(int(t) & 0xFFFFFFFF, np.arange(n_pos // 8, dtype=np.uint64), DOM_FLIP, ctr2(t, 0, 0), k0, k1)
    return np.stack(words, axis=-1).astype(np.uint32)


def flip_bit(words, root, pair):
    """Flip bit of pair `pair` for root position(s) `root`."""
    root = np.asarray(root, dtype=np.int64)
    w = words[root >> 3, (root & 7) >> 1].astype(np.uint64)
    return ((w >> (16 * (root & 1) + pair).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)


def icm_step(G, spins, seed, t, moving):
    """One S12 move of a group: spins[32, nvars] (uint8, row = replica bit), the group's key, timestep t, moving[16] (bool: pair j
    moves).  Returns (new spins, clusters[16], largest[16], minus[16])."""
    spins = np.array(spins, dtype=np.uint8)
    words = flip_words(G.n_pos, seed, t)
    clusters, largest, minus = (np.zeros(16, dtype=np.int64) for _ in range(3))
    a_pos, b_pos = G.pos[G.owner], G.pos[G.other]
    for j in range(16):
        if not moving[j]:
            continue
        d = spins[2 * j] != spins[2 * j + 1]                         # [nvars]
        act = d[G.owner] & d[G.other]
        lab = labels_from_bonds(G.n_pos, a_pos[act], b_pos[act])
        sites = np.nonzero(d)[0]
        roots = lab[G.pos[sites]]
        minus[j] = len(sites)
        if len(sites):
            sizes = np.bincount(roots, minlength=G.n_pos)
            clusters[j], largest[j] = (sizes > 0).sum(), sizes.max()
            f = flip_bit(words, roots, j)
            spins[2 * j, sites] ^= f
            spins[2 * j + 1, sites] ^= f
    return spins, clusters, largest, minus


def run(G, seeds, timesteps, k, betas=None, beta_replica=None, states=None, t0=0, biases=None, real=False, n_total=None):
    """Timesteps t0 .. t0 + timesteps - 1 of the experiments `seeds` (whole groups are simulated) with icm_every = k (0: Metropolis
    only).  real: the real-coupling family (engine E, `biases`) instead of the bit-sliced one (engine D).
    Returns (states[32 groups, nvars], energies[R, timesteps], (clusters, largest, minus)[R // 2] of the last move or None)."""
    from oracle import oracle as O

    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    R, groups = len(seeds), (len(seeds) + 31) // 32
    n_total = R if n_total is None else n_total

    def metropolis(n_steps, t, st, b):
        if real:
            return O.rj_run(G.ea, G.eb, G.ej, G.nvars, seeds, n_steps, betas=b, beta_replica=beta_replica, biases=biases, states=st, t0=t,
                            per_step=True)
        return O.pk_run(G.ea, G.eb, G.ej, G.nvars, seeds, n_steps, betas=b, beta_replica=beta_replica, states=st, t0=t, per_step=True)

    def energy(spins):
        return O.rj_energy(G.ea, G.eb, G.ej, G.nvars, spins, biases) if real else G.energy(spins)

    if states is None:
        _, states, _ = metropolis(0, 0, None, [])
    states = np.array(states, dtype=np.uint8)
    energies = np.zeros((R, timesteps))
    stats = None
    n = 0
    while n < timesteps:
        t = t0 + n
        if k and t % k == k - 1:
            out = [np.zeros(16 * groups, dtype=np.int64) for _ in range(3)]
            for g in range(groups):
                rows = slice(32 * g, 32 * g + 32)
                moving = [32 * g + 2 * j + 1 < n_total for j in range(16)]
                states[rows], c, l, m = icm_step(G, states[rows], int(seeds[32 * g]), t, moving)
                for o, v in zip(out, (c, l, m)):
                    o[16 * g:16 * g + 16] = v
            stats = tuple(o[:R // 2] for o in out)
            energies[:, n] = [energy(states[r]) for r in range(R)]
            n += 1
            continue
        stretch = timesteps - n if not k else min(timesteps - n, k - 1 - t % k)
        _, states, eps = metropolis(stretch, t, states, None if betas is None else betas[n:n + stretch])
        energies[:, n:n + stretch] = eps
        n += stretch
    return states, energies, stats


def integrated_autocorrelation_time(series):
    """tau_int of the rows of series[chains, steps] (mean over chains of the autocorrelation, summed to the first negative value)."""
    x = series - series.mean(axis=1, keepdims=True)
    var = (x * x).mean()
    tau = 0.5
    for lag in range(1, series.shape[1] // 4):
        rho = (x[:, :-lag] * x[:, lag:]).mean() / var
        if rho <= 0:
            break
        tau += rho
    return tau


# The seeded sampling checks (tests/test_packed_icm_host.py with this module alone; tests/test_gpu_packed_icm.py on the device
# with the same numbers).
# (a) The periodic 4 x 4 triangular lattice with a seeded +-J sign pattern (frustrated: odd cycles with both signs), k = 2
# against exact enumeration.  beta = 0.5; 64 chains (32 pairs, two groups), TRI_THERM timesteps from the random start, then
# TRI_STEPS measured.
TRI_BETA = 0.5
TRI_CHAINS = 64
TRI_THERM = 100
TRI_STEPS = 400
TRI_SEED = 0x1C3A0000
TRI_SIGN_SEED = 12
# (b) Cubic 6^3 +-J (seeded signs) at beta = 0.5 (well inside the paramagnet: T_c of the 3-d +-J glass is near beta = 0.9, so
# Metropolis sweeps alone equilibrate in tens of timesteps): 64 chains with k = 2 against 64 Metropolis-only chains, other seeds.
CUBIC_BETA = 0.5
CUBIC_CHAINS = 64
CUBIC_THERM = 100
CUBIC_STEPS = 300
CUBIC_SIGN_SEED = 7
CUBIC_SEEDS = (0x1C3B0000, 0x1C3B0001)

# Observed with this module alone (tests/test_packed_icm_host.py re-runs both and pins the figures):
#   (a) 4 x 4 triangular +-J, beta = 0.5, k = 2: tau_int(E) = 1.4 timesteps, so 100 timesteps thermalise and 400 give > 100
#       independent values per chain; <E> = -25.0253 against -25.0633 from exact enumeration, z = +0.62
#   (b) cubic 6^3 +-J, beta = 0.5: tau_int(E) = 2.1 timesteps with k = 2 and 1.5 with Metropolis sweeps alone (every second
#       timestep of the k = 2 chain has no sweep), so 100 timesteps thermalise and 300 give > 70 independent values;
#       <E> = -289.12 +- 0.28 against -289.29 +- 0.25, z = +0.44
# tests/test_gpu_packed_icm.py runs the same chains on the device; bit-exactness makes them the same numbers.
TRI_TAU, TRI_Z = 1.4, 0.62
CUBIC_TAU, CUBIC_TAU_METROPOLIS, CUBIC_Z = 2.1, 1.5, 0.44


def tri_glass():
    ea, eb, _ = triangular_lattice_edges(4, 4)
    ej = np.random.default_rng(TRI_SIGN_SEED).choice([-1.0, 1.0], len(ea))
    return ea, eb, ej


def cubic_glass(exact, L=6):
    ea, eb, _ = exact.cubic_lattice_edges(L, -1.0)
    ej = np.random.default_rng(CUBIC_SIGN_SEED).choice([-1.0, 1.0], len(ea))
    return ea, eb, ej

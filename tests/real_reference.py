"""Exact host reference and graph builders for the replica-packed real-coupling family (tests/test_real_reference_host.py,
tests/test_gpu_real_variants.py).

exact_energy: E = sum_e J_e s_a s_b - sum_i h_i s_i over the edge list as given (a self-loop counts J, a bond given twice counts
twice), from the ORIGINAL f64 couplings and biases in exact rational arithmetic.

energy_bound: how far an energy of this family may lie from that, derived from how the path forms it (pk_energy in
isingmc.hip, rj_energy_from_counts_kernel, rj_energy in the oracle).  With F_i = |h_i| + sum of |J_e| over the bonds at site i and
kE = floor(log2 max_i F_i) + 2 - 30, every bond coupling and every bias x is carried as two integers
    hi = rint(x 2^-kE),   lo = rint((x - hi 2^kE) 2^(24 - kE)).
x - hi 2^kE is exact in f64 (both are multiples of ulp(x) and the difference is no larger than x), its size is at most 2^(kE - 1),
so |lo| <= 2^23 fits and the rounding of lo (to nearest: not a truncation) leaves
    |x - (hi 2^kE + lo 2^(kE - 24))| <= 2^(kE - 25) = q                                       per term, N terms.
The level sums S_hi, S_lo over the configuration are exact integers (|S_hi| < N 2^29, |S_lo| <= N 2^23: exact as f64 for the
N < 2^24 of any graph here), both ldexp are exact, and the value returned is fl(fl(2^kE S_hi + 2^(kE - 24) S_lo) + self) with
self the f64 running sum of the n_s self-loop couplings.  Each fl is one rounding, relative error at most u = 2^-53: the bond and
bias part A = sum_k +-(x_k + d_k), |d_k| <= q, |A| <= S + N q with S = sum_k |x_k|, passes through two of them, the self-loop
part (sum of sizes S_s) through n_s (n_s - 1 inside the running sum, one at the end).  So
    |E - E_exact| <= N q + ((1 + u)^2 - 1) (S + N q) + gamma(n_s) S_s,   gamma(m) = m u / (1 - m u).
tests/test_gpu_real_k1.py asserts N q + 4 eps S = N q + 8 u S: the same first term and a rounding term four times the one derived
here; that form is an upper bound of this one (without self-loops) and stays valid, this module uses the derived one.  N counts
every bond of the edge list that is no self-loop, and every site when biases are given (a zero term has no error; counting it
keeps the bound an upper bound).  Nothing here is taken from what a kernel returns.

The builders use fixed numpy seeds; what each is named for (eligibility, heavy sites and their shifts, maximum degree and slot
count, colour count and class sizes) is asserted on the host by tests/test_real_reference_host.py.
"""
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

Graph = namedtuple("Graph", "name ea eb ej nvars biases scale")

U = Fraction(1, 2 ** 53)
LO_BITS = 24
SLOT_COUNTS = (4, 7, 11, 15, 23, 31)
THREADS = {4: 256, 7: 256, 11: 128, 15: 128, 23: 64, 31: 64}     # RjShape<SLOTS>::THREADS
CLASS_PAD = 256                                                  # colour classes are padded to whole 256-position blocks
N_SITES = 1302
SCALE = 0.6                                                      # the typical coupling: standard deviation of the Gaussian J


# ---- exact energy ---------------------------------------------------------------------------------------------------------------
class _ExactSum:
    """sum_k sign_k x_k for fixed f64 x and varying signs, exactly: the x as integers over one power of two, cut into 30-bit
    limbs so that numpy's int64 dot products cannot overflow (|limb| < 2^30, fewer than 2^30 terms)."""

    def __init__(self, values):
        ratios = [float(x).as_integer_ratio() for x in values]
        self.den = max([d for _, d in ratios], default=1)
        nums = [n * (self.den // d) for n, d in ratios]
        limbs = max([abs(n).bit_length() for n in nums], default=0) // 30 + 1
        self.limbs = np.zeros((limbs, len(nums)), dtype=np.int64)
        for k, n in enumerate(nums):
            sign, n = (-1, -n) if n < 0 else (1, n)
            for j in range(limbs):
                self.limbs[j, k] = sign * ((n >> (30 * j)) & 0x3FFFFFFF)

    def __call__(self, signs):
        parts = self.limbs @ np.asarray(signs, dtype=np.int64)
        return Fraction(sum(int(p) << (30 * j) for j, p in enumerate(parts)), self.den)


class Exact:
    """the exact Hamiltonian of one graph, prepared once: energy(spins) as a Fraction"""

    def __init__(self, ea, eb, ej, nvars, biases=None):
        self.a, self.b, self.nvars = np.asarray(ea).astype(np.int64), np.asarray(eb).astype(np.int64), nvars
        self.bonds = _ExactSum(ej)
        self.fields = None if biases is None else _ExactSum(biases)

    def energy(self, spins):
        s = np.where(np.asarray(spins).astype(bool), 1, -1).astype(np.int64)
        assert s.shape == (self.nvars,)
        e = self.bonds(s[self.a] * s[self.b])
        return e if self.fields is None else e - self.fields(s)


def exact_energy(ea, eb, ej, nvars, spins, biases=None):
    return Exact(ea, eb, ej, nvars, biases).energy(spins)


# ---- the bound ------------------------------------------------------------------------------------------------------------------
def site_weights(ea, eb, ej, nvars, biases=None):
    """F_i = |h_i| + the sum of |J_e| over the bonds at site i (self-loops are not bonds)"""
    a, b, w = np.asarray(ea).astype(np.int64), np.asarray(eb).astype(np.int64), np.abs(np.asarray(ej, dtype=np.float64))
    off = a != b
    f = np.zeros(nvars) if biases is None else np.abs(np.asarray(biases, dtype=np.float64))
    np.add.at(f, a[off], w[off])
    np.add.at(f, b[off], w[off])
    return f


def energy_log2(ea, eb, ej, nvars, biases=None):
    """kE: the hi level's quantum is 2^kE, the lo level's 2^(kE - 24)"""
    fmax = float(site_weights(ea, eb, ej, nvars, biases).max()) if nvars else 0.0
    return math.frexp(fmax)[1] - 1 + 2 - 30 if fmax > 0.0 else 0


def energy_bound(ea, eb, ej, nvars, biases=None):
    a, b = np.asarray(ea), np.asarray(eb)
    off = a != b
    ones = lambda n: np.ones(n, dtype=np.int64)
    n_terms = int(np.count_nonzero(off)) + (0 if biases is None else nvars)
    total = _ExactSum(np.abs(ej[off]))(ones(int(np.count_nonzero(off))))
    if biases is not None:
        total += _ExactSum(np.abs(biases))(ones(nvars))
    q = Fraction(2) ** (energy_log2(ea, eb, ej, nvars, biases) - LO_BITS - 1)
    n_self = int(np.count_nonzero(~off))
    self_total = _ExactSum(np.abs(ej[~off]))(ones(n_self))
    return n_terms * q + ((1 + U) ** 2 - 1) * (total + n_terms * q) + n_self * U / (1 - n_self * U) * self_total


# ---- what the library derives from an edge list, restated for the host tests ---------------------------------------------------------
def degrees(g):
    off = g.ea != g.eb
    return np.bincount(np.concatenate([g.ea[off], g.eb[off]]).astype(np.int64), minlength=g.nvars)


def slots_for(max_degree):
    """graph.hip: the smallest ELL width of the family that holds the longest row"""
    return next(s for s in SLOT_COUNTS if max_degree <= s)


def greedy_colours(g):
    """host_logic.cpp greedy_colouring: in index order, the smallest colour no lower-indexed neighbour has"""
    nbrs = [[] for _ in range(g.nvars)]
    for a, b in zip(g.ea.tolist(), g.eb.tolist()):
        if a != b:
            nbrs[max(a, b)].append(min(a, b))
    colour = np.zeros(g.nvars, dtype=np.uint32)
    for i in range(g.nvars):
        used = {int(colour[j]) for j in nbrs[i]}
        colour[i] = next(c for c in range(len(used) + 1) if c not in used)
    return colour


def class_sizes(colours):
    return [int(c) for c in np.bincount(colours)]


def blocks_per_class(colours, slots):
    """workgroup-sized blocks the padded positions of each class make"""
    return [(c + CLASS_PAD - 1) // CLASS_PAD * CLASS_PAD // THREADS[slots] for c in class_sizes(colours)]


# ---- builders -------------------------------------------------------------------------------------------------------------------
# offsets 1, 3, 7, 13, 21, ...: odd (a bond joins sites of different parity), distinct, below half a turn
OFFSETS = [1 + j * (j + 1) for j in range(15)]
N_OFFSETS = {4: 2, 7: 3, 11: 5, 15: 7, 23: 10, 31: 15}
HALF_TURN = N_SITES // 2                                         # 651, odd: one more bond per site at 31 slots
HUB = 400                                                        # takes extra bonds until its degree is SLOTS exactly
HUB_OFFSETS = (301, 303, 305)
ISOLATED = 200                                                   # degree 0 (even: class 0 whatever its neighbours)
LEAF_EVEN, LEAF_ODD = 600, 901                                   # degree 1: the bond to LEAF_EVEN + 1 / to LEAF_ODD - 1
ODD_BOND = (ISOLATED + 1, ISOLATED + 3)                          # equal parity, both one bond short: the third colour
HEAVY_BOND = (1000, 1001)                                        # J = 0.99 x 2^18 ~ 4e5 scale: both ends heavy
HEAVY_BOND2 = (1001, 1004)                                       # J = -4e3: 1001's weight passes a power of two, 1004 is heavy too
PIN_UP, PIN_DOWN = 50, 75                                        # h = 1e6 scale on an even site, -4e3 scale on an odd one


def _circulant(slots, odd, bias, heavy, seed):
    n = N_SITES
    pairs = [(i, (i + d) % n) for d in OFFSETS[:N_OFFSETS[slots]] for i in range(n)]
    if slots == 31:
        pairs += [(i, i + HALF_TURN) for i in range(HALF_TURN)]
    base_degree = 2 * N_OFFSETS[slots] + (slots == 31)
    pairs += [(HUB, HUB + d) for d in HUB_OFFSETS[:slots - base_degree]]
    keep = {(LEAF_EVEN, LEAF_EVEN + 1), (LEAF_ODD - 1, LEAF_ODD)}
    lonely = {ISOLATED, LEAF_EVEN, LEAF_ODD}
    pairs = [p for p in pairs if not (lonely & set(p)) or p in keep]
    if odd:
        pairs.append(ODD_BOND)
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(pairs))
    flip = rng.random(len(pairs)) < 0.5                          # both orientations in the edge list
    ea = np.array([pairs[k][int(flip[k])] for k in order], dtype=np.uint64)
    eb = np.array([pairs[k][1 - int(flip[k])] for k in order], dtype=np.uint64)
    ej = rng.normal(size=len(pairs)) * SCALE
    biases = rng.normal(size=n) * (0.5 * SCALE) if bias else None
    if heavy:
        # 0.99 x 2^18: site 1000's weight stays below 2^18, site 1001's (this bond and the next) passes it: two shifts
        for (a, b), j in ((HEAVY_BOND, 0.99 * 2.0 ** 18), (HEAVY_BOND2, -4e3)):
            hit = np.flatnonzero((np.minimum(ea, eb) == a) & (np.maximum(ea, eb) == b))
            assert len(hit) == 1, (a, b)
            ej[hit[0]] = j
        if bias:
            biases[PIN_UP], biases[PIN_DOWN] = 1e6 * SCALE, -4e3 * SCALE
    name = f"{'odd-cycle' if odd else 'bipartite'}-{slots}-{'bias' if bias else 'nobias'}-{'heavy' if heavy else 'light'}"
    return Graph(name, ea, eb, ej, n, biases, SCALE)


def bipartite_circulant(slots, bias, heavy):
    """1302 sites on a ring, bonds i -- i + d for odd offsets d: the index-order greedy colouring colours by parity (two classes
    of 651 sites = 768 positions: 3 / 6 / 11 blocks of 256 / 128 / 64 threads, the last one part-filled).  One site of degree
    SLOTS exactly (HUB; every site at 4 and 31 slots), one of degree 0, two of degree 1, Gaussian couplings."""
    return _circulant(slots, False, bias, heavy, 100 + slots)


def odd_cycle(slots, bias, heavy):
    """the same graph (same couplings) plus ONE bond between two odd sites: three colours, classes of 651, 650 and 1 sites"""
    return _circulant(slots, True, bias, heavy, 100 + slots)


def all_graphs():
    return [f(slots, bias, heavy) for f in (bipartite_circulant, odd_cycle) for slots in SLOT_COUNTS for bias in (False, True)
            for heavy in (False, True)]


# ---- the oracle's configurations after every step --------------------------------------------------------------------------------------
def oracle_trajectory(oracle, g, seeds, T, betas=None, beta_replica=None, t0=0, states=None):
    """(spins uint8[T, 32 G, nvars], energies f64[R, T]) of oracle engine E, one call per timestep (the engine continues in the
    array it is handed); R = len(seeds), rows beyond R are the padding replicas of the last group"""
    spins, eps = [], []
    for k in range(T):
        e, states = oracle.rj_run(g.ea, g.eb, g.ej, g.nvars, seeds, 1, betas=None if betas is None else [betas[k]],
                                  beta_replica=beta_replica, biases=g.biases, states=states, t0=t0 + k)
        spins.append(states.copy())
        eps.append(e)
    return np.stack(spins), np.stack(eps, axis=1)

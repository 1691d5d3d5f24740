"""Philox4x32-R and the Metropolis sweep of the periodic, field-free, one-|J| checkerboard lattice at R rounds, restated in numpy
-- TEST INFRASTRUCTURE, no GPU, no oracle.

The C oracle knows ten rounds only, so this module is the yardstick of the option "philox_rounds" = 7.  It is
written from the text of DESIGN.md S2 (layout), S3 (acceptance, thresholds) and S6 (counters, ties):

 * colour c = (x + y) & 1; the colour-c sites of row y are x = 2 i + ((y + c) & 1); plane c keeps spin i of row y at bit i & 31 of
   word y wpr + (i >> 5), wpr = W / 64; a replica is plane 0 followed by plane 1; quad Q = words 4 Q .. 4 Q + 3 of a plane;
 * a bond is satisfied when J s s' < 0; a spin with k <= 2 satisfied bonds flips, one with k = 3 / 4 flips iff its 39-bit uniform
   u = prefix << 32 | low is below T = floor(exp(-beta |J| 4 (k - 2)) 2^39);
 * bit p (MSB first) of the 7-bit prefix of the spin at word q, bit b of quad Q is bit b of word q of
   Philox_R(key, (t_lo, Q, "LATS", ctr2(t, colour, p))); `low` is drawn for a tie alone (prefix == T >> 32) and is word n % 4 of
   call 7 + n / 4 for the n-th tie of the quad in (word, bit) order;
 * colour 0 first, then colour 1 on the updated colour-0 spins; the initial configuration is ten rounds whatever R is (domain
   "LATI": the caller takes it from the oracle).

It is pinned at R = 10 against Random123's known answers and against the C oracle's trajectories by
tests/test_philox_rounds_host.py before anything trusts it at R = 7.  The sweep also returns the number of ties of every quad."""
import json
import os
from collections import namedtuple

import numpy as np

import lat_variants_reference as LV
from tie_reference import ALWAYS, N_PLANES, threshold

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK, S32 = np.uint64(0xFFFFFFFF), np.uint64(32)
DOM_LAT_SWEEP = int.from_bytes(b"LATS", "big")
ROUNDS = (7, 10)


def philox_round(c, k0, k1):
    """one round on four uint64 arrays holding 32-bit values, with the round key (k0, k1)"""
    c0, c1, c2, c3 = c
    p0, p1 = M0 * c0, M1 * c2
    return [(p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & MASK]


def round_key(k0, k1, r):
    """the key of round r + 1: bumped r times"""
    return (int(k0) + r * W0) & 0xFFFFFFFF, (int(k1) + r * W1) & 0xFFFFFFFF


def philox4x32(R, c0, c1, c2, c3, k0, k1, first_round=0):
    """Philox4x32-R, vectorised: counter words broadcast against each other; four uint32 arrays.  first_round > 0 continues a
    shorter call: rounds first_round + 1 .. R on the words passed in."""
    c = [np.asarray(x, dtype=np.uint64) for x in np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3)])]
    for r in range(first_round, R):
        c = philox_round(c, *round_key(k0, k1, r))
    return [x.astype(np.uint32) for x in c]


def ctr2(t, colour, call):
    return (((int(t) >> 32) & 0xFFFF) << 16) | (int(colour) << 8) | int(call)


# ---- layout (S2) -------------------------------------------------------------------------------------------------------------------
Layout = namedtuple("Layout", "W H wpr wpp nquads c w b")
_LAYOUTS = {}


def layout(W, H):
    if (W, H) not in _LAYOUTS:
        y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        c = (x + y) & 1
        i = x >> 1
        wpr = W // 64
        _LAYOUTS[(W, H)] = Layout(W, H, wpr, H * wpr, H * wpr // 4, c, y * wpr + (i >> 5), i & 31)
    return _LAYOUTS[(W, H)]


def unpack(L, words):
    """uint8[H, W] spins of one replica's 2 wpp words"""
    return ((np.asarray(words, dtype=np.uint32)[L.c * L.wpp + L.w] >> L.b.astype(np.uint32)) & np.uint32(1)).astype(np.uint8)


def pack(L, spins):
    words = np.zeros(2 * L.wpp, dtype=np.uint32)
    np.bitwise_or.at(words, (L.c * L.wpp + L.w).ravel(), (spins.astype(np.uint32) << L.b.astype(np.uint32)).ravel())
    return words


# ---- one timestep (S3, S6) ----------------------------------------------------------------------------------------------------------
def satisfied_bonds(case, spins):
    """int[H, W]: satisfied bonds of every site; jright / jdown hold 1 where J > 0, and J s s' < 0 means equal spins for J < 0"""
    right = (spins != np.roll(spins, -1, axis=1)) == (case.jright == 1)   # the bond (x, y) - (x + 1, y)
    down = (spins != np.roll(spins, -1, axis=0)) == (case.jdown == 1)     # the bond (x, y) - (x, y + 1)
    return right.astype(np.int64) + np.roll(right, 1, axis=1) + down + np.roll(down, 1, axis=0)


def sweep(case, words, seed, t, beta, rounds):
    """One timestep of one replica at `rounds` Philox rounds.  Returns (the new words, ties[colour][quad])."""
    assert rounds in ROUNDS
    L = layout(case.W, case.H)
    spins = unpack(L, words)
    k0, k1 = int(seed) & 0xFFFFFFFF, int(seed) >> 32
    T = {3: threshold(beta, 4.0 * case.jx), 4: threshold(beta, 8.0 * case.jx)}
    quads = np.arange(L.nquads, dtype=np.uint64)
    ties = np.zeros((2, L.nquads), dtype=np.int64)
    Q, q = L.w >> 2, L.w & 3

    def call(colour, index, which=quads):
        return np.stack(philox4x32(rounds, int(t) & 0xFFFFFFFF, which, DOM_LAT_SWEEP, ctr2(t, colour, index), k0, k1))   # [4, quads]

    for colour in (0, 1):
        mine = L.c == colour
        k = satisfied_bonds(case, spins)
        prefix = np.zeros((L.H, L.W), dtype=np.int64)
        for p in range(N_PLANES):
            prefix = (prefix << 1) | ((call(colour, p)[q, Q] >> L.b.astype(np.uint32)) & 1)
        thr = np.where(k == 4, T[4], np.where(k == 3, T[3], ALWAYS)).astype(np.int64)
        flip = mine & ((thr >= ALWAYS) | (prefix < (thr >> 32)))
        tie = mine & (thr < ALWAYS) & (prefix == (thr >> 32))
        ys, xs = np.nonzero(tie)
        order = np.lexsort((L.b[ys, xs], L.w[ys, xs]))   # by quad, then (word, bit) inside it
        n_in_quad = {}
        for y, x in zip(ys[order], xs[order]):
            quad = int(Q[y, x])
            n = n_in_quad.get(quad, 0)
            n_in_quad[quad] = n + 1
            low = int(call(colour, N_PLANES + n // 4, np.array([quad], dtype=np.uint64))[n % 4, 0])
            flip[y, x] = ((int(prefix[y, x]) << 32) | low) < int(thr[y, x])
        for quad, n in n_in_quad.items():
            ties[colour, quad] = n
        spins = spins ^ flip.astype(np.uint8)
    return pack(L, spins), ties


def tie_classes(case, words, seed, t, beta, rounds):
    """(ties of class 3, ties of class 4) of the timestep `sweep` would make: for the coverage condition of the fixtures"""
    L = layout(case.W, case.H)
    spins, out = unpack(L, words), [0, 0]
    k0, k1 = int(seed) & 0xFFFFFFFF, int(seed) >> 32
    T = {3: threshold(beta, 4.0 * case.jx), 4: threshold(beta, 8.0 * case.jx)}
    Q, q = L.w >> 2, L.w & 3
    for colour in (0, 1):
        k = satisfied_bonds(case, spins)
        prefix = np.zeros((L.H, L.W), dtype=np.int64)
        for p in range(N_PLANES):
            words_p = np.stack(philox4x32(rounds, int(t) & 0xFFFFFFFF, np.arange(L.nquads, dtype=np.uint64), DOM_LAT_SWEEP, ctr2(t, colour, p), k0, k1))
            prefix = (prefix << 1) | ((words_p[q, Q] >> L.b.astype(np.uint32)) & 1)
        for n, cls in enumerate((3, 4)):
            if T[cls] < ALWAYS:
                out[n] += int(((L.c == colour) & (k == cls) & (prefix == (T[cls] >> 32))).sum())
        if colour == 0:
            spins = unpack(L, sweep_colour0(case, words, seed, t, beta, rounds))
    return tuple(out)


def sweep_colour0(case, words, seed, t, beta, rounds):
    """the words after the colour-0 half of the timestep alone (colour 1's spins as they were)"""
    L = layout(case.W, case.H)
    new, _ = sweep(case, words, seed, t, beta, rounds)
    keep = np.asarray(words, dtype=np.uint32).copy()
    keep[:L.wpp] = new[:L.wpp]
    return keep


def energy(case, words):
    """E = sum over bonds of J s s', exact: |J| times an integer"""
    L = layout(case.W, case.H)
    s = 2 * unpack(L, words).astype(np.int64) - 1
    jr, jd = 2 * case.jright.astype(np.int64) - 1, 2 * case.jdown.astype(np.int64) - 1
    return case.jx * float((jr * s * np.roll(s, -1, axis=1)).sum() + (jd * s * np.roll(s, -1, axis=0)).sum())


# ---- trajectories --------------------------------------------------------------------------------------------------------------------
Run = namedtuple("Run", "start steps")          # start: words[R, 2 wpp]; steps: one Step per timestep
Step = namedtuple("Step", "words ties")         # words[R, 2 wpp] after the timestep; ties[R, 2, nquads] of it


def run(O, W, H, coupling, seeds, betas, rounds, t0=0, start=None):
    """`len(betas)` timesteps of the replicas of `seeds` from timestep t0; betas[k] is a float or an array of one beta per replica.
    rounds: one round count, or one per timestep.  start: words[R, 2 wpp] (default: the oracle's initial configurations, which
    are ten rounds of domain "LATI" whatever the option says)."""
    case = LV.make_case(W, H, coupling)
    if start is None:
        lat = LV.oracle_lat(O, case)
        start = np.stack([lat.init(s) for s in seeds])
    cur, steps = np.array(start, dtype=np.uint32), []
    for k, beta in enumerate(betas):
        R_k = rounds if np.isscalar(rounds) else rounds[k]
        out = [sweep(case, cur[r], seeds[r], t0 + k, float(np.asarray(beta).ravel()[r % np.asarray(beta).size]), R_k) for r in range(len(seeds))]
        cur = np.stack([o[0] for o in out])
        steps.append(Step(cur.copy(), np.stack([o[1] for o in out])))
    return Run(np.array(start, dtype=np.uint32), steps)


def energies(case, words):
    return np.array([energy(case, w) for w in words])


# ---- the fixed cases of tests/test_gpu_philox_rounds.py ----------------------------------------------------------------------------
# Every kernel test runs UNIFORM (one call of these betas: two ordering steps, so that most spins sit in the costly classes and
# ties are common; beta 0: both classes flip outright) and then PER_REPLICA (three more timesteps under per-replica betas).
UNIFORM = (1.2, 0.9, 0.9, 0.4407, 0.0, 0.9)
PER_REPLICA = (np.array([0.7, 0.9, 1.1]),) * 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "philox7_tie_cases.json")

# kernel group -> the shapes its test runs (names of tests/lat_variants_reference.py and tests/strip_ladder_reference.py)
GROUPS = {
    "resident": ((64, 4), (256, 8)),                  # the smallest resident shapes: non-VEC and VEC
    "stream": ((192, 12), (768, 12), (1024, 32)),     # lat_sweep_kernel / lat_sweep_measure_kernel <F,*,F>, <T,*,F>, <T,*,T>
    "loop": ((512, 512),),                            # 1024 quads: sweep_iters 2 and 4, the largest 512 x 512 allows
    "strip": ((256, 128), (256, 512)),                # two strips of one wave / of four waves
}


def fixture():
    with open(GOLDEN) as f:
        return json.load(f)


def case_seeds(group, coupling):
    """the three seeds of a group's cases: the searched one first (tests/golden/make_philox7_tie_cases.py), then two of LV.SEEDS"""
    return np.array([fixture()["seeds"][group][coupling], int(LV.SEEDS[1]), int(LV.SEEDS[2])], dtype=np.uint64)


_RUNS = {}


def case_run(O, group, shape, coupling, rounds=7, seeds=None):
    """the reference trajectory of one fixed case: UNIFORM then PER_REPLICA, computed once and shared"""
    seeds = case_seeds(group, coupling) if seeds is None else seeds
    key = (shape, coupling, rounds, tuple(int(s) for s in seeds))
    if key not in _RUNS:
        _RUNS[key] = run(O, shape[0], shape[1], coupling, seeds, list(UNIFORM) + list(PER_REPLICA), rounds)
    return _RUNS[key]


def coverage(O, group, coupling, rounds=7, seeds=None):
    """(ties of class 3, ties of class 4, the most ties in one quad) over the group's cases"""
    seeds = case_seeds(group, coupling) if seeds is None else seeds
    n3 = n4 = most = 0
    for shape in GROUPS[group]:
        case = LV.make_case(shape[0], shape[1], coupling)
        traj = case_run(O, group, shape, coupling, rounds, seeds)
        betas = list(UNIFORM) + list(PER_REPLICA)
        before = traj.start
        for k, step in enumerate(traj.steps):
            most = max(most, int(step.ties.max()))
            for r in range(len(seeds)):
                if step.ties[r].sum():
                    a, b = tie_classes(case, before[r], seeds[r], k, float(np.asarray(betas[k]).ravel()[r % np.asarray(betas[k]).size]), rounds)
                    n3, n4 = n3 + a, n4 + b
            before = step.words
    return n3, n4, most

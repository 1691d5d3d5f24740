"""The population-annealing resampling of DESIGN.md S14, restated with numpy and Python integers -- TEST INFRASTRUCTURE, no GPU.

Written from the S14 text alone: reference energy, the exponent as three separately rounded f64 operations, 2^32 fixed-point
weights of the oracle's det_exp, exact integer sums, the offset from one Philox4x32-10 call, the source of slot j as the replica
whose interval of R C holds j S + u, and the two gathers on arrays in the device layouts (rows of a checkerboard container,
bits of the words of a replica-packed one).  sources() and bit_gather() are the definition, one Python step per slot;
sources_fast() and bit_gather_fast() are their vectorised twins for the populations of tests/test_gpu_pa_large.py.
"""
import math
from fractions import Fraction

import numpy as np

DOM_RESAMPLE = int.from_bytes(b"PARS", "big")


def weights(energies, dbeta):
    """(W as Python integers, E_ref)."""
    from oracle import oracle as O

    e = np.asarray(energies, dtype=np.float64)
    eref = np.float64(e.min() if dbeta >= 0 else e.max())
    x = -(np.float64(dbeta) * (e - eref))   # numpy rounds every operation on its own
    return [int(math.floor(math.ldexp(O.det_exp(float(v)), 32))) for v in x], float(eref)


def offset(seed, step, total):
    from oracle import oracle as O

    r = O.philox([int(step) & 0xFFFFFFFF, int(step) >> 32, 0, DOM_RESAMPLE], [int(seed) & 0xFFFFFFFF, int(seed) >> 32])
    U = (int(r[1]) << 32) | int(r[0])
    return (U * total) >> 64


def sources(seed, step, energies, dbeta):
    """dict(src uint32[R], sum, eref, distinct, mean_energy, weights)."""
    W, eref = weights(energies, dbeta)
    R, S = len(W), sum(W)
    C = np.cumsum(np.array(W, dtype=object))
    u = offset(seed, step, S)
    src = np.zeros(R, dtype=np.uint32)
    r = 0
    for j in range(R):
        t = j * S + u
        while not t < R * int(C[r]):
            r += 1
        assert (R * int(C[r - 1]) if r else 0) <= t
        src[j] = r
    return dict(src=src, sum=S, eref=eref, distinct=len(set(src.tolist())), mean_energy=float(np.mean(np.asarray(energies, dtype=np.float64))),
                weights=W)


def sources_fast(seed, step, energies, dbeta):
    """The vectorised twin of sources() for populations up to 2^21 (sources() stays the definition; tests/test_pa_host.py holds the
    two equal).  One det_exp per distinct exponent; the prefix sums in uint64 (S <= R 2^32 <= 2^53: exact); the quotient
    q[j] = floor((j S + u) / R) from S = a R + b as j a + floor((j b + u) / R), every term below 2^64 (j, b < 2^21, u < 2^53,
    a <= 2^32); the source of slot j is the smallest r with R C[r] > j S + u, that is the smallest r with C[r] > q[j].
    Returns the keys of sources() (weights as uint64[R]), needs_high_words: R S >= 2^64, the populations at which the device's
    128-bit compare has non-zero high words, and low_word_carries: the number of slots j at which the low word of j S overflows
    when u is added (it can only happen once R S >= 2^64)."""
    from oracle import oracle as O

    e = np.asarray(energies, dtype=np.float64)
    R = len(e)
    assert 0 < R <= 1 << 21
    eref = np.float64(e.min() if dbeta >= 0 else e.max())
    x = -(np.float64(dbeta) * (e - eref))
    distinct_x, inverse = np.unique(x, return_inverse=True)
    W = np.array([int(math.floor(math.ldexp(O.det_exp(float(v)), 32))) for v in distinct_x], dtype=np.uint64)[inverse.ravel()]
    C = np.cumsum(W, dtype=np.uint64)
    S = int(C[-1])
    assert S <= R << 32
    u = offset(seed, step, S)
    a, b = divmod(S, R)
    j = np.arange(R, dtype=np.uint64)
    q = j * np.uint64(a) + (j * np.uint64(b) + np.uint64(u)) // np.uint64(R)
    src = np.searchsorted(C, q, side="right").astype(np.uint32)
    low = j * np.uint64(S % (1 << 64))   # the low word of j S (uint64 arrays wrap)
    return dict(src=src, sum=S, eref=float(eref), distinct=len(np.unique(src)), mean_energy=float(np.mean(e)), weights=W,
                needs_high_words=R * S >= 1 << 64, low_word_carries=int((low + np.uint64(u) < low).sum()))


def log_q(rec, R, dbeta):
    """ln Q of a step record: the estimate of ln Z(beta_to) - ln Z(beta_from)."""
    return math.log(Fraction(rec["sum"], R << 32)) - dbeta * rec["eref"]


def row_gather(rows, src):
    """u32[R][state_words] of a checkerboard container: new[j] = old[src[j]]."""
    rows = np.asarray(rows)
    return rows[np.asarray(src, dtype=np.int64)].copy()


def bit_gather(words, src, padding=None):
    """u32[groups][n_pos] of a replica-packed container, replica s = bit s % 32 of group s / 32: the slots j < len(src) take the
    bit of slot src[j]; slots beyond and the positions marked in padding[n_pos] (bool) keep their bits."""
    words = np.asarray(words, dtype=np.uint32)
    out = words.copy()
    groups, n_pos = words.shape
    real = np.ones(n_pos, dtype=bool) if padding is None else ~np.asarray(padding, dtype=bool)
    for j, sj in enumerate(np.asarray(src, dtype=np.int64)):
        bit = (words[sj // 32] >> np.uint32(sj % 32)) & np.uint32(1)
        new = (out[j // 32] & ~np.uint32(1 << (j % 32))) | (bit << np.uint32(j % 32))
        out[j // 32] = np.where(real, new, out[j // 32])
    return out


def bit_gather_fast(words, src, padding=None):
    """The vectorised twin of bit_gather(): 32 passes, one per target bit, each over every target group at once."""
    words = np.asarray(words, dtype=np.uint32)
    src = np.asarray(src, dtype=np.int64)
    groups, n_pos = words.shape
    R = len(src)
    owned = (R + 31) // 32   # groups with at least one slot below R
    real = np.ones(n_pos, dtype=bool) if padding is None else ~np.asarray(padding, dtype=bool)
    cols = np.nonzero(real)[0]
    live = np.ascontiguousarray(words[:, cols])   # the real positions alone: padding keeps its words
    acc = np.zeros((owned, len(cols)), dtype=np.uint32)
    for b in range(32):
        s = src[b::32]   # the sources of bit b of groups 0, 1, ...
        acc[:len(s)] |= ((live[s >> 5] >> (s & 31).astype(np.uint32)[:, None]) & np.uint32(1)) << np.uint32(b)
    mask = np.full(owned, 0xFFFFFFFF, dtype=np.uint32)
    if R % 32:
        mask[-1] = (1 << (R % 32)) - 1
    out = words.copy()
    out[:owned, cols] = (live[:owned] & ~mask[:, None]) | acc
    return out


def spins_to_words(G, spins):
    """spins[32 groups, nvars] (row = slot) -> u32[groups][n_pos] in the packed device layout (padding positions zero)."""
    spins = np.asarray(spins, dtype=np.uint32)
    groups = spins.shape[0] // 32
    words = np.zeros((groups, G.n_pos), dtype=np.uint32)
    for s in range(spins.shape[0]):
        words[s // 32, G.pos] |= spins[s] << np.uint32(s % 32)
    return words


def words_to_spins(G, words):
    words = np.asarray(words, dtype=np.uint32)
    return np.stack([((words[s // 32, G.pos] >> np.uint32(s % 32)) & 1).astype(np.uint8) for s in range(32 * words.shape[0])])


def gather_spins(G, spins, src):
    """The bit gather applied to the slots x sites array the packed restatements carry."""
    pad = np.ones(G.n_pos, dtype=bool)
    pad[G.pos] = False
    return words_to_spins(G, bit_gather(spins_to_words(G, spins), src, pad))

"""The population-annealing resampling of DESIGN.md S14, restated with numpy and Python integers -- TEST INFRASTRUCTURE, no GPU.

Written from the S14 text alone: reference energy, the exponent as three separately rounded f64 operations, 2^32 fixed-point
weights of the oracle's det_exp, exact integer sums, the offset from one Philox4x32-10 call, the source of slot j as the replica
whose interval of R C holds j S + u, and the two gathers on arrays in the device layouts (rows of a checkerboard container,
bits of the words of a replica-packed one).
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

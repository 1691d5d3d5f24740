"""The step chooser of population annealing, restated with numpy and Python integers -- TEST INFRASTRUCTURE, no GPU.

Written from the S25 text alone.  The weights are those of tests/pa_reference.py (weights(): reference energy, the exponent as
three separately rounded f64 operations, 2^32 fixed point of the oracle's det_exp), taken once per DISTINCT energy -- the weight
of a replica depends on its energy alone, and min E is among the distinct energies -- and carried to the replicas by their
multiplicities.  Sums, products and the predicate are Python integers of any width.
"""
import math

import numpy as np

import pa_reference as PA

GRID = 65536


def target32(target):
    """t32 = ceil(target 2^32): the scaling is exact, the ceiling taken on a Python float that holds an exact value."""
    return math.ceil(math.ldexp(float(target), 32))


def candidate_dbeta(k, dbeta_max):
    """dbeta_k = double(k) * (dbeta_max 2^-16): an exact scaling, then one rounded multiplication."""
    return float(np.float64(k) * np.float64(math.ldexp(float(dbeta_max), -16)))


def evaluate(levels, counts, R, k, dbeta_max, t32):
    """dict(k, dbeta, sum, num, holds) of candidate k on the population of counts[i] replicas at energy levels[i]."""
    dbeta = candidate_dbeta(k, dbeta_max)
    W, _ = PA.weights(levels, dbeta)
    S = sum(int(c) * w for c, w in zip(counts, W))
    N = sum(int(c) * min(S, R * w) for c, w in zip(counts, W))
    return dict(k=k, dbeta=dbeta, sum=S, num=N, holds=(N << 32) >= t32 * R * S)


def choose_step(energies, dbeta_max, target):
    """dict(k, dbeta, sum, num) of the chosen step, and `evaluated`: the record of every candidate the search looked at, in order."""
    e = np.asarray(energies, dtype=np.float64)
    R = len(e)
    levels, counts = np.unique(e, return_counts=True)
    t32 = target32(target)
    assert 1 <= t32 <= 1 << 32 and dbeta_max > 0 and R >= 1
    seen = {}

    def at(k):
        if k not in seen:
            seen[k] = evaluate(levels, counts, R, k, dbeta_max, t32)
        return seen[k]

    lo, width = 0, GRID
    for rnd in range(4):
        step = width // 16
        jstar = 0
        for j in range(1, 17 if rnd == 0 else 16):
            if not at(lo + j * step)["holds"]:
                break
            jstar = j
        lo += jstar * step
        width = step
        if rnd == 0 and jstar == 16:
            break
    k = max(lo, 1)
    res = at(k)   # (k = 1 is the first candidate of the last round when lo stays 0: nothing new is evaluated here)
    return dict(k=k, dbeta=res["dbeta"], sum=res["sum"], num=res["num"], evaluated=list(seen.values()))


def overlap(choice, R):
    """N / (R S) as an exact fraction."""
    from fractions import Fraction
    return Fraction(choice["num"], R * choice["sum"])

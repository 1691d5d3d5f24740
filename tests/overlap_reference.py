"""Spin and link overlaps between two configurations of one graph, restated in numpy on site arrays and the edge
list -- TEST INFRASTRUCTURE, no GPU, no layout.

For pair p = (row pa[p] of A, row pb[p] of B), spins s = 2 x - 1 of the bool / uint8 rows states() returns:
    spin[p] = sum_i s_i^a s_i^b                                   every site 0 .. nvars - 1, whether it is in an edge or not
    link[p] = sum_e s_{a_e}^a s_{b_e}^a s_{a_e}^b s_{b_e}^b       one term per entry of the edge list as the graph was created from
                                                                  it: zero couplings included, duplicated entries separate terms
An entry with a_e == b_e is accepted by graph creation (its J is a constant of the energy); its term here is (s_a^a)^2 (s_a^b)^2 =
+1 whatever the spins, which the formula gives without a special case.  No coupling and no bias enters.  Both results are int64.
"""
import numpy as np


def overlaps(A, B, ea, eb, pa, pb):
    """A[Ra, nvars], B[Rb, nvars]: configurations (bool or 0 / 1); ea, eb: the edge list; pa, pb: the rows of every pair.
    Returns (spin, link), int64[len(pa)] each."""
    A, B = np.asarray(A) != 0, np.asarray(B) != 0
    ea, eb = np.asarray(ea, dtype=np.int64), np.asarray(eb, dtype=np.int64)
    pa, pb = np.asarray(pa, dtype=np.int64), np.asarray(pb, dtype=np.int64)
    spin = np.zeros(len(pa), dtype=np.int64)
    link = np.zeros(len(pa), dtype=np.int64)
    for p, (ra, rb) in enumerate(zip(pa, pb)):
        q = 1 - 2 * (A[ra] != B[rb]).astype(np.int8)   # s_i^a s_i^b of every site (one row at a time: the populations are large)
        spin[p] = q.sum(dtype=np.int64)
        link[p] = (q[ea] * q[eb]).sum(dtype=np.int64)
    return spin, link


def default_pairs(count):
    """The pairing of the isoenergetic moves inside one container: (2 p, 2 p + 1); a last replica without a partner is left out."""
    p = np.arange(count // 2, dtype=np.int64)
    return 2 * p, 2 * p + 1

"""The rows of the observable series, restated in numpy from the configurations alone -- TEST INFRASTRUCTURE, no
GPU, no layout.

For the configurations A bool[R, N] (True = spin up, what States.states() returns), per replica r:
    magnetisation[r]      sum_i s_i,                       s_i = 2 A[r, i] - 1
    by_class[r][t][c]     sum of s_i over the sites i with tables[t][i] == c   (NO_CLASS sites count nowhere, an empty class gives 0)
The sample points of a period are those of the overlap series: sample_points is its function, not a copy.
"""
import numpy as np

from class_overlap_reference import NO_CLASS
from overlap_series_reference import sample_points  # noqa: F401  (re-exported: the rule is stated once)


def magnetisation(A):
    """int64[R]"""
    A = np.asarray(A).astype(np.int64)
    return 2 * A.sum(axis=1) - A.shape[1]


def class_sums(A, tables, n_classes):
    """int64[R, n_tables, n_classes]"""
    s = 2 * np.asarray(A).astype(np.int64) - 1
    tables = np.asarray(tables).astype(np.int64)
    out = np.zeros((s.shape[0], len(tables), n_classes), dtype=np.int64)
    for t, table in enumerate(tables):
        for c in range(n_classes):
            out[:, t, c] = s[:, table == c].sum(axis=1)  # (c < n_classes <= NO_CLASS: a NO_CLASS site matches no c)
    assert n_classes <= NO_CLASS
    return out

"""The row format of the overlap series, restated in numpy on top of tests/overlap_reference.py and
tests/class_overlap_reference.py -- TEST INFRASTRUCTURE, no GPU, no layout.

A row is int64[n_pairs][1 + link + n_tables * n_classes]: for pair p = (row pa[p] of A, row pb[p] of B)
    entry 0                           the spin overlap                     (overlap_reference.overlaps()[0])
    entry 1, with link                the link overlap                     (overlap_reference.overlaps()[1])
    the n_tables * n_classes behind   out[p][t][c], t major                (class_overlap_reference.overlaps_by_class)
"""
import numpy as np

import class_overlap_reference as CR
import overlap_reference as OR


def entries(link, n_tables=0, n_classes=0):
    return 1 + (1 if link else 0) + n_tables * n_classes


def row(A, B, ea, eb, pa, pb, link=True, tables=None, n_classes=0):
    """int64[len(pa), entries]: one row of the log for the configurations A, B."""
    spin, lnk = OR.overlaps(A, B, ea, eb, pa, pb)
    parts = [spin[:, None]] + ([lnk[:, None]] if link else [])
    if tables is not None:
        parts.append(CR.overlaps_by_class(A, B, tables, n_classes, pa, pb).reshape(len(spin), -1))
    return np.concatenate(parts, axis=1).astype(np.int64)


def split(rows, link, n_tables=0, n_classes=0):
    """rows int64[n, P, entries] -> (spin[n, P], link[n, P] or None, by_class[n, P, T, C] or None): what OverlapSeries.get returns."""
    rows = np.asarray(rows, dtype=np.int64)
    n, P, E = rows.shape
    assert E == entries(link, n_tables, n_classes)
    off = 2 if link else 1
    by_class = rows[:, :, off:].reshape(n, P, n_tables, n_classes) if n_tables else None
    return rows[:, :, 0], (rows[:, :, 1] if link else None), by_class


def sample_points(t0, every, t_from, t_to):
    """The timesteps t in (t_from, t_to] with (t - t0) % every == 0: where a periodic series with base t0 takes its rows."""
    return [t for t in range(t_from + 1, t_to + 1) if (t - t0) % every == 0]

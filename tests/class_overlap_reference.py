"""The spin overlap between two configurations resolved by a class label per site, restated in numpy on site arrays
-- TEST INFRASTRUCTURE, no GPU, no layout -- and the segment rule of the replica-packed layout for the host twin.

For pair p = (row pa[p] of A, row pb[p] of B), spins s = 2 x - 1 of the bool / uint8 rows states() returns, and table t:
    out[p][t][c] = sum over the sites i with cls[t][i] == c of s_i^a s_i^b            int64, NO_CLASS sites counted nowhere
"""
import numpy as np

NO_CLASS = 0xFFFFFFFF
PAD_SITE = 0xFFFFFFFF
SEGMENT_MAX = 1024


def overlaps_by_class(A, B, tables, n_classes, pa, pb):
    """A[Ra, nvars], B[Rb, nvars]: configurations (bool or 0 / 1); tables[n_tables, nvars]; pa, pb: the rows of every pair.
    Returns int64[len(pa), n_tables, n_classes]."""
    A, B = np.asarray(A) != 0, np.asarray(B) != 0
    tables = np.atleast_2d(np.asarray(tables, dtype=np.int64))
    out = np.zeros((len(pa), len(tables), n_classes), dtype=np.int64)
    valid = [t != NO_CLASS for t in tables]
    for p, (ra, rb) in enumerate(zip(np.asarray(pa, dtype=np.int64), np.asarray(pb, dtype=np.int64))):
        q = 1 - 2 * (A[ra] != B[rb]).astype(np.int64)   # s_i^a s_i^b of every site
        for t, cls in enumerate(tables):
            out[p, t] = np.bincount(cls[valid[t]], weights=q[valid[t]], minlength=n_classes).astype(np.int64)
    return out


def class_sizes(tables, n_classes):
    tables = np.atleast_2d(np.asarray(tables, dtype=np.int64))
    return np.stack([np.bincount(t[t != NO_CLASS], minlength=n_classes) for t in tables]).astype(np.uint64)


def class_segments(site, tables, n_classes):
    """The segment rule: per table the positions p with site[p] != PAD_SITE and a class, sorted by (class, position), cut class by
    class into runs of at most SEGMENT_MAX.  Returns (order, seg[n_seg, 4] = {table, class, first, count})."""
    site = np.asarray(site, dtype=np.int64)
    order, seg = [], []
    for t, cls in enumerate(np.atleast_2d(np.asarray(tables, dtype=np.int64))):
        for c in range(n_classes):
            members = [p for p in range(len(site)) if site[p] != PAD_SITE and cls[site[p]] == c]
            for k in range(0, len(members), SEGMENT_MAX):
                run = members[k:k + SEGMENT_MAX]
                seg.append((t, c, len(order), len(run)))
                order.extend(run)
    return np.array(order, dtype=np.uint32), np.array(seg, dtype=np.uint32).reshape(-1, 4)


# ---- graphs of the real-coupling family, as tests/test_gpu_overlaps.py builds its own ------------------------------------------
def gaussian_glass_2d(W=12, H=10, seed=2024):
    """A W x H periodic square lattice with Gaussian couplings and Gaussian biases: (ea, eb, ej, nvars, biases)."""
    rng = np.random.default_rng(seed)
    y, x = np.divmod(np.arange(W * H), W)
    ea = np.concatenate([y * W + x, y * W + x]).astype(np.uint64)
    eb = np.concatenate([y * W + (x + 1) % W, ((y + 1) % H) * W + x]).astype(np.uint64)
    return ea, eb, rng.normal(size=len(ea)), W * H, rng.normal(size=W * H)


def degree_15_graph():
    """300 sites, degrees up to 15, Gaussian couplings with zeros among them, one duplicated entry and one entry a_e == b_e."""
    rng = np.random.default_rng(15)
    n, pairs, deg = 300, set(), np.zeros(300, dtype=int)
    while len(pairs) < 1900:
        a, b = (int(v) for v in rng.integers(0, n, 2))
        if a != b and deg[a] < 14 and deg[b] < 14 and (min(a, b), max(a, b)) not in pairs:
            pairs.add((min(a, b), max(a, b)))
            deg[a] += 1
            deg[b] += 1
    pairs = sorted(pairs)
    rng.shuffle(pairs)
    full = [p for p in pairs if deg[p[0]] == 14 and deg[p[1]] == 14]
    assert full, "no bond between two sites of degree 14 to duplicate"
    pairs.append((full[0][1], full[0][0]))
    pairs.append((5, 5))
    ea, eb = np.array([p[0] for p in pairs], dtype=np.uint64), np.array([p[1] for p in pairs], dtype=np.uint64)
    ej = rng.normal(size=len(ea))
    ej[:-2:40] = 0.0
    return ea, eb, ej, n

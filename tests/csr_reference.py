"""Exact host reference and graph builders for the f64 CSR family (tests/test_csr_reference_host.py, tests/test_gpu_csr.py).

exact_energy: E = sum_e J_e s_a s_b - sum_i h_i s_i over the edge list as given, in exact rational arithmetic.

energy_bound: worst-case rounding error of any of the three f64 evaluations of that sum the project has.  Every one of them is
a sum of the terms +-J_e (or two halves +-J_e / 2 of it: a product with +-1 or 0.5 is exact) and +-h_i by f64 additions alone,
so the computed value is sum_k x_k prod_j (1 + d_j) with |d_j| <= u = 2^-53, one factor per addition the term passes through
(Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), and the error is at most gamma_m sum_k |x_k| with
gamma_m = m u / (1 - m u), m = the largest number of additions any term passes through, whatever their order:
  * device (gen_measure_kernel + gen_reduce_kernel, gen_resident_kernel): a coupling passes through at most max_degree additions
    of its row's field (the first one to 0.0), one subtraction of the bias, at most nvars - 1 additions among the site terms in
    any tree (padding adds exact zeros) and the addition of the self-loop constant: nvars + max_degree + 1; a self-loop passes
    through one addition per self-loop and that last one.  nvars + max_degree + 4 covers both when there are no more self-loops
    than sites, which every builder below keeps;
  * oracle (orc_energy): one running sum over the edge list and then the biases: a term passes through at most
    n_edges + nvars additions.
m is the larger of the two counts.  Derived, not measured; no test tightens it.

The builders use fixed numpy seeds.  Each returns a Graph; what its name promises (row lengths, class sizes, float-losslessness,
staged LDS bytes) is asserted on the host by tests/test_csr_reference_host.py.
"""
from collections import namedtuple
from fractions import Fraction

import numpy as np

Graph = namedtuple("Graph", "name ea eb ej nvars biases")

U = Fraction(1, 2 ** 53)
CLASS_PAD = 256          # colour classes are padded to whole 256-position blocks (greedy_colouring)
LDS_DEFAULT = 64 * 1024  # dynamic LDS a launch gets without hipFuncSetAttribute
LDS_MAX = 150 * 1024     # run_gen_resident's cap on the staged bytes


def _exact_sum(values, signs):
    """sum_k signs[k] * values[k] as a Fraction; values are floats (dyadic rationals), signs are +-1 integers."""
    ratios = [float(x).as_integer_ratio() for x in values]
    den = max([d for _, d in ratios], default=1)
    return Fraction(sum(int(s) * n * (den // d) for s, (n, d) in zip(signs, ratios)), den)


def exact_energy(ea, eb, ej, nvars, spins, biases=None):
    s = np.where(np.asarray(spins).astype(bool), 1, -1).astype(np.int64)
    assert s.shape == (nvars,)
    e = _exact_sum(ej, s[np.asarray(ea, dtype=np.int64)] * s[np.asarray(eb, dtype=np.int64)])
    if biases is not None:
        e -= _exact_sum(biases, s)
    return e


def energy_bound(ej, biases, nvars, max_degree):
    m = max(nvars + max_degree + 4, len(ej) + nvars)
    gamma = m * U / (1 - m * U)
    total = _exact_sum(np.abs(ej), np.ones(len(ej), dtype=np.int64))
    if biases is not None:
        total += _exact_sum(np.abs(biases), np.ones(len(biases), dtype=np.int64))
    return gamma * total


# ---- what the library derives from an edge list, restated for the host tests --------------------------------------------------
def row_lengths(g):
    """directed entries per site's CSR row: both ends of every bond, duplicates counted, self-loops left out (build_adjacency)"""
    off = g.ea != g.eb
    return np.bincount(np.concatenate([g.ea[off], g.eb[off]]).astype(np.int64), minlength=g.nvars)


def max_degree(g):
    return int(row_lengths(g).max()) if g.nvars else 0


def float_lossless(g):
    """graph.hip keeps f32 couplings when every coupling of the CSR (self-loops are not in it) survives the round trip"""
    w = g.ej[g.ea != g.eb]
    with np.errstate(over="ignore"):
        return bool(np.all(w.astype(np.float32).astype(np.float64) == w))


def class_sizes(oracle, g):
    """sites per colour class, in class order"""
    nc, colours, _ = oracle.gen_colouring(g.ea, g.eb, g.ej, g.nvars)
    return [int(c) for c in np.bincount(colours, minlength=nc)]


def n_positions(oracle, g):
    return sum((c + CLASS_PAD - 1) // CLASS_PAD * CLASS_PAD for c in class_sizes(oracle, g))


def gen_stage_words(n_pos, edges2, has_bias, w_bytes, stage):
    """general_types.hpp gen_stage_words: 32-bit LDS words of the resident kernel's STAGE 1 / 2"""
    off = (n_pos // 32 + 1) & ~1
    if stage == 1:
        if has_bias:
            off += 2 * n_pos
        off += edges2 * (w_bytes // 4)
        off = (off + 1) & ~1
    return off + (n_pos + 1) + n_pos + edges2


def stage_bytes(oracle, g, stage):
    edges2 = 2 * int(np.count_nonzero(g.ea != g.eb))
    return 4 * gen_stage_words(n_positions(oracle, g), edges2, g.biases is not None, 4 if float_lossless(g) else 8, stage)


# ---- couplings and biases -----------------------------------------------------------------------------------------------------
def couplings(kind, ea, eb, rng):
    """'float': multiples of 1/8 of both signs (f32 holds them); 'double': Gaussian (f32 does not); 'extreme': Gaussian plus one
    1e-50 and one 1e39 coupling on bonds of the CSR (f32 turns them into 0 and inf)."""
    m = len(ea)
    if kind == "float":
        return rng.integers(1, 17, m) / 8.0 * rng.choice([-1.0, 1.0], m)
    ej = rng.normal(size=m)
    if kind == "extreme":
        bonds = np.flatnonzero(ea != eb)
        ej[bonds[len(bonds) // 3]] = 1e-50
        ej[bonds[2 * len(bonds) // 3]] = 1e39
    else:
        assert kind == "double"
    return ej


def _edges(pairs):
    a = np.array([p[0] for p in pairs], dtype=np.uint64)
    b = np.array([p[1] for p in pairs], dtype=np.uint64)
    return a, b


def random_graph(kind, bias, n=300, m=900, seed=11):
    """n sites, m random bonds (self-loops and duplicate bonds come with them), all classes within one 256-position block"""
    rng = np.random.default_rng(seed)
    ea = rng.integers(0, n, m).astype(np.uint64)
    eb = rng.integers(0, n, m).astype(np.uint64)
    ea[:3], eb[:3] = [5, 5, 9], [5, 6, 9]          # two self-loops for sure
    ea[3:5], eb[3:5] = [5, 6], [6, 5]              # and one bond three times, in both orientations
    ej = couplings(kind, ea, eb, rng)
    return Graph(f"random{n}-{kind}-{'bias' if bias else 'nobias'}", ea, eb, ej, n, rng.normal(size=n) if bias else None)


def lds_graph(window, seed=12):
    """f64 couplings and biases, about degree 6: 'small' stages everything within the default 64 KB; 'mid' needs more than 64 KB
    for STAGE 1 and fits the 150 KB cap; 'big' is beyond the cap with STAGE 1 and needs more than 64 KB with STAGE 2."""
    n = {"small": 300, "mid": 1100, "big": 2300}[window]
    rng = np.random.default_rng(seed)
    ea = rng.integers(0, n, 3 * n).astype(np.uint64)
    eb = rng.integers(0, n, 3 * n).astype(np.uint64)
    return Graph(f"lds-{window}", ea, eb, couplings("double", ea, eb, rng), n, rng.normal(size=n))


def ring_graph(n, kind, bias=False, seed=13):
    """a ring of n sites (n even): two classes of n / 2 sites"""
    rng = np.random.default_rng(seed)
    ea = np.arange(n, dtype=np.uint64)
    eb = (ea + 1) % np.uint64(n)
    return Graph(f"ring{n}-{kind}", ea, eb, couplings(kind, ea, eb, rng), n, rng.normal(size=n) if bias else None)


def big_class_graph():
    """classes of 1300 sites: more positions than the 1024 threads of a resident workgroup"""
    return ring_graph(2600, "double", bias=True, seed=14)._replace(name="big-class")


def tiny_class_graph(seed=15):
    """40 sites in classes of fewer than 64: every wave but the first of a class holds padding alone"""
    rng = np.random.default_rng(seed)
    pairs = [(i, j) for i in range(40) for j in range(i + 1, 40) if (i % 4) != (j % 4) and rng.random() < 0.5]
    pairs += [(i, (i + 1) % 40) for i in range(40) if (i + 1) % 40 % 4 != i % 4]
    ea, eb = _edges(pairs)
    return Graph("tiny-class", ea, eb, couplings("double", ea, eb, rng), 40, rng.normal(size=40))


DEGREE_MIX = (7, 8, 9, 15, 16, 17, 40)


def degree_mix_graph(kind="double", seed=16):
    """Stars: three hubs for each row length of DEGREE_MIX (around the batch of 8 directed edges: 8k - 1, 8k, 8k + 1, and one
    long row), leaves of row length 1, isolated sites (row length 0).  The first hub of each length has one bond twice; some
    hubs, leaves and isolated sites carry self-loops.  The sites are shuffled, so hubs and leaves fall into both classes."""
    rng = np.random.default_rng(seed)
    pairs, nxt, hubs = [], 0, []
    for d in DEGREE_MIX:
        for copy in range(3):
            hub, nxt = nxt, nxt + 1
            hubs.append(hub)
            leaves = d - 1 if copy == 0 else d      # the doubled bond takes two entries of the row
            for k in range(leaves):
                pairs.append((hub, nxt + k) if k % 2 else (nxt + k, hub))
            if copy == 0:
                pairs.append((hub, nxt))                # the duplicate, in the other orientation
            nxt += leaves
    isolated = list(range(nxt, nxt + 6))
    nvars = nxt + 6
    pairs += [(h, h) for h in hubs[::4]] + [(isolated[0], isolated[0]), (isolated[1], isolated[1]), (hubs[0] + 1, hubs[0] + 1)]
    order = rng.permutation(len(pairs))
    relabel = rng.permutation(nvars)
    for label, hub in enumerate(hubs[1::3]):       # the second hub of each length takes a label below its leaves': class 0
        other = int(np.flatnonzero(relabel == label)[0])
        relabel[other], relabel[hub] = relabel[hub], label
    ea, eb = _edges([pairs[k] for k in order])
    ea, eb = relabel[ea.astype(np.int64)].astype(np.uint64), relabel[eb.astype(np.int64)].astype(np.uint64)
    return Graph(f"degree-mix-{kind}", ea, eb, couplings(kind, ea, eb, rng), nvars, rng.normal(size=nvars))


MULTI_CLASS_SIZES = [600, 65, 64, 1]


def multi_class_graph(kind, seed=17):
    """Not bipartite; the greedy colouring gives classes of 600, 65, 64 sites and 1 site: three 256-position blocks and three
    times one.  Sites 0..599 have no bonds among themselves; the next 65 see only those; the next 64 see one site of each
    earlier class (a triangle each); the last site sees one of every class."""
    rng = np.random.default_rng(seed)
    pairs = []
    c1 = range(600, 665)
    c2 = range(665, 729)
    for j in c1:
        pairs += [(j, int(q)) for q in rng.choice(600, 5, replace=False)]
    first_c0 = {j: next(b for a, b in pairs if a == j) for j in c1}
    for k in c2:
        j = 600 + (k - 665)
        pairs += [(int(first_c0[j]), k), (k, j)] + [(k, int(q)) for q in rng.choice(600, 3, replace=False)]
    pairs += [(729, 0), (600, 729), (729, 665)]
    ea, eb = _edges(pairs)
    return Graph(f"multi-class-{kind}", ea, eb, couplings(kind, ea, eb, rng), 730, rng.normal(size=730))


def one_block_graph(seed=18):
    """bipartite, 64 + 64 sites, degree 4: each class is ONE 256-position block with one wave of sites"""
    rng = np.random.default_rng(seed)
    pairs = [(2 * i, 2 * ((i + s) % 64) + 1) for i in range(64) for s in (0, 1, 5, 17)]
    ea, eb = _edges(pairs)
    return Graph("one-block", ea, eb, couplings("double", ea, eb, rng), 128, rng.normal(size=128))


def all_graphs():
    out = [random_graph(kind, bias) for kind in ("float", "extreme") for bias in (False, True)]
    out += [lds_graph(w) for w in ("small", "mid", "big")]
    out += [big_class_graph(), tiny_class_graph(), one_block_graph()]
    out += [f(kind) for f in (degree_mix_graph, multi_class_graph) for kind in ("float", "double")]
    out += [ring_graph(640, kind) for kind in ("float", "double")]
    return out


def oracle_trajectory(oracle, g, seed, betas):
    """uint8[T, nvars]: the configuration of oracle engine C after every timestep, from the random start of `seed`"""
    out = np.zeros((len(betas), g.nvars), dtype=np.uint8)
    state = None
    for k, beta in enumerate(betas):
        _, state = oracle.gen_run(g.ea, g.eb, g.ej, g.nvars, seed, [beta], biases=g.biases, t0=k,
                                  state=None if state is None else state.copy())
        out[k] = state
    return out

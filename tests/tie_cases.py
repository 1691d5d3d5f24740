"""The searched high-tie quads of tests/golden/tie_cases.json and the all-satisfied systems they are run on -- TEST
INFRASTRUCTURE shared by tests/test_tie_cases_host.py (CPU) and tests/test_gpu_ties.py.

A system is built from a gauge eps = +-1 per site: couplings J_ij = -|J| eps_i eps_j, start s = eps, fields h_i = h eps_i.  Every
bond is satisfied and every spin points along its field (eps = 1 everywhere: the ferromagnet from the all-up start; random eps:
a Mattis-gauged +-J glass), so the cost of a flip (S3's general form) is dE = 2|Jx| n_x + 2|Jy| n_y + 2 h with n the number of
EXISTING bonds of the site per direction -- one class for all spins but those on an open edge."""
import json
import os

import numpy as np

import tie_reference as TR

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tie_cases.json")


def load(domain, colour=0):
    """The fixture's records of one domain; colour = 1: the LATS records searched for the lattice's second colour."""
    with open(FIXTURE) as f:
        return [c for c in json.load(f)["cases"] if c["domain"] == domain and c["colour"] == colour]


def case_id(c):
    return f"{c['domain']}{'-c1' if c['colour'] else ''}-n{c['n_ties']}-Q{c['Q']}-{'hi' if c['t'] >> 32 else 'lo'}-{c['seed'] & 0xFFFF:04x}"


def most_ties(domain, pred=lambda c: True):
    """The fixture's case with the most ties among those that satisfy pred (the first of equals)."""
    return max((c for c in load(domain) if pred(c)), key=lambda c: c["n_ties"])


def beta_and_threshold(case, dE):
    """beta that puts the class of cost dE on the case's prefix value, with the host-side checks of the issue: the threshold's
    top 7 bits are v and its low word lies in the middle half, so that both outcomes of a tie occur."""
    beta = TR.beta_for(case["v"], dE)
    T = TR.threshold(beta, dE)
    assert T >> 32 == case["v"], (T >> 32, case["v"])
    assert 2 ** 30 <= (T & 0xFFFFFFFF) <= 3 * 2 ** 30, hex(T)
    return beta, T


# ---- checkerboard lattices (S2 / S3) ------------------------------------------------------------------------
MODES = {  # mode: (h, open, |Jy|)
    "ferro": (0.0, False, 1.0), "mattis": (0.0, False, 1.0), "field": (0.25, False, 1.0), "field_signs": (0.8, False, 1.0),
    "open": (0.0, True, 1.0), "open_field": (0.3, True, 1.0), "aniso": (0.0, False, 0.6)}


class LatticeSystem:
    def __init__(self, exact, W, H, mode):
        self.W, self.H, self.mode = W, H, mode
        self.h, self.open, self.jy = MODES[mode]
        gauged = mode in ("mattis", "field_signs")
        eps = np.random.default_rng(W * H).choice([-1.0, 1.0], W * H) if gauged else np.ones(W * H)
        ea, eb, _ = exact.square_lattice_edges(W, H, -1.0)
        ej = -eps[ea.astype(np.int64)] * eps[eb.astype(np.int64)]
        ej[1::2] *= self.jy                                              # (right, down) pairs: the vertical bonds
        self.jright, self.jdown = (ej[0::2] > 0).astype(np.uint8), (ej[1::2] > 0).astype(np.uint8)
        keep = np.ones(len(ea), dtype=bool)
        if self.open:
            keep &= ~((ea % W == W - 1) & (eb % W == 0)) & ~((ea // W == H - 1) & (eb // W == 0))
        self.ea, self.eb, self.ej = ea[keep], eb[keep], ej[keep]
        self.biases = self.h * eps if self.h else None
        self.field_neg = (eps < 0).astype(np.uint8) if mode == "field_signs" else None
        self.start = (eps > 0).astype(np.uint8)
        self.gauged = gauged

    def oracle_lat(self, O):
        return O.Lat(self.W, self.H, 1.0, 0, self.jright if self.gauged else None, self.jdown if self.gauged else None, field=self.h,
                     open_x=self.open, open_y=self.open, jabs_y=None if self.jy == 1.0 else self.jy, field_neg=self.field_neg)

    def dE(self, x, y):
        nx = 2 - (self.open and x in (0, self.W - 1))
        ny = 2 - (self.open and y in (0, self.H - 1))
        return 2.0 * 1.0 * nx + 2.0 * self.jy * ny + 2.0 * self.h

    def bulk_dE(self):
        return 2.0 * 1.0 * 2 + 2.0 * self.jy * 2 + 2.0 * self.h

    def quad_sites(self, Q, colour=0):
        """(x, y) of the spin at word q, bit b of quad Q of the colour's plane, at index 32 q + b (S2)."""
        wpr, out = self.W // 64, []
        for q in range(4):
            y, xw = divmod(4 * Q + q, wpr)
            out += [(2 * (32 * xw + b) + ((y + colour) & 1), y) for b in range(32)]
        return out

    def first_pass(self, case):
        """(beta, flips, ties, highest call) of the colour-0 pass over the case's quad from the all-satisfied start."""
        beta, _ = beta_and_threshold(case, self.bulk_dE())
        thresholds = [TR.threshold(beta, self.dE(x, y)) for x, y in self.quad_sites(case["Q"])]
        return (beta,) + TR.class_pass("LATS", case["seed"], case["t"], 0, case["Q"], thresholds, list(range(128)))

    def second_pass(self, case, spins_after):
        """(beta, flips, ties, highest call) of the colour-1 pass over the quad of a colour-1 case.  spins_after[H * W]: the
        configuration after the timestep, whose colour-0 sites are what the colour-1 pass saw; a colour-1 spin still sat on its
        gauge then, so a bond is satisfied iff the neighbour does too: dE = 2 |J| (sat - unsat) per direction + 2 h."""
        assert case["colour"] == 1 and not self.open
        beta, _ = beta_and_threshold(case, self.bulk_dE())
        on_gauge = (np.asarray(spins_after).reshape(self.H, self.W) == self.start.reshape(self.H, self.W))
        thresholds = []
        for x, y in self.quad_sites(case["Q"], colour=1):
            sx = int(on_gauge[y, (x + 1) % self.W]) + int(on_gauge[y, (x - 1) % self.W])
            sy = int(on_gauge[(y + 1) % self.H, x]) + int(on_gauge[(y - 1) % self.H, x])
            thresholds.append(TR.threshold(beta, 2.0 * 1.0 * (2 * sx - 2) + 2.0 * self.jy * (2 * sy - 2) + 2.0 * self.h))
        return (beta,) + TR.class_pass("LATS", case["seed"], case["t"], 1, case["Q"], thresholds, list(range(128)))

    def quad_bits(self, state_words, Q, colour=0):
        """The 128 spin bits of quad Q out of a replica's packed words (plane 0 then plane 1)."""
        base = colour * self.H * (self.W // 64) + 4 * Q
        return [(int(state_words[base + q]) >> b) & 1 for q in range(4) for b in range(32)]


# ---- replica-packed graphs (S6) ----------------------------------------------------------------------------
class PackedSystem:
    """An L^3 periodic cubic lattice, gauged or not, with some bonds removed: `cut` = [(site, k)]: the first k bonds from
    the site to higher-numbered neighbours are removed.  32 replicas, all started on the gauge (every bond satisfied)."""

    def __init__(self, exact, O, L=8, gauged=False, cut=()):
        n = L ** 3
        eps = np.random.default_rng(n).choice([-1.0, 1.0], n) if gauged else np.ones(n)
        ea, eb, _ = exact.cubic_lattice_edges(L, -1.0)
        keep = np.ones(len(ea), dtype=bool)
        for site, k in cut:
            lo = np.minimum(ea, eb)
            keep[np.flatnonzero((lo == site) & keep)[:k]] = False
        self.ea, self.eb = ea[keep], eb[keep]
        self.ej = -eps[self.ea.astype(np.int64)] * eps[self.eb.astype(np.int64)]
        self.nvars = n
        self.start = (eps > 0).astype(np.uint8)
        _, self.colours, self.pos = O.gen_colouring(self.ea, self.eb, self.ej, n)
        self.site_of = {int(p): i for i, p in enumerate(self.pos)}
        self.degree = np.bincount(np.concatenate([self.ea, self.eb]).astype(np.int64), minlength=n)

    def quad_site(self, p, q):
        return self.site_of[p + 64 * q]

    def first_pass(self, case, betas=None):
        """(beta, flips, ties, highest call) of class 0's pass over the case's position-quad; betas: one per replica bit
        (default: the case's beta for the degree-`bulk` sites on every replica)."""
        beta, _ = beta_and_threshold(case, 2.0 * 6)
        betas = [beta] * 32 if betas is None else betas
        thresholds = []
        for q in range(4):
            d = int(self.degree[self.quad_site(case["Q"], q)])
            thresholds += [TR.threshold(betas[b], 2.0 * d) for b in range(32)]
        return (beta,) + TR.class_pass("PKSW", case["seed"], case["t"], 0, case["Q"], thresholds, list(range(128)))

    def quad_bits(self, spins, p):
        """spins[32, nvars] of the group's replicas -> the 128 bits of the position-quad led by p at index 32 q + b."""
        return [int(spins[b][self.quad_site(p, q)]) for q in range(4) for b in range(32)]


def seeds_for(case, n):
    """n seeds, the case's first (replica 0: the lattice replica under test, the leader of the packed group)."""
    other = np.random.default_rng(case["seed"] & 0xFFFFFFFF).integers(0, 2 ** 63, size=n, dtype=np.uint64)
    other[0] = case["seed"]
    return other


def tie_rows(system, case, ties):
    """The degrees (rows of the packed threshold table) of the position-quad's words that hold ties."""
    return sorted({int(system.degree[system.quad_site(case["Q"], q)]) for q, _ in ties})


def diluted(exact, O, case):
    """The 8^3 ferromagnet with bonds cut at the sites of the case's position-quad that hold the fewest ties: the word with
    the fewest loses one bond (degree 5), the next one two (degree 4).  The colouring and the positions must not move."""
    full = PackedSystem(exact, O)
    per_word = [sum(1 for q, _ in case["ties"] if q == w) for w in range(4)]
    order = sorted(range(4), key=lambda w: (per_word[w], w))
    system = PackedSystem(exact, O, cut=[(full.quad_site(case["Q"], order[0]), 1), (full.quad_site(case["Q"], order[1]), 2)])
    np.testing.assert_array_equal(system.pos, full.pos)
    assert sorted(int(system.degree[system.quad_site(case["Q"], q)]) for q in range(4)) == [4, 5, 6, 6]
    return system


DILUTED_SEEDS = (0x746E, 0xA55F, 0xCC61)  # low 16 bits of the seeds of the cases that keep >= 9 ties over two rows when diluted


def diluted_cases(cases):
    out = [c for c in cases if c["seed"] & 0xFFFF in DILUTED_SEEDS]
    assert len(out) == len(DILUTED_SEEDS)
    return out

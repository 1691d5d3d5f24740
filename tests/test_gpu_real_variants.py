"""Every kernel variant of the replica-packed real-coupling family on forced shapes: the 48 rj_sweep_kernel<SLOTS, UB, PARTIAL,
HEAVY> and the 24 rj_measure_kernel<SLOTS, BIP, UP> (csrc/real_kernels.hpp), the grid-stride loops of both (`real_target_wgs`,
`real_measure_wgs`), a continued run.  Spins bit for bit against oracle engine E, energies bit for bit against engine E AND
against the exact Hamiltonian of the original f64 couplings (tests/real_reference.py) within its derived bound, magnetisations
from the spins.  tests/test_real_reference_host.py shows on the host that each graph has the shape its test is named for and
that engine E alone keeps the bound on these graphs.

Which test reaches what:
 * test_sweep_instantiations: SLOTS x {schedule: UB true, per-replica betas: UB false} x {whole: PARTIAL false; few, inside:
   PARTIAL true} x {light: HEAVY false, heavy: HEAVY true} = all 48 sweep kernels, on the two-colour graph with fields;
 * test_measure_instantiations: SLOTS x {bipartite: BIP true, odd-cycle: BIP false} x {energies(), per-step energies: UP
   false; magnetisations(): UP true} = all 24 measurement kernels, each with and without fields and heavy sites;
 * the stride and continuation tests run a subset of the same kernels through their other loop counts.

Shapes the layout rules out: colour classes are padded to 256 positions, so no block of the measurement holds sites of two
classes and none is cut by the end of the scan (`base < scan_end` holds for whole blocks only); a class never has fewer
positions than a workgroup has threads.  A group that a container owns in part is decided in whole Philox calls (four replica
bits): the foreign bits checked for being untouched are those of the calls that are not drawn.

What no eligible graph can show: the `y >>= sy` of a heavy site.  rj_eligible admits a heavy site only when one term holds 3/4 of
its weight F, so |X| >= F / 2 >= 2^28 of the site's own quanta, while the bound y stays below Lambda_q(u) < 2^28 unless
u < 2^16: with or without the shift the decision is the sign of X, but for about 2^-16 of the uphill attempts at heavy sites --
a few thousand per case here.  The spec's shift is tested on the host (test_real_path_host.py, oracle.rj_accept)."""
import math
from fractions import Fraction

import numpy as np
import pytest

import real_reference as RR

pytestmark = pytest.mark.gpu

SCHEDULE = [0.0, -0.3, 30.0, 0.7]     # per step, in units of 1 / the typical coupling: infinite temperature, a negative beta, frozen
SEED_GEN = 201
RATIOS = {}                           # measurement kernel -> largest |E_gpu - E_exact| / energy_bound seen
_TRAJ, _EXACT, _BOUND, _GRAPHS, _RUNS = {}, {}, {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def report_ratios():
    yield
    for kernel, ratio in sorted(RATIOS.items()):
        print(f"\n[real] largest |E_gpu - E_exact| / energy_bound, {kernel}: {ratio:.4f}")


def graph(kind, slots, bias, heavy):
    key = (kind, slots, bias, heavy)
    if key not in _GRAPHS:
        _GRAPHS[key] = (RR.bipartite_circulant if kind == "bipartite" else RR.odd_cycle)(slots, bias, heavy)
    return _GRAPHS[key]


def replica_betas(R, scale):
    """a geomspace from 1e-7 to 3 (a heavy site's shift lies on both sides of the acceptance scale's within one launch), and
    0, a negative and a large beta at replicas 1, R / 2 and R - 2"""
    betas = list(np.geomspace(1e-7, 3.0, R - 3))
    for at, beta in ((1, 0.0), (R // 2, -0.3), (R - 2, 30.0)):
        betas.insert(at, beta)
    return np.array(betas) / scale


def schedule(g, T):
    return [b / g.scale for b in SCHEDULE[:T]]


def exact(g):
    if g.name not in _EXACT:
        _EXACT[g.name] = RR.Exact(g.ea, g.eb, g.ej, g.nvars, g.biases)
        _BOUND[g.name] = RR.energy_bound(g.ea, g.eb, g.ej, g.nvars, g.biases)
    return _EXACT[g.name], _BOUND[g.name]


def trajectory(oracle, g, seeds, T, mode):
    """engine E's configurations and energies after every step, and the exact energies of those configurations: once per case"""
    R = len(seeds)
    key = (g.name, int(seeds[0]), R, T, mode)
    if key not in _TRAJ:
        kw = dict(betas=schedule(g, T)) if mode == "schedule" else dict(beta_replica=replica_betas(R, g.scale))
        spins, eps = RR.oracle_trajectory(oracle, g, seeds, T, **kw)
        ex, _ = exact(g)
        e_exact = [[ex.energy(spins[t, r]) for t in range(T)] for r in range(R)]
        spins.setflags(write=False)
        eps.setflags(write=False)
        _TRAJ[key] = (spins, eps, e_exact)
    return _TRAJ[key]


def measure_kernel(g_handle, slots, up=False):
    return f"rj_measure_kernel<{slots}, {'true' if g_handle.info.n_colours == 2 else 'false'}, {'true' if up else 'false'}>"


def check_energy(kernel, g, e_gpu, e_exact):
    _, bound = exact(g)
    assert math.isfinite(e_gpu)
    err = abs(Fraction(float(e_gpu)) - e_exact)
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), float(err / bound))
    assert err <= bound, (kernel, g.name, float(err), float(bound))


class Run:
    """one container on the real-coupling family: T steps under `options`, with a schedule or per-replica betas; `rng` = (lo, hi):
    the shard [lo, hi) of the seeds"""

    def __init__(self, capi, g, slots, seeds, T, mode, options=None, rng=None, keep=False):
        self.g, self.slots, self.T, self.mode = g, slots, T, mode
        self.lo, self.hi = (0, len(seeds)) if rng is None else rng
        handle = capi.Graph(g.ea, g.eb, g.ej, nvars=g.nvars, biases=g.biases, stable_path=True)
        colours = RR.greedy_colours(g)
        assert handle.info.real_slots == slots and handle.info.n_colours == int(colours.max()) + 1
        assert handle.info.real_energy_log2 == RR.energy_log2(g.ea, g.eb, g.ej, g.nvars, g.biases)
        assert (handle.info.real_heavy_sites > 0) == g.name.endswith("heavy")
        st = capi.States(handle, seeds, replica_range=rng)
        assert st.family == "packed_real" and st.count == self.hi - self.lo
        for name, value in (options or {}).items():
            st.set_option(name, value)
        self.kernel = measure_kernel(handle, slots)
        self.n_pos = 256 * sum((c + 255) // 256 for c in RR.class_sizes(colours))
        self.raw_before = st.raw_state()
        if mode == "per_replica":
            st.set_betas(replica_betas(len(seeds), g.scale)[self.lo:self.hi])
            self.eps = st.do_time_steps(T, per_step_energies=True)
        else:
            self.eps = st.do_time_steps(T, schedule(g, T), per_step_energies=True)
        self.raw = st.raw_state()
        self.spins = st.states().astype(np.uint8)
        self.energies = st.energies()
        self.mags = st.magnetisations()
        if keep:
            self.st, self.handle = st, handle
        else:
            st.close()
            handle.close()

    def close(self):
        self.st.close()
        self.handle.close()

    def same_as(self, other, lo=0):
        """the same bits as rows lo .. of `other`"""
        rows = slice(lo, lo + len(self.spins))
        assert np.array_equal(self.spins, other.spins[rows])
        assert np.array_equal(self.energies.view(np.uint64), other.energies[rows].view(np.uint64))
        assert np.array_equal(self.eps.view(np.uint64), other.eps[rows].view(np.uint64))
        assert np.array_equal(self.mags, other.mags[rows])

    def check(self, oracle, seeds, groups=None):
        """against engine E and the exact Hamiltonian; groups: only these replica groups (the oracle gets their seeds alone)"""
        g, T = self.g, self.T
        if groups is None:
            spins, eps, e_exact = trajectory(oracle, g, seeds, T, self.mode)
            rows = [(r, r) for r in range(self.lo, self.hi)]
            parts = [(spins, eps, e_exact, rows)]
        else:
            parts = []
            for grp in groups:
                sub = seeds[32 * grp:32 * grp + 32]
                spins, eps = RR.oracle_trajectory(oracle, g, sub, T, betas=schedule(g, T))
                ex, _ = exact(g)
                e_exact = [[ex.energy(spins[t, r]) for t in range(T)] for r in range(0, len(sub), 11)]
                parts.append((spins, eps, e_exact, [(32 * grp + r, r) for r in range(len(sub))]))
        for spins, eps, e_exact, rows in parts:
            for r_gpu, r_ref in rows:
                k = r_gpu - self.lo
                assert np.array_equal(self.spins[k], spins[-1, r_ref]), (g.name, r_gpu)
                assert np.array_equal(self.eps[k].view(np.uint64), eps[r_ref].view(np.uint64)), (g.name, r_gpu)
                assert self.energies[k] == eps[r_ref, -1]
                assert self.mags[k] == 2 * int(np.count_nonzero(self.spins[k])) - g.nvars
                if groups is None or r_ref % 11 == 0:
                    ee = e_exact[r_ref] if groups is None else e_exact[r_ref // 11]
                    for t in range(T):
                        check_energy(self.kernel, g, self.eps[k, t], ee[t])

    def foreign_bits_untouched(self, masks):
        """masks[group]: replica bits of that group whose Philox calls this container does not draw"""
        before, after = self.raw_before.reshape(-1, self.n_pos), self.raw.reshape(-1, self.n_pos)
        assert before.shape[0] == len(masks)
        for grp, mask in enumerate(masks):
            assert np.any(before[grp] & np.uint32(mask))                       # a random start fills whole words
            assert np.array_equal(before[grp] & np.uint32(mask), after[grp] & np.uint32(mask)), grp


def cached_run(capi, oracle, key, make):
    """a run other cases compare themselves with, checked against the oracle when it is made"""
    if key not in _RUNS:
        _RUNS[key] = make()
    return _RUNS[key]


# ---- sweep kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heavy", [False, True], ids=["light", "heavy"])
@pytest.mark.parametrize("owned", ["whole", "few", "inside"])
@pytest.mark.parametrize("mode", ["schedule", "per_replica"])
@pytest.mark.parametrize("slots", RR.SLOT_COUNTS)
def test_sweep_instantiations(capi, oracle, slots, mode, owned, heavy):
    """rj_sweep_kernel<slots, UB, PARTIAL, HEAVY> on the two-colour graph with fields, T = 4.  whole: 64 replicas.  few: 5
    replicas, q_hi = 2.  inside: the shard [13, 45) of 64: q_lo = 3 in its first group, q_hi = 4 in its second; equal to rows
    13 .. 44 of the whole run."""
    g = graph("bipartite", slots, True, heavy)
    T = 4
    if owned == "few":
        seeds = capi.make_seeds(SEED_GEN, 5)
        run = Run(capi, g, slots, seeds, T, mode)
        run.check(oracle, seeds)
        run.foreign_bits_untouched([0xFFFFFF00])
        return
    seeds = capi.make_seeds(SEED_GEN, 64)
    whole = cached_run(capi, oracle, (g.name, mode, "whole"), lambda: Run(capi, g, slots, seeds, T, mode))
    if owned == "whole":
        whole.check(oracle, seeds)
    else:
        shard = Run(capi, g, slots, seeds, T, mode, rng=(13, 45))
        shard.check(oracle, seeds)
        shard.same_as(whole, lo=13)
        # bit 12 of the first group and bits 13 .. 15 of the second share a Philox call with owned bits and are decided with them
        shard.foreign_bits_untouched([0x00000FFF, 0xFFFF0000])


# ---- measurement kernels ----------------------------------------------------------------------------------------------------------
def by_hand(g, pattern):
    """the energy of all up (sum J - sum h) and of the parity pattern (even sites up: every bond between the parities counts -J)"""
    if pattern == "up":
        e = sum(Fraction(float(j)) for j in g.ej)
        return e - (sum(Fraction(float(h)) for h in g.biases) if g.biases is not None else 0)
    e = sum(Fraction(float(j)) * (1 if (int(a) + int(b)) % 2 == 0 else -1) for a, b, j in zip(g.ea, g.eb, g.ej))
    if g.biases is not None:
        e -= sum(Fraction(float(h)) * (1 if i % 2 == 0 else -1) for i, h in enumerate(g.biases))
    return e


@pytest.mark.parametrize("heavy", [False, True], ids=["light", "heavy"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("kind", ["bipartite", "odd-cycle"])
@pytest.mark.parametrize("slots", RR.SLOT_COUNTS)
def test_measure_instantiations(capi, oracle, slots, kind, bias, heavy):
    """rj_measure_kernel<slots, BIP, UP>: energies() and the energies of 3 steps (UP false, hi and lo level), magnetisations()
    (UP true), 37 replicas.  Two colours without fields: the scan ends with class 0; with fields: class 1 through the bias-only
    gather (a site without bonds there: the own-bit nibble alone).  Then replica 0 all up and replica 1 in the parity pattern:
    their energies are known by hand."""
    g = graph(kind, slots, bias, heavy)
    seeds = capi.make_seeds(SEED_GEN + 1, 37)
    run = Run(capi, g, slots, seeds, 3, "schedule", keep=True)
    try:
        assert (run.handle.info.n_colours == 2) == (kind == "bipartite")
        run.check(oracle, seeds)
        up, parity = np.ones(g.nvars, dtype=np.uint8), (np.arange(g.nvars) % 2 == 0).astype(np.uint8)
        run.st.set_state(0, up)
        run.st.set_state(1, parity)
        e, m = run.st.energies(), run.st.magnetisations()
        assert np.array_equal(e[2:].view(np.uint64), run.energies[2:].view(np.uint64)) and np.array_equal(m[2:], run.mags[2:])
        assert m[0] == g.nvars and m[1] == 0
        for r, spins, pattern in ((0, up, "up"), (1, parity, "parity")):
            assert e[r] == oracle.rj_energy(g.ea, g.eb, g.ej, g.nvars, spins, g.biases)
            want = by_hand(g, pattern)
            assert want == exact(g)[0].energy(spins)
            check_energy(run.kernel, g, e[r], want)
    finally:
        run.close()


# ---- grid-stride loops ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("owned", ["whole", "few"])
@pytest.mark.parametrize("mode", ["schedule", "per_replica"])
@pytest.mark.parametrize("slots", [4, 15, 31])
def test_sweep_stride(capi, oracle, slots, mode, owned):
    """`real_target_wgs` = 1 (the option path does not clamp): ONE workgroup per group walks the 3 / 6 / 11 blocks of a class,
    `base += gridDim.x * THREADS`; the default rule gives every block a workgroup.  Heavy sites, fields; 64 and 5 replicas."""
    g = graph("bipartite", slots, True, True)
    seeds = capi.make_seeds(SEED_GEN, 64 if owned == "whole" else 5)
    forced = Run(capi, g, slots, seeds, 4, mode, options={"real_target_wgs": 1})
    forced.check(oracle, seeds)
    forced.same_as(Run(capi, g, slots, seeds, 4, mode))
    if owned == "few":
        forced.foreign_bits_untouched([0xFFFFFF00])


@pytest.mark.parametrize("kind", ["bipartite", "odd-cycle"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("slots", [4, 15, 31])
def test_measure_stride(capi, oracle, slots, bias, kind):
    """`real_measure_wgs` = 1 and = 3 against the default (every block a workgroup of its own at this size): 20 replicas are one
    group, so the scan's 3 .. 28 blocks are walked by 1 and by 3 workgroups, `base += gridDim.x * THREADS`, an uneven share
    where 3 does not divide them.  energies() and per-step energies (UP false), magnetisations() (UP true): the same bits."""
    g = graph(kind, slots, bias, True)
    seeds = capi.make_seeds(SEED_GEN + 2, 20)
    default = Run(capi, g, slots, seeds, 3, "schedule")
    default.check(oracle, seeds)
    for wgs in (1, 3):
        Run(capi, g, slots, seeds, 3, "schedule", options={"real_measure_wgs": wgs}).same_as(default)


def test_many_groups_default_rule(capi, oracle):
    """96 groups (3072 replicas) at 31 slots under the default rules: the measurement's share of the resident workgroups per
    group is smaller than the scan's 24 blocks of 64 threads.  Groups 0, 47 and 95 against engine E, every 11th replica of
    them against the exact Hamiltonian; all magnetisations from the spins."""
    g = graph("bipartite", 31, True, True)
    seeds = capi.make_seeds(SEED_GEN + 3, 3072)
    run = Run(capi, g, 31, seeds, 2, "schedule")
    run.check(oracle, seeds, groups=(0, 47, 95))
    assert np.array_equal(run.mags, 2 * run.spins.sum(axis=1, dtype=np.int64) - g.nvars)


# ---- a continued run ----------------------------------------------------------------------------------------------------------------
def test_continuation_with_set_state(capi, oracle):
    """23 slots, heavy sites, fields: two steps, set_state on replica 5, two more steps -- the timestep counter and the heavy
    tables in one sequence, against rj_run(..., t0 = 2) continued from the same configurations"""
    g = graph("bipartite", 23, True, True)
    seeds = capi.make_seeds(SEED_GEN + 4, 37)
    betas = schedule(g, 4)
    run = Run(capi, g, 23, seeds, 2, "schedule", keep=True)
    try:
        run.check(oracle, seeds)
        pattern = (np.arange(g.nvars) % 3 == 0).astype(np.uint8)
        run.st.set_state(5, pattern)
        assert run.st.timestep == 2
        eps = run.st.do_time_steps(2, betas[2:], per_step_energies=True)
        states = np.array(trajectory(oracle, g, seeds, 2, "schedule")[0][-1])
        states[5] = pattern
        spins, eps_ref = RR.oracle_trajectory(oracle, g, seeds, 2, betas=betas[2:], t0=2, states=states)
        got = run.st.states().astype(np.uint8)
        assert np.array_equal(got, spins[-1, :37])
        assert np.array_equal(eps.view(np.uint64), eps_ref.view(np.uint64))
        assert np.array_equal(run.st.energies().view(np.uint64), eps_ref[:, -1].copy().view(np.uint64))
        assert np.array_equal(run.st.magnetisations(), 2 * got.sum(axis=1, dtype=np.int64) - g.nvars)
        ex, _ = exact(g)
        for r in (0, 5, 36):
            for t in range(2):
                check_energy(run.kernel, g, eps[r, t], ex.energy(spins[t, r]))
    finally:
        run.close()

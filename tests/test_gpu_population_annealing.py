"""Population annealing on the device: the resampling step of every served family against the restatement of
tests/pa_reference.py (bit-exact: packed words, energies, step record, families, after every stage), caller-supplied source
tables, the composition with isoenergetic cluster moves, the refusals, and the free-energy estimate of
Lattice.run_population_annealing against Kaufman's exact partition function."""
import numpy as np
import pytest

import icm_reference as ICM
import pa_reference as PA
import packed_icm_reference as IR

pytestmark = pytest.mark.gpu

SEED = 0x0123456789ABCDEF
BETA = 0.3


# ---- the two kinds of population: a device container and its restatement, driven through one interface ----------------------
class _Board:
    """Checkerboard container + one oracle.Lat state per replica."""

    def __init__(self, capi, exact, W, H, glass, R, k=0, seed_gen=11):
        self.W, self.H, self.k = W, H, k
        ea, eb, ej = exact.square_lattice_edges(W, H, -1.0, np.random.default_rng(W + H) if glass else None)
        self.jr, self.jd = ICM.couplings(W, H, ej)
        self.lat = ICM.make_lat(W, H, self.jr, self.jd)
        self.seeds = capi.make_seeds(seed_gen, R)
        self.g = capi.Graph(ea, eb, ej, device=0)
        self.st = capi.States(self.g, self.seeds)
        assert self.st.family == "checkerboard"
        if k:
            self.st.set_icm_every(k)
        self.ref = [self.lat.init(s) for s in self.seeds]
        self.t = 0

    def sweeps(self, n, beta, per_step_energies=False):
        out = self.st.do_time_steps(n, beta, per_step_energies=per_step_energies)
        self.advance(n, beta)
        return out

    def advance(self, n, beta):
        if self.k:
            spins = [self.lat.unpack(w) for w in self.ref]
            spins, _, _ = ICM.run_replicas(self.W, self.H, self.jr, self.jd, list(self.seeds), spins, self.t, [beta] * n, self.k)
            self.ref = [self.lat.pack(s.ravel()) for s in spins]
        else:
            for w, s in zip(self.ref, self.seeds):
                for t in range(self.t, self.t + n):
                    self.lat.sweep(w, s, t, beta)
        self.t += n

    def energies(self):
        """The energies of the restatement's configurations: no call into the library."""
        return np.array([self.lat.energy_mag(w)[0] for w in self.ref])

    def snapshot(self):
        """The raw device words before a gather: gather() then checks the words after it against the restatement's row gather."""
        self.raw = self.st.raw_state().reshape(len(self.seeds), -1)

    def gather(self, src):
        assert np.array_equal(self.st.raw_state().reshape(self.raw.shape), PA.row_gather(self.raw, src)), "raw words differ"
        self.ref = [w.copy() for w in PA.row_gather(np.stack(self.ref), src)]

    def compare(self):
        assert np.array_equal(self.st.packed(), np.stack(self.ref)), "packed words differ"
        e = self.st.energies()
        assert np.array_equal(e, [self.lat.energy_mag(w)[0] for w in self.ref])
        assert self.st.timestep == self.t
        return e


class _Packed:
    """Replica-packed container of either family + the slots x sites array of the packed restatements (unowned slots included)."""

    def __init__(self, capi, G, R, real=False, biases=None, k=0, seed_gen=12):
        self.G, self.real, self.biases, self.k = G, real, biases, k
        self.seeds = capi.make_seeds(seed_gen, R)
        if real:
            self.g = capi.Graph(G.ea, G.eb, G.ej, nvars=G.nvars, biases=biases, stable_path=True)
        else:
            self.g = capi.Graph(G.ea, G.eb, G.ej, nvars=G.nvars, force_general=True)
        self.st = capi.States(self.g, self.seeds)
        assert self.st.family == ("packed_real" if real else "packed_bitsliced")
        if k:
            self.st.set_icm_every(k)
        self.ref, _, _ = IR.run(G, self.seeds, 0, 0, betas=[], biases=biases, real=real)
        self.e_ref = None
        self.t = 0

    def sweeps(self, n, beta, per_step_energies=False):
        out = self.st.do_time_steps(n, beta, per_step_energies=per_step_energies)
        self.ref, e, _ = IR.run(self.G, self.seeds, n, self.k, betas=[beta] * n, states=self.ref, t0=self.t, biases=self.biases, real=self.real)
        self.e_ref = e[:, -1]
        self.t += n
        return out

    def snapshot(self):
        """The raw device words u32[groups][n_pos] before a gather, padding positions and unowned bits included."""
        self.raw = self.st.raw_state().reshape(-1, self.G.n_pos)
        assert self.raw.shape[0] == (len(self.seeds) + 31) // 32

    def gather(self, src):
        # word for word: every bit of every word, owned or not, real position or padding
        padding = np.ones(self.G.n_pos, dtype=bool)
        padding[self.G.pos] = False
        after = self.st.raw_state().reshape(self.raw.shape)
        assert np.array_equal(after, PA.bit_gather(self.raw, src, padding)), "raw words differ"
        self.ref = PA.gather_spins(self.G, self.ref, src)
        self.e_ref = None

    def compare(self):
        R = len(self.seeds)
        assert np.array_equal(self.st.packed(), np.stack([self.G.pack(self.ref[r]) for r in range(R)])), "packed words differ"
        e = self.st.energies()
        if self.e_ref is None:
            energy = (lambda s: self.oracle_energy(s))
            self.e_ref = np.array([energy(self.ref[r]) for r in range(R)])
        assert np.array_equal(e, self.e_ref)
        assert self.st.timestep == self.t
        return e

    def energies(self):
        """The energies of the restatement's configurations: no call into the library."""
        if self.e_ref is None:
            self.e_ref = np.array([self.oracle_energy(self.ref[r]) for r in range(len(self.seeds))])
        return self.e_ref

    def oracle_energy(self, spins):
        from oracle import oracle as O
        return O.rj_energy(self.G.ea, self.G.eb, self.G.ej, self.G.nvars, spins, self.biases) if self.real else self.G.energy(spins)


def _cubic(exact, L, glass):
    ea, eb, ej = IR.cubic_glass(exact, L)
    return IR.Graph(ea, eb, ej if glass else np.full(len(ej), -1.0), L ** 3)


def _gaussian_64x8(exact):
    ea, eb, _ = exact.square_lattice_edges(64, 8, -1.0)
    rng = np.random.default_rng(648)
    return IR.Graph(ea, eb, rng.normal(size=len(ea)), 512), rng.normal(size=512)


def _make(capi, exact, monkeypatch, kind, R, k=0):
    if kind[0] == "board":
        _, W, H, glass = kind
        return _Board(capi, exact, W, H, glass, R, k=k)
    if kind[0] == "strip":
        monkeypatch.setenv("ISINGMC_STRIP", "1")
        return _Board(capi, exact, 1024, 128, False, R, k=k)
    monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
    if kind[0] == "cubic":
        return _Packed(capi, _cubic(exact, kind[1], kind[2]), R, k=k)
    G, h = _gaussian_64x8(exact)
    return _Packed(capi, G, R, real=True, biases=h, k=k)


def _resample_and_compare(P, e, dbeta, step, families):
    """pa_resample on the device against the restatement fed with the energies the library itself returned."""
    R = len(e)
    want = PA.sources(SEED, step, e, dbeta)
    P.snapshot()
    P.st.pa_resample(dbeta, SEED, step)
    got = P.st.pa_last()
    assert np.array_equal(got["src"], want["src"])
    assert got["sum"] == want["sum"] and got["eref"] == want["eref"] and got["distinct"] == want["distinct"]
    bound = R * 2.0 ** -52 * np.abs(e).mean()   # the worst case of any summation order
    print(f"mean energy {got['mean_energy']!r} numpy {want['mean_energy']!r} bound {bound:.3e}")
    assert abs(got["mean_energy"] - want["mean_energy"]) <= bound
    P.gather(want["src"])
    families = families[want["src"]]
    assert np.array_equal(P.st.pa_families(), families)
    P.compare()   # the timestep counter has not moved
    return want, families


CASES = ([(("board", 64, 4, glass), R) for glass in (False, True) for R in (1, 2, 37)] +
         [(("board", 128, 64, glass), R) for glass in (False, True) for R in (1, 2, 37)] +
         [(("strip",), 8)] +
         [(("cubic", 6, True), R) for R in (32, 33, 70)] + [(("cubic", 8, False), R) for R in (32, 33, 70)] +
         [(("real",), 45)])
TABLE_CASES = ([(("board", W, H, glass), 37) for W, H in ((64, 4), (128, 64)) for glass in (False, True)] +
               [(("strip",), 8), (("cubic", 6, True), 70), (("cubic", 8, False), 70), (("real",), 70)])
FAMILIES = [(("board", 64, 4, True), 37), (("strip",), 8), (("cubic", 6, True), 70), (("cubic", 8, False), 70), (("real",), 45)]


def _id(case):
    return "-".join(str(x) for x in case[0]) + f"-R{case[1]}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_resampling_between_sweeps(capi, exact, monkeypatch, case):
    kind, R = case
    P = _make(capi, exact, monkeypatch, kind, R)
    P.compare()
    P.sweeps(3, BETA)
    e = P.compare()
    fam = np.arange(R, dtype=np.uint32)
    assert np.array_equal(P.st.pa_families(), fam)
    _, fam = _resample_and_compare(P, e, 0.05, 1, fam)
    P.sweeps(2, BETA + 0.05)
    e = P.compare()
    _, fam = _resample_and_compare(P, e, 0.05, 2, fam)   # a second step: the buffers have swapped once already
    P.sweeps(2, BETA + 0.1)
    P.compare()
    P.st.pa_reset_families()
    assert np.array_equal(P.st.pa_families(), np.arange(R))


@pytest.mark.parametrize("case", FAMILIES, ids=_id)
def test_zero_step_is_the_identity_and_a_large_step_keeps_few(capi, exact, monkeypatch, case):
    kind, R = case
    P = _make(capi, exact, monkeypatch, kind, R)
    P.sweeps(3, BETA)
    e = P.compare()
    before = P.st.packed()
    fam = np.arange(R, dtype=np.uint32)
    want, fam = _resample_and_compare(P, e, 0.0, 7, fam)
    assert np.array_equal(want["src"], np.arange(R)) and want["distinct"] == R and want["sum"] == R << 32
    assert np.array_equal(P.st.packed(), before)
    P.sweeps(1, BETA)
    e = P.compare()
    # a step that leaves fewer than R / 8 sources (one, for the strip case's R = 8) and, on the packed shapes, gives one replica
    # more than 32 copies: dbeta (spread of E) = 20, doubled until the RESTATEMENT's table says so
    packed = kind[0] in ("cubic", "real")
    for factor in (20.0, 40.0, 80.0, 160.0, 320.0, 640.0):
        dbeta = factor / (e.max() - e.min())
        table = PA.sources(SEED, 8, e, dbeta)
        counts = np.bincount(table["src"], minlength=R)
        if (table["distinct"] < R / 8 or table["distinct"] == 1) and (not packed or counts.max() > 32):
            break
    else:
        pytest.fail("no step concentrates this population")
    want, fam = _resample_and_compare(P, e, dbeta, 8, fam)
    print(f"dbeta {dbeta:.4f} (factor {factor}): {want['distinct']} distinct sources of {R}, the largest family {counts.max()}")
    P.sweeps(2, BETA)
    P.compare()


def _tables(R, rng):
    return {"reversed": np.arange(R)[::-1].copy(), "repeats": rng.integers(0, R, R)}


@pytest.mark.parametrize("case", TABLE_CASES, ids=_id)
def test_caller_supplied_tables(capi, exact, monkeypatch, case):
    kind, R = case
    P = _make(capi, exact, monkeypatch, kind, R)
    P.sweeps(1, BETA)
    fam = np.arange(R, dtype=np.uint32)
    for name, src in _tables(R, np.random.default_rng(R)).items():
        P.snapshot()
        P.st.pa_apply_sources(src)
        P.gather(src)
        fam = fam[src]
        P.compare()
        assert np.array_equal(P.st.pa_families(), fam), name
        P.sweeps(1, BETA)   # bits nobody owns and padding take part in the bit-sliced sweep: a damaged word shows here
        P.compare()
    with pytest.raises(ValueError, match="not a replica"):
        P.st.pa_apply_sources(np.full(R, R))
    P.compare()


def test_one_target_group_fed_by_32_source_groups(capi, exact, monkeypatch):
    R = 1056
    P = _make(capi, exact, monkeypatch, ("cubic", 6, True), R)
    rng = np.random.default_rng(33)
    src = rng.integers(0, R, R)
    src[:32] = 32 * (1 + np.arange(32)) + rng.permutation(32)   # bit b of group 0 <- some bit of group b + 1
    P.snapshot()
    P.st.pa_apply_sources(src)
    P.gather(src)
    P.compare()
    P.sweeps(1, BETA)
    P.compare()


@pytest.mark.parametrize("case", [(("board", 64, 4, True), 6), (("cubic", 6, True), 70), (("real",), 45)], ids=_id)
def test_composition_with_isoenergetic_cluster_moves(capi, exact, monkeypatch, case):
    kind, R = case
    P = _make(capi, exact, monkeypatch, kind, R, k=2)
    P.sweeps(3, BETA)   # sweep, move, sweep
    e = P.compare()
    _resample_and_compare(P, e, 0.05, 1, np.arange(R, dtype=np.uint32))
    assert P.st.timestep == 3
    P.sweeps(4, BETA + 0.05)   # move, sweep, move, sweep
    P.compare()


def test_refusals_leave_the_container_untouched(capi, exact, monkeypatch):
    ea, eb, ej = exact.square_lattice_edges(64, 4, -1.0)
    seeds = capi.make_seeds(3, 8)

    def refused(st, match):
        before = st.packed() if st.count else None
        with pytest.raises(ValueError, match=match):
            st.pa_resample(0.05, SEED, 1)
        with pytest.raises(ValueError, match=match):
            st.pa_apply_sources(np.arange(st.count))
        with pytest.raises(ValueError, match="no resampling"):
            st.pa_last()
        if st.count:
            assert np.array_equal(st.packed(), before)

    g = capi.Graph(ea, eb, ej, device=0)
    st = capi.States(g, seeds)
    with pytest.raises(ValueError, match="finite"):
        st.pa_resample(float("nan"), SEED, 1)
    with pytest.raises(ValueError, match="finite"):
        st.pa_resample(float("inf"), SEED, 1)
    st.pt_attach(np.linspace(0.1, 0.4, 8), 0, 8, 1, 7)
    refused(st, "ladder")
    st.pt_detach()
    st.set_betas(np.linspace(0.1, 0.4, 8))
    refused(st, "per-replica betas")
    st.set_betas(None)
    refused(capi.States(g, seeds, replica_range=(0, 4)), "shard")
    refused(capi.States(g, seeds, replica_range=(4, 8)), "shard")
    refused(capi.States(g, seeds[:0]), "no replica")
    fa, fb, fj = exact.square_lattice_edges(256, 16, -1.0)
    field = capi.Graph(fa, fb, fj, biases=np.full(256 * 16, 0.25), device=0)
    assert field.kind == capi.KIND_LATTICE2D and field.info.fast_path == 1
    refused(capi.States(field, seeds), "fields")
    keep = np.ones(len(fa), dtype=bool)
    keep[2 * np.arange(255, 256 * 16, 256)] = False   # the right bonds of the last column: open in x
    opened = capi.Graph(fa[keep], fb[keep], fj[keep], nvars=256 * 16, device=0)
    assert opened.kind == capi.KIND_LATTICE2D and opened.info.fast_path == 2
    refused(capi.States(opened, seeds), "open boundaries")
    G = _cubic(exact, 6, True)
    csr = capi.States(capi.Graph(G.ea, G.eb, G.ej, nvars=G.nvars), seeds[:2])
    assert csr.family == "csr_f64"
    refused(csr, "f64 CSR")
    # and the container that refused everything above still resamples
    st.do_time_steps(2, BETA)
    st.pa_resample(0.05, SEED, 1)
    assert st.pa_last()["sum"] >= 1 << 32


# ---- physics ---------------------------------------------------------------------------------------------------------------
PA_W, PA_H, PA_POP, PA_SWEEPS = 64, 16, 1024, 4
PA_BETAS = np.linspace(0.0, 0.3, 16)
PA_SEED_GENS = (101, 202, 303, 404, 505, 606, 707, 808)


def _anneal(exact, seed_gen, **kw):
    import py_monte_carlo
    ea, eb, ej = exact.square_lattice_edges(PA_W, PA_H, -1.0)
    lat = py_monte_carlo.Lattice.from_arrays(ea, eb, ej, seed_gen=seed_gen)
    return lat.run_population_annealing(PA_BETAS, PA_SWEEPS, PA_POP, **kw)


def test_free_energy_against_kaufman(exact):
    """N ln 2 + log_z_ratio[-1] over eight seeded runs against the exact ln Z(0.3) = 809.5327 of the 64 x 16 torus: (a) the
    sample standard deviation is at most 0.5 (twice what an independent numpy implementation of the rule shows), (b) the mean is
    within 4 standard errors, (c) so is the final mean energy."""
    N = PA_W * PA_H
    runs = [_anneal(exact, sg, return_states=False) for sg in PA_SEED_GENS]
    lnz = np.array([N * np.log(2.0) + r.log_z_ratio[-1] for r in runs])
    want = exact.kaufman_lnZ(PA_W, PA_H, 0.3)
    std = lnz.std(ddof=1)
    print(f"ln Z {lnz.mean():.4f} +- {std / np.sqrt(8):.4f} (std {std:.4f}) exact {want:.4f}")
    assert abs(want - 809.5327) < 1e-3
    assert std <= 0.5
    assert abs(lnz.mean() - want) <= 4 * std / np.sqrt(8)
    e = np.array([r.mean_energy[-1] for r in runs])
    e_want = exact.kaufman_energy(PA_W, PA_H, 0.3)
    print(f"<E> {e.mean():.3f} +- {e.std(ddof=1) / np.sqrt(8):.3f} exact {e_want:.3f}")
    assert abs(e.mean() - e_want) <= 4 * e.std(ddof=1) / np.sqrt(8)
    r = runs[0]
    assert r.log_z_ratio[0] == 0.0 and r.log_z_ratio.shape == (16,) and r.mean_energy.shape == (16,)
    assert r.distinct_sources.shape == (15,) and (r.distinct_sources <= PA_POP).all() and r.states is None
    counts = np.bincount(r.families, minlength=PA_POP)
    assert r.rho_t == pytest.approx(PA_POP * ((counts / PA_POP) ** 2).sum())


def test_a_run_repeats_and_follows_the_c_abi(capi, exact):
    a, b = _anneal(exact, 42), _anneal(exact, 42)
    for name in ("energies", "states", "log_z_ratio", "mean_energy", "distinct_sources", "families"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert a.states.shape == (PA_POP, PA_W * PA_H) and a.states.dtype == np.bool_
    # the same schedule through the C ABI, step by step with blocking calls: configurations, records and the ln Q sum
    ea, eb, ej = exact.square_lattice_edges(PA_W, PA_H, -1.0)
    seeds = capi.make_seeds(42, PA_POP + 1)
    g = capi.Graph(ea, eb, ej, device=0)
    st = capi.States(g, seeds[:PA_POP])
    log_z, recs = [0.0], []
    for k, beta in enumerate(PA_BETAS):
        if k:
            dbeta = beta - PA_BETAS[k - 1]
            st.pa_resample(dbeta, seeds[PA_POP], k)
            recs.append(st.pa_last())
            log_z.append(log_z[-1] + PA.log_q(recs[-1], PA_POP, dbeta))
        st.do_time_steps(PA_SWEEPS, beta)
    assert np.array_equal(st.energies(), a.energies) and np.array_equal(st.states(), a.states)
    assert np.array_equal(st.pa_families(), a.families)
    assert np.array_equal(a.distinct_sources, [r["distinct"] for r in recs])
    assert np.array_equal(a.mean_energy[:-1], [r["mean_energy"] for r in recs])
    assert abs(a.mean_energy[-1] - a.energies.mean()) <= PA_POP * 2.0 ** -52 * np.abs(a.energies).mean()   # any summation order
    assert np.abs(a.log_z_ratio - np.array(log_z)).max() <= 1e-12 * 16 * max(1.0, np.abs(log_z).max())   # f64 log and a 16-term sum
    # ... and in one enqueue-only call
    st2 = capi.States(g, seeds[:PA_POP])
    log = st2.pa_run(PA_BETAS, PA_SWEEPS, seeds[PA_POP])
    assert st2.timestep == PA_SWEEPS * len(PA_BETAS)
    assert np.array_equal(st2.packed(), st.packed()) and np.array_equal(st2.pa_families(), a.families)
    for name in ("sum", "eref", "distinct", "mean_energy"):
        assert np.array_equal(log[name], [r[name] for r in recs]), name
    last = st2.pa_last()
    assert last["sum"] == recs[-1]["sum"] and np.array_equal(last["src"], recs[-1]["src"])


@pytest.mark.parametrize("case", [(("strip",), 8), (("cubic", 6, True), 70), (("cubic", 8, False), 33), (("real",), 45)], ids=_id)
def test_one_call_schedule_equals_the_blocking_loop(capi, exact, monkeypatch, case):
    """isingmc_pa_run (everything enqueued, preset acceptance tables, a device log of records) against the loop of
    pa_resample / do_time_steps on a second container of the same seeds, on the paths that upload tables per call."""
    kind, R = case
    P, Q = _make(capi, exact, monkeypatch, kind, R), _make(capi, exact, monkeypatch, kind, R)
    betas = np.array([0.25, 0.3, 0.3, 0.42])
    log = P.st.pa_run(betas, 3, SEED)
    for k, beta in enumerate(betas):
        if k:
            Q.st.pa_resample(beta - betas[k - 1], SEED, k)
            rec = Q.st.pa_last()
            for name in ("sum", "eref", "distinct", "mean_energy"):
                assert log[name][k - 1] == rec[name], (name, k)
        Q.st.do_time_steps(3, beta)
    assert P.st.timestep == Q.st.timestep == 12
    assert np.array_equal(P.st.raw_state(), Q.st.raw_state())
    assert np.array_equal(P.st.energies(), Q.st.energies()) and np.array_equal(P.st.pa_families(), Q.st.pa_families())


def test_python_argument_checks(exact):
    import py_monte_carlo
    ea, eb, ej = exact.square_lattice_edges(64, 4, -1.0)   # a checkerboard container
    lat = py_monte_carlo.Lattice.from_arrays(ea, eb, ej, seed_gen=1)
    for betas, sweeps, pop in (([], 1, 4), ([0.2, 0.1], 1, 4), ([0.1], 0, 4), ([0.1], 1, 0)):
        with pytest.raises(ValueError):
            lat.run_population_annealing(betas, sweeps, pop)
    lat.set_devices([0, 0])
    with pytest.raises(ValueError, match="one device"):
        lat.run_population_annealing([0.1, 0.2], 1, 4)
    lat.set_devices([0])
    lat.set_global_bias(0.5)
    with pytest.raises(ValueError):   # a field: no family this graph can run on is served
        lat.run_population_annealing([0.1, 0.2], 1, 4)
    lat.set_global_bias(0.0)
    lat.set_initial_state([True] * 256)
    r = lat.run_population_annealing([0.0], 1, 4)   # one beta: no resampling at all
    assert r.log_z_ratio.tolist() == [0.0] and r.distinct_sources.shape == (0,) and r.rho_t == 1.0


# ---- heating, vanishing weights, call sequences without a host measurement, growth -----------------------------------------
@pytest.mark.parametrize("case", FAMILIES, ids=_id)
def test_heating_steps(capi, exact, monkeypatch, case):
    """dbeta < 0: the reference energy is the MAXIMUM, the weights fall towards the low energies."""
    kind, R = case
    P = _make(capi, exact, monkeypatch, kind, R)
    P.sweeps(3, BETA)
    e = P.compare()
    fam = np.arange(R, dtype=np.uint32)
    want, fam = _resample_and_compare(P, e, -0.05, 1, fam)
    assert want["eref"] == e.max() and want["eref"] > e.min()
    assert want["weights"][int(np.argmax(e))] == 1 << 32 and want["weights"][int(np.argmin(e))] < 1 << 32
    P.sweeps(2, BETA - 0.05)
    e = P.compare()
    want, fam = _resample_and_compare(P, e, -0.05, 2, fam)
    assert want["eref"] == e.max() and want["eref"] > e.min()
    P.sweeps(1, BETA - 0.1)
    P.compare()


def _all_up_at_slot_5(P):
    n = P.st.graph.nvars
    P.st.set_state(5, np.ones(n, dtype=np.uint8))
    if isinstance(P, _Board):
        P.ref[5] = P.lat.pack(np.ones(n, dtype=np.uint8))
    else:
        P.ref[5] = 1
        P.e_ref = None


@pytest.mark.parametrize("case", [(("board", 128, 64, False), 37, 0.05), (("cubic", 8, False), 70, 0.1)], ids=lambda c: _id(c[:2]))
def test_weights_that_vanish(capi, exact, monkeypatch, case):
    """One replica in the ground state of a ferromagnet among replicas near beta = 0.1: every other exponent is below -40, where
    det_exp returns 0, so S = 2^32 exactly and one replica takes every slot; heated by the same step on a twin container, that
    replica alone gets no copy."""
    kind, R, dbeta = case
    P = _make(capi, exact, monkeypatch, kind, R)
    P.sweeps(2, 0.1)
    _all_up_at_slot_5(P)
    e = P.compare()
    assert int(np.argmin(e)) == 5
    for _ in range(4):   # the RESTATEMENT says whether the step is large enough
        W = PA.sources(SEED, 1, e, dbeta)["weights"]
        if W[5] == 1 << 32 and sum(W) == 1 << 32:
            break
        dbeta *= 2
    else:
        pytest.fail("no step leaves one weight")
    assert -dbeta * (np.delete(e, 5).min() - e[5]) < -40.0
    want, fam = _resample_and_compare(P, e, dbeta, 1, np.arange(R, dtype=np.uint32))
    assert want["sum"] == 1 << 32 and want["distinct"] == 1 and (want["src"] == 5).all() and (fam == 5).all()
    assert (P.st.pa_families() == 5).all() and P.st.pa_last()["sum"] == 1 << 32
    P.sweeps(1, 0.1)
    P.compare()
    Q = _make(capi, exact, monkeypatch, kind, R)
    Q.sweeps(2, 0.1)
    _all_up_at_slot_5(Q)
    e = Q.compare()
    want, fam = _resample_and_compare(Q, e, -dbeta, 1, np.arange(R, dtype=np.uint32))
    assert want["weights"][5] == 0 and 5 not in want["src"] and 5 not in fam and want["distinct"] > 1
    Q.sweeps(1, 0.1)
    Q.compare()


SEQUENCE_CASES = [(("board", 64, 4, True), 37), (("strip",), 8), (("cubic", 6, True), 70), (("real",), 45)]


@pytest.mark.parametrize("case", SEQUENCE_CASES, ids=_id)
def test_two_resamplings_in_a_row(capi, exact, monkeypatch, case):
    """No host measurement between the two: the second step weighs the energies e[src] of the gathered population."""
    kind, R = case
    P = _make(capi, exact, monkeypatch, kind, R)
    P.sweeps(3, BETA)
    e = P.compare()
    first = PA.sources(SEED, 1, e, 0.05)
    e1 = e[first["src"]]
    second = PA.sources(SEED, 2, e1, 0.05)
    P.snapshot()
    P.st.pa_resample(0.05, SEED, 1)
    P.st.pa_resample(0.05, SEED, 2)
    got = P.st.pa_last()
    assert np.array_equal(got["src"], second["src"])
    assert got["sum"] == second["sum"] and got["eref"] == second["eref"] and got["distinct"] == second["distinct"]
    assert abs(got["mean_energy"] - second["mean_energy"]) <= R * 2.0 ** -52 * np.abs(e1).mean()
    both = first["src"][second["src"]]   # new[j] = old[first[second[j]]]
    P.gather(both)
    assert np.array_equal(P.st.pa_families(), both)
    assert np.array_equal(P.compare(), e[both])
    P.sweeps(1, BETA)
    P.compare()


@pytest.mark.parametrize("case", SEQUENCE_CASES, ids=_id)
def test_resampling_straight_after_other_measurements(capi, exact, monkeypatch, case):
    """pa_resample directly after a run that returned per-step energies, and directly after magnetisations(): the restatement is
    fed with the energies of its own configurations, the library is not asked for them in between."""
    kind, R = case
    P = _make(capi, exact, monkeypatch, kind, R)
    P.sweeps(2, BETA)
    P.compare()
    fam = np.arange(R, dtype=np.uint32)
    per_step = P.sweeps(2, BETA, per_step_energies=True)
    e = P.energies()
    assert np.array_equal(per_step[:, -1], e)
    _, fam = _resample_and_compare(P, e, 0.05, 1, fam)
    P.sweeps(2, BETA + 0.05)
    e = P.energies()
    m = P.st.magnetisations()
    assert m.shape == (R,)
    _, fam = _resample_and_compare(P, e, 0.05, 2, fam)
    m = P.st.magnetisations()   # ... and once more with nothing but a resampling since the last measurement
    e = P.energies()
    _, fam = _resample_and_compare(P, e, 0.05, 3, fam)
    P.sweeps(1, BETA + 0.1)
    P.compare()


@pytest.mark.parametrize("case", [(("board", 64, 4, True), 37), (("cubic", 6, True), 64)], ids=_id)
def test_growth_after_a_resampling(capi, exact, monkeypatch, case):
    """append on a resampled container (on the cubic graph the 65th replica opens a group): the family table is kept, the new slot
    founds its own family, and the next resampling runs on buffers of the new size."""
    kind, R = case
    P = _make(capi, exact, monkeypatch, kind, R)
    P.sweeps(2, BETA)
    e = P.compare()
    _, fam = _resample_and_compare(P, e, 0.05, 1, np.arange(R, dtype=np.uint32))
    assert len(set(fam.tolist())) < R
    seed = capi.make_seeds(77, 1)[0]
    P.st.append(seed)
    P.seeds = np.append(P.seeds, seed)
    if isinstance(P, _Board):
        P.ref.append(P.lat.init(seed))
    else:
        start, _, _ = IR.run(P.G, np.array([seed], dtype=np.uint64), 0, 0, betas=[])   # a new group, keyed by its first seed
        P.ref = np.concatenate([P.ref, start])
        P.e_ref = None
    fam = np.append(fam, np.uint32(R))
    assert P.st.count == R + 1 and np.array_equal(P.st.pa_families(), fam)
    P.compare()
    P.sweeps(2, BETA + 0.05)
    e = P.compare()
    assert np.array_equal(P.st.pa_families(), fam)
    want, fam = _resample_and_compare(P, e, 0.05, 2, fam)   # raw words, word for word, inside
    assert len(want["src"]) == R + 1
    P.sweeps(1, BETA + 0.1)
    P.compare()
    P.st.pa_reset_families()
    assert np.array_equal(P.st.pa_families(), np.arange(R + 1))

"""Cluster moves, minimum records, population annealing, ladders, sampling and call sequences with the replica lanes FORCED.

`run_steps` spreads a call's replicas (streaming checkerboard kernels) or replica groups (both replica-packed families) over
several streams, and everything that cuts a call -- a Swendsen-Wang step, an isoenergetic move, an update of the minimum
records -- joins the lanes and forks them again behind it.  The measured rule turns lanes on at production sizes only, so the
small shapes of the features' own test files never reach those joins.  Here `set_option("streams", n)` / `("pk_streams", n)`
force the lane count at any size: every case runs on containers of the same graph and seeds with one, two and three lanes and
everything they hold must be equal BIT FOR BIT (raw words, energies as f64 bit patterns, timesteps, statistics, records, step
records, permutations, samples).  On the smallest shape of every family the three-lane container is also compared with the
Python restatement the feature's own test file uses (cluster_reference, icm_reference, packed_cluster_reference,
packed_icm_reference, minimum_reference, pa_reference), so that the equality does not rest on the one-lane run alone.  There is
no tolerance anywhere: every compared value is an integer or an f64 produced by the same arithmetic.

Shapes: checkerboard 64 x 4 and 192 x 344 with 1 (lanes clamp to one), 2 (three clamp to two), 5 (2 + 2 + 1) and 40 replicas;
bit-sliced 6^3 +-J and the diluted graph of tests/test_gpu_overlaps.py with 70 (3 groups), 97 (4 groups: with three lanes the
third holds no group), 33 (a second group of one bit) experiments and the shard [20, 50) of 70; the real-coupling 12 x 10
Gaussian glass with biases with 70 and 97.  The multi-class kernels (field, open boundaries) serve lattices of whole quads per
row only, W % 256 == 0: their streaming path is reached at 256 x 4; a 64 x 4 lattice with a field or an open boundary runs on
the f64 CSR family, which has no lanes, and is kept as a case that must not be disturbed by the option.  Cases 1-3 run once
more at 512^2 x 6 and 12^3 x 97, where a lane cannot have drained by chance before a misplaced join matters.
"""
import numpy as np
import pytest

import cluster_reference as CR
import icm_reference as ICM
import minimum_reference as MR
import pa_reference as PA
import packed_cluster_reference as PCR
import packed_icm_reference as PIR

pytestmark = pytest.mark.gpu

LANES = (1, 2, 3)
BOARD_R = [(1, None), (2, None), (5, None), (40, None)]
PACKED_R = [(70, None), (97, None), (33, None), (70, (20, 50))]
REAL_R = [(70, None), (97, None)]


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


# ---- graphs of every family, containers with a forced lane count ------------------------------------------------------------
class Family:
    """One graph, the containers made on it with a forced lane count, and what the restatements need of it."""

    def __init__(self, capi, family, g, edges, **kw):
        self.capi, self.family, self.g, self.edges = capi, family, g, edges
        self.W = self.H = self.G = self.biases = self.lat = None
        self.reference = False      # the smallest shape of its family: compared with the Python restatement too
        self.__dict__.update(kw)
        self._classes = None

    def force(self, st, lanes):
        if self.family in ("checkerboard", "csr_f64"):   # LatStream / McStream: no LDS-resident kernel, no strips
            st.set_option("disable_resident", 1)
            st.set_option("strip", 0)
            st.set_option("streams", lanes)
        else:
            st.set_option("pk_streams", lanes)

    def make(self, seeds, lanes, cut=None):
        st = self.capi.States(self.g, seeds, replica_range=cut)
        assert st.family == self.family
        self.force(st, lanes)
        return st

    @property
    def real(self):
        return self.family == "packed_real"

    @property
    def classes(self):
        """Two class tables over the sites (three classes; the second table leaves every fifth site aside)."""
        if self._classes is None:
            i = np.arange(self.g.nvars)
            second = np.where(i % 5 == 0, self.capi.NO_CLASS, (i // 7) % 2)
            self._classes = self.capi.SiteClasses(self.g, np.stack([i % 3, second]), 3)
        return self._classes


def _family(spec, capi, exact, oracle, monkeypatch):
    kind, _, rest = spec.partition(":")
    if kind == "board":   # board:WxH:uniform|glass
        shape, _, signs = rest.partition(":")
        W, H = (int(v) for v in shape.split("x"))
        ea, eb, ej = exact.square_lattice_edges(W, H, -1.0, np.random.default_rng(W + 7 * H) if signs == "glass" else None)
        g = capi.Graph(ea, eb, ej)
        assert g.kind == capi.KIND_LATTICE2D and g.info.fast_path == 0
        jr, jd = ICM.couplings(W, H, ej)
        return Family(capi, "checkerboard", g, (ea, eb, ej), W=W, H=H, jr=jr, jd=jd, glass=signs == "glass", lat=ICM.make_lat(W, H, jr, jd),
                      reference=(W, H) == (64, 4))
    if kind in ("field", "open"):   # field:WxH / open:WxH: the constructors of tests/test_gpu_field_open.py
        W, H = (int(v) for v in rest.split("x"))
        ea, eb, ej = exact.square_lattice_edges(W, H, -1.0)
        biases, h, lattice = None, 0.25, W % 256 == 0
        if kind == "field":
            biases = np.full(W * H, h)
            lat = oracle.Lat(W, H, 1.0, 0, field=h)
        else:
            keep = ~((ea % W == W - 1) & (eb % W == 0))   # the right bonds of the last column
            ea, eb, ej = ea[keep], eb[keep], ej[keep]
            lat = oracle.Lat(W, H, 1.0, 0, open_x=True, open_y=False)
        g = capi.Graph(ea, eb, ej, nvars=W * H, biases=biases)
        # whole quads per row (W % 256 == 0) or the f64 CSR family, which has no lanes
        assert (g.kind == capi.KIND_LATTICE2D and g.info.fast_path == (1 if kind == "field" else 2)) if lattice else g.kind == capi.KIND_GENERAL
        return Family(capi, "checkerboard" if lattice else "csr_f64", g, (ea, eb, ej), W=W, H=H, biases=biases, lat=lat if lattice else None)
    monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
    if kind == "cubic":   # cubic:L, the seeded +-J glass of tests/packed_icm_reference.py
        L = int(rest)
        ea, eb, ej = PIR.cubic_glass(exact, L)
        g = capi.Graph(ea, eb, ej, nvars=L ** 3, force_general=True)
        return Family(capi, "packed_bitsliced", g, (ea, eb, ej), G=PIR.Graph(ea, eb, ej, L ** 3) if L == 6 else None, reference=L == 6)
    if kind == "diluted":
        from test_gpu_overlaps import _diluted_graph
        ea, eb, ej, n = _diluted_graph()
        return Family(capi, "packed_bitsliced", capi.Graph(ea, eb, ej, nvars=n, force_general=True), (ea, eb, ej))
    assert kind == "real"   # the 12 x 10 Gaussian glass with biases
    ea, eb, _ = exact.square_lattice_edges(12, 10, 1.0)
    rng = np.random.default_rng(1210)
    ej, biases = rng.normal(size=len(ea)), 0.3 * rng.normal(size=120)
    g = capi.Graph(ea, eb, ej, nvars=120, biases=biases, stable_path=True)
    return Family(capi, "packed_real", g, (ea, eb, ej), G=PIR.Graph(ea, eb, ej, 120), biases=biases, reference=True)


def _pops(*groups):
    """pytest params (spec, R, cut) of (specs, [(R, cut)]) groups; R is the number of experiments, cut a shard of them."""
    out = []
    for specs, pops in groups:
        for spec in specs:
            for R, cut in pops:
                out.append(pytest.param(spec, R, cut, id=f"{spec}-{R}" + (f"-shard{cut[0]}_{cut[1]}" if cut else "")))
    return out


UNIFORM_BOARDS = ["board:64x4:uniform", "board:192x344:uniform"]
GLASS_BOARDS = ["board:64x4:glass", "board:192x344:glass"]
BIT_SLICED = ["cubic:6", "diluted"]
CLUSTER_POPS = _pops((UNIFORM_BOARDS, BOARD_R), (BIT_SLICED, PACKED_R))
ALL_POPS = _pops((UNIFORM_BOARDS + GLASS_BOARDS, BOARD_R), (BIT_SLICED, PACKED_R), (["real"], REAL_R))


# ---- what a container holds, and the comparison of two of them ---------------------------------------------------------------
def _snap(st, cluster=False, icm=False, best=False, pa=False):
    out = dict(timestep=st.timestep, raw=st.raw_state(), energies=_bits(st.energies()))
    if cluster:
        out["cluster_count"], out["cluster_largest"] = st.cluster_stats()
    if icm:
        out["icm_count"], out["icm_largest"], out["icm_minus"] = st.icm_stats()
    if best:
        e, s, t, n = st.best()
        out.update(best_energies=_bits(e), best_states=s, best_timesteps=t, best_improvements=n, best_raw=st.best_raw())
    if pa:
        last = st.pa_last()
        out.update(pa_src=last["src"], pa_sum=last["sum"], pa_eref=_bits(last["eref"]), pa_distinct=last["distinct"], pa_mean=_bits(last["mean_energy"]))
    return out


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        assert np.array_equal(a[key], b[key]), f"{what}: {key} differs"


def _on_lanes(fam, seeds, cut, body, lanes=LANES):
    """body(st) -> (dict, extra) on a fresh container per lane count; the dicts must be equal.  Returns the last container, its
    dict and its extra."""
    first = None
    for n in lanes:
        st = fam.make(seeds, n, cut)
        snap, extra = body(st)
        if first is None:
            first = snap
        else:
            _assert_same(first, snap, f"{n} lanes against {lanes[0]}")
    return st, snap, extra


def _seeds(capi, tag, R, cut):
    return capi.make_seeds(tag + R, R)   # (a shard is cut out of all R experiments)


def _rows(cut, R):
    return slice(*cut) if cut else slice(0, R)


# ---- the restatements ----------------------------------------------------------------------------------------------------------
def _check_cluster(fam, st, seeds, cut, start, betas, k):
    T = len(betas)
    if fam.family == "checkerboard":
        packed, e, stats = st.packed(), st.energies(), st.cluster_stats()
        for r, seed in enumerate(seeds):
            spins, e_ref, ref_stats = CR.run(fam.W, fam.H, -1.0, int(seed), start[r].astype(np.uint8), 0, betas, k)
            assert np.array_equal(packed[r], fam.lat.pack(spins.ravel())), f"replica {r}: configurations differ"
            assert e[r] == e_ref[-1] and (int(stats[0][r]), int(stats[1][r])) == ref_stats, r
        return
    ref, e_ref, ref_stats = PCR.run(fam.G, seeds, T, k, betas=betas)
    rows = _rows(cut, len(seeds))
    assert np.array_equal(st.states().astype(np.uint8), ref[rows])
    assert np.array_equal(st.energies(), e_ref[rows, -1])
    for got, want in zip(st.cluster_stats(), ref_stats):
        assert np.array_equal(got.astype(np.int64), want[rows])


def _check_icm(fam, st, seeds, cut, start, betas, k):
    T = len(betas)
    if fam.family == "checkerboard":
        spins, e_ref, ref_stats = ICM.run_replicas(fam.W, fam.H, fam.jr, fam.jd, [int(s) for s in seeds], [s.astype(np.uint8) for s in start], 0, betas, k)
        packed, e = st.packed(), st.energies()
        for r in range(len(seeds)):
            assert np.array_equal(packed[r], fam.lat.pack(spins[r].ravel())), f"replica {r}: configurations differ"
            assert e[r] == e_ref[r, -1]
        got = st.icm_stats()
        assert [tuple(int(a[p]) for a in got) for p in range(len(seeds) // 2)] == ref_stats
        return
    ref, e_ref, ref_stats = PIR.run(fam.G, seeds, T, k, betas=betas, biases=fam.biases, real=fam.real)
    rows = _rows(cut, len(seeds))
    assert np.array_equal(st.states().astype(np.uint8), ref[rows])
    assert np.array_equal(st.energies(), e_ref[rows, -1])
    for got, want in zip(st.icm_stats(), ref_stats):
        assert np.array_equal(got.astype(np.int64), want[rows.start // 2:rows.stop // 2])


def _assert_records(st, rec):
    e, s, t, n = st.best()
    assert np.array_equal(_bits(e), _bits(rec.energy)) and np.array_equal(s, rec.state)
    assert np.array_equal(t, rec.timestep) and n == rec.improvements


# ---- 1. Swendsen-Wang steps inside a long call ------------------------------------------------------------------------------
def _cluster_body(k, T, beta):
    def body(st):
        st.set_cluster_every(k)
        start = st.states()
        st.do_time_steps(T, beta)
        return _snap(st, cluster=True), start
    return body


@pytest.mark.parametrize("spec,R,cut", CLUSTER_POPS)
def test_swendsen_wang_steps(capi, exact, oracle, monkeypatch, spec, R, cut):
    """cluster_every = 7 in one call of 50 timesteps (Metropolis stretches of 6 on the lanes between the steps), and
    cluster_every = 1 for 5 timesteps (every step joins, nothing forks again)."""
    fam = _family(spec, capi, exact, oracle, monkeypatch)
    seeds = _seeds(capi, 1000, R, cut)
    for k, T in ((7, 50), (1, 5)):
        beta = 0.42 if fam.family == "checkerboard" else 0.5
        st, _, start = _on_lanes(fam, seeds, cut, _cluster_body(k, T, beta))
        assert st.timestep == T
        if fam.reference:
            _check_cluster(fam, st, seeds, cut, start, [beta] * T, k)


# ---- 2. isoenergetic moves ----------------------------------------------------------------------------------------------------
def _icm_body(k, T, beta):
    def body(st):
        st.set_icm_every(k)
        start = st.states()
        st.do_time_steps(T, beta)
        return _snap(st, icm=True), start
    return body


@pytest.mark.parametrize("spec,R,cut", ALL_POPS)
def test_isoenergetic_moves(capi, exact, oracle, monkeypatch, spec, R, cut):
    fam = _family(spec, capi, exact, oracle, monkeypatch)
    seeds = _seeds(capi, 2000, R, cut)
    st, _, start = _on_lanes(fam, seeds, cut, _icm_body(5, 43, 0.6))
    assert st.timestep == 43
    if fam.reference:
        _check_icm(fam, st, seeds, cut, start, [0.6] * 43, 5)


# ---- 3. minimum records -------------------------------------------------------------------------------------------------------
# call lengths 1, 7, 50, 7: the periods straddle the calls.  Hot, then a cooling ramp (a schedule: one acceptance table per
# timestep, which the packed runner rewrites stretch by stretch behind a join) along which the energies keep falling, so that
# nearly every update copies configurations; then hot again: updates that improve nothing
MIN_CALLS = [(1, 0.2), (7, 0.1), (50, np.linspace(0.05, 1.2, 50)), (7, 0.1)]


def _minimum_body(every, icm):
    def body(st):
        if icm:
            st.set_icm_every(5)
        st.set_track_best(every)
        for n, beta in MIN_CALLS:
            st.do_time_steps(n, beta)
        return _snap(st, icm=bool(icm), best=True), None
    return body


def _twin_records(twin, every):
    """The one-lane, untracked twin stepped from update point to update point and read there: tests/minimum_reference.py."""
    rec = MR.Records(twin.count, twin.graph.nvars)
    for n, beta in MIN_CALLS:
        k = 0
        while k < n:
            m = min(n - k, every - twin.timestep % every)
            twin.do_time_steps(m, beta if np.ndim(beta) == 0 else beta[k:k + m])
            k += m
            if twin.timestep % every == 0:
                rec.update(twin.timestep, twin.energies(), twin.states())
    return rec


@pytest.mark.parametrize("icm", [0, 5], ids=["plain", "icm5"])
@pytest.mark.parametrize("spec,R,cut", ALL_POPS)
def test_minimum_records(capi, exact, oracle, monkeypatch, spec, R, cut, icm):
    """track_best every 1, 3 and 16; with icm_every = 5 on top two different cutters act in one call."""
    fam = _family(spec, capi, exact, oracle, monkeypatch)
    seeds = _seeds(capi, 3000, R, cut)
    for every in (1, 3, 16):
        st, snap, _ = _on_lanes(fam, seeds, cut, _minimum_body(every, icm))
        assert st.timestep == 65 and snap["best_improvements"] >= st.count
        if fam.reference:
            twin = fam.make(seeds, 1, cut)
            if icm:
                twin.set_icm_every(icm)
            rec = _twin_records(twin, every)
            _assert_records(st, rec)
            assert np.array_equal(st.raw_state(), twin.raw_state()) and np.array_equal(_bits(st.energies()), _bits(twin.energies()))
            assert (rec.timestep > 16).any(), "no record is set along the ramp: the updates after the first copy nothing"


# ---- cases 1-3 once more where a lane cannot have drained by chance -----------------------------------------------------------
@pytest.mark.parametrize("case", ["cluster7", "cluster1", "icm", "minimum1", "minimum3", "minimum16", "minimum3_icm"])
@pytest.mark.parametrize("spec,R", [("board:512x512", 6), ("cubic:12", 97)])
def test_large_shapes_three_lanes_against_one(capi, exact, oracle, monkeypatch, spec, R, case):
    """512^2 x 6 and 12^3 x 97: three lanes against one, no restatement.  (Swendsen-Wang steps need one coupling sign: the
    lattice is uniform for them and a +-J glass otherwise.)"""
    if spec.startswith("board"):
        spec += ":uniform" if case.startswith("cluster") else ":glass"
    fam = _family(spec, capi, exact, oracle, monkeypatch)
    seeds = capi.make_seeds(4000, R)
    beta = 0.42 if fam.family == "checkerboard" else 0.5
    body = {"cluster7": _cluster_body(7, 50, beta), "cluster1": _cluster_body(1, 5, beta), "icm": _icm_body(5, 43, 0.6),
            "minimum1": _minimum_body(1, 0), "minimum3": _minimum_body(3, 0), "minimum16": _minimum_body(16, 0),
            "minimum3_icm": _minimum_body(3, 5)}[case]
    _on_lanes(fam, seeds, None, body, lanes=(1, 3))


# ---- 4. population annealing --------------------------------------------------------------------------------------------------
PA_BETAS = np.linspace(0.1, 0.8, 8)
PA_SWEEPS = 12
PA_SEED = 0x0123456789ABCDEF


def _pa_prepare(fam, st):
    if fam.real:
        st.set_icm_every(5)
    else:
        st.set_cluster_every(5)


@pytest.mark.parametrize("spec,R,cut", _pops((UNIFORM_BOARDS, BOARD_R[1:]), (BIT_SLICED, PACKED_R[:3]), (["real"], REAL_R)))
def test_population_annealing(capi, exact, oracle, monkeypatch, spec, R, cut):
    """pa_run over 8 betas, 12 sweeps each, with a cluster period (checkerboard, bit-sliced) or an ICM period (real couplings) and
    the minimum records on; then the overlaps of the final population, whose last sweeps ran on the lanes."""
    fam = _family(spec, capi, exact, oracle, monkeypatch)
    seeds = _seeds(capi, 5000, R, cut)

    def body(st):
        _pa_prepare(fam, st)
        st.set_track_best(1 << 62)   # the update points are the resamplings and the end of the run
        log = st.pa_run(PA_BETAS, PA_SWEEPS, PA_SEED)
        snap = _snap(st, best=True, pa=True)
        snap.update(log_sum=log["sum"], log_eref=_bits(log["eref"]), log_distinct=log["distinct"], log_mean=_bits(log["mean_energy"]))
        snap["spin"], snap["link"] = st.overlaps()
        snap["by_class"] = st.overlaps_by_class(fam.classes)
        return snap, log

    st, snap, log = _on_lanes(fam, seeds, cut, body)
    assert st.timestep == len(PA_BETAS) * PA_SWEEPS
    if not fam.reference:
        return
    # the twin: one lane, driven step by step -- the sources of tests/pa_reference.py from the energies read on the host
    twin = fam.make(seeds, 1)
    _pa_prepare(fam, twin)
    rec = MR.Records(R, fam.g.nvars)
    for k, beta in enumerate(PA_BETAS):
        if k:
            e = twin.energies()
            rec.update(twin.timestep, e, twin.states())
            ref = PA.sources(PA_SEED, k, e, PA_BETAS[k] - PA_BETAS[k - 1])
            assert ref["sum"] == int(log["sum"][k - 1]) and ref["distinct"] == int(log["distinct"][k - 1])
            assert _bits(ref["eref"]) == _bits(log["eref"][k - 1])
            twin.pa_apply_sources(ref["src"])
        twin.do_time_steps(PA_SWEEPS, float(beta))
    rec.update(twin.timestep, twin.energies(), twin.states())
    assert np.array_equal(snap["pa_src"], ref["src"])
    _assert_records(st, rec)
    assert np.array_equal(st.raw_state(), twin.raw_state()) and np.array_equal(_bits(st.energies()), _bits(twin.energies()))


# ---- 5. ladders -----------------------------------------------------------------------------------------------------------------
def _ladder_run(monkeypatch, lanes, edges, betas, copies, icm_every, track):
    """A ladder whose rung containers are created with the lane count forced (the switches are read when a container is created):
    a dozen rounds of 10 sweeps; everything it holds afterwards."""
    from pyisingmontecarlo_amd.tempering import ClassicalTempering

    for name, value in (("STREAMS", lanes), ("PK_STREAMS", lanes), ("DISABLE_RESIDENT", 1), ("STRIP", 0)):
        monkeypatch.setenv("ISINGMC_" + name, str(value))
    pt = ClassicalTempering(edges, seed=4711, copies=copies)
    for beta in betas:
        pt.add_graph(float(beta))
    if icm_every:
        pt.set_replica_cluster_update_every(icm_every)
    if track:
        pt.set_track_minimum(True)
    pt.timesteps(120, 10)
    containers = [c._states for c in pt._pair] if copies == 2 else [pt._states]
    out = dict(permutation=pt.get_permutation(), swaps=pt.get_total_swaps())
    for i, st in enumerate(containers):
        for key, value in _snap(st, best=track).items():
            out[f"{key}{i}"] = value
    if copies == 2:
        out["icm_count"], out["icm_largest"], out["icm_minus"] = pt.get_replica_cluster_stats()
        out["spin"], out["link"] = pt.get_overlaps()
    return out, pt


@pytest.mark.parametrize("track", [False, True], ids=["untracked", "tracked"])
@pytest.mark.parametrize("case", ["lattice_host_swaps", "lattice_on_stream", "lattice_two_copies_icm", "bit_sliced_on_stream"])
def test_ladders(capi, exact, monkeypatch, case, track):
    if case.startswith("lattice"):
        edges = exact.square_lattice_edges(64, 4, -1.0, np.random.default_rng(9))
        betas = np.linspace(0.3, 0.44, 8)
    else:   # 40 rungs: two replica groups
        monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
        edges = PIR.cubic_glass(exact, 6)
        betas = np.linspace(0.4, 0.61, 40)
    if case == "lattice_host_swaps":
        monkeypatch.setenv("ISINGMC_PT_HOST", "1")
    copies, icm_every = (2, 3) if case == "lattice_two_copies_icm" else (1, 0)
    first = None
    for lanes in LANES:
        out, pt = _ladder_run(monkeypatch, lanes, edges, betas, copies, icm_every, track)
        assert pt._on_stream == (case != "lattice_host_swaps") and out["swaps"] > 0
        assert pt._states.family == ("checkerboard" if case.startswith("lattice") else "packed_bitsliced")
        if first is None:
            first = out
        else:
            _assert_same(first, out, f"{lanes} lanes against 1")


# ---- 6. between two containers, nothing waited for -------------------------------------------------------------------------
@pytest.mark.parametrize("spec,R,cut", _pops((GLASS_BOARDS, BOARD_R[1:]), (["cubic:6"], PACKED_R[:2]), (["real"], REAL_R[:1])))
def test_moves_and_overlaps_between_two_containers(capi, exact, oracle, monkeypatch, spec, R, cut):
    """A and B (a ladder attached to each) run 20 timesteps on their lanes with enqueue-only calls; then, with nothing waited
    for, a move between them and the overlaps between them."""
    fam = _family(spec, capi, exact, oracle, monkeypatch)
    betas = np.linspace(0.3, 0.7, R)
    first = None
    for lanes in LANES:
        a, b = fam.make(capi.make_seeds(6000, R), lanes), fam.make(capi.make_seeds(6001, R), lanes)
        for st, seed in ((a, 5), (b, 6)):
            assert st.pt_can_attach(R, 0, R, 1)
            st.pt_attach(betas, 0, R, 1, seed)
        a.pt_time_steps(20)
        b.pt_time_steps(20)
        a.icm_between(b)
        spin, link = a.overlaps(b)
        out = dict(spin=spin, link=link, by_class=a.overlaps_by_class(fam.classes, b))
        out["count"], out["largest"], out["minus"] = a.icm_between_stats()
        for name, st in (("a", a), ("b", b)):
            out.update({f"{name}_{key}": value for key, value in _snap(st).items()})
        assert a.timestep == b.timestep == 21
        if first is None:
            first = out
        else:
            _assert_same(first, out, f"{lanes} lanes against 1")


# ---- 7. sampling --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec,R,cut", _pops((GLASS_BOARDS, BOARD_R), (["cubic:6"], PACKED_R)))
def test_sampling(capi, exact, oracle, monkeypatch, spec, R, cut):
    fam = _family(spec, capi, exact, oracle, monkeypatch)

    def body(st):
        energies, states = st.run_sampling(0.5, 9, 3, 4)
        snap = _snap(st)
        snap.update(sample_energies=_bits(energies), sample_states=states)
        return snap, None

    st, _, _ = _on_lanes(fam, _seeds(capi, 7000, R, cut), cut, body)
    assert st.timestep == 9 + 3 * 4


# ---- 8. per-step energies: the calls that ignore the forced lanes, between calls that take them ----------------------------
@pytest.mark.parametrize("spec,R,cut", _pops((GLASS_BOARDS, BOARD_R[2:]), (["cubic:6"], PACKED_R[:2]), (["real"], REAL_R[:1])))
def test_per_step_energies_between_lane_calls(capi, exact, oracle, monkeypatch, spec, R, cut):
    fam = _family(spec, capi, exact, oracle, monkeypatch)

    def body(st):
        before = st.do_time_steps(9, 0.5, per_step_energies=True)
        st.do_time_steps(50, 0.5)
        after = st.do_time_steps(9, 0.5, per_step_energies=True)
        snap = _snap(st)
        snap.update(before=_bits(before), after=_bits(after))
        return snap, None

    _on_lanes(fam, _seeds(capi, 8000, R, cut), cut, body)


# ---- the multi-class kernels: plain sweeps only (the newer features refuse these lattices) -----------------------------------
@pytest.mark.parametrize("R", [2, 5, 40])
@pytest.mark.parametrize("spec", ["field:256x4", "open:256x4", "field:64x4", "open:64x4"])
def test_multi_class_lattices(capi, exact, oracle, monkeypatch, spec, R):
    fam = _family(spec, capi, exact, oracle, monkeypatch)
    seeds = capi.make_seeds(9000 + R, R)
    T, beta = 50, 0.6

    def body(st):
        st.do_time_steps(T, beta)
        return dict(_snap(st), magnetisations=st.magnetisations()), None

    st, _, _ = _on_lanes(fam, seeds, None, body)
    if fam.lat is not None:   # oracle engine B, field and missing bonds included
        ref = [fam.lat.init(s) for s in seeds]
        for r, s in enumerate(seeds):
            for t in range(T):
                fam.lat.sweep(ref[r], s, t, beta)
        assert np.array_equal(st.packed(), np.stack(ref))
        assert np.array_equal(st.energies(), [fam.lat.energy_mag(x)[0] for x in ref])
    else:   # the f64 CSR family: configurations against the general oracle (its energies are sums in another order)
        ea, eb, ej = fam.edges
        spins = st.states()
        for r, s in enumerate(seeds):
            assert np.array_equal(spins[r].astype(np.uint8), oracle.gen_run(ea, eb, ej, fam.g.nvars, int(s), [beta] * T, biases=fam.biases)[1])


# ---- 9. a sequence fuzz ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec,R", [("board:64x4:uniform", 5), ("cubic:6", 62), ("real", 37)])
def test_call_sequences_on_changing_lanes(capi, exact, oracle, monkeypatch, spec, R):
    """30 seeded operations on a container whose lane count changes between the calls and on a one-lane twin, compared after
    every operation.  (62 bit-sliced experiments: the appends open a third replica group.)"""
    fam = _family(spec, capi, exact, oracle, monkeypatch)
    rng = np.random.default_rng(R)
    seeds = capi.make_seeds(9500, R)
    pair = [fam.make(seeds, 3), fam.make(seeds, 1)]
    can_cluster = not fam.real
    kinds = ["steps"] * 6 + ["icm", "track", "track", "best_update", "best_reset", "set_state", "append", "streams", "streams"] + ["cluster"] * can_cluster
    track, records, appended = 0, False, 0
    for i in range(30):
        kind = "steps" if i == 0 else str(rng.choice(kinds))
        if kind == "steps":
            n, beta = int(rng.integers(1, 25)), float(rng.choice([0.2, 0.44, 0.9]))
            for st in pair:
                st.do_time_steps(n, beta)
        elif kind in ("cluster", "icm"):
            k = int(rng.choice([0, 1, 3, 7] if kind == "cluster" else [0, 2, 5]))
            for st in pair:   # one non-local move at a time
                st.set_icm_every(0)
                st.set_cluster_every(k if kind == "cluster" else 0)
                st.set_icm_every(k if kind == "icm" else 0)
        elif kind == "track":
            track = int(rng.choice([0, 1, 3, 16]))
            records = records or track > 0
            for st in pair:
                st.set_track_best(track)
        elif kind == "best_update":
            records = True
            for st in pair:
                st.best_update()
        elif kind == "best_reset":
            for st in pair:
                st.best_reset()
        elif kind == "set_state":
            r, spins = int(rng.integers(0, pair[0].count)), rng.integers(0, 2, fam.g.nvars).astype(np.uint8)
            for st in pair:
                st.set_state(r, spins)
        elif kind == "append":
            if track or appended >= 4:   # refused while tracking is on (the records are sized for the replicas held)
                continue
            appended, records = appended + 1, False
            for st in pair:
                st.append(9600 + appended)
        else:
            pair[0].set_option("streams" if fam.family == "checkerboard" else "pk_streams", int(rng.choice(LANES)))
        _assert_same(_snap(pair[0], best=records), _snap(pair[1], best=records), f"operation {i} ({kind})")
    assert pair[0].timestep > 30

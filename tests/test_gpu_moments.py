"""Per-site spin sums and per-bond sums on the device against a twin: a container with the same graph and seeds is
driven from sample point to sample point through the existing calls and read with get_states(); tests/moments_reference.py sums
what it returns.  The tracked container runs one long call, so the cutting of the stretch is under test too.  Everything is
compared exactly.

(The issue asks for a checkerboard run on an edge list with a duplicated and a zero-J entry.  The lattice recogniser takes no such
list -- every bond once, one |J| per direction -- so that list is run where the library serves it, on the real-coupling packed
family; the checkerboard path's own edge table is exercised by a shuffled edge list instead.)"""
import json
import os

import numpy as np
import pytest

import moments_reference as MR
import packed_icm_reference as IR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _drive_twin(twin, acc, timesteps, beta, every, t0):
    """`timesteps` steps of the twin, `every` at a time counted from t0; a sample after each full period"""
    k = 0
    while k < timesteps:
        m = min(timesteps - k, every - (twin.timestep - t0) % every) if every else timesteps - k
        twin.do_time_steps(m, beta)
        k += m
        if every and (twin.timestep - t0) % every == 0:
            acc.add(twin.states())


def _assert_sums(st, acc, bonds):
    n, site, bond = st.moments()
    assert n == acc.n
    assert site.dtype == np.int64 and np.array_equal(site, acc.site)
    if bonds:
        assert bond.dtype == np.int64 and np.array_equal(bond, acc.bond)
    else:
        assert bond is None


def _assert_same_container(a, b):
    assert a.timestep == b.timestep
    assert np.array_equal(_bits(a.energies()), _bits(b.energies()))
    assert np.array_equal(a.raw_state(), b.raw_state())


def _track_and_compare(make, ea, eb, every, timesteps, beta, per_replica=False, bonds=False, prepare=lambda st: None):
    """a tracked container in one call, its twin in pieces, an untracked container in one call"""
    st, twin, plain = make(), make(), make()
    for c in (st, twin, plain):
        prepare(c)
    st.set_moments_every(every, per_replica=per_replica, bonds=bonds)
    assert st.moments_every == (every, per_replica, bonds)
    st.do_time_steps(timesteps, beta)
    plain.do_time_steps(timesteps, beta)
    acc = MR.Accumulator(ea, eb, per_replica)
    _drive_twin(twin, acc, timesteps, beta, every, 0)
    assert acc.n == timesteps // every
    _assert_sums(st, acc, bonds)
    _assert_same_container(st, twin)
    _assert_same_container(st, plain)
    return st


def _glass(exact, W=128, H=6, seed=5):
    return exact.square_lattice_edges(W, H, -1.0, np.random.default_rng(seed))


# ---- checkerboard lattice ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("R", [3, 300])   # 300: more replicas than one register chunk of the summed kernel (2^8 - 1)
def test_lattice_summed_with_bonds(capi, exact, R, shuffled):
    ea, eb, ej = _glass(exact)   # 128 x 6: two words per row
    if shuffled:   # another order and orientation of the entries: the host's edge table
        perm = np.random.default_rng(1).permutation(len(ea))
        flip = np.random.default_rng(2).random(len(ea)) < 0.5
        ea, eb, ej = np.where(flip, eb, ea)[perm], np.where(flip, ea, eb)[perm], ej[perm]
    g = capi.Graph(ea, eb, ej)
    assert g.kind == capi.KIND_LATTICE2D
    st = _track_and_compare(lambda: capi.States(g, capi.make_seeds(11, R)), ea, eb, 2, 7, 0.5, bonds=True)
    assert st.family == "checkerboard"


def test_lattice_summed_sites_alone(capi, exact):
    ea, eb, ej = _glass(exact)
    g = capi.Graph(ea, eb, ej)
    st = _track_and_compare(lambda: capi.States(g, capi.make_seeds(12, 5)), ea, eb, 3, 7, 0.4)
    with pytest.raises(ValueError, match="no bond sums"):
        bond = np.zeros(g.n_edges, dtype=np.int64)
        capi._check(capi.lib().isingmc_moments_get(st._h, None, None, bond.ctypes.data_as(capi.C.c_void_p)))


@pytest.mark.parametrize("planes,samples", [(2, 8), (None, 3)])   # K = 2: two flushes and a remainder that moments() flushes
def test_lattice_per_replica(capi, exact, planes, samples):
    ea, eb, ej = _glass(exact)
    g = capi.Graph(ea, eb, ej)

    def prepare(st):
        if planes:
            st.set_option("moments_planes", planes)
    _track_and_compare(lambda: capi.States(g, capi.make_seeds(13, 5)), ea, eb, 1, samples, 0.5, per_replica=True, prepare=prepare)


# ---- replica-packed families ---------------------------------------------------------------------------------------------------
def test_packed_bit_sliced_and_a_shard(capi, exact, monkeypatch):
    monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
    ea, eb, ej = IR.cubic_glass(exact, 6)
    g = capi.Graph(ea, eb, ej, nvars=216, force_general=True)
    whole = lambda: capi.States(g, capi.make_seeds(207, 40))                            # the second group owns 8 bits
    shard = lambda: capi.States(g, capi.make_seeds(207, 50), replica_range=(5, 45))     # pk_bit0 = 5, 40 replicas
    for make in (whole, shard):
        st = _track_and_compare(make, ea, eb, 2, 6, 0.6, bonds=True)
        assert st.family == "packed_bitsliced" and st.count == 40

        def planes2(c):
            c.set_option("moments_planes", 2)
        _track_and_compare(make, ea, eb, 1, 7, 0.6, per_replica=True, prepare=planes2)   # two flushes and a remainder
    # the unowned bits of the shard's groups are simulated (a shard runs whole groups) and must not count: the twin cannot see them


def test_packed_real_with_a_self_loop(capi, exact, monkeypatch):
    monkeypatch.setenv("ISINGMC_FORCE_REAL", "1")
    ea, eb, _ = exact.square_lattice_edges(12, 12, -1.0)
    rng = np.random.default_rng(2024)
    ea, eb = np.append(ea, 17).astype(np.uint64), np.append(eb, 17).astype(np.uint64)   # an entry a == b
    g = capi.Graph(ea, eb, rng.normal(size=len(ea)), nvars=144, biases=rng.normal(size=144), force_general=True)
    st = _track_and_compare(lambda: capi.States(g, capi.make_seeds(300, 33)), ea, eb, 2, 6, 0.7, bonds=True)
    assert st.family == "packed_real"
    n, _, bond = st.moments()
    assert bond[-1] == n * 33
    _track_and_compare(lambda: capi.States(g, capi.make_seeds(300, 33)), ea, eb, 1, 4, 0.7, per_replica=True)


def test_duplicated_and_zero_coupling_entries(capi, exact, monkeypatch):
    """the 128 x 6 list with one entry twice and one entry of J = 0 between two sites that share no other bond"""
    monkeypatch.setenv("ISINGMC_FORCE_REAL", "1")
    ea, eb, ej = _glass(exact)
    ea, eb, ej = np.append(ea, [ea[10], 0]).astype(np.uint64), np.append(eb, [eb[10], 200]).astype(np.uint64), np.append(ej, [ej[10], 0.0])
    g = capi.Graph(ea, eb, ej, nvars=768, force_general=True)
    st = _track_and_compare(lambda: capi.States(g, capi.make_seeds(301, 3)), ea, eb, 2, 6, 0.5, bonds=True)
    assert st.family == "packed_real"
    bond = st.moments()[2]
    assert bond[10] == bond[-2]


# ---- cluster periods -----------------------------------------------------------------------------------------------------------
def test_with_swendsen_wang_steps(capi, exact):
    ea, eb, ej = exact.square_lattice_edges(128, 6, -1.0)
    g = capi.Graph(ea, eb, ej)
    _track_and_compare(lambda: capi.States(g, capi.make_seeds(21, 4)), ea, eb, 2, 9, 0.4, bonds=True, prepare=lambda st: st.set_cluster_every(3))


def test_with_isoenergetic_moves(capi, exact):
    ea, eb, ej = _glass(exact)
    g = capi.Graph(ea, eb, ej)
    _track_and_compare(lambda: capi.States(g, capi.make_seeds(22, 4)), ea, eb, 2, 9, 0.8, bonds=True, prepare=lambda st: st.set_icm_every(2))


# ---- the sums against the energies -----------------------------------------------------------------------------------------------
def test_energy_identity(capi, exact):
    """The library's energy is E = sum_e J_e s_a s_b (J < 0 ferromagnetic, as in tests/golden/kaufman.json): the bond sums weighted
    with the couplings are the energies of the sampled timesteps, summed over timesteps and replicas.  Both sides are integers."""
    ea, eb, ej = _glass(exact)
    g = capi.Graph(ea, eb, ej)
    st = capi.States(g, capi.make_seeds(31, 6))
    every, T = 3, 14
    st.set_moments_every(every, bonds=True)
    e = st.do_time_steps(T, 0.6, per_step_energies=True)   # [R, T]: the energy after every timestep
    n, _, bond = st.moments()
    assert n == T // every
    sampled = e[:, every - 1::every]
    assert sampled.shape == (6, n)
    assert int(np.dot(ej.astype(np.int64), bond)) == int(np.rint(sampled).astype(np.int64).sum()) and np.array_equal(sampled, np.rint(sampled))


def test_kaufman_energy_from_the_bond_sums(capi, exact):
    """A 64 x 16 ferromagnetic torus at the critical beta of tests/golden/kaufman.json, 64 replicas: the energy per site from the
    bond sums against Kaufman's exact value, within 5 standard errors; the standard error from the spread of the per-replica means
    of the same samples' energies across the replicas.  Seeded: deterministic."""
    with open(os.path.join(ROOT, "tests", "golden", "kaufman.json")) as f:
        beta = [c["beta"] for c in json.load(f)["cases"] if c["W"] == 64][-1]
    assert beta == 0.4407
    W, H, R, every, T = 64, 16, 64, 10, 2000
    ea, eb, ej = exact.square_lattice_edges(W, H, -1.0)
    g = capi.Graph(ea, eb, ej)
    st = capi.States(g, capi.make_seeds(41, R))
    st.do_time_steps(2000, beta)   # thermalised
    st.set_moments_every(every, bonds=True)
    e = st.do_time_steps(T, beta, per_step_energies=True)
    n, _, bond = st.moments()
    N = W * H
    assert n == T // every
    got = float(ej[0]) * float(bond.sum()) / (n * R * N)   # -J sum_e bond[e] / (n R N) with the ferromagnetic strength J = -ej = 1
    means = e[:, every - 1::every].mean(axis=1) / N                  # per replica
    stderr = means.std(ddof=1) / np.sqrt(R)
    want = exact.kaufman_energy(W, H, beta) / N
    print(f"energy per site {got:.6f}, exact {want:.6f}, standard error {stderr:.6f}, z {(got - want) / stderr:+.2f}")
    assert abs(got - means.mean()) < 1e-12   # the same samples
    assert abs(got - want) < 5 * stderr


# ---- bookkeeping ---------------------------------------------------------------------------------------------------------------
def test_bookkeeping(capi, exact):
    ea, eb, ej = _glass(exact)
    g = capi.Graph(ea, eb, ej)
    seeds = capi.make_seeds(51, 4)
    st, twin = capi.States(g, seeds), capi.States(g, seeds)
    acc = MR.Accumulator(ea, eb)
    with pytest.raises(ValueError, match="holds no moment sums"):
        st.moments()
    assert st.moments_every == (0, False, False)
    # by hand, never switched on: sites alone
    for c in (st, twin):
        c.do_time_steps(3, 0.5)
    st.accumulate_moments()
    acc.add(twin.states())
    _assert_sums(st, acc, False)
    # switched on with bonds: other sums, from zero; t0 = 3
    st.set_moments_every(2, bonds=True)
    acc.reset()
    st.do_time_steps(3, 0.5)           # samples at t = 5
    st.do_time_steps(4, 0.7)           # ... 7, 9 across the calls
    _drive_twin(twin, acc, 3, 0.5, 2, 3)
    _drive_twin(twin, acc, 4, 0.7, 2, 3)
    assert acc.n == 3
    _assert_sums(st, acc, True)
    st.accumulate_moments()            # t = 10: off the period
    acc.add(twin.states())
    _assert_sums(st, acc, True)
    # off: the sums stay and nothing is added
    st.set_moments_every(0)
    assert st.moments_every == (0, False, True)
    st.do_time_steps(4, 0.5)
    twin.do_time_steps(4, 0.5)
    _assert_sums(st, acc, True)
    # on again with the same flags: goes on counting, from the new t0 = 14
    st.set_moments_every(3, bonds=True)
    st.do_time_steps(4, 0.5)           # sample at t = 17
    _drive_twin(twin, acc, 4, 0.5, 3, 14)
    assert acc.n == 5
    _assert_sums(st, acc, True)
    # the timestep set by hand re-bases t0
    for c in (st, twin):
        c.timestep = 100
    st.do_time_steps(7, 0.5)           # samples at 103, 106
    _drive_twin(twin, acc, 7, 0.5, 3, 100)
    assert acc.n == 7
    _assert_sums(st, acc, True)
    st.reset_moments()
    acc.reset()
    n, site, bond = st.moments()
    assert n == 0 and not site.any() and not bond.any()
    st.do_time_steps(2, 0.5)           # t = 109: (109 - 100) % 3 == 0
    _drive_twin(twin, acc, 2, 0.5, 3, 100)
    assert acc.n == 1
    _assert_sums(st, acc, True)
    _assert_same_container(st, twin)


def test_sampling_run(capi, exact):
    """isingmc_run_sampling_moments takes the samples of isingmc_run_sampling"""
    ea, eb, ej = _glass(exact)
    g = capi.Graph(ea, eb, ej)
    seeds = capi.make_seeds(52, 4)
    st, twin = capi.States(g, seeds), capi.States(g, seeds)
    e = st.run_sampling_moments(0.5, 3, 2, 5, bonds=True)
    e_ref, states = twin.run_sampling(0.5, 3, 2, 5)   # [R, S], [R, S, N]
    assert st.moments_every == (0, False, True)
    n, site, bond = st.moments()
    samples = np.swapaxes(states, 0, 1)
    assert n == 5 and np.array_equal(site, MR.site_sums(samples)) and np.array_equal(bond, MR.bond_sums(samples, ea, eb))
    assert np.array_equal(_bits(e), _bits(e_ref[:, -1]))
    _assert_same_container(st, twin)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _unchanged(st, before):
    assert (st.timestep, st.moments_every) == before[:2] and np.array_equal(st.raw_state(), before[2])


def _snapshot(st):
    return st.timestep, st.moments_every, st.raw_state()


def test_refusals(capi, exact):
    ea, eb, ej = _glass(exact)
    g = capi.Graph(ea, eb, ej)
    seeds = capi.make_seeds(61, 4)
    st = capi.States(g, seeds)
    st.do_time_steps(2, 0.5)
    before = _snapshot(st)
    with pytest.raises(ValueError, match="per replica are not offered"):
        st.set_moments_every(1, per_replica=True, bonds=True)
    _unchanged(st, before)
    st.set_option("moments_bytes", 1000)
    with pytest.raises(ValueError, match="moments_bytes"):
        st.set_moments_every(1)
    with pytest.raises(ValueError, match="moments_bytes"):
        st.accumulate_moments()
    _unchanged(st, before)
    st.set_option("moments_bytes", 256 * g.state_words)       # the site sums fit exactly; bonds and per-replica totals do not
    with pytest.raises(ValueError, match="moments_bytes"):
        st.set_moments_every(1, bonds=True)
    with pytest.raises(ValueError, match="32 times the state"):
        st.set_moments_every(1, per_replica=True)
    st.set_option("moments_planes", 17)
    st.set_option("moments_bytes", 1 << 30)
    with pytest.raises(ValueError, match="moments_planes"):
        st.set_moments_every(1, per_replica=True)
    _unchanged(st, before)
    # a ladder attached
    ladder = capi.States(g, seeds)
    ladder.pt_attach(np.linspace(0.2, 0.8, 4), 0, 4, 1, 7)
    with pytest.raises(ValueError, match="ladder is attached"):
        ladder.set_moments_every(1)
    assert ladder.moments_every == (0, False, False)
    # ... and the calls refused while accumulation is on
    st.set_moments_every(2)
    before = _snapshot(st)
    with pytest.raises(ValueError, match="moment sums are switched on"):
        st.pt_attach(np.linspace(0.2, 0.8, 4), 0, 4, 1, 7)
    with pytest.raises(ValueError, match="moment sums are switched on"):
        st.pa_run([0.2, 0.4], 2, 9)
    with pytest.raises(ValueError, match="moment sums are switched on"):
        st.pa_resample(0.1, 9, 1)
    with pytest.raises(ValueError, match="moment sums are switched on"):
        st.append(12345)
    with pytest.raises(ValueError, match="switched on for this container already"):
        st.run_sampling_moments(0.5, 1, 1, 1)
    _unchanged(st, before)
    assert st.count == 4 and st.moments()[0] == 0


def test_refused_on_the_csr_family(capi, exact, monkeypatch):
    monkeypatch.setenv("ISINGMC_DISABLE_PACKED", "1")
    monkeypatch.setenv("ISINGMC_DISABLE_REAL", "1")
    ea, eb, ej = IR.cubic_glass(exact, 6)
    g = capi.Graph(ea, eb, ej, nvars=216, force_general=True)
    st = capi.States(g, capi.make_seeds(62, 3))
    assert st.family == "csr_f64"
    before = _snapshot(st)
    for call in (lambda: st.set_moments_every(1), st.accumulate_moments, lambda: st.run_sampling_moments(0.5, 1, 1, 1)):
        with pytest.raises(ValueError, match="f64 CSR"):
            call()
    _unchanged(st, before)


def test_refused_with_a_field(capi, exact):
    ea, eb, ej = exact.square_lattice_edges(256, 4, -1.0)   # (the field kernels want whole quads per row)
    g = capi.Graph(ea, eb, ej, biases=np.full(1024, 0.25))
    assert g.kind == capi.KIND_LATTICE2D and g.info.fast_path != 0
    st = capi.States(g, capi.make_seeds(63, 3))
    with pytest.raises(ValueError, match="field"):
        st.set_moments_every(1)


# ---- the Python classes ----------------------------------------------------------------------------------------------------------
def _edge_list(ea, eb, ej):
    return [((int(a), int(b)), float(j)) for a, b, j in zip(ea, eb, ej)]


def test_lattice_run_monte_carlo_and_measure_spins(exact):
    import py_monte_carlo
    ea, eb, ej = _glass(exact)
    R, S, freq, therm = 4, 5, 2, 3
    lat = py_monte_carlo.Lattice(_edge_list(ea, eb, ej), seed_gen=77)
    e_ref, states = lat.run_monte_carlo_sampling(0.5, S * freq, R, thermalization_time=therm, sampling_freq=freq)
    spins = 2.0 * states.astype(np.float64) - 1.0   # [R, S, N]
    e, mean = lat.run_monte_carlo_and_measure_spins(0.5, S * freq, R, thermalization_time=therm, sampling_freq=freq)
    assert mean.dtype == np.float64 and mean.shape == (R, 768)
    assert np.array_equal(mean, spins.sum(axis=1) / S)
    assert np.array_equal(_bits(e), _bits(e_ref[:, -1]))
    e, mean, bonds = lat.run_monte_carlo_and_measure_spins(0.5, S * freq, R, thermalization_time=therm, sampling_freq=freq, per_experiment=False, bonds=True)
    assert mean.shape == (768,) and np.array_equal(mean, spins.sum(axis=(0, 1)) / (S * R))
    a, b = ea.astype(np.int64), eb.astype(np.int64)
    assert bonds.shape == (len(ea),) and np.array_equal(bonds, (spins[:, :, a] * spins[:, :, b]).sum(axis=(0, 1)) / (S * R))
    assert np.array_equal(_bits(e), _bits(e_ref[:, -1]))


def test_classic_ising_measured_spins(exact):
    import py_monte_carlo
    ea, eb, ej = _glass(exact)
    ci, twin = (py_monte_carlo.ClassicIsing(_edge_list(ea, eb, ej), None, 3, 21) for _ in range(2))
    ci.set_measure_spins_every(2, bonds=True)
    ci.run_monte_carlo(0.5, 6)
    acc = MR.Accumulator(ea, eb)
    for _ in range(3):
        twin.run_monte_carlo(0.5, 2)
        acc.add(twin.get_states())
    n, site, bond = ci.get_measured_spins()
    assert n == 3 and np.array_equal(site, acc.site) and np.array_equal(bond, acc.bond)
    with pytest.raises(ValueError, match="moment sums are switched on"):
        ci.add_graph()
    ci.reset_measured_spins()
    assert ci.get_measured_spins()[0] == 0
    ci.set_measure_spins_every(1, per_experiment=True)
    ci.run_monte_carlo(0.5, 2)
    n, site, bond = ci.get_measured_spins()
    assert n == 2 and site.shape == (3, 768) and bond is None

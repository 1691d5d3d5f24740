"""The lag ring on the device against a twin: a container with the same graph and seeds is driven from sample point to
sample point through the existing calls and read with states(); tests/autocorrelation_reference.py applies the rule to what it
returns.  The container with the ring runs one long call, so the cutting of the stretch is under test too, and a plain container
without a ring shows that the ring perturbs nothing.  Counts and sums are compared as integers.

The checkerboard kernel does not tile its lags (an LDS counter per lag, up to 256), so there is no "tile width + 1" case for it; the
packed kernel gathers ACR_PK_LAG_TILE = 8 lags in LDS at a time, and L = 9 crosses that tile.  A workgroup of the checkerboard kernel
covers 256 x ACR_LAT_WORDS = 1024 state words of a replica: 64 x 516 has 1032 (a plane of the checkerboard path is a multiple of
four words, a replica's words of eight: one word more does not exist).  A workgroup of the packed kernel covers 256 x ACR_PK_ITER = 2048 positions: 14^3 has 3072.  Neither
launcher splits a grid below 2^20 replicas, so no case for that."""
import numpy as np
import pytest

import autocorrelation_reference as AR
import packed_icm_reference as IR

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _glass(exact, W=128, H=6, seed=5):
    return exact.square_lattice_edges(W, H, -1.0, np.random.default_rng(seed))


def _drive_twin(twin, ring, timesteps, beta, every, t0):
    """`timesteps` steps of the twin, cut at the sample points counted from t0; a sample after each full period"""
    k = 0
    while k < timesteps:
        m = min(timesteps - k, every - (twin.timestep - t0) % every) if every else timesteps - k
        twin.do_time_steps(m, beta)
        k += m
        if every and (twin.timestep - t0) % every == 0:
            ring.add(twin.states())


def _assert_ring(ac, ring):
    counts, diff = ac.get()
    assert ac.samples == ring.samples and ac.n_lags == ring.L
    assert counts.dtype == np.uint64 and diff.dtype == np.uint64 and diff.shape == (ring.R, ring.L + 1)
    assert np.array_equal(counts, ring.counts)
    assert np.array_equal(diff, ring.diff), np.argwhere(diff != ring.diff)[:8]
    assert not diff[:, 0].any() and not diff[:, counts == 0].any()


def _assert_same_container(a, b):
    assert a.timestep == b.timestep
    assert np.array_equal(_bits(a.energies()), _bits(b.energies()))
    assert np.array_equal(a.raw_state(), b.raw_state())


def _track_and_compare(make, L, every, timesteps, beta, prepare=lambda st: None):
    """a container with the ring in one call, its twin in pieces, a plain container in one call"""
    st, twin, plain = make(), make(), make()
    for c in (st, twin, plain):
        prepare(c)
    ac = st.autocorrelation(L)
    ac.set_every(every)
    st.do_time_steps(timesteps, beta)
    plain.do_time_steps(timesteps, beta)
    ring = AR.LagRing(L, st.count)
    _drive_twin(twin, ring, timesteps, beta, every, 0)
    assert ring.samples == timesteps // every
    _assert_ring(ac, ring)
    _assert_same_container(st, twin)
    _assert_same_container(st, plain)
    return st, ac


# ---- checkerboard lattice ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,every,timesteps", [(4, 2, 13),    # 6 samples: the ring wraps
                                               (8, 2, 7),     # 3 samples: lags 3 .. 8 unreached, n_l = 0 and sums 0
                                               (1, 1, 5)])    # one slot: every sample replaces the snapshot it was compared with
def test_lattice(capi, exact, L, every, timesteps):
    g = capi.Graph(*_glass(exact))   # 128 x 6: two words per row
    assert g.kind == capi.KIND_LATTICE2D
    st, _ = _track_and_compare(lambda: capi.States(g, capi.make_seeds(11, 3)), L, every, timesteps, 0.5)
    assert st.family == "checkerboard"


def test_lattice_of_more_words_than_one_workgroup(capi, exact):
    g = capi.Graph(*exact.square_lattice_edges(64, 516, -1.0, np.random.default_rng(6)))   # 2 x 516 words per replica: 1024 + 8
    assert g.kind == capi.KIND_LATTICE2D and g.info.state_words == 1032
    _track_and_compare(lambda: capi.States(g, capi.make_seeds(12, 2)), 2, 1, 4, 0.45)


# ---- replica-packed families ---------------------------------------------------------------------------------------------------
def test_packed_bit_sliced_and_a_shard(capi, exact, monkeypatch):
    monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
    ea, eb, ej = IR.cubic_glass(exact, 6)
    g = capi.Graph(ea, eb, ej, nvars=216, force_general=True)
    whole = lambda: capi.States(g, capi.make_seeds(207, 40))                            # the second group owns 8 bits
    shard = lambda: capi.States(g, capi.make_seeds(207, 50), replica_range=(5, 45))     # pk_bit0 = 5, 40 replicas
    for make in (whole, shard):
        st, _ = _track_and_compare(make, 4, 2, 13, 0.6)
        assert st.family == "packed_bitsliced" and st.count == 40
    _track_and_compare(shard, 9, 1, 12, 0.6)   # nine lags: one more than the LDS tile of the packed kernel; the ring wraps
    # the unowned bits of the shard's groups are simulated (a shard runs whole groups) and must not count: the twin cannot see them


def test_packed_of_more_positions_than_one_workgroup(capi, exact, monkeypatch):
    monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
    ea, eb, ej = IR.cubic_glass(exact, 14)
    g = capi.Graph(ea, eb, ej, nvars=2744, force_general=True)   # two colour classes of 1372 sites, padded to 1536 positions each
    st, _ = _track_and_compare(lambda: capi.States(g, capi.make_seeds(208, 33)), 2, 1, 4, 0.6)
    assert st.family == "packed_bitsliced"


def test_packed_real(capi, exact, monkeypatch):
    monkeypatch.setenv("ISINGMC_FORCE_REAL", "1")
    ea, eb, _ = exact.square_lattice_edges(12, 12, -1.0)
    rng = np.random.default_rng(2024)
    g = capi.Graph(ea, eb, rng.normal(size=len(ea)), nvars=144, biases=rng.normal(size=144), force_general=True)
    st, _ = _track_and_compare(lambda: capi.States(g, capi.make_seeds(300, 33)), 4, 2, 13, 0.7)
    assert st.family == "packed_real"


# ---- non-local steps: a sample follows whatever kind of timestep it is ----------------------------------------------------------
def test_with_swendsen_wang_steps(capi, exact):
    g = capi.Graph(*exact.square_lattice_edges(128, 6, -1.0))
    _track_and_compare(lambda: capi.States(g, capi.make_seeds(21, 4)), 3, 1, 9, 0.4, prepare=lambda st: st.set_cluster_every(3))


def test_with_isoenergetic_moves(capi, exact):
    g = capi.Graph(*_glass(exact))
    _track_and_compare(lambda: capi.States(g, capi.make_seeds(22, 4)), 3, 2, 9, 0.8, prepare=lambda st: st.set_icm_every(2))


# ---- exact physics, no tolerance --------------------------------------------------------------------------------------------------
def _every_spin_flips(st, N):
    """beta = 0: every proposal is accepted outright, so a timestep flips every spin"""
    L, T = 5, 8
    ac = st.autocorrelation(L)
    ac.set_every(1)
    st.do_time_steps(T, 0.0)
    counts, diff = ac.get()
    assert list(counts) == [T - l for l in range(L + 1)]
    for l in range(L + 1):
        assert np.all(diff[:, l] == (int(counts[l]) * N if l % 2 else 0)), l


def test_beta_zero_lattice(capi, exact):
    g = capi.Graph(*_glass(exact))
    _every_spin_flips(capi.States(g, capi.make_seeds(31, 3)), 768)


def test_beta_zero_packed(capi, exact, monkeypatch):
    monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
    g = capi.Graph(*IR.cubic_glass(exact, 6), nvars=216, force_general=True)
    _every_spin_flips(capi.States(g, capi.make_seeds(32, 50), replica_range=(5, 45)), 216)


# ---- bookkeeping ---------------------------------------------------------------------------------------------------------------
def test_bookkeeping(capi, exact):
    g = capi.Graph(*_glass(exact))
    seeds = capi.make_seeds(51, 4)
    st, twin = capi.States(g, seeds), capi.States(g, seeds)
    ac, ring = st.autocorrelation(3), AR.LagRing(3, 4)
    assert (ac.samples, ac.n_lags) == (0, 3)
    _assert_ring(ac, ring)
    # by hand, no period
    for c in (st, twin):
        c.do_time_steps(3, 0.5)
    ac.sample()
    ring.add(twin.states())
    _assert_ring(ac, ring)
    # a period from t0 = 3, the run cut into three calls
    ac.set_every(2)
    for n, beta in ((3, 0.5), (4, 0.7), (2, 0.5)):   # samples at t = 5 | 7, 9 | 11
        st.do_time_steps(n, beta)
        _drive_twin(twin, ring, n, beta, 2, 3)
    assert ring.samples == 5
    _assert_ring(ac, ring)
    ac.sample()                          # t = 12: off the period
    ring.add(twin.states())
    _assert_ring(ac, ring)
    # off: ring and sums stay and nothing is added
    ac.set_every(0)
    for c in (st, twin):
        c.do_time_steps(4, 0.5)
    _assert_ring(ac, ring)
    # a reset in the middle: sums and sample number to 0; the period stays (none here), the next samples start a new ring
    ac.reset()
    ring.reset()
    _assert_ring(ac, ring)
    ac.set_every(3)                      # t0 = 16
    st.do_time_steps(7, 0.5)             # samples at 19, 22
    _drive_twin(twin, ring, 7, 0.5, 3, 16)
    assert ring.samples == 2
    _assert_ring(ac, ring)
    # the timestep set by hand restarts the sample points; the ring goes on
    for c in (st, twin):
        c.timestep = 100
    st.do_time_steps(7, 0.5)             # samples at 103, 106
    _drive_twin(twin, ring, 7, 0.5, 3, 100)
    assert ring.samples == 4
    _assert_ring(ac, ring)
    ac.reset()                           # with the period on: it stays
    ring.reset()
    st.do_time_steps(2, 0.5)             # t = 109: (109 - 100) % 3 == 0
    _drive_twin(twin, ring, 2, 0.5, 3, 100)
    assert ring.samples == 1
    _assert_ring(ac, ring)
    _assert_same_container(st, twin)
    # a second ring only after the first has gone
    with pytest.raises(ValueError, match="one ring per container"):
        st.autocorrelation(2)
    ac.close()
    st.autocorrelation(2).close()


def test_sampling_runs_take_samples_too(capi, exact):
    """a ring's period inside isingmc_run_sampling and isingmc_run_sampling_moments; isingmc_run_sampling_autocorr takes the samples
    of isingmc_run_sampling"""
    g = capi.Graph(*_glass(exact))
    seeds = capi.make_seeds(52, 4)
    for run in (lambda c: c.run_sampling(0.5, 3, 2, 5), lambda c: c.run_sampling_moments(0.5, 3, 2, 5)):
        st, plain = capi.States(g, seeds), capi.States(g, seeds)
        ac = st.autocorrelation(4)
        ac.set_every(3)                  # t0 = 0; 13 timesteps: samples at 3, 6, 9, 12
        run(st)
        _, states = capi.States(g, seeds).run_sampling(0.5, 0, 3, 4)   # the configurations at 3, 6, 9, 12: [R, S, N]
        run(plain)
        counts, diff = ac.get()
        r_counts, r_diff = AR.diff_from_samples(states, 4)
        assert ac.samples == 4 and np.array_equal(counts, r_counts) and np.array_equal(diff, r_diff)
        _assert_same_container(st, plain)
    st, twin = capi.States(g, seeds), capi.States(g, seeds)
    ac = st.autocorrelation(3)
    ac.sample()                          # (the run resets the ring first)
    e = ac.run_sampling(0.5, 3, 2, 5, site_sums=True)
    e_ref, states = twin.run_sampling(0.5, 3, 2, 5)
    counts, diff = ac.get()
    r_counts, r_diff = AR.diff_from_samples(states, 3)
    assert ac.samples == 5 and np.array_equal(counts, r_counts) and np.array_equal(diff, r_diff)
    n, site, _ = st.moments()
    assert n == 5 and np.array_equal(site, 2 * states.astype(np.int64).sum(axis=1) - 5)
    assert st.moments_every[0] == 0 and np.array_equal(_bits(e), _bits(e_ref[:, -1]))
    _assert_same_container(st, twin)
    st.do_time_steps(4, 0.5)             # the run's period is off again
    assert ac.samples == 5


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _snapshot(st):
    return st.timestep, st.count, st.raw_state()


def _unchanged(st, before):
    assert (st.timestep, st.count) == before[:2] and np.array_equal(st.raw_state(), before[2])


def test_refusals(capi, exact):
    W, H = 256, 4   # (fields, open boundaries and anisotropy stay on the checkerboard path from 256 columns on)
    N = W * H
    ea, eb, ej = exact.square_lattice_edges(W, H, -1.0)
    x = np.arange(N) % W
    right = np.arange(len(ea)) % 2 == 0
    seeds = capi.make_seeds(61, 4)
    cases = {
        "f64 CSR": capi.Graph(*exact.cubic_lattice_edges(6), 216),   # a small graph without the force flag
        "field": capi.Graph(ea, eb, ej, N, biases=np.full(N, 0.5)),
        "open": capi.Graph(*[a[~(right & (np.repeat(x, 2) == W - 1))] for a in (ea, eb, ej)], N),
        "anisotropic": capi.Graph(ea, eb, np.where(right, -1.0, -2.0), N),
    }
    for reason, g in cases.items():
        st = capi.States(g, seeds[:2])
        st.do_time_steps(2, 0.5)
        before = _snapshot(st)
        with pytest.raises(ValueError, match=reason):
            st.autocorrelation(4)
        _unchanged(st, before)
    g = capi.Graph(*_glass(exact))
    st = capi.States(g, seeds)
    st.do_time_steps(2, 0.5)
    before = _snapshot(st)
    for L in (0, 257):
        with pytest.raises(ValueError, match="1 .. 256"):
            st.autocorrelation(L)
    st.set_option("autocorr_bytes", 4 * 4 * 4 * g.info.state_words)   # four snapshots of four replicas, no room for the sums
    with pytest.raises(ValueError, match="larger than the option autocorr_bytes"):
        st.autocorrelation(4)
    st.autocorrelation(3).close()
    _unchanged(st, before)
    st.set_option("autocorr_bytes", 1 << 30)
    # a ladder attached
    ladder = capi.States(g, seeds)
    ladder.pt_attach(np.linspace(0.2, 0.8, 4), 0, 4, 1, 7)
    ladder.pt_run(4, 2)
    before_ladder = _snapshot(ladder), ladder.pt_state()
    with pytest.raises(ValueError, match="ladder is attached"):
        ladder.autocorrelation(4)
    _unchanged(ladder, before_ladder[0])
    assert all(np.array_equal(x, y) for x, y in zip(ladder.pt_state(), before_ladder[1]))
    # ... and the calls refused while a ring lives, with no period on: each leaves the container, the ring and its sums as they were
    ac = st.autocorrelation(4)
    ac.sample()
    sums = ac.get()
    for call in (lambda: st.pt_attach(np.linspace(0.2, 0.8, 4), 0, 4, 1, 7), lambda: st.pa_run([0.2, 0.4], 2, 9),
                 lambda: st.pa_resample(0.1, 9, 1), lambda: st.append(12345)):
        with pytest.raises(ValueError, match="a lag ring is live"):
            call()
        _unchanged(st, before)
        assert ac.samples == 1 and all(np.array_equal(x, y) for x, y in zip(ac.get(), sums))
    ac.set_every(2)
    with pytest.raises(ValueError, match="samples on a period already"):
        ac.run_sampling(0.5, 1, 1, 1)
    _unchanged(st, before)
    assert ac.samples == 1 and all(np.array_equal(x, y) for x, y in zip(ac.get(), sums))
    ac.close()
    st.append(12345)   # the ring has gone: the container takes replicas again
    assert st.count == 5


# ---- the Python classes ----------------------------------------------------------------------------------------------------------
def _edge_list(ea, eb, ej):
    return [((int(a), int(b)), float(j)) for a, b, j in zip(ea, eb, ej)]


def test_lattice_run_monte_carlo_and_measure_variable_autocorrelation(exact):
    """connected=False: the float64 of the numpy form on the samples of run_monte_carlo_sampling, with ==.
    connected=True subtracts (1/N) sum_i <s_i>_r^2; the library adds the N = 768 squares one after another, numpy pairwise: the
    same formula, another order of the additions.  Measured on the MI355X (this test's printed line): the largest difference to the
    numpy form is 2.6e-15 at both lag counts, about 12 units of the last place of a number below 1 -- what the rounding of 768
    additions allows ((N - 1) 2^-53 = 8.5e-14 at worst, sqrt(N) 2^-53 = 3e-15 typically).  Asserted: 3e-14, that difference's order of
    magnitude above it."""
    import py_monte_carlo
    from pyisingmontecarlo_amd import correlation as K
    ea, eb, ej = _glass(exact)
    R, S, freq, therm, N = 4, 7, 2, 3, 768
    lat = py_monte_carlo.Lattice(_edge_list(ea, eb, ej), seed_gen=77)
    _, states = lat.run_monte_carlo_sampling(0.5, S * freq, R, thermalization_time=therm, sampling_freq=freq)   # [R, S, N]
    for max_lag, L in ((4, 4), (32, S - 1)):
        counts, diff = AR.diff_from_samples(states, L)
        want = K.autocorrelation(diff, counts, N)
        got = lat.run_monte_carlo_and_measure_variable_autocorrelation(0.5, S * freq, R, sampling_wait_buffer=therm, sampling_freq=freq, max_lag=max_lag)
        assert got.dtype == np.float64 and got.shape == (R, L + 1)
        assert np.array_equal(got, want) and np.all(got[:, 0] == 1.0)
        spins = 2.0 * states.astype(np.float64) - 1.0
        direct = np.stack([(spins[:, l:] * spins[:, :S - l]).sum(axis=2).mean(axis=1) / N for l in range(L + 1)], axis=1)
        assert np.all(np.abs(got - direct) < 1e-12)   # ... which is the correlation it is named after
        conn = lat.run_monte_carlo_and_measure_variable_autocorrelation(0.5, S * freq, R, sampling_wait_buffer=therm, sampling_freq=freq, max_lag=max_lag,
                                                                        connected=True)
        mean = spins.sum(axis=1) / S
        ref = want - ((mean * mean).sum(axis=1) / N)[:, None]
        print(f"connected, L = {L}: largest difference to the numpy form {np.abs(conn - ref).max():.3e}")
        assert conn.shape == (R, L + 1) and np.all(np.abs(conn - ref) <= 3e-14)


def test_classic_ising_measured_autocorrelation(exact):
    import py_monte_carlo
    from pyisingmontecarlo_amd import correlation as K
    ea, eb, ej = _glass(exact)
    ci, twin = (py_monte_carlo.ClassicIsing(_edge_list(ea, eb, ej), None, 3, 21) for _ in range(2))
    ci.set_measure_autocorrelation_every(2, max_lag=3)
    ci.run_monte_carlo(0.5, 6)
    ci.run_monte_carlo(0.6, 5)           # samples at 2, 4, 6 | 8, 10 over the two calls
    ring = AR.LagRing(3, 3)
    for n, beta in ((2, 0.5), (2, 0.5), (2, 0.5), (2, 0.6), (2, 0.6), (1, 0.6)):
        twin.run_monte_carlo(beta, n)
        if n == 2:
            ring.add(twin.get_states())
    lags, counts, corr = ci.get_measured_autocorrelation()
    assert lags.dtype == np.int64 and list(lags) == [0, 2, 4, 6]
    assert ring.samples == 5 and np.array_equal(counts, ring.counts)
    assert corr.shape == (3, 4) and np.array_equal(corr, K.autocorrelation(ring.diff, ring.counts, 768)) and np.all(corr[:, 0] == 1.0)
    assert np.array_equal(ci.get_states(), twin.get_states())
    with pytest.raises(ValueError, match="a lag ring is live"):
        ci.add_graph()
    ci.reset_measured_autocorrelation()
    lags, counts, corr = ci.get_measured_autocorrelation()
    assert not counts.any() and np.all(np.isnan(corr))
    ci.set_measure_autocorrelation_every(0)
    ci.run_monte_carlo(0.5, 2)
    assert not ci.get_measured_autocorrelation()[1].any()

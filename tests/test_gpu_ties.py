"""Every bit-sliced sweep kernel on quads that were SEARCHED for their ties (tests/golden/tie_cases.json).

The n-th tie of a quad takes word n % 4 of Philox call 7 + n / 4.  Random inputs reach the fifth tie a few times in a thousand
quads and the ninth once in a million, so `N_PLANES + (nres >> 2)` beyond the first refill, the word index after a refill and
the 4 / 5 boundary between the two branches of `quad_ties` are reached here and nowhere else: a container is created with the
case's seed, put on an all-satisfied start (every spin of the first pass in one class), moved to the case's timestep and run
at the beta whose threshold has the case's prefix value on top.  After one timestep the target quad of the first colour /
class must show the flips of tests/tie_reference.py (plane 0 and the sites of class 0 are final after their pass); the whole
configuration and the energy must equal the oracle's after 1 and after 3 timesteps.

Kernels that serve only calls of several timesteps (the strip kernel needs two; the resident kernels' multi-step launches) are
run in ONE call of three timesteps with the energy after every step: there the first timestep shows through its energy and
through the final configuration, not through the target quad itself, whose reference flips are checked against the oracle.

A precondition that does not hold -- fewer ties than claimed, another kernel family, a threshold off the prefix value --
fails the test."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tie_cases as TC  # noqa: E402

LATS, PKSW = TC.load("LATS"), TC.load("PKSW")
LATS_C1 = TC.load("LATS", colour=1)                                    # searched for the second colour, prefix value 0
LATS_Q0 = [c for c in LATS if c["Q"] == 0]
LATS_ROW = [c for c in LATS if 1 <= c["Q"] <= 6]                       # an interior row of a 256-wide lattice
FAST_PATH = {"ferro": 0, "mattis": 0, "field": 1, "field_signs": 1, "open": 2, "aniso": 3, "open_field": 4}


def _few(cases):
    """The boundary cases (exactly 4, 5, 8, 9 ties) and the two with the most ties, one of them with t >= 2^32."""
    out = [next(c for c in cases if c["n_ties"] == n) for n in (4, 5, 8, 9)]
    out.append(TC.most_ties(cases[0]["domain"], lambda c: c in cases))
    out.append(TC.most_ties(cases[0]["domain"], lambda c: c in cases and c["t"] >= 2 ** 32))
    return [c for i, c in enumerate(out) if c not in out[:i]]


def _top(cases, hi=False):
    return TC.most_ties(cases[0]["domain"], lambda c: c in cases and (not hi or c["t"] >= 2 ** 32))


def _run_lattice(capi, oracle, exact, W, H, mode, case, options, replicas=2, per_step=False, one_call=False, min_ties=None):
    sysm = TC.LatticeSystem(exact, W, H, mode)
    colour = case["colour"]
    beta = TC.beta_and_threshold(case, sysm.bulk_dE())[0]
    g = capi.Graph(sysm.ea, sysm.eb, sysm.ej, nvars=W * H, biases=sysm.biases)
    assert g.kind == capi.KIND_LATTICE2D and g.info.fast_path == FAST_PATH[mode]
    assert bool(g.info.uniform_sign) == (not sysm.gauged) and bool(g.info.field_signs) == (mode == "field_signs")
    seeds = TC.seeds_for(case, replicas)
    st = capi.States(g, seeds)
    assert st.family == "checkerboard"
    for name, value in options.items():
        st.set_option(name, value)
    for r in range(replicas):
        st.set_state(r, sysm.start)
    st.timestep = case["t"]
    lat = sysm.oracle_lat(oracle)
    ref = [lat.pack(sysm.start) for _ in seeds]
    np.testing.assert_array_equal(st.packed(), np.stack(ref))
    before = sysm.quad_bits(ref[0], case["Q"], colour)
    ref_e = np.zeros((replicas, 3))
    after1 = None
    for k in range(3):
        for r in range(replicas):
            lat.sweep(ref[r], seeds[r], case["t"] + k, beta)
            ref_e[r, k] = lat.energy_mag(ref[r])[0]
        if k == 0:
            after1 = [x.copy() for x in ref]
    # colour 0: from the all-satisfied start; colour 1: from what the colour-0 pass left (its sites are final after it)
    _, flips, ties, highest = sysm.second_pass(case, lat.unpack(after1[0])) if colour else sysm.first_pass(case)
    if min_ties is None:                                               # one class for the whole quad: the fixture's ties exactly
        assert [list(t) for t in ties] == case["ties"]
    else:
        assert len(ties) >= min_ties, len(ties)
    assert highest == 7 + (len(ties) - 1) // 4
    # the oracle's own pass over the quad is the reference's (also on the CPU, tests/test_tie_cases_host.py)
    assert [a ^ b for a, b in zip(before, sysm.quad_bits(after1[0], case["Q"], colour))] == flips
    if one_call:                                                       # kernels that need a call of several timesteps
        eps = st.do_time_steps(3, beta, per_step_energies=True)
        np.testing.assert_array_equal(eps, ref_e)                      # ... show the first timestep through its energy
    else:
        eps = st.do_time_steps(1, beta, per_step_energies=per_step)
        packed = st.packed()
        got = [a ^ b for a, b in zip(before, sysm.quad_bits(packed[0], case["Q"], colour))]
        assert got == flips, [(i >> 5, i & 31) for i in range(128) if got[i] != flips[i]]
        np.testing.assert_array_equal(packed, np.stack(after1))
        np.testing.assert_array_equal(st.energies(), ref_e[:, 0])
        if per_step:
            np.testing.assert_array_equal(eps[:, 0], ref_e[:, 0])
        eps = st.do_time_steps(2, beta, per_step_energies=per_step)
        if per_step:
            np.testing.assert_array_equal(eps, ref_e[:, 1:])
    assert st.timestep == case["t"] + 3
    np.testing.assert_array_equal(st.packed(), np.stack(ref))
    np.testing.assert_array_equal(st.energies(), ref_e[:, 2])


# ---- quad_ties (lattice_kernels.hpp) ----------------------------------------------------------------------------
STREAM = {"disable_resident": 1, "strip": 0, "sweep_iters": 1}


@pytest.mark.parametrize("mode", ["ferro", "mattis"])
@pytest.mark.parametrize("case", LATS_Q0 + [c for c in LATS if c["Q"] == 1], ids=TC.case_id)
def test_lat_sweep_kernel_64x8(capi, oracle, exact, mode, case):
    """lat_sweep_kernel<false, PMJ, false>: W % 256 != 0 (not `vec`), `disable_resident` keeps the 2-quad lattice off
    lat_resident_fits, one timestep per call keeps it off the strip plan: run_lat_stream, one quad per thread."""
    _run_lattice(capi, oracle, exact, 64, 8, mode, case, STREAM)


@pytest.mark.parametrize("mode", ["ferro", "mattis"])
@pytest.mark.parametrize("case", _few(LATS_Q0) + LATS_ROW, ids=TC.case_id)
def test_lat_sweep_kernel_256x8(capi, oracle, exact, mode, case):
    """lat_sweep_kernel<true, PMJ, false>: a `vec` geometry (W % 256 == 0) whose `cols_log2` stays -1 -- one quad per row
    makes rows_per_pair = 128, which does not divide H = 8, and 8 quads are no multiple of 64 -- so launch_lat_sweep takes
    neither the loop kernel nor the division-free mapping (run_lat_stream; resident and strip switched off)."""
    _run_lattice(capi, oracle, exact, 256, 8, mode, case, STREAM)


@pytest.mark.parametrize("mode", ["ferro", "mattis"])
@pytest.mark.parametrize("case", _few(LATS_Q0), ids=TC.case_id)
def test_lat_sweep_kernel_256x128(capi, oracle, exact, mode, case):
    """lat_sweep_kernel<true, PMJ, true>, the division-free one-quad mapping: `cols_log2` = 0 here (H % 128 == 0 and 128
    quads per colour, a multiple of 64) and `sweep_iters = 1` keeps launch_lat_sweep off the loop kernel (run_lat_stream;
    `disable_resident` because 128 quads would fit lat_resident_fits, `strip = 0`)."""
    _run_lattice(capi, oracle, exact, 256, 128, mode, case, STREAM)


@pytest.mark.parametrize("W,H,iters", [(1024, 256, 2), (1024, 256, 4), (4096, 512, 16)])
@pytest.mark.parametrize("mode", ["ferro", "mattis"])
@pytest.mark.parametrize("pick", ["n5", "top", "top_hi"])
def test_lat_sweep_loop_kernel(capi, oracle, exact, W, H, iters, mode, pick):
    """lat_sweep_loop_kernel<PMJ>: run_lat_stream with `sweep_iters` = 2, 4, 16 (sweep_loop_iters: 256 * iters divides the
    quads of a plane and 2 * iters divides H).  Quad 0 belongs to thread 0, which loops: the lane with the many ties
    diverges from its wave in its first iteration."""
    case = next(c for c in LATS_Q0 if c["n_ties"] == 5) if pick == "n5" else _top(LATS_Q0, hi=pick == "top_hi")
    assert case["n_ties"] == 5 or case["n_ties"] >= 9
    _run_lattice(capi, oracle, exact, W, H, mode, case, {"disable_resident": 1, "strip": 0, "sweep_iters": iters},
                 replicas=2 if W == 1024 else 1)


@pytest.mark.parametrize("mode", ["ferro", "mattis"])
@pytest.mark.parametrize("iters", [1, 4])
def test_lat_sweep_measure_kernel(capi, oracle, exact, mode, iters):
    """Energies after every timestep on run_lat_stream: the colour-0 launch is followed by lat_sweep_measure_kernel for
    colour 1, whose counters must give the oracle's energy after every step.  That kernel only ever runs colour 1, so its
    own tie stage is reached by the cases searched for colour 1 at the prefix value 0 (beta = ln 256 / 8: one colour-0 spin
    in 256 flips, and a colour-1 spin next to it leaves the class); >= 9 ties must be left on this lattice."""
    case = _top(LATS_Q0)
    assert case["n_ties"] >= 9
    options = {"disable_resident": 1, "strip": 0, "sweep_iters": iters}
    _run_lattice(capi, oracle, exact, 1024, 256, mode, case, options, per_step=True)
    assert len(LATS_C1) >= 2
    for case in LATS_C1:
        _run_lattice(capi, oracle, exact, 1024, 256, mode, case, options, per_step=True, min_ties=9)


@pytest.mark.parametrize("spread", [0, 1])
@pytest.mark.parametrize("mode", ["ferro", "mattis"])
@pytest.mark.parametrize("case", _few(LATS_Q0), ids=TC.case_id)
def test_lat_resident_kernels_64x64(capi, oracle, exact, spread, mode, case):
    """64 x 64 = 16 quads per colour: lat_resident_fits, so run_lat_resident; `resident_spread` = 0: lat_resident_kernel
    (one lane per quad), 1: lat_resident_spread_kernel (16 * 8 <= 1024: eight lanes share a quad's calls)."""
    _run_lattice(capi, oracle, exact, 64, 64, mode, case, {"resident_spread": spread})
    _run_lattice(capi, oracle, exact, 64, 64, mode, case, {"resident_spread": spread}, one_call=True)  # three timesteps in one launch


@pytest.mark.parametrize("mode", ["ferro", "mattis"])
@pytest.mark.parametrize("nw", [1, 4])
@pytest.mark.parametrize("case", _few(LATS_Q0), ids=TC.case_id)
def test_lat_strip_kernel(capi, oracle, exact, mode, nw, case):
    """lat_strip_kernel on 1024 x 128 (`strip_nw` = 4: two strips of 64 rows per replica; 1: eight of 16 rows): `strip = 1`
    with resident off and a call of three timesteps (strip_plan needs >= 2).  The first tie call of a quad is drawn before the wait for the neighbour strip."""
    _run_lattice(capi, oracle, exact, 1024, 128, mode, case, {"disable_resident": 1, "strip": 1, "strip_nw": nw}, one_call=True)


# ---- mc_quad_body.inc -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["field", "field_signs", "open", "open_field", "aniso"])
@pytest.mark.parametrize("kernel", ["sweep", "resident", "resident_spread"])
def test_multi_class_kernels(capi, oracle, exact, mode, kernel):
    """lat_mc_sweep_kernel (256 x 16, `disable_resident`: run_mc_stream) and lat_mc_resident_kernel (256 x 8,
    lat_resident_fits: run_mc_resident, one lane per quad with `resident_spread` = 0, else eight).  The quad is an interior
    row, so the open lattices have their edge column in it; +-h fields come with the gauge, sigma = +1 everywhere."""
    options = {"sweep": {"disable_resident": 1}, "resident": {"resident_spread": 0}, "resident_spread": {"resident_spread": 1}}[kernel]
    for case in LATS_ROW:
        assert case["n_ties"] >= 10                                    # an open edge takes at most one spin out of the class
        _run_lattice(capi, oracle, exact, 256, 16 if kernel == "sweep" else 8, mode, case, options, min_ties=9)
    if kernel != "sweep":
        _run_lattice(capi, oracle, exact, 256, 8, mode, LATS_ROW[0], options, min_ties=9, one_call=True)


# ---- packed_kernels.hpp / packed_uni_kernels.hpp ----------------------------------------------------------------
def _run_packed(capi, oracle, monkeypatch, sysm, case, options, degree, other_beta_bits=(), min_ties=None):
    betas = None
    if other_beta_bits:
        beta0 = sysm.first_pass(case)[0]
        betas = [beta0 * (0.5 + 0.2 * other_beta_bits.index(b)) if b in other_beta_bits else beta0 for b in range(32)]
    beta, flips, ties, highest = sysm.first_pass(case, betas)
    if min_ties is None:
        assert [list(t) for t in ties] == case["ties"]
    else:
        assert len(ties) >= min_ties, len(ties)
    monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")                    # the family is fixed at creation
    g = capi.Graph(sysm.ea, sysm.eb, sysm.ej, nvars=sysm.nvars)
    assert g.kind == capi.KIND_GENERAL and g.info.packed_degree == degree
    seeds = TC.seeds_for(case, 32)
    st = capi.States(g, seeds, initial_state=sysm.start)
    assert st.family == "packed_bitsliced"
    for name, value in options.items():
        st.set_option(name, value)
    if betas is not None:
        st.set_betas(betas)
    st.timestep = case["t"]
    start = np.tile(sysm.start, (32, 1))
    np.testing.assert_array_equal(st.states().astype(np.uint8), start)
    ref, ref_e = start, None
    for n_steps, t0 in ((1, case["t"]), (2, case["t"] + 1)):
        kw = dict(beta_replica=betas) if betas is not None else dict(betas=[beta] * n_steps)
        ref_e, ref = oracle.pk_run(sysm.ea, sysm.eb, sysm.ej, sysm.nvars, seeds, n_steps, states=ref.copy(), t0=t0, **kw)
        st.do_time_steps(n_steps, None if betas is not None else beta)
        got = st.states().astype(np.uint8)
        if n_steps == 1:                                               # class 0's sites are final after class 0's pass
            quad = [a ^ b for a, b in zip(sysm.quad_bits(start, case["Q"]), sysm.quad_bits(got, case["Q"]))]
            assert quad == flips, [(i >> 5, i & 31) for i in range(128) if quad[i] != flips[i]]
        np.testing.assert_array_equal(got, ref)
        np.testing.assert_array_equal(st.energies(), ref_e)
    assert st.timestep == case["t"] + 3
    return ties


@pytest.mark.parametrize("uniform_kernel", [True, False])
@pytest.mark.parametrize("case", PKSW, ids=TC.case_id)
def test_packed_kernels_cubic_ferromagnet(capi, oracle, exact, monkeypatch, uniform_kernel, case):
    """8^3 periodic cubic ferromagnet, every site of degree 6 and both classes whole 256-blocks: pk_launch_timestep sends
    them to pk_sweep_uni_kernel (`packed_degree` = 6), and with `disable_packed_uniform` = 1 to pk_sweep_kernel."""
    _run_packed(capi, oracle, monkeypatch, TC.PackedSystem(exact, oracle), case, {"disable_packed_uniform": int(not uniform_kernel)}, 6)


@pytest.mark.parametrize("case", _few(PKSW), ids=TC.case_id)
def test_packed_uniform_kernel_mattis_glass(capi, oracle, exact, monkeypatch, case):
    """pk_sweep_uni_kernel's +-J instantiation (`pk_uni_pmj`): the Mattis-gauged 8^3 glass started on its gauge."""
    sysm = TC.PackedSystem(exact, oracle, gauged=True)
    assert (sysm.ej > 0).any() and (sysm.ej < 0).any()
    _run_packed(capi, oracle, monkeypatch, sysm, case, {}, 6)


@pytest.mark.parametrize("case", TC.diluted_cases(PKSW), ids=TC.case_id)
def test_packed_kernel_diluted_lattice(capi, oracle, exact, monkeypatch, case):
    """pk_sweep_kernel on a diluted lattice (`packed_degree` = 0: no one-degree kernel): the sites of the target
    position-quad have degrees 6, 6, 5 and 4, each word with its own row of the threshold table.  The cases are those of
    the fixture that keep >= 9 ties on this lattice with a tie in a second row (a site of lower degree ties at its own
    prefix value): both are asserted."""
    sysm = TC.diluted(exact, oracle, case)
    ties = _run_packed(capi, oracle, monkeypatch, sysm, case, {}, 0, min_ties=9)
    assert len(TC.tie_rows(sysm, case, ties)) >= 2


@pytest.mark.parametrize("uniform_kernel", [True, False])
@pytest.mark.parametrize("case", [c for c in PKSW if c["n_ties"] >= 9], ids=TC.case_id)
def test_packed_kernels_per_replica_betas(capi, oracle, exact, monkeypatch, uniform_kernel, case):
    """Per-replica betas (`set_betas`: one table row entry per replica, tab[PK_TAB_LO + row * 32 + b]): the case's beta on
    all replicas but three that hold none of the case's ties, so the ties stay and run across the refills."""
    free = [b for b in range(32) if b not in {b for _, b in case["ties"]}][:3]
    assert len(free) == 3
    ties = _run_packed(capi, oracle, monkeypatch, TC.PackedSystem(exact, oracle), case, {"disable_packed_uniform": int(not uniform_kernel)}, 6,
                       other_beta_bits=tuple(free), min_ties=case["n_ties"])
    assert {tuple(t) for t in case["ties"]} <= set(ties)


def test_set_option_names(capi, exact):
    """Every switch of a container can be set by its name, in either case, with or without the ISINGMC_ prefix -- also
    `disable_packed_uniform`, which begins with the name of a family switch; the four family switches are refused."""
    g = capi.Graph(*exact.square_lattice_edges(64, 8, -1.0))
    st = capi.States(g, TC.seeds_for(LATS[0], 1))
    for name in ("disable_packed_uniform", "DISABLE_PACKED_UNIFORM", "ISINGMC_DISABLE_PACKED_UNIFORM", "isingmc_disable_resident",
                 "strip", "sweep_iters", "resident_spread", "streams", "pk_streams", "cluster_workspace_bytes", "gen_stage", "gen_rb",
                 "GEN_RB", "real_measure_wgs", "ISINGMC_REAL_MEASURE_WGS"):
        st.set_option(name, 1)
    for name in ("force_real", "disable_real", "force_packed", "disable_packed", "ISINGMC_DISABLE_PACKED", "Force_Packed"):
        with pytest.raises(ValueError, match="fixed when it is created"):
            st.set_option(name, 1)
    with pytest.raises(ValueError, match="unknown option"):
        st.set_option("disable_packed_uniforms", 1)

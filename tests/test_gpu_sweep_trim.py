"""The class stage of the two-class sweep kernels on uniform couplings (quad_classes, lattice_kernels.hpp).

With one coupling sign for the whole graph the bond masks are no longer formed: `up ^ dn` and `ce ^ si` hold neither the own
word nor the sign, and `a0 & a1`, `a2 & a3` are 3-input functions of (own, up, dn) / (own, ce, si) whose truth table one scalar
branch per quad picks by the sign.  The two tables (J = -1 and J = +1), the untouched +-J form and what follows the class masks
(the `any_all` branch at beta = 0, the four per-plane threshold selectors, per-replica thresholds) must give the oracle's
configurations and energies bit for bit after 1 and after 3 timesteps.

Shapes (resident and strip kernels switched off on the container, so the streaming kernels run):
  256 x 64    one quad per row, 64 quads per colour = one wave whose lanes are 64 different rows, rows 0 and H-1 among them: every
              lane wraps its rows itself.  The host gives the division-free mapping only where H is a multiple of the 128 rows a
              wave pair shares, and the looping kernel only where 256 * sweep_iters divides the quads of a colour: here both
              forced counts fall back to lat_sweep_kernel<true, PMJ, false>.
  256 x 512   the smallest lattice of that row length which the looping kernel takes (cols_log2 = 0, 512 quads per colour, two
              quads per thread): its waves that hold row 0 and row H-1 wrap per lane, the others walk by a scalar offset.
  4096 x 32   the benchmark's row length (cols_log2 = 4), 512 quads per colour: sweep_iters = 2 is lat_sweep_loop_kernel with
              one workgroup, 16 does not divide the plane and falls back to lat_sweep_kernel<true, PMJ, true>.
  4096 x 256  the smallest lattice of the benchmark's row length on which 16 quads per thread divide the plane (4096 quads per
              colour = one workgroup): the benchmark's own form of lat_sweep_loop_kernel, its 16-step walk included.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEEDS = np.array([0x0123456789ABCDEF, 42, 2**64 - 1, 7], dtype=np.uint64)
SHAPES = [(256, 64, 2), (256, 64, 16), (256, 512, 2), (4096, 32, 2), (4096, 32, 16), (4096, 256, 16)]
COUPLINGS = ["ferro", "antiferro", "glass"]       # J = -1 (sign mask all ones), J = +1 (sign mask zero), +-J sign planes
BETA_C = 0.4407

_reference = {}
_beta_sel = []


def selector_beta(oracle):
    """The first beta on a grid of 0.001 whose thresholds' top 7 bits, taken plane by plane as (bit of T3) | (bit of T4) << 1,
    show all four selector values of plane_step / quad_planes; neither class is accepted outright."""
    if not _beta_sel:
        for k in range(1, 2000):
            beta = k * 0.001
            h3, h4 = oracle.threshold_fixed(beta, 4.0) >> 32, oracle.threshold_fixed(beta, 8.0) >> 32
            sels = [((h3 >> p) & 1) | (((h4 >> p) & 1) << 1) for p in range(6, -1, -1)]
            if h3 < 128 and h4 < 128 and set(sels) == {0, 1, 2, 3}:
                _beta_sel.append((beta, h3, h4, sels))
                break
    assert _beta_sel, "no beta with all four selector values"
    return _beta_sel[0]


def _lattice(oracle, exact, W, H, coupling):
    if coupling == "glass":
        ea, eb, ej = exact.square_lattice_edges(W, H, 1.0, np.random.default_rng(31))
        return (ea, eb, ej), oracle.Lat(W, H, 1.0, 0, (ej[0::2] > 0).astype(np.uint8), (ej[1::2] > 0).astype(np.uint8))
    J = -1.0 if coupling == "ferro" else 1.0
    return exact.square_lattice_edges(W, H, J), oracle.Lat(W, H, 1.0, int(J > 0))


def _oracle_run(oracle, exact, W, H, coupling, seeds, betas):
    """Packed spins and energies after 1 and after 3 sweeps, computed once per case and left unchanged."""
    key = (W, H, coupling, tuple(int(s) for s in seeds), tuple(betas))
    if key not in _reference:
        lat = _lattice(oracle, exact, W, H, coupling)[1]
        out = {1: ([], []), 3: ([], [])}
        for s, beta in zip(seeds, betas):
            ref = lat.init(s)
            for t in range(3):
                lat.sweep(ref, s, t, beta)
                if t + 1 in out:
                    out[t + 1][0].append(ref.copy())
                    out[t + 1][1].append(lat.energy_mag(ref)[0])
        for T in out:
            packed, energies = np.stack(out[T][0]), np.array(out[T][1])
            packed.setflags(write=False)
            out[T] = (packed, energies)
        _reference[key] = out
    return _reference[key]


def _check(capi, oracle, exact, W, H, iters, coupling, seeds, betas):
    (ea, eb, ej), _ = _lattice(oracle, exact, W, H, coupling)
    g = capi.Graph(ea, eb, ej)
    assert g.kind == capi.KIND_LATTICE2D and g.info.fast_path == 0 and bool(g.info.uniform_sign) == (coupling != "glass")
    st = capi.States(g, seeds)
    assert st.family == "checkerboard"
    st.set_option("disable_resident", 1)
    st.set_option("strip", 0)
    st.set_option("sweep_iters", iters)
    per_replica = len(set(betas)) > 1
    if per_replica:
        st.set_betas(list(betas))
    ref = _oracle_run(oracle, exact, W, H, coupling, seeds, betas)
    done = 0
    for T in (1, 3):
        if per_replica:
            st.do_time_steps(T - done)
        else:
            st.do_time_steps(T - done, betas[0])
        done = T
        np.testing.assert_array_equal(st.packed(), ref[T][0], err_msg=f"spins after {T} timestep(s)")
        np.testing.assert_array_equal(st.energies(), ref[T][1], err_msg=f"energies after {T} timestep(s)")


def test_selector_beta_shows_all_four_selectors(oracle):
    beta, h3, h4, sels = selector_beta(oracle)
    print(f"beta = {beta:.3f}: top bits of T3 = {h3:07b}, of T4 = {h4:07b}, selectors from the top plane down = {sels}")
    assert sorted(set(sels)) == [0, 1, 2, 3]
    # beta = 0 accepts both classes outright (any_all), the headline beta neither
    assert oracle.threshold_fixed(0.0, 4.0) >> 39 == 1 and oracle.threshold_fixed(0.0, 8.0) >> 39 == 1
    assert oracle.threshold_fixed(BETA_C, 4.0) >> 39 == 0


@pytest.mark.parametrize("beta", ["zero", "critical", "selectors"])
@pytest.mark.parametrize("coupling", COUPLINGS)
@pytest.mark.parametrize("W,H,iters", SHAPES)
def test_one_beta_equals_the_oracle(capi, oracle, exact, W, H, iters, coupling, beta):
    b = {"zero": 0.0, "critical": BETA_C, "selectors": selector_beta(oracle)[0]}[beta]
    _check(capi, oracle, exact, W, H, iters, coupling, SEEDS[:2], (b, b))


@pytest.mark.parametrize("coupling", COUPLINGS)
@pytest.mark.parametrize("W,H,iters", SHAPES)
def test_per_replica_betas_equal_the_oracle(capi, oracle, exact, W, H, iters, coupling):
    """Four replicas, four thresholds pairs: accepted outright, the headline, all four selectors, and a cold one."""
    _check(capi, oracle, exact, W, H, iters, coupling, SEEDS, (0.0, BETA_C, selector_beta(oracle)[0], 0.9))

"""lat_sweep_loop_kernel with its addressing hoisted out of the quad loop, and the resident-sized choice of quads per thread.

A looping thread works out its quad, its row and its load offsets once; from one iteration to the next only a wave-uniform
scalar offset and the quad index advance, and the wave that holds row 0 or row H-1 in an iteration wraps its rows per lane.
Every count of quads per thread decides the same quads with the same Philox counters, so all of them must give the oracle's
configurations and energies bit for bit.  The shapes are the smallest that reach each branch; they would fit the LDS-resident
or the strip kernel, which are switched off on the container so that the streaming kernels run.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEEDS = np.array([0x0123456789ABCDEF, 42, 2**64 - 1], dtype=np.uint64)

_reference = {}


def _oracle_run(oracle, exact, W, H, glass, seeds, betas, T):
    """Packed spins and energies after T sweeps from the oracle engine, computed once per case and left unchanged."""
    key = (W, H, glass, tuple(int(s) for s in seeds), tuple(betas), T)
    if key not in _reference:
        if glass:
            _, _, ej = exact.square_lattice_edges(W, H, 1.0, np.random.default_rng(31))
            lat = oracle.Lat(W, H, 1.0, 0, (ej[0::2] > 0).astype(np.uint8), (ej[1::2] > 0).astype(np.uint8))
        else:
            lat = oracle.Lat(W, H, 1.0, 0)
        packed, energies = [], []
        for s, beta in zip(seeds, betas):
            ref = lat.init(s)
            for t in range(T):
                lat.sweep(ref, s, t, beta)
            packed.append(ref)
            energies.append(lat.energy_mag(ref)[0])
        packed, energies = np.stack(packed), np.array(energies)
        packed.setflags(write=False)
        _reference[key] = (packed, energies)
    return _reference[key]


def _streaming_states(capi, exact, W, H, glass, seeds, iters):
    ea, eb, ej = exact.square_lattice_edges(W, H, -1.0 if not glass else 1.0, np.random.default_rng(31) if glass else None)
    g = capi.Graph(ea, eb, ej)
    assert g.kind == capi.KIND_LATTICE2D and bool(g.info.uniform_sign) != glass
    st = capi.States(g, seeds)
    st.set_option("disable_resident", 1)
    st.set_option("strip", 0)
    if iters is not None:
        st.set_option("sweep_iters", iters)
    return st


def _check(capi, oracle, exact, W, H, glass, seeds, betas, T, iters):
    st = _streaming_states(capi, exact, W, H, glass, seeds, iters)
    if len(set(betas)) > 1:
        st.set_betas(list(betas))
        st.do_time_steps(T)
    else:
        st.do_time_steps(T, betas[0])
    packed, energies = _oracle_run(oracle, exact, W, H, glass, seeds, betas, T)
    np.testing.assert_array_equal(st.packed(), packed, err_msg=f"spins, {iters} quads per thread")
    np.testing.assert_array_equal(st.energies(), energies, err_msg=f"energies, {iters} quads per thread")


@pytest.mark.parametrize("iters", [1, 2, 4])
def test_rows_of_four_quads_every_count_equals_the_oracle(capi, oracle, exact, iters):
    """1024 x 256, uniform J: cols_log2 = 2, 1024 quads per colour, a wave spans 16 rows.  With 4 quads per thread one workgroup
    walks the whole plane: every thread crosses row blocks, wave 0 wraps row 0 in its first iteration and wave 3 wraps row
    H-1 in its last."""
    _check(capi, oracle, exact, 1024, 256, False, SEEDS, (0.4407,) * 3, 3, iters)


@pytest.mark.parametrize("iters", [1, 2, 4])
def test_rows_of_64_quads_every_count_equals_the_oracle(capi, oracle, exact, iters):
    """16384 x 16: cols_log2 = 6, a wave never leaves its row and the row itself is wave-uniform."""
    _check(capi, oracle, exact, 16384, 16, False, SEEDS[:2], (0.4407,) * 2, 2, iters)


def test_glass_with_per_replica_betas_four_quads_per_thread(capi, oracle, exact):
    """The +-J instantiation (sign words addressed by the walking quad index) with one threshold pair per replica."""
    _check(capi, oracle, exact, 1024, 256, True, SEEDS, (0.2, 0.4407, 0.9), 3, 4)


@pytest.mark.parametrize("iters", [16, 32])
def test_headline_row_length_16_and_32_quads_per_thread(capi, oracle, exact, iters):
    """4096 x 512: the benchmark's row length (cols_log2 = 4, a wave spans 4 rows) and the smallest height at which 32 quads per
    thread leave a whole workgroup (8192 quads per colour, a thread's quads 16 rows apart)."""
    _check(capi, oracle, exact, 4096, 512, False, SEEDS[:2], (0.4407,) * 2, 2, iters)


def test_resident_sized_launch_chosen_by_the_host_equals_one_quad_per_thread(capi, exact):
    """Nothing forced.  1024 x 256 x 4096 replicas are 16384 one-quad workgroups; a device of 256 CUs holds 8 x 256 = 2048
    workgroups of the looping kernel at once, so the host picks 4 quads per thread (4096 workgroups, two whole rounds): the
    smallest shape at which the resident-sized rule goes beyond two quads per thread.  On another device the rule may pick
    another count; the result must be that of the one-quad kernel whatever it picks."""
    seeds = capi.make_seeds(77, 4096)
    a = _streaming_states(capi, exact, 1024, 256, False, seeds, None)
    a.do_time_steps(3, 0.4407)
    b = _streaming_states(capi, exact, 1024, 256, False, seeds, 1)
    b.do_time_steps(3, 0.4407)
    np.testing.assert_array_equal(a.packed(), b.packed())
    np.testing.assert_array_equal(a.energies(), b.energies())

"""The plane and flip stages of the two-class sweep kernels (quad_planes, quad_ties, quad_new_words; lattice_kernels.hpp).

The flip decision is folded into the final xor (one 3-input function of own word, class mask and "below the threshold", into which
the tie loops record their wins), and all-zero threshold planes that are neighbours in processing order are applied in pairs.
Neither changes a Philox call or a decision: configurations and energies must equal the oracle's bit for bit after 1 and after
3 timesteps.

Betas, by the planes of hz = (top 7 bits of T3) | (top 7 bits of T4), processed from the least significant bit up; k = the run of
zero bits at the top of hz:
  k = 0            no zero plane at the top
  k = 1            one: stays on the single form unless the plane below it is zero too
  k = 2            the headline beta 0.4407: the two top planes form a pair
  k = 3            a pair and a single at the top
  k = 7            every plane zero (three pairs and a single): every surviving spin of the costly classes is a tie, so the
                   tie loops get the most traffic a threshold can give them (the refill path of five or more ties in a
                   quad is reached for certain by the searched seeds of tests/test_gpu_ties.py)
  lone             a zero plane between two non-zero ones: no pair may swallow it
  beta = 0         both classes accepted outright
  and one launch with per-replica betas of k = 0, 2, 3, 7.
Shapes (resident and strip kernels switched off on the container, so the streaming kernels run), as tests/test_gpu_sweep_trim.py:
  256 x 64, sweep_iters 2     falls back to lat_sweep_kernel
  256 x 512, 2                looping kernel, lanes spanning rows, per-lane wrap waves
  4096 x 32, 2                looping kernel at the benchmark's row length, one workgroup
  4096 x 32, 16               falls back to lat_sweep_kernel<..., true>
  4096 x 256, 16              the benchmark's own 16-quad walk
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEEDS = np.array([0x0123456789ABCDEF, 42, 2**64 - 1, 7], dtype=np.uint64)
SHAPES = [(256, 64, 2), (256, 512, 2), (4096, 32, 2), (4096, 32, 16), (4096, 256, 16)]
COUPLINGS = ["ferro", "antiferro", "glass"]       # J = -1 (sign mask all ones), J = +1 (sign mask zero), +-J sign planes
BETA_C = 0.4407
N_PLANES = 7
CASES = ["k0", "k1", "k2", "k3", "k7", "lone", "zero"]
# the beta ranges of each run length, from exp(-4 beta) * 128 (T4 < T3: the top of hz is the top of T3)
RANGES = {"k0": (0.0, 0.173), "k1": (0.173, 0.3466), "k2": (0.3466, 0.52), "k3": (0.52, 0.693), "k7": (1.22, 2.0)}

_reference = {}
_betas = {}


def _hz(oracle, beta):
    h3, h4 = oracle.threshold_fixed(beta, 4.0) >> 32, oracle.threshold_fixed(beta, 8.0) >> 32
    return None if (h3 >> N_PLANES) or (h4 >> N_PLANES) else (h3 | h4)


def _top_run(hz):
    k = 0
    while k < N_PLANES and not (hz >> (N_PLANES - 1 - k)) & 1:
        k += 1
    return k


def _forms(hz):
    """What each processing step does, least significant plane first: 'n' non-zero, 'o' left open, 'p' applied as a pair, 's' single."""
    out, i = [], 0
    while i < N_PLANES:
        if (hz >> i) & 1:
            out.append("n")
        elif i + 1 < N_PLANES and not (hz >> (i + 1)) & 1:
            out += ["o", "p"]
            i += 1
        else:
            out.append("s")
        i += 1
    return "".join(out)


def case_betas(oracle):
    """The first beta on a grid of 0.001 for each case (k = 2 is the headline beta itself)."""
    if not _betas:
        for k in range(1, 2000):
            beta = k * 0.001
            hz = _hz(oracle, beta)
            if hz is None:
                continue
            name = "k%d" % _top_run(hz)
            if name in RANGES and name != "k2" and name not in _betas and RANGES[name][0] < beta < RANGES[name][1]:
                _betas[name] = beta
            lone = any(not (hz >> i) & 1 and (hz >> (i - 1)) & 1 and (hz >> (i + 1)) & 1 for i in range(1, N_PLANES - 1))
            if lone and "lone" not in _betas:
                _betas["lone"] = beta
        _betas["k2"] = BETA_C
        _betas["zero"] = 0.0
    return _betas


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


def test_the_search_found_every_case(oracle):
    b = case_betas(oracle)
    for name in CASES:
        assert name in b, f"no beta for case {name}"
    for name in CASES[:-1]:
        hz = _hz(oracle, b[name])
        print(f"{name}: beta = {b[name]:.4f}, hz = {hz:07b}, steps from the least significant plane up = {_forms(hz)}")
    for k in (0, 1, 2, 3, 7):
        name = "k%d" % k
        assert _top_run(_hz(oracle, b[name])) == k and RANGES[name][0] < b[name] < RANGES[name][1]
    assert b["k2"] == BETA_C and _forms(_hz(oracle, BETA_C)).endswith("op")        # the headline: its two top planes are a pair
    assert _forms(_hz(oracle, b["k1"])).endswith("ns")                               # a single zero plane at the top
    assert _forms(_hz(oracle, b["k3"]))[-3:] == "ops"                                # a pair, then a single
    assert _forms(_hz(oracle, b["k7"])) == "opopops"                                 # three pairs and a single
    assert "nsn" in _forms(_hz(oracle, b["lone"]))                                   # the lone zero plane stays single
    assert oracle.threshold_fixed(0.0, 4.0) >> 39 == 1 and oracle.threshold_fixed(0.0, 8.0) >> 39 == 1   # accepted outright


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("coupling", COUPLINGS)
@pytest.mark.parametrize("W,H,iters", SHAPES)
def test_one_beta_equals_the_oracle(capi, oracle, exact, W, H, iters, coupling, case):
    b = case_betas(oracle)[case]
    _check(capi, oracle, exact, W, H, iters, coupling, SEEDS, (b, b, b, b))


@pytest.mark.parametrize("coupling", COUPLINGS)
@pytest.mark.parametrize("W,H,iters", SHAPES)
def test_per_replica_betas_equal_the_oracle(capi, oracle, exact, W, H, iters, coupling):
    """Four replicas of one launch with k = 0, 2, 3 and 7: the pairing is decided per replica."""
    b = case_betas(oracle)
    _check(capi, oracle, exact, W, H, iters, coupling, SEEDS, (b["k0"], b["k2"], b["k3"], b["k7"]))

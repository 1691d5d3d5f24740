"""Host side of tests/test_gpu_csr.py: the exact reference agrees with the oracle within the derived bound, and every graph
builder of tests/csr_reference.py has the rows, classes, coupling format and staged LDS size its GPU test relies on."""
from fractions import Fraction

import numpy as np
import pytest

import csr_reference as CR

GRAPHS = {g.name: g for g in CR.all_graphs()}


def test_exact_energy_by_hand():
    ea, eb = np.array([0, 1, 1, 2], dtype=np.uint64), np.array([1, 0, 1, 2], dtype=np.uint64)   # a doubled bond, two self-loops
    ej = np.array([0.1, 1e-50, 1e39, -0.25])
    h = np.array([0.5, -3.0, 0.0])
    e = CR.exact_energy(ea, eb, ej, 3, [1, 0, 1], h)
    want = -Fraction(0.1) - Fraction(1e-50) + Fraction(1e39) - Fraction(0.25) - (Fraction(0.5) + Fraction(3.0))
    assert e == want
    assert CR.exact_energy(ea, eb, ej, 3, [1, 1, 1]) == Fraction(0.1) + Fraction(1e-50) + Fraction(1e39) - Fraction(0.25)
    m = max(3 + 2 + 4, 4 + 3)
    assert CR.energy_bound(ej, h, 3, 2) == m * CR.U / (1 - m * CR.U) * (Fraction(0.1) + Fraction(1e-50) + Fraction(1e39) + Fraction(0.25)
                                                                       + Fraction(3.5))


@pytest.mark.parametrize("name", list(GRAPHS))
def test_oracle_energies_within_bound(oracle, name):
    g = GRAPHS[name]
    bound = CR.energy_bound(g.ej, g.biases, g.nvars, CR.max_degree(g))
    assert int(np.count_nonzero(g.ea == g.eb)) <= g.nvars       # (the bound's derivation counts on it)
    rng = np.random.default_rng(1)
    for spins in (np.ones(g.nvars, dtype=np.uint8), np.zeros(g.nvars, dtype=np.uint8), rng.integers(0, 2, g.nvars).astype(np.uint8)):
        e = oracle.energy(g.ea, g.eb, g.ej, g.nvars, spins, g.biases)
        assert abs(Fraction(e) - CR.exact_energy(g.ea, g.eb, g.ej, g.nvars, spins, g.biases)) <= bound
    betas = [0.0, -0.3, 30.0, 0.7]
    e, spins, eps = oracle.gen_run(g.ea, g.eb, g.ej, g.nvars, 1234, betas, biases=g.biases, per_step=True)
    assert abs(Fraction(e) - CR.exact_energy(g.ea, g.eb, g.ej, g.nvars, spins, g.biases)) <= bound
    traj = CR.oracle_trajectory(oracle, g, 1234, betas)
    assert np.array_equal(traj[-1], spins)
    for k in range(len(betas)):
        assert abs(Fraction(eps[k]) - CR.exact_energy(g.ea, g.eb, g.ej, g.nvars, traj[k], g.biases)) <= bound


@pytest.mark.parametrize("name", list(GRAPHS))
def test_coupling_format(name):
    g = GRAPHS[name]
    assert CR.float_lossless(g) == ("float" in name)
    if "float" in name:
        assert np.all(g.ej * 8 == np.round(g.ej * 8)) and (g.ej > 0).any() and (g.ej < 0).any()
    if "extreme" in name:
        bonds = g.ej[g.ea != g.eb]
        assert 1e-50 in bonds and 1e39 in bonds and np.float32(1e-50) == 0


def test_random_graph_has_self_loops_and_duplicates():
    g = CR.random_graph("extreme", True)
    assert g.nvars == 300 and np.count_nonzero(g.ea == g.eb) >= 2
    pairs = {}
    for a, b in zip(g.ea, g.eb):
        pairs[(min(a, b), max(a, b))] = pairs.get((min(a, b), max(a, b)), 0) + 1
    assert pairs[(5, 6)] >= 3


def test_lds_windows(oracle):
    small, mid, big = (CR.lds_graph(w) for w in ("small", "mid", "big"))
    for g in (small, mid, big):
        assert not CR.float_lossless(g) and g.biases is not None
        assert CR.n_positions(oracle, g) * 4 // 32 <= 32 * 1024 and g.nvars <= 8000     # gen_resident_fits
    assert CR.stage_bytes(oracle, small, 2) < CR.stage_bytes(oracle, small, 1) <= CR.LDS_DEFAULT
    assert CR.LDS_DEFAULT < CR.stage_bytes(oracle, mid, 1) <= CR.LDS_MAX     # <double, 1> through hipFuncSetAttribute
    assert CR.stage_bytes(oracle, mid, 2) <= CR.LDS_DEFAULT
    assert CR.stage_bytes(oracle, big, 1) > CR.LDS_MAX                       # a forced STAGE 1 falls back to 0
    assert CR.LDS_DEFAULT < CR.stage_bytes(oracle, big, 2) <= CR.LDS_MAX     # <double, 2> through hipFuncSetAttribute
    for kind in ("float", "extreme"):
        for bias in (False, True):
            assert CR.stage_bytes(oracle, CR.random_graph(kind, bias), 1) <= CR.LDS_DEFAULT


def test_gen_stage_words_by_hand():
    # 512 positions, 100 directed edges: 16 state words; f64 biases 1024, f64 couplings 200; rowptr 513, site 512, nbr 100
    assert CR.gen_stage_words(512, 100, True, 8, 1) == 16 + 1024 + 200 + 513 + 512 + 100
    assert CR.gen_stage_words(512, 100, False, 4, 1) == 16 + 100 + 513 + 512 + 100
    assert CR.gen_stage_words(512, 101, False, 4, 1) == 16 + 101 + 1 + 513 + 512 + 101     # 8-byte alignment behind the couplings
    assert CR.gen_stage_words(512, 100, True, 8, 2) == 16 + 513 + 512 + 100
    assert CR.gen_stage_words(32, 0, False, 4, 2) == 2 + 33 + 32                            # one state word, padded to two


def test_class_sizes(oracle):
    assert max(CR.class_sizes(oracle, CR.random_graph("float", False))) <= 256
    assert CR.class_sizes(oracle, CR.big_class_graph()) == [1300, 1300]            # > 1024: the resident kernel's strided loop
    assert max(CR.class_sizes(oracle, CR.tiny_class_graph())) < 64
    assert len(CR.class_sizes(oracle, CR.tiny_class_graph())) >= 3
    for kind in ("float", "double"):
        assert CR.class_sizes(oracle, CR.ring_graph(640, kind)) == [320, 320]      # two blocks: 256 sites, then 64 and padding
        assert CR.class_sizes(oracle, CR.multi_class_graph(kind)) == CR.MULTI_CLASS_SIZES
    assert CR.class_sizes(oracle, CR.one_block_graph()) == [64, 64]
    assert CR.n_positions(oracle, CR.one_block_graph()) == 512
    g = CR.multi_class_graph("double")
    assert CR.n_positions(oracle, g) == 768 + 3 * 256
    # not bipartite: a triangle
    adj = {}
    for a, b in zip(g.ea.tolist(), g.eb.tolist()):
        adj.setdefault(a, set()).add(b)
        adj.setdefault(b, set()).add(a)
    assert any(adj[665] & adj[q] for q in adj[665])


def rb_rule(blocks, R):
    """the rule for the replicas per thread of one class (step_policy.hpp, gen_replicas_per_thread; tests/test_step_policy_host.py
    holds this restatement against it)"""
    rb = 8
    while rb > 1 and (R < rb or blocks * ((R + rb - 1) // rb) < 2048):
        rb //= 2
    return rb


def test_rb_rule_shapes(oracle):
    assert rb_rule(1, 16387) == 8 and 16387 % 8 == 3                               # one block per class: 8 per thread, a tail of 3
    blocks = [(c + 255) // 256 for c in CR.MULTI_CLASS_SIZES]
    assert [rb_rule(b, 8003) for b in blocks] == [8, 2, 2, 2] and 8003 % 8 == 3    # two widths within one timestep
    assert [rb_rule(b, 13) for b in blocks] == [1, 1, 1, 1]
    assert 32768 + 5 > 32768 * 1 and 32768 + 5 <= 32768 * 8                        # gen_rb = 1 cuts the grid, gen_rb = 8 does not


def test_degree_mix_rows(oracle):
    for kind in ("float", "double"):
        g = CR.degree_mix_graph(kind)
        rows = CR.row_lengths(g)
        for d in (0, 1) + CR.DEGREE_MIX:
            assert np.count_nonzero(rows == d) >= 3, d
        assert np.count_nonzero(g.ea == g.eb) >= 5
        seen = set()
        dup = 0
        for a, b in zip(g.ea.tolist(), g.eb.tolist()):
            dup += (min(a, b), max(a, b)) in seen and a != b
            seen.add((min(a, b), max(a, b)))
        assert dup == len(CR.DEGREE_MIX)
        nc, colours, _ = oracle.gen_colouring(g.ea, g.eb, g.ej, g.nvars)
        assert nc == 2
        for d in CR.DEGREE_MIX:                                                    # three hubs of each row length, in both classes
            assert len(colours[rows == d]) == 3 and {int(c) for c in colours[rows == d]} == {0, 1}
        assert CR.max_degree(g) == 40

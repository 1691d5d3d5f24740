"""Minimum tracking without a GPU: the numpy restatement against hand cases, and the public surface."""
import os
import re

import numpy as np

import minimum_reference as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("isingmc_states_set_track_best", "isingmc_states_track_best", "isingmc_best_update", "isingmc_best_get",
               "isingmc_best_raw_state", "isingmc_best_reset")


def _states(*rows):
    return np.array(rows, dtype=np.bool_)


def test_records_start_at_infinity_and_the_first_update_records_everyone():
    rec = MR.Records(3, 2)
    assert np.all(np.isinf(rec.energy)) and np.all(rec.energy > 0) and rec.improvements == 0
    better = rec.update(5, [4.0, -1.0, 1e300], _states([1, 0], [0, 1], [1, 1]))
    assert better.all() and rec.improvements == 3
    assert np.array_equal(rec.energy, [4.0, -1.0, 1e300]) and np.array_equal(rec.timestep, [5, 5, 5])
    assert np.array_equal(rec.state, _states([1, 0], [0, 1], [1, 1]))


def test_ties_keep_the_earliest_timestep():
    t = [1, 2, 3, 4]
    e = [[2.0, 0.0], [1.0, 0.0], [1.0, -2.0], [3.0, -2.0]]
    s = [_states([0, 0], [0, 0]), _states([0, 1], [0, 1]), _states([1, 0], [1, 0]), _states([1, 1], [1, 1])]
    rec = MR.records(t, e, s)
    assert np.array_equal(rec.energy, [1.0, -2.0])
    assert np.array_equal(rec.timestep, [2, 3])           # replica 0 ties at t = 3, replica 1 at t = 4: neither moves the record
    assert np.array_equal(rec.state, _states([0, 1], [1, 0]))
    assert rec.improvements == 2 + 1 + 1 + 0
    assert [b.tolist() for b in rec.improved] == [[True, True], [True, False], [False, True], [False, False]]


def test_a_nan_energy_never_records():
    rec = MR.Records(1, 1)
    assert not rec.update(1, [np.nan], _states([1])).any() and np.isinf(rec.energy[0])


def test_reset_sets_the_records_back_but_keeps_the_kept_configurations():
    rec = MR.records([1], [[-3.0]], [_states([1, 1])])
    rec.reset()
    assert np.isinf(rec.energy[0]) and rec.timestep[0] == 0 and rec.improvements == 0 and rec.state.all()
    assert rec.update(9, [7.0], _states([0, 1])).all()   # a worse energy than before the reset records again
    assert rec.energy[0] == 7.0 and rec.timestep[0] == 9 and np.array_equal(rec.state, _states([0, 1]))


def test_word_level_merge_and_owned_masks():
    # 40 replicas from bit 20 on: groups 0 (bits 20..31) and 1 (bits 0..27)
    assert np.array_equal(MR.owned_masks(40, 20, 2), [0xFFF00000, 0x0FFFFFFF])
    raw0 = np.array([[0xFFFFFFFF, 0x0], [0xAAAAAAAA, 0x55555555]], dtype=np.uint32)
    raw1 = ~raw0
    all_of_them, some = np.ones(40, dtype=bool), np.zeros(40, dtype=bool)
    some[[0, 12]] = True   # bit 20 of group 0, bit 0 of group 1
    best = MR.merge_words([raw0, raw1], [all_of_them, some], 20, 2)
    own = MR.owned_masks(40, 20, 2)[:, None]
    want = raw0.copy()
    want[0] = (want[0] & ~np.uint32(1 << 20)) | (raw1[0] & np.uint32(1 << 20))
    want[1] = (want[1] & ~np.uint32(1)) | (raw1[1] & np.uint32(1))
    assert np.array_equal(best & own, want & own)


def test_every_new_symbol_is_declared_exported_and_wrapped(capi):
    header = open(os.path.join(ROOT, "include", "isingmc.h")).read()
    declared = set(re.findall(r"\b(isingmc_[a-z0-9_]+)\s*\(", header))
    new = {n for n in declared if n.startswith("isingmc_best_") or "track_best" in n}
    assert new == set(NEW_SYMBOLS)
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), f"libisingmc.so does not export {name}"
        assert name in capi.EXPORTED_SYMBOLS
    assert L.isingmc_abi_version() == 4


def test_the_python_surface_exists(capi):
    import py_monte_carlo
    from pyisingmontecarlo_amd.tempering import ClassicalTempering

    for name in ("set_track_best", "track_best", "best_update", "best", "best_raw", "best_reset"):
        assert hasattr(capi.States, name)
    for name in ("set_track_minimum", "get_minimum", "reset_minimum"):
        assert hasattr(py_monte_carlo.ClassicIsing, name)
    assert hasattr(py_monte_carlo.Lattice, "run_monte_carlo_annealing_and_get_minimum")
    assert "track_minimum" in py_monte_carlo.Lattice.run_population_annealing.__doc__
    for name in ("set_track_minimum", "get_minimum"):
        assert hasattr(ClassicalTempering, name)

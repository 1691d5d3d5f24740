"""The tempering driver against (A) the library calls and results recorded from the driver as it stood before its loops were
folded into one schedule (tests/golden/ladder_traces.json, by tests/golden/make_ladder_traces.py over the recording engine of
tests/recording_engine.py: equal traces are equal launches, copies and synchronisations on the device) and (B) its schedule
function against the order rule of DESIGN.md S21 applied one timestep at a time.  No GPU."""
import itertools
import json
import os

import pytest

import recording_engine as R
from pyisingmontecarlo_amd import tempering as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ladder_traces.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("kind", R.KINDS)
def test_every_call_makes_the_recorded_library_calls_and_returns_the_recorded_values(capi, golden, monkeypatch, kind):
    monkeypatch.delenv("ISINGMC_PT_HOST", raising=False)
    got = json.loads(json.dumps(R.run_case(T, kind, monkeypatch)))
    want = golden[kind]
    assert [c[0] for c in got] == [c[0] for c in want]
    for (call, result, trace), (_, want_result, want_trace) in zip(got, want):
        assert trace == want_trace, call
        assert result == want_result, call


def test_the_fixture_covers_what_it_is_for(golden):
    """Every kind of ladder; real swaps; the fused call cut by a sample; a move, a sample and a round on one boundary."""
    assert set(golden) == set(R.KINDS)
    for kind, calls in golden.items():
        swaps = [c[1] for c in calls if c[0] == "get_total_swaps()"]
        assert swaps[0] > 0 and swaps[-1] > 0, kind
    names = lambda calls, call: [e[1] for c in calls if c[0] == call for e in c[2]]   # noqa: E731
    cut = names(golden["pair_stream"], "timesteps(24, 2)")
    assert "pt_run" in cut and "record" in cut and "pt_swap" in cut
    for kind in ("pair_host", "pair_stream"):
        meet = names(golden[kind], "timesteps(12, 4)")
        i = len(meet) - 1 - meet[::-1].index("icm_between")
        assert meet[i + 1] == "record" and meet[i + 2] in ("pt_measure", "energies")


def brute_force(t, n_steps, f, k, every, origin, sample):
    """(move, overlap sample, round, state sample) per timestep of the call: the S21 rule, literally."""
    out = []
    for done in range(1, n_steps + 1):
        out.append((bool(k) and t % k == k - 1, bool(every) and (t + 1 - origin) % every == 0, f > 0 and done % f == 0,
                    bool(sample) and done % sample == 0))
        t += 1
    return out


def expand(stretches, f):
    """The stretches of schedule() as one (move, overlap sample, round, state sample) per timestep."""
    out, done = [], 0
    for n, kind, overlap_due, round_due, sample_due in stretches:
        for i in range(1, n + 1):
            done += 1
            inside = kind == T.FUSED and done % f == 0   # a fused stretch holds its rounds, and nothing else
            out.append((kind == T.MOVE, False, inside, False) if i < n else
                       (kind == T.MOVE, overlap_due, round_due or inside, sample_due))
    return out


GRID = list(itertools.product(range(8), range(14), (0, 1, 2, 3, 5), (0, 1, 2, 3, 4), (0, 1, 3, 4), (0, 2)))


@pytest.mark.parametrize("fuse", [T.NO_FUSE, T.FUSE_ROUNDS, T.FUSE_CALL])
@pytest.mark.parametrize("sample", [0, 1, 2, 3])
def test_schedule_against_the_rule_one_timestep_at_a_time(fuse, sample):
    for t, n_steps, f, k, every, origin in GRID:
        got = list(T.schedule(t, n_steps, f, k, every, origin, sample=sample, fuse=fuse))
        where = (t, n_steps, f, k, every, origin, sample, fuse)
        assert expand(got, f) == brute_force(t, n_steps, f, k, every, origin, sample), where
        done = 0
        for j, (n, kind, overlap_due, round_due, sample_due) in enumerate(got):
            assert n > 0 and (n == 1 or kind != T.MOVE), where
            if kind == T.FUSED:   # only where asked for, from a round boundary, whole rounds (or the call's end), nothing due behind it
                assert fuse and f and done % f == 0 and not (overlap_due or round_due or sample_due), where
                assert n % f == 0 or (fuse == T.FUSE_CALL and done + n == n_steps and not (every or sample)), where
            done += n
            if kind == T.SWEEPS and done < n_steps:   # no stretch ends where nothing happens
                assert overlap_due or round_due or sample_due or got[j + 1][1] == T.MOVE, where
        assert done == n_steps, where
        if fuse == T.NO_FUSE:
            assert all(kind != T.FUSED for _, kind, _, _, _ in got), where
        elif f and not (k or every or sample) and n_steps >= f:   # an uncut call: one library call, or whole rounds and the rest
            assert [(n, kind) for n, kind, _, _, _ in got] == ([(n_steps, T.FUSED)] if fuse == T.FUSE_CALL or n_steps % f == 0 else
                                                               [(n_steps // f * f, T.FUSED), (n_steps % f, T.SWEEPS)]), where


def test_frequencies_are_normalised_in_one_place():
    assert T._frequencies(None, None) == (1, 1) and T._frequencies(0, 2) == (0, 2) and T._frequencies(-3, 5) == (0, 5)
    with pytest.raises(ValueError, match="sampling_freq must be positive"):
        T._frequencies(1, 0)

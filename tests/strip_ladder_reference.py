"""The cases of the strip-ladder census (tests/test_gpu_strip_ladder.py) and everything they need that is not the kernel -- TEST
INFRASTRUCTURE, no GPU.  lat_strip_kernel<PMJ, NW, LAD = true> (csrc/strip_kernels.hpp) holds the exchange rounds of a
tempering ladder inside one persistent launch; which instantiation a ladder runs on follows from the couplings' signs (PMJ) and
the strip_nw option (NW).  Here: the two selection rules restated (strip_plan and pt_rounds_in_kernel of csrc/step_policy.hpp, which
isingmc_pt_run of csrc/tempering.hip asks; tests/test_step_policy_host.py holds the restatements against them), the smallest shapes of every geometry branch, the couplings, the ladders with their call
sequences, and the host twin: ClassicalTempering on the host swap step over the CPU oracle engine, driven one round at a time, its
rounds recorded through the numpy rule of ladder_statistics_reference.py.  tests/test_strip_ladder_host.py proves without a GPU that
the cases select what they claim and that the twin's rounds are not vacuous."""
import copy
import functools
from collections import namedtuple

import numpy as np

import ladder_statistics_reference as SR
from helpers import OracleLatEngine
from oracle import exact as X


# ---- strip_plan (csrc/step_policy.hpp) restated -----------------------------------------------------------------------------------
def strip_plan(W, H, nw):
    """(qpr, S, strips) of a W x H lattice cut into strips of nw wavefronts, None where the strip kernel does not serve it: a row
    holds qpr = W / 256 quads (4 words of 32 spins of one colour), a power of two <= 32; a strip is S = 64 nw / qpr rows; the
    strips divide the lattice and there are at least two."""
    if nw not in (1, 4) or W % 256:
        return None
    qpr = W // 256
    if qpr & (qpr - 1) or not 1 <= qpr <= 32:
        return None
    S = 64 * nw // qpr
    if H % S or H // S < 2:
        return None
    return qpr, S, H // S


# ---- pt_rounds_in_kernel (csrc/step_policy.hpp), the in_kernel condition of isingmc_pt_run, restated ------------------------------
def rounds_inside_the_launch(n_slots, n_rungs, timesteps, swap_every, passes=1, tracking=False):
    """Exchange rounds that pt_run(timesteps, swap_every) decides inside one persistent launch, 0 where it takes one launch per
    round: at least two rounds, the container holds the whole ladder, rounds * swap_every <= 65536 timesteps, every replica in one
    pass, no minimum / moment / overlap-series tracking.  The last round of the call is always decided at the kernel boundary."""
    rounds = timesteps // swap_every
    if rounds < 2 or n_slots != n_rungs or rounds * swap_every > 65536 or passes != 1 or tracking:
        return 0
    return rounds - 1


# what tests/test_strip_ladder_host.py asserts of the two restatements beside the shapes table, and tests/test_step_policy_host.py of
# the library's rules: ((W, H, nw), expected strip_plan) and ((n_slots, n_rungs, timesteps, swap_every[, passes, tracking]), expected)
STRIP_PLAN_CASES = (((768, 256, 4), None), ((16384, 16, 4), None),                      # qpr = 3; qpr = 64
                    ((256, 128, 4), None), ((256, 128, 1), (1, 64, 2)),                 # the same lattice, cut by NW
                    ((8192, 4, 4), None), ((1024, 48, 4), None))                        # the NW = 1 shapes exist for NW = 1 only
IN_KERNEL_CASES = (((8, 8, 26, 4), 5), ((8, 8, 9, 3), 2), ((8, 8, 7, 1), 6),            # (the first two: test_inside_the_persistent_launch)
                   ((8, 8, 3, 3), 0), ((8, 8, 5, 3), 0),                                # one round: at the kernel boundary
                   ((4, 8, 26, 4), 0),                                                  # a shard of the ladder
                   ((8, 8, 65536, 1), 65535), ((8, 8, 65537, 1), 0), ((8, 8, 65540, 2), 0),
                   ((8, 8, 65537, 3), 21844),                                           # 21845 rounds = 65535 timesteps: the tail does not count
                   ((8, 8, 26, 4, 2), 0), ((8, 8, 26, 4, 1, True), 0),                  # two passes; tracking
                   ((1, 1, 8, 1), 7))                                                   # a ladder of one rung still runs its rounds inside

# ---- shapes: the smallest at which each geometry branch of the kernel exists -------------------------------------------------------
#        NW: ((W, H), qpr, S, strips)
SHAPES = {1: (((256, 128), 1, 64, 2),     # up-neighbour and down-neighbour strip are the same strip
              ((1024, 48), 4, 16, 3),
              ((8192, 4), 32, 2, 2)),     # every row of a strip is a boundary row
          4: (((256, 512), 1, 256, 2),    # the ql < 6 wave-pair row mapping
              ((1024, 192), 4, 64, 3),
              ((8192, 16), 32, 8, 2))}

# ---- couplings ---------------------------------------------------------------------------------------------------------------------
#            name: (J, glass)   every |J| is dyadic: all energies are exact in f64
COUPLINGS = {"fm": (-1.0, False), "half": (-0.5, False), "afm": (1.0, False), "glass": (-1.0, True)}

# ---- call sequences: warm-up timesteps (no round), then two pt_run(timesteps, swap_every) ------------------------------------------
# A: 7 rounds after every timestep (odd: the second call starts on an odd round; 6 inside the launch: the ring of four mailboxes and
#    both counter parities wrap), then 3 rounds after every 3rd timestep and a tail of 2
# B: 3 rounds after every 3rd timestep and a tail of 1 (odd again), then 8 rounds after every timestep (7 inside the launch)
# C: A at length: 21 rounds and 5 rounds with a tail of 1 -- enough rounds for a replica to travel down a 5-rung ladder and back
SCHEDULES = {"A": (2, ((7, 1), (11, 3))), "B": (2, ((10, 3), (8, 1))), "C": (2, ((21, 1), (16, 3)))}

Case = namedtuple("Case", "name nw W H coupling schedule seed contains betas fallback")


def _case(nw, shape, coupling, schedule, seed, contains, betas, fallback=False):
    W, H = shape
    name = f"nw{nw}-{W}x{H}-{coupling}-{len(betas)}rungs-{schedule}"
    return Case(name, nw, W, H, coupling, schedule, seed, contains, tuple(float(b) for b in betas), fallback)


# The betas were searched with the oracle engine alone (the twin below, on a CPU), so that every ladder's rounds hold what
# tests/test_strip_ladder_host.py asks of them.  Above every ladder, what its twin's rounds contain (Case.contains: the host test
# recounts it):
#   att = pairs attempted, acc = accepted in all, "+" = accepted with d >= 0, "a" = accepted with -40 <= d < 0,
#   "r" = refused with -40 <= d < 0, "R" = refused with d < -40 (strip_det_exp returns 0), trips = completed round trips
CASES = (
    # -- <PMJ = false, NW = 1> --------------------------------------------------------------------------------------------------------
    _case(1, (256, 128), "fm", "A", 11, "att 0 acc 0 + 0 a 0 r 0 R 0 trips 0",
          [0.4400]),
    _case(1, (1024, 48), "half", "B", 12, "att 6 acc 6 + 3 a 3 r 0 R 0 trips 5",
          [0.8800, 0.8810]),
    _case(1, (256, 128), "afm", "C", 13, "att 52 acc 43 + 19 a 24 r 9 R 0 trips 4",
          [0.4400, 0.4404, 0.4408, 0.4412, 0.4416]),
    _case(1, (8192, 4), "fm", "B", 14, "att 22 acc 13 + 6 a 7 r 4 R 5 trips 0",
          [0.4400, 0.4410, 0.4420, 0.4430, 0.6000], fallback=True),
    _case(1, (1024, 48), "afm", "A", 15, "att 35 acc 28 + 18 a 10 r 7 R 0 trips 0",
          [0.4400, 0.4410, 0.4420, 0.4430, 0.4440, 0.4450, 0.4460, 0.4470]),
    # -- <PMJ = true, NW = 1> ---------------------------------------------------------------------------------------------------------
    _case(1, (8192, 4), "glass", "B", 21, "att 0 acc 0 + 0 a 0 r 0 R 0 trips 0",
          [0.9000]),
    _case(1, (256, 128), "glass", "A", 22, "att 5 acc 5 + 1 a 4 r 0 R 0 trips 4",
          [0.9000, 0.9020]),
    _case(1, (1024, 48), "glass", "A", 23, "att 20 acc 13 + 6 a 7 r 2 R 5 trips 0",
          [0.9000, 0.9020, 0.9040, 0.9060, 1.2000], fallback=True),
    _case(1, (8192, 4), "glass", "B", 24, "att 39 acc 35 + 15 a 20 r 4 R 0 trips 2",
          [0.9000, 0.9020, 0.9040, 0.9060, 0.9080, 0.9100, 0.9120, 0.9140]),
    # -- <PMJ = false, NW = 4> --------------------------------------------------------------------------------------------------------
    _case(4, (1024, 192), "half", "B", 31, "att 0 acc 0 + 0 a 0 r 0 R 0 trips 0",
          [0.8800]),
    _case(4, (8192, 16), "fm", "A", 32, "att 5 acc 3 + 2 a 1 r 2 R 0 trips 2",
          [0.4400, 0.4405]),
    _case(4, (1024, 192), "afm", "A", 33, "att 20 acc 11 + 8 a 3 r 4 R 5 trips 0",
          [0.4400, 0.4405, 0.4410, 0.4415, 0.6000], fallback=True),
    _case(4, (256, 512), "fm", "B", 34, "att 39 acc 30 + 15 a 15 r 9 R 0 trips 0",
          [0.4400, 0.4405, 0.4410, 0.4415, 0.4420, 0.4425, 0.4430, 0.4435]),
    # -- <PMJ = true, NW = 4> ---------------------------------------------------------------------------------------------------------
    _case(4, (256, 512), "glass", "A", 41, "att 0 acc 0 + 0 a 0 r 0 R 0 trips 0",
          [0.9000]),
    _case(4, (1024, 192), "glass", "B", 42, "att 6 acc 5 + 3 a 2 r 1 R 0 trips 4",
          [0.9000, 0.9010]),
    _case(4, (8192, 16), "glass", "B", 43, "att 22 acc 15 + 6 a 9 r 2 R 5 trips 0",
          [0.9000, 0.9010, 0.9020, 0.9030, 1.2000], fallback=True),
    _case(4, (256, 512), "glass", "A", 44, "att 35 acc 33 + 23 a 10 r 2 R 0 trips 1",
          [0.9000, 0.9010, 0.9020, 0.9030, 0.9040, 0.9050, 0.9060, 0.9070]),
)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
INSTANTIATIONS = tuple((pmj, nw) for pmj in (False, True) for nw in (1, 4))


def instantiation(case):
    """(PMJ, NW) of the lat_strip_kernel<PMJ, NW, true> that the case's ladder runs on"""
    return COUPLINGS[case.coupling][1], case.nw


def calls(case):
    return SCHEDULES[case.schedule][1]


def warm_up(case):
    return SCHEDULES[case.schedule][0]


@functools.lru_cache(maxsize=None)
def edges(case):
    """(ea, eb, ej) of the case's lattice; the glass is seeded by the case"""
    J, glass = COUPLINGS[case.coupling]
    return X.square_lattice_edges(case.W, case.H, J, np.random.default_rng(1000 + case.seed) if glass else None)


def oracle_engine(case):
    """the CPU oracle behind the engine interface of ClassicalTempering"""
    J, glass = COUPLINGS[case.coupling]
    if not glass:
        return OracleLatEngine(case.W, case.H, abs(J), int(J > 0))
    ej = edges(case)[2]
    return OracleLatEngine(case.W, case.H, abs(J), 0, (ej[0::2] > 0).astype(np.uint8), (ej[1::2] > 0).astype(np.uint8))


# ---- the host twin -----------------------------------------------------------------------------------------------------------------
Pair = namedtuple("Pair", "round lo d accepted")                       # one attempted pair (lo, lo + 1) of one round
After = namedtuple("After", "perm swaps round states energies stats")  # the ladder after one call; stats: SR.Statistics
Twin = namedtuple("Twin", "slot_seeds pairs after")


@functools.lru_cache(maxsize=None)
def twin(case):
    """The case's ladder on the host swap step over the oracle engine: the warm-up, then every call one round at a time.  Computed
    once per case and shared: nobody changes what it returns."""
    from pyisingmontecarlo_amd.tempering import ClassicalTempering
    pt = ClassicalTempering(edges(case), seed=case.seed, engine_factory=lambda: oracle_engine(case))
    for b in case.betas:
        pt.add_graph(b)
    G, betas = len(case.betas), np.array(case.betas)
    ref, pairs, after = SR.Statistics(G), [], []
    pt.timesteps(warm_up(case))
    for T, f in calls(case):
        for _ in range(T // f):
            pt.timesteps(f)
            before, energies, rnd = pt._perm.copy(), pt._states.energies(), pt._round
            pt._swap_step()
            ref.round(rnd, before, pt._perm, energies)
            for lo in range(rnd & 1, G - 1, 2):   # d as the exchange step forms it: f64, (beta_lo - beta_hi) (E_lo - E_hi)
                d = (betas[lo] - betas[lo + 1]) * (energies[before[lo]] - energies[before[lo + 1]])
                pairs.append(Pair(rnd, lo, float(d), bool(before[lo] != pt._perm[lo])))
        if T % f:
            pt.timesteps(T % f)
        after.append(After(pt.get_permutation().copy(), pt.get_total_swaps(), pt._round, pt._states.states(), pt._states.energies(),
                           copy.deepcopy(ref)))
    assert not pt._on_stream
    return Twin(tuple(pt._slot_seeds), tuple(pairs), tuple(after))


def counts(pairs):
    """what a ladder's rounds contain, by the letters of the table above"""
    acc = [p for p in pairs if p.accepted]
    ref = [p for p in pairs if not p.accepted]
    return {"att": len(pairs), "acc": len(acc), "+": sum(p.d >= 0 for p in acc), "a": sum(-40 <= p.d < 0 for p in acc),
            "r": sum(-40 <= p.d < 0 for p in ref), "R": sum(p.d < -40 for p in ref)}


def contains(tw):
    """a twin's counts in the words of Case.contains"""
    n = counts(tw.pairs) | {"trips": int(tw.after[-1].stats.round_trips.sum())}
    return " ".join(f"{k} {v}" for k, v in n.items())

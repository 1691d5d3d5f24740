"""A recording stand-in for the engine behind ClassicalTempering -- TEST INFRASTRUCTURE, no GPU, no physics.  Its containers log
every method call (scalars as they are, arrays as lists) into one shared list and return deterministic values: energies are a
fixed function of (slot, timestep), so that the library's host exchange code really swaps.  Two forms: RecStates has the methods
the host swap step uses (plus the move and the series between two containers, with host slot tables); RecStreamStates adds the
pt_* calls of a ladder on the device's stream, carried out on the host by the same exchange code.  RecGroup stands in for
_capi.PtGroup.  run_case() drives one kind of ladder through the call list whose traces tests/golden/ladder_traces.json holds."""
import numpy as np

from pyisingmontecarlo_amd import _capi

KINDS = ("host", "stream", "shards", "pair_host", "pair_stream")
BETAS = (0.1, 0.2, 0.3, 0.4, 0.5)
NVARS = 4


def plain(x):
    """Arguments and results as JSON holds them: arrays and tuples as lists, NaN as None, containers by name."""
    if isinstance(x, (RecStates, RecSeries)):
        return x.name
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, np.ndarray):
        x = x.tolist()
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, (np.integer, np.bool_)):
        return x.item()
    if isinstance(x, (float, np.floating)):
        return None if np.isnan(x) else float(x)
    return x


class RecSeries:
    def __init__(self, log, name, by_rung):
        self.log, self.name, self.by_rung, self.rows = log, name, by_rung, 0

    def _call(self, method, *args):
        self.log.append(plain([self.name, method] + list(args)))

    def record(self, slots_a=None, slots_b=None):
        self._call("record", slots_a, slots_b)
        self.rows += 1

    def get(self):
        self._call("get")
        return self.rows

    def reset(self):
        self._call("reset")
        self.rows = 0

    def close(self):
        self._call("close")


class RecStates:
    def __init__(self, log, name, seeds, lo, hi):
        self.log, self.name, self.seeds, self.lo, self.hi, self.t = log, name, [int(s) for s in seeds], lo, hi, 0

    def _call(self, method, *args):
        self.log.append(plain([self.name, method] + list(args)))

    def _energy(self, t):
        """float64[n_local]: what the slots of this container measure after timestep t - 1."""
        return np.array([float((3 * s + 5 * t + self.seeds[s] % 7) % 13) - 6.0 for s in range(self.lo, self.hi)])

    def set_betas(self, betas):
        self._call("set_betas", betas)

    def do_time_steps(self, timesteps, beta=None, per_step_energies=False):
        self._call("do_time_steps", timesteps, beta, per_step_energies)
        out = np.stack([self._energy(self.t + k + 1) for k in range(timesteps)], axis=1) if per_step_energies else None
        self.t += timesteps
        return out

    def energies(self):
        self._call("energies")
        return self._energy(self.t)

    def states(self, out=None):
        self._call("states")
        res = np.array([[(5 * s + 3 * self.t + i) % 3 == 0 for i in range(NVARS)] for s in range(self.lo, self.hi)], dtype=np.bool_)
        if out is None:
            return res
        out[...] = res
        return out

    def set_track_best(self, k):
        self._call("set_track_best", k)

    def best_update(self):
        self._call("best_update")

    def icm_between(self, other, slots_a=None, slots_b=None):
        self._call("icm_between", other, slots_a, slots_b)
        self.t += 1
        other.t += 1

    def overlap_series(self, other=None, n_pairs=None, classes=None, link=True, by_rung=False, capacity=4096):
        self._call("overlap_series", other, n_pairs, classes, link, by_rung, capacity)
        return RecSeries(self.log, self.name + ".series", by_rung)


class RecStreamStates(RecStates):
    def pt_can_attach(self, n_rungs, slot_offset, slots_per_rank, world_size):
        self._call("pt_can_attach", n_rungs, slot_offset, slots_per_rank, world_size)
        return True

    def pt_attach(self, ladder_betas, slot_offset, slots_per_rank, world_size, seed):
        self._call("pt_attach", ladder_betas, slot_offset, slots_per_rank, world_size, seed)
        G = len(ladder_betas)
        self.pt_betas, self.pt_seed, self.per, self.world = [float(b) for b in ladder_betas], int(seed), slots_per_rank, world_size
        self.perm, self.round, self.swaps = np.arange(G, dtype=np.uint32), 0, 0
        self.measured, self.gathered = None, None     # this shard's energies / every rank's blocks of `per` (a RecGroup fills it)
        self.stats, self.stats_on = None, False

    def pt_buffers(self):
        self._call("pt_buffers")
        return None, None

    def pt_time_steps(self, timesteps):
        self._call("pt_time_steps", timesteps)
        self.t += timesteps

    def _round(self, in_kernel=False):
        G = len(self.pt_betas)
        all_e = self.measured if self.world == 1 else self.gathered
        slot_e = np.concatenate([all_e[r * self.per:r * self.per + self.per] for r in range(self.world)])[:G] if self.world > 1 else all_e
        before = self.perm.copy()
        self.swaps += _capi.pt_swap_round(self.pt_seed, self.round, self.pt_betas, slot_e, self.perm)
        if self.stats_on:
            _capi.pt_statistics_round(self.stats, self.round, before, self.perm, slot_e)
            self.stats["in_kernel_rounds"] += int(in_kernel)
        self.round += 1

    def pt_run(self, timesteps, swap_every):
        self._call("pt_run", timesteps, swap_every)
        assert self.world == 1
        for _ in range(timesteps // swap_every):
            self.t += swap_every
            self.measured = self._energy(self.t)
            self._round(in_kernel=True)
        self.t += timesteps % swap_every

    def pt_measure(self):
        self._call("pt_measure")
        self.measured = self._energy(self.t)

    def pt_swap(self):
        self._call("pt_swap")
        self._round()

    def pt_state(self):
        self._call("pt_state")
        return self.perm.copy(), self.round, self.swaps

    def pt_set_statistics(self, on=True):
        self._call("pt_set_statistics", on)
        if self.stats is None:
            self.stats = _capi.pt_statistics_zeros(len(self.pt_betas))
        self.stats_on = bool(on)

    def pt_statistics(self):
        self._call("pt_statistics")
        return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.stats.items()}

    def pt_reset_statistics(self):
        self._call("pt_reset_statistics")
        self.stats = _capi.pt_statistics_zeros(len(self.pt_betas))

    def synchronize(self):
        self._call("synchronize")


class RecEngine:
    """make_states logs and hands out containers named after the order they were made in: a, b, ..."""

    def __init__(self, log, names, stream, device=None):
        self.log, self.names, self.stream, self.device, self.nvars = log, names, stream, device, NVARS
        self.supports_on_stream_pt = stream

    def make_states(self, seeds, replica_range=None):
        name = next(self.names)
        self.log.append(plain([name, "make_states", self.device, seeds, replica_range]))
        lo, hi = replica_range if replica_range is not None else (0, len(seeds))
        return (RecStreamStates if self.stream else RecStates)(self.log, name, seeds, lo, hi)


class RecGroup:
    """_capi.PtGroup over RecStreamStates shards: the all-gather hands every shard every shard's block."""

    def __init__(self, log, shards, backend=0):
        self.log, self.shards, self.backend = log, list(shards), "copy"
        log.append(["group", "create", [s.name for s in self.shards], backend])

    def allgather(self):
        self.log.append(["group", "allgather"])
        self._gather()

    def _gather(self):
        per = self.shards[0].per
        blocks = [np.concatenate([s.measured, np.zeros(per - len(s.measured))]) for s in self.shards]
        for s in self.shards:
            s.gathered = np.concatenate(blocks)

    def run(self, timesteps, swap_every):
        self.log.append(["group", "run", timesteps, swap_every])
        for _ in range(timesteps // swap_every):
            for s in self.shards:
                s.t += swap_every
                s.measured = s._energy(s.t)
            self._gather()
            for s in self.shards:
                s._round(in_kernel=True)
        for s in self.shards:
            s.t += timesteps % swap_every

    def synchronize(self):
        self.log.append(["group", "synchronize"])


def make_ladder(tempering, kind, log, monkeypatch, seed=11, moves=0):
    """A 5-rung ladder of one of KINDS on recording engines; monkeypatch (pytest's, or anything with its setattr) swaps
    tempering.HipEngine and _capi.PtGroup for the in-process kind."""
    stream = kind in ("stream", "shards", "pair_stream")
    edges = [((i, (i + 1) % NVARS), 1.0) for i in range(NVARS)]
    names = iter("abcdefgh")
    if kind == "shards":
        monkeypatch.setattr(tempering, "HipEngine", lambda ea, eb, ej, nvars, device=0: RecEngine(log, names, True, device))
        monkeypatch.setattr(_capi, "PtGroup", lambda shards, backend=0: RecGroup(log, shards, backend))
        lad = tempering.ClassicalTempering(edges, seed, devices=[0, 0])
    else:
        lad = tempering.ClassicalTempering(edges, seed, engine_factory=lambda: RecEngine(log, names, stream),
                                           copies=2 if kind.startswith("pair") else 1)
    for beta in BETAS:
        lad.add_graph(beta)
    if moves:
        lad.set_replica_cluster_update_every(moves)
    return lad


def run_case(tempering, kind, monkeypatch):
    """The call list of one kind of ladder: [[call, returned value or error, the library calls it made], ...].  Ladder A takes
    the calls without cluster moves, ladder B (copies=2: a move every 3rd timestep) the ones where a move, a sample and a round
    meet, and the sampling form again, now cut at moves."""
    pair = kind.startswith("pair")
    log, out = [], []

    def call(lad, name, *args):
        try:
            res = getattr(lad, name)(*args)
        except ValueError as e:
            res = "ValueError: " + str(e)
        if name == "timesteps_sample" and not isinstance(res, str):   # shapes, the states as bits, the energies
            res = [[list(r.shape), str(r.dtype)] for r in res] + [np.packbits(res[0]).tolist(), res[1]]
        out.append(plain([name + repr(args), res, list(log)]))
        del log[:]

    a = make_ladder(tempering, kind, log, monkeypatch)
    call(a, "set_ladder_statistics", True)
    call(a, "timesteps", 7, 2)
    call(a, "get_permutation")
    call(a, "get_total_swaps")
    call(a, "timesteps", 5)
    call(a, "set_ladder_statistics", False)
    call(a, "timesteps", 6, 3)
    call(a, "get_ladder_statistics")
    call(a, "set_ladder_statistics", True)
    call(a, "timesteps", 0)
    call(a, "set_track_minimum", True)
    if pair:
        call(a, "set_measure_overlaps_every", 5)
    call(a, "timesteps", 24, 2)
    call(a, "get_permutation")
    call(a, "get_total_swaps")
    call(a, "get_ladder_statistics")
    call(a, "reset_ladder_statistics")
    call(a, "timesteps_sample", 12, 3, 4)
    call(a, "timesteps_sample", 7, 0, 2)
    call(a, "get_ladder_statistics")
    call(a, "timesteps_sample", 5)
    call(a, "get_permutation")
    call(a, "get_total_swaps")
    if pair:
        call(a, "get_measured_overlaps")
        b = make_ladder(tempering, kind, log, monkeypatch, seed=12, moves=3)
        call(b, "set_measure_overlaps_every", 4)
        call(b, "timesteps", 12, 4)
        call(b, "timesteps_sample", 12, 3, 4)
        call(b, "timesteps", 7, 2)
        call(b, "get_permutation")
        call(b, "get_total_swaps")
        call(b, "get_measured_overlaps")
    return out

"""Classical parallel tempering on a beta ladder, with the API shape of the reference's
LatticeTempering (src/tempering.rs:29-299; quantum SSE there -- the classical ladder is this build's
own): add_graph(beta), timesteps(t), timesteps_sample(timesteps, replica_swap_freq,
sampling_freq) -> (bool[G,S,N] states, float64[G] time-averaged energies), get_total_swaps().

Replica slots are sharded over the ranks of a torch.distributed group (one process per GPU) -- or, with
`devices=[...]`, over several GPUs driven by THIS process through the library's own RCCL group
(isingmc_pt_group_*: no torch, no launcher; what a Rust / pyo3 host of the C ABI would use).  The swap
step exchanges TEMPERATURES, never configurations: every rank all-gathers one float64 energy per slot
(RCCL over xGMI with backend nccl), evaluates the same Philox-keyed decisions in libisingmc's host code
(isingmc_host_pt_swap_round) and re-labels its own slots' betas.  No spin ever crosses a link.
"""
import os

import numpy as np

from . import _capi
from . import distributed as D


class HipEngine:
    """Default engine: the HIP library through the C ABI.  (Tests inject a CPU-oracle engine with the
    same two methods to exercise the sharding logic without a GPU; the product never does.)"""

    def __init__(self, ea, eb, ej, nvars, device=0):
        self.graph = _capi.Graph(ea, eb, ej, nvars=nvars, device=device)
        self.nvars = self.graph.nvars
        # sweeps, measurement, exchange decisions and beta relabelling all on the engine's HIP stream: periodic field-free
        # lattices, and graphs on the replica-packed paths (whether a container is packed depends on the graph and its
        # size: pt_attach refuses otherwise and the ladder falls back to the host swap step)
        self.supports_on_stream_pt = ((self.graph.kind == _capi.KIND_LATTICE2D and self.graph.info.fast_path == 0) or
                                      self.graph.kind == _capi.KIND_GENERAL)

    def make_states(self, seeds, replica_range=None):
        """seeds of ALL slots + this rank's [lo, hi): group membership on the replica-packed path follows the global
        slot index, so the ladder's trajectories do not depend on the number of ranks."""
        return _capi.States(self.graph, seeds, replica_range=replica_range)


def _split(edges):
    if isinstance(edges, tuple) and len(edges) == 3 and hasattr(edges[0], "__len__") and not isinstance(edges[0], tuple):
        ea, eb, ej = edges
    else:
        ea = [e[0][0] for e in edges]
        eb = [e[0][1] for e in edges]
        ej = [e[1] for e in edges]
    ea = np.ascontiguousarray(ea, dtype=np.uint64)
    eb = np.ascontiguousarray(eb, dtype=np.uint64)
    ej = np.ascontiguousarray(ej, dtype=np.float64)
    if ea.size == 0:
        raise ValueError("Must supply some edges for graph")
    return ea, eb, ej


def betas_from_flow(betas, n_up, n_down, n_rungs=None):
    """A new ladder from the measured replica flow (get_ladder_statistics()["n_up"], ["n_down"]), by the feedback idea of Katzgraber,
    Trebst, Huse and Troyer (2006): in a ladder that wastes no rung the flow fraction f = n_up / (n_up + n_down) falls linearly
    with the rung index from 1 at rung 0 to 0 at the last rung.  The method: (1) f per rung, with f = 1 at rung 0 and f = 0 at
    the last rung by definition, rungs without a labelled visit taking the linear interpolation in the rung index between their
    measured neighbours; (2) f made monotone by a running maximum from the last rung (the end where f = 0) towards rung 0;
    (3) the piecewise-linear f(beta) through the measured points inverted at the n_rungs (default: as many as before) equidistant
    values 1, ..., 0; (4) the two end betas kept as they are.  Pure numpy, no device.  A heuristic: it moves rungs towards
    the bottlenecks of the measured flow, it needs enough round trips for f to mean anything, and it wants iterating."""
    betas = np.asarray(betas, dtype=np.float64)
    up, down = np.asarray(n_up, dtype=np.float64), np.asarray(n_down, dtype=np.float64)
    n = len(betas)
    m = n if n_rungs is None else int(n_rungs)
    if n < 2 or m < 2 or up.shape != (n,) or down.shape != (n,):
        raise ValueError("betas, n_up and n_down must have one entry per rung of a ladder of at least two rungs")
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(up + down > 0, up / (up + down), np.nan)
    f[0], f[-1] = 1.0, 0.0
    known = ~np.isnan(f)
    f = np.interp(np.arange(n), np.flatnonzero(known), f[known])
    f = np.maximum.accumulate(f[::-1])            # from the last rung on: non-decreasing, 0 ... 1
    target = (m - 1 - np.arange(m)) / float(m - 1)
    out = np.interp(target, f, betas[::-1])
    out[0], out[-1] = betas[0], betas[-1]
    return out


TRACK_AT_ROUNDS = 1 << 62      # set_track_best period of a ladder: no timestep reaches it, the exchange rounds update the records
COPY_SEED_XOR = 0x9E3779B97F4A7C15  # copy 1 of a copies=2 ladder is the ladder of seed ^ this

SWEEPS, MOVE, FUSED = 0, 1, 2               # a stretch of schedule(): Metropolis sweeps, one cluster move, sweeps with their rounds inside
NO_FUSE, FUSE_ROUNDS, FUSE_CALL = 0, 1, 2   # what a ladder takes as one FUSED library call: nothing, whole rounds, the call's partial last block too


def schedule(t, T, f=0, k=0, every=0, origin=0, sample=0, fuse=NO_FUSE):
    """Where a call of T timesteps that starts at absolute timestep t is cut: the countdown of tempering.rs:172-212 and the order
    rule of DESIGN.md S21, for every loop of this file.  Pure: integers in, integers out.  f: an exchange round after every f-th
    timestep of the CALL (<= 0: none; a partial last block gets none); k: absolute timestep u is a cluster move iff u % k == k - 1
    (0: none); every, origin: an overlap sample follows timestep u iff (u + 1 - origin) % every == 0 (0: none); sample: a state
    sample follows every sample-th timestep of the call (0: none).  Yields (n, kind, overlap_due, round_due, sample_due) per
    stretch: n timesteps of one kind -- SWEEPS, MOVE (n == 1) or, where `fuse` allows, FUSED: sweeps with their rounds inside one
    library call, starting on a round boundary and ending before the next sample or move -- and what follows the stretch's last
    timestep, in this order: the overlap sample, the exchange round, the state sample."""
    f, done = max(int(f), 0), 0
    if fuse == FUSE_CALL and f and T > 0 and not (k or every or sample):   # nothing cuts the call: the closed form, no loop to set up
        yield T, FUSED, False, False, False
        return
    while done < T:
        kind, n = SWEEPS, T - done
        if k and t % k == k - 1:
            kind, n = MOVE, 1
        else:
            if k:
                n = min(n, k - 1 - t % k)   # Metropolis timesteps before the next cluster move
            u = every - (t - origin) % every if every else None   # timesteps up to and including the one the next sample follows
            if sample and (u is None or sample - done % sample < u):
                u = sample - done % sample
            fused = 0
            if f and fuse and done % f == 0:
                fused = (n if u is None else min(n, u - 1)) // f * f   # the sample goes between its timestep and that timestep's round
                if fuse == FUSE_CALL and u is None and n == T - done:
                    fused = n
            if fused:
                kind, n = FUSED, fused
            else:
                n = min(n, f - done % f) if f else n
                n = n if u is None else min(n, u)
        t, done = t + n, done + n
        yield (n, kind, bool(every) and (t - origin) % every == 0, kind != FUSED and f > 0 and done % f == 0,
               bool(sample) and done % sample == 0)


def _frequencies(replica_swap_freq, sampling_freq):
    """(exchange period, sampling period) of timesteps_sample: both default to 1 (tempering.rs:163-164), <= 0 exchanges never."""
    sampling_freq = 1 if sampling_freq is None else int(sampling_freq)
    if sampling_freq <= 0:
        raise ValueError("sampling_freq must be positive")
    return max(1 if replica_swap_freq is None else int(replica_swap_freq), 0), sampling_freq


def _inverse(perm):
    """slot -> rung from rung -> slot."""
    inv = np.empty(len(perm), dtype=np.int64)
    inv[perm] = np.arange(len(perm))
    return inv


def _by_rung(states, rungs):
    """bool[C, G, S, N] by slot and the rung every slot held at every sample, int64[C, G, S] -> the states by rung."""
    out = np.empty_like(states)
    for c in range(states.shape[0]):
        for s in range(states.shape[2]):
            out[c, rungs[c, :, s], s, :] = states[c, :, s, :]
    return out


class _HostLadder:
    """What the loops of ClassicalTempering need of a ladder -- sweep, plain, exchange, slot_sums, read_states, perm, total_swaps,
    synchronize, the three statistics calls; `fuse` and, where it is not NO_FUSE, run -- chosen once when the ladder is built.
    This one is the host swap step, on any number of ranks: one float64 per slot gathered over the ranks, the decisions in the
    library's host code, the betas pushed back into the container.  Permutation, round and swap counts live on the owner."""
    fuse, backend = NO_FUSE, None

    def __init__(self, owner):
        self.o, self.st, self.local = owner, owner._states, owner._hi > owner._lo
        self.stats = None   # the arrays of _capi.pt_statistics_zeros
        self.push_betas()

    def push_betas(self):
        o = self.o
        beta_of_slot = np.empty(len(o._betas), dtype=np.float64)
        beta_of_slot[o._perm] = o._betas
        if self.local:
            self.st.set_betas(beta_of_slot[o._lo:o._hi])

    def sweep(self, n):
        if self.local:
            self.st.do_time_steps(n)

    plain = sweep   # timesteps(t) without a period; on the device's stream too it stays do_time_steps and does not wait

    def gather(self, local):
        """float64[G] in slot order on every rank, from every rank's block: the swap step's all-gather."""
        o, G = self.o, len(self.o._betas)
        gathered = D.all_gather_f64(local, o._per, o._group)
        out = np.empty(G, dtype=np.float64)
        for r in range(o._world):
            lo, hi = D.shard_bounds(G, o._world, r)
            out[lo:hi] = gathered[r * o._per:r * o._per + (hi - lo)]
        return out

    def slot_sums(self, n):
        """n timesteps; every slot's energy summed over them, float64[G] on every rank."""
        return self.gather(self.st.do_time_steps(n, per_step_energies=True).sum(axis=1) if self.local else np.zeros(0))

    def exchange(self):
        o = self.o
        local = self.st.energies() if self.local else np.zeros(0)
        if o._track_minimum and self.local:
            self.st.best_update()
        slot_e = self.gather(local)
        before = o._perm.copy() if o._stats_on else None
        o._total_swaps += _capi.pt_swap_round(o._seed, o._round, o._betas, slot_e, o._perm)
        if o._stats_on:   # the host twin of what the exchange kernels keep; every rank computes the same
            _capi.pt_statistics_round(self.stats, o._round, before, o._perm, slot_e)
        o._round += 1
        self.push_betas()

    def read_states(self, out):
        if self.local:
            self.st.states(out=out)

    def perm(self):
        return self.o._perm

    def total_swaps(self):
        return self.o._total_swaps

    def synchronize(self):
        pass

    def set_statistics(self, on):
        if self.stats is None:
            self.stats = _capi.pt_statistics_zeros(len(self.o._betas))

    def raw_statistics(self):
        return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.stats.items()}

    def reset_statistics(self):
        self.stats = _capi.pt_statistics_zeros(len(self.o._betas))


class _StreamLadder(_HostLadder):
    """The ladder on the engine's HIP stream, alone or as a rank of a torch group (every rank then holds slots): sweeps,
    measurement, exchange decisions and beta relabelling are enqueued, the device owns permutation and counts.  plain, gather,
    slot_sums and read_states are the host ladder's."""

    def __init__(self, owner):
        self.o, self.st, self.local, self.shards = owner, owner._states, True, [owner._states]
        self.st.pt_attach(owner._betas, owner._lo, owner._per, owner._world, owner._seed)
        self.local_e, self.all_e = self.st.pt_buffers()
        self.stream = self.st.pt_stream() if owner._world > 1 else None
        self.fuse = FUSE_CALL if owner._world == 1 else NO_FUSE   # single rank: a whole call is one library call (one persistent launch on mid-size lattices)

    def sweep(self, n):
        for st in self.shards:
            st.pt_time_steps(n)

    def run(self, n, f):
        self.st.pt_run(n, f)

    def exchange(self):
        # measure -> [RCCL all-gather on the engine's stream] -> exchange kernel: nothing waits on the host
        self.st.pt_measure()
        if self.o._world > 1:
            import torch
            import torch.distributed as dist
            group, world, per = self.o._group, self.o._world, self.o._per
            if dist.get_backend(group) == "nccl":
                with torch.cuda.stream(self.stream):
                    dist.all_gather_into_tensor(self.all_e, self.local_e, group=group)
            else:
                # gloo (several ranks rehearsing on one GPU): the same exchange through the host -- wait for the
                # measurement, gather on the CPU, put the result where the exchange kernel reads it
                self.st.synchronize()
                send = self.local_e.cpu()
                recv = torch.empty(world * per, dtype=torch.float64)
                dist.all_gather_into_tensor(recv, send, group=group)
                self.all_e.copy_(recv)
                torch.cuda.synchronize()
        self.st.pt_swap()

    def perm(self):
        self.o._perm = self.st.pt_state()[0]
        return self.o._perm

    def total_swaps(self):
        return int(self.st.pt_state()[2])

    def synchronize(self):
        self.st.synchronize()

    def set_statistics(self, on):
        for st in self.shards:
            st.pt_set_statistics(True)   # the first switch-on allocates; switched on and off again before any round: zeros
            if not on:
                st.pt_set_statistics(False)

    def raw_statistics(self):
        return self.st.pt_statistics()   # (devices=[...]: shard 0's block; every shard's is the same)

    def reset_statistics(self):
        for st in self.shards:
            st.pt_reset_statistics()


class _GroupLadder(_StreamLadder):
    """The in-process ladder of devices=[...]: one shard per device, the same ladder attached to each, an isingmc_pt_group
    between them.  Shard 0 answers for the ladder's state (perm, total_swaps, raw_statistics: every shard's is the same)."""
    fuse = FUSE_CALL

    def __init__(self, owner, G):
        n = len(owner._devices)
        if n == 0:
            raise ValueError("devices must name at least one GPU")
        owner._per = D.block_size(G, n)
        seeds = np.array(owner._slot_seeds, dtype=np.uint64)
        self.bounds = [D.shard_bounds(G, n, k) for k in range(n)]
        if any(hi <= lo for lo, hi in self.bounds):
            raise ValueError("more devices than blocks of rungs: every device needs at least one slot")
        self.shards = []
        for k, dev in enumerate(owner._devices):
            engine = HipEngine(owner._ea, owner._eb, owner._ej, owner.nvars, device=dev)
            st = engine.make_states(seeds, self.bounds[k])
            if not (engine.supports_on_stream_pt and st.pt_can_attach(G, self.bounds[k][0], owner._per, n)):
                raise ValueError("the in-process ladder needs on-stream tempering on every shard (a periodic field-free lattice or "
                                 "a replica-packed graph; on the bit-sliced path shards of whole 32-slot groups): " + _capi.last_error())
            self.shards.append(st)
        for k, st in enumerate(self.shards):
            st.pt_attach(owner._betas, self.bounds[k][0], owner._per, n, owner._seed)
        self.group = _capi.PtGroup(self.shards, owner._group_backend)
        self.o, self.st = owner, self.shards[0]
        owner._shards, owner._states, owner._lo, owner._hi, owner._on_stream = self.shards, self.shards[0], 0, G, True

    backend = property(lambda self: self.group.backend)

    def plain(self, n):
        self.sweep(n)
        self.synchronize()

    def run(self, n, f):
        self.group.run(n, f)

    def exchange(self):
        for st in self.shards:
            st.pt_measure()
        self.group.allgather()
        for st in self.shards:
            st.pt_swap()

    def slot_sums(self, n):
        return np.concatenate([st.do_time_steps(n, per_step_energies=True).sum(axis=1) for st in self.shards])

    def read_states(self, out):
        for (lo, hi), st in zip(self.bounds, self.shards):
            st.states(out=out[lo:hi])

    def synchronize(self):
        self.group.synchronize()


class ClassicalTempering:
    def __init__(self, edges, seed=None, *, group=None, device=None, engine_factory=None, devices=None, group_backend=0, copies=1, rng_rounds=None):
        """devices: HIP ordinals of an IN-PROCESS ladder -- shard k of the slots lives on devices[k] and the exchange step runs
        through the library's RCCL group (group_backend 0: RCCL when the devices are distinct, else device copies; 1: RCCL;
        2: copies).  Mutually exclusive with a torch.distributed `group`.

        copies=2: two ladders over the same betas on one device, for isoenergetic cluster moves between the two
        configurations at every rung (set_replica_cluster_update_every).  Copy 0 is the ladder copies=1 would build; copy 1 is
        the ladder of the seed `seed ^ COPY_SEED_XOR`.  Single process, single device only.  Served: periodic field-free 2-D
        lattices, and every graph whose containers run on a replica-packed family -- with ISINGMC_FORCE_PACKED=1,
        the stable-path flag or a large enough graph that is the 3-d +-J glass and every Gaussian glass.

        rng_rounds: rounds of Philox4x32 in the draws of the Metropolis sweeps, 10 or 7; None leaves the containers'
        default (10 unless ISINGMC_PHILOX_ROUNDS says 7).  The exchange decisions draw with ten rounds either way.  copies 1 and 2,
        one process, one device: with devices=[...] or a torch.distributed group of several ranks 7 is refused.  ValueError at the
        first timestep when the graph's containers run on a family that 7 does not serve."""
        self._ea, self._eb, self._ej = _split(edges)
        if copies not in (1, 2):
            raise ValueError("copies must be 1 or 2")
        if rng_rounds not in (None, 7, 10):
            raise ValueError("rng_rounds must be 7 or 10")
        self._rng_rounds = None if rng_rounds is None else int(rng_rounds)
        self._ncopies = int(copies)
        self._icm_every = 0
        self._track_minimum = False
        self._pair = None
        self._devices = None if devices is None else [int(d) for d in devices]
        self._group_backend = int(group_backend)
        self._shards = None    # devices=[...]: the containers, one per device
        self._lads = None      # the _HostLadder / _StreamLadder / _GroupLadder behind the loops, one per copy: chosen by _materialise
        self._t = 0            # absolute timestep of the ladder the calls are made on (a pair drives its copies: theirs stays 0)
        if self._devices is not None and (group is not None or D.world_rank(group)[0] > 1):
            raise ValueError("devices=[...] is the in-process ladder: not inside a torch.distributed job")
        self.nvars = int(max(self._ea.max(), self._eb.max())) + 1  # tempering.rs:44-49
        self._group = group
        self._world, self._rank = D.world_rank(group)
        if self._rng_rounds == 7 and (self._devices is not None or self._world > 1):
            raise ValueError("rng_rounds=7 is for a ladder on one process and one device: not with devices=[...] or a "
                             "torch.distributed group of several ranks")
        if seed is None:
            if self._world > 1:
                raise ValueError("a seed is required when the ladder is sharded over several ranks")
            seed = int(_capi.make_seeds(None, 1)[0])
        self._seed = int(seed)
        if self._ncopies == 2:
            if devices is not None:
                raise ValueError("copies=2 is a single-device ladder: not with devices=[...]")
            if self._world > 1:
                raise ValueError("copies=2 is a single-process ladder: not inside a torch.distributed group of several ranks")
            # both copies share ONE engine (one graph handle: the cluster move pairs replicas of one graph); each is a plain
            # copies=1 ladder, the second one on a seed of its own, so that nothing it draws disturbs the first one's stream
            shared = []

            def factory():
                if not shared:
                    shared.append((engine_factory or (lambda: HipEngine(self._ea, self._eb, self._ej, self.nvars,
                                                                         device=self._default_device())))())
                return shared[0]

            self._pair = [ClassicalTempering((self._ea, self._eb, self._ej), s, device=device, engine_factory=factory, rng_rounds=rng_rounds)
                          for s in (self._seed, self._seed ^ COPY_SEED_XOR)]
            self._icm_stats, self._icm_pending = None, False
        self._ovl_series, self._ovl_every, self._ovl_t0, self._ovl_classes = None, 0, 0, None   # overlap series
        self._obs_series, self._obs_every, self._obs_t0 = None, 0, 0   # the observable series by rung, one per copy
        self._betas = []
        self._slot_seeds = []
        self._n_drawn = 0
        self._device = device
        self._engine_factory = engine_factory or (lambda: HipEngine(self._ea, self._eb, self._ej, self.nvars,
                                                                    device=self._default_device()))
        self._states = None
        self._perm = None       # rung -> slot
        self._round = 0
        self._total_swaps = 0
        self._on_stream = False
        self._stats_on, self._stats_seen = False, False   # ladder statistics: counting now / switched on at least once

    def _default_device(self):
        if self._device is not None:
            return self._device
        return int(os.environ.get("ISINGMC_DEVICE", os.environ.get("LOCAL_RANK", "0")))

    # -- tempering.rs:70-113 -------------------------------------------------------------------
    def add_graph(self, beta, seed=None):
        """Add a rung at inverse temperature `beta` (betas must be added in ladder order: the swap
        step pairs neighbouring rungs)."""
        if self._states is not None:
            raise ValueError("add every rung before the first timestep")
        if not np.isfinite(beta):
            raise ValueError("beta must be finite")
        if self._pair is not None:   # copy 0: exactly what a copies=1 ladder does; copy 1 draws from its own stream
            self._pair[0].add_graph(beta, seed)
            self._pair[1].add_graph(beta)
            self._betas.append(float(beta))
            return
        if seed is None:  # seed.unwrap_or_else(|| self.tempering.rng_mut().gen())
            self._n_drawn += 1
            seed = int(_capi.make_seeds(self._seed, self._n_drawn)[-1])
        self._betas.append(float(beta))
        self._slot_seeds.append(int(seed))

    def get_num_graphs(self):
        return len(self._betas)

    def get_total_swaps(self):  # tempering.rs:297-299
        return sum(lad.total_swaps() for lad in self._lads or [])

    def get_betas(self):
        return np.array(self._betas)

    def get_permutation(self):
        """rung -> replica slot currently holding that temperature (copies=2: uint32[2, G], one row per copy)."""
        if self._pair is not None:
            return np.stack([c.get_permutation() for c in self._pair])
        self._materialise()
        return self._lads[0].perm().copy()

    # -------------------------------------------------------------------------------------------
    def set_replica_cluster_update_every(self, k):
        """copies=2 only, before the first timestep: with k > 0 ladder timestep t is an isoenergetic cluster move between the two
        configurations at every rung (S13 on the replica-packed general-graph families) iff t % k == k - 1, in
        place of that timestep's sweep; 0 switches it off.  A graph whose containers run on the f64 CSR family is refused at the
        first move ("general-graph kernel family")."""
        if self._pair is None:
            raise ValueError("replica cluster updates need two configurations per temperature: build the ladder with copies=2")
        if self._states is not None:
            raise ValueError("set the replica cluster update period before the first timestep")
        if int(k) < 0:
            raise ValueError("k must not be negative")
        self._icm_every = int(k)

    def get_replica_cluster_update_every(self):
        return self._icm_every

    def get_replica_cluster_stats(self):
        """The last cluster move per rung: (number of q = -1 clusters, size of the largest, number of q = -1 sites), three
        uint64[G] arrays; None before the first move."""
        if self._pair is None:
            raise ValueError("replica cluster updates need copies=2")
        if self._icm_stats is None and self._icm_pending:
            self._icm_stats = self._pair[0]._states.icm_between_stats()
            self._icm_pending = False
        return self._icm_stats

    def get_overlaps(self, link=True):
        """copies=2 only: (spin, link) between the two configurations currently at every rung, int64[G] each in the order of
        get_betas() (link is None when not asked for): spin = sum_i s_i s'_i, link = sum over the edge-list entries
        of s_a s_b s'_a s'_b.  Pair r is the pair _pair_icm moves: (copy 0's slot at rung r, copy 1's slot at rung r), with the
        ladders' device permutations on the on-stream path and the host tables on the host swap path as slot tables.  Reads
        only: no configuration, random number or timestep changes."""
        if self._pair is None:
            raise ValueError("overlaps need two configurations per temperature: build the ladder with copies=2")
        self._materialise()
        a, b = self._pair
        if not hasattr(a._states, "overlaps"):
            raise ValueError("this engine has no overlap measurement between containers (overlaps)")
        perm = self.get_permutation()
        return a._states.overlaps(b._states, perm[0], perm[1], link=link)

    def site_classes(self, tables, n_classes=None):
        """copies=2 only: the class tables (one array of nvars classes or a stack [n_tables, nvars]) as a device-resident class
        set of the ladder's graph, for get_overlaps_by_class: built once, used at every measurement."""
        if self._pair is None:
            raise ValueError("overlaps need two configurations per temperature: build the ladder with copies=2")
        self._materialise()
        states = self._pair[0]._states
        if not hasattr(states, "overlaps_by_class"):
            raise ValueError("this engine has no overlap measurement by site class (overlaps_by_class)")
        return _capi.SiteClasses(states.graph, tables, n_classes)

    def get_overlaps_by_class(self, classes, n_classes=None):
        """copies=2 only: int64[G, n_tables, n_classes], entry r the spin overlap between the two configurations currently at
        rung r resolved by site class: out[r, t, c] = sum of s_i s'_i over the sites of class c of table t, in the
        order of get_betas() and for the pairs of get_overlaps().  classes: what site_classes() returned, or class tables (a
        class set is then built for this one call).  Reads only."""
        own = not isinstance(classes, _capi.SiteClasses)
        if own:
            classes = self.site_classes(classes, n_classes)
        try:
            self._materialise()
            a, b = self._pair
            perm = self.get_permutation()
            return a._states.overlaps_by_class(classes, b._states, perm[0], perm[1])
        finally:
            if own:
                classes.close()

    # -- the overlaps at every rung, logged on the device once per sample -----------------------------------------
    def set_measure_overlaps_every(self, k, link=True, classes=None, capacity=4096):
        """copies=2 only: from now on a row of overlaps between the two configurations at every rung follows each k-th timestep,
        logged on the device without the host waiting (0: off, the rows stay; a call with k > 0 starts a new log of `capacity`
        rows).  Where several things fall on one boundary the order is the timestep (a sweep or a cluster move), the sample, the
        exchange round: a configuration counts at the beta it was just swept at.  classes: what site_classes() returned, class
        tables, or None.  On the device's stream the pairs are read from the ladders' permutations on the device; on the host
        swap path the host permutations go with every record.  No configuration, random number or exchange decision changes."""
        if int(k) < 0:
            raise ValueError("k must not be negative")
        if self._pair is None:
            raise ValueError("overlaps need two configurations per temperature: build the ladder with copies=2")
        if self._devices is not None or self._world > 1:   # (copies=2 refuses both at construction: kept for the message)
            raise ValueError("the overlap series is for a ladder on one process and one device: not with devices=[...] or a "
                             "torch.distributed group of several ranks")
        if int(k) == 0:
            self._ovl_every = 0
            return
        self._materialise()
        a, b = self._pair
        if not hasattr(a._states, "overlap_series"):
            raise ValueError("this engine has no overlap series (overlap_series)")
        if classes is not None and not isinstance(classes, _capi.SiteClasses):
            classes = self.site_classes(classes)
        series = a._states.overlap_series(b._states, len(self._betas), classes, link=link, by_rung=self._on_stream, capacity=capacity)
        if self._ovl_series is not None:
            self._ovl_series.close()
        self._ovl_series, self._ovl_classes = series, classes
        self._ovl_every, self._ovl_t0 = int(k), self._t

    def get_measured_overlaps(self):
        """(timesteps uint64[n], spin int64[n, G], link int64[n, G] or None, by_class int64[n, G, T, C] or None): the rows logged
        so far in the order of get_betas(), the exact integers of get_overlaps() / get_overlaps_by_class().  Synchronises."""
        if self._ovl_series is None:
            raise ValueError("no overlaps are logged: call set_measure_overlaps_every(k) first")
        return self._ovl_series.get()

    def reset_measured_overlaps(self):
        """The log back to no rows; the period stays."""
        if self._ovl_series is None:
            raise ValueError("no overlaps are logged: call set_measure_overlaps_every(k) first")
        self._ovl_series.reset()

    def _pair_sample(self):
        """The sample behind timestep self._t - 1: before any exchange round on the same boundary."""
        if self._on_stream:
            self._ovl_series.record()   # the rung permutations are read on the device
        else:
            self._ovl_series.record(self._pair[0]._perm, self._pair[1]._perm)

    # -- every slot's lowest-energy configuration ---------------------------------------------------------------
    def set_track_minimum(self, on):
        """Keep, on the device, the lowest-energy configuration every SLOT has held at an exchange round: the round's own energy
        measurement serves the records too (one launch per round while it is on; rounds never run inside one persistent launch).
        Records belong to the slot (the configuration), not to the rung.  copies 1 and 2, one process, one device."""
        if self._devices is not None or self._world > 1:
            raise ValueError("minimum tracking is for a ladder on one process and one device: not with devices=[...] or a "
                             "torch.distributed group of several ranks")
        self._track_minimum = bool(on)
        if self._pair is not None:
            for c in self._pair:
                c.set_track_minimum(on)
        elif self._states is not None:
            self._apply_track_minimum()

    def _apply_track_minimum(self):
        if not hasattr(self._states, "set_track_best"):
            raise ValueError("this engine keeps no minimum records (set_track_best)")
        # the update points are the exchange rounds: a period no timestep reaches leaves the sweeps between them uncut
        self._states.set_track_best(TRACK_AT_ROUNDS if self._track_minimum else 0)

    def get_minimum(self):
        """(energies float64[G], states bool[G, N], timesteps uint64[G], rungs int64[G]) per SLOT: the lowest energy the slot's
        configuration had at an exchange round, that configuration, the timestep of that round, and the rung the slot holds now.
        copies=2: one leading row per copy."""
        if self._pair is not None:
            self._materialise()
            return tuple(np.stack(x) for x in zip(*(c.get_minimum() for c in self._pair)))
        self._materialise()
        if not self._track_minimum:
            raise ValueError("minimum tracking is off: call set_track_minimum(True) first")
        e, st, t, _ = self._states.best()
        rungs = np.empty(len(self._betas), dtype=np.int64)
        rungs[self.get_permutation()] = np.arange(len(self._betas))
        return e, st, t, rungs

    # -- thermal averages <s_i> at every rung, summed on the device ------------------------------------------------
    def _per_rung_states(self, what="spin sums per rung", needs="set_moments_every", keeps="spin sums"):
        """The container(s) that hold the sums (or the observable series) per rung, one per copy; ValueError where the ladder cannot
        have them."""
        if self._devices is not None:
            raise ValueError(what + " are for a ladder on one device: not with devices=[...] (a shard holds part of the ladder)")
        if self._world > 1:
            raise ValueError(what + " are for a ladder on one process: not inside a torch.distributed group of several ranks")
        self._materialise()
        copies = self._pair if self._pair is not None else [self]
        for c in copies:
            if not hasattr(c._states, needs):
                raise ValueError("this engine keeps no %s (%s)" % (keeps, needs))
            if not c._on_stream:
                raise ValueError(what + " need the ladder on the device's stream: this ladder takes the host swap step "
                                 "(ISINGMC_PT_HOST=1, or a container that pt_can_attach refuses)")
        return [c._states for c in copies]

    def set_measure_spins_every(self, k):
        """A sample of every rung follows each k-th timestep from now on (0: off, the sums stay): rung i adds the configuration that
        holds beta i at that moment, before any exchange round that follows the timestep.  Before or after the first timestep (the
        ladder is built here if it is not yet); no configuration, energy, random number or exchange decision changes."""
        if int(k) < 0:
            raise ValueError("k must not be negative")
        for st in self._per_rung_states():
            st.set_moments_every(int(k), per_rung=True)

    def get_measured_spins(self):
        """(n_samples, means float64[G, N]): the thermal average of every spin at every rung over the samples taken, True = +1, in
        the order of get_betas() (zeros before the first sample).  copies=2: float64[2, G, N], one leading row per copy."""
        out = []
        for st in self._per_rung_states():
            if not st.moments_per_rung:
                raise ValueError("no spin sums per rung are held: call set_measure_spins_every(k) first")
            n, site, _ = st.moments()
            out.append((n, site / float(max(n, 1))))
        if self._pair is None:
            return out[0]
        if out[0][0] != out[1][0]:   # (both copies stand at one timestep with one period)
            raise RuntimeError("the two copies of the ladder hold different numbers of samples")
        return out[0][0], np.stack([m for _, m in out])

    def reset_measured_spins(self):
        """Sums and sample count back to zero; the period stays."""
        for st in self._per_rung_states():
            st.reset_moments()

    # -- energy and magnetisation of every rung per sample, logged on the device --------------------------------------
    def _obs_states(self):
        return self._per_rung_states("observables per rung", "observable_series", "observable series")

    def set_measure_observables_every(self, k, classes=None, capacity=4096):
        """A row of the observable series follows each k-th timestep from now on (0: off, the rows stay): per rung the energy, the
        magnetisation and, with class tables (as site_classes takes them), the magnetisation by class of the configuration that
        holds that rung at that moment, before any exchange round that follows the timestep.  The period lives in the library, one
        series by rung per copy; a call with k > 0 starts a new log of `capacity` rows.  No configuration, energy, random number or
        exchange decision changes."""
        if int(k) < 0:
            raise ValueError("k must not be negative")
        if int(k) == 0:
            for series in self._obs_series or []:
                series.set_every(0)
            self._obs_every = 0
            return
        states = self._obs_states()
        for series in self._obs_series or []:
            series.close()   # (the old logs go, and their periods with them, before the new ones take the containers' periods)
        self._obs_series = None
        made = []
        for st in states:
            cls = classes if classes is None or isinstance(classes, _capi.SiteClasses) else _capi.SiteClasses(st.graph, classes)
            series = st.observable_series(classes=cls, by_rung=True, capacity=int(capacity))
            series.set_every(int(k))
            made.append(series)
        self._obs_series, self._obs_every, self._obs_t0 = made, int(k), self._t

    def _obs_room(self, T):
        """Before a call of T timesteps moves anything: ValueError when the rows of the call would not fit the logs.  (The library
        refuses each of its calls by the same count; a call of this class is several of them, on two copies.)"""
        if not self._obs_every or not self._obs_series:
            return
        k, since = self._obs_every, self._t - self._obs_t0
        samples = (since + int(T)) // k - since // k
        for series in self._obs_series:
            room = series.capacity - series.count
            if samples > room:
                raise ValueError("the observable series of this ladder would run full: the call takes %d samples and the log has room "
                                 "for %d of its %d rows (get_measured_observables, then reset_measured_observables; or switch the "
                                 "period off)" % (samples, room, series.capacity))

    def get_measured_observables(self):
        """(timesteps uint64[n], energy float64[n, G], magnetisation int64[n, G], by_class int64[n, G, T, K] or None), the columns
        in the order of get_betas().  copies=2: the three arrays get a leading axis of 2, one entry per copy.  One wait per copy."""
        if not self._obs_series:
            raise ValueError("no observables are logged: call set_measure_observables_every(k) first")
        out = [series.get() for series in self._obs_series]
        if self._pair is None:
            return out[0]
        if not np.array_equal(out[0][0], out[1][0]):   # (both copies stand at one timestep with one period)
            raise RuntimeError("the two copies of the ladder hold rows of different timesteps")
        return (out[0][0],) + tuple(None if a is None else np.stack([a, b]) for a, b in zip(out[0][1:], out[1][1:]))

    def reset_measured_observables(self):
        """The row count back to zero; the period stays."""
        if not self._obs_series:
            raise ValueError("no observables are logged: call set_measure_observables_every(k) first")
        for series in self._obs_series:
            series.reset()

    # -- what choosing the ladder needs: pair acceptance, replica flow, energy sums, kept by the exchange rounds ------
    def set_ladder_statistics(self, on=True):
        """From now on every exchange round counts (on=False: stops, the values stay): per pair of neighbouring rungs the attempts
        and accepted exchanges, per rung the energy sums of the configuration that was swept at it and how often the configuration
        it holds last visited rung 0 (up) or the last rung (down), per slot the completed round trips rung 0 -> last rung -> rung 0.
        Before or after the first timestep.  On the device's stream the exchange kernels keep them (rounds inside a persistent
        launch included: nothing waits on the host); on the host swap path this class keeps the same numbers through the
        library's host twin; with devices=[...] and in a torch.distributed group every shard holds the whole ladder's, identical.
        No configuration, energy, random number or exchange decision changes."""
        if self._pair is not None:
            for c in self._pair:
                c.set_ladder_statistics(on)
            return
        self._stats_on = bool(on)
        self._stats_seen = self._stats_seen or self._stats_on
        if self._states is not None:
            self._lads[0].set_statistics(self._stats_on)

    def _statistics_ladder(self):
        if not self._stats_seen:
            raise ValueError("this ladder holds no statistics: call set_ladder_statistics() first")
        self._materialise()
        return self._lads[0]

    def get_ladder_statistics(self):
        """dict: rounds, in_kernel_rounds (of them, decided inside persistent launches); attempts, accepts uint64[G - 1] and
        acceptance float64[G - 1] = accepts / attempts per pair (i, i + 1), NaN where a pair has no attempt; n_up, n_down uint64[G] and
        flow float64[G] = n_up / (n_up + n_down), NaN where a rung has no labelled visit; mean_energy, var_energy float64[G] from
        the energy sums over the rounds (NaN before the first round) -- all in the order of get_betas(); round_trips uint64[G] and
        labels uint8[G] (0 none, 1 up, 2 down) per replica SLOT, slot s being the configuration that started at rung s (where it is
        now: get_permutation()).  copies=2: every entry has a leading axis of 2, one row per copy."""
        if self._pair is not None:
            both = [c.get_ladder_statistics() for c in self._pair]
            return {k: np.stack([np.asarray(d[k]) for d in both]) for k in both[0]}
        raw = self._statistics_ladder().raw_statistics()
        out = {k: raw[k] for k in ("rounds", "in_kernel_rounds", "attempts", "accepts")}
        with np.errstate(divide="ignore", invalid="ignore"):
            out["acceptance"] = np.where(raw["attempts"] > 0, raw["accepts"] / raw["attempts"].astype(np.float64), np.nan)
            visits = (raw["n_up"] + raw["n_down"]).astype(np.float64)
            out["n_up"], out["n_down"] = raw["n_up"], raw["n_down"]
            out["flow"] = np.where(visits > 0, raw["n_up"] / visits, np.nan)
            rounds = float(raw["rounds"]) if raw["rounds"] else np.nan
            out["mean_energy"] = raw["sum_e"] / rounds
            out["var_energy"] = raw["sum_e2"] / rounds - out["mean_energy"] ** 2
        out["round_trips"], out["labels"] = raw["round_trips"], raw["labels"]
        return out

    def reset_ladder_statistics(self):
        """Every count and sum back to zero, the labels to none; the setting stays."""
        if self._pair is not None:
            for c in self._pair:
                c.reset_ladder_statistics()
            return
        self._statistics_ladder().reset_statistics()

    # -- building the ladder: which of the three kinds it is gets decided here, once ----------------------------------------------
    def _materialise(self):
        if self._states is not None:
            return
        G = len(self._betas)
        if G == 0:
            raise ValueError("no graphs: call add_graph(beta) first")
        if self._pair is not None:
            return self._materialise_pair()
        self._perm = np.arange(G, dtype=np.uint32)
        if self._devices is not None:
            self._lads = [_GroupLadder(self, G)]
        else:
            self._per = D.block_size(G, self._world)
            self._lo, self._hi = D.shard_bounds(G, self._world, self._rank)
            self._engine = self._engine_factory()
            self._states = self._engine.make_states(np.array(self._slot_seeds, dtype=np.uint64), (self._lo, self._hi))
            if self._rng_rounds is not None and self._world == 1:
                if not hasattr(self._states, "set_option"):
                    raise ValueError("this engine's containers have no option 'philox_rounds' (rng_rounds)")
                self._states.set_option("philox_rounds", self._rng_rounds)
            self._on_stream = (bool(getattr(self._engine, "supports_on_stream_pt", False)) and self._hi > self._lo and
                               os.environ.get("ISINGMC_PT_HOST", "0") in ("", "0"))  # ISINGMC_PT_HOST=1: the host swap step (A/B runs)
            # eligibility first, WITHOUT side effects (e.g. a real-coupling graph too small for the packed kernels, a bit-sliced shard
            # that cuts a replica group: the host swap step serves those) ...
            if self._on_stream:
                self._on_stream = self._states.pt_can_attach(G, self._lo, self._per, self._world)
            if self._world > 1:  # ... then every rank must take the same path (the collective differs) ...
                flags = D.all_gather_f64(np.array([float(self._on_stream)]), 1, self._group)  # (a rank without slots has no buffers to gather into: host path for all)
                self._on_stream = bool(flags.min() > 0)
            self._lads = [_StreamLadder(self) if self._on_stream else _HostLadder(self)]   # ... and only then does anyone attach
            if self._track_minimum:
                self._apply_track_minimum()
        if self._stats_seen:   # (set_ladder_statistics(True) has been called at least once: the statistics exist from here on)
            self._lads[0].set_statistics(self._stats_on)

    def _materialise_pair(self):
        """copies=2: two copies=1 ladders on one engine; the loops below walk both and add the cuts at cluster moves and samples."""
        a, b = self._pair
        a._materialise()
        b._materialise()
        if a._on_stream != b._on_stream:   # (one graph, one geometry: cannot differ)
            raise RuntimeError("the two copies of the ladder took different exchange paths")
        if self._icm_every and not hasattr(a._states, "icm_between"):
            raise ValueError("this engine has no isoenergetic cluster move between containers (icm_between)")
        self._states, self._on_stream, self._lads = a._states, a._on_stream, a._lads + b._lads
        self._lo, self._hi = a._lo, a._hi
        self._icm_pending = False

    def group_backend(self):
        """'rccl' or 'copy' for an in-process ladder (devices=[...]), else None."""
        self._materialise()
        return self._lads[0].backend

    def _swap_step(self):
        """One exchange round of a copies=1 ladder that has been built."""
        self._lads[0].exchange()

    def _pair_icm(self):
        """Timestep self._t of both copies as a cluster move between the configurations at equal rungs."""
        a, b = self._pair
        if self._on_stream:
            a._states.icm_between(b._states)   # the rung permutations are read on the device
        else:
            a._states.icm_between(b._states, a._perm, b._perm)
        self._icm_stats, self._icm_pending = None, True

    # -- the two loops: both walk schedule(), which holds the order "timestep, overlap sample, exchange round, state sample" ----------
    def timesteps(self, t, replica_swap_freq=None):
        """tempering.rs:150-152 (parallel_timesteps): t sweeps on every rung.  replica_swap_freq (extension):
        an exchange round after every `replica_swap_freq` sweeps, as in the loop of tempering.rs:177-194."""
        if self._pair is None or t > 0:   # (a call without timesteps does not build a copies=2 ladder)
            self._materialise()
        if t <= 0:
            return
        self._obs_room(t)
        t, f, lads = int(t), int(replica_swap_freq or 0), self._lads
        if not f and self._pair is None:
            self._t += t
            return lads[0].plain(t)
        # a copies=1 ladder hands the library whole calls where it can, a pair whole rounds: its copies meet at moves and samples
        fuse = lads[0].fuse if self._pair is None else min(lads[0].fuse, FUSE_ROUNDS)
        for n, kind, overlap_due, round_due, _ in schedule(self._t, t, f, self._icm_every, self._ovl_every, self._ovl_t0, 0, fuse):
            for lad in lads:
                if kind == FUSED:
                    lad.run(n, f)
                elif kind == SWEEPS:
                    lad.sweep(n)
            if kind == MOVE:
                self._pair_icm()
            self._t += n
            if overlap_due:
                self._pair_sample()
            if round_due:
                for lad in lads:
                    lad.exchange()
        for lad in lads:
            lad.synchronize()

    def timesteps_sample(self, timesteps, replica_swap_freq=None, sampling_freq=None):
        """tempering.rs:156-222: countdown scheduler of run / swap / sample.

        Returns (states, energies[, rungs]): energies float64[G] = time average per rung (identical on
        every rank).  Single process: states bool[G, S, N] indexed by rung.  Sharded: states
        bool[G_local, S, N] of this rank's slots plus rungs int[G_local, S] = the rung each local slot
        held at each sample (configurations never leave their GPU).  copies=2: states bool[2, G, S, N] by rung and
        energies float64[2, G], one row per copy.
        """
        self._materialise()
        self._obs_room(timesteps)
        f, sampling_freq = _frequencies(replica_swap_freq, sampling_freq)
        lads, G, S = self._lads, len(self._betas), timesteps // sampling_freq
        perms = [lad.perm() for lad in lads]   # (on the device's stream the device owns the ladder state)
        states = np.zeros((len(lads), self._hi - self._lo, S, self.nvars), dtype=np.bool_)   # by slot first
        rungs = np.zeros(states.shape[:3], dtype=np.int64)
        energy_acc = np.zeros((len(lads), G), dtype=np.float64)
        k = 0
        for n, kind, _, round_due, sample_due in schedule(self._t, timesteps, f, self._icm_every, sample=sampling_freq):
            if kind == MOVE:
                self._pair_icm()
            for i, lad in enumerate(lads):
                # energy_acc[rung] += te * t (tempering.rs:185), te = mean energy over the block; the energy after a move counts as
                # that timestep's energy
                energy_acc[i] += (lad.st.energies() if kind == MOVE else lad.slot_sums(n))[perms[i]]
            self._t += n
            if round_due:
                for i, lad in enumerate(lads):
                    lad.exchange()
                    perms[i] = lad.perm()
            if sample_due:
                if k < S:
                    for i, lad in enumerate(lads):
                        lad.read_states(states[i, :, k, :])
                        rungs[i, :, k] = _inverse(perms[i])[self._lo:self._hi]
                k += 1
        energies = energy_acc / max(timesteps, 1)
        if self._world > 1:
            return states[0], energies[0], rungs[0]
        by_rung = _by_rung(states, rungs)
        return (by_rung, energies) if self._pair is not None else (by_rung[0], energies[0])

"""Cost of the spin sums per rung of a tempering ladder, HIP events on the container's stream:
  1. one per-rung sample in units of one sweep of the same container, beside one per-replica sample of a plain container of the
     same shape and betas (the two alternate, best and median of five), at 1024^2 +-J x 64 rungs (checkerboard) and 64^3 +-J x 64
     rungs (bit-sliced);
  2. pt_run(200, 10) with the sums switched on (a sample every 10th timestep) relative to off, alternating on the same container,
     at those shapes and at 1024^2 x 256 and 64^3 x 1024.
Output kept in profiles/2026-10-20_ladder_moments.txt."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from oracle import exact as X  # noqa: E402
from pyisingmontecarlo_amd import _capi as capi  # noqa: E402


def say(*a):
    print(" ".join(str(x) for x in a), flush=True)


def timed(st, fn):
    """milliseconds of what fn enqueues on the container's stream, between two events"""
    stream = st.pt_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.synchronize()
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(xs):
    return f"{min(xs) * 1e3:.1f} us (median {float(np.median(xs)) * 1e3:.1f})"


def ladder(g, betas, seed=7):
    st = capi.States(g, capi.make_seeds(1, len(betas)))
    st.pt_attach(betas, 0, len(betas), 1, seed)
    return st


def sample_cost(name, g, betas):
    G, K = len(betas), 8
    st = ladder(g, betas)
    plain = capi.States(g, capi.make_seeds(1, G))
    plain.set_betas(betas)
    say(f"== {name} x {G} rungs: family {st.family}")
    st.pt_run(40, 2)   # a permutation to route by
    perm, _, swaps = st.pt_state()
    moved = int((perm != np.arange(G)).sum())
    mixed = int((perm[:32] >= 32).sum()) if G > 32 else 0
    say(f"after pt_run(40, 2): {swaps} swaps, {moved} of {G} rungs off their first slot, {mixed} rungs of the first 32 held by slots >= 32")
    sweep = min(timed(st, lambda: st.pt_time_steps(50)) for _ in range(5)) / 50
    say(f"sweep {sweep * 1e3:.1f} us")
    st.set_moments_every(1 << 40, per_rung=True)
    plain.set_moments_every(1 << 40, per_replica=True)
    n = 2 * ((1 << K) - 1)   # two flushes included
    rung, replica = [], []
    for c in (st, plain):
        for _ in range((1 << K) - 1):
            c.accumulate_moments()
    for _ in range(5):
        rung.append(timed(st, lambda: [st.accumulate_moments() for _ in range(n)]) / n)
        replica.append(timed(plain, lambda: [plain.accumulate_moments() for _ in range(n)]) / n)
    say(f"per rung    K={K}: {stats(rung)} per sample (flushes included, {n} samples) = {min(rung) / sweep:.2f} sweeps")
    say(f"per replica K={K}: {stats(replica)} per sample (plain container, same betas)     = {min(replica) / sweep:.2f} sweeps")
    say(f"per rung / per replica = {min(rung) / min(replica):.2f}")


def run_cost(name, g, betas, T=200, f=10):
    st = ladder(g, betas)
    say(f"== {name} x {len(betas)} rungs: family {st.family}, pt_run({T}, {f})")
    st.pt_run(T, f)
    on, off = [], []
    for _ in range(5):
        st.set_moments_every(0)
        off.append(timed(st, lambda: st.pt_run(T, f)))
        st.set_moments_every(f, per_rung=True)
        on.append(timed(st, lambda: st.pt_run(T, f)))
    say(f"off {min(off):.3f} ms (median {float(np.median(off)):.3f}), on {min(on):.3f} ms (median {float(np.median(on)):.3f}): "
        f"on / off = {min(on) / min(off):.3f}, {T // f} samples, {st.moments()[0]} in the sums")


with open(capi.lib()._name, "rb") as fh:
    say("# libisingmc.so sha256", hashlib.sha256(fh.read()).hexdigest())
lat = capi.Graph(*X.square_lattice_edges(1024, 1024, -1.0, np.random.default_rng(3)))
lat_betas = lambda G: 0.4400 + 0.0003 * np.arange(G) / G   # noqa: E731
sample_cost("1024^2 +-J lattice", lat, lat_betas(64))
run_cost("1024^2 +-J lattice", lat, lat_betas(64))
run_cost("1024^2 +-J lattice", lat, lat_betas(256))
os.environ["ISINGMC_FORCE_PACKED"] = "1"
ea, eb, _ = X.cubic_lattice_edges(64, -1.0)
ej = np.random.default_rng(4).choice([-1.0, 1.0], len(ea))
cub = capi.Graph(ea, eb, ej, nvars=64 ** 3, force_general=True)
cub_betas = lambda G: 0.9 + 0.0005 * np.arange(G)   # noqa: E731
sample_cost("64^3 +-J cubic", cub, cub_betas(64))
run_cost("64^3 +-J cubic", cub, cub_betas(64))
run_cost("64^3 +-J cubic", cub, cub_betas(1024))
say("done")

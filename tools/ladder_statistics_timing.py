"""Cost of the ladder statistics, HIP events on the container's stream:
  1. pt_run(200, 10) at 1024^2 x 64 rungs (the persistent strip launch with 19 of its 20 rounds inside it), statistics off and on,
     alternating on the same container, best and median of five;
  2. pt_run(200, 1) at 4^3 +-J x 33 rungs on the bit-sliced packed family (one launch per round), off and on.
--parent: the library named by ISINGMC_LIB_PATH is the parent commit's (no statistics entry points): the off figure alone, for the
comparison of the two binaries (run the two alternately, one process each).
Output kept in profiles/2026-10-20_ladder_statistics.txt."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from oracle import exact as X  # noqa: E402
from pyisingmontecarlo_amd import _capi as capi  # noqa: E402

PARENT = "--parent" in sys.argv
if PARENT:
    for name in [n for n in capi._PROTOTYPES if "statistics" in n]:
        del capi._PROTOTYPES[name]


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


def fmt(xs):
    return f"{min(xs):.3f} ms (median {float(np.median(xs)):.3f})"


def run_cost(name, g, betas, T, f):
    st = capi.States(g, capi.make_seeds(1, len(betas)))
    st.pt_attach(betas, 0, len(betas), 1, 7)
    say(f"== {name} x {len(betas)} rungs: family {st.family}, pt_run({T}, {f})")
    st.pt_run(T, f)
    on, off = [], []
    for _ in range(5):
        if not PARENT:
            st.pt_set_statistics(False)
        off.append(timed(st, lambda: st.pt_run(T, f)))
        if not PARENT:
            st.pt_set_statistics(True)
            on.append(timed(st, lambda: st.pt_run(T, f)))
    if PARENT:
        say(f"parent {fmt(off)}")
        return
    s = st.pt_statistics()
    say(f"off {fmt(off)}, on {fmt(on)}: on / off = {min(on) / min(off):.3f}; {s['rounds']} rounds counted, "
        f"{s['in_kernel_rounds']} of them inside persistent launches, {int(s['accepts'].sum())} accepted of {int(s['attempts'].sum())}")


with open(capi.lib()._name, "rb") as fh:
    say("# libisingmc.so sha256", hashlib.sha256(fh.read()).hexdigest(), "(parent)" if PARENT else "")
lat = capi.Graph(*X.square_lattice_edges(1024, 1024, -1.0))
run_cost("1024^2 lattice", lat, 0.4400 + 0.0003 * np.arange(64) / 64, 200, 10)
os.environ["ISINGMC_FORCE_PACKED"] = "1"
ea, eb, _ = X.cubic_lattice_edges(4, -1.0)
ej = np.random.default_rng(4).choice([-1.0, 1.0], len(ea))
cub = capi.Graph(ea, eb, ej, nvars=64, force_general=True)
run_cost("4^3 +-J cubic", cub, 0.30 + 0.02 * np.arange(33), 200, 1)
say("done")

#!/usr/bin/env python3
"""A fixed list of short calls that between them take every path of the step loop and every outcome of its launch rules
(csrc/step_policy.hpp) that default options reach.  Results do not depend on the path, so what a change of the policy changes is the
list of kernel dispatches: run this under a kernel trace (rocprofv3 --kernel-trace -- python tools/step_policy_cases.py) once per
library (ISINGMC_LIB_PATH selects one) and compare name, grid, workgroup size and LDS bytes of the two lists.

Two rules are not reachable at default options and are forced, as the lines say: the CSR kernels at 64 replicas of a 200 x 200
lattice (the bit-sliced family takes that container), and the streaming sweep of a lattice the strip kernel serves."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import exact as X  # noqa: E402
from pyisingmontecarlo_amd import _capi  # noqa: E402

BETA = 0.44


def states(edges, R, **graph_args):
    g = _capi.Graph(*edges, **graph_args)
    return g, _capi.States(g, _capi.make_seeds(7, R))


def run(name, edges, R, timesteps, per_step=False, energies=False, **graph_args):
    g, st = states(edges, R, **graph_args)
    st.do_time_steps(timesteps, BETA, per_step_energies=per_step)
    if energies:
        st.energies()
    print(f"{name}: family {st.family}, {R} replicas, {timesteps} timesteps", flush=True)
    del st, g


def main():
    lat = X.square_lattice_edges
    run("64x4 (resident, spread form)", lat(64, 4), 8, 3)
    run("512x512 (resident, one lane per quad)", lat(512, 512), 8, 3)
    run("1024x192 (768 quads: resident)", lat(1024, 192), 8, 3)
    run("1024x1024 (strips)", lat(1024, 1024), 8, 3)
    g, st = states(lat(1024, 192), 8)
    st.pt_attach(np.linspace(0.40, 0.47, 8), 0, 8, 1, 11)
    st.pt_run(26, 4)
    st.synchronize()
    print("1024x192 ladder of 8: pt_run(26, 4), rounds inside the strip launch", flush=True)
    del st, g
    run("256x1028 (streaming, two lanes)", lat(256, 1028), 8, 64)
    run("256x1028 (streaming, energies per step)", lat(256, 1028), 8, 64, per_step=True)
    run("1024x1024 x 64", lat(1024, 1024), 64, 4)
    run("1024x1024 x 256 (looping sweep, two quads)", lat(1024, 1024), 256, 2)
    run("2048x2048 x 256 (looping sweep, whole rounds)", lat(2048, 2048), 256, 2)
    run("256x16 with a field (multi-class, resident)", lat(256, 16), 8, 3, biases=np.full(256 * 16, 0.5))
    run("1024x1024 with a field (multi-class, streaming)", lat(1024, 1024), 8, 8, biases=np.full(1024 * 1024, 0.5))
    run("16x16 torus, general path (resident CSR, staged)", lat(16, 16), 4, 3, force_general=True)
    run("200x200 general path x 13 (CSR, one replica per thread)", lat(200, 200), 13, 2, force_general=True)
    os.environ["ISINGMC_DISABLE_PACKED"] = "1"   # read when the container is created
    run("200x200 general path x 64, bit-sliced family disabled (CSR, two replicas per thread)", lat(200, 200), 64, 2, force_general=True)
    del os.environ["ISINGMC_DISABLE_PACKED"]
    ea, eb, _ = X.cubic_lattice_edges(16)
    run("16^3 +-J glass x 1024 (bit-sliced)", (ea, eb, np.random.default_rng(3).choice([-1.0, 1.0], len(ea))), 1024, 4, energies=True)
    ea, eb, _ = X.cubic_lattice_edges(24)
    run("24^3 Gaussian glass x 64 (real couplings)", (ea, eb, np.random.default_rng(4).standard_normal(len(ea))), 64, 4, energies=True)
    os.environ["ISINGMC_STRIP"] = "0"
    run("1024x1024, strips off (streaming, one lane)", lat(1024, 1024), 8, 3)
    del os.environ["ISINGMC_STRIP"]
    print("done", flush=True)


if __name__ == "__main__":
    main()

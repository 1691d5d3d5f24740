"""Cost of one lag-ring sample in sweeps of the same container, next to get_states() + numpy for the same integers,
and the step loop with the feature off.  Medians of five, HIP events on the container's stream.

  python tools/autocorrelation_timing.py [--quick]      the cost of a sample
  python tools/autocorrelation_timing.py --off          the feature-off figures alone: run it in alternating processes with
                                                        ISINGMC_LIB_PATH pointing at this binary and at the parent commit's

Shapes: 1024^2 x 256 (checkerboard) and 64^3 +-J x 1024 (replica-packed bit-sliced), L = 8 and L = 32; feature off: do_time_steps at
the shape of bench.py (4096^2 x 256) and pt_run(200, 10) at 1024^2 x 64 rungs.  Prints one line per figure."""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import exact as X  # noqa: E402
from pyisingmontecarlo_amd import _capi  # noqa: E402


class Events:
    """a pair of HIP events on a container's stream"""

    def __init__(self, st):
        self.hip = C.CDLL(None)   # the runtime the library itself runs on, where it is among the process's global symbols
        if not hasattr(self.hip, "hipEventCreate"):
            self.hip = C.CDLL("libamdhip64.so")
        self.stream = C.c_void_p()
        _capi._check(_capi.lib().isingmc_states_stream(st._h, C.byref(self.stream)))
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        assert self.hip.hipEventCreate(C.byref(self.e0)) == 0 and self.hip.hipEventCreate(C.byref(self.e1)) == 0

    def time_ms(self, body):
        assert self.hip.hipEventRecord(self.e0, self.stream) == 0
        body()
        assert self.hip.hipEventRecord(self.e1, self.stream) == 0
        assert self.hip.hipEventSynchronize(self.e1) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.e0, self.e1) == 0
        return ms.value


def median5(f):
    return statistics.median(f() for _ in range(5))


def sample_cost(name, st, beta, lags, sweeps):
    N, R = st.graph.nvars, st.count
    st.do_time_steps(20, beta)
    sweep_ms = median5(lambda: st.do_time_steps_timed(sweeps, beta)) / sweeps
    state_bytes = st.raw_state().nbytes
    print(f"{name}: sweep {sweep_ms:.4f} ms, state {state_bytes / 2 ** 20:.1f} MiB")
    ev = Events(st)
    for L in lags:
        ac = st.autocorrelation(L)
        for _ in range(L + 2):   # fill the ring: every lag live
            st.do_time_steps(1, beta)
            ac.sample()
        st.synchronize()

        def one():
            st.do_time_steps(1, beta)
            st.synchronize()
            return ev.time_ms(ac.sample)
        ms = median5(one)
        gbs = (L + 2) * state_bytes / ms / 1e6
        print(f"{name}: L = {L}: sample {ms:.4f} ms = {ms / sweep_ms:.1f} sweeps; (L + 2) state passes at {gbs:.0f} GB/s")
        ac.close()
    # the same integers through get_states() + numpy: one configuration out, one comparison per lag on the host
    L = lags[0]
    prev = [st.states() for _ in range(L)]

    def host():
        t0 = time.perf_counter()
        cur = st.states()
        for p in prev:
            (cur != p).sum(axis=1)
        return (time.perf_counter() - t0) * 1e3
    ms = median5(host)
    print(f"{name}: get_states() + numpy against L = {L} stored samples {ms:.1f} ms = {ms / sweep_ms:.0f} sweeps ({N * R / 1e6:.0f} M spins)")


def feature_off():
    """what the parent commit's binary runs too: ISINGMC_LIB_PATH selects the binary, one process per measurement"""
    g = _capi.Graph(*X.square_lattice_edges(4096, 4096, -1.0))
    st = _capi.States(g, _capi.make_seeds(1, 256))
    st.do_time_steps(20, 0.4407)
    print(f"feature off: do_time_steps 4096^2 x 256: {median5(lambda: st.do_time_steps_timed(100, 0.4407)) / 100:.4f} ms per sweep")
    st.close()
    g = _capi.Graph(*X.square_lattice_edges(1024, 1024, -1.0))
    st = _capi.States(g, _capi.make_seeds(2, 64))
    st.pt_attach(np.linspace(0.40, 0.48, 64), 0, 64, 1, 7)
    st.pt_run(200, 10)
    st.synchronize()
    ev = Events(st)
    print(f"feature off: pt_run(200, 10) 1024^2 x 64 rungs: {median5(lambda: ev.time_ms(lambda: st.pt_run(200, 10))):.3f} ms")


def main():
    quick = "--quick" in sys.argv
    if "--off" in sys.argv:
        return feature_off()
    g = _capi.Graph(*X.square_lattice_edges(1024, 1024, -1.0))
    sample_cost("1024^2 x 256", _capi.States(g, _capi.make_seeds(3, 256)), 0.4407, (8,) if quick else (8, 32), 50)
    os.environ["ISINGMC_FORCE_PACKED"] = "1"
    ea, eb, _ = X.cubic_lattice_edges(64, -1.0)
    ej = np.random.default_rng(4).choice([-1.0, 1.0], len(ea))
    g = _capi.Graph(ea, eb, ej, nvars=64 ** 3, force_general=True)
    sample_cost("64^3 +-J x 1024", _capi.States(g, _capi.make_seeds(5, 1024)), 0.9, (8,) if quick else (8, 32), 20)


if __name__ == "__main__":
    main()

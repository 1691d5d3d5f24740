"""Population annealing at the populations where its kernels take their second branch: more than one scan block
(R >= 1025), the high words of the 128-bit compare (R S >= 2^64: R >= 65 536), the second launch of the row gather (R > 32 768),
the carry loop of the scan's second pass and the second launch of the bit gather (R > 2^20).

No per-replica restatement is affordable here.  Every step is checked against the vectorised restatement of
tests/pa_reference.py (sources_fast, bit_gather_fast; tests/test_pa_host.py holds them equal to the definitions): the source
table and the step record exactly, the raw device words after the gather word for word, the energies and the family table; on
the checkerboard family a sample of slots is then swept once more on the device and with the oracle from the gathered rows, which
shows that the Philox keys stayed with the slots.  Which branch a case reaches is asserted on the RESTATEMENT's figures
(needs_high_words, low_word_carries) before the device is asked."""
import time

import numpy as np
import pytest

import icm_reference as ICM
import pa_reference as PA
import packed_icm_reference as IR

pytestmark = pytest.mark.gpu

SEED = 0x0123456789ABCDEF
BETA = 0.3
ROWS_PER_LAUNCH = 32768            # grid.y of one gather launch (rows of a board, groups of a packed container)
MILLION = (1 << 20) + 1025         # 1026 scan blocks (a second chunk of pass 2); 32 801 groups, the last owning ONE bit


class _Pop:
    """A container of one family and what the checks need of its layout; the time spent is booked to 'device' (library calls,
    copies to the host included) or 'numpy' (the restatement and the comparisons)."""

    def __init__(self, capi, exact, monkeypatch, kind, R, same_start=False, seed_gen=21):
        self.kind, self.R = kind, R
        self.clock = {"device": 0.0, "numpy": 0.0}
        self.seeds = capi.make_seeds(seed_gen, R)
        if kind[0] == "board":
            W, H = 64, 4
            ea, eb, ej = exact.square_lattice_edges(W, H, -1.0, np.random.default_rng(W + H) if kind[1] else None)
            self.lat = ICM.make_lat(W, H, *ICM.couplings(W, H, ej))
            self.g = capi.Graph(ea, eb, ej, device=0)
            nvars, family = W * H, "checkerboard"
        else:
            monkeypatch.setenv("ISINGMC_FORCE_PACKED", "1")
            if kind[0] == "cubic":
                ea, eb, ej = IR.cubic_glass(exact, 6)
                G = IR.Graph(ea, eb, ej, 216)
                self.g = capi.Graph(G.ea, G.eb, G.ej, nvars=G.nvars, force_general=True)
                family = "packed_bitsliced"
            else:
                ea, eb, _ = exact.square_lattice_edges(64, 8, -1.0)
                rng = np.random.default_rng(648)
                G = IR.Graph(ea, eb, rng.normal(size=len(ea)), 512)
                self.g = capi.Graph(G.ea, G.eb, G.ej, nvars=G.nvars, biases=rng.normal(size=512), stable_path=True)
                family = "packed_real"
            self.n_pos = G.n_pos
            self.padding = np.ones(G.n_pos, dtype=bool)
            self.padding[G.pos] = False
            nvars = G.nvars
        start = np.random.default_rng(5).integers(0, 2, nvars).astype(np.uint8) if same_start else None
        self.st = self.device(capi.States, self.g, self.seeds, initial_state=start)
        assert self.st.family == family and self.st.count == R

    def device(self, fn, *args, **kw):
        t0 = time.perf_counter()
        out = fn(*args, **kw)
        self.clock["device"] += time.perf_counter() - t0
        return out

    def numpy(self, fn, *args, **kw):
        t0 = time.perf_counter()
        out = fn(*args, **kw)
        self.clock["numpy"] += time.perf_counter() - t0
        return out

    def raw(self):
        words = self.device(self.st.raw_state)
        if self.kind[0] == "board":
            return words.reshape(self.R, -1)
        words = words.reshape(-1, self.n_pos)
        assert words.shape[0] == (self.R + 31) // 32
        return words

    def gathered(self, raw, src):
        if np.array_equal(src, np.arange(self.R)):
            return raw   # (test_pa_host.py: both gathers of the restatement leave the words as they are under the identity)
        if self.kind[0] == "board":
            return PA.row_gather(raw, src)
        return PA.bit_gather_fast(raw, src, self.padding)

    def report(self, name):
        print(f"{name}: device {self.clock['device']:.2f} s, numpy {self.clock['numpy']:.2f} s")


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        pytest.fail(f"{what}: {len(bad)} of {got.size} differ, the first at {bad[0].tolist()}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}")


def _resample(P, dbeta, step, fam):
    """One pa_resample against sources_fast fed with the energies the library returned just before it."""
    st, R = P.st, P.R
    e, raw, t = P.device(st.energies), P.raw(), st.timestep
    want = P.numpy(PA.sources_fast, SEED, step, e, dbeta)
    print(f"R {R} dbeta {dbeta} step {step}: S / (R 2^32) = {want['sum'] / (R << 32):.5f}, distinct {want['distinct']}, "
          f"high words {want['needs_high_words']}, low-word carries {want['low_word_carries']}")
    P.device(st.pa_resample, dbeta, SEED, step)
    got = P.device(st.pa_last)
    _same(got["src"], want["src"], "source table")
    assert got["sum"] == want["sum"] and got["eref"] == want["eref"] and got["distinct"] == want["distinct"]
    assert want["eref"] == (e.min() if dbeta >= 0 else e.max())
    bound = R * 2.0 ** -52 * np.abs(e).mean()   # the worst case of any summation order
    print(f"mean energy {got['mean_energy']!r} numpy {want['mean_energy']!r} bound {bound:.3e}")
    assert abs(got["mean_energy"] - want["mean_energy"]) <= bound
    src = want["src"]
    expect = P.numpy(P.gathered, raw, src)
    after = P.raw()
    P.numpy(_same, after, expect, "raw words after the gather")
    _same(P.device(st.energies), e[src], "energies after the gather")
    fam = fam[src]
    _same(P.device(st.pa_families), fam, "families")
    assert st.timestep == t
    return want, fam


def _apply(P, src, fam):
    """pa_apply_sources with a caller's table: the words, the energies and the families."""
    st = P.st
    e, raw, t = P.device(st.energies), P.raw(), st.timestep
    P.device(st.pa_apply_sources, src)
    expect = P.numpy(P.gathered, raw, src)
    after = P.raw()
    P.numpy(_same, after, expect, "raw words after the caller's table")
    _same(P.device(st.energies), e[src], "energies after the caller's table")
    fam = fam[src]
    _same(P.device(st.pa_families), fam, "families")
    assert st.timestep == t
    return fam


def _sample_slots(R):
    """At least 16 slots spread over the table: 0, R - 1, both sides of every launch boundary of the row gather."""
    edges = [k for b in range(ROWS_PER_LAUNCH, R, ROWS_PER_LAUNCH) for k in (b - 1, b)]
    spread = np.linspace(0, R - 1, 16).astype(np.int64).tolist()
    return sorted(set([0, R - 1] + edges + spread))


def _slots_follow_their_seeds(P, beta):
    """One more timestep on the device and with the oracle from the gathered rows, the slot's own seed, the container's timestep."""
    assert P.kind[0] == "board"
    slots = _sample_slots(P.R)
    t = P.st.timestep
    before = P.device(P.st.packed)[slots]
    P.device(P.st.do_time_steps, 1, beta)
    after = P.device(P.st.packed)[slots]
    for k, slot in enumerate(slots):
        row = before[k].copy()
        P.lat.sweep(row, P.seeds[slot], t, beta)
        assert np.array_equal(after[k], row), f"slot {slot} of {P.R}"
    assert P.st.timestep == t + 1


FAMILIES = {"board-glass": ("board", True), "board-uniform": ("board", False), "cubic": ("cubic",), "real": ("real",)}


@pytest.mark.parametrize("R", [1025, 2048, 3000])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_more_than_one_scan_block(capi, exact, oracle, monkeypatch, family, R):
    """Passes 1 and 3 of the scan beyond the first block (a non-zero offset), the weights loop with a second and third element
    per thread (R = 3000: some threads with two, some with three)."""
    P = _Pop(capi, exact, monkeypatch, FAMILIES[family], R)
    fam = np.arange(R, dtype=np.uint32)
    P.st.do_time_steps(3, BETA)
    want, fam = _resample(P, 0.05, 1, fam)
    assert want["distinct"] < R   # (S itself is read from C[R - 1], an element of the scan's last block)
    P.st.do_time_steps(2, BETA + 0.05)
    _, fam = _resample(P, 0.05, 2, fam)   # the buffers have swapped once already
    if family.startswith("board"):
        _slots_follow_their_seeds(P, BETA + 0.1)


@pytest.mark.parametrize("R", [65535, 65536])
def test_equal_energies_at_the_threshold_of_the_high_words(capi, exact, oracle, monkeypatch, R):
    """R replicas of one configuration: S = R 2^32, so R S < 2^64 at R = 65 535 and R S = 2^64 at R = 65 536 -- the smallest
    population whose compare needs its high words.  The table is the identity."""
    P = _Pop(capi, exact, monkeypatch, ("board", True), R, same_start=True)
    fam = np.arange(R, dtype=np.uint32)
    before = P.raw()
    want, fam = _resample(P, 0.7, 1, fam)
    assert want["needs_high_words"] == (R == 65536)
    assert np.array_equal(want["src"], np.arange(R)) and want["sum"] == R << 32 and want["distinct"] == R
    _same(P.raw(), before, "raw words")
    _slots_follow_their_seeds(P, BETA)


@pytest.mark.parametrize("family", ["board-glass", "real"])
def test_second_launch_of_the_row_gather(capi, exact, oracle, monkeypatch, family):
    """R = 65 536 + 37: three launches of the row gather (r0 = 32 768 and 65 536, the last with 37 rows), 65 scan blocks, a
    weights loop of 64 or 65 elements per thread; cooling on one container and heating on its twin.  (With the energies two
    sweeps leave, S / (R 2^32) is far below (65 536 / R)^2 = 0.9989: the restatement says the high words are still zero here.
    test_a_million_replicas reaches them with a table that is not the identity.)"""
    R = 65536 + 37
    for dbeta in (0.05, -0.05):
        P = _Pop(capi, exact, monkeypatch, FAMILIES[family], R)
        P.st.do_time_steps(2, BETA)
        want, _ = _resample(P, dbeta, 1, np.arange(R, dtype=np.uint32))
        assert want["src"].max() > 2 * ROWS_PER_LAUNCH and want["distinct"] < R
        if family.startswith("board"):
            assert {32767, 32768, 65535, 65536} <= set(_sample_slots(R))
            _slots_follow_their_seeds(P, BETA + dbeta)


@pytest.mark.parametrize("family", ["board-glass", "cubic"])
def test_a_million_replicas(capi, exact, oracle, monkeypatch, family):
    """R = 2^20 + 1025, the smallest population that takes the carry loop of the scan's second pass (1026 block sums) and the
    second launch of the bit gather (32 801 groups: g0 = 32 768 with 33 groups, the last owning one bit); 33 launches of the row
    gather.  (a) equal energies: the identity, with R S >= 2^64 and slots whose low word carries; (b) two sweeps and
    dbeta = 0.05; (c) dbeta = 0.002 on the same population: a table that is not the identity with a mean weight large enough
    that the low word of j S + u carries at some slots (at dbeta = 0.05 the restatement counts none or one); (d) a caller's
    table that crosses every launch boundary in both directions and feeds every target group from many source groups."""
    R = MILLION
    P = _Pop(capi, exact, monkeypatch, FAMILIES[family], R, same_start=True)
    fam = np.arange(R, dtype=np.uint32)
    want, fam = _resample(P, 0.7, 1, fam)
    assert want["needs_high_words"] and want["low_word_carries"] > 0
    assert np.array_equal(want["src"], np.arange(R)) and want["sum"] == R << 32 and want["distinct"] == R
    P.device(P.st.do_time_steps, 2, BETA)
    want, fam = _resample(P, 0.05, 2, fam)
    assert want["distinct"] < R
    want, fam = _resample(P, 0.002, 3, fam)
    assert want["needs_high_words"] and want["low_word_carries"] > 0 and want["distinct"] < R
    src = ((np.arange(R, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(R)).astype(np.uint32)
    fam = _apply(P, src, fam)
    if family.startswith("board"):
        _slots_follow_their_seeds(P, BETA)
    P.report(f"{family} R = {R}")

"""Search (seed, t, Q) for quads with many ties and write tests/golden/tie_cases.json -- TEST INFRASTRUCTURE, numpy only.

DESIGN.md S3 / S6: the 7-bit prefixes of the 128 spins of a quad are the bits of seven Philox calls that depend on
(key, t, Q, colour) alone.  From an all-satisfied start every spin of the first pass is in one class, and beta chooses which of
the 128 prefix values v ties: a quad in which one value v is shared by n spins is a quad with n ties at that beta.  Such quads
cannot be forced, but they can be found.

    python tests/golden/make_tie_cases.py [--quads N] [--procs P]

searches N quads per domain ("LATS": the checkerboard sweep, colour 0; "PKSW": the replica-packed sweep, class 0) and keeps, per
domain, one case each with exactly 4, 5, 8 and 9 ties and the cases with the most ties (those with Q = 0, which every lattice
has; for LATS also rows 1..3 of a 256-wide lattice, interior rows for the open-boundary kernels, one case at Q = 1, the second
quad of 64 x 8; and cases with t >= 2^32).  The committed fixture is the output of the command without arguments: N = 3 * 10^8
quads per domain and pass, about four minutes per pass on eight processes.  The result is a function of N alone: chunk k of a
domain draws from numpy's PCG64 seeded with (domain, k).

A third pass searches the SECOND colour of the lattice sweep (records with "colour": 1), for the kernels that only ever run
colour 1.  Its spins are in one class only where no neighbour flipped in the colour-0 pass, so this pass looks at the prefix
value v = 0 alone: there a colour-0 spin flips with probability 1/256 and a colour-1 spin keeps its four satisfied bonds with
probability 0.98; the tests count the ties that are left on the lattice they use.
"""
import argparse
import json
import multiprocessing as mp
import os
import time

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK, S32 = np.uint64(0xFFFFFFFF), np.uint64(32)
DOMAINS = {"LATS": int.from_bytes(b"LATS", "big"), "PKSW": int.from_bytes(b"PKSW", "big")}
N_PLANES = 7
CHUNK = 50000
LAT_Q = (0, 0, 0, 1, 2, 3)  # quad of sample i: Q = LAT_Q[i % 6]; PKSW: leader position p = i % 64


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays holding 32-bit values; returns uint32[4, n]."""
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack([c0, c1, c2, c3]).astype(np.uint32)


def prefixes(dom, seeds, ts, qs, colour=0):
    """uint8[n, 128]: the prefix of the spin at word q, bit b of every sample's quad at index 32 q + b (class 0; lattice: the given colour)."""
    n = len(seeds)
    k0, k1 = seeds & MASK, seeds >> S32
    hi = (((ts >> S32) & np.uint64(0xFFFF)) << np.uint64(16)) | np.uint64(colour << 8)
    pref = np.zeros((4, n, 32), dtype=np.uint8)
    shifts = np.arange(32, dtype=np.uint32)
    for p in range(N_PLANES):
        w = philox(ts & MASK, qs, np.full(n, DOMAINS[dom], dtype=np.uint64), hi | np.uint64(p), k0, k1)
        pref |= (((w[:, :, None] >> shifts) & np.uint32(1)).astype(np.uint8) << np.uint8(N_PLANES - 1 - p))
    return pref.transpose(1, 0, 2).reshape(n, 128)


def samples(dom, chunk, colour=0):
    rng = np.random.default_rng([DOMAINS[dom], chunk] + [colour] * (colour != 0))
    seeds = rng.integers(0, 2 ** 63, size=CHUNK, dtype=np.uint64)
    ts = rng.integers(0, 2 ** 20, size=CHUNK, dtype=np.uint64)
    high = rng.integers(1, 2 ** 16, size=CHUNK, dtype=np.uint64) << S32  # every other sample: bits 32..47 of t set
    ts = np.where(np.arange(CHUNK) % 2 == 1, ts | high, ts)
    i = np.arange(CHUNK)
    qs = (np.asarray(LAT_Q)[i % 6] if dom == "LATS" else i % 64).astype(np.uint64)
    if colour:
        qs[:] = 0
    return seeds, ts, qs


def search_chunk(args):
    dom, chunk, colour = args
    seeds, ts, qs = samples(dom, chunk, colour)
    pref = prefixes(dom, seeds, ts, qs, colour)
    if colour:  # the second colour: the prefix value 0 alone, from 10 ties on
        n0 = (pref == 0).sum(axis=1)
        return [(int(n0[j]), int(seeds[j]), int(ts[j]), 0, 0, colour) for j in np.flatnonzero(n0 >= 10)]
    off = (np.arange(CHUNK, dtype=np.int64)[:, None] * 128 + pref).ravel()
    counts = np.bincount(off, minlength=CHUNK * 128).reshape(CHUNK, 128)
    mx = counts.max(axis=1)
    out = []
    keep = np.flatnonzero(mx >= 9)
    for n in (4, 5, 8):  # plentiful: the first of the chunk at Q = 0 will do
        hit = np.flatnonzero((mx == n) & ((qs == 0) | (dom == "PKSW")))
        keep = np.concatenate([keep, hit[:1]])
    for j in keep:
        out.append((int(mx[j]), int(seeds[j]), int(ts[j]), int(qs[j]), int(counts[j].argmax()), 0))
    return out


def record(dom, n, seed, t, q, v, colour):
    pref = prefixes(dom, np.array([seed], dtype=np.uint64), np.array([t], dtype=np.uint64), np.array([q], dtype=np.uint64), colour)[0]
    ties = [[int(i) >> 5, int(i) & 31] for i in np.flatnonzero(pref == v)]
    assert len(ties) == n
    return {"domain": dom, "colour": colour, "seed": seed, "t": t, "Q": q, "v": v, "n_ties": n, "ties": ties}


def boundary_sensitive(dom, c):
    """The last tie of a case with exactly 5 (9) ties is the first one of call 8 (9).  Its fate at the mid-bin threshold (low
    word 2^31) must differ from what word 3 and word 0 of the previous call would give it: a kernel that stays in the previous
    call there, at either word, then decides this spin wrongly instead of escaping by chance."""
    n, seed, t, q = c[:4]
    one = lambda x: np.array([x], dtype=np.uint64)
    words = lambda call: philox(one(t) & MASK, one(q), one(DOMAINS[dom]), one((((t >> 32) & 0xFFFF) << 16) | call), one(seed) & MASK, one(seed) >> S32)[:, 0]
    own, prev = words(N_PLANES + (n - 1) // 4), words(N_PLANES + (n - 1) // 4 - 1)
    return (own[0] < 2 ** 31) != (prev[3] < 2 ** 31) and (own[0] < 2 ** 31) != (prev[0] < 2 ** 31)


def select(dom, found):
    """The fixture's cases of one domain out of everything the search kept (deterministic: ties by (seed, t))."""
    found = sorted(set(found), key=lambda c: (-c[0], c[1], c[2]))
    chosen = []

    def take(pred, k):
        got = [c for c in found if pred(c) and c not in chosen][:k]
        chosen.extend(got)
        return got

    def first(c):  # LATS: quad 0 of colour 0, which every lattice has; PKSW: any leader of block 0
        return c[5] == 0 and (dom == "PKSW" or c[3] == 0)

    for n in (4, 5, 8, 9):
        assert take(lambda c: c[0] == n and first(c) and c[2] < 2 ** 32 and (n in (4, 8) or boundary_sensitive(dom, c)), 1), (dom, n)
    take(lambda c: c[0] >= 13, 2)                                    # wanted, not required
    take(lambda c: c[0] >= 9 and first(c) and c[2] < 2 ** 32, 5)     # the most ties, small t
    take(lambda c: c[0] >= 9 and first(c) and c[2] >= 2 ** 32, 3)    # ... and with bits 32..47 of t set
    if dom == "LATS":
        take(lambda c: c[0] >= 9 and c[3] in (1, 2, 3), 3)          # interior rows of a 256-wide lattice
        take(lambda c: c[0] >= 9 and c[3] == 1, 1)                  # the second quad of 64 x 8
        take(lambda c: c[5] == 1, 4)                                # the second colour, v = 0
    return [record(dom, *c) for c in chosen]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quads", type=int, default=300_000_000, help="quads searched per domain and pass")
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "tie_cases.json"))
    a = ap.parse_args()
    n_chunks = (a.quads + CHUNK - 1) // CHUNK
    cases, searched = [], {}
    with mp.Pool(a.procs) as pool:
        for dom in DOMAINS:
            t0, found, hist = time.time(), [], {}
            jobs = [(dom, k, 0) for k in range(n_chunks)] + [(dom, k, 1) for k in range(n_chunks) if dom == "LATS"]
            for res in pool.imap_unordered(search_chunk, jobs, chunksize=4):
                found.extend(res)
            for c in found:
                if c[0] >= 9 and c[5] == 0:
                    hist[c[0]] = hist.get(c[0], 0) + 1
            searched[dom] = {"quads": n_chunks * CHUNK, "max_bin_histogram_from_9": {str(k): hist[k] for k in sorted(hist)}}
            if dom == "LATS":
                n1 = [c[0] for c in found if c[5] == 1]
                searched[dom]["colour_1_v0_histogram_from_10"] = {str(k): n1.count(k) for k in sorted(set(n1))}
            print(dom, "quads", n_chunks * CHUNK, "seconds", round(time.time() - t0, 1), "max-bin histogram (>= 9):", sorted(hist.items()), flush=True)
            cases.extend(select(dom, found))
    with open(a.out, "w") as f:
        f.write('{"generator": "tests/golden/make_tie_cases.py",\n "searched": %s,\n "cases": [\n  ' % json.dumps(searched))
        f.write(",\n  ".join(json.dumps(c) for c in cases))  # one record per line
        f.write("\n ]\n}\n")
    print("wrote", a.out, len(cases), "cases")


if __name__ == "__main__":
    main()

"""One class pass over one quad of the bit-sliced sweeps, restated spin by spin -- TEST INFRASTRUCTURE.

Written from the S3 / S6 text alone, on Python integers: no bit-slicing, no branch on the number of ties, no oracle.  The
uniform of a spin is the 39-bit `u = prefix << 32 | low`: bit p (MSB first) of the 7-bit prefix of the spin at word q, bit b of
quad Q is bit b of word q of `P(key, (t_lo, Q, domain, ctr2(t, colour, p)))`; `low` is drawn only for a tie (prefix equal to the
top 7 bits of the spin's threshold) and is word `n % 4` of call `7 + n / 4` for the n-th tie of the quad in (word, bit) order.
A spin that does not tie is decided by its prefix whatever `low` is, so it keeps `low = 0` here.  The spin flips iff `u < T`.
"""
import math

from cluster_reference import ctr2, philox4x32_10

N_PLANES = 7
THR_BITS = 39
ALWAYS = 1 << THR_BITS
DOMAINS = {"LATS": int.from_bytes(b"LATS", "big"), "PKSW": int.from_bytes(b"PKSW", "big")}
ABSENT = -1  # class of a word's bits that hold no spin (a padding position of the packed layout)


def threshold(beta, dE):
    """T = floor(exp(-beta dE) 2^39) from the host's f64 exp; 2^39 = always, in particular for dE <= 0."""
    if dE <= 0.0:
        return ALWAYS
    p = math.exp(-beta * dE)
    if not p < 1.0:
        return ALWAYS
    return int(math.floor(math.ldexp(p, THR_BITS)))


def beta_for(v, dE):
    """The beta that puts the top 7 bits of the threshold of a class with energy cost dE on the prefix value v (mid-bin)."""
    return -math.log((v + 0.5) / 128.0) / dE


def call(domain, key, t, colour, Q, index):
    """The four 32-bit words of call `index` of quad Q (plane calls 0..6, tie calls from 7 on) as Python integers."""
    key, t = int(key), int(t)
    words = philox4x32_10(t & 0xFFFFFFFF, int(Q), DOMAINS[domain], ctr2(t, colour, index), key & 0xFFFFFFFF, key >> 32)
    return [int(w) for w in words]


def class_pass(domain, key, t, colour, Q, thresholds, classes):
    """thresholds[k]: T of class k; classes[32 q + b]: the class of the spin at word q, bit b (ABSENT: no spin).
    Returns (flip[128] of 0 / 1, (word, bit) of every tie in tie order, highest call index used)."""
    planes = [call(domain, key, t, colour, Q, p) for p in range(N_PLANES)]
    flips, ties, highest = [], [], N_PLANES - 1
    for q in range(4):
        for b in range(32):
            k = classes[32 * q + b]
            if k == ABSENT:
                flips.append(0)
                continue
            T = int(thresholds[k])
            if T >= ALWAYS:
                flips.append(1)
                continue
            prefix = 0
            for p in range(N_PLANES):
                prefix = (prefix << 1) | ((planes[p][q] >> b) & 1)
            low = 0
            if prefix == T >> 32:
                n = len(ties)
                highest = N_PLANES + n // 4
                low = call(domain, key, t, colour, Q, highest)[n % 4]
                ties.append((q, b))
            flips.append(int(((prefix << 32) | low) < T))
    return flips, ties, highest

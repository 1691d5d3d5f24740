"""The 3-input truth tables of the sweep kernels' plane and flip stages (lattice_kernels.hpp), checked against their Boolean
expressions on all eight input combinations.  No GPU needed: the constants are read from the header.

v_bitop3_b32(a, b, c) with table T gives bit ((a << 2) | (b << 1) | c) of T, bit by bit.

  BITOP_FLIP       (own, und0, lt)  own ^ (~und0 | lt)       a spin flips unless it is in a costly class (und0) and its prefix
                                                             is not below the threshold (lt, tie wins included)
  BITOP_ZERO_PAIR  (x, ra, rb)      x & ~(ra | rb)           two all-zero planes at once: (x & ~ra) & ~rb
  BITOP_LT         (r, tb, lt)      (~r & tb) | (~(r ^ tb) & lt)
  BITOP_UND        (und, r, tb)     und & ~(r ^ tb)
  BITOP_LT_NOT / BITOP_UND_NOT      the same two with ~tb in tb's place (class 3 = "not class 4" among the costly spins)
"""
import itertools
import os
import re

import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyisingmontecarlo_amd", "csrc", "lattice_kernels.hpp")


@pytest.fixture(scope="module")
def tables():
    text = open(HEADER).read()
    found = {name: int(val, 16) for name, val in re.findall(r"\b(BITOP_\w+) = (0x[0-9A-Fa-f]+)", text)}
    # every use of a table in the header goes through its name: no stray literal of the plane / flip stages is left
    assert not re.search(r"bitop3_b32\([^;]*\b(st|rr|prev)\b[^;]*, 0x[0-9A-Fa-f]+\)", text)
    return found


def table_of(f):
    return sum((f(a, b, c) & 1) << ((a << 2) | (b << 1) | c) for a, b, c in itertools.product((0, 1), repeat=3))


def bitop3(a, b, c, table, width=32):
    """the instruction itself on `width`-bit words"""
    out = 0
    for i in range(width):
        idx = (((a >> i) & 1) << 2) | (((b >> i) & 1) << 1) | ((c >> i) & 1)
        out |= ((table >> idx) & 1) << i
    return out


def test_flip_fold(tables):
    assert tables["BITOP_FLIP"] == table_of(lambda own, und0, lt: own ^ ((~und0 | lt) & 1)) == 0x4B
    # the form it replaces: acc = ~(eq3 | eq4) | lt | tie wins, new = own ^ acc
    for own, und0, lt in itertools.product((0, 1), repeat=3):
        acc = (1 - und0) | lt
        assert (tables["BITOP_FLIP"] >> ((own << 2) | (und0 << 1) | lt)) & 1 == own ^ acc


def test_zero_plane_pair(tables):
    assert tables["BITOP_ZERO_PAIR"] == table_of(lambda x, ra, rb: x & ~(ra | rb)) == 0x10
    for x, ra, rb in itertools.product((0, 1), repeat=3):   # = the two single steps one after the other
        assert (tables["BITOP_ZERO_PAIR"] >> ((x << 2) | (ra << 1) | rb)) & 1 == (x & (1 - ra)) & (1 - rb)


def test_plane_step_tables(tables):
    assert tables["BITOP_LT"] == table_of(lambda r, tb, lt: ((1 - r) & tb) | ((1 - (r ^ tb)) & lt)) == 0x8E
    assert tables["BITOP_UND"] == table_of(lambda und, r, tb: und & (1 - (r ^ tb))) == 0x90
    assert tables["BITOP_LT_NOT"] == table_of(lambda r, e, lt: ((1 - r) & (1 - e)) | ((1 - (r ^ (1 - e))) & lt)) == 0x2B
    assert tables["BITOP_UND_NOT"] == table_of(lambda und, r, e: und & (1 - (r ^ (1 - e)))) == 0x60


def test_words_without_class3_mask(tables):
    """Whole-word check of the state without eq3: for every (class, threshold bits) the planes run on (eq4, und0) give the same
    und, and the same lt INSIDE und0, as the planes run on (eq3, eq4); outside und0 the flip table ignores lt."""
    import random
    rng = random.Random(5)
    M = 0xFFFFFFFF
    for _ in range(200):
        eq4 = rng.getrandbits(32)
        eq3 = rng.getrandbits(32) & ~eq4 & M
        und0 = eq3 | eq4
        own = rng.getrandbits(32)
        lt_a = lt_b = 0
        und_a = und_b = und0
        for _plane in range(7):
            r, sel = rng.getrandbits(32), rng.randrange(4)
            tbw = (eq3 if sel & 1 else 0) | (eq4 if sel & 2 else 0)
            lt_a, und_a = bitop3(r, tbw, lt_a, tables["BITOP_LT"]), bitop3(und_a, r, tbw, tables["BITOP_UND"])
            if sel == 1:
                lt_b, und_b = bitop3(r, eq4, lt_b, tables["BITOP_LT_NOT"]), bitop3(und_b, r, eq4, tables["BITOP_UND_NOT"])
            elif sel == 0:
                lt_b, und_b = lt_b & ~r & M, und_b & ~r & M
            else:
                w = und0 if sel == 3 else eq4
                lt_b, und_b = bitop3(r, w, lt_b, tables["BITOP_LT"]), bitop3(und_b, r, w, tables["BITOP_UND"])
            assert und_a == und_b and (lt_a & und0) == (lt_b & und0)
        old = own ^ (((~und0 & M) | lt_a) & M)
        assert bitop3(own, und0, lt_b, tables["BITOP_FLIP"]) == old

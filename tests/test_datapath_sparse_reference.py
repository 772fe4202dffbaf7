"""The sparse (2:4) MFMA datapath check's reference against a plain recomputation in fractions: the compressed A is
expanded to dense through the index words and multiplied densely, decoded here from the formats' value tables. And the
conditions on the inputs that make every stage exact in any summation order (datapath_sparse_kernel.h)."""
from fractions import Fraction

import pytest

from rocm_k8s_device_plugin_amd.testing import datapath_sparse_reference as db

NONCES = (0xFFFFFFFF, 0xDEADBEEF)
# (element bits, exponent bits, mantissa bits, bias) of A and of B per data kind; int8 has no float fields
FORMAT = {db.F16: ((16, 5, 10, 15),) * 2, db.BF16: ((16, 8, 7, 127),) * 2, db.I8: ((8, 0, 0, 0),) * 2,
          db.FP8: ((8, 4, 3, 7), (8, 5, 2, 15))}


def _decode(code, width, eb, mb, bias):
    if not eb:
        return Fraction(code - 256 * (code >> 7))
    sign, field, m = code >> width - 1, code >> mb & (1 << eb) - 1, code & (1 << mb) - 1
    assert 0 < field < (1 << eb) - 1 or (field == 0 and m == 0), code          # no subnormal, Inf or NaN
    return (-1) ** sign * (Fraction((1 << mb) + m) * Fraction(2) ** (field - bias - mb) if field else 0)


def _elements(stage, side, rc, h, nw):
    width, eb, mb, bias = FORMAT[db.KIND[stage]][side]
    stream = sum(d << 32 * i for i, d in enumerate(db.fragment(stage, side, rc, h, nw)))
    return [_decode(stream >> width * e & (1 << width) - 1, width, eb, mb, bias) for e in range((128, 256)[side] // width)]


def _f32(word):
    mag = Fraction((1 << 23) + (word & 0x7FFFFF)) * Fraction(2) ** ((word >> 23 & 0xFF) - 150)
    assert 0 < word >> 23 & 0xFF < 255, hex(word)
    return -mag if word >> 31 else mag


@pytest.mark.parametrize("stage,nonce", [(s, n) for s in range(db.STAGES) for n in NONCES])
def test_tile_equals_a_dense_recomputation_and_the_inputs_make_it_exact(stage, nonce):
    dim, G, KB, sixteen = db.DIM[stage], db.groups(stage), db.kb(stage), db.bits(stage) == 16
    i8, summing = db.KIND[stage] == db.I8, db.MODE[stage] == db.SUM
    for wave in range(4):
        nw = db.wave_nonce(nonce, 0, wave)
        a = [[Fraction(0)] * (G * KB) for _ in range(dim)]
        seen = [set() for _ in range(G * KB // 4)]                              # index pairs per group position
        for row in range(dim):
            for h in range(G):
                word, comp = db.index_word(stage, row, h, nw), _elements(stage, 0, row, h, nw)
                used = word >> 16 * db.ABID[stage] & 0xFFFF if sixteen else word
                assert not sixteen or (word >> 16 * (1 - db.ABID[stage]) & 0xFFFF) != used
                for t in range(KB // 4):
                    f0, f1 = used >> 4 * t & 3, used >> 4 * t + 2 & 3
                    assert f0 < f1
                    seen[h * (KB // 4) + t].add((f0, f1))
                    for c, f in ((2 * t, f0), (2 * t + 1, f1)):
                        a[row][db.k_of(stage, h, 4 * t + f)] = comp[c]
                if db.MODE[stage] == db.SEL_B or i8:                            # band: dword by dword complements
                    d = db.fragment(stage, 0, row, h, nw)
                    assert d[1] == d[0] ^ 0xFFFFFFFF and d[3] == d[2] ^ 0xFFFFFFFF
        b = [[v for h in range(G) for v in _elements(stage, 1, col, h, nw)] for col in range(dim)]
        if db.MODE[stage] == db.SEL_A or i8:
            for col, h in ((col, h) for col in range(dim) for h in range(G)):
                d = db.fragment(stage, 1, col, h, nw)
                assert all(d[i + 1] == d[i] ^ 0xFFFFFFFF for i in (0, 2, 4, 6))
        if db.MODE[stage] == db.SEL_B:                                          # one pattern for all rows
            assert set().union(*seen) == set(db.PAIRS) and all(len(s) == 1 for s in seen)
        else:
            assert all(s == set(db.PAIRS) for s in seen), seen
        if wave:
            continue                                                           # the image holds wave 0's tiles
        tile = db.expected_tile(stage, nw)
        for row in range(dim):
            for col in range(dim):
                word = tile[row * dim + col]
                cu, cx = db.c_term(stage, row, col, nw)
                c = Fraction(cu) * Fraction(2) ** cx
                terms = [x * y for x, y in zip(a[row], b[col]) if x * y]
                assert word != 0
                if i8:
                    assert sum(map(abs, terms)) + abs(c) < 2 ** 31 and len(terms) <= G * KB // 2
                    assert (word - (1 << 32) if word >> 31 else word) == sum(terms) + c
                    continue
                assert _f32(word) == sum(terms) + c
                if not summing:
                    assert len(terms) == 1 and c == 0
                    continue
                q = Fraction(2) ** cx
                assert len(terms) == G * KB // 2 and (c / q) % 2 == 1 and all((t / q) % 2 == 1 for t in terms)
                assert sum(map(abs, terms)) + abs(c) < 2 ** 24 * q

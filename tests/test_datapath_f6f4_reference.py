"""The fp6 / fp4 MX-scaled MFMA datapath check's reference without a GPU: its tiles against a plain recomputation in
exact fractions from the formats' value tables, and the recipe's conditions (datapath_f6f4_kernel.h) stage by stage."""
from fractions import Fraction

import pytest

from rocm_k8s_device_plugin_amd.testing import datapath_f6f4_reference as db

NONCES = (0xFFFFFFFF, 0xDEADBEEF)


def _value(code, fmt):
    """A code's value from the format's table: +-(2^M + m) * 2^(E - bias - M), E >= 1; +-m * 2^(1 - bias - M), E = 0."""
    ebits, mbits, bias = {0: (4, 3, 7), 2: (2, 3, 1), 3: (3, 2, 3), 4: (2, 1, 1)}[fmt]
    field, m = (code >> mbits) % (1 << ebits), code % (1 << mbits)
    mag = Fraction((1 << mbits) + m) * Fraction(2) ** (field - bias - mbits) if field else Fraction(m, 1 << bias + mbits - 1)
    return -mag if code >> (ebits + mbits) else mag


def _terms(stage, row, col, nw):
    """[C, products in k order] of one output, each an exact fraction. A 6- or 4-bit fragment is 32 consecutive k,
    an 8-bit one two runs of 16; a scale block is 32 consecutive k."""
    ga, x = db.c_term(stage, row, col, nw)
    out, groups = [ga * Fraction(2) ** x], 2 if db.DIM[stage] == 32 else 4
    for k in range(32 * groups):
        vs = []
        for side, rc in ((0, row), (1, col)):
            fmt = db.FMT[side][stage]
            h, e = (k >> 5, k & 31) if fmt else (k >> 4 & groups - 1, k % 16 + 16 * (k // (16 * groups)))
            vs.append(_value(db.elem(stage, side, rc, h, e, nw), fmt))
        scale = Fraction(2) ** (db.scale_byte(stage, 0, row, k >> 5, nw) + db.scale_byte(stage, 1, col, k >> 5, nw) - 254)
        out.append(vs[0] * vs[1] * scale)
    return out


def _f32_bits(v):
    """A non-zero fraction that is a normal f32, converted once."""
    top = v.numerator.bit_length() - v.denominator.bit_length()
    top -= abs(v) < Fraction(2) ** top                                 # 2^top <= |v| < 2^(top+1)
    sig = abs(v) / Fraction(2) ** (top - 23)
    assert sig.denominator == 1 and 1 << 23 <= sig < 1 << 24 and -126 <= top <= 127, v
    return (v < 0) << 31 | top + 127 << 23 | int(sig) & 0x7FFFFF


@pytest.mark.parametrize("stage", range(db.STAGES))
@pytest.mark.parametrize("nonce", NONCES)
def test_tiles_equal_an_exact_recomputation_and_meet_the_stages_conditions(nonce, stage):
    nw, dim = db.wave_nonce(nonce, 0, 0), db.DIM[stage]
    tile = db.tiles_image(nonce, 1)[0, db.TILE_OFFSET[stage]:db.TILE_OFFSET[stage] + db.STAGE_WORDS[stage]]
    assert (tile != 0).all()                                           # no output word is zero
    for row, col in ((r, c) for r in range(dim) for c in range(dim)):
        ts = _terms(stage, row, col, nw)
        assert int(tile[row * dim + col]) == _f32_bits(sum(ts)), (row, col)
        if stage in db.PRODUCT_STAGES:                                 # every partial sum, in any order, is an exact f32
            q = Fraction(2) ** db.quantum(stage, row, col, nw)
            assert sum(abs(t) for t in ts) < (1 << 24) * q
            assert (ts[0] / q) % 2 == 1 and all(t != 0 and (t / q) % 2 == 0 for t in ts[1:])
        else:                                                          # C = +0 and one non-zero product
            assert ts[0] == 0 and sum(t != 0 for t in ts[1:]) == 1


@pytest.mark.parametrize("stage,side", [(0, 0), (1, 1), (2, 0), (3, 1)])
@pytest.mark.parametrize("nonce", NONCES)
def test_band_fragments_hold_band_codes_and_toggle_every_operand_bit(nonce, stage, side):
    fmt = db.FMT[side][stage]
    low, hot_positions = (1 << db.width(fmt) - 1) - 1, set()
    for wave in range(db.WAVES):
        nw = db.wave_nonce(nonce, 0, wave)
        for rc in range(db.DIM[stage]):
            hot_positions.add(db.onehot_pos(nw, stage, rc))
            for group in range(db.DIM[stage] == 16 and 4 or 2):
                words = db.fragment(stage, side, rc, group, nw)
                half = len(words) // 2                                 # 6 or 4 dwords: the second half complements the first
                assert len(words) == db.width(fmt) and all(words[d] ^ words[d + half] == db.M32 for d in range(half))
                codes = [db.elem(stage, side, rc, group, e, nw) for e in range(32)]
                assert all(0 < c & low < low for c in codes)           # never +-0 or their complements
    assert len(hot_positions) == 64                                    # the waves' rotations: every position (stage 3: 64 of 128)

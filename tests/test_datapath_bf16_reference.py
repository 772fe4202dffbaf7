"""The bf16 MFMA datapath check's recipe, on the independent reference alone
(testing/datapath_bf16_reference.py), CPU only, in Python integers: every
operand halfword lies in its band, in the product stages every term is a
multiple of the output's quantum and no partial sum of any order needs more
than 24 bits, no output word is zero, operand and result words toggle all 32
bits for every nonce, the one-hot stages select every k, and the image tells
every wrong-kernel model apart."""
import itertools
import random

import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import datapath_bf16_reference as db
from rocm_k8s_device_plugin_amd.testing import datapath_i8_reference as d8
from rocm_k8s_device_plugin_amd.testing import datapath_reference as dp

WAVE_NONCES = sorted({db.wave_nonce(n, wg, wave) for n in dp.NONCES for wg, wave in dp.WG_WAVES})
GRID = 2


def test_the_cases_are_those_of_the_int8_check():
    assert WAVE_NONCES == sorted({d8.wave_nonce(n, wg, wave) for n in dp.NONCES for wg, wave in dp.WG_WAVES})
    assert len(WAVE_NONCES) == len(dp.NONCES) * len(dp.WG_WAVES)
    assert db.wave_nonce(0xFFFFFFFF, 0, 1) < 0xFFFFFFFF            # wraps at 2^32
    assert db.WG_WORDS == 4 * 1024 + 256 and len({db.MAGIC, dp.MAGIC, d8.MAGIC}) == 3
    assert db.DEPTH == (16, 16, 16, 16, 32)


def _fields(h):
    return h >> 15, h >> 7 & 0xFF, h & 0x7F


def test_every_operand_halfword_is_in_its_band():
    """Band words: exponent field 97..158 (no zero, subnormal, Inf, NaN); one-hot: one +-2^f with f in
    -90..90 and bf16 +0 elsewhere; product stages: the row's / column's exponent field, an odd mantissa;
    stage 3: A all +0, C's exponent field 1..254."""
    for nw in WAVE_NONCES:
        for stage in range(db.STAGES):
            a, b, c = db.operands(stage, nw)
            for which, rows in (("a", a), ("b", b)):
                onehot = stage in (db.ONE_HOT_A if which == "a" else db.ONE_HOT_B)
                for rc, frag in enumerate(rows):
                    el = db.elements(frag)
                    assert len(el) == db.DEPTH[stage]
                    if which == "a" and stage in db.ZERO_A:
                        assert el == [0] * 16
                    elif onehot:
                        (k,) = [k for k, h in enumerate(el) if h]
                        _, e, m = _fields(el[k])
                        assert m == 0 and e - 127 in db.F_RANGE and k == db.onehot_position(stage, rc, nw)
                    elif stage in db.PRODUCT_STAGES:
                        exps = {_fields(h)[1] for h in el}
                        assert len(exps) == 1 and exps.pop() in db.BAND
                        assert all(_fields(h)[2] & 1 for h in el)
                    else:
                        assert all(_fields(h)[1] in db.BAND for h in el), (stage, which, rc)
            for row in c:
                for w in row:
                    if stage in (0, 1):
                        assert w == 0
                    else:
                        assert 1 <= (w >> 23 & 0xFF) <= 254
    # the band is closed under complement
    assert all((255 - e) in db.BAND for e in db.BAND) and all((255 - e) in db.C_BAND for e in db.C_BAND)
    # the mapping reaches both ends of the band and nothing outside it
    assert {db.band16(h << 7) >> 7 & 0xFF for h in range(256)} == set(db.BAND)


def test_band_fragments_pair_each_dword_with_its_complement():
    for nw in WAVE_NONCES[:4]:
        for stage, which in ((0, 0), (1, 1), (3, 1)):
            for frag in db.operands(stage, nw)[which]:
                for k in range(0, len(frag), 2):
                    assert frag[k] ^ frag[k + 1] == 0xFFFFFFFF
        _, _, c3 = db.operands(3, nw)
        assert all(row[0] ^ row[1] == 0xFFFFFFFF for row in c3)


@pytest.mark.parametrize("stage", db.PRODUCT_STAGES)
def test_every_term_is_a_multiple_of_the_quantum_and_no_partial_sum_needs_more_than_24_bits(stage):
    """In units of q = 2^(Ea_i + Eb_j - 268): every product is an odd integer in [129^2, 255^2], C an odd
    integer below 2^20, and the sum of the magnitudes, which bounds every subset sum and so every partial
    sum of every order and tree shape, is below 2^24."""
    dim, bound = db.DIM[stage], (2 ** 21 if stage == 2 else 2 ** 22)
    for nw in WAVE_NONCES:
        for i in range(dim):
            for j in range(dim):
                x = db.quantum(stage, i, j, nw)
                assert -74 <= x <= 48
                units = []
                for m, e in db.terms(stage, nw, i, j):
                    assert e >= x or m % (1 << (x - e)) == 0, (stage, i, j)
                    units.append(m << (e - x) if e >= x else m >> (x - e))
                assert len(units) == 1 + db.DEPTH[stage]
                assert units[0] & 1 and abs(units[0]) < 2 ** 20
                assert all(u & 1 and 129 ** 2 <= abs(u) <= 255 ** 2 for u in units[1:])
                assert sum(abs(u) for u in units) < bound <= 2 ** 24
                assert sum(units) & 1                               # odd: the result is not zero


def _units(stage, nw, i, j):
    x = db.quantum(stage, i, j, nw)
    out = []
    for m, e in db.terms(stage, nw, i, j):
        assert e >= x or m % (1 << (x - e)) == 0
        out.append(m << (e - x) if e >= x else m >> (x - e))
    return out


def test_every_subset_sum_of_a_handful_of_outputs_exhaustively():
    """Stage 2 (17 terms): all 2^17 subset sums of a few outputs, which is every partial sum any order or
    tree can form. Stage 4 (33 terms): every prefix of many random orders."""
    nw = WAVE_NONCES[1]
    for i, j in ((0, 0), (31, 31), (7, 20), (19, 3)):
        sums = np.zeros(1, dtype=np.int64)
        for u in _units(2, nw, i, j):
            sums = np.concatenate([sums, sums + u])
        assert len(sums) == 2 ** 17 and np.abs(sums).max() < 2 ** 21
        assert (sums == 0).sum() >= 1                               # the empty sum; a partial sum may be zero
    rng = random.Random(7)
    for i, j in ((0, 0), (15, 15), (4, 9)):
        units = _units(4, nw, i, j)
        for _ in range(200):
            rng.shuffle(units)
            assert max(abs(s) for s in itertools.accumulate(units)) < 2 ** 22


def test_no_output_word_is_zero_and_every_output_is_a_normal_f32():
    for nw in WAVE_NONCES:
        for stage in range(db.STAGES):
            tile = db.expected_tile(stage, nw)                      # f32_word refuses an inexact or subnormal value
            assert len(tile) == db.TILE_WORDS[stage]
            assert all(w & 0x7FFFFFFF and 1 <= (w >> 23 & 0xFF) <= 254 for w in tile), (hex(nw), stage)


def test_operand_and_result_words_toggle_all_32_bits():
    for nw in WAVE_NONCES:
        assert db.toggle_masks(nw) == {"A": 0xFFFFFFFF, "B": 0xFFFFFFFF, "C": 0xFFFFFFFF, "D": 0xFFFFFFFF}, hex(nw)


@pytest.mark.parametrize("stage", (0, 1))
def test_one_hot_stages_select_every_k_and_return_the_selected_element_scaled(stage):
    rotations = set()
    for nw in WAVE_NONCES:
        pos = db.selected_positions(stage, nw)
        assert sorted(pos) == sorted(list(range(16)) * 2), hex(nw)  # 32 columns over 16 k: each k twice
        assert pos == [db.onehot_position(stage, rc, nw) for rc in range(32)]
        rotations.add(pos[0])
        a, b, _ = db.operands(stage, nw)
        tile = db.expected_tile(stage, nw)
        full, hot = (a, b) if stage == 0 else (b, a)
        for i in range(32):
            for j in range(32):
                f, h = (i, j) if stage == 0 else (j, i)
                m, e = db.bf16_value(db.elements(full[f])[pos[h]])
                s, x = db.bf16_value(db.onehot_entry(stage, h, nw))
                assert abs(s) == 128 and tile[32 * i + j] == db.f32_word((m * s, e + x))
    assert len(rotations) > 4                                       # the rotation moves with the nonce


def test_stage_3_returns_c_and_the_product_stages_cancel():
    for nw in WAVE_NONCES[:4]:
        _, _, c3 = db.operands(3, nw)
        assert db.expected_tile(3, nw) == tuple(w for row in c3 for w in row)
        for stage in db.PRODUCT_STAGES:
            dim = db.DIM[stage]
            plus = minus = cancelled = 0
            for i in range(dim):
                for j in range(dim):
                    units = _units(stage, nw, i, j)
                    plus += sum(u > 0 for u in units)
                    minus += sum(u < 0 for u in units)
                    cancelled += abs(sum(units)) < max(abs(u) for u in units)
            assert plus > dim * dim * 4 and minus > dim * dim * 4 and cancelled > dim * dim // 8, (stage, cancelled)


WRONG = ["A bit 20 stuck at 0", "A's K-blocks of the lane halves swapped", "B bit 5 stuck at 1", "C bit 12 stuck at 1",
         "C dropped", "D bit 30 stuck at 0", "fragment element order of A reversed", "operands decoded as f16",
         "products truncated to their top 8 bits"]


def test_the_image_tells_every_wrong_kernel_model_apart():
    for nonce in dp.NONCES:
        good = db.tiles_image(nonce, GRID)
        models = db.wrong_kernel_models(nonce, GRID)
        assert sorted(models) == WRONG
        for name, image in models.items():
            assert image.shape == good.shape
            for wg in range(GRID):
                assert (image[wg] != good[wg]).sum() > 100, (name, hex(nonce), wg)
            v = db.verdict(db.healthy(GRID, nonce)[0], image, GRID, nonce)
            assert not v["ok"] and v["records_ok"] == 0, (name, v)


def test_rounding_of_the_models_is_to_nearest_even():
    one = 1 << 23
    assert db.f32_round((one, -23)) == 0x3F800000 and db.f32_round((-3, 0)) == 0xC0400000
    assert db.f32_round((2 * one + 1, 0)) == db.f32_round((2 * one, 0))          # a tie, to even
    assert db.f32_round((2 * one + 3, 0)) == db.f32_round((2 * one + 4, 0))
    assert db.f32_round((4 * one - 1, 0)) == db.f32_round((4 * one, 0))          # the carry moves the exponent
    assert db.f32_round((1, -149)) == 1 and db.f32_round((1, -150)) == 0 and db.f32_round((3, -150)) == 2
    assert db.f32_round((1, 128)) == 0x7F800000 and db.f32_round((0, 5)) == 0
    with pytest.raises(AssertionError):
        db.f32_word((2 * one + 1, 0))                                              # 25 bits: no exact f32


@pytest.mark.parametrize("bit", range(32))
def test_reference_verdict_fails_every_stuck_bit(bit):
    recs, tiles = db.healthy(1, 0xDEADBEEF)
    for value in (0, 1):
        v = db.verdict(recs, db.stuck_bit(tiles, bit, value), 1, 0xDEADBEEF)
        assert not v["ok"] and v["tile_bad"] > 0 and v["first_bad_xor"] == 1 << bit, (bit, value, v)


def test_accumulator_elements_cover_each_tile_once():
    for stage in range(db.STAGES):
        seen = sorted(db.accumulator_element(stage, lane, reg) for lane in range(64)
                      for reg in range(db.ACC_REGS[stage]))
        dim = db.DIM[stage]
        assert seen == [(i, j) for i in range(dim) for j in range(dim)]


def test_injection_image_changes_one_counter_and_at_most_one_word():
    nonce = 7
    good = db.tiles_image(nonce, GRID)
    for stage in range(db.STAGES):
        for wave in range(4):
            inj = {"kind": "mfma", "wg": 1, "wave": wave, "lane": 37, "index": stage * 16 + 2, "mask": 0x80000001}
            bad, tiles = db.injection_image(nonce, GRID, inj)
            assert bad.sum() == 1 and bad[1, stage] == 1
            diff = np.argwhere(tiles != good)
            assert len(diff) == (1 if wave == 0 else 0)
            if wave == 0:
                i, j = db.accumulator_element(stage, 37, 2)
                assert tuple(diff[0]) == (1, db.TILE_OFFSET[stage] + i * db.DIM[stage] + j)
    # an index that names no register of its stage does nothing
    for index in (4 * 16 + 4, 5 * 16, 1000):
        inj = {"kind": "mfma", "wg": 1, "wave": 0, "lane": 0, "index": index, "mask": 1}
        bad, tiles = db.injection_image(nonce, GRID, inj)
        assert bad.sum() == 0 and (tiles == good).all()
    bad, tiles = db.injection_image(nonce, GRID, None)
    assert bad.sum() == 0 and (tiles == good).all()

"""The f16 MFMA datapath check's recipe, on the independent reference alone
(testing/datapath_f16_reference.py), CPU only, in Python integers: the band is
closed under complement and band fragments pair each dword with its
complement, the one-hot stages return the selected element times the hot
element and select every k position, stage 2's outputs are 22-bit products,
in the sum stages every term is an odd multiple of the output's quantum and no
partial sum of any order needs more than 23 bits, every k of all four
instruction shapes carries a term, no output word is zero, and the image tells
every wrong-kernel model apart."""
import itertools
import random

import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import datapath_bf16_reference as dbf
from rocm_k8s_device_plugin_amd.testing import datapath_f16_reference as db
from rocm_k8s_device_plugin_amd.testing import datapath_fp8_reference as df8
from rocm_k8s_device_plugin_amd.testing import datapath_i8_reference as d8
from rocm_k8s_device_plugin_amd.testing import datapath_reference as dp

WAVE_NONCES = sorted({db.wave_nonce(n, wg, wave) for n in dp.NONCES for wg, wave in dp.WG_WAVES})
FEW = WAVE_NONCES[:4]
GRID = 2


def test_the_cases_are_those_of_the_int8_check_and_the_layout_is_the_issues():
    assert WAVE_NONCES == sorted({d8.wave_nonce(n, wg, wave) for n in dp.NONCES for wg, wave in dp.WG_WAVES})
    assert db.wave_nonce(0xFFFFFFFF, 0, 1) < 0xFFFFFFFF            # wraps at 2^32
    assert db.WG_WORDS == 5 * 1024 + 2 * 256 and db.STAGES == 7
    assert len({db.MAGIC, dp.MAGIC, d8.MAGIC, dbf.MAGIC, df8.MAGIC}) == 5
    assert db.MAGIC == int.from_bytes(b"DPHF", "big")
    # 32x32x16 four times, 16x16x32, 32x32x8, 16x16x16
    assert db.DIM == (32, 32, 32, 32, 16, 32, 16) and db.DEPTH == (16, 16, 16, 16, 32, 8, 16)
    assert db.DWORDS == (4, 4, 4, 4, 4, 2, 2) and db.BLOCKS == (2, 2, 2, 2, 4, 2, 4)
    assert db.TILE_OFFSET == (0, 1024, 2048, 3072, 4096, 4352, 5376)
    assert db.TILE_OFFSET[-1] + db.TILE_WORDS[-1] == db.WG_WORDS


def test_the_band_is_closed_under_complement_and_holds_no_special_value():
    band = [h for h in range(1 << 16) if db.in_band(h)]
    assert len(band) == 2 * 30 * 1024
    assert {db.band16(h) for h in range(1 << 16)} == set(band)      # the mapping reaches all of it, and only it
    assert all(db.in_band(h ^ 0xFFFF) for h in band)
    for h in band[::97]:
        m, e = db.f16_value(h)
        assert 1024 <= abs(m) < 2048 and -24 <= e <= 5              # +-(1024+m) * 2^(E-25), E in 1..30
        assert db.f32_value(db.widen(h)) == (m << 13, e - 13)       # the integer widening keeps the value
    assert db.widen(0) == 0 and db.widen(0x8000) == 0x80000000
    # IEEE half: 0x3C00 = 1, 0x7BFF = 65504, 0x0400 = 2^-14
    assert db.f16_value(0x3C00) == (1024, -10) and db.f16_value(0x7BFF) == (2047, 5)
    assert db.f16_value(0x0400) == (1024, -24)


def test_band_fragments_pair_each_dword_with_its_complement():
    for nw in WAVE_NONCES:
        for stage, which in ((0, 0), (1, 1), (2, 0)):
            for frag in db.operands(stage, nw)[which]:
                assert len(frag) == 8 and all(db.in_band(h) for h in db.elements(frag))
                assert all(frag[k] ^ frag[k + 1] == 0xFFFFFFFF for k in range(0, 8, 2))
        masks = db.toggle_masks(nw)
        assert masks == {"A": 0xFFFFFFFF, "B": 0xFFFFFFFF}          # all 32 bits, both values, in every fragment


@pytest.mark.parametrize("stage", db.ONE_HOT_STAGES)
def test_one_hot_stages_select_every_position_and_return_the_selected_element_times_the_hot_one(stage):
    rotations = set()
    for nw in WAVE_NONCES:
        pos = db.selected_positions(stage, nw)
        assert pos == [db.onehot_position(stage, rc, nw) for rc in range(32)]
        assert sorted(pos) == sorted(list(range(16)) * 2), hex(nw)  # 32 rows / columns over 16 k: each k twice
        rotations.add(pos[0])
        a, b, c = db.operands(stage, nw)
        assert all(w == 0 for row in c for w in row)
        tile = db.expected_tile(stage, nw)
        hot_is_b = stage in db.ONE_HOT_B
        full, hot = (a, b) if hot_is_b else (b, a)
        for i in range(32):
            for j in range(32):
                f, h = (i, j) if hot_is_b else (j, i)
                m, e = db.f16_value(db.elements(full[f])[pos[h]])
                hm, he = db.f16_value(db.onehot_entry(stage, h, nw))
                assert db.in_band(db.onehot_entry(stage, h, nw)) and db.elements(hot[h])[pos[h]] == \
                    db.onehot_entry(stage, h, nw)
                if stage in db.FULL_HOT:
                    assert 1024 <= abs(hm) < 2048
                else:
                    assert abs(hm) == 1024                          # a power of two
                w = tile[32 * i + j]
                assert w == db.f32_word((m * hm, e + he))
                assert 127 - 28 <= (w >> 23 & 0xFF) <= 127 + 31     # |D| in [2^-28, 2^32)
    assert len(rotations) >= 4                                      # the rotation moves with the nonce


def test_stage_2_outputs_are_22_bit_products_that_use_the_whole_multiplier():
    wide = low_a = low_b = 0
    for nw in FEW:
        a, b, _ = db.operands(2, nw)
        pos = db.selected_positions(2, nw)
        for i in range(32):
            for j in range(32):
                (m, _), (hm, _) = db.f16_value(db.elements(a[i])[pos[j]]), db.f16_value(db.onehot_entry(2, j, nw))
                p = abs(m * hm)
                assert 2 ** 20 <= p < 2 ** 22
                wide += (p & -p).bit_length() == 1                  # an odd product: all 22 (21) bits significant
                low_a += bool(m & 7)
                low_b += bool(hm & 7)
        word = db.expected_tile(2, nw)
        assert any(w & 0x4 for w in word)                           # a 22-bit product's lowest bit is D's bit 2
        assert not any(w & 0x3 for w in word)
    assert wide > 500 and low_a > 3000 and low_b > 3000             # mantissa bits 0..2 of both operands matter


def _units(stage, nw, i, j):
    x = db.quantum(stage, i, j, nw)
    out = []
    for m, e in db.terms(stage, nw, i, j):
        assert e >= x or m % (1 << (x - e)) == 0, (stage, i, j)             # a multiple of q
        out.append(m << (e - x) if e >= x else m >> (x - e))
    return out


@pytest.mark.parametrize("stage", db.SUM_STAGES)
def test_every_term_is_an_odd_multiple_of_the_quantum_and_no_partial_sum_needs_more_than_23_bits(stage):
    """In units of q: C an odd integer below 2^21, every product an odd integer of at most 2047 * 63 < 2^17, and
    the sum of the magnitudes, which bounds every subset sum and so every partial sum of every order and tree
    shape, below 2^23 < 2^24. Every k of the instruction's shape carries a term."""
    dim = db.DIM[stage]
    for nw in (WAVE_NONCES if dim == 16 else FEW):
        a, b, _ = db.operands(stage, nw)
        for rows, narrow in ((a, stage in db.NARROW_A), (b, stage not in db.NARROW_A)):
            for frag in rows:
                el = db.elements(frag)
                assert len(el) == db.DEPTH[stage] and len({h >> 10 & 0x1F for h in el}) == 1 and db.in_band(el[0])
                if narrow:                                          # +-(32 + m') * 2^(E-20), m' odd
                    assert all(h & 0x1F == 0 and h & 0x20 for h in el)
                else:                                               # +-(1024 + m) * 2^(E-25), m odd
                    assert all(h & 1 for h in el)
        for i in range(dim):
            for j in range(dim):
                assert -43 <= db.quantum(stage, i, j, nw) <= 15
                units = _units(stage, nw, i, j)
                assert len(units) == 1 + db.DEPTH[stage]            # C and one term per k
                assert units[0] & 1 and abs(units[0]) < 2 ** 21
                assert all(u & 1 and 1025 * 33 <= abs(u) <= 2047 * 63 < 2 ** 17 for u in units[1:])
                assert sum(abs(u) for u in units[1:]) < (2 ** 22 if db.DEPTH[stage] == 32 else 2 ** 21)
                assert sum(abs(u) for u in units) < 2 ** 23
                assert sum(units) & 1                               # odd: the result is not zero


def test_every_subset_sum_of_a_handful_of_outputs_exhaustively():
    """Stage 3 (17 terms): all 2^17 subset sums of a few outputs, which is every partial sum any order or
    tree can form. The other sum stages: every prefix of many random orders."""
    nw = WAVE_NONCES[1]
    for i, j in ((0, 0), (31, 31), (7, 20), (19, 3)):
        sums = np.zeros(1, dtype=np.int64)
        for u in _units(3, nw, i, j):
            sums = np.concatenate([sums, sums + u])
        assert len(sums) == 2 ** 17 and np.abs(sums).max() < 2 ** 23
    rng = random.Random(7)
    for stage in (4, 5, 6):
        for i, j in ((0, 0), (15, 15), (4, 9)):
            units = _units(stage, nw, i, j)
            for _ in range(100):
                rng.shuffle(units)
                assert max(abs(s) for s in itertools.accumulate(units)) < 2 ** 23


def test_the_sum_stages_mix_signs_and_cancel():
    for nw in FEW[:2]:
        for stage in db.SUM_STAGES:
            dim = db.DIM[stage]
            plus = minus = cancelled = 0
            for i in range(dim):
                for j in range(dim):
                    units = _units(stage, nw, i, j)
                    plus += sum(u > 0 for u in units)
                    minus += sum(u < 0 for u in units)
                    cancelled += abs(sum(units[1:])) < max(abs(u) for u in units[1:])
            assert plus > dim * dim * 2 and minus > dim * dim * 2 and cancelled > dim * dim // 16, (stage, cancelled)


def test_no_output_word_is_zero_and_every_output_is_a_normal_f32():
    for nw in WAVE_NONCES:
        for stage in range(db.STAGES):
            tile = db.expected_tile(stage, nw)                      # f32_word refuses an inexact or subnormal value
            assert len(tile) == db.TILE_WORDS[stage]
            assert all(w & 0x7FFFFFFF and 1 <= (w >> 23 & 0xFF) <= 254 for w in tile), (hex(nw), stage)


WRONG = sorted(["halves of A's dwords swapped", "A's K-blocks of the lane groups swapped",
                "A of the legacy forms laid out by the x16 k-map", "operands decoded as bf16",
                "mantissa bits 0..2 of A and B dropped", "products truncated to their top 16 bits", "C dropped",
                "A bit 17 stuck at 0", "B bit 2 stuck at 1", "C bit 12 stuck at 1", "D bit 30 stuck at 0"])
LEGACY = {5, 6}


def test_the_image_tells_every_wrong_kernel_model_apart():
    for nonce in dp.NONCES[:2]:
        good = db.tiles_image(nonce, GRID)
        models = db.wrong_kernel_models(nonce, GRID)
        assert sorted(models) == WRONG
        for name, image in models.items():
            assert image.shape == good.shape
            for wg in range(GRID):
                assert (image[wg] != good[wg]).sum() > 100, (name, hex(nonce), wg)
            v = db.verdict(db.healthy(GRID, nonce)[0], image, GRID, nonce)
            assert not v["ok"] and v["records_ok"] == 0, (name, v)
            stages = {db.stage_of_word(int(w)) for w in np.flatnonzero(image[0] != good[0])}
            if "legacy" in name:
                assert stages == LEGACY, (name, stages)             # both legacy forms, and only they
            elif name == "mantissa bits 0..2 of A and B dropped":
                assert stages == set(range(db.STAGES)), (name, stages)
            elif name == "products truncated to their top 16 bits":
                assert stages == {2, 3, 4, 5, 6}, (name, stages)    # a power of two times 11 bits fits 16 bits
            else:
                assert stages & LEGACY and stages - LEGACY, (name, stages)


@pytest.mark.parametrize("bit", range(32))
def test_reference_verdict_fails_every_stuck_bit_of_d_the_recipe_can_set(bit):
    """A 22-bit product sets D's bits 2 and up, an odd sum below 2^23 quanta bits 1 and up (bit 1 only from
    2^22 on): bit 0 of D is never set and stuck at 0 there shows nothing, like a bit 1 no output of this image
    sets. Every other stuck bit fails the verdict."""
    recs, tiles = db.healthy(1, 0xDEADBEEF)
    ever = int(np.bitwise_or.reduce(tiles.ravel()))
    assert not ever & 1 and ever >> 2 == 2 ** 30 - 1
    for value in (0, 1):
        v = db.verdict(recs, db.stuck_bit(tiles, bit, value), 1, 0xDEADBEEF)
        if value == 0 and not ever >> bit & 1:
            assert bit < 2 and v["ok"]
        else:
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
    for index in (4 * 16 + 4, 6 * 16 + 4, 7 * 16, 1000):
        inj = {"kind": "mfma", "wg": 1, "wave": 0, "lane": 0, "index": index, "mask": 1}
        bad, tiles = db.injection_image(nonce, GRID, inj)
        assert bad.sum() == 0 and (tiles == good).all()
    bad, tiles = db.injection_image(nonce, GRID, None)
    assert bad.sum() == 0 and (tiles == good).all()

"""The fp8 / MX-scaled MFMA datapath check's recipe, on the independent
reference alone (testing/datapath_fp8_reference.py), CPU only, in Python
integers: every operand byte and scale byte lies in its band and band fragments
pair each dword with its complement, the one-hot stages return the selected
element times the powers of two as a normal f32 and select every position and
every scale byte position, in the product stages every term is a multiple of
the output's quantum and no partial sum of any order needs more than 24 bits,
no output word is zero, and the image tells every wrong-kernel model apart."""
import itertools
import random

import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import datapath_bf16_reference as dbf
from rocm_k8s_device_plugin_amd.testing import datapath_fp8_reference as db
from rocm_k8s_device_plugin_amd.testing import datapath_i8_reference as d8
from rocm_k8s_device_plugin_amd.testing import datapath_reference as dp

WAVE_NONCES = sorted({db.wave_nonce(n, wg, wave) for n in dp.NONCES for wg, wave in dp.WG_WAVES})
FEW = WAVE_NONCES[:4]
GRID = 2


def test_the_cases_are_those_of_the_int8_check_and_the_layout_is_the_issues():
    assert WAVE_NONCES == sorted({d8.wave_nonce(n, wg, wave) for n in dp.NONCES for wg, wave in dp.WG_WAVES})
    assert db.wave_nonce(0xFFFFFFFF, 0, 1) < 0xFFFFFFFF            # wraps at 2^32
    assert db.WG_WORDS == 6 * 1024 + 2 * 256 and len({db.MAGIC, dp.MAGIC, d8.MAGIC, dbf.MAGIC}) == 4
    assert db.MAGIC == int.from_bytes(b"DPF8", "big")
    assert db.DEPTH == (16, 16, 16, 32, 64, 64, 64, 128)
    assert db.TILE_OFFSET == (0, 1024, 2048, 3072, 3328, 4352, 5376, 6400)
    # the formats of the eight stages: fp8_fp8, bf8_bf8, fp8_bf8, bf8_fp8; cbsz / blgp 0,1  1,0  0,0  1,1
    assert list(zip(db.FMT_A, db.FMT_B)) == [(0, 0), (1, 1), (0, 1), (1, 0), (0, 1), (1, 0), (0, 0), (1, 1)]


def test_the_bands_are_closed_under_complement_and_hold_no_special_value():
    for fmt in (db.E4M3, db.E5M2):
        band = [b for b in range(256) if db.in_band(b, fmt)]
        assert {db.band8(h, fmt) for h in range(256)} == set(band)          # the mapping reaches all of it, only it
        assert all(db.in_band(b ^ 0xFF, fmt) for b in band)
        top = 15 if fmt == db.E4M3 else 31
        for b in band:
            _, m, e = db.fields(b, fmt)
            assert 1 <= e < top                                             # no zero, subnormal, Inf or NaN
            mant, exp = db.fp8_value(b, fmt)
            assert abs(mant) == (8 + m if fmt == db.E4M3 else 4 + m) and exp == e - (10 if fmt == db.E4M3 else 17)
    assert all(255 - s in db.SCALE_BAND for s in db.SCALE_BAND) and 255 not in db.SCALE_BAND
    assert db.SCALE_BASE[0] + 0 >= db.SCALE_BAND[0] and db.SCALE_BASE[-1] + 3 <= db.SCALE_BAND[-1]
    # the OCP values: e4m3 0x38 = 1, 0x7E = 448; e5m2 0x3C = 1, 0x7B = 57344
    assert db.fp8_value(0x38, db.E4M3) == (8, -3) and db.fp8_value(0x7E, db.E4M3) == (14, 5)
    assert db.fp8_value(0x3C, db.E5M2) == (4, -2) and db.fp8_value(0x7B, db.E5M2) == (7, 13)


def test_every_operand_byte_and_scale_byte_is_in_its_band():
    for nw in WAVE_NONCES:
        for stage in range(db.STAGES):
            a, b, c, sa, sb = db.operands(stage, nw)
            for which, rows, fmt in ((0, a, db.FMT_A[stage]), (1, b, db.FMT_B[stage])):
                onehot = stage in (db.ONE_HOT_B if which else db.ONE_HOT_A)
                for rc, frag in enumerate(rows):
                    el = db.byte_list(frag)
                    assert len(el) == db.DEPTH[stage]
                    if onehot:
                        (k,) = [k for k, byte in enumerate(el) if byte]
                        _, m, e = db.fields(el[k], fmt)
                        assert m == 0 and db.in_band(el[k], fmt) and k == db.onehot_position(stage, rc, nw)
                    elif stage in db.PRODUCT_STAGES:
                        exps = {db.fields(byte, fmt)[2] for byte in el}
                        assert len(exps) == 1 and exps.pop() in db.EXP_BAND[fmt]
                        assert all(db.fields(byte, fmt)[1] & 1 for byte in el)
                    else:
                        assert all(db.in_band(byte, fmt) for byte in el), (stage, which, rc)
                        assert all(frag[k] ^ frag[k + 1] == 0xFFFFFFFF for k in range(0, len(frag), 2))
            assert (sa is None) == (sb is None) == (stage not in db.SCALED_STAGES)
            for which, words in ((0, sa), (1, sb)):
                for rc, row in enumerate(words or ()):
                    for h, w in enumerate(row):
                        four = [w >> 8 * p & 0xFF for p in range(4)]
                        assert all(s in db.SCALE_BAND for s in four) and len(set(four)) == 4, (stage, which, rc, h)
                        assert four[db.SCALE_SEL[stage][which]] == db.scale_byte(nw, stage, which, rc, h)
                        if stage in db.PRODUCT_STAGES:
                            d = four[db.SCALE_SEL[stage][which]] - db.scale_base(nw, stage, which, rc)
                            assert 0 <= d <= 3 and db.scale_base(nw, stage, which, rc) in db.SCALE_BASE
            for row in c:
                assert all((w == 0) == (stage in db.ONE_HOT_STAGES) for w in row)


def test_every_scale_byte_position_is_selected_for_a_and_for_b():
    assert sorted(sel[0] for sel in db.SCALE_SEL.values()) == [0, 1, 2, 3]
    assert sorted(sel[1] for sel in db.SCALE_SEL.values()) == [0, 1, 2, 3]
    assert all(a != b for a, b in db.SCALE_SEL.values())                    # and A's differs from B's in every stage


def test_every_bit_of_the_operand_and_scale_paths_takes_both_values_in_every_band_fragment():
    for nw in FEW:
        for stage, which in ((0, 0), (1, 1), (4, 0), (5, 1)):
            dw = db.DWORDS[stage]
            for row in db.operands(stage, nw)[which]:
                for h in range(db.BLOCKS[stage]):
                    frag = row[h * dw:(h + 1) * dw]
                    ones = zeros = 0
                    for w in frag:
                        ones, zeros = ones | w, zeros | (w ^ 0xFFFFFFFF)
                    assert ones & zeros == 0xFFFFFFFF
        # the scale bytes' eight bits over a tile
        for stage in (4, 5):
            for which in (0, 1):
                sel = [s for row in db.selected_scales(stage, which, db.operands(stage, nw)[3 + which]) for s in row]
                assert all(any(s >> bit & 1 for s in sel) and any(not s >> bit & 1 for s in sel) for bit in range(8))


@pytest.mark.parametrize("stage", db.ONE_HOT_STAGES)
def test_one_hot_stages_select_every_position_and_return_the_selected_element_scaled(stage):
    """D = +-(band element) * 2^f * 2^(sa + sb - 254), a normal f32 by the bound: |element| in 2^-14..2^16,
    f in -14..15, the scales' sum in -60..62, so |D| in 2^-88..2^93 whatever the formats."""
    positions = db.DEPTH[stage]
    rotations = set()
    for base in (0x1234567, 0xFFFFFFFF):
        waves = [db.wave_nonce(base, 3, v) for v in range(4)]
        if stage in db.SCALED_STAGES:                   # 32 entries over 64 positions: the four waves together
            assert {p for nw in waves for p in db.selected_positions(stage, nw)} == set(range(64))
    for nw in WAVE_NONCES:
        pos = db.selected_positions(stage, nw)
        assert pos == [db.onehot_position(stage, rc, nw) for rc in range(32)]
        assert len(set(pos)) == min(32, positions)
        if positions == 16:
            assert sorted(pos) == sorted(list(range(16)) * 2), hex(nw)      # 32 columns over 16 k: each k twice
        rotations.add(pos[0])
        a, b, _, sa, sb = db.operands(stage, nw)
        ssa, ssb = db.selected_scales(stage, 0, sa), db.selected_scales(stage, 1, sb)
        tile = db.expected_tile(stage, nw)
        hot_is_b = stage in db.ONE_HOT_B
        full, hot = (a, b) if hot_is_b else (b, a)
        ffull, fhot = (db.FMT_A[stage], db.FMT_B[stage]) if hot_is_b else (db.FMT_B[stage], db.FMT_A[stage])
        for i in range(32):
            for j in range(32):
                f, h = (i, j) if hot_is_b else (j, i)
                m, e = db.fp8_value(db.byte_list(full[f])[pos[h]], ffull)
                s, x = db.fp8_value(db.onehot_entry(stage, fhot, h, nw), fhot)
                blk = db.scale_block(stage, pos[h])
                scale = ssa[i][blk] + ssb[j][blk] - 254
                assert abs(s) == (8, 4)[fhot] and -14 <= x + (3, 2)[fhot] <= 15 and -60 <= scale <= 62
                w = tile[32 * i + j]
                assert w == db.f32_word((m * s, e + x + scale)) and 127 - 88 <= (w >> 23 & 0xFF) <= 127 + 93
    assert len(rotations) >= 4                                              # the rotation moves with the nonce


def _units(stage, nw, i, j):
    x = db.quantum(stage, i, j, nw)
    out = []
    for m, e in db.terms(stage, nw, i, j):
        assert e >= x or m % (1 << (x - e)) == 0, (stage, i, j)             # a multiple of q
        out.append(m << (e - x) if e >= x else m >> (x - e))
    return out


@pytest.mark.parametrize("stage", db.PRODUCT_STAGES)
def test_every_term_is_a_multiple_of_the_quantum_and_no_partial_sum_needs_more_than_24_bits(stage):
    """In units of q: C an odd integer below 2^20, every product an odd integer below 2^8 times 2^(d + d')
    (d = d' = 0 in the non-scaled stages), and the sum of the magnitudes, which bounds every subset sum and
    so every partial sum of every order and tree shape, below 2^21, 2^21, 2^22, 2^23 <= 2^24."""
    dim, scaled = db.DIM[stage], stage in db.SCALED_STAGES
    bound = {2: 2 ** 21, 3: 2 ** 21, 6: 2 ** 22, 7: 2 ** 23}[stage]
    lo, hi = {(0, 1): (9 * 5, 15 * 7), (1, 0): (9 * 5, 15 * 7), (0, 0): (81, 225), (1, 1): (25, 49)}[
        (db.FMT_A[stage], db.FMT_B[stage])]
    for nw in (WAVE_NONCES if dim == 16 else FEW):
        for i in range(dim):
            for j in range(dim):
                assert -62 <= db.quantum(stage, i, j, nw) <= 56
                units = _units(stage, nw, i, j)
                assert len(units) == 1 + db.DEPTH[stage]
                assert units[0] & 1 and abs(units[0]) < 2 ** 20
                for k, u in enumerate(units[1:]):
                    h = db.scale_block(stage, k)
                    shift = (db.scale_offset(nw, stage, 0, i, h) + db.scale_offset(nw, stage, 1, j, h)) if scaled else 0
                    assert u % (1 << shift) == 0 and (u >> shift) & 1 and lo <= abs(u >> shift) <= hi < 2 ** 8
                    assert abs(u) < (2 ** 14 if scaled else 2 ** 8)
                assert sum(abs(u) for u in units) < bound <= 2 ** 24
                assert sum(units) & 1                                       # odd: the result is not zero


def test_every_subset_sum_of_a_handful_of_outputs_exhaustively():
    """Stage 2 (17 terms): all 2^17 subset sums of a few outputs, which is every partial sum any order or
    tree can form. Stages 3, 6 and 7 (33, 65, 129 terms): every prefix of many random orders."""
    nw = WAVE_NONCES[1]
    for i, j in ((0, 0), (31, 31), (7, 20), (19, 3)):
        sums = np.zeros(1, dtype=np.int64)
        for u in _units(2, nw, i, j):
            sums = np.concatenate([sums, sums + u])
        assert len(sums) == 2 ** 17 and np.abs(sums).max() < 2 ** 21
    rng = random.Random(7)
    for stage, bound in ((3, 2 ** 21), (6, 2 ** 22), (7, 2 ** 23)):
        for i, j in ((0, 0), (15, 15), (4, 9)):
            units = _units(stage, nw, i, j)
            for _ in range(100):
                rng.shuffle(units)
                assert max(abs(s) for s in itertools.accumulate(units)) < bound


def test_the_product_stages_mix_signs_scales_and_cancel():
    for nw in FEW[:2]:
        for stage in db.PRODUCT_STAGES:
            dim = db.DIM[stage]
            plus = minus = cancelled = 0
            for i in range(dim):
                for j in range(dim):
                    units = _units(stage, nw, i, j)
                    plus += sum(u > 0 for u in units)
                    minus += sum(u < 0 for u in units)
                    cancelled += abs(sum(units[1:])) < max(abs(u) for u in units[1:])
            assert plus > dim * dim * 4 and minus > dim * dim * 4 and cancelled > dim * dim // 16, (stage, cancelled)
        for stage in (6, 7):                            # the blocks of one output carry different scales
            offs = {(db.scale_offset(nw, stage, 0, i, h), db.scale_offset(nw, stage, 1, i, h))
                    for i in range(db.DIM[stage]) for h in range(db.BLOCKS[stage])}
            assert {d for d, _ in offs} == {0, 1, 2, 3} == {d for _, d in offs}


def test_no_output_word_is_zero_and_every_output_is_a_normal_f32():
    for nw in WAVE_NONCES:
        for stage in range(db.STAGES):
            tile = db.expected_tile(stage, nw)                      # f32_word refuses an inexact or subnormal value
            assert len(tile) == db.TILE_WORDS[stage]
            assert all(w & 0x7FFFFFFF and 1 <= (w >> 23 & 0xFF) <= 254 for w in tile), (hex(nw), stage)


WRONG = sorted(["byte order of A's fragments reversed", "A's K-blocks swapped", "e4m3 read as e5m2 and e5m2 as e4m3",
                "the fnuz exponent bias", "the scales ignored", "the scale taken from the next byte",
                "the scale taken from the neighbouring lane", "the scales applied to C as well", "C dropped",
                "each lane's scale applied to its own fragment",
                "A bit 20 stuck at 0", "B bit 5 stuck at 1", "scale bit 2 stuck at 1", "scale bit 27 stuck at 0",
                "C bit 12 stuck at 1", "D bit 30 stuck at 0"])


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
            # a model of the scale path shows in the scaled stages alone, one of an operand path in both families
            stages = {db.stage_of_word(int(w)) for w in np.flatnonzero(image[0] != good[0])}
            if "scale" in name:
                assert stages and stages <= set(db.SCALED_STAGES), (name, stages)
            elif name != "D bit 30 stuck at 0":
                assert stages & set(db.SCALED_STAGES) and (stages - set(db.SCALED_STAGES) or name == "C dropped"), name


@pytest.mark.parametrize("bit", range(32))
def test_reference_verdict_fails_every_stuck_bit_of_d_the_recipe_can_set(bit):
    """Every sum is below 2^21 q, so bits 0..2 of D are never set (tests/test_native_datapath_fp8.py): stuck at
    0 there shows nothing, every other stuck bit does."""
    recs, tiles = db.healthy(1, 0xDEADBEEF)
    for value in (0, 1):
        v = db.verdict(recs, db.stuck_bit(tiles, bit, value), 1, 0xDEADBEEF)
        if bit < 3 and value == 0:
            assert v["ok"]
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
    for index in (3 * 16 + 4, 7 * 16 + 4, 8 * 16, 1000):
        inj = {"kind": "mfma", "wg": 1, "wave": 0, "lane": 0, "index": index, "mask": 1}
        bad, tiles = db.injection_image(nonce, GRID, inj)
        assert bad.sum() == 0 and (tiles == good).all()
    bad, tiles = db.injection_image(nonce, GRID, None)
    assert bad.sum() == 0 and (tiles == good).all()

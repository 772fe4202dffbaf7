"""The int8 MFMA datapath check's recipe, on the independent reference alone
(testing/datapath_i8_reference.py), CPU only, in Python integers: no output
comes near int32 overflow in any summation order, operand and result words
toggle all 32 bits for every nonce, the one-hot stages select every fragment
position exactly once, and the image tells every wrong-kernel model apart."""
import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import datapath_i8_reference as d8
from rocm_k8s_device_plugin_amd.testing import datapath_reference as dp

WAVE_NONCES = sorted({d8.wave_nonce(n, wg, wave) for n in dp.NONCES for wg, wave in dp.WG_WAVES})
GRID = 2


def test_the_cases_are_those_of_the_f32_check():
    assert len(WAVE_NONCES) == len(dp.NONCES) * len(dp.WG_WAVES)
    assert d8.wave_nonce(0xFFFFFFFF, 0, 1) < 0xFFFFFFFF            # wraps at 2^32
    assert d8.WG_WORDS == 4 * 1024 + 256 and d8.MAGIC != dp.MAGIC


@pytest.mark.parametrize("stage", range(d8.STAGES))
def test_no_output_can_overflow_in_any_summation_order(stage):
    """|C| + sum |a|*|b| bounds every partial sum of every order."""
    for nw in WAVE_NONCES:
        assert d8.overflow_margin(stage, nw) <= 2 ** 31 - 1, f"wave nonce {nw:#x}"
    # the stages with a product sum: the bound the recipe states
    if stage in (2, 4):
        depth = d8.BLOCKS[stage] * 16
        for nw in WAVE_NONCES[:3]:
            assert d8.overflow_margin(stage, nw) <= 2 ** 30 + depth * 128 * 128


def test_any_bytes_fragments_pair_each_dword_with_its_complement():
    for nw in WAVE_NONCES[:4]:
        for stage, which in ((0, 0), (1, 1), (2, 0), (2, 1), (3, 1), (4, 0), (4, 1)):
            for frag in d8.operands(stage, nw)[which]:
                for k in range(0, len(frag), 2):
                    assert frag[k] ^ frag[k + 1] == 0xFFFFFFFF
        _, _, c3 = d8.operands(3, nw)
        assert all(row[0] ^ row[1] == 0xFFFFFFFF for row in c3)
        a3, _, _ = d8.operands(3, nw)
        assert all(w == 0 for frag in a3 for w in frag)


def test_operand_and_result_words_toggle_all_32_bits():
    for nw in WAVE_NONCES:
        assert d8.toggle_masks(nw) == {"A": 0xFFFFFFFF, "B": 0xFFFFFFFF, "C": 0xFFFFFFFF, "D": 0xFFFFFFFF}, hex(nw)


@pytest.mark.parametrize("stage", (0, 1))
def test_one_hot_stages_select_each_of_the_32_positions_exactly_once(stage):
    rotations = set()
    for nw in WAVE_NONCES:
        pos = d8.selected_positions(stage, nw)
        assert sorted(pos) == list(range(32)), hex(nw)
        assert pos == [d8.onehot_position(stage, rc, nw) for rc in range(32)]
        rotations.add(pos[0])
        # the tile is the selected byte of the other operand, with the selector's sign
        a, b, _ = d8.operands(stage, nw)
        tile = d8.expected_tile(stage, nw)
        full, hot = (a, b) if stage == 0 else (b, a)
        for i in range(32):
            for j in range(32):
                f, h = (i, j) if stage == 0 else (j, i)
                p = pos[h]
                sign = d8.signed_bytes(hot[h][p // 4])[p % 4]
                assert d8.signed32(tile[32 * i + j]) == sign * d8.signed_bytes(full[f][p // 4])[p % 4]
    assert len(rotations) > 4                                       # the rotation moves with the nonce


def test_stage_3_returns_c_and_the_product_stages_mix_signs():
    for nw in WAVE_NONCES[:4]:
        _, _, c3 = d8.operands(3, nw)
        assert d8.expected_tile(3, nw) == tuple(w for row in c3 for w in row)
        for stage in (2, 4):
            a, b, c = d8.operands(stage, nw)
            dim = d8.DIM[stage]
            tile = d8.expected_tile(stage, nw)
            grew = shrank = 0
            for i in range(dim):
                for j in range(dim):
                    cv, dv = d8.signed32(c[i][j]), d8.signed32(tile[dim * i + j])
                    assert abs(cv) <= 2 ** 30
                    grew += abs(dv) > abs(cv)
                    shrank += abs(dv) < abs(cv)
            assert grew > dim * dim // 8 and shrank > dim * dim // 8, (stage, grew, shrank)


def test_the_image_tells_every_wrong_kernel_model_apart():
    want = ["16x16 tile stored with the 32x32 row formula", "A's K-blocks swapped against B's", "C dropped",
            "bytes unsigned", "dwords of A reversed within a block", "transposed store"]
    for nonce in dp.NONCES:
        good = d8.tiles_image(nonce, GRID)
        models = d8.wrong_kernel_models(nonce, GRID)
        assert sorted(models) == want
        for name, image in models.items():
            assert image.shape == good.shape
            for wg in range(GRID):
                assert (image[wg] != good[wg]).sum() > 100, (name, hex(nonce), wg)
            v = d8.verdict(d8.healthy(GRID, nonce)[0], image, GRID, nonce)
            assert not v["ok"] and v["records_ok"] == 0, (name, v)


@pytest.mark.parametrize("bit", range(32))
def test_reference_verdict_fails_every_stuck_bit(bit):
    recs, tiles = d8.healthy(1, 0xDEADBEEF)
    for value in (0, 1):
        v = d8.verdict(recs, d8.stuck_bit(tiles, bit, value), 1, 0xDEADBEEF)
        assert not v["ok"] and v["tile_bad"] > 0 and v["first_bad_xor"] == 1 << bit, (bit, value, v)


def test_accumulator_elements_cover_each_tile_once():
    for stage in range(d8.STAGES):
        seen = sorted(d8.accumulator_element(stage, lane, reg) for lane in range(64)
                      for reg in range(d8.ACC_REGS[stage]))
        dim = d8.DIM[stage]
        assert seen == [(i, j) for i in range(dim) for j in range(dim)]


def test_injection_image_changes_one_counter_and_at_most_one_word():
    nonce = 7
    good = d8.tiles_image(nonce, GRID)
    for stage in range(d8.STAGES):
        for wave in range(4):
            inj = {"kind": "mfma", "wg": 1, "wave": wave, "lane": 37, "index": stage * 16 + 2, "mask": 0x80000001}
            bad, tiles = d8.injection_image(nonce, GRID, inj)
            assert bad.sum() == 1 and bad[1, stage] == 1
            diff = np.argwhere(tiles != good)
            assert len(diff) == (1 if wave == 0 else 0)
            if wave == 0:
                i, j = d8.accumulator_element(stage, 37, 2)
                assert tuple(diff[0]) == (1, d8.TILE_OFFSET[stage] + i * d8.DIM[stage] + j)
    # an index that names no register of its stage does nothing
    for index in (4 * 16 + 4, 5 * 16, 1000):
        inj = {"kind": "mfma", "wg": 1, "wave": 0, "lane": 0, "index": index, "mask": 1}
        bad, tiles = d8.injection_image(nonce, GRID, inj)
        assert bad.sum() == 0 and (tiles == good).all()
    bad, tiles = d8.injection_image(nonce, GRID, None)
    assert bad.sum() == 0 and (tiles == good).all()

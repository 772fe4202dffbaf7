"""The MFMA datapath check's recipe, on the independent reference alone
(testing/datapath_reference.py), CPU only, in exact rational arithmetic:
every stage is exact in both k orders, no output word is zero, and the operand
and result words toggle all 32 bits for every nonce."""
import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import datapath_reference as dp
from rocm_k8s_device_plugin_amd.testing import kernel_reference as ref

WAVE_NONCES = sorted({dp.wave_nonce(n, wg, wave) for n in dp.NONCES for wg, wave in dp.WG_WAVES})


def test_the_cases_cover_the_issue_nonces_and_more_than_one_wave():
    assert dp.NONCES == (0, 1, 6, 7, 12345, 0xDEADBEEF, 0xFFFFFFF9, 0xFFFFFFFF)
    assert len(dp.WG_WAVES) >= 2 and len(WAVE_NONCES) == len(dp.NONCES) * len(dp.WG_WAVES)
    assert dp.wave_nonce(0xFFFFFFFF, 0, 1) < 0xFFFFFFFF            # wraps at 2^32


@pytest.mark.parametrize("stage", range(dp.STAGES))
def test_every_product_and_partial_sum_is_a_normal_fp32_in_both_k_orders(stage):
    for nw in WAVE_NONCES:
        assert dp.exactness_violations(stage, nw) == [], f"wave nonce {nw:#x}"


def test_the_codec_refuses_what_fp32_cannot_hold_exactly():
    from fractions import Fraction
    assert dp.encode(Fraction(1)) == 0x3F800000 and dp.decode(0xBF800000) == -1
    assert dp.encode(Fraction(2 ** 24 - 1)) == 0x4B7FFFFF
    for bad in (Fraction(2 ** 24 + 1), Fraction(1, 3), Fraction(2) ** -127, Fraction(2) ** 128):
        assert not dp.is_normal(bad)
    for w in (0x00000001, 0x7F800000, 0x7FC00000):
        with pytest.raises(AssertionError):
            dp.decode(w)


def test_no_output_word_is_zero_and_none_is_special():
    for nw in WAVE_NONCES:
        for stage in range(dp.STAGES):
            t = np.array(dp.expected_tile(stage, nw), dtype=np.uint32)
            field = t >> 23 & 0xFF
            assert ((field >= 1) & (field <= 254)).all(), (stage, nw)


def test_operand_and_result_words_toggle_all_32_bits():
    for nw in WAVE_NONCES:
        assert dp.toggle_masks(nw) == {"A": 0xFFFFFFFF, "B": 0xFFFFFFFF, "C": 0xFFFFFFFF, "D": 0xFFFFFFFF}, hex(nw)


def test_stage_2_sums_stay_below_2_to_24_at_one_scale_and_cancel():
    """The accumulate adder sees both effective additions and subtractions."""
    for nw in WAVE_NONCES[:4]:
        a, b, c = dp.operands(2, nw)
        grew = shrank = 0
        for i in range(dp.ROWS):
            for j in range(dp.COLS):
                scale = dp._scale(nw, dp.SEL_ROW, i) * dp._scale(nw, dp.SEL_COL, j)
                terms = [dp.decode(c[i][j]) / scale] + [dp.decode(a[i][k]) * dp.decode(b[k][j]) / scale
                                                        for k in range(dp.DEPTH)]
                assert all(t.denominator == 1 for t in terms)
                assert abs(terms[0]) < 2 ** 22 and abs(terms[1]) < 2 ** 22 and abs(terms[2]) < 2 ** 22
                assert 0 < abs(sum(terms)) < 2 ** 24
                grew += abs(sum(terms)) > abs(terms[0])
                shrank += abs(sum(terms)) < abs(terms[0])
        assert grew > 100 and shrank > 100, (grew, shrank)


def test_todays_probe_passes_a_stuck_low_bit_and_the_datapath_verdict_does_not():
    """The gap this check closes: bit 0 stuck at 0 in every output word leaves
    the liveness tile (small integers) unchanged for every nonce and iteration
    count of its tests, so the probe and the sweep pass; the datapath tiles change."""
    for nonce in ref.NONCES:
        for iters in (1, 4, 64):
            t = ref.tile_f32(nonce, iters)
            stuck = (t.view(np.uint32) & np.uint32(0xFFFFFFFE)).view(np.float32)
            assert (stuck.view(np.uint32) == t.view(np.uint32)).all()
    for nonce in dp.NONCES:
        recs, tiles = dp.healthy(2, nonce)
        v = dp.verdict(recs, dp.stuck_bit(tiles, 0, 0), 2, nonce)
        assert not v["ok"] and v["first_bad_xor"] == 1 and v["tile_bad"] > 1000


@pytest.mark.parametrize("bit", range(32))
def test_reference_verdict_fails_every_stuck_bit(bit):
    recs, tiles = dp.healthy(1, 0xDEADBEEF)
    for value in (0, 1):
        v = dp.verdict(recs, dp.stuck_bit(tiles, bit, value), 1, 0xDEADBEEF)
        assert not v["ok"] and v["first_bad_xor"] == 1 << bit, (bit, value, v)

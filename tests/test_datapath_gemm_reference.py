"""The bf16 GEMM pipeline check's reference against exact Fractions, and the conditions on the operands that make
every D word exact in any summation order and chain split (datapath_gemm_kernel.h)."""
from fractions import Fraction

import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import datapath_gemm_reference as db

NONCES = (0xFFFFFFFF, 0xDEADBEEF)


def _bf16(code):
    field = code >> 7 & 0xFF
    assert 0 < field < 255, hex(code)                                    # no zero, subnormal, Inf or NaN
    return (-1) ** (code >> 15) * Fraction(128 + (code & 0x7F)) * Fraction(2) ** (field - 134)


def _f32(word):
    assert 0 < word >> 23 & 0xFF < 255, hex(word)
    return (-1) ** (word >> 31) * Fraction((1 << 23) + (word & 0x7FFFFF)) * Fraction(2) ** ((word >> 23 & 0xFF) - 150)


@pytest.mark.parametrize("nonce", NONCES)
def test_bands_alternation_bit_coverage_bound_and_odd_sum(nonce):
    ks, K = db.KSTEPS_MAX, db.KSTEPS_MAX * db.KSTEP
    a, b = db.a_elements(nonce, 1, ks), db.b_elements(nonce, ks).T        # both [row or column][k]
    fields = (db.exp_fields(db.wg_seed(nonce, 1), db.SPACE_EA), db.exp_fields(nonce, db.SPACE_EB))
    block = np.arange(K) >> 5 & 1
    for side, (x, e) in enumerate(zip((a, b), fields)):
        assert all(int(v) in db.E_BAND for v in e)
        e = e.astype(np.int64)[:, None]
        full = (block == side)[None, :]                                  # A full in the even blocks, B in the odd
        assert ((x >> 7 & 0xFF) == np.where(full, e, e - 4)).all()
        assert ((x & 1) == full).all() and ((x & 0x1F)[:, block != side] == 0x10).all()   # m and m' odd
        # along every row (column of B) the sign and the seven mantissa bits take both values; the exponent field
        # of one row is E or E - 4 only, so its bits 0 and 1 are fixed there: all 16 bits toggle over the panel
        assert ((np.bitwise_or.reduce(x, axis=1) & ~np.bitwise_and.reduce(x, axis=1)) & 0x807F == 0x807F).all()
        assert int(np.bitwise_or.reduce(x, axis=None) & ~np.bitwise_and.reduce(x, axis=None)) == 0xFFFF
    au, bu, g = db.units(a, fields[0][:, None]), db.units(b, fields[1][:, None]), db.ga(nonce, 1)
    assert (np.abs(au * bu[:1]) <= 255 * 15).all() and (au % 2 == 1).all() and (bu % 2 == 1).all() and (g % 2 != 0).all()
    bound = int((np.abs(au) @ np.abs(bu).T + np.abs(g)).max())            # Python integers from here
    assert bound <= K // 2 * 2 * 255 * 15 + (1 << 20) - 1 == 8_882_175 < 1 << 24
    assert (db.integers(nonce, 1, ks) % 2 != 0).all()                     # an even count of odd terms plus the odd ga


@pytest.mark.parametrize("nonce,ksteps", [(NONCES[0], 1), (NONCES[1], 3)])
def test_d_image_equals_sums_of_exact_fractions(nonce, ksteps):
    recs, tiles = db.healthy(2, nonce, ksteps)
    a, b, q, g = db.a_elements(nonce, 1, ksteps), db.b_elements(nonce, ksteps), db.qx(nonce, 1), db.ga(nonce, 1)
    for row, col in ((0, 0), (5, 127), (64, 63), (127, 64), (77, 1)):
        want = int(g[row, col]) * Fraction(2) ** int(q[row, col]) + sum(
            _bf16(int(a[row, k])) * _bf16(int(b[k, col])) for k in range(ksteps * db.KSTEP))
        assert _f32(int(tiles[1, row * 128 + col])) == want
    assert recs[1, db.REC_FOLD:db.REC_FOLD + 2].tolist() == [
        int(np.bitwise_xor.reduce(a[:64], axis=None)), sum(int(v) for v in a[:64].ravel()) & db.M32]


def test_projection_rejects_one_changed_word_anywhere_in_a_row():
    nonce, ksteps, row = NONCES[1], 2, 9
    n = db.integers(nonce, 0, ksteps)[row]
    assert db.projection_ok(n, nonce, 0, ksteps, row)
    for col in range(db.TILE):
        for delta in (1, -1, 1 << 23):
            wrong = n.copy()
            wrong[col] += delta
            assert not db.projection_ok(wrong, nonce, 0, ksteps, row), (col, delta)


def test_image_differs_from_the_wrong_kernel_models():
    nonce, ksteps = NONCES[1], 3
    right = db.integers(nonce, 0, ksteps)
    models = db.wrong_kernel_models(nonce, ksteps)
    assert sorted(models) == ["B read untransposed", "LDS buffers swapped", "halves swapped within a dword",
                              "one k-step dropped", "one k-step repeated"]
    for name, wrong in models.items():
        assert (wrong != right).mean() > 0.99, name

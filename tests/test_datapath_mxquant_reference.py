"""The MX quantise check's reference on its own: the recipe's properties at the GPU test's shapes and at production
shape, and that the healthy quantised image differs from every wrong-kernel model's."""
import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import datapath_mxquant_reference as db

SHAPES = [(1, 1, 0xFFFFFFFF), (1, 2, 0xDEADBEEF), (1, 3, 0xDEADBEEF), (2, 2, 0xFFFFFFFF), (2, db.HSTEPS, 0x5EED142F)]


@pytest.mark.parametrize("grid,hsteps,nonce", SHAPES)
def test_the_recipe_has_its_properties(grid, hsteps, nonce):
    # exact O(1) H, no zero block, scale bytes in the band and varying, the 2**24 bound of every Y word: asserted inside
    counts, codes = db.check(grid, nonce, hsteps)
    print(counts, codes.tolist())
    assert set(counts) == set(db.CLASSES) and min(counts.values()) > 0 and (np.delete(codes, 8) > 0).all()


def test_the_rule_on_hand_made_words():
    # one block, amax 28 * 2**-3 (exponent field 128): E = 126, values are S / 4
    s = np.array([[27, 1, -1, 3, 5, 7, 9, 10, 11, 14, 18, 20, 22, 24, 26, 28, -28, 2, 4, 6, 8, 12, 16, -16] + [1] * 8])
    codes, e8 = db.quantise(db.f32_words(s, np.full(s.shape, -3)))
    assert e8.tolist() == [[126]]
    assert codes[0, :24].tolist() == [7, 0, 8, 2, 2, 4, 4, 4, 5, 6, 6, 6, 7, 7, 7, 7, 15, 1, 2, 3, 4, 5, 6, 14]


@pytest.mark.parametrize("grid,hsteps,nonce", SHAPES[1:4])
def test_every_wrong_kernel_model_leaves_another_image(grid, hsteps, nonce):
    healthy = db.healthy(grid, nonce, hsteps)[1][grid - 1]
    wrong = db.wrong_images(nonce, grid - 1, hsteps)
    assert len(wrong) == len(db.MODELS) + 4
    assert {name: int((img != healthy).sum()) for name, img in wrong.items() if (img == healthy).all()} == {}

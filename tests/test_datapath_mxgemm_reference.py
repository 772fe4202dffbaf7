"""The MXFP4 GEMM pipeline check's numpy reference on its own: the exactness bound, and that the operands reach every
case the check is for."""
import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import datapath_mxgemm_reference as db


@pytest.mark.parametrize("ksteps", [1, 2, 3, 8])
def test_the_bound_holds_and_no_output_is_zero(ksteps):
    assert db.worst_case_quanta(ksteps) < 1 << 24
    n = db.integers(0xDEADBEEF, 1, ksteps)                 # asserts the magnitudes' sum below 2**24 for every output
    assert (n % 2 == 1).all() and (db.healthy(2, 0xDEADBEEF, ksteps)[1] != 0).all()


def test_every_code_delta_and_op_sel_byte_occurs():
    a, b = db.codes(7, 0, 1), db.codes(7, None, 1)
    assert set(np.unique(a)) == set(np.unique(b)) == set(range(16)) - {0, 8}      # free codes: all but +-0
    sa, sb = db.scales(7, 0, 2), db.scales(7, None, 2)
    assert set(np.unique(sa - db.scale_base(7, 0)[:, None])) == {0, 1, 2, 3}
    assert set(np.unique(sb - db.scale_base(7, None)[:, None])) == {0, 1}
    assert (sa[:, :-1] != sa[:, 1:]).any(axis=1).all()     # the scale changes inside every row
    g = db.gathered(sa)                                    # [row][step][lane group]: four op_sel bytes each
    assert g.shape == (128, 2, 2)
    for sel in range(4):                                   # byte `sel` of lane group h is block 2 * sel + h of the step
        for h in range(2):
            assert ((g[:, :, h] >> 8 * sel & 0xFF) == sa.reshape(128, 2, 8)[:, :, 2 * sel + h]).all()

"""The fused attention check's reference: S by full dot products is the three live terms and lies in -6..6, the online
recurrence keeps every l and O a whole number of quanta below 2**24 at the largest N (datapath_attn_kernel.h), and the
nonces the GPU tests use exercise both a rising and a standing running max."""
import pytest

from rocm_k8s_device_plugin_amd.testing import datapath_attn_reference as da

NONCES = (0xFFFFFFFF, 0xDEADBEEF)


@pytest.mark.parametrize("nonce", NONCES)
def test_full_dot_products_are_the_live_terms_and_lie_in_minus_6_to_6(nonce):
    s = da.scores(nonce, 1, 2, da.KBLOCKS_MAX)
    assert (s == da.live_scores(nonce, 1, 2, da.KBLOCKS_MAX)).all() and s.min() >= -6 and s.max() <= 6
    q, k = da.q_integers(nonce, 1, 2), da.k_integers(nonce, 1, da.KBLOCKS_MAX)
    assert min(abs(q).min(), abs(k).min()) >= 1 and abs(q).max() <= 4 and abs(k).max() <= 13   # exact, non-zero bf16


@pytest.mark.parametrize("nonce", NONCES)
def test_the_online_replay_holds_its_bound_at_8_key_blocks_and_ends_where_the_closed_form_does(nonce):
    s, v = da.scores(nonce, 0, 1, da.KBLOCKS_MAX), da.v_integers(nonce, 0, da.KBLOCKS_MAX)
    m, l, o, _ = da.online(s, v)                       # asserts the quantum and the 2**24 bound at every block
    want = da.state(s, v)
    assert (m == want[0]).all() and (l == want[1]).all() and (o == want[2]).all()
    assert l.max() < 1 << 21 and abs(o).max() < 1 << 23


@pytest.mark.parametrize("kblocks", (2, 3))
@pytest.mark.parametrize("nonce", NONCES)
def test_the_test_nonces_have_a_query_whose_max_rises_late_and_one_whose_max_stays(nonce, kblocks):
    rises = da.online(da.scores(nonce, 0, 1, kblocks), da.v_integers(nonce, 0, kblocks))[3]
    assert any(rises) and not all(rises), [len(r) for r in rises]

"""The split-K GEMM check's reference: its D is the GEMM pipeline check's D for the same panels at ksteps_total, every
split's partial is a whole number of quanta and all magnitudes stay below 2**24, so any arrival order is exact
(datapath_splitk_kernel.h); the ledger words are as the header defines them."""
import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import datapath_gemm_reference as dg
from rocm_k8s_device_plugin_amd.testing import datapath_splitk_reference as ds

SIZES = [(1, 1, 1), (1, 2, 2), (1, 3, 3), (2, 8, 1)]
NONCE = 0xDEADBEEF


@pytest.mark.parametrize("tiles,splits,ksteps", SIZES)
def test_d_is_the_gemm_checks_d_at_ksteps_total_and_odd(tiles, splits, ksteps):
    recs, d, led = ds.healthy(tiles, splits, ksteps, NONCE)
    assert (d == dg.healthy(tiles, NONCE, splits * ksteps)[1]).all()
    for t in range(tiles):
        assert (ds.integers(NONCE, t, splits, ksteps) % 2 != 0).all()         # odd, so never zero
    assert recs.shape == (tiles * splits, ds.REC_WORDS) and recs[:, ds.REC_MAGIC].tolist() == [0x4450534B] * (tiles * splits)


@pytest.mark.parametrize("nonce", (0xFFFFFFFF, NONCE))
def test_partials_are_whole_quanta_and_every_magnitude_stays_below_2_to_24_at_production_size(nonce):
    splits, ksteps, tile = ds.SPLITS, ds.KSTEPS, 1
    parts = [ds.partial(nonce, tile, splits, ksteps, s) for s in range(splits)]
    assert all(p.dtype == np.int64 for p in parts)                             # integers of quanta by construction
    bound = int((sum(np.abs(p) for p in parts) + np.abs(dg.ga(nonce, tile))).max())
    assert bound <= 8_882_175 < 1 << 24                                       # so C plus any subset, in any order
    assert (dg.ga(nonce, tile) + sum(parts) == dg.integers(nonce, tile, splits * ksteps)).all()
    # each partial alone is a representable addend: zero or below 2**24
    assert max(int(np.abs(p).max()) for p in parts) < 1 << 24


@pytest.mark.parametrize("tiles,splits,ksteps", SIZES)
def test_ledger_words_are_as_defined(tiles, splits, ksteps):
    t = tiles - 1
    led = ds.ledger(NONCE, t, splits, ksteps)
    a, b = dg.a_elements(NONCE, t, splits * ksteps), dg.b_elements(NONCE, splits * ksteps)
    who = 0
    for s in range(splits):
        who ^= NONCE ^ (t * splits + s)
    assert led == [splits, who, int(a.sum()) & ds.M32, int(np.bitwise_xor.reduce(a, axis=None)),
                   int(b.sum()) & ds.M32, int(np.bitwise_xor.reduce(b, axis=None)), 0, 0]
    short = ds.ledger(NONCE, t, splits, ksteps, skip=(splits - 1,))
    assert short[0] == splits - 1 and short[1] == who ^ NONCE ^ (t * splits + splits - 1)
    # a record's folds are those of its k-range: the four waves' A sums cover the part twice (two waves per row half)
    f = ds.folds(NONCE, t, splits, ksteps, 0)
    assert (f[1] + f[9]) & ds.M32 == int(a[:, ds.k_range(0, ksteps)].sum()) & ds.M32 and f[0:2] == f[4:6]

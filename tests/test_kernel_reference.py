"""The independent kernel references (testing/kernel_reference.py), CPU only:
they agree with the generators in liveness_kernel.h, they tell the right tile
from plausible wrong ones, probe_verify.h::verify_tile rejects what it must,
and the comparisons the GPU tests apply (tests/test_gpu_kernels_raw.py) fail
on the output of a wrong kernel.

The header and verify_tile are reached through native/tests/kernel_contract_cli.cpp,
a host-only program: the one the native build produced, or compiled here by
the C++ compiler (testing/contract_cli.py)."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import contract_cli
from rocm_k8s_device_plugin_amd.testing import kernel_reference as ref
from rocm_k8s_device_plugin_amd.testing import raw_kernels

REPO = Path(__file__).resolve().parent.parent
NONCES, ITERS = ref.NONCES, ref.ITERS
TILE_CASES = [(n, it) for n in NONCES for it in ITERS]


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return contract_cli.contract_cli(tmp_path_factory.mktemp("kernel_contract"))


def _gen(cli, lines):
    r = subprocess.run([str(cli), "gen"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = [int(x) for x in r.stdout.split()]
    assert len(out) == len(lines)
    return out


def _verify(cli, records):
    """records: (out float32[1024], meta uint32[4], nonce, iters) -> [(ok, mismatches, error)]"""
    blob = b"".join(struct.pack("<Ii", nonce, iters) + np.asarray(out, dtype=np.float32).tobytes()
                    + np.asarray(meta, dtype=np.uint32).tobytes() for out, meta, nonce, iters in records)
    r = subprocess.run([str(cli), "verify"], input=blob, capture_output=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(records)
    return [(int(ok), int(mism), err) for ok, mism, err in (ln.split("\t") for ln in lines)]


def _meta(nonce):
    return np.array([ref.PROBE_MAGIC, nonce, 3, 0x1234], dtype=np.uint32)


# ---- the reference's generators are the header's ---------------------------------
def test_tile_generators_agree_with_header(cli):
    lines, want = [], []
    for n in NONCES:
        for i in range(32):
            for k in range(2):
                lines.append(f"a {i} {k} {n}")
                want.append(ref.probe_a(i, k, n))
        for k in range(2):
            for j in range(32):
                lines.append(f"b {k} {j} {n}")
                want.append(ref.probe_b(k, j, n))
        for i in range(32):
            for j in range(32):
                lines.append(f"c {i} {j} {n}")
                want.append(ref.probe_c(i, j, n))
        for wg in (0, 1, 255, 0x3FFFFFFF, 0x40000000):
            for wave in range(4):
                lines.append(f"sweep_nonce {n} {wg} {wave}")
                want.append(ref.sweep_nonce(n, wg, wave))
    assert _gen(cli, lines) == want


def test_generators_wrap_at_2_to_32():
    """With nonce 0xFFFFFFF9 the sum i*3 + k*5 + nonce passes 2^32 for most
    (i, k): a reference without the wrap would produce other operands."""
    n = 0xFFFFFFF9
    no_wrap = [(i * 3 + k * 5 + n) % 7 - 3 for i in range(32) for k in range(2)]
    assert [ref.probe_a(i, k, n) for i in range(32) for k in range(2)] != no_wrap
    assert ref.sweep_nonce(0xFFFFFFFF, 1, 1) == 4


def test_sweep_lds_pattern_agrees_with_header(cli):
    words = list(range(64)) + list(range(ref.SWEEP_LDS_WORDS - 64, ref.SWEEP_LDS_WORDS))
    cases = [(i, n, wg) for n in (0, 0xDEADBEEF, 0xFFFFFFFF) for wg in (0, 1, 255) for i in words]
    got = _gen(cli, [f"lds {i} {n} {wg}" for i, n, wg in cases])
    assert got == [ref.sweep_lds_pattern(i, n, wg) for i, n, wg in cases]


def test_burn_bf16_bits_agree_with_header(cli):
    cases = [(lane, j, n) for n in ref.BURN_NONCES + (12345,) for lane in range(64) for j in range(32)]
    got = _gen(cli, [f"burn {lane} {j} {n}" for lane, j, n in cases])
    assert got == [ref.burn_bf16_bits(lane, j, n) for lane, j, n in cases]


def test_burn_operands_lie_in_the_documented_range():
    for n in ref.BURN_NONCES:
        mags = np.concatenate([np.abs(m).ravel() for m in ref.burn_operands(n)])
        assert mags.min() >= 2.0 ** -7 and mags.max() < 1.0
    assert max(np.abs(m).max() for m in ref.burn_operands(0)) > 0.5      # not the +-[2^-7, 2^-1) once documented


def test_hbm_pattern_agrees_with_header(cli):
    """The fold of the index's high word is reached in production above 16 GiB,
    a size no GPU test can run in seconds: checked here instead."""
    words = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 34 - 1]
    cases = [(w, s) for s in (0, 1, 0xFFFFFFFF) for w in words]
    got = _gen(cli, [f"hbm {w} {s}" for w, s in cases])
    assert got == [ref.hbm_pattern(w, s) for w, s in cases]
    assert ref.hbm_pattern(2 ** 32, 0) != ref.hbm_pattern(0, 0)           # the high word counts
    for first in (0, 2 ** 32 - 3):                                         # the array form is the scalar form
        assert ref.hbm_pattern_words(8, 7, first).tolist() == [ref.hbm_pattern(first + i, 7) for i in range(8)]


def test_arg_struct_layout_equals_the_ctypes_mirrors(cli):
    r = subprocess.run([str(cli), "layout"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = {}
    for ln in r.stdout.splitlines():
        s, f, v = ln.split()
        got.setdefault(s, []).append((f, int(v)))
    want = {}
    for name, cls in raw_kernels.ARG_STRUCTS.items():
        want[name] = [(f, getattr(cls, f).offset) for f, _ in cls._fields_] + [("sizeof", __import__("ctypes").sizeof(cls))]
    assert got == want
    assert dict(got["mi355x_liveness_args"])["sizeof"] == 32


# ---- discrimination, on the reference alone --------------------------------------
@pytest.mark.parametrize("iters", ITERS)
def test_tile_is_exact_in_fp32_and_differs_from_every_wrong_kernel_model(iters):
    for nonce in NONCES:
        t = ref.tile(nonce, iters)
        assert np.abs(t).max() < 1 << 24
        assert (t.astype(np.float32).astype(np.int64) == t).all()
        models = ref.wrong_tile_models(nonce, iters)
        assert len(models) == 8
        for name, wrong in models.items():
            assert int((wrong != t).sum()) >= 675, (name, nonce, iters)


def test_scratch_image_is_the_register_layout():
    t = ref.tile_f32(12345, 4)
    img = ref.scratch_image(t)
    assert img.shape == (16, 64) and img.dtype == np.float32
    # every tile element appears exactly once: rebuild the tile from the image
    back = np.full((32, 32), np.nan, dtype=np.float32)
    for r in range(16):
        for lane in range(64):
            back[(r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), lane & 31] = img[r, lane]
    assert (back == t).all()
    assert img[5, 40] == t[1 + 8 + 4, 8]


def test_burn_checksum_tolerance_is_meaningful():
    """Wrong fragment layouts and one iteration more lie at least 100 x bound
    from the reference, 25 times the accepted margin. (Nonce 12345 is not a
    burn test nonce: its checksum is near zero, iters+1 comes within 2 x bound
    of the accepted band.)"""
    for nonce in ref.BURN_NONCES:
        for iters in ref.BURN_ITERS:
            checksum, abs_sum = ref.burn_checksum(nonce, iters)
            bound = ref.burn_bound(iters, abs_sum)
            assert 0 < bound < 1e-3 * abs_sum
            models = ref.wrong_burn_models(nonce, iters)
            assert len(models) == 3
            for name, wrong in models.items():
                assert abs(wrong - checksum) >= 100 * bound, (name, nonce, iters)
    c1, s1 = ref.burn_checksum(1, 1)
    c3, s3 = ref.burn_checksum(1, 3)
    assert c3 == pytest.approx(3 * c1, rel=1e-12) and s3 == pytest.approx(3 * s1, rel=1e-12)


# ---- verify_tile -----------------------------------------------------------------
def test_verify_tile_accepts_the_reference_tile(cli):
    res = _verify(cli, [(ref.tile_f32(n, it), _meta(n), n, it) for n, it in TILE_CASES])
    assert res == [(1, 0, "")] * len(TILE_CASES)


@pytest.mark.parametrize("iters", ITERS)
def test_verify_tile_rejects_every_single_bit_flip(cli, iters):
    """All 32 bits, the sign of a zero element included (-0.0 == 0.0 as floats)."""
    records, which = [], []
    for nonce in NONCES:
        good = ref.tile_f32(nonce, iters).ravel().view(np.uint32)
        for word in (0, 17, 511, 1023):
            for bit in range(32):
                bits = good.copy()
                bits[word] ^= np.uint32(1 << bit)
                records.append((bits.view(np.float32), _meta(nonce), nonce, iters))
                which.append((nonce, word, bit))
    for who, (ok, mism, err) in zip(which, _verify(cli, records)):
        assert (ok, mism) == (0, 1) and "1/1024" in err, (who, ok, mism, err)


def test_verify_tile_rejects_a_negative_zero(cli):
    """The first +0.0 element of every tile that has one, with its sign flipped."""
    records = []
    for n, it in TILE_CASES:
        bits = ref.tile_f32(n, it).ravel().view(np.uint32).copy()
        zeros = np.flatnonzero(bits == 0)
        if zeros.size:
            bits[zeros[0]] = 0x80000000
            records.append((bits.view(np.float32), _meta(n), n, it))
    assert len(records) >= 10
    for ok, mism, err in _verify(cli, records):
        assert (ok, mism) == (0, 1), (ok, mism, err)


def test_verify_tile_rejects_every_wrong_kernel_model(cli):
    records, names = [], []
    for n, it in TILE_CASES:
        for name, wrong in ref.wrong_tile_models(n, it).items():
            records.append((wrong.astype(np.float32), _meta(n), n, it))
            names.append((name, n, it))
    for who, (ok, mism, err) in zip(names, _verify(cli, records)):
        assert ok == 0 and mism >= 675 and "differ" in err, (who, ok, mism, err)


def test_verify_tile_rejects_wrong_iters_and_wrong_meta(cli):
    records, kinds = [], []
    for n, it in TILE_CASES:
        t = ref.tile_f32(n, it)
        records += [(t, _meta(n), n, it + 1), (t, _meta(n), n, it - 1)]
        kinds += ["iters", "iters"]
        bad_magic = _meta(n)
        bad_magic[ref.META_MAGIC] ^= 1
        bad_nonce = _meta(n)
        bad_nonce[ref.META_NONCE] ^= 0x80000000
        records += [(t, bad_magic, n, it), (t, bad_nonce, n, it)]
        kinds += ["meta", "meta"]
    for kind, (ok, mism, err) in zip(kinds, _verify(cli, records)):
        if kind == "iters":
            assert ok == 0 and mism > 0 and "differ" in err, (ok, mism, err)
        else:
            assert ok == 0 and mism == 0 and err.startswith("meta mismatch"), (ok, mism, err)


# ---- the GPU tests' comparisons fail on a wrong kernel's output ----------------------
def _good_liveness(nonce, iters):
    t = ref.tile_f32(nonce, iters)
    return t.copy(), ref.scratch_image(t), _meta(nonce)


def test_check_liveness_accepts_the_reference_output():
    for n, it in TILE_CASES:
        ref.check_liveness(*_good_liveness(n, it), n, it)


@pytest.mark.parametrize("model", ["transposed_output", "iters_plus_1", "half_wave_rows_swapped", "only_k0",
                                   "c_dropped"])
def test_check_liveness_fails_on_wrong_kernel_models(model):
    for n, it in TILE_CASES:
        out, scratch, meta = _good_liveness(n, it)
        wrong = ref.wrong_tile_models(n, it)[model].astype(np.float32)
        with pytest.raises(AssertionError, match="out: "):
            ref.check_liveness(wrong, scratch, meta, n, it)
        # the same wrong accumulators left in scratch, the tile repaired on the way out
        with pytest.raises(AssertionError, match="scratch: "):
            ref.check_liveness(out, ref.scratch_image(wrong), meta, n, it)


def test_check_liveness_fails_on_layout_meta_and_unwritten_output():
    n, it = 35, 64
    out, scratch, meta = _good_liveness(n, it)
    with pytest.raises(AssertionError, match="scratch: "):       # slots register-major within a lane
        ref.check_liveness(out, scratch.T.copy().reshape(16, 64), meta, n, it)
    unwritten = out.copy()
    unwritten.view(np.uint32)[31, 31] = 0xFFFFFFFF                 # one element left at the prefill
    with pytest.raises(AssertionError, match="out: 1/1024"):
        ref.check_liveness(unwritten, scratch, meta, n, it)
    neg_zero = out.copy()
    zeros = np.argwhere(out == 0)
    assert len(zeros)
    neg_zero[tuple(zeros[0])] = -0.0                               # equal as floats, not as bits
    with pytest.raises(AssertionError, match="out: 1/1024"):
        ref.check_liveness(neg_zero, scratch, meta, n, it)
    for word, value in ((ref.META_MAGIC, 0), (ref.META_NONCE, n + 1), (ref.META_XCC, 8)):
        m = meta.copy()
        m[word] = value
        with pytest.raises(AssertionError, match="meta"):
            ref.check_liveness(out, scratch, m, n, it)


def _good_sweep(nonce, iters, grid=4):
    recs = np.zeros((grid, 16), dtype=np.uint32)
    for wg in range(grid):
        recs[wg, [ref.REC_MAGIC, ref.REC_NONCE, ref.REC_WG, ref.REC_ARRIVED]] = [ref.SWEEP_MAGIC, nonce ^ wg, wg, grid]
        recs[wg, [ref.REC_T0_LO, ref.REC_T0_HI, ref.REC_T1_LO, ref.REC_T1_HI]] = [0xFFFFFFF0, 1, 5, 2]
    tiles = np.stack([ref.tile_f32(ref.sweep_nonce(nonce, wg, 0), iters) for wg in range(grid)])
    return recs, tiles


def test_check_sweep_on_reference_and_wrong_outputs():
    n, it = 0xFFFFFFFF, 4
    recs, tiles = _good_sweep(n, it)
    ref.check_sweep(recs, tiles, n, it, 4)
    bad = tiles.copy()
    bad[2] = bad[2].T                                          # a transposed store in one workgroup
    with pytest.raises(AssertionError, match="wg 2 tile"):
        ref.check_sweep(recs, bad, n, it, 4)
    bad = tiles.copy()
    bad[1] = ref.tile_f32(ref.sweep_nonce(n, 1, 1), it)       # wave 1's tile in wave 0's place
    with pytest.raises(AssertionError, match="wg 1 tile"):
        ref.check_sweep(recs, bad, n, it, 4)
    with pytest.raises(AssertionError, match="tile"):
        ref.check_sweep(recs, tiles, n, it + 1, 4)
    for word, value in ((ref.REC_MAGIC, 0), (ref.REC_WG, 0), (ref.REC_NONCE, n), (ref.REC_MFMA_BAD, 1),
                        (ref.REC_LDS_BAD, 1), (ref.REC_ARRIVED, 0), (ref.REC_ARRIVED, 5), (ref.REC_T1_HI, 1)):
        r = recs.copy()
        r[3, word] = value
        with pytest.raises(AssertionError, match="wg 3"):
            ref.check_sweep(r, tiles, n, it, 4)


def test_check_hbm_fill_and_check_on_reference_and_wrong_outputs():
    n16, seed = 4 * 768 * 2 + 768 + 5, 0xFFFFFFFF
    img = ref.hbm_fill_image(n16, seed)
    assert img[:5].tolist() == [ref.hbm_pattern(w, seed) for w in range(5)]
    ref.check_hbm_fill(img, n16, seed)
    poisoned = ref.hbm_fill_image(n16, seed, n16 - 1)
    assert np.flatnonzero(poisoned != img).tolist() == [4 * (n16 - 1)]
    assert int(poisoned[-4]) == int(img[-4]) ^ 0xFFFFFFFF
    ref.check_hbm_fill(poisoned, n16, seed, n16 - 1)
    with pytest.raises(AssertionError, match="buf: 1/"):
        ref.check_hbm_fill(poisoned, n16, seed)                      # poison where none was asked for
    with pytest.raises(AssertionError, match="buf: 1/"):
        ref.check_hbm_fill(img, n16, seed, 0)                        # the poison not written
    skipped = img.copy()
    skipped[-4:] = 0x5A5A5A5A                                        # the last unit never written
    with pytest.raises(AssertionError, match="buf: 4/"):
        ref.check_hbm_fill(skipped, n16, seed)
    with pytest.raises(AssertionError, match="buf: "):
        ref.check_hbm_fill(ref.hbm_fill_image(n16, 0), n16, seed)    # the seed ignored

    none = np.array([0], np.uint32), np.array([ref.M64], np.uint64)
    ref.check_hbm_check(*none, [])
    ref.check_hbm_check(np.array([5], np.uint32), np.array([7], np.uint64), [(9, 0), (7, 1), (7, 2), (7, 3), (7, 0)])
    with pytest.raises(AssertionError, match="bad 0"):
        ref.check_hbm_check(*none, [(3, 0)])                         # a remainder unit never read
    with pytest.raises(AssertionError, match="bad 1, want 4"):
        ref.check_hbm_check(np.array([1], np.uint32), np.array([3], np.uint64), [(3, w) for w in range(4)])
    with pytest.raises(AssertionError, match="first_bad"):           # a max where a min belongs
        ref.check_hbm_check(np.array([2], np.uint32), np.array([9], np.uint64), [(9, 0), (7, 1)])
    with pytest.raises(AssertionError, match="first_bad"):           # only the low word of first_bad updated
        ref.check_hbm_check(np.array([1], np.uint32), np.array([0xFFFFFFFF00000007], np.uint64), [(7, 1)])


def _good_burn(nonce, iters, grid=2, checksum=None):
    recs = np.zeros((grid, 16), dtype=np.uint32)
    value = ref.burn_checksum(nonce, iters)[0] if checksum is None else checksum
    for wg in range(grid):
        recs[wg, [ref.PREC_MAGIC, ref.PREC_WG, ref.PREC_NONCE]] = [ref.PERF_MAGIC, wg, nonce ^ wg]
        recs[wg, [ref.PREC_RT0_LO, ref.PREC_RT1_LO, ref.PREC_CYC_LO]] = [100, 100, 40]
        recs[wg, ref.PREC_SUM:ref.PREC_SUM + 4] = np.array([value] * 4, dtype=np.float32).view(np.uint32)
    counters = np.array([1, 2, 3, 4], dtype=np.uint32)
    return recs, counters.copy(), counters


def test_check_burn_on_reference_and_wrong_outputs():
    for nonce in ref.BURN_NONCES:
        for iters in ref.BURN_ITERS:
            # the reference rounded to fp32 is well inside the band (half an ulp of a sum of ~1000 terms)
            assert ref.check_burn(*_good_burn(nonce, iters), nonce, iters, 2) < 0.1
            for name, wrong in ref.wrong_burn_models(nonce, iters).items():
                with pytest.raises(AssertionError, match="x bound"):
                    ref.check_burn(*_good_burn(nonce, iters, checksum=wrong), nonce, iters, 2)
            with pytest.raises(AssertionError, match="x bound"):
                ref.check_burn(*_good_burn(nonce, iters, checksum=float("nan")), nonce, iters, 2)
    n, it = 1, 2
    recs, host, dev = _good_burn(n, it)
    one_wave = recs.copy()
    one_wave[1, ref.PREC_SUM + 2] ^= 1                              # one wave, one bit
    with pytest.raises(AssertionError, match="checksums differ"):
        ref.check_burn(one_wave, host, dev, n, it, 2)
    with pytest.raises(AssertionError, match="hbm_counters_host"):
        ref.check_burn(recs, np.array([1, 2, 3, 0], np.uint32), dev, n, it, 2)
    for word, value in ((ref.PREC_MAGIC, 0), (ref.PREC_WG, 0), (ref.PREC_NONCE, n), (ref.PREC_RT1_LO, 99),
                        (ref.PREC_CYC_LO, 0)):
        r = recs.copy()
        r[1, word] = value
        with pytest.raises(AssertionError, match="wg 1"):
            ref.check_burn(r, host, dev, n, it, 2)


def test_check_canaries():
    fill = raw_kernels.CANARY_FILL
    good = np.full((2, raw_kernels.CANARY_BYTES), fill, dtype=np.uint8)
    ref.check_canaries({"x.out": good}, fill)
    for where in ((0, raw_kernels.CANARY_BYTES - 1), (1, 0)):       # the byte before, the byte after
        hit = good.copy()
        hit[where] = 0
        with pytest.raises(AssertionError, match="x.out: 1 guard bytes"):
            ref.check_canaries({"x.out": hit}, fill)
    with pytest.raises(AssertionError):
        ref.check_canaries({}, fill)

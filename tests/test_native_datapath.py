"""datapath_kernel.h and datapath_verify.h against the independent reference
(testing/datapath_reference.py), CPU only, through the host-only program
native/tests/datapath_contract_cli.cpp: the generators word for word, the
argument struct against its ctypes mirror, and the shipped verdict on the
reference image with stuck bits, single flips, wrong-kernel models and wrong
records."""
import ctypes
import subprocess

import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import datapath_reference as dp
from rocm_k8s_device_plugin_amd.testing import raw_kernels

GRID = 3
NONCE = 0xDEADBEEF


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return dp.contract_cli(tmp_path_factory.mktemp("datapath_contract"))


def _gen(cli, lines):
    r = subprocess.run([str(cli), "gen"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = [int(x) for x in r.stdout.split()]
    assert len(out) == len(lines)
    return out


def test_generators_agree_with_header_word_for_word(cli):
    lines, want = [], []
    for n in dp.NONCES:
        for wg, wave in dp.WG_WAVES + ((0x3FFFFFFF, 2), (0x40000000, 3)):
            lines.append(f"wave_nonce {n} {wg} {wave}")
            want.append(dp.wave_nonce(n, wg, wave))
        for wg, wave in dp.WG_WAVES[:2]:
            nw = dp.wave_nonce(n, wg, wave)
            for stage in range(dp.STAGES):
                a, b, c = dp.operands(stage, nw)
                for i in range(32):
                    for k in range(2):
                        lines.append(f"a {stage} {i} {k} {nw}")
                        want.append(a[i][k])
                for k in range(2):
                    for j in range(32):
                        lines.append(f"b {stage} {k} {j} {nw}")
                        want.append(b[k][j])
                for i in range(32):
                    for j in range(32):
                        lines.append(f"c {stage} {i} {j} {nw}")
                        want.append(c[i][j])
    assert _gen(cli, lines) == want


def test_layout_equals_the_ctypes_mirror_and_the_reference_constants(cli):
    r = subprocess.run([str(cli), "layout"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    structs, defines = {}, {}
    for ln in r.stdout.splitlines():
        s, f, v = ln.split()
        if s == "define":
            defines[f] = int(v)
        else:
            structs.setdefault(s, []).append((f, int(v)))
    want = {name: [(f, getattr(cls, f).offset) for f, _ in cls._fields_] + [("sizeof", ctypes.sizeof(cls))]
            for name, cls in raw_kernels.DATAPATH_ARG_STRUCTS.items()}
    assert structs == want
    assert dict(structs["mi355x_datapath_args"])["sizeof"] == 24
    assert "mi355x_datapath_args" not in raw_kernels.ARG_STRUCTS       # that dict mirrors liveness_kernel.h only
    assert defines == {"MI355X_DP_THREADS": dp.THREADS, "MI355X_DP_STAGES": dp.STAGES,
                       "MI355X_DP_WG_WORDS": dp.WG_WORDS, "MI355X_DP_REC_WORDS": dp.REC_WORDS,
                       "MI355X_DP_MAGIC": dp.MAGIC, "MI355X_DPREC_MAGIC": dp.REC_MAGIC, "MI355X_DPREC_WG": dp.REC_WG,
                       "MI355X_DPREC_NONCE": dp.REC_NONCE, "MI355X_DPREC_XCC": dp.REC_XCC,
                       "MI355X_DPREC_HWID": dp.REC_HWID, "MI355X_DPREC_BAD": dp.REC_BAD}


def _patches(good, changed):
    """The word replacements that turn the tile image `good` into `changed`."""
    g, c = np.asarray(good).ravel(), np.asarray(changed).ravel()
    return [(dp.TILES, int(i), int(c[i])) for i in np.flatnonzero(g != c)]


def _apply(recs, tiles, patches):
    arrays = [np.array(recs, dtype=np.uint32).ravel(), np.array(tiles, dtype=np.uint32).ravel()]
    for arr, idx, val in patches:
        arrays[arr][idx] = val & 0xFFFFFFFF
    return arrays


def _check(cli, recs, tiles, grid, nonce, variants):
    """Every variant through the shipped verdict, each equal to the reference verdict field by field."""
    names = list(variants)
    got = dp.verdicts(cli, [dp.case(recs, tiles, grid, nonce, [variants[n] for n in names])], 1 + len(names))
    dp.assert_verdict(got[0], dp.verdict(recs, tiles, grid, nonce), "as given")
    out = {}
    for name, g in zip(names, got[1:]):
        r, t = _apply(recs, tiles, variants[name])
        dp.assert_verdict(g, dp.verdict(r, t, grid, nonce), str(name))
        out[name] = g
    return got[0], out


@pytest.mark.parametrize("nonce", dp.NONCES)
def test_healthy_image_passes_and_reports_coverage(cli, nonce):
    recs, tiles = dp.healthy(GRID, nonce, placement=[(0, 5), (1, 5), (1, 6)])
    good, _ = _check(cli, recs, tiles, GRID, nonce, {})
    assert good["ok"] is True and good["records_ok"] == GRID and good["tile_bad"] == 0 and good["error"] == ""
    assert (good["cus_covered"], good["simds_covered"], good["xccs_covered"]) == (3, 12, 2)
    assert good["first_bad_stage"] == -1 and good["first_bad_xor"] == 0


def test_every_stuck_bit_fails_the_shipped_verdict(cli):
    recs, tiles = dp.healthy(GRID, NONCE)
    variants = {(bit, value): _patches(tiles, dp.stuck_bit(tiles, bit, value)) for bit in range(32) for value in (0, 1)}
    assert all(variants.values())                       # every stuck bit changes some word
    _, got = _check(cli, recs, tiles, GRID, NONCE, variants)
    for (bit, value), g in got.items():
        assert g["ok"] is False and g["first_bad_xor"] == 1 << bit, (bit, value, g)
        assert f"(bit {bit})" in g["error"] and "stage 0" in g["error"]


def test_one_flipped_bit_is_one_bad_word_with_its_xor(cli):
    recs, tiles = dp.healthy(GRID, NONCE)
    flat = tiles.ravel()
    variants = {}
    for bit in range(32):
        wg, stage, word = bit % GRID, bit % dp.STAGES, (bit * 37 + 5) % dp.TILE_WORDS
        idx = wg * dp.WG_WORDS + stage * dp.TILE_WORDS + word
        variants[(bit, wg, stage, word)] = [(dp.TILES, idx, int(flat[idx]) ^ 1 << bit)]
    _, got = _check(cli, recs, tiles, GRID, NONCE, variants)
    for (bit, wg, stage, word), g in got.items():
        assert g["ok"] is False and g["tile_bad"] == 1 and g["records_ok"] == GRID - 1
        assert g["first_bad_xor"] == 1 << bit
        assert (g["first_bad_wg"], g["first_bad_stage"], g["first_bad_word"]) == (wg, stage, word)
        assert f"wg {wg} stage {stage} word {word} xor 0x{1 << bit:08x} (bit {bit})" in g["error"]


def test_wrong_kernel_models_fail(cli):
    recs, tiles = dp.healthy(GRID, NONCE)
    models = dp.wrong_kernel_models(NONCE, GRID)
    assert sorted(models) == ["C omitted", "half-waves exchanged", "k operands crossed", "second k term dropped",
                              "stages in another order", "transposed store"]
    _, got = _check(cli, recs, tiles, GRID, NONCE, {n: _patches(tiles, t) for n, t in models.items()})
    for name, g in got.items():
        assert g["ok"] is False and g["records_ok"] == 0 and g["tile_bad"] > 100, (name, g)


def test_wrong_records_fail(cli):
    recs, tiles = dp.healthy(GRID, NONCE)
    r = lambda wg, word, value: [(dp.RECORDS, wg * dp.REC_WORDS + word, value)]   # noqa: E731
    variants = {
        "missing record": r(1, dp.REC_MAGIC, 0),
        "another workgroup's record": r(1, dp.REC_WG, 2),
        "wrong echoed nonce": r(2, dp.REC_NONCE, (NONCE ^ 2) + 1),
        "device bad count, stage 0": r(0, dp.REC_BAD, 1),
        "device bad count, stage 3": r(0, dp.REC_BAD + 3, 7),
    }
    _, got = _check(cli, recs, tiles, GRID, NONCE, variants)
    for name, g in got.items():
        assert g["ok"] is False and g["records_ok"] == GRID - 1 and g["tile_bad"] == 0, (name, g)
        assert g["error"].startswith(f"{GRID - 1}/{GRID} workgroups exact")
    assert got["device bad count, stage 3"]["stage_bad"] == [0, 0, 0, 7]
    assert got["device bad count, stage 3"]["mfma_bad"] == 7
    # an absent record counts for nothing: its tile is not looked at either
    both = variants["missing record"] + [(dp.TILES, dp.WG_WORDS + 9, 0)]
    _, got = _check(cli, recs, tiles, GRID, NONCE, {"missing, tile wrong too": both})
    assert got["missing, tile wrong too"]["tile_bad"] == 0


def test_unwritten_buffers_fail(cli):
    """What the host prefills (records 0, tiles 0xFF) is no verdict."""
    recs = np.zeros((GRID, dp.REC_WORDS), dtype=np.uint32)
    tiles = np.full(GRID * dp.WG_WORDS, 0xFFFFFFFF, dtype=np.uint32)
    good, _ = _check(cli, recs, tiles, GRID, NONCE, {})
    assert good["ok"] is False and good["records_ok"] == 0

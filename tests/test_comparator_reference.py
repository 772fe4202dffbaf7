"""CPU side of tests/test_gpu_comparators.py: the argument structs of the
test-only build (MI355X_TEST_INJECT) against their ctypes mirrors, the raw
launcher's handling of "code_object" / "inject", the reference images under an
injection, and that the comparisons the GPU tests apply fail on what a kernel
with a wrong comparator would write."""
import ctypes
import subprocess

import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import contract_cli
from rocm_k8s_device_plugin_amd.testing import datapath_reference as dp
from rocm_k8s_device_plugin_amd.testing import kernel_reference as ref
from rocm_k8s_device_plugin_amd.testing import raw_kernels

GRID, WG, NONCE, ITERS = 2, 1, 0xDEADBEEF, 1
INJECT_FLAG = ("-DMI355X_TEST_INJECT=1",)


def _layout(exe):
    r = subprocess.run([str(exe), "inject-layout"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    structs, defines = {}, {}
    for ln in r.stdout.splitlines():
        s, f, v = ln.split()
        if s == "define":
            defines[f] = int(v)
        else:
            structs.setdefault(s, []).append((f, int(v)))
    return structs, defines


def _mirror(structs: dict) -> dict:
    return {name: [(f, getattr(cls, f).offset) for f, _ in cls._fields_] + [("sizeof", ctypes.sizeof(cls))]
            for name, cls in structs.items()}


# ---- layout of the extended structs -------------------------------------------------------------
def test_sweep_args_of_the_inject_build_equal_the_ctypes_mirror(tmp_path):
    """The header compiled as the test-only code object is: with MI355X_TEST_INJECT."""
    structs, defines = _layout(contract_cli.compile_cli(tmp_path / "kernel_contract_cli_inject", INJECT_FLAG))
    assert structs == _mirror(raw_kernels.INJECT_ARG_STRUCTS)
    assert dict(structs["mi355x_sweep_args"])["sizeof"] == 64
    # the production fields keep their places: the extension only trails
    prod = _mirror({"mi355x_sweep_args": raw_kernels.SweepArgs})["mi355x_sweep_args"][:-1]
    assert structs["mi355x_sweep_args"][:len(prod)] == prod
    assert defines == {"MI355X_PROBE_MAX_ITERS": ref.PROBE_MAX_ITERS, "MI355X_SWEEP_THREADS": 256,
                       "MI355X_SWEEP_LDS_WORDS": ref.SWEEP_LDS_WORDS,
                       "MI355X_INJECT_NONE": raw_kernels.INJECT_KINDS["none"],
                       "MI355X_INJECT_MFMA": raw_kernels.INJECT_KINDS["mfma"],
                       "MI355X_INJECT_LDS": raw_kernels.INJECT_KINDS["lds"]}


def test_datapath_args_of_the_inject_build_equal_the_ctypes_mirror(tmp_path):
    structs, defines = _layout(dp.compile_cli(tmp_path / "datapath_contract_cli_inject", INJECT_FLAG))
    assert structs == _mirror(raw_kernels.DATAPATH_INJECT_ARG_STRUCTS)
    assert dict(structs["mi355x_datapath_args"])["sizeof"] == 48
    prod = _mirror({"mi355x_datapath_args": raw_kernels.DatapathArgs})["mi355x_datapath_args"][:-1]
    assert structs["mi355x_datapath_args"][:len(prod)] == prod
    assert defines == {"MI355X_DP_INJECT_NONE": raw_kernels.INJECT_KINDS["none"],
                       "MI355X_DP_INJECT_MFMA": raw_kernels.INJECT_KINDS["mfma"]}


def test_the_production_build_has_no_injection_fields(tmp_path):
    """Without the macro the structs are the shipped ones and `inject-layout` prints no struct."""
    for exe in (contract_cli.contract_cli(tmp_path), dp.contract_cli(tmp_path)):
        structs, defines = _layout(exe)
        assert structs == {} and defines
    assert ctypes.sizeof(raw_kernels.SweepArgs) == 40 and ctypes.sizeof(raw_kernels.DatapathArgs) == 24


# ---- the launcher's requests ---------------------------------------------------------------------
def test_launcher_packs_the_injection_words_and_refuses_what_no_build_has(tmp_path):
    ptrs = {"records": 0x1000, "tiles": 0x2000, "arrive": 0x3000}
    base = {"id": "x", "kernel": "sweep", "nonce": 7, "iters": 1, "grid": 2, "wait_ticks": 9}
    _, make, wgs = raw_kernels.plan(base, tmp_path)
    assert type(make(ptrs)) is raw_kernels.SweepArgs and wgs == 2                        # production by default
    _, make, _ = raw_kernels.plan(dict(base, code_object="inject"), tmp_path)
    off = make(ptrs)
    assert type(off) is raw_kernels.SweepInjectArgs and off.inject_kind == 0 and off.inject_mask == 0
    inj = {"kind": "lds", "wg": 1, "index": 40943, "mask": 1 << 31}
    a = raw_kernels.plan(dict(base, code_object="inject", inject=inj), tmp_path)[1](ptrs)
    assert (a.inject_kind, a.inject_wg, a.inject_index, a.inject_mask) == (2, 1, 40943, 1 << 31)
    assert (a.records, a.nonce, a.iters, a.grid, a.wait_ticks) == (0x1000, 7, 1, 2, 9)
    dpreq = {"id": "y", "kernel": "datapath", "nonce": 7, "grid": 2, "code_object": "inject",
             "inject": {"kind": "mfma", "wg": 1, "wave": 3, "lane": 63, "index": 63, "mask": 1}}
    d = raw_kernels.plan(dpreq, tmp_path)[1](ptrs)
    assert (d.inject_kind, d.inject_wg, d.inject_wave, d.inject_lane, d.inject_index, d.inject_mask) == (1, 1, 3, 63, 63, 1)
    for bad in (dict(base, inject=inj),                                                  # an injection into production
                dict(base, code_object="debug"),
                dict(dpreq, inject=dict(dpreq["inject"], kind="lds")),
                {"id": "z", "kernel": "liveness", "nonce": 1, "iters": 1, "code_object": "inject"}):
        with pytest.raises(ValueError):
            raw_kernels.plan(bad, tmp_path)[1](ptrs)


# ---- the reference images ------------------------------------------------------------------------
def test_register_layout_covers_the_tile_once():
    seen = {ref.accumulator_element(lane, r) for lane in range(64) for r in range(16)}
    assert seen == {(i, j) for i in range(32) for j in range(32)}
    assert ref.accumulator_element(0, 0) == (0, 0) and ref.accumulator_element(63, 15) == (31, 31)
    assert ref.accumulator_element(32, 0) == (4, 0) and ref.accumulator_element(31, 15) == (27, 31)
    assert dp.accumulator_element(37, 6) == ref.accumulator_element(37, 6) == (14, 5)
    # the liveness kernel's scratch image is the same statement of the layout
    t = ref.tile(NONCE, 4)
    img = ref.scratch_image(t)
    assert all(img[r, lane] == t[ref.accumulator_element(lane, r)] for r in range(16) for lane in range(64))


@pytest.mark.parametrize("wave", range(4))
def test_sweep_image_under_an_mfma_injection(wave):
    healthy = ref.sweep_tiles(NONCE, ITERS, GRID)
    inj = {"kind": "mfma", "wg": WG, "wave": wave, "lane": 37, "index": 6, "mask": 1 << 23}
    img = ref.sweep_injection_image(NONCE, ITERS, GRID, inj)
    assert img["mfma_bad"].tolist() == [0, 1] and img["lds_bad"].tolist() == [0, 0]
    diff = np.argwhere(img["tiles"].view(np.uint32) != healthy.view(np.uint32))
    if wave == 0:
        assert diff.tolist() == [[WG, 14, 5]]
        assert int(img["tiles"].view(np.uint32)[WG, 14, 5]) ^ int(healthy.view(np.uint32)[WG, 14, 5]) == 1 << 23
    else:
        assert diff.size == 0


def test_sweep_image_under_an_lds_injection_and_out_of_range():
    healthy = ref.sweep_tiles(NONCE, ITERS, GRID)
    img = ref.sweep_injection_image(NONCE, ITERS, GRID, {"kind": "lds", "wg": WG, "index": ref.SWEEP_LDS_WORDS - 1, "mask": 1})
    assert img["lds_bad"].tolist() == [0, 1] and img["mfma_bad"].tolist() == [0, 0]
    ref.assert_bit_equal(img["tiles"], healthy, "tiles")
    for nothing in (None, {"kind": "lds", "wg": WG, "index": ref.SWEEP_LDS_WORDS, "mask": 1},
                    {"kind": "mfma", "wg": WG, "wave": 1, "lane": 5, "index": 16, "mask": 1},
                    {"kind": "mfma", "wg": WG, "wave": 0, "lane": 5, "index": 3, "mask": 0},
                    {"kind": "mfma", "wg": GRID, "wave": 0, "lane": 5, "index": 3, "mask": 1}):
        img = ref.sweep_injection_image(NONCE, ITERS, GRID, nothing)
        assert not img["mfma_bad"].any() and not img["lds_bad"].any()
        ref.assert_bit_equal(img["tiles"], healthy, "tiles")


@pytest.mark.parametrize("stage", range(4))
@pytest.mark.parametrize("wave", (0, 3))
def test_datapath_image_under_an_injection(stage, wave):
    healthy = dp.tiles_image(NONCE, GRID)
    inj = {"kind": "mfma", "wg": WG, "wave": wave, "lane": 37, "index": stage * 16 + 6, "mask": 1 << 31}
    bad, tiles = dp.injection_image(NONCE, GRID, inj)
    assert bad.tolist() == [[0, 0, 0, 0], [int(s == stage) for s in range(4)]]
    diff = np.argwhere(tiles != healthy)
    assert diff.tolist() == ([[WG, stage, 14, 5]] if wave == 0 else [])
    if wave == 0:
        assert int(tiles[WG, stage, 14, 5]) ^ int(healthy[WG, stage, 14, 5]) == 1 << 31
    bad, tiles = dp.injection_image(NONCE, GRID, dict(inj, index=64))
    assert not bad.any() and (tiles == healthy).all()


# ---- the comparisons fail on what a wrong comparator writes ----------------------------------------
def _sweep_written(inject, mfma=(0, 0), lds=(0, 0)):
    """Records and tiles of a sweep whose counters are as given and whose tiles are as a correct
    kernel's under `inject` (the accumulator was spoilt whatever the comparator does)."""
    recs, _ = ref.healthy_sweep(GRID, NONCE, ITERS, ref.spread_placement(GRID, 8))
    recs[:, ref.REC_MFMA_BAD], recs[:, ref.REC_LDS_BAD] = mfma, lds
    return recs, ref.sweep_injection_image(NONCE, ITERS, GRID, inject)["tiles"]


def test_check_sweep_under_injection_fails_on_wrong_comparators():
    mfma = {"kind": "mfma", "wg": WG, "wave": 2, "lane": 5, "index": 3, "mask": 1 << 31}
    lds = {"kind": "lds", "wg": WG, "index": 256, "mask": 1}
    ref.check_sweep(*_sweep_written(mfma, mfma=(0, 1)), NONCE, ITERS, GRID, inject=mfma)
    ref.check_sweep(*_sweep_written(lds, lds=(0, 1)), NONCE, ITERS, GRID, inject=lds)
    wrong = {
        "comparison skipped for wave != 0, or by float value on a zero": (_sweep_written(mfma), mfma),
        "counter credited to another workgroup": (_sweep_written(mfma, mfma=(1, 0)), mfma),
        "ctr[0] and ctr[1] swapped into the record": (_sweep_written(mfma, lds=(0, 1)), mfma),
        "ctr[1] and ctr[0] swapped into the record": (_sweep_written(lds, mfma=(0, 1)), lds),
        "lds read-back never fires": (_sweep_written(lds), lds),
        "every lane counts the wave's wrong word": (_sweep_written(mfma, mfma=(0, 64)), mfma),
    }
    for name, ((recs, tiles), inject) in wrong.items():
        with pytest.raises(AssertionError):
            ref.check_sweep(recs, tiles, NONCE, ITERS, GRID, inject=inject)
            pytest.fail(f"{name}: passed")
    # the injected word never reached wave 0's tile, or reached it from another wave
    w0 = dict(mfma, wave=0)
    recs, _ = _sweep_written(w0, mfma=(0, 1))
    with pytest.raises(AssertionError):
        ref.check_sweep(recs, ref.sweep_tiles(NONCE, ITERS, GRID), NONCE, ITERS, GRID, inject=w0)
    recs, tiles = _sweep_written(w0, mfma=(0, 1))
    with pytest.raises(AssertionError):
        ref.check_sweep(recs, tiles, NONCE, ITERS, GRID, inject=mfma)


def test_check_raw_under_injection_fails_on_wrong_comparators():
    inj = {"kind": "mfma", "wg": WG, "wave": 3, "lane": 5, "index": 2 * 16 + 3, "mask": 1}
    recs, tiles = dp.healthy(GRID, NONCE)
    recs[:, dp.REC_HWID:dp.REC_HWID + 4] |= 1
    good = recs.copy()
    good[WG, dp.REC_BAD + 2] = 1
    dp.check_raw(good, tiles, NONCE, GRID, inject=inj)
    ctr0 = recs.copy()
    ctr0[WG, dp.REC_BAD] = 1                                   # added to ctr[0] instead of ctr[stage]
    other_wg = recs.copy()
    other_wg[0, dp.REC_BAD + 2] = 1
    for wrong in (recs, ctr0, other_wg):
        with pytest.raises(AssertionError):
            dp.check_raw(wrong, tiles, NONCE, GRID, inject=inj)
    with pytest.raises(AssertionError):                        # the hook off must leave every counter 0
        dp.check_raw(good, tiles, NONCE, GRID)

"""The comparators that run on the GPU: do they fire on a wrong word?

mi355x_chip_sweep judges waves 1-3 of every CU and the whole LDS by counters it
computes itself (MI355X_REC_MFMA_BAD, MI355X_REC_LDS_BAD), and
mi355x_mfma_datapath judges waves 1-3 by ctr[stage] (MI355X_DPREC_BAD); only
wave 0's tiles reach the host. The other GPU tests see those counters at zero
on a healthy GPU, which a comparator that never fires would also give. Here the
test-only build of the same sources (liveness_gfx950_inject.hsaco,
MI355X_TEST_INJECT) xors one accumulator register or one LDS word, chosen by
runtime arguments, before the comparison; the counters, the tiles and the
shipped verdicts must then say exactly that, and nothing else.

One child process (testing/raw_kernels.py) runs one request list under a 120 s
limit; every test asserts on the arrays it saved, against
kernel_reference.sweep_injection_image / datapath_reference.injection_image,
which are written from the documented register layout alone. Grid 2, the
injection in workgroup 1: workgroup 0 must stay clean. An injection is a wrong
data word; nothing here faults, hangs or leaves a buffer (the canaries say so).

Last, one production liveness launch at MI355X_PROBE_MAX_ITERS with a nonce
whose tile holds the element that limits the bound, bit for bit against the
integer reference. Measured launch times go to comparators_box.json and are not
judged."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import contract_cli
from rocm_k8s_device_plugin_amd.testing import datapath_reference as dp
from rocm_k8s_device_plugin_amd.testing import kernel_reference as ref
from rocm_k8s_device_plugin_amd.testing import raw_kernels

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
GRID, WG = 2, 1                      # workgroups launched; the one that gets the wrong word
SWEEP_ITERS, SWEEP_WAIT_TICKS = 1, 100000
NONCE = 0xDEADBEEF

OFF_SWEEP = [(0, 1), (0xFFFFFFFF, 4)]
OFF_DATAPATH = [0, 0xFFFFFFFF]

# (wave, lane, register, bit): every wave, lanes 0 / 31 / 32 / 63, registers 0 / 15, bits 0 / 22 / 23 / 30 / 31
SWEEP_MFMA = [(0, 0, 0, 0), (0, 63, 15, 31), (1, 31, 0, 22), (1, 32, 15, 23), (2, 32, 0, 30), (2, 0, 15, 31),
              (3, 63, 0, 0), (3, 31, 15, 30), (0, 32, 15, 23), (0, 31, 0, 22)]


def _zero_element():
    """(wave, lane, register) of the first element of waves 1-3 of workgroup WG whose exact value is 0."""
    for wave in (1, 2, 3):
        for lane in range(64):
            for reg in range(ref.ACC_REGS):
                if ref.sweep_wave_value(NONCE, SWEEP_ITERS, WG, wave, lane, reg) == 0:
                    return wave, lane, reg
    raise AssertionError("no zero element in waves 1-3")


SIGN_OF_ZERO = _zero_element()
SWEEP_LDS = [(w, b) for w in (0, 255, 256, ref.SWEEP_LDS_WORDS - 1) for b in (0, 31)]
# (stage, wave, lane, register, bit): every stage, waves 0 and 3, bits 0 / 23 / 31
DATAPATH = [(0, 0, 0, 0, 0), (0, 3, 63, 15, 23), (1, 0, 31, 15, 31), (1, 3, 32, 0, 0), (2, 0, 63, 0, 23),
            (2, 3, 0, 15, 31), (3, 0, 32, 15, 0), (3, 3, 31, 0, 31)]
# an index past the accumulator / the LDS pattern / the four stages: the hook does nothing
OUT_OF_RANGE = {"sweep_mfma_16": ("sweep", {"kind": "mfma", "wg": WG, "wave": 1, "lane": 5, "index": 16, "mask": 1}),
                "sweep_lds_end": ("sweep", {"kind": "lds", "wg": WG, "index": ref.SWEEP_LDS_WORDS, "mask": 1}),
                "dp_64": ("datapath", {"kind": "mfma", "wg": WG, "wave": 1, "lane": 5, "index": 64, "mask": 1})}

# the bound: the tile of this nonce holds the one element whose partial sums reach 2^24 first
BOUND_ID, BOUND_NONCE, BOUND_ELEMENT = "live_at_bound", 0xFFFFFFBC, (21, 6)


def _mfma(wave, lane, reg, bit):
    return {"kind": "mfma", "wg": WG, "wave": wave, "lane": lane, "index": reg, "mask": 1 << bit}


def _lds(word, bit):
    return {"kind": "lds", "wg": WG, "index": word, "mask": 1 << bit}


def _dp(stage, wave, lane, reg, bit):
    return {"kind": "mfma", "wg": WG, "wave": wave, "lane": lane, "index": stage * 16 + reg, "mask": 1 << bit}


def _sweep_req(rid, nonce, iters, inject=None):
    req = {"id": rid, "kernel": "sweep", "code_object": "inject", "nonce": nonce, "iters": iters, "grid": GRID,
           "wait_ticks": SWEEP_WAIT_TICKS}
    return dict(req, inject=inject) if inject else req


def _dp_req(rid, nonce, inject=None):
    req = {"id": rid, "kernel": "datapath", "code_object": "inject", "nonce": nonce, "grid": GRID}
    return dict(req, inject=inject) if inject else req


def _mfma_id(case):
    return "sweep_mfma_w{}_l{}_r{}_b{}".format(*case)


def _lds_id(case):
    return "sweep_lds_{}_b{}".format(*case)


def _dp_id(case):
    return "dp_s{}_w{}_l{}_r{}_b{}".format(*case)


SIGN_ID = "sweep_sign_of_zero"


def _requests():
    reqs = [_sweep_req(f"off_sweep_{n:08x}_{it}", n, it) for n, it in OFF_SWEEP]
    reqs += [_dp_req(f"off_dp_{n:08x}", n) for n in OFF_DATAPATH]
    reqs += [_sweep_req(_mfma_id(c), NONCE, SWEEP_ITERS, _mfma(*c)) for c in SWEEP_MFMA]
    reqs.append(_sweep_req(SIGN_ID, NONCE, SWEEP_ITERS, _mfma(*SIGN_OF_ZERO, 31)))
    reqs += [_sweep_req(_lds_id(c), NONCE, SWEEP_ITERS, _lds(*c)) for c in SWEEP_LDS]
    reqs += [_dp_req(_dp_id(c), NONCE, _dp(*c)) for c in DATAPATH]
    for rid, (kernel, inject) in OUT_OF_RANGE.items():
        reqs.append(_sweep_req(rid, NONCE, SWEEP_ITERS, inject) if kernel == "sweep" else _dp_req(rid, NONCE, inject))
    reqs.append({"id": BOUND_ID, "kernel": "liveness", "nonce": BOUND_NONCE, "iters": ref.PROBE_MAX_ITERS})
    return reqs


class Run:
    def __init__(self, outdir, requests, returncode, stderr):
        self.outdir, self.requests, self.returncode, self.stderr = outdir, requests, returncode, stderr
        self.by_id = {r["id"]: r for r in requests}

    def load(self, rid: str, name: str) -> np.ndarray:
        path = self.outdir / f"{rid}.{name}.npy"
        if not path.exists():
            pytest.fail(f"{path.name} was not written; the launcher exited {self.returncode}:\n{self.stderr[-3000:]}")
        return np.load(path)

    def status(self) -> dict:
        path = self.outdir / "status.json"
        return json.loads(path.read_text()) if path.exists() else {}


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    work = tmp_path_factory.mktemp("comparators")
    requests = _requests()
    (work / "requests.json").write_text(json.dumps(requests))
    outdir = work / "out"
    cmd = [sys.executable, "-m", "rocm_k8s_device_plugin_amd.testing.raw_kernels", str(work / "requests.json"),
           str(outdir)]
    try:
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=120)
        rc, err = p.returncode, p.stderr
    except subprocess.TimeoutExpired as e:
        err = e.stderr if isinstance(e.stderr, str) else (e.stderr or b"").decode(errors="replace")
        rc, err = "timeout", f"timed out after {e.timeout} s\n{err}"
    r = Run(outdir, requests, rc, err)
    _record_in_box(r, launch_us=r.status().get("launch_us", {}), bound={
        "nonce": BOUND_NONCE, "iters": ref.PROBE_MAX_ITERS,
        "launch_to_synchronize_us": r.status().get("launch_us", {}).get(BOUND_ID)})      # measured, never asserted
    return r


def _record_in_box(run, **figures):
    """Measured figures go to comparators_box.json, in $MI355X_BOX_DIR when it is set (the
    directory a GPU run's records are collected from), else next to the arrays."""
    box_dir = Path(os.environ.get("MI355X_BOX_DIR") or run.outdir.parent)
    box_dir.mkdir(parents=True, exist_ok=True)
    path = box_dir / "comparators_box.json"
    box = json.loads(path.read_text()) if path.exists() else {}
    box.update(figures)
    path.write_text(json.dumps(box, indent=1))


@pytest.fixture(scope="module")
def sweep_cli(tmp_path_factory):
    return contract_cli.contract_cli(tmp_path_factory.mktemp("kernel_contract"))


@pytest.fixture(scope="module")
def dp_cli(tmp_path_factory):
    return dp.contract_cli(tmp_path_factory.mktemp("datapath_contract"))


BUFFERS = {"liveness": ("out", "meta", "scratch"), "sweep": ("records", "tiles", "arrive"),
           "datapath": ("records", "tiles")}


def test_launcher_ran_every_request(run):
    assert run.returncode == 0, run.stderr[-3000:]
    status = run.status()
    assert status["error"] is None and status["completed"] == [r["id"] for r in run.requests]
    assert sorted(status["launch_us"]) == sorted(r["id"] for r in run.requests)
    print("launch to synchronize, us:", {k: round(v, 1) for k, v in status["launch_us"].items()})


def test_all_canaries_intact(run):
    for req in run.requests:
        got = {f"{req['id']}.{n}": run.load(req["id"], f"{n}.canary") for n in BUFFERS[req["kernel"]]}
        assert all(c.shape == (2, raw_kernels.CANARY_BYTES) for c in got.values())
        ref.check_canaries(got, raw_kernels.CANARY_FILL)


# ---- hook off: the test-only build is the production kernel ------------------------------------
@pytest.mark.parametrize("nonce,iters", OFF_SWEEP)
def test_inject_build_with_the_hook_off_sweeps_like_production(run, nonce, iters):
    rid = f"off_sweep_{nonce:08x}_{iters}"
    ref.check_sweep(run.load(rid, "records"), run.load(rid, "tiles"), nonce, iters, GRID)
    assert int(run.load(rid, "arrive")[0]) == GRID


@pytest.mark.parametrize("nonce", OFF_DATAPATH)
def test_inject_build_with_the_hook_off_is_the_production_datapath(run, nonce):
    rid = f"off_dp_{nonce:08x}"
    records = run.load(rid, "records")
    dp.check_raw(records, run.load(rid, "tiles"), nonce, GRID)
    assert (records.reshape(GRID, dp.REC_WORDS)[:, 12:] == 0).all()


@pytest.mark.parametrize("rid", list(OUT_OF_RANGE))
def test_an_index_out_of_range_injects_nothing(run, rid):
    kernel, _ = OUT_OF_RANGE[rid]
    if kernel == "sweep":
        ref.check_sweep(run.load(rid, "records"), run.load(rid, "tiles"), NONCE, SWEEP_ITERS, GRID)
    else:
        dp.check_raw(run.load(rid, "records"), run.load(rid, "tiles"), NONCE, GRID)


# ---- the sweep's comparators -------------------------------------------------------------------
def _sweep_verdict(run, cli, rid, want_error):
    """The shipped verdict on what the kernel wrote, against the reference verdict."""
    records, tiles = run.load(rid, "records"), run.load(rid, "tiles")
    case = dict(grid=GRID, nonce=NONCE, iters=SWEEP_ITERS)
    got, = contract_cli.sweep_verdicts(cli, [contract_cli.sweep_case(records, tiles, num_xcc=0, **case)], 1)
    print("sweep verdict:", got)
    ref.assert_verdict(got, ref.sweep_verdict(records, tiles, num_xcc=0, **case), ref.SWEEP_FLOAT_DIGITS, rid)
    assert got["ok"] is False and got["records_ok"] == GRID - 1 and got["all_resident"] is False, got
    assert want_error in got["error"] and f"{GRID - 1}/{GRID} workgroups correct" in got["error"], got["error"]
    return got


def _check_sweep_mfma(run, cli, rid, wave, lane, reg, bit):
    inject = run.by_id[rid]["inject"]
    assert inject == _mfma(wave, lane, reg, bit)
    records, tiles = run.load(rid, "records"), run.load(rid, "tiles")
    print(rid, "mfma_bad / lds_bad per workgroup:", records.reshape(GRID, 16)[:, [ref.REC_MFMA_BAD, ref.REC_LDS_BAD]].tolist())
    # counter 1 in workgroup WG and 0 elsewhere; the tiles the healthy image but for wave 0's one word
    ref.check_sweep(records, tiles, NONCE, SWEEP_ITERS, GRID, inject=inject)
    healthy = ref.sweep_tiles(NONCE, SWEEP_ITERS, GRID)
    diff = np.flatnonzero(tiles.view(np.uint32) != healthy.view(np.uint32).ravel())
    i, j = ref.accumulator_element(lane, reg)
    assert diff.tolist() == ([WG * 1024 + i * 32 + j] if wave == 0 else []), diff
    if wave == 0:
        assert int(tiles.view(np.uint32)[diff[0]]) ^ int(healthy.view(np.uint32).ravel()[diff[0]]) == 1 << bit
    got = _sweep_verdict(run, cli, rid, "(mfma_bad=1 lds_bad=0 tile_bad={})".format(1 if wave == 0 else 0))
    assert (got["mfma_bad"], got["lds_bad"], got["tile_bad"]) == (1, 0, 1 if wave == 0 else 0), got


@pytest.mark.parametrize("wave,lane,reg,bit", SWEEP_MFMA)
def test_sweep_counts_a_wrong_mfma_word(run, sweep_cli, wave, lane, reg, bit):
    _check_sweep_mfma(run, sweep_cli, _mfma_id((wave, lane, reg, bit)), wave, lane, reg, bit)


def test_sweep_counts_a_flipped_sign_of_a_zero_element(run, sweep_cli):
    """-0.0 == 0.0 as floats: a comparison by value lets this word through, and in waves 1-3 nothing
    else looks at it. The element's exact value is 0, and c >= +0 plus products that cancel is +0.0
    under round to nearest in either k order, so the healthy word is 0x00000000 and the injected
    one 0x80000000."""
    wave, lane, reg = SIGN_OF_ZERO
    assert wave != 0 and ref.sweep_wave_value(NONCE, SWEEP_ITERS, WG, wave, lane, reg) == 0
    i, j = ref.accumulator_element(lane, reg)
    assert ref.tile_f32(ref.sweep_nonce(NONCE, WG, wave), SWEEP_ITERS).view(np.uint32)[i, j] == 0     # +0.0
    _check_sweep_mfma(run, sweep_cli, SIGN_ID, wave, lane, reg, 31)


@pytest.mark.parametrize("word,bit", SWEEP_LDS)
def test_sweep_counts_a_bad_lds_cell(run, sweep_cli, word, bit):
    rid = _lds_id((word, bit))
    inject = run.by_id[rid]["inject"]
    assert inject == _lds(word, bit)
    records, tiles = run.load(rid, "records"), run.load(rid, "tiles")
    print(rid, "mfma_bad / lds_bad per workgroup:", records.reshape(GRID, 16)[:, [ref.REC_MFMA_BAD, ref.REC_LDS_BAD]].tolist())
    ref.check_sweep(records, tiles, NONCE, SWEEP_ITERS, GRID, inject=inject)
    ref.assert_bit_equal(tiles, ref.sweep_tiles(NONCE, SWEEP_ITERS, GRID), "tiles")     # the LDS is not the tile's path
    got = _sweep_verdict(run, sweep_cli, rid, "(mfma_bad=0 lds_bad=1 tile_bad=0)")
    assert (got["mfma_bad"], got["lds_bad"], got["tile_bad"]) == (0, 1, 0), got


# ---- the datapath kernel's comparator ----------------------------------------------------------
@pytest.mark.parametrize("stage,wave,lane,reg,bit", DATAPATH)
def test_datapath_counts_a_wrong_mfma_word_in_its_stage(run, dp_cli, stage, wave, lane, reg, bit):
    rid = _dp_id((stage, wave, lane, reg, bit))
    inject = run.by_id[rid]["inject"]
    assert inject == _dp(stage, wave, lane, reg, bit)
    records, tiles = run.load(rid, "records"), run.load(rid, "tiles")
    print(rid, "stage_bad per workgroup:", records.reshape(GRID, dp.REC_WORDS)[:, dp.REC_BAD:dp.REC_BAD + 4].tolist())
    # ctr[stage] of workgroup WG is 1, every other counter 0; the tiles healthy but for wave 0's one word
    dp.check_raw(records, tiles, NONCE, GRID, inject=inject)
    healthy = dp.tiles_image(NONCE, GRID).ravel()
    diff = np.flatnonzero(tiles != healthy)
    i, j = dp.accumulator_element(lane, reg)
    word = i * 32 + j
    assert diff.tolist() == ([WG * dp.WG_WORDS + stage * dp.TILE_WORDS + word] if wave == 0 else []), diff
    got, = dp.verdicts(dp_cli, [dp.case(records, tiles, GRID, NONCE)], 1)
    print("datapath verdict:", got)
    dp.assert_verdict(got, dp.verdict(records, tiles, GRID, NONCE), rid)
    assert got["ok"] is False and got["records_ok"] == GRID - 1 and got["mfma_bad"] == 1, got
    assert got["stage_bad"] == [int(s == stage) for s in range(4)], got
    assert f"{GRID - 1}/{GRID} workgroups exact (device_bad=1 tile_bad={1 if wave == 0 else 0})" in got["error"], got["error"]
    if wave == 0:
        assert got["tile_bad"] == 1, got
        assert (got["first_bad_wg"], got["first_bad_stage"], got["first_bad_word"], got["first_bad_xor"]) == (
            WG, stage, word, 1 << bit), got
        assert f"first bad: wg {WG} stage {stage} word {word} xor 0x{1 << bit:08x} (bit {bit})" in got["error"]
    else:               # the device counter alone turned the verdict
        assert got["tile_bad"] == 0 and got["first_bad_wg"] == -1 and got["first_bad_xor"] == 0, got


# ---- the liveness tile at the iteration bound --------------------------------------------------
def test_liveness_tile_is_exact_at_the_iteration_bound(run):
    """About 1.4 million dependent MFMAs in one wave; at the bound the limiting element is
    1 + 12 * 1398101 = 16777213, the last count at which each of its partial sums is below 2^24."""
    i, j = BOUND_ELEMENT
    triple = (ref.probe_c(i, j, BOUND_NONCE),
              ref.probe_a(i, 0, BOUND_NONCE) * ref.probe_b(0, j, BOUND_NONCE),
              ref.probe_a(i, 1, BOUND_NONCE) * ref.probe_b(1, j, BOUND_NONCE))
    assert triple == (1, 6, 6)                                        # the tile holds the limiting element
    want = ref.tile(BOUND_NONCE, ref.PROBE_MAX_ITERS)
    assert int(want[i, j]) == 16777213 and int(np.abs(want).max()) == 16777213
    print("launch to synchronize at the bound, us:", run.status().get("launch_us", {}).get(BOUND_ID))
    out, scratch, meta = run.load(BOUND_ID, "out"), run.load(BOUND_ID, "scratch"), run.load(BOUND_ID, "meta")
    ref.check_liveness(out.reshape(32, 32), scratch.reshape(16, 64), meta, BOUND_NONCE, ref.PROBE_MAX_ITERS)


def test_probe_program_clamps_iters_to_the_bound(run):
    """--iters beyond the bound: the probe runs the bound, says so, and its host check agrees with the tile
    (the same nonce: the limiting element is in it). Started only after the launcher ended normally."""
    from rocm_k8s_device_plugin_amd.ops.native import probe_executable
    assert run.returncode == 0, run.stderr[-3000:]
    p = subprocess.run([str(probe_executable("hsa")), "--devices", "0", "--nonce", str(BOUND_NONCE), "--iters",
                        str(1 << 30), "--timeout", "20"], cwd=REPO, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    d = json.loads(p.stdout)["devices"][0]
    _record_in_box(run, probe_at_bound={k: d.get(k) for k in ("iters", "kernel_us", "total_us")})
    assert d["ok"] is True and d["iters"] == ref.PROBE_MAX_ITERS and d["mismatches"] == 0 and d["nonce"] == BOUND_NONCE, d

"""The MFMA datapath check on a real MI355X: every byte mi355x_mfma_datapath
writes against the independent reference (testing/datapath_reference.py), the
shipped verdict on those bytes, the probe program one-shot and in serve mode,
and the in-process binding.

A module fixture runs the child processes in order, each under its own
timeout, and starts nothing further after one ended abnormally (a signal, an
abort, a timeout); the tests assert on what the children left. The grids are
the smallest at which the kernel can go wrong: one workgroup, and three (more
than one, not a power of two); the production grid (one workgroup per CU) runs
once, through the shipped probe, and its measured figures are recorded, not
asserted."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import datapath_reference as dp
from rocm_k8s_device_plugin_amd.testing import kernel_reference as ref
from rocm_k8s_device_plugin_amd.testing import raw_kernels

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
GRIDS = (1, 3)
NONCES = (0, 0xFFFFFFFF, 0xDEADBEEF)
RAW_CASES = [(g, n) for g in GRIDS for n in NONCES]
FLIP_BITS = (0, 22, 23, 30, 31)
CORRUPT = {"bit30": "2:517:30", "bit0": "2:517:0"}
SERVE_INPUT = "probe 4 10 0:101\ndatapath 10 0:102\nprobe 4 10 0:103\nquit\n"
BINDING_NONCE = 0xDEADBEEF
BINDING_CODE = ("import json; from rocm_k8s_device_plugin_amd.ops.native import hip; "
                f"print(json.dumps(hip().hsa_datapath_check(0, {BINDING_NONCE}, 10.0)))")
ABNORMAL = (124, 134, 137, 139)


def _raw_id(grid, nonce):
    return f"dp_{grid}_{nonce:08x}"


class Step:
    def __init__(self, rc, out, err):
        self.rc, self.out, self.err = rc, out, err

    @property
    def abnormal(self):
        return self.rc == "timeout" or self.rc < 0 or self.rc in ABNORMAL


class Steps:
    def __init__(self, work):
        self.work, self.done, self.stopped_at = work, {}, None

    def run(self, name, cmd, timeout, stdin=None, env=None):
        if self.stopped_at:
            return
        try:
            p = subprocess.run(cmd, cwd=REPO, input=stdin, capture_output=True, text=True, timeout=timeout,
                               env=dict(os.environ, **(env or {})))
            step = Step(p.returncode, p.stdout, p.stderr)
        except subprocess.TimeoutExpired as e:
            err = e.stderr if isinstance(e.stderr, str) else (e.stderr or b"").decode(errors="replace")
            step = Step("timeout", "", f"timed out after {e.timeout} s\n{err}")
        self.done[name] = step
        if step.abnormal:
            self.stopped_at = name

    def get(self, name) -> Step:
        if name not in self.done:
            bad = self.done[self.stopped_at]
            pytest.fail(f"{name} was not started: {self.stopped_at} ended abnormally ({bad.rc}):\n{bad.err[-3000:]}")
        return self.done[name]

    def load(self, rid, name) -> np.ndarray:
        path = self.work / "out" / f"{rid}.{name}.npy"
        if not path.exists():
            raw = self.get("raw")
            pytest.fail(f"{path.name} was not written; the launcher exited {raw.rc}:\n{raw.err[-3000:]}")
        return np.load(path)


@pytest.fixture(scope="module")
def steps(tmp_path_factory):
    from rocm_k8s_device_plugin_amd.ops.native import probe_executable
    work = tmp_path_factory.mktemp("datapath")
    requests = [{"id": _raw_id(g, n), "kernel": "datapath", "nonce": n, "grid": g} for g, n in RAW_CASES]
    (work / "requests.json").write_text(json.dumps(requests))
    probe = str(probe_executable("hsa"))
    s = Steps(work)
    s.run("raw", [sys.executable, "-m", "rocm_k8s_device_plugin_amd.testing.raw_kernels", str(work / "requests.json"),
                  str(work / "out")], 120)
    s.run("probe", [probe, "--datapath", "--devices", "0", "--timeout", "10"], 60)
    for name, spec in CORRUPT.items():
        s.run(f"probe_{name}", [probe, "--datapath", "--devices", "0", "--timeout", "10", "--corrupt-datapath", spec],
              60)
    s.run("serve", [probe, "--serve", "--keep"], 60, stdin=SERVE_INPUT)
    s.run("binding", [sys.executable, "-c", BINDING_CODE], 120)
    return s


# ---- 1. raw launcher: every byte against the reference image -------------------------
def test_launcher_ran_every_request(steps):
    raw = steps.get("raw")
    assert raw.rc == 0, raw.err[-3000:]
    status = json.loads((steps.work / "out" / "status.json").read_text())
    assert status["error"] is None and status["completed"] == [_raw_id(g, n) for g, n in RAW_CASES]
    assert "torch" not in status["hip_library"]


@pytest.mark.parametrize("grid,nonce", RAW_CASES)
def test_records_and_tiles_equal_the_reference_image(steps, grid, nonce):
    rid = _raw_id(grid, nonce)
    records, tiles = steps.load(rid, "records"), steps.load(rid, "tiles")
    assert records.dtype == np.uint32 and records.size == grid * dp.REC_WORDS
    assert tiles.dtype == np.uint32 and tiles.size == grid * dp.WG_WORDS
    # every tile byte, every record byte that is not the hardware's to choose; device bad counts 0; HW_ID non-zero
    dp.check_raw(records, tiles, nonce, grid)
    assert (records.reshape(grid, dp.REC_WORDS)[:, 12:] == 0).all()       # the reserved words were written too
    canaries = {f"{rid}.{n}": steps.load(rid, f"{n}.canary") for n in ("records", "tiles")}
    assert all(c.shape == (2, raw_kernels.CANARY_BYTES) for c in canaries.values())
    ref.check_canaries(canaries, raw_kernels.CANARY_FILL)


# ---- 2. the shipped verdict on what the kernel wrote -----------------------------------
@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return dp.contract_cli(tmp_path_factory.mktemp("datapath_contract"))


@pytest.mark.parametrize("grid,nonce", RAW_CASES)
def test_verdict_on_what_the_kernel_wrote(steps, cli, grid, nonce):
    rid = _raw_id(grid, nonce)
    records, tiles = steps.load(rid, "records"), steps.load(rid, "tiles")
    wg, stage, word = grid - 1, 2, 517
    idx = wg * dp.WG_WORDS + stage * dp.TILE_WORDS + word
    flips = [[(dp.TILES, idx, int(tiles[idx]) ^ 1 << b)] for b in FLIP_BITS]
    got = dp.verdicts(cli, [dp.case(records, tiles, grid, nonce, flips)], 1 + len(flips))
    print("datapath verdict:", got[0])
    dp.assert_verdict(got[0], dp.verdict(records, tiles, grid, nonce), rid)
    assert got[0]["ok"] is True and got[0]["records_ok"] == grid and got[0]["error"] == "", got[0]
    for b, g in zip(FLIP_BITS, got[1:]):
        wrong = tiles.copy()
        wrong[idx] ^= np.uint32(1 << b)
        dp.assert_verdict(g, dp.verdict(records, wrong, grid, nonce), f"{rid} bit {b}")
        assert g["ok"] is False and g["tile_bad"] == 1 and g["first_bad_xor"] == 1 << b, g
        assert (g["first_bad_wg"], g["first_bad_stage"], g["first_bad_word"]) == (wg, stage, word), g


# ---- 3. the shipped probe, one-shot, at the production grid ----------------------------
def _record_in_box(steps, **figures):
    """Measured figures go to datapath_box.json, in $MI355X_BOX_DIR when it is set (the
    directory a GPU run's records are collected from), else next to the arrays."""
    box_dir = Path(os.environ.get("MI355X_BOX_DIR") or steps.work)
    box_dir.mkdir(parents=True, exist_ok=True)
    path = box_dir / "datapath_box.json"
    box = json.loads(path.read_text()) if path.exists() else {}
    box.update(figures)
    path.write_text(json.dumps(box, indent=1))


def test_probe_one_shot_at_the_production_grid(steps):
    p = steps.get("probe")
    doc = json.loads(p.out) if p.out.strip() else {}
    d = (doc.get("devices") or [{}])[0]
    _record_in_box(steps, production_grid={k: d.get(k) for k in (
        "grid", "cu_count", "num_xcc", "kernel_us", "total_us", "cus_covered", "simds_covered", "xccs_covered")})
    print("datapath probe:", d)                                     # before anything is asserted
    assert p.rc == 0, (p.rc, p.out[-2000:], p.err[-2000:])
    assert doc["ok"] is True and doc["datapath"] is True
    assert d["ok"] is True and d["records_ok"] == d["grid"] == d["cu_count"] > 0, d
    assert d["mfma_bad"] == 0 and d["tile_bad"] == 0 and d["error"] == "" and d["first_bad_stage"] == -1, d


@pytest.mark.parametrize("name", list(CORRUPT))
def test_probe_names_stage_word_and_bit_of_an_injected_flip(steps, name):
    stage, word, bit = (int(x) for x in CORRUPT[name].split(":"))
    p = steps.get(f"probe_{name}")
    assert p.rc == 1, (p.rc, p.out[-2000:], p.err[-2000:])
    doc = json.loads(p.out)
    d = doc["devices"][0]
    assert doc["ok"] is False and d["ok"] is False and d["tile_bad"] == 1 and d["records_ok"] == d["grid"] - 1, d
    assert (d["first_bad_wg"], d["first_bad_stage"], d["first_bad_word"], d["first_bad_xor"]) == (0, stage, word, 1 << bit)
    assert f"stage {stage} word {word} xor 0x{1 << bit:08x} (bit {bit})" in d["error"], d["error"]


# ---- 4. serve mode: the check borrows the kept queue and gives it back -------------------
def test_serve_mode_borrows_the_kept_queue_and_returns_it(steps):
    p = steps.get("serve")
    lines = [json.loads(ln) for ln in p.out.splitlines() if ln.startswith("{")]
    kept = (lines[2].get("devices") or [{}])[0] if len(lines) > 2 else {}
    _record_in_box(steps, kept_queue={k: kept.get(k) for k in (
        "grid", "kept_queue", "kernel_us", "total_us", "cus_covered", "simds_covered", "xccs_covered")})
    assert p.rc == 0, (p.rc, p.out[-2000:], p.err[-2000:])     # the figures are recorded before anything is asserted
    hello, first, check, after = lines
    assert hello["serve"] and hello["ok"]
    assert first["devices"][0]["ok"] and first["devices"][0]["nonce"] == 101, first
    d = check["devices"][0]
    assert check["ok"] is True and check["datapath"] is True and d["ok"] is True and d["kept_queue"] is True, check
    assert d["nonce"] == 102 and d["records_ok"] == d["grid"] == d["cu_count"], d
    assert after["devices"][0]["ok"] and after["devices"][0]["nonce"] == 103, after
    assert "datapath" not in first and "datapath" not in after        # the probe replies are what they were


# ---- 5. the in-process binding ------------------------------------------------------------
def test_in_process_binding(steps):
    p = steps.get("binding")
    assert p.rc == 0, (p.rc, p.out[-2000:], p.err[-2000:])
    d = json.loads(p.out.splitlines()[-1])
    assert d["ok"] is True and d["nonce"] == BINDING_NONCE and d["records_ok"] == d["grid"] == d["cu_count"], d
    assert d["tile_bad"] == 0 and d["mfma_bad"] == 0 and list(d["stage_bad"]) == [0, 0, 0, 0], d

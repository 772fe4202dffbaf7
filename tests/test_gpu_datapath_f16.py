"""The f16 MFMA datapath check on a real MI355X: every byte
mi355x_mfma_datapath_f16 writes against the independent reference
(testing/datapath_f16_reference.py), the on-device comparator under the
test-only injection hook, the shipped verdict on those bytes, the probe
program one-shot and in serve mode, and the in-process binding.

A module fixture runs the child processes in order, each under its own
timeout, and starts nothing further after one ended abnormally (a signal, an
abort, a timeout); the tests assert on what the children left. The grids are
the smallest at which the kernel can go wrong: one workgroup (four wave nonces,
all seven stages), and three (workgroup indexing, the record stride), launched
with five workgroups so that two of them must stop at the `wg >= grid` guard
(the canaries behind the buffers show a write past them); the production grid (one workgroup per CU) runs
once, through the shipped probe, and its measured figures are recorded, not
asserted. One test needs no device: the production code object compiles to the
same bytes with the two f16 files' test-only blocks deleted."""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import datapath_f16_reference as db
from rocm_k8s_device_plugin_amd.testing import kernel_reference as ref
from rocm_k8s_device_plugin_amd.testing import raw_kernels

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
GRIDS = (1, 3)
NONCES = (0xFFFFFFFF, 0xDEADBEEF)
OVER_LAUNCH = {3: 5}                  # grid -> workgroups launched
RAW_CASES = [(g, n) for g in GRIDS for n in NONCES]
FLIP_BITS = (0, 7, 8, 19, 30, 31)
# the comparator under the hook: grid 2, a fault in workgroup 1. Every stage once, every wave once; wave 0's
# reaches the stored tile too, the others only the counter; all four instruction shapes from wave 0 (stages 0,
# 4, 5, 6); and the hook present but off
INJECT_GRID, INJECT_NONCE = 2, 0xDEADBEEF
INJECTIONS = {
    "stage0_wave0": {"kind": "mfma", "wg": 1, "wave": 0, "lane": 37, "index": 0 * 16 + 6, "mask": 1 << 0},
    "stage1_wave1": {"kind": "mfma", "wg": 1, "wave": 1, "lane": 0, "index": 1 * 16 + 15, "mask": 1 << 31},
    "stage2_wave2": {"kind": "mfma", "wg": 1, "wave": 2, "lane": 63, "index": 2 * 16 + 0, "mask": 1 << 19},
    "stage3_wave3": {"kind": "mfma", "wg": 1, "wave": 3, "lane": 32, "index": 3 * 16 + 2, "mask": 1 << 7},
    "stage4_wave0": {"kind": "mfma", "wg": 1, "wave": 0, "lane": 49, "index": 4 * 16 + 3, "mask": 1 << 30},
    "stage5_wave0": {"kind": "mfma", "wg": 1, "wave": 0, "lane": 31, "index": 5 * 16 + 12, "mask": 1 << 23},
    "stage6_wave1": {"kind": "mfma", "wg": 1, "wave": 1, "lane": 62, "index": 6 * 16 + 3, "mask": 1 << 12},
    "stage6_wave0": {"kind": "mfma", "wg": 1, "wave": 0, "lane": 17, "index": 6 * 16 + 1, "mask": 1 << 3},
    "no_register": {"kind": "mfma", "wg": 1, "wave": 0, "lane": 5, "index": 4 * 16 + 4, "mask": 1 << 30},
    "off": None,
}
CORRUPT = {"wide": "2:5:30", "legacy": "5:1023:31", "narrow": "6:201:0"}
SERVE_INPUT = "probe 4 10 0:101\ndatapath_f16 10 0:102\ndatapath 10 0:103\nprobe 4 10 0:104\nquit\n"
BINDING_NONCE = 0xDEADBEEF
BINDING_CODE = ("import json; from rocm_k8s_device_plugin_amd.ops.native import hip; "
                f"print(json.dumps(hip().hsa_datapath_f16_check(0, {BINDING_NONCE}, 10.0)))")
ABNORMAL = (124, 134, 137, 139)


def _raw_id(grid, nonce):
    return f"dphf_{grid}_{nonce:08x}"


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
    work = tmp_path_factory.mktemp("datapath_f16")
    requests = [{"id": _raw_id(g, n), "kernel": "datapath_f16", "nonce": n, "grid": g,
                 "launch_grid": OVER_LAUNCH.get(g, g)} for g, n in RAW_CASES]
    for name, inj in INJECTIONS.items():
        req = {"id": f"inj_{name}", "kernel": "datapath_f16", "nonce": INJECT_NONCE, "grid": INJECT_GRID,
               "code_object": "inject"}
        if inj is not None:
            req["inject"] = inj
        requests.append(req)
    (work / "requests.json").write_text(json.dumps(requests))
    probe = str(probe_executable("hsa"))
    s = Steps(work)
    s.run("raw", [sys.executable, "-m", "rocm_k8s_device_plugin_amd.testing.raw_kernels", str(work / "requests.json"),
                  str(work / "out")], 120)
    s.run("probe", [probe, "--datapath-f16", "--devices", "0", "--timeout", "10"], 60)
    for name, spec in CORRUPT.items():
        s.run(f"probe_{name}", [probe, "--datapath-f16", "--devices", "0", "--timeout", "10",
                                "--corrupt-datapath-f16", spec], 60)
    s.run("probe_no_gpu", [probe, "--datapath-f16", "--devices", "99", "--nonce", "7000", "--timeout", "10"], 60)
    s.run("probe_hip", [str(probe_executable("hip")), "--datapath-f16", "--devices", "0", "--nonce", "7100"], 60)
    s.run("serve", [probe, "--serve", "--keep"], 60, stdin=SERVE_INPUT)
    s.run("binding", [sys.executable, "-c", BINDING_CODE], 120)
    return s


# ---- 1. raw launcher, production code object: every byte against the reference image ------------
def test_launcher_ran_every_request(steps):
    raw = steps.get("raw")
    assert raw.rc == 0, raw.err[-3000:]
    status = json.loads((steps.work / "out" / "status.json").read_text())
    want = [_raw_id(g, n) for g, n in RAW_CASES] + [f"inj_{name}" for name in INJECTIONS]
    assert status["error"] is None and status["completed"] == want
    assert "torch" not in status["hip_library"]


def _canaries_intact(steps, rid):
    canaries = {f"{rid}.{n}": steps.load(rid, f"{n}.canary") for n in ("records", "tiles")}
    assert all(c.shape == (2, raw_kernels.CANARY_BYTES) for c in canaries.values())
    ref.check_canaries(canaries, raw_kernels.CANARY_FILL)


@pytest.mark.parametrize("grid,nonce", RAW_CASES)
def test_records_and_tiles_equal_the_reference_image(steps, grid, nonce):
    rid = _raw_id(grid, nonce)
    records, tiles = steps.load(rid, "records"), steps.load(rid, "tiles")
    assert records.dtype == np.uint32 and records.size == grid * db.REC_WORDS
    assert tiles.dtype == np.uint32 and tiles.size == grid * db.WG_WORDS
    # every tile byte, every record byte that is not the hardware's to choose; device bad counts 0; HW_ID non-zero
    db.check_raw(records, tiles, nonce, grid)
    assert (records.reshape(grid, db.REC_WORDS)[:, 15:] == 0).all()       # the reserved word was written too
    _canaries_intact(steps, rid)


# ---- 2. raw launcher, inject code object: the on-device comparator sees one wrong word ------------
@pytest.mark.parametrize("name", list(INJECTIONS))
def test_injected_word_is_counted_once_in_its_stage_and_workgroup(steps, name):
    rid, inj = f"inj_{name}", INJECTIONS[name]
    records, tiles = steps.load(rid, "records"), steps.load(rid, "tiles")
    bad = records.reshape(INJECT_GRID, db.REC_WORDS)[:, db.REC_BAD:db.REC_BAD + db.STAGES]
    print(f"datapath f16 injection {name}: counters {bad.tolist()}")            # before anything is asserted
    db.check_raw(records, tiles, INJECT_NONCE, INJECT_GRID, inject=inj)
    want = np.zeros((INJECT_GRID, db.STAGES), dtype=np.int64)
    hits = inj is not None and inj["index"] % 16 < db.ACC_REGS[inj["index"] // 16]   # it names a register
    if hits:
        want[1, inj["index"] // 16] = 1
    assert (bad == want).all(), bad.tolist()
    changed = np.flatnonzero(tiles != db.tiles_image(INJECT_NONCE, INJECT_GRID).ravel())
    assert len(changed) == (1 if hits and inj["wave"] == 0 else 0)              # only wave 0's tile is stored
    _canaries_intact(steps, rid)


# ---- 3. the shipped verdict on what the kernel wrote -----------------------------------------------
@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return db.contract_cli(tmp_path_factory.mktemp("datapath_f16_contract"))


@pytest.mark.parametrize("grid,nonce", RAW_CASES)
def test_verdict_on_what_the_kernel_wrote(steps, cli, grid, nonce):
    rid = _raw_id(grid, nonce)
    records, tiles = steps.load(rid, "records"), steps.load(rid, "tiles")
    wg = grid - 1
    places = [(stage, (517 + 37 * stage) % db.TILE_WORDS[stage]) for stage in range(db.STAGES)]
    flips, what = [], []
    for stage, word in places:
        idx = wg * db.WG_WORDS + db.TILE_OFFSET[stage] + word
        for b in FLIP_BITS:
            flips.append([(db.TILES, idx, int(tiles[idx]) ^ 1 << b)])
            what.append((stage, word, idx, b))
    got = db.verdicts(cli, [db.case(records, tiles, grid, nonce, flips)], 1 + len(flips))
    print("datapath f16 verdict:", got[0])
    db.assert_verdict(got[0], db.verdict(records, tiles, grid, nonce), rid)
    assert got[0]["ok"] is True and got[0]["records_ok"] == grid and got[0]["error"] == "", got[0]
    for (stage, word, idx, b), g in zip(what, got[1:]):
        wrong = tiles.copy()
        wrong[idx] ^= np.uint32(1 << b)
        db.assert_verdict(g, db.verdict(records, wrong, grid, nonce), f"{rid} stage {stage} bit {b}")
        assert g["ok"] is False and g["tile_bad"] == 1 and g["first_bad_xor"] == 1 << b, g
        assert (g["first_bad_wg"], g["first_bad_stage"], g["first_bad_word"]) == (wg, stage, word), g
        assert f"(bit {b})" in g["error"]


def test_verdict_names_an_injected_word_from_the_device(steps, cli):
    """Wave 0's injected words reach the verdict as the kernel stored them."""
    for name in ("stage0_wave0", "stage4_wave0", "stage5_wave0", "stage6_wave0"):
        inj = INJECTIONS[name]
        records, tiles = steps.load(f"inj_{name}", "records"), steps.load(f"inj_{name}", "tiles")
        g, = db.verdicts(cli, [db.case(records, tiles, INJECT_GRID, INJECT_NONCE)], 1)
        stage, reg = divmod(inj["index"], 16)
        i, j = db.accumulator_element(stage, inj["lane"], reg)
        assert g["ok"] is False and g["records_ok"] == 1 and g["tile_bad"] == 1 and g["mfma_bad"] == 1, g
        assert (g["first_bad_wg"], g["first_bad_stage"], g["first_bad_word"], g["first_bad_xor"]) == \
            (1, stage, i * db.DIM[stage] + j, inj["mask"]), g
        assert g["stage_bad"] == [int(s == stage) for s in range(db.STAGES)]


# ---- 4. the shipped probe, one-shot, at the production grid ----------------------------------------
def _record_in_box(steps, **figures):
    """Measured figures go to datapath_f16_box.json, in $MI355X_BOX_DIR when it is set (the
    directory a GPU run's records are collected from), else next to the arrays."""
    box_dir = Path(os.environ.get("MI355X_BOX_DIR") or steps.work)
    box_dir.mkdir(parents=True, exist_ok=True)
    path = box_dir / "datapath_f16_box.json"
    box = json.loads(path.read_text()) if path.exists() else {}
    box.update(figures)
    path.write_text(json.dumps(box, indent=1))


def test_probe_one_shot_at_the_production_grid(steps):
    p = steps.get("probe")
    doc = json.loads(p.out) if p.out.strip() else {}
    d = (doc.get("devices") or [{}])[0]
    _record_in_box(steps, production_grid={k: d.get(k) for k in (
        "grid", "cu_count", "num_xcc", "kernel_us", "total_us", "cus_covered", "simds_covered", "xccs_covered")})
    print("datapath f16 probe:", d)                                  # before anything is asserted
    assert p.rc == 0, (p.rc, p.out[-2000:], p.err[-2000:])
    assert doc["ok"] is True and doc["datapath_f16"] is True and "datapath" not in doc
    assert d["ok"] is True and d["records_ok"] == d["grid"] == d["cu_count"] > 0, d
    assert d["mfma_bad"] == 0 and d["stage_bad"] == [0] * 7 and d["tile_bad"] == 0, d
    assert d["error"] == "" and d["first_bad_stage"] == -1, d


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


def test_replies_that_never_reach_a_device(steps):
    """An ordinal past the visible GPUs, and the HIP build, which has no such check."""
    p = steps.get("probe_no_gpu")
    doc = json.loads(p.out)
    d = doc["devices"][0]
    assert p.rc == 1 and doc["ok"] is False and doc["datapath_f16"] is True, doc
    assert d["ok"] is False and d["ordinal"] == 99 and d["error"].startswith("no such GPU (count="), d
    assert d["stage_bad"] == [0] * 7 and d["kept_queue"] is False, d
    assert d["first_bad_wg"] == d["first_bad_stage"] == d["first_bad_word"] == -1, d
    p = steps.get("probe_hip")
    doc = json.loads(p.out)
    d = doc["devices"][0]
    assert p.rc == 1 and doc["ok"] is False and d["ok"] is False and d["nonce"] == 7100, doc
    assert d["error"] == "--datapath-f16 needs the HSA-direct build (mi355x-liveness-probe)", d
    assert d["first_bad_wg"] == d["first_bad_stage"] == d["first_bad_word"] == -1, d


# ---- 5. serve mode: the check borrows the kept queue and gives it back ------------------------------
def test_serve_mode_borrows_the_kept_queue_and_leaves_the_neighbours_alone(steps):
    p = steps.get("serve")
    lines = [json.loads(ln) for ln in p.out.splitlines() if ln.startswith("{")]
    kept = (lines[2].get("devices") or [{}])[0] if len(lines) > 2 else {}
    _record_in_box(steps, kept_queue={k: kept.get(k) for k in (
        "grid", "kept_queue", "kernel_us", "total_us", "cus_covered", "simds_covered", "xccs_covered")})
    assert p.rc == 0, (p.rc, p.out[-2000:], p.err[-2000:])     # the figures are recorded before anything is asserted
    hello, first, check, f32, after = lines
    assert hello["serve"] and hello["ok"] and "datapath_f16" not in hello
    assert first["devices"][0]["ok"] and first["devices"][0]["nonce"] == 101, first
    d = check["devices"][0]
    assert check["ok"] is True and check["datapath_f16"] is True and "datapath" not in check, check
    assert d["ok"] is True and d["kept_queue"] is True and d["nonce"] == 102, d
    assert d["records_ok"] == d["grid"] == d["cu_count"] and d["stage_bad"] == [0] * 7, d
    f = f32["devices"][0]
    assert f32["ok"] is True and f32["datapath"] is True and "datapath_f16" not in f32, f32
    assert f["ok"] is True and f["kept_queue"] is True and f["nonce"] == 103 and len(f["stage_bad"]) == 4, f
    assert after["devices"][0]["ok"] and after["devices"][0]["nonce"] == 104, after
    for reply in (first, after):                                     # the probe replies are what they were
        assert "datapath" not in reply and "datapath_f16" not in reply
        assert sorted(reply) == ["devices", "hip_device_count", "ok", "perf", "sweep", "t_ready_ns"]


# ---- 6. the in-process binding ------------------------------------------------------------------------
def test_in_process_binding(steps):
    p = steps.get("binding")
    assert p.rc == 0, (p.rc, p.out[-2000:], p.err[-2000:])
    d = json.loads(p.out.splitlines()[-1])
    assert d["ok"] is True and d["nonce"] == BINDING_NONCE and d["records_ok"] == d["grid"] == d["cu_count"], d
    assert d["tile_bad"] == 0 and d["mfma_bad"] == 0 and list(d["stage_bad"]) == [0] * 7, d


# ---- 7. the test-only hook leaves the production code object alone ---------------------------------
def _without_inject_blocks(text: str) -> str:
    out, n = re.subn(r"^#if defined\(MI355X_TEST_INJECT\)\n.*?^#endif\n", "", text, flags=re.M | re.S)
    assert n >= 1 and "MI355X_TEST_INJECT" not in out
    return out


def test_production_code_object_is_the_same_without_the_inject_blocks(tmp_path):
    """health_kernels.hip compiled as the production code object is (no MI355X_TEST_INJECT), once as it is and
    once with the `#if defined(MI355X_TEST_INJECT)` blocks of datapath_f16_kernel.{h,hip} deleted, both named
    by the same relative paths: the same sha256."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    children = []
    for which in ("as_is", "stripped"):         # both at once, each from its own directory by relative paths only
        tree = tmp_path / which / "health"
        shutil.copytree(REPO / "native" / "src" / "health", tree)
        shutil.copytree(REPO / "native" / "include", tmp_path / which / "include")
        if which == "stripped":
            for name in ("datapath_f16_kernel.h", "datapath_f16_kernel.hip"):
                (tree / name).write_text(_without_inject_blocks((tree / name).read_text()))
        children.append(subprocess.Popen(
            [hipcc, "--offload-arch=gfx950", "-O3", "-I", "../include", "-I", ".", "--genco", "--no-gpu-bundle-output",
             "health_kernels.hip", "-o", "out.hsaco"], cwd=tree, stderr=subprocess.PIPE, text=True))
    digests = []
    for child in children:
        _, err = child.communicate(timeout=300)
        assert child.returncode == 0, err[-3000:]
    for which in ("as_is", "stripped"):
        digests.append(hashlib.sha256((tmp_path / which / "health" / "out.hsaco").read_bytes()).hexdigest())
    print("datapath f16 production code object sha256:", digests)
    assert digests[0] == digests[1]

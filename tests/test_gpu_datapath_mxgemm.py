"""The MXFP4 GEMM pipeline check on a real MI355X. A module fixture runs the child processes in order, each under its
own timeout, and starts nothing further after one ended abnormally (test_gpu_datapath_f16.Steps). One k-step is the
prologue only, two use both LDS buffers, three reuse the first with the scale prefetch wrapping; grid 2 launched with 3
workgroups covers the panel offsets and the `wg >= grid` guard, with canaries around all six buffers."""
import json
import os
import sys
from pathlib import Path

import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import datapath_mxgemm_reference as db
from rocm_k8s_device_plugin_amd.testing import raw_kernels

from test_gpu_datapath_f16 import Steps, _canaries_intact      # the children's runner and the canary check

pytestmark = pytest.mark.gpu

RAW_CASES = [(1, 1, 0xFFFFFFFF), (1, 2, 0xDEADBEEF), (1, 3, 0xDEADBEEF), (2, 2, 0xFFFFFFFF)]
# the inject build at grid 2, two k-steps, each hook on workgroup 1; a flipped code or scale bit leaves D exact
INJECT_NONCE, INJECT_KSTEPS = 0xDEADBEEF, 2
INJECTIONS = {"mfma": dict(kind="mfma", wg=1, wave=2, lane=37, index=1 * 16 + 6, mask=1 << 30),
              "lds_a": dict(kind="lds", wg=1, step=1, index=1234, mask=1 << 9),
              "lds_b": dict(kind="lds", wg=1, step=0, index=4096 + 2999, mask=1 << 28),
              "hbm": dict(kind="hbm", wg=1, index=101 * INJECT_KSTEPS * 128 + 70, mask=0x10),
              "scale": dict(kind="scale", wg=1, wave=1, lane=40, index=1 * 16 + 2 * 4 + 0, mask=1 << 16),
              "off": None}
CORRUPT = ("0:5:31", "1:18:0", "2:7:9", "3:16383:20")
SERVE_INPUT = "probe 4 10 0:101\ndatapath_mxgemm 10 0:102\ndatapath 10 0:103\nprobe 4 10 0:104\nquit\n"
BINDING = ("import json; from rocm_k8s_device_plugin_amd.ops.native import hip; "
           "print(json.dumps(hip().hsa_datapath_mxgemm_check(0, 3735928559, 10.0)))")


def _rid(grid, ksteps, nonce):
    return f"dpmx_{grid}_{ksteps}_{nonce:08x}"


@pytest.fixture(scope="module")
def steps(tmp_path_factory):
    from rocm_k8s_device_plugin_amd.ops.native import probe_executable
    work = tmp_path_factory.mktemp("datapath_mxgemm")
    requests = [{"id": _rid(g, k, n), "kernel": "datapath_mxgemm", "nonce": n, "grid": g, "ksteps": k,
                 "launch_grid": {2: 3}.get(g, g)} for g, k, n in RAW_CASES]
    requests += [{"id": f"inj_{name}", "kernel": "datapath_mxgemm", "nonce": INJECT_NONCE, "grid": 2,
                  "ksteps": INJECT_KSTEPS, "code_object": "inject", **({"inject": inj} if inj else {})}
                 for name, inj in INJECTIONS.items()]
    (work / "requests.json").write_text(json.dumps(requests))
    probe = [str(probe_executable("hsa")), "--datapath-mxgemm", "--timeout", "10", "--devices"]
    s = Steps(work)
    s.run("raw", [sys.executable, "-m", "rocm_k8s_device_plugin_amd.testing.raw_kernels", str(work / "requests.json"),
                  str(work / "out")], 120)
    s.run("probe", probe + ["0"], 60)
    for spec in CORRUPT:
        s.run(f"corrupt_{spec}", probe + ["0", "--corrupt-datapath-mxgemm", spec], 60)
    s.run("hip", [str(probe_executable("hip")), "--datapath-mxgemm", "--devices", "0", "--nonce", "7100"], 60)
    s.run("serve", [probe[0], "--serve", "--keep"], 60, stdin=SERVE_INPUT)
    s.run("binding", [sys.executable, "-c", BINDING], 120)
    return s


def _compare(steps, rid, want_rec, want):
    folds, words = db.compare_raw(steps.load(rid, "records"), steps.load(rid, "tiles"), want_rec, want)
    _canaries_intact(steps, rid)                                       # records and tiles
    for name in ("a", "b", "sa", "sb"):
        assert (steps.load(rid, f"{name}.canary") == raw_kernels.CANARY_FILL).all(), (rid, name)
    print(f"{rid}: {len(folds)} fold words and {len(words)} D words differ; first {folds[:6]} {words[:8]}")
    assert folds == [] and words == []


@pytest.mark.parametrize("grid,ksteps,nonce", RAW_CASES)
def test_records_folds_operands_and_tiles_equal_the_reference_image(steps, grid, ksteps, nonce):
    rid = _rid(grid, ksteps, nonce)
    filled = b"".join(steps.load(rid, name).tobytes() for name in ("a", "b", "sa", "sb"))
    assert filled == db.operand_bytes(grid, nonce, ksteps)
    _compare(steps, rid, *db.healthy(grid, nonce, ksteps))


@pytest.mark.parametrize("name", list(INJECTIONS))
def test_each_hook_changes_what_it_should_and_nothing_else(steps, name):
    want_rec, want = db.healthy(2, INJECT_NONCE, INJECT_KSTEPS)
    if INJECTIONS[name]:
        clean = want_rec[1].copy(), want[1].copy()
        want_rec[1], want[1] = db.injected(INJECTIONS[name]["kind"], INJECT_NONCE, 1, INJECT_KSTEPS, INJECTIONS[name])
        # the words the prediction moves: a code's row or column whole; of a scale block's 64 words those whose
        # block sum is not zero
        changed = int((want_rec[1] != clean[0]).sum()), int((want[1] != clean[1]).sum())
        folds, words = {"mfma": (0, 1), "lds_a": (4, 128), "lds_b": (4, 128), "hbm": (4, 128), "scale": (2, 64)}[name]
        assert changed[0] == folds and (changed[1] == words or name == "scale" and words // 2 < changed[1] <= words)
    _compare(steps, f"inj_{name}", want_rec, want)                     # workgroup 0 untouched, workgroup 1 as predicted


def _device(steps, name, rc, box=None):
    """The child's device object; `box`: its figures go to $MI355X_BOX_DIR/datapath_mxgemm_box.json, recorded, not asserted."""
    out = steps.get(name).out
    assert steps.get(name).rc == rc, (steps.get(name).rc, out[-2000:], steps.get(name).err[-2000:])
    doc = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1 if box != "kept_queue" else 2])
    d = doc["devices"][0] if "devices" in doc else doc
    assert "devices" not in doc or (doc["datapath_mxgemm"] is True and "datapath" not in doc and doc["ok"] is (rc == 0))
    if box:
        path = Path(os.environ.get("MI355X_BOX_DIR") or steps.work) / "datapath_mxgemm_box.json"
        path.parent.mkdir(parents=True, exist_ok=True)
        keys = "grid ksteps cu_count kept_queue fill_us kernel_us verify_us total_us cus_covered simds_covered xccs_covered"
        figures = {k: d[k] for k in keys.split()}
        figures["gemm_tflops"] = 2 * 128 * 128 * 256 * d["ksteps"] * d["grid"] / d["kernel_us"] / 1e6
        path.write_text(json.dumps({**(json.loads(path.read_text()) if path.exists() else {}), box: figures}, indent=1) + "\n")
    return d


@pytest.mark.parametrize("name,box", [("probe", "production_grid"), ("serve", "kept_queue"), ("binding", None)])
def test_check_passes_one_shot_on_the_kept_queue_and_through_the_binding(steps, name, box):
    d = _device(steps, name, 0, box)
    assert d["ok"] is True and d["records_ok"] == d["grid"] == d["cu_count"] > 0 and d["error"] == "", d
    assert d["mfma_bad"] == 0 and list(d["stage_bad"]) == [0] * 4 and d["tile_bad"] == 0 and d["ksteps"] == db.KSTEPS, d
    assert d["kept_queue"] == (name == "serve") and d["nonce"] == {"serve": 102, "binding": 0xDEADBEEF}.get(name, d["nonce"])


@pytest.mark.parametrize("spec", CORRUPT)
def test_probe_names_stage_word_and_bit_of_an_injected_flip(steps, spec):
    stage, word, bit = (int(x) for x in spec.split(":"))
    d = _device(steps, f"corrupt_{spec}", 1)
    assert d["ok"] is False and d["records_ok"] == d["grid"] - 1 and list(d["stage_bad"]) == [int(s == stage) for s in range(4)], d
    assert (d["first_bad_wg"], d["first_bad_stage"], d["first_bad_word"], d["first_bad_xor"]) == (
        word // (16384 if stage == 3 else 16), stage, word, 1 << bit), d
    assert f"stage {stage} word {word} xor 0x{1 << bit:08x} (bit {bit})" in d["error"], d["error"]


def test_the_hip_entry_point_refuses_and_serve_mode_leaves_the_neighbours_replies_as_they_were(steps):
    d = _device(steps, "hip", 1)
    assert d["nonce"] == 7100 and d["error"] == "--datapath-mxgemm needs the HSA-direct build (mi355x-liveness-probe)", d
    hello, first, check, f32, after = (json.loads(ln) for ln in steps.get("serve").out.splitlines() if ln.startswith("{"))
    assert f32["datapath"] is True and "datapath_mxgemm" not in f32 and f32["ok"] is True, f32
    for reply, nonce in ((first, 101), (after, 104)):
        assert reply["devices"][0]["ok"] and reply["devices"][0]["nonce"] == nonce, reply

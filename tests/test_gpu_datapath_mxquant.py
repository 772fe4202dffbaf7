"""The MX quantise check on a real MI355X. A module fixture runs the child processes in order, each under its own
timeout, and starts nothing further after one ended abnormally (test_gpu_datapath_f16.Steps). One slab is the prologue
only, two use both W1 buffers and all four op_sel bytes, three reuse the first with the scale prefetch wrapping; grid 2
launched with 3 workgroups covers the panel offsets and the `wg >= grid` guard, with canaries around all seven buffers.
Nothing is compared with a tolerance."""
import json
import os
import sys
from pathlib import Path

import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import datapath_mxquant_reference as db
from rocm_k8s_device_plugin_amd.testing import raw_kernels

from test_gpu_datapath_f16 import Steps, _canaries_intact      # the children's runner and the canary check

pytestmark = pytest.mark.gpu

RAW_CASES = [(1, 1, 0xFFFFFFFF), (1, 2, 0xDEADBEEF), (1, 3, 0xDEADBEEF), (2, 2, 0xFFFFFFFF)]
# the inject build at grid 2, two slabs, each hook on workgroup 1. `h` sets bit 2 of the exponent field of one
# accumulator word (x 16): the block's amax crosses four binades. (changed fold words, image dwords, Y words):
INJECT_NONCE, INJECT_HSTEPS = 0xDEADBEEF, 2
INJECTIONS = {"h": (dict(kind="h", wg=1, wave=2, lane=39, index=1 * 64 + 1 * 16 + 5, mask=1 << 25), (4, 5, 128)),
              "q": (dict(kind="q", wg=1, step=1, index=777, mask=1 << 13), (0, 1, 128)),
              "scale": (dict(kind="scale", wg=1, wave=1, lane=40, index=1 * 8 + 0 * 4 + 0, mask=1 << 16), (2, 0, 64)),
              "scale_w2": (dict(kind="scale", wg=1, wave=2, lane=5, index=0 * 8 + 1 * 4 + 3, mask=1 << 8), (2, 0, 64)),
              "mfma": (dict(kind="mfma", wg=1, wave=2, lane=37, index=1 * 16 + 6, mask=1 << 30), (0, 0, 1)),
              "off": (None, (0, 0, 0))}
CORRUPT = ("0:5:31", "1:18:0", f"2:{db.img_words(db.HSTEPS) + 8191}:9", "3:16383:20")
SERVE_INPUT = "probe 4 10 0:101\ndatapath_mxquant 10 0:102\ndatapath 10 0:103\nprobe 4 10 0:104\nquit\n"
BINDING = ("import json; from rocm_k8s_device_plugin_amd.ops.native import hip; "
           "print(json.dumps(hip().hsa_datapath_mxquant_check(0, 3735928559, 10.0)))")
OPERANDS = ("x", "w1", "w2", "sb")


def _rid(grid, hsteps, nonce):
    return f"dpmq_{grid}_{hsteps}_{nonce:08x}"


@pytest.fixture(scope="module")
def steps(tmp_path_factory):
    from rocm_k8s_device_plugin_amd.ops.native import probe_executable
    work = tmp_path_factory.mktemp("datapath_mxquant")
    requests = [{"id": _rid(g, h, n), "kernel": "datapath_mxquant", "nonce": n, "grid": g, "hsteps": h,
                 "launch_grid": {2: 3}.get(g, g)} for g, h, n in RAW_CASES]
    requests += [{"id": f"inj_{name}", "kernel": "datapath_mxquant", "nonce": INJECT_NONCE, "grid": 2,
                  "hsteps": INJECT_HSTEPS, "code_object": "inject", **({"inject": inj} if inj else {})}
                 for name, (inj, _) in INJECTIONS.items()]
    (work / "requests.json").write_text(json.dumps(requests))
    probe = [str(probe_executable("hsa")), "--datapath-mxquant", "--timeout", "10", "--devices"]
    s = Steps(work)
    s.run("raw", [sys.executable, "-m", "rocm_k8s_device_plugin_amd.testing.raw_kernels", str(work / "requests.json"),
                  str(work / "out")], 120)
    s.run("probe", probe + ["0"], 60)
    for spec in CORRUPT:
        s.run(f"corrupt_{spec}", probe + ["0", "--corrupt-datapath-mxquant", spec], 60)
    s.run("hip", [str(probe_executable("hip")), "--datapath-mxquant", "--devices", "0", "--nonce", "7100"], 60)
    s.run("serve", [probe[0], "--serve", "--keep"], 60, stdin=SERVE_INPUT)
    s.run("binding", [sys.executable, "-c", BINDING], 120)
    return s


def _compare(steps, rid, want):
    folds, dwords, words = db.compare_raw(*(steps.load(rid, name) for name in ("records", "image", "tiles")), *want)
    _canaries_intact(steps, rid)                                       # records and tiles
    for name in ("image",) + OPERANDS:
        assert (steps.load(rid, f"{name}.canary") == raw_kernels.CANARY_FILL).all(), (rid, name)
    print(f"{rid}: {len(folds)} fold words, {len(dwords)} image dwords and {len(words)} Y words differ; first "
          f"{folds[:6]} {dwords[:8]} {words[:8]}")
    assert folds == [] and dwords == [] and words == []


@pytest.mark.parametrize("grid,hsteps,nonce", RAW_CASES)
def test_operands_records_image_and_tiles_equal_the_reference(steps, grid, hsteps, nonce):
    rid = _rid(grid, hsteps, nonce)
    assert b"".join(steps.load(rid, name).tobytes() for name in OPERANDS) == db.operand_bytes(grid, nonce, hsteps)
    _compare(steps, rid, db.healthy(grid, nonce, hsteps))


@pytest.mark.parametrize("name", list(INJECTIONS))
def test_each_hook_changes_what_it_should_and_nothing_else(steps, name):
    inj, moved = INJECTIONS[name]
    want = db.healthy(2, INJECT_NONCE, INJECT_HSTEPS)
    if inj:
        clean = [part[1].copy() for part in want]
        bad = db.injected(inj["kind"], INJECT_NONCE, 1, INJECT_HSTEPS, inj)
        changed = tuple(int((b != c).sum()) for b, c in zip(bad, clean))
        # of a scale block's 64 Y words those whose block sum is not zero move
        assert changed == moved or name.startswith("scale") and changed[:2] == moved[:2] and 32 < changed[2] <= 64, changed
        if name == "h":                                                # the block's scale byte and all its code dwords
            token, block = 32 * inj["wave"] + (inj["lane"] & 31), inj["index"] // 16
            at = np.flatnonzero(bad[1] != clean[1]).tolist()
            assert at == [token * 16 * INJECT_HSTEPS + 4 * block + d for d in range(4)] + [
                2048 * INJECT_HSTEPS + token * INJECT_HSTEPS + block // 4]
            codes = (bad[1][at[:4]][:, None] >> (4 * np.arange(8))) & 15, (clean[1][at[:4]][:, None] >> (4 * np.arange(8))) & 15
            assert ((codes[0] != codes[1]).sum() == 32) and (bad[2] != clean[2]).reshape(128, 128)[token].all()
        for part, b in zip(want, bad):
            part[1] = b
    _compare(steps, f"inj_{name}", want)                               # workgroup 0 untouched, workgroup 1 as predicted


def _device(steps, name, rc, box=None):
    """The child's device object; `box`: its figures go to $MI355X_BOX_DIR/datapath_mxquant_box.json, recorded, not asserted."""
    out = steps.get(name).out
    assert steps.get(name).rc == rc, (steps.get(name).rc, out[-2000:], steps.get(name).err[-2000:])
    doc = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1 if box != "kept_queue" else 2])
    d = doc["devices"][0] if "devices" in doc else doc
    assert "devices" not in doc or (doc["datapath_mxquant"] is True and "datapath" not in doc and doc["ok"] is (rc == 0))
    if box:
        path = Path(os.environ.get("MI355X_BOX_DIR") or steps.work) / "datapath_mxquant_box.json"
        path.parent.mkdir(parents=True, exist_ok=True)
        keys = "grid hsteps cu_count kept_queue fill_us kernel_us verify_us total_us cus_covered simds_covered xccs_covered"
        figures = {k: d[k] for k in keys.split()}
        path.write_text(json.dumps({**(json.loads(path.read_text()) if path.exists() else {}), box: figures}, indent=1) + "\n")
    return d


@pytest.mark.parametrize("name,box", [("probe", "production_grid"), ("serve", "kept_queue"), ("binding", None)])
def test_check_passes_one_shot_on_the_kept_queue_and_through_the_binding(steps, name, box):
    d = _device(steps, name, 0, box)
    assert d["ok"] is True and d["records_ok"] == d["grid"] == d["cu_count"] > 0 and d["error"] == "", d
    assert d["mfma_bad"] == 0 and list(d["stage_bad"]) == [0] * 4 and d["tile_bad"] == 0 and d["hsteps"] == db.HSTEPS, d
    assert d["kept_queue"] == (name == "serve") and d["nonce"] == {"serve": 102, "binding": 0xDEADBEEF}.get(name, d["nonce"])


@pytest.mark.parametrize("spec", CORRUPT)
def test_probe_names_stage_word_and_bit_of_an_injected_flip(steps, spec):
    stage, word, bit = (int(x) for x in spec.split(":"))
    d = _device(steps, f"corrupt_{spec}", 1)
    assert d["ok"] is False and d["records_ok"] == d["grid"] - 1 and list(d["stage_bad"]) == [int(s == stage) for s in range(4)], d
    assert (d["first_bad_wg"], d["first_bad_stage"], d["first_bad_word"], d["first_bad_xor"]) == (
        word // {2: db.img_words(db.HSTEPS), 3: 16384}.get(stage, 16), stage, word, 1 << bit), d
    assert f"stage {stage} word {word} xor 0x{1 << bit:08x} (bit {bit})" in d["error"], d["error"]


def test_the_hip_entry_point_refuses_and_serve_mode_leaves_the_neighbours_replies_as_they_were(steps):
    d = _device(steps, "hip", 1)
    assert d["nonce"] == 7100 and d["error"] == "--datapath-mxquant needs the HSA-direct build (mi355x-liveness-probe)", d
    hello, first, check, f32, after = (json.loads(ln) for ln in steps.get("serve").out.splitlines() if ln.startswith("{"))
    assert f32["datapath"] is True and "datapath_mxquant" not in f32 and f32["ok"] is True, f32
    for reply, nonce in ((first, 101), (after, 104)):
        assert reply["devices"][0]["ok"] and reply["devices"][0]["nonce"] == nonce, reply

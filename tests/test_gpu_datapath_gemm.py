"""The bf16 GEMM pipeline check on a real MI355X. A module fixture runs the child processes in order, each under its
own timeout, and starts nothing further after one ended abnormally (test_gpu_datapath_f16.Steps). One k-step has no
loop-carried state, two use both LDS buffers, three wrap to the first; grid 3 launched with 5 workgroups covers the
per-workgroup strides and the `wg >= grid` guard, with canaries around all four buffers."""
import json
import os
import sys
from pathlib import Path

import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import datapath_gemm_reference as db
from rocm_k8s_device_plugin_amd.testing import raw_kernels

from test_gpu_datapath_f16 import Steps, _canaries_intact      # the children's runner and the canary check

pytestmark = pytest.mark.gpu

RAW_CASES = [(g, k, n) for g, k in ((1, 1), (1, 2), (1, 3), (3, 3)) for n in (0xFFFFFFFF, 0xDEADBEEF)]
# the inject build at grid 2, three k-steps, each hook on workgroup 1. Every mask is mantissa bit 6 of the low element
# of a dword: the element stays one of the recipe's, so the wrong D is still exact and the reference predicts it.
INJECT_NONCE, INJECT_KSTEPS, BIT = 0xDEADBEEF, 3, 0x0040
INJECTIONS = {"mfma": dict(kind="mfma", wg=1, wave=2, lane=37, index=1 * 16 + 6, mask=1 << 30),
              "lds_a": dict(kind="lds", wg=1, step=1, index=1234, mask=BIT),
              "lds_b": dict(kind="lds", wg=1, step=2, index=4096 + 2999, mask=BIT),
              "hbm": dict(kind="hbm", wg=1, index=101 * INJECT_KSTEPS * 64 + 70, mask=BIT),
              "off": None}
CORRUPT = ("0:5:31", "1:2:0", "2:16383:20")
SERVE_INPUT = "probe 4 10 0:101\ndatapath_gemm 10 0:102\ndatapath 10 0:103\nprobe 4 10 0:104\nquit\n"
BINDING = ("import json; from rocm_k8s_device_plugin_amd.ops.native import hip; "
           "print(json.dumps(hip().hsa_datapath_gemm_check(0, 3735928559, 10.0)))")


def _rid(grid, ksteps, nonce):
    return f"dpgm_{grid}_{ksteps}_{nonce:08x}"


@pytest.fixture(scope="module")
def steps(tmp_path_factory):
    from rocm_k8s_device_plugin_amd.ops.native import probe_executable
    work = tmp_path_factory.mktemp("datapath_gemm")
    requests = [{"id": _rid(g, k, n), "kernel": "datapath_gemm", "nonce": n, "grid": g, "ksteps": k,
                 "launch_grid": {3: 5}.get(g, g)} for g, k, n in RAW_CASES]
    requests += [{"id": f"inj_{name}", "kernel": "datapath_gemm", "nonce": INJECT_NONCE, "grid": 2,
                  "ksteps": INJECT_KSTEPS, "code_object": "inject", **({"inject": inj} if inj else {})}
                 for name, inj in INJECTIONS.items()]
    (work / "requests.json").write_text(json.dumps(requests))
    probe = [str(probe_executable("hsa")), "--datapath-gemm", "--timeout", "10", "--devices"]
    s = Steps(work)
    s.run("raw", [sys.executable, "-m", "rocm_k8s_device_plugin_amd.testing.raw_kernels", str(work / "requests.json"),
                  str(work / "out")], 120)
    s.run("probe", probe + ["0"], 60)
    for spec in CORRUPT:
        s.run(f"corrupt_{spec}", probe + ["0", "--corrupt-datapath-gemm", spec], 60)
    s.run("no_gpu", probe + ["99", "--nonce", "7000"], 60)
    s.run("hip", [str(probe_executable("hip")), "--datapath-gemm", "--devices", "0", "--nonce", "7100"], 60)
    s.run("serve", [probe[0], "--serve", "--keep"], 60, stdin=SERVE_INPUT)
    s.run("binding", [sys.executable, "-c", BINDING], 120)
    return s


def _all_canaries_intact(steps, rid):
    _canaries_intact(steps, rid)                                       # records and tiles
    for name in ("a", "b"):
        assert (steps.load(rid, f"{name}.canary") == raw_kernels.CANARY_FILL).all(), (rid, name)


@pytest.mark.parametrize("grid,ksteps,nonce", RAW_CASES)
def test_records_folds_operands_and_tiles_equal_the_reference_image(steps, grid, ksteps, nonce):
    rid = _rid(grid, ksteps, nonce)
    folds, words = db.compare_raw(steps.load(rid, "records"), steps.load(rid, "tiles"), nonce, grid, ksteps)
    _all_canaries_intact(steps, rid)                                   # every byte but where it ran, and none beyond
    filled = steps.load(rid, "a").tobytes() + steps.load(rid, "b").tobytes()
    assert filled == db.operand_bytes(grid, nonce, ksteps)
    print(f"{rid}: {len(folds)} fold words and {len(words)} D words differ; first {folds[:4]} {words[:8]}")
    assert folds == [] and words == []


@pytest.mark.parametrize("name", list(INJECTIONS))
def test_each_hook_changes_what_it_should_and_nothing_else(steps, name):
    inj, K = INJECTIONS[name], INJECT_KSTEPS * 64
    got_rec = steps.load(f"inj_{name}", "records").reshape(2, db.REC_WORDS)
    got = steps.load(f"inj_{name}", "tiles").reshape(2, db.WG_WORDS)
    want_rec, want = db.healthy(2, INJECT_NONCE, INJECT_KSTEPS)
    a, b = db.a_elements(INJECT_NONCE, 1, INJECT_KSTEPS).copy(), db.b_elements(INJECT_NONCE, INJECT_KSTEPS).copy()
    rows, cols = slice(0, 128), slice(0, 128)                          # where D may differ
    if name == "mfma":                                                 # accumulator 1 = row block 0, column block 1
        r, lane = inj["index"] % 16, inj["lane"]
        word = (64 * (inj["wave"] >> 1) + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * 128 + 64 * (inj["wave"] & 1) + 32 + (lane & 31)
        want[1, word] ^= inj["mask"]
    elif name in ("lds_a", "lds_b", "hbm"):
        if name == "hbm":
            which, row, k = "a", inj["index"] // K, inj["index"] % K
        else:                                                          # the element the swizzle put at that LDS dword
            which, x, y = db.lds_source(inj["index"])
            row, k, col = (x, 64 * inj["step"] + y, None) if which == "a" else (None, 64 * inj["step"] + x, y)
        assert which == {"lds_a": "a", "lds_b": "b", "hbm": "a"}[name]
        if which == "a":
            a[row, k] ^= BIT
            rows = slice(row, row + 1)
        else:
            b[k, col] ^= BIT
            cols = slice(col, col + 1)
        want[1] = db.f32_words(db.integers(INJECT_NONCE, 1, INJECT_KSTEPS, a=a, b=b), db.qx(INJECT_NONCE, 1)).reshape(-1)
        want_rec[1, db.REC_FOLD:] = db.folds(INJECT_NONCE, 1, INJECT_KSTEPS, a=a, b=b)
        clean = db.healthy(2, INJECT_NONCE, INJECT_KSTEPS)
        outside = np.ones((128, 128), dtype=bool)
        outside[rows, cols] = False
        assert (want[1].reshape(128, 128) != clean[1][1].reshape(128, 128))[rows, cols].any()
        assert (want[1].reshape(128, 128) == clean[1][1].reshape(128, 128))[outside].all()
        assert (want_rec[1] != clean[0][1]).sum() == 4                 # xor and sum of the two waves that read it
    keep = [db.REC_MAGIC, db.REC_WG, db.REC_NONCE, db.REC_KSTEPS] + list(range(db.REC_FOLD, db.REC_WORDS))
    assert np.argwhere(got_rec[:, keep] != want_rec[:, keep]).tolist() == []
    assert np.argwhere(got != want).tolist() == []                     # workgroup 0 untouched, workgroup 1 as predicted


def _device(steps, name, rc, box=None):
    """The child's device object; `box`: its figures go to $MI355X_BOX_DIR/datapath_gemm_box.json, recorded, not asserted."""
    out = steps.get(name).out
    assert steps.get(name).rc == rc, (steps.get(name).rc, out[-2000:], steps.get(name).err[-2000:])
    doc = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1 if box != "kept_queue" else 2])
    d = doc["devices"][0] if "devices" in doc else doc
    assert "devices" not in doc or (doc["datapath_gemm"] is True and "datapath" not in doc and doc["ok"] is (rc == 0))
    if box:
        path = Path(os.environ.get("MI355X_BOX_DIR") or steps.work) / "datapath_gemm_box.json"
        path.parent.mkdir(parents=True, exist_ok=True)
        keys = "grid ksteps cu_count kept_queue fill_us kernel_us verify_us total_us cus_covered simds_covered xccs_covered"
        figures = {k: d[k] for k in keys.split()}
        figures["gemm_tflops"] = 2 * 128 * 128 * 64 * d["ksteps"] * d["grid"] / d["kernel_us"] / 1e6
        path.write_text(json.dumps({**(json.loads(path.read_text()) if path.exists() else {}), box: figures}, indent=1) + "\n")
    return d


@pytest.mark.parametrize("name,box", [("probe", "production_grid"), ("serve", "kept_queue"), ("binding", None)])
def test_check_passes_one_shot_on_the_kept_queue_and_through_the_binding(steps, name, box):
    d = _device(steps, name, 0, box)
    assert d["ok"] is True and d["records_ok"] == d["grid"] == d["cu_count"] > 0 and d["error"] == "", d
    assert d["mfma_bad"] == 0 and list(d["stage_bad"]) == [0] * 3 and d["tile_bad"] == 0 and d["ksteps"] == db.KSTEPS, d
    assert d["kept_queue"] == (name == "serve") and d["nonce"] == {"serve": 102, "binding": 0xDEADBEEF}.get(name, d["nonce"])


@pytest.mark.parametrize("spec", CORRUPT)
def test_probe_names_stage_word_and_bit_of_an_injected_flip(steps, spec):
    stage, word, bit = (int(x) for x in spec.split(":"))
    d = _device(steps, f"corrupt_{spec}", 1)
    assert d["ok"] is False and d["records_ok"] == d["grid"] - 1 and list(d["stage_bad"]) == [int(s == stage) for s in range(3)], d
    assert (d["first_bad_wg"], d["first_bad_stage"], d["first_bad_word"], d["first_bad_xor"]) == (0, stage, word, 1 << bit)
    assert f"stage {stage} word {word} xor 0x{1 << bit:08x} (bit {bit})" in d["error"], d["error"]


def test_an_ordinal_past_the_gpus_and_the_hip_entry_point_reach_no_device(steps):
    d = _device(steps, "no_gpu", 1)
    assert d["ordinal"] == 99 and d["error"].startswith("no such GPU (count=") and d["stage_bad"] == [0] * 3, d
    assert d["first_bad_wg"] == d["first_bad_stage"] == d["first_bad_word"] == -1 and d["kept_queue"] is False, d
    d = _device(steps, "hip", 1)
    assert d["nonce"] == 7100 and d["error"] == "--datapath-gemm needs the HSA-direct build (mi355x-liveness-probe)", d


def test_serve_mode_leaves_the_neighbours_replies_as_they_were(steps):
    hello, first, check, f32, after = (json.loads(ln) for ln in steps.get("serve").out.splitlines() if ln.startswith("{"))
    assert f32["datapath"] is True and "datapath_gemm" not in f32 and f32["ok"] is True, f32
    assert f32["devices"][0]["nonce"] == 103 and len(f32["devices"][0]["stage_bad"]) == 4, f32
    for reply, nonce in ((first, 101), (after, 104)):
        assert reply["devices"][0]["ok"] and reply["devices"][0]["nonce"] == nonce, reply
        assert sorted(reply) == ["devices", "hip_device_count", "ok", "perf", "sweep", "t_ready_ns"]

"""The split-K GEMM check on a real MI355X. A module fixture runs the child processes in order, each under its own
timeout, and starts nothing further after one ended abnormally (test_gpu_datapath_f16.Steps). (1, 1, 1) is one add per
word onto C with no loop state; (1, 2, 2) has two contributors to every word and uses both LDS buffers; (1, 3, 3) an odd
split count and the buffer wrap; (2, 8, 1), launched with 19 workgroups for 16, the tile strides, eight contributors
across XCDs and the `wg >= grid` guard; canaries around all seven buffers."""
import json
import os
import sys
from pathlib import Path

import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import datapath_gemm_reference as dg
from rocm_k8s_device_plugin_amd.testing import datapath_splitk_reference as ds
from rocm_k8s_device_plugin_amd.testing import raw_kernels

from test_gpu_datapath_f16 import Steps, _canaries_intact      # the children's runner and the canary check

pytestmark = pytest.mark.gpu

RAW_CASES = [(t, s, k, n) for t, s, k in ((1, 1, 1), (1, 2, 2), (1, 3, 3), (2, 8, 1)) for n in (0xFFFFFFFF, 0xDEADBEEF)]
# the inject build at (2, 2, 2), each hook on workgroup 3 (tile 1, split 1). The mask is the sign bit: the addend stays
# a whole number of quanta, so the wrong D is still exact and the reference predicts it.
INJECT_SIZES, INJECT_NONCE = (2, 2, 2), 0xDEADBEEF
INJECTIONS = {"atomic": dict(kind="atomic", wg=3, wave=2, lane=37, index=23, mask=1 << 31),
              "drop": dict(kind="drop", wg=3, wave=1, lane=58, index=60),
              "off": None}
CORRUPT = ("0:13:31", "2:278533:30", "3:8:0")        # a fold word of workgroup 1, a D word of tile 17, arrivals of tile 1
SERVE_INPUT = "probe 4 10 0:101\ndatapath_splitk 10 0:102\ndatapath 10 0:103\nprobe 4 10 0:104\nquit\n"
BINDING = ("import json; from rocm_k8s_device_plugin_amd.ops.native import hip; "
           "print(json.dumps(hip().hsa_datapath_splitk_check(0, 3735928559, 10.0)))")
BUFFERS = ("records", "tiles", "out_ledger", "a", "b", "d", "ledger")


def _rid(tiles, splits, ksteps, nonce):
    return f"dpsk_{tiles}_{splits}_{ksteps}_{nonce:08x}"


@pytest.fixture(scope="module")
def steps(tmp_path_factory):
    from rocm_k8s_device_plugin_amd.ops.native import probe_executable
    work = tmp_path_factory.mktemp("datapath_splitk")
    requests = [{"id": _rid(t, s, k, n), "kernel": "datapath_splitk", "nonce": n, "tiles": t, "splits": s, "ksteps": k,
                 "launch_grid": {16: 19}.get(t * s, t * s)} for t, s, k, n in RAW_CASES]
    requests += [{"id": f"inj_{name}", "kernel": "datapath_splitk", "nonce": INJECT_NONCE,
                  **dict(zip(("tiles", "splits", "ksteps"), INJECT_SIZES)), "code_object": "inject",
                  **({"inject": inj} if inj else {})} for name, inj in INJECTIONS.items()]
    (work / "requests.json").write_text(json.dumps(requests))
    probe = [str(probe_executable("hsa")), "--datapath-splitk", "--timeout", "10", "--devices"]
    s = Steps(work)
    s.run("raw", [sys.executable, "-m", "rocm_k8s_device_plugin_amd.testing.raw_kernels", str(work / "requests.json"),
                  str(work / "out")], 120)
    s.run("probe", probe + ["0"], 60)
    for spec in CORRUPT:
        s.run(f"corrupt_{spec}", probe + ["0", "--corrupt-datapath-splitk", spec], 60)
    s.run("no_gpu", probe + ["99", "--nonce", "7000"], 60)
    s.run("hip", [str(probe_executable("hip")), "--datapath-splitk", "--devices", "0", "--nonce", "7100"], 60)
    s.run("serve", [probe[0], "--serve", "--keep"], 60, stdin=SERVE_INPUT)
    s.run("binding", [sys.executable, "-c", BINDING], 120)
    return s


def _compare(steps, rid, sizes, nonce, want=None):
    """The three difference lists of compare_raw; all canaries, and the drain's copies against what it copied."""
    got = {name: steps.load(rid, name) for name in BUFFERS}
    _canaries_intact(steps, rid)                                       # records and tiles
    for name in BUFFERS[2:]:
        assert (steps.load(rid, f"{name}.canary") == raw_kernels.CANARY_FILL).all(), (rid, name)
    assert got["d"].tobytes() == got["tiles"].tobytes() and got["ledger"].tobytes() == got["out_ledger"].tobytes()
    filled = got["a"].tobytes() + got["b"].tobytes()
    assert filled == dg.operand_bytes(sizes[0], nonce, sizes[1] * sizes[2])   # the GEMM check's operand bytes
    return ds.compare_raw(got["records"], got["tiles"], got["out_ledger"], *sizes, nonce, want)


@pytest.mark.parametrize("tiles,splits,ksteps,nonce", RAW_CASES)
def test_records_operands_tiles_and_ledgers_equal_the_reference_image(steps, tiles, splits, ksteps, nonce):
    rid = _rid(tiles, splits, ksteps, nonce)
    folds, words, ledger = _compare(steps, rid, (tiles, splits, ksteps), nonce)
    print(f"{rid}: {len(folds)} fold, {len(words)} D and {len(ledger)} ledger words differ; first {folds[:4]} {words[:8]} {ledger[:8]}")
    assert folds == [] and words == [] and ledger == []


@pytest.mark.parametrize("name", list(INJECTIONS))
def test_each_hook_changes_one_d_word_as_predicted_and_nothing_else(steps, name):
    inj, (tiles, splits, ksteps) = INJECTIONS[name], INJECT_SIZES
    want = ds.healthy(*INJECT_SIZES, INJECT_NONCE)
    if inj:
        tile, split = divmod(inj["wg"], splits)
        word = ds.acc_word(inj["wave"], inj["lane"], inj["index"])
        addend = int(ds.partial(INJECT_NONCE, tile, splits, ksteps, split).reshape(-1)[word])
        assert addend != 0
        n = ds.integers(INJECT_NONCE, tile, splits, ksteps).reshape(-1).copy()
        n[word] -= 2 * addend if name == "atomic" else addend          # the sign flipped, or the add left out
        want[1][tile] = dg.f32_words(n, dg.qx(INJECT_NONCE, tile).reshape(-1))
        assert (want[1] != ds.healthy(*INJECT_SIZES, INJECT_NONCE)[1]).sum() == 1
    assert _compare(steps, f"inj_{name}", INJECT_SIZES, INJECT_NONCE, want) == ([], [], [])   # ledgers included


def _device(steps, name, rc, box=None):
    """The child's device object; `box`: its figures go to $MI355X_BOX_DIR/datapath_splitk_box.json, recorded, not asserted."""
    out = steps.get(name).out
    assert steps.get(name).rc == rc, (steps.get(name).rc, out[-2000:], steps.get(name).err[-2000:])
    doc = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1 if box != "kept_queue" else 2])
    d = doc["devices"][0] if "devices" in doc else doc
    assert "devices" not in doc or (doc["datapath_splitk"] is True and "datapath" not in doc and doc["ok"] is (rc == 0))
    if box:
        path = Path(os.environ.get("MI355X_BOX_DIR") or steps.work) / "datapath_splitk_box.json"
        path.parent.mkdir(parents=True, exist_ok=True)
        keys = ("grid tiles splits ksteps cu_count kept_queue fill_us kernel_us drain_us verify_us total_us cus_covered "
                "simds_covered xccs_covered xccs_per_tile_min")
        figures = {k: d[k] for k in keys.split()}
        figures["f32_atomics_per_us"] = d["grid"] * ds.TILE_WORDS / d["kernel_us"]
        path.write_text(json.dumps({**(json.loads(path.read_text()) if path.exists() else {}), box: figures}, indent=1) + "\n")
    return d


@pytest.mark.parametrize("name,box", [("probe", "production_grid"), ("serve", "kept_queue"), ("binding", None)])
def test_check_passes_one_shot_on_the_kept_queue_and_through_the_binding(steps, name, box):
    d = _device(steps, name, 0, box)
    assert d["ok"] is True and d["records_ok"] == d["tiles"] == d["cu_count"] // 8 > 0 and d["error"] == "", d
    assert d["grid"] == d["tiles"] * d["splits"] and (d["splits"], d["ksteps"]) == (ds.SPLITS, ds.KSTEPS), d
    assert d["mfma_bad"] == 0 and list(d["stage_bad"]) == [0] * 4 and d["tile_bad"] == d["ledger_bad"] == 0, d
    assert d["kept_queue"] == (name == "serve") and d["nonce"] == {"serve": 102, "binding": 0xDEADBEEF}.get(name, d["nonce"])
    assert 1 <= d["xccs_per_tile_min"] <= d["xccs_covered"], d            # reported, not required


@pytest.mark.parametrize("spec", CORRUPT)
def test_probe_names_stage_word_and_bit_of_an_injected_flip(steps, spec):
    stage, word, bit = (int(x) for x in spec.split(":"))
    d = _device(steps, f"corrupt_{spec}", 1)
    tile = {0: word // 8 // ds.SPLITS, 2: word // ds.TILE_WORDS, 3: word // 8}[stage]
    assert d["ok"] is False and d["records_ok"] == d["tiles"] - 1 and list(d["stage_bad"]) == [int(s == stage) for s in range(4)], d
    assert (d["first_bad_wg"], d["first_bad_stage"], d["first_bad_word"], d["first_bad_xor"]) == (tile, stage, word, 1 << bit)
    assert f"tile {tile} stage {stage} word {word} xor 0x{1 << bit:08x} (bit {bit})" in d["error"], d["error"]


def test_an_ordinal_past_the_gpus_and_the_hip_entry_point_reach_no_device(steps):
    d = _device(steps, "no_gpu", 1)
    assert d["ordinal"] == 99 and d["error"].startswith("no such GPU (count=") and d["stage_bad"] == [0] * 4, d
    assert d["first_bad_wg"] == d["first_bad_stage"] == d["first_bad_word"] == -1 and d["kept_queue"] is False, d
    d = _device(steps, "hip", 1)
    assert d["nonce"] == 7100 and d["error"] == "--datapath-splitk needs the HSA-direct build (mi355x-liveness-probe)", d


def test_serve_mode_leaves_the_neighbours_replies_as_they_were(steps):
    hello, first, check, f32, after = (json.loads(ln) for ln in steps.get("serve").out.splitlines() if ln.startswith("{"))
    assert f32["datapath"] is True and "datapath_splitk" not in f32 and f32["ok"] is True, f32
    assert f32["devices"][0]["nonce"] == 103 and len(f32["devices"][0]["stage_bad"]) == 4, f32
    for reply, nonce in ((first, 101), (after, 104)):
        assert reply["devices"][0]["ok"] and reply["devices"][0]["nonce"] == nonce, reply
        assert sorted(reply) == ["devices", "hip_device_count", "ok", "perf", "sweep", "t_ready_ns"]

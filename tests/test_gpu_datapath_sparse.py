"""The sparse (2:4) MFMA datapath check on a real MI355X. A module fixture runs the child processes in order,
each under its own timeout, and starts nothing further after one ended abnormally (test_gpu_datapath_f16.Steps).
Grid 1 gives four wave nonces, all ten stages; grid 3 launched with 5 workgroups covers
the indexing, the strides and the `wg >= grid` guard, with canaries behind both buffers."""
import json
import os
import sys
from pathlib import Path

import pytest

from rocm_k8s_device_plugin_amd.testing import datapath_sparse_reference as db

from test_gpu_datapath_f16 import Steps, _canaries_intact      # the children's runner and the canary check

pytestmark = pytest.mark.gpu

RAW_CASES = [(g, n) for g in (1, 3) for n in (0xFFFFFFFF, 0xDEADBEEF)]
# the inject build at grid 2, one wrong word in workgroup 1: (wave, lane, index = stage * 16 + accumulator register,
# bit). Every stage and wave, the 16x16 stages' last register, a register they do not have, and the hook off.
INJECT_NONCE = 0xDEADBEEF
INJECTIONS = {"stage0": (0, 37, 0 * 16 + 13, 0), "stage1": (1, 0, 1 * 16 + 6, 31), "stage2": (2, 63, 2 * 16 + 15, 19),
              "stage3": (3, 32, 3 * 16 + 9, 7), "stage4": (0, 49, 4 * 16 + 3, 30), "stage5": (1, 18, 5 * 16 + 0, 12),
              "stage6": (2, 27, 6 * 16 + 2, 23), "stage7": (0, 62, 7 * 16 + 11, 3), "stage8": (3, 1, 8 * 16 + 0, 16),
              "stage9": (0, 20, 9 * 16 + 5, 27), "no_register": (0, 5, 8 * 16 + 4, 30), "off": None}
INJECTIONS = {k: v and dict(kind="mfma", wg=1, wave=v[0], lane=v[1], index=v[2], mask=1 << v[3])
              for k, v in INJECTIONS.items()}
CORRUPT = ("0:1023:31", "4:255:0", "7:513:20")
SERVE_INPUT = "probe 4 10 0:101\ndatapath_sparse 10 0:102\ndatapath 10 0:103\nprobe 4 10 0:104\nquit\n"
BINDING = ("import json; from rocm_k8s_device_plugin_amd.ops.native import hip; "
           "print(json.dumps(hip().hsa_datapath_sparse_check(0, 3735928559, 10.0)))")


@pytest.fixture(scope="module")
def steps(tmp_path_factory):
    from rocm_k8s_device_plugin_amd.ops.native import probe_executable
    work = tmp_path_factory.mktemp("datapath_sparse")
    requests = [{"id": f"dpsp_{g}_{n:08x}", "kernel": "datapath_sparse", "nonce": n, "grid": g,
                 "launch_grid": {3: 5}.get(g, g)} for g, n in RAW_CASES]
    requests += [{"id": f"inj_{name}", "kernel": "datapath_sparse", "nonce": INJECT_NONCE, "grid": 2,
                  "code_object": "inject", **({"inject": inj} if inj else {})} for name, inj in INJECTIONS.items()]
    (work / "requests.json").write_text(json.dumps(requests))
    probe = [str(probe_executable("hsa")), "--datapath-sparse", "--timeout", "10", "--devices"]
    s = Steps(work)
    s.run("raw", [sys.executable, "-m", "rocm_k8s_device_plugin_amd.testing.raw_kernels", str(work / "requests.json"),
                  str(work / "out")], 120)
    s.run("probe", probe + ["0"], 60)
    for spec in CORRUPT:
        s.run(f"corrupt_{spec}", probe + ["0", "--corrupt-datapath-sparse", spec], 60)
    s.run("no_gpu", probe + ["99", "--nonce", "7000"], 60)
    s.run("hip", [str(probe_executable("hip")), "--datapath-sparse", "--devices", "0", "--nonce", "7100"], 60)
    s.run("serve", [probe[0], "--serve", "--keep"], 60, stdin=SERVE_INPUT)
    s.run("binding", [sys.executable, "-c", BINDING], 120)
    return s


@pytest.mark.parametrize("grid,nonce", RAW_CASES)
def test_records_and_tiles_equal_the_reference_image(steps, grid, nonce):
    rid = f"dpsp_{grid}_{nonce:08x}"
    bad, differing = db.compare_raw(steps.load(rid, "records"), steps.load(rid, "tiles"), nonce, grid)
    _canaries_intact(steps, rid)                                       # every byte but where it ran, and none beyond
    assert not bad.any() and differing == []


@pytest.mark.parametrize("name", list(INJECTIONS))
def test_injected_word_is_counted_once_in_its_stage_and_workgroup(steps, name):
    tiles = steps.load(f"inj_{name}", "tiles").reshape(2, db.WG_WORDS)
    bad, differing = db.compare_raw(steps.load(f"inj_{name}", "records"), tiles, INJECT_NONCE, 2)
    inj, hits = INJECTIONS[name], name not in ("no_register", "off")
    stage = inj["index"] // 16 if hits else -1
    assert bad.tolist() == [[0] * 10, [int(s == stage) for s in range(10)]]
    assert len(differing) == (1 if hits and inj["wave"] == 0 else 0)              # only wave 0's tile is stored
    for wg, w in differing:                                                      # there: that stage, exactly the mask
        assert wg == 1 and 0 <= w - db.TILE_OFFSET[stage] < db.STAGE_WORDS[stage]
        assert int(tiles[wg, w]) ^ int(db.tiles_image(INJECT_NONCE, 2)[wg, w]) == inj["mask"]


def _device(steps, name, rc, box=None):
    """The child's device object; `box`: its figures go to $MI355X_BOX_DIR/datapath_sparse_box.json, recorded, not asserted."""
    out = steps.get(name).out
    assert steps.get(name).rc == rc, (steps.get(name).rc, out[-2000:], steps.get(name).err[-2000:])
    doc = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1 if box != "kept_queue" else 2])
    d = doc["devices"][0] if "devices" in doc else doc
    assert "devices" not in doc or (doc["datapath_sparse"] is True and "datapath" not in doc and doc["ok"] is (rc == 0))
    if box:
        path = Path(os.environ.get("MI355X_BOX_DIR") or steps.work) / "datapath_sparse_box.json"
        path.parent.mkdir(parents=True, exist_ok=True)
        keys = "grid cu_count kept_queue kernel_us total_us cus_covered simds_covered xccs_covered"
        figures = {k: d[k] for k in keys.split()}
        path.write_text(json.dumps({**(json.loads(path.read_text()) if path.exists() else {}), box: figures}, indent=1) + "\n")
    return d


@pytest.mark.parametrize("name,box", [("probe", "production_grid"), ("serve", "kept_queue"), ("binding", None)])
def test_check_passes_one_shot_on_the_kept_queue_and_through_the_binding(steps, name, box):
    d = _device(steps, name, 0, box)
    assert d["ok"] is True and d["records_ok"] == d["grid"] == d["cu_count"] > 0 and d["error"] == "", d
    assert d["mfma_bad"] == 0 and list(d["stage_bad"]) == [0] * 10 and d["tile_bad"] == 0, d
    assert d["kept_queue"] == (name == "serve") and d["nonce"] == {"serve": 102, "binding": 0xDEADBEEF}.get(name, d["nonce"])


@pytest.mark.parametrize("spec", CORRUPT)
def test_probe_names_stage_word_and_bit_of_an_injected_flip(steps, spec):
    stage, word, bit = (int(x) for x in spec.split(":"))
    d = _device(steps, f"corrupt_{spec}", 1)
    assert d["ok"] is False and d["tile_bad"] == 1 and d["records_ok"] == d["grid"] - 1, d
    assert (d["first_bad_wg"], d["first_bad_stage"], d["first_bad_word"], d["first_bad_xor"]) == (0, stage, word, 1 << bit)
    assert f"stage {stage} word {word} xor 0x{1 << bit:08x} (bit {bit})" in d["error"], d["error"]


def test_an_ordinal_past_the_gpus_and_the_hip_entry_point_reach_no_device(steps):
    d = _device(steps, "no_gpu", 1)
    assert d["ordinal"] == 99 and d["error"].startswith("no such GPU (count=") and d["stage_bad"] == [0] * 10, d
    assert d["first_bad_wg"] == d["first_bad_stage"] == d["first_bad_word"] == -1 and d["kept_queue"] is False, d
    d = _device(steps, "hip", 1)
    assert d["nonce"] == 7100 and d["error"] == "--datapath-sparse needs the HSA-direct build (mi355x-liveness-probe)", d


def test_serve_mode_leaves_the_neighbours_replies_as_they_were(steps):
    hello, first, check, f32, after = (json.loads(ln) for ln in steps.get("serve").out.splitlines() if ln.startswith("{"))
    assert f32["datapath"] is True and "datapath_sparse" not in f32 and f32["ok"] is True, f32
    assert f32["devices"][0]["nonce"] == 103 and len(f32["devices"][0]["stage_bad"]) == 4, f32
    for reply, nonce in ((first, 101), (after, 104)):
        assert reply["devices"][0]["ok"] and reply["devices"][0]["nonce"] == nonce, reply
        assert sorted(reply) == ["devices", "hip_device_count", "ok", "perf", "sweep", "t_ready_ns"]

"""The fused attention check on a real MI355X. A module fixture runs the child processes in order, each under its own
timeout, and starts nothing further after one ended abnormally (test_gpu_datapath_f16.Steps). (1, 1, 1) is one block
with no rescale and no buffer swap: the case that settles the lane maps; (1, 1, 2) uses both LDS buffers and a real
rescale; (1, 1, 3) an odd count and the buffer wrap; (2, 2, 2), launched with 5 workgroups for 4, the head strides, two
workgroups sharing K and V and the `wg >= grid` guard; canaries around all six buffers."""
import json
import os
import sys
from pathlib import Path

import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import datapath_attn_reference as da
from rocm_k8s_device_plugin_amd.testing import raw_kernels

from test_gpu_datapath_f16 import Steps, _canaries_intact      # the children's runner and the canary check

pytestmark = pytest.mark.gpu

RAW_CASES = [(h, q, k, n) for h, q, k in ((1, 1, 1), (1, 1, 2), (1, 1, 3), (2, 2, 2)) for n in (0xFFFFFFFF, 0xDEADBEEF)]
# the inject build at (2, 2, 2), each hook on workgroup 3 (head 1, query block 1). The mask is the sign bit: -S is still
# in -6..6 and -O still a whole number of quanta, so the reference predicts every changed word.
INJECT_SIZES, INJECT_NONCE = (2, 2, 2), 0xDEADBEEF
INJECTIONS = {"s": dict(kind="s", wg=3, wave=2, lane=37, index=32 + 16 + 9, mask=1 << 31),
              "o": dict(kind="o", wg=3, wave=1, lane=58, index=16 + 6, mask=1 << 31),
              "off": None}
CORRUPT = ("0:13:31", "2:4403:22", "3:139269:30")    # a fold word of workgroup 1, an l word and an O word of workgroup 17
SERVE_INPUT = "probe 4 10 0:101\ndatapath_attn 10 0:102\ndatapath 10 0:103\nprobe 4 10 0:104\nquit\n"
BINDING = ("import json; from rocm_k8s_device_plugin_amd.ops.native import hip; "
           "print(json.dumps(hip().hsa_datapath_attn_check(0, 3735928559, 10.0)))")
BUFFERS = ("records", "tiles", "ml", "q", "k", "v")


def _rid(heads, qblocks, kblocks, nonce):
    return f"dpat_{heads}_{qblocks}_{kblocks}_{nonce:08x}"


@pytest.fixture(scope="module")
def steps(tmp_path_factory):
    from rocm_k8s_device_plugin_amd.ops.native import probe_executable
    work = tmp_path_factory.mktemp("datapath_attn")
    requests = [{"id": _rid(h, q, k, n), "kernel": "datapath_attn", "nonce": n, "heads": h, "qblocks": q, "kblocks": k,
                 "launch_grid": {4: 5}.get(h * q, h * q)} for h, q, k, n in RAW_CASES]
    requests += [{"id": f"inj_{name}", "kernel": "datapath_attn", "nonce": INJECT_NONCE,
                  **dict(zip(("heads", "qblocks", "kblocks"), INJECT_SIZES)), "code_object": "inject",
                  **({"inject": inj} if inj else {})} for name, inj in INJECTIONS.items()]
    (work / "requests.json").write_text(json.dumps(requests))
    probe = [str(probe_executable("hsa")), "--datapath-attn", "--timeout", "10", "--devices"]
    s = Steps(work)
    s.run("raw", [sys.executable, "-m", "rocm_k8s_device_plugin_amd.testing.raw_kernels", str(work / "requests.json"),
                  str(work / "out")], 120)
    s.run("probe", probe + ["0"], 60)
    for spec in CORRUPT:
        s.run(f"corrupt_{spec}", probe + ["0", "--corrupt-datapath-attn", spec], 60)
    s.run("no_gpu", probe + ["99", "--nonce", "7000"], 60)
    s.run("hip", [str(probe_executable("hip")), "--datapath-attn", "--devices", "0", "--nonce", "7100"], 60)
    s.run("serve", [probe[0], "--serve", "--keep"], 60, stdin=SERVE_INPUT)
    s.run("binding", [sys.executable, "-c", BINDING], 120)
    return s


def _compare(steps, rid, sizes, nonce, want=None):
    """The three difference lists of compare_raw; all canaries, and the filled operands against the reference's bytes."""
    got = {name: steps.load(rid, name) for name in BUFFERS}
    _canaries_intact(steps, rid)                                       # records and tiles (O)
    for name in BUFFERS[2:]:
        assert (steps.load(rid, f"{name}.canary") == raw_kernels.CANARY_FILL).all(), (rid, name)
    assert tuple(got[name].tobytes() for name in "qkv") == da.operand_bytes(*sizes, nonce)
    return da.compare_raw(got["records"], got["ml"], got["tiles"], *sizes, nonce, want)


@pytest.mark.parametrize("heads,qblocks,kblocks,nonce", RAW_CASES)
def test_records_operands_stats_and_o_equal_the_reference_image(steps, heads, qblocks, kblocks, nonce):
    rid = _rid(heads, qblocks, kblocks, nonce)
    folds, stats, words = _compare(steps, rid, (heads, qblocks, kblocks), nonce)
    inexact = steps.load(rid, "records").reshape(-1, da.REC_WORDS)[:, da.REC_EXP_INEXACT].tolist()
    print(f"{rid}: exp_inexact {inexact}; {len(folds)} fold, {len(stats)} m / l and {len(words)} O words differ; "
          f"first {folds[:4]} {stats[:8]} {words[:8]}")
    assert folds == [] and stats == [] and words == []


@pytest.mark.parametrize("name", list(INJECTIONS))
def test_each_hook_changes_exactly_the_words_the_reference_predicts(steps, name):
    inj, (heads, qblocks, kblocks) = INJECTIONS[name], INJECT_SIZES
    want = da.healthy(*INJECT_SIZES, INJECT_NONCE)
    if name == "s":                                   # one score of the head negated: that query's whole row changes
        head, qb = divmod(inj["wg"], qblocks)
        query, key = da.s_word(inj["wave"], inj["lane"], inj["index"])

        def flipped(h):
            s = da.scores(INJECT_NONCE, h, qblocks, kblocks).copy()
            if h == head:
                assert s[qb * da.QBLOCK + query, key] != 0
                s[qb * da.QBLOCK + query, key] *= -1
            return s
        want = da.image_of(INJECT_NONCE, heads, qblocks, kblocks, flipped)
        changed = [np.argwhere(a != b)[:, 0].tolist() for a, b in zip(want[1:], da.healthy(*INJECT_SIZES, INJECT_NONCE)[1:])]
        assert set(changed[0]) <= {inj["wg"]} and set(changed[1]) == {inj["wg"]} and len(changed[1]) > 32
    elif name == "o":                                 # one O word's sign
        word = da.o_word(inj["wave"], inj["lane"], inj["index"])
        assert want[2][inj["wg"], word] != 0
        want[2][inj["wg"], word] ^= np.uint32(1 << 31)
    assert _compare(steps, f"inj_{name}", INJECT_SIZES, INJECT_NONCE, want) == ([], [], [])


def _device(steps, name, rc, box=None):
    """The child's device object; `box`: its figures go to $MI355X_BOX_DIR/datapath_attn_box.json, recorded, not asserted."""
    out = steps.get(name).out
    assert steps.get(name).rc == rc, (steps.get(name).rc, out[-2000:], steps.get(name).err[-2000:])
    doc = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1 if box != "kept_queue" else 2])
    d = doc["devices"][0] if "devices" in doc else doc
    assert "devices" not in doc or (doc["datapath_attn"] is True and "datapath" not in doc and doc["ok"] is (rc == 0))
    if box:
        path = Path(os.environ.get("MI355X_BOX_DIR") or steps.work) / "datapath_attn_box.json"
        path.parent.mkdir(parents=True, exist_ok=True)
        keys = ("grid heads qblocks kblocks cu_count kept_queue fill_us kernel_us verify_us total_us exp_inexact "
                "cus_covered simds_covered xccs_covered")
        figures = {k: d[k] for k in keys.split()}
        path.write_text(json.dumps({**(json.loads(path.read_text()) if path.exists() else {}), box: figures}, indent=1) + "\n")
    return d


@pytest.mark.parametrize("name,box", [("probe", "production_grid"), ("serve", "kept_queue"), ("binding", None)])
def test_check_passes_one_shot_on_the_kept_queue_and_through_the_binding(steps, name, box):
    d = _device(steps, name, 0, box)
    assert d["ok"] is True and d["records_ok"] == d["grid"] == d["heads"] * d["qblocks"] > 0 and d["error"] == "", d
    assert d["heads"] == d["cu_count"] // 4 and (d["qblocks"], d["kblocks"]) == (da.QBLOCKS, da.KBLOCKS), d
    assert d["mfma_bad"] == 0 and list(d["stage_bad"]) == [0] * 4 and d["tile_bad"] == 0, d
    assert d["kept_queue"] == (name == "serve") and d["nonce"] == {"serve": 102, "binding": 0xDEADBEEF}.get(name, d["nonce"])


@pytest.mark.parametrize("spec", CORRUPT)
def test_probe_names_stage_word_and_bit_of_an_injected_flip(steps, spec):
    stage, word, bit = (int(x) for x in spec.split(":"))
    d = _device(steps, f"corrupt_{spec}", 1)
    wg = word // {0: 8, 2: da.ML_WORDS, 3: da.O_WORDS}[stage]
    assert d["ok"] is False and d["records_ok"] == d["grid"] - 1 and list(d["stage_bad"]) == [int(s == stage) for s in range(4)], d
    assert (d["first_bad_wg"], d["first_bad_stage"], d["first_bad_word"], d["first_bad_xor"]) == (wg, stage, word, 1 << bit)
    assert f"workgroup {wg} stage {stage} word {word} xor 0x{1 << bit:08x} (bit {bit})" in d["error"], d["error"]


def test_an_ordinal_past_the_gpus_and_the_hip_entry_point_reach_no_device(steps):
    d = _device(steps, "no_gpu", 1)
    assert d["ordinal"] == 99 and d["error"].startswith("no such GPU (count=") and d["stage_bad"] == [0] * 4, d
    assert d["first_bad_wg"] == d["first_bad_stage"] == d["first_bad_word"] == -1 and d["kept_queue"] is False, d
    d = _device(steps, "hip", 1)
    assert d["nonce"] == 7100 and d["error"] == "--datapath-attn needs the HSA-direct build (mi355x-liveness-probe)", d


def test_serve_mode_leaves_the_neighbours_replies_as_they_were(steps):
    hello, first, check, f32, after = (json.loads(ln) for ln in steps.get("serve").out.splitlines() if ln.startswith("{"))
    assert f32["datapath"] is True and "datapath_attn" not in f32 and f32["ok"] is True, f32
    assert f32["devices"][0]["nonce"] == 103 and len(f32["devices"][0]["stage_bad"]) == 4, f32
    for reply, nonce in ((first, 101), (after, 104)):
        assert reply["devices"][0]["ok"] and reply["devices"][0]["nonce"] == nonce, reply
        assert sorted(reply) == ["devices", "hip_device_count", "ok", "perf", "sweep", "t_ready_ns"]

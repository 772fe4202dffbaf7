"""testing/stub_probe.py against mi355x-liveness-probe on a real MI355X: one
transcript through one `--serve --keep` session of the HSA probe and through
the stub, reply by reply, and the one-shot form of each of the five kinds.

The real replies are written to probe_contract_box.json in $MI355X_BOX_DIR
(default: the test's temporary directory) before anything is asserted, with
times and nonces left in and nothing judged; profiles/probe_contract_box.json
is a copy from an MI355X, which tests/test_probe_contract.py holds the stub to
on machines without a GPU.

The session has a 60 s limit of its own, is never retried and is killed in any
case; the one-shot processes run one after another, and none is started after
one that ended abnormally."""
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
STUB = REPO / "rocm_k8s_device_plugin_amd" / "testing" / "stub_probe.py"
# (request line, kind or None for a line the server refuses, ordinal, nonce)
TRANSCRIPT = [
    ("probe 1 10 0:1", "probe", 0, 1),
    ("@5 probe 4 10 0:2", "probe", 0, 2),
    ("sweep 1 10 0:3", "sweep", 0, 3),
    ("perf 1024 10 64 0:4", "perf", 0, 4),             # 64 MiB: the smallest buffer accepted
    ("datapath 10 0:5", "datapath", 0, 5),
    ("datapath_i8 10 0:6", "datapath_i8", 0, 6),
    ("probe 4 10 99:7", "probe", 99, 7),               # no such agent
    ("nonsense", None, None, None),
    ("probe 4 10 0:8", "probe", 0, 8),
]
ONESHOT = {"probe": ["--devices", "0", "--nonce", "9", "--iters", "4", "--timeout", "10"],
           "sweep": ["--sweep", "--devices", "0", "--nonce", "9", "--iters", "1", "--timeout", "10"],
           "perf": ["--perf", "--perf-mib", "64", "--perf-iters", "1024", "--devices", "0", "--nonce", "9", "--timeout", "10"],
           "datapath": ["--datapath", "--devices", "0", "--nonce", "9", "--timeout", "10"],
           "datapath_i8": ["--datapath-i8", "--devices", "0", "--nonce", "9", "--timeout", "10"]}
BAD_REQUEST = {"ok": False, "error": "bad request", "devices": []}
ABNORMAL = (124, 134, 137, 139)


def shape(v):
    """Keys in order with the JSON type of each value; an array by the types of its elements."""
    if isinstance(v, bool):
        return "bool"
    if isinstance(v, (int, float)):
        return "number"
    if isinstance(v, str):
        return "string"
    if v is None:
        return "null"
    if isinstance(v, list):
        return ["array", sorted({json.dumps(shape(x)) for x in v})]
    return [[k, shape(x)] for k, x in v.items()]


def envelope(doc):
    return {k: ([] if k == "devices" else v) for k, v in doc.items()}


def session(argv, env=None):
    """One serve session over the transcript: (exit status, hello, replies in
    request order). A tagged request is answered on a worker thread, so its
    reply may come after a later one's: it is found by its id."""
    text = "".join(line + "\n" for line, _, _, _ in TRANSCRIPT) + "quit\n"
    p = subprocess.Popen(argv, cwd=REPO, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         env=env)
    try:
        out, err = p.communicate(text, timeout=60)
    finally:
        if p.poll() is None:
            p.kill()
            p.wait()
    docs = [json.loads(ln) for ln in out.splitlines()]
    assert docs, (p.returncode, err[-3000:])
    hello, docs = docs[0], docs[1:]
    tagged = [d for d in docs if "id" in d]
    rest = [d for d in docs if "id" not in d]
    ordered = [(tagged.pop(0) if tagged else None) if line.startswith("@") else (rest.pop(0) if rest else None)
               for line, _, _, _ in TRANSCRIPT]
    return p.returncode, hello, ordered, err


def stub_env():
    env = {k: v for k, v in os.environ.items() if not k.startswith("MI355X_STUB_")}
    env.pop("ROCR_VISIBLE_DEVICES", None)
    return env


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from rocm_k8s_device_plugin_amd.ops.native import probe_executable
    probe = str(probe_executable("hsa"))
    t0 = time.monotonic()
    rc, hello, replies, err = session([probe, "--serve", "--keep"])
    real = {"serve_rc": rc, "hello": hello, "serve": replies, "serve_stderr": err[-2000:], "oneshot": {},
            "oneshot_rc": {}}
    if rc == 0:
        for kind, args in ONESHOT.items():
            try:
                p = subprocess.run([probe, *args], cwd=REPO, capture_output=True, text=True, timeout=60)
            except subprocess.TimeoutExpired:
                real["oneshot_rc"][kind] = "timeout"
                break
            real["oneshot_rc"][kind] = p.returncode
            if p.returncode < 0 or p.returncode in ABNORMAL:
                break                                   # nothing more on a GPU that just faulted
            real["oneshot"][kind] = json.loads(p.stdout.splitlines()[-1])
    real["wall_s"] = time.monotonic() - t0
    box = {"hello": hello, "wall_s": round(real["wall_s"], 3),
           "serve": [{"request": line, "kind": kind, "reply": reply} for (line, kind, _, _), reply in
                     zip(TRANSCRIPT, replies)],
           "oneshot": real["oneshot"]}
    box_dir = Path(os.environ.get("MI355X_BOX_DIR") or tmp_path_factory.mktemp("probe_contract"))
    box_dir.mkdir(parents=True, exist_ok=True)
    (box_dir / "probe_contract_box.json").write_text(json.dumps(box, indent=1) + "\n")

    src, shello, sreplies, _ = session([sys.executable, str(STUB), "--serve", "--keep"], env=stub_env())
    stub = {"serve_rc": src, "hello": shello, "serve": sreplies, "oneshot": {}}
    for kind, args in ONESHOT.items():
        p = subprocess.run([sys.executable, str(STUB), *args], capture_output=True, text=True, timeout=60, env=stub_env())
        stub["oneshot"][kind] = json.loads(p.stdout.splitlines()[-1])
    return real, stub


def test_the_session_ran_to_its_end(run):
    real, stub = run
    assert real["serve_rc"] == 0 and stub["serve_rc"] == 0, real["serve_stderr"]
    assert all(r is not None for r in real["serve"]) and all(r is not None for r in stub["serve"])
    assert real["oneshot_rc"] == dict.fromkeys(ONESHOT, 0), real["oneshot_rc"]
    assert shape(real["hello"]) == shape(stub["hello"]) and real["hello"]["ok"] is True


def test_reply_by_reply_the_stub_has_the_probes_keys_order_and_types(run):
    real, stub = run
    for (line, kind, _, _), r, s in zip(TRANSCRIPT, real["serve"], stub["serve"]):
        assert list(r) == list(s), (line, list(r), list(s))
        assert shape(envelope(r)) == shape(envelope(s)), line
        assert len(r["devices"]) == len(s["devices"]) == (0 if kind is None else 1), line
        for a, b in zip(r["devices"], s["devices"]):
            assert list(a) == list(b), (line, list(a), list(b))
            assert shape(a) == shape(b), line
        assert ("id" in r) == line.startswith("@")
        if kind is not None:
            assert r["sweep"] is (kind == "sweep") and r["perf"] is (kind == "perf"), line
            assert [k for k in ("datapath", "datapath_i8") if k in r] == [k for k in (kind,) if k.startswith("datapath")]


def test_nonces_and_ordinals_are_echoed(run):
    real, stub = run
    for (line, kind, ordinal, nonce), r, s in zip(TRANSCRIPT, real["serve"], stub["serve"]):
        if kind is None:
            continue
        (d,), (e,) = r["devices"], s["devices"]
        assert d["ordinal"] == e["ordinal"] == ordinal, line
        if ordinal == 99:       # the reply never reached a device: no nonce, no agent, and the stub says the same
            assert r["ok"] is False and d["ok"] is False and d["error"].startswith("no such GPU"), d
            assert {k: v for k, v in d.items() if k != "error"} == {k: v for k, v in e.items() if k != "error"}
        else:
            assert r["ok"] is True and d["ok"] is True and d["nonce"] == e["nonce"] == nonce, (line, d)
    assert real["serve"][1]["id"] == stub["serve"][1]["id"] == 5


def test_a_bad_line_is_refused_and_the_next_request_answered(run):
    real, stub = run
    lines = [line for line, _, _, _ in TRANSCRIPT]
    at = lines.index("nonsense")
    assert real["serve"][at] == stub["serve"][at] == BAD_REQUEST
    assert real["serve"][at + 1]["ok"] is True and real["serve"][at + 1]["devices"][0]["nonce"] == 8


def test_every_check_reply_names_the_agent_the_probe_reply_names(run):
    real, _ = run
    probe = real["serve"][0]["devices"][0]
    assert probe["pci_bus_id"] and probe["kfd_node_id"] >= 0, probe
    for (line, kind, ordinal, _), r in zip(TRANSCRIPT, real["serve"]):
        if kind is not None and ordinal == 0:
            d = r["devices"][0]
            assert (d["pci_bus_id"], d["kfd_node_id"]) == (probe["pci_bus_id"], probe["kfd_node_id"]), (line, d)
    for kind, doc in real["oneshot"].items():
        d = doc["devices"][0]
        assert (d["pci_bus_id"], d["kfd_node_id"]) == (probe["pci_bus_id"], probe["kfd_node_id"]), (kind, d)


def test_one_shot_documents_have_the_stubs_envelope(run):
    real, stub = run
    for kind in ONESHOT:
        r, s = real["oneshot"][kind], stub["oneshot"][kind]
        assert list(r) == list(s), (kind, list(r), list(s))
        assert shape(envelope(r)) == shape(envelope(s)), kind
        (a,), (b,) = r["devices"], s["devices"]
        assert list(a) == list(b) and shape(a) == shape(b), kind
        assert r["ok"] is True and a["nonce"] == b["nonce"] == 9, (kind, a)

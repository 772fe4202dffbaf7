"""The datapath_f16 kind of testing/stub_probe.py against mi355x-liveness-probe
on a real MI355X, as tests/test_gpu_probe_contract.py does for the other five
kinds (which keeps them): one short transcript through one `--serve --keep`
session of the HSA probe and through the stub, and the one-shot form.

The real replies are written to probe_contract_f16_box.json in
$MI355X_BOX_DIR (default: the test's temporary directory) before anything is
asserted; tests/golden/probe_contract_f16_box.json is a copy from an MI355X,
which tests/test_probe_contract_f16.py holds the stub and the printers to on
machines without a GPU.

The session has a 60 s limit of its own, is never retried and is killed in any
case; the one-shot process is not started after a session that ended abnormally."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

from test_gpu_probe_contract import ABNORMAL, BAD_REQUEST, REPO, STUB, envelope, shape, stub_env

pytestmark = pytest.mark.gpu

# (request line, kind or None for a line the server refuses, ordinal, nonce)
TRANSCRIPT = [
    ("probe 1 10 0:1", "probe", 0, 1),
    ("datapath_f16 10 0:2", "datapath_f16", 0, 2),
    ("@5 datapath_f16 10 0:3", "datapath_f16", 0, 3),
    ("datapath_f16 10 99:4", "datapath_f16", 99, 4),      # no such agent
    ("datapath_f1610 0:5", None, None, None),
    ("datapath_i8 10 0:6", "datapath_i8", 0, 6),
]
ONESHOT = ["--datapath-f16", "--devices", "0", "--nonce", "9", "--timeout", "10"]


def session(argv, env=None):
    """(exit status, hello, replies in request order, stderr); requests go one at a
    time, so a tagged reply cannot overtake."""
    p = subprocess.Popen(argv, cwd=REPO, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         env=env)
    try:
        out, err = p.communicate("".join(line + "\n" for line, _, _, _ in TRANSCRIPT) + "quit\n", timeout=60)
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


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from rocm_k8s_device_plugin_amd.ops.native import probe_executable
    probe = str(probe_executable("hsa"))
    rc, hello, replies, err = session([probe, "--serve", "--keep"])
    real = {"serve_rc": rc, "hello": hello, "serve": replies, "serve_stderr": err[-2000:], "oneshot": None,
            "oneshot_rc": None}
    if rc == 0:
        try:
            p = subprocess.run([probe, *ONESHOT], cwd=REPO, capture_output=True, text=True, timeout=60)
            real["oneshot_rc"] = p.returncode
            if p.returncode >= 0 and p.returncode not in ABNORMAL:
                real["oneshot"] = json.loads(p.stdout.splitlines()[-1])
        except subprocess.TimeoutExpired:
            real["oneshot_rc"] = "timeout"
    box = {"hello": hello,
           "serve": [{"request": line, "kind": kind, "reply": reply} for (line, kind, _, _), reply in
                     zip(TRANSCRIPT, replies)],
           "oneshot": {"datapath_f16": real["oneshot"]}}
    box_dir = Path(os.environ.get("MI355X_BOX_DIR") or tmp_path_factory.mktemp("probe_contract_f16"))
    box_dir.mkdir(parents=True, exist_ok=True)
    (box_dir / "probe_contract_f16_box.json").write_text(json.dumps(box, indent=1) + "\n")

    src, shello, sreplies, _ = session([sys.executable, str(STUB), "--serve", "--keep"], env=stub_env())
    p = subprocess.run([sys.executable, str(STUB), *ONESHOT], capture_output=True, text=True, timeout=60, env=stub_env())
    return real, {"serve_rc": src, "hello": shello, "serve": sreplies, "oneshot": json.loads(p.stdout.splitlines()[-1])}


def test_the_session_ran_to_its_end(run):
    real, stub = run
    assert real["serve_rc"] == 0 and stub["serve_rc"] == 0, real["serve_stderr"]
    assert all(r is not None for r in real["serve"]) and all(r is not None for r in stub["serve"])
    assert real["oneshot_rc"] == 0
    assert shape(real["hello"]) == shape(stub["hello"]) and real["hello"]["ok"] is True


def test_reply_by_reply_the_stub_has_the_probes_keys_order_and_types(run):
    real, stub = run
    for (line, kind, ordinal, nonce), r, s in zip(TRANSCRIPT, real["serve"], stub["serve"]):
        assert list(r) == list(s), (line, list(r), list(s))
        assert shape(envelope(r)) == shape(envelope(s)), line
        assert len(r["devices"]) == len(s["devices"]) == (0 if kind is None else 1), line
        for a, b in zip(r["devices"], s["devices"]):
            assert list(a) == list(b) and shape(a) == shape(b), (line, list(a), list(b))
        assert ("id" in r) == line.startswith("@")
        if kind is None:
            assert r == s == BAD_REQUEST
            continue
        # only this kind's reply carries its key
        assert [k for k in ("datapath", "datapath_i8", "datapath_f16") if k in r] == \
            [k for k in (kind,) if k.startswith("datapath")], line
        (d,), (e,) = r["devices"], s["devices"]
        assert d["ordinal"] == e["ordinal"] == ordinal, line
        if ordinal == 99:       # the reply never reached a device: no agent, and the stub says the same
            assert r["ok"] is False and d["ok"] is False and d["error"].startswith("no such GPU"), d
            assert {k: v for k, v in d.items() if k != "error"} == {k: v for k, v in e.items() if k != "error"}
        else:
            assert r["ok"] is True and d["ok"] is True and d["nonce"] == e["nonce"] == nonce, (line, d)
    assert real["serve"][2]["id"] == stub["serve"][2]["id"] == 5


def test_the_check_runs_on_the_kept_queue_and_names_the_probes_agent(run):
    real, _ = run
    probe = real["serve"][0]["devices"][0]
    for r in real["serve"][1:3]:
        d = r["devices"][0]
        assert r["datapath_f16"] is True and d["kept_queue"] is True and len(d["stage_bad"]) == 7, d
        assert d["records_ok"] == d["grid"] == d["cu_count"] > 0 and d["tile_bad"] == 0 and d["mfma_bad"] == 0, d
        assert (d["pci_bus_id"], d["kfd_node_id"]) == (probe["pci_bus_id"], probe["kfd_node_id"]), d


def test_one_shot_document_has_the_stubs_envelope(run):
    real, stub = run
    r, s = real["oneshot"], stub["oneshot"]
    assert list(r) == list(s), (list(r), list(s))
    assert shape(envelope(r)) == shape(envelope(s))
    (a,), (b,) = r["devices"], s["devices"]
    assert list(a) == list(b) and shape(a) == shape(b)
    assert r["ok"] is True and r["datapath_f16"] is True and a["nonce"] == b["nonce"] == 9, a

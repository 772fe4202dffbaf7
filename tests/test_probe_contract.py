"""testing/stub_probe.py against the program it stands in for, CPU only.

Every CPU test of the health engine, the daemon, the Python monitor and the
PreStart gate talks to the stub, so the stub must say what
mi355x-liveness-probe says. The real wire format is reached without a GPU
through native/tests/probe_contract_cli.cpp: `replies` prints what the
printers of native/src/health/probe_json.h give, `parse` what
native/src/health/probe_request.h makes of a request line.

* the printers' bytes are pinned (tests/golden/probe_contract_replies.json, and
  the format strings probe_main.cpp held before they moved);
* every stub reply has the real reply's keys, order and JSON types, in every mode;
* every stub fault mode carries the figures and the error text the shipped
  verdict gives for that fault (testing/probe_contract.py builds the records);
* one corpus of request lines goes through the real parser and the stub's;
* a recording from an MI355X (profiles/probe_contract_box.json), when there is
  one, is held to the same shapes.
"""
import json
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest

from rocm_k8s_device_plugin_amd.testing import contract_cli, probe_contract, stub_probe

REPO = Path(__file__).resolve().parent.parent
STUB = REPO / "rocm_k8s_device_plugin_amd" / "testing" / "stub_probe.py"
GOLDEN = REPO / "tests" / "golden" / "probe_contract_replies.json"
BEFORE = REPO / "tests" / "golden" / "probe_contract_checks_before.json"
BOX = REPO / "profiles" / "probe_contract_box.json"
KINDS = ("probe", "sweep", "perf", "datapath", "datapath_i8")
CHECKS = KINDS[1:]


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return contract_cli.probe_contract_cli(tmp_path_factory.mktemp("probe_contract_cli"))


@pytest.fixture(scope="module")
def replies_text(cli):
    return contract_cli.probe_replies_text(cli)


@pytest.fixture(scope="module")
def replies(replies_text):
    return json.loads(replies_text)


# ---- shapes ------------------------------------------------------------------------------------
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


def envelope_shape(doc):
    return shape({k: ([] if k == "devices" else v) for k, v in doc.items()})


def check_lengths(kind, d):
    """The length rule of a reply's arrays."""
    per = min(16, d["num_xcc"] if d.get("num_xcc", 0) > 0 else 8)
    if kind == "sweep":
        assert len(d["wgs_per_xcc"]) == per, d
    if kind == "perf":
        assert len(d["xcd_clock_mhz"]) == per, d
    if kind == "datapath":
        assert len(d["stage_bad"]) == 4, d
    if kind == "datapath_i8":
        assert len(d["stage_bad"]) == 5, d


def same_device_shape(kind, got, real, what):
    assert [k for k in got] == [k for k in real], (what, "keys or their order")
    assert shape(got) == shape(real), what
    check_lengths(kind, got)


def test_the_printers_obey_their_own_length_rule(replies):
    for kind in CHECKS:
        blank, f8, f16 = (replies["devices"][kind][k] for k in ("blank", "filled8", "filled16"))
        assert shape(f8) == shape(f16) and [k for k in blank] == [k for k in f8]
        assert (f8["num_xcc"], f16["num_xcc"], blank["num_xcc"]) == (8, 16, 0)
        for d in (blank, f8, f16):
            check_lengths(kind, d)
        assert blank["kfd_node_id"] == -1 and blank["pci_bus_id"] == ""      # never reached a device
        assert f8["error"] == 'a "quoted" back\\slash'
        numbers = [v for k, v in f8.items() if shape(v) == "number" and k != "num_xcc"]
        numbers += [x for v in f8.values() if isinstance(v, list) for x in v]
        assert 0 not in numbers and len(set(numbers)) == len(numbers), kind    # a swapped argument would show


# ---- the printers' bytes -----------------------------------------------------------------------
def test_replies_are_the_recorded_bytes(replies_text):
    """Any change to a printer (a renamed key, another precision, another order) shows here first."""
    assert replies_text == GOLDEN.read_text()


# probe_main.cpp's format strings before they moved into probe_json.h
OLD_PROBE = ("{\"ordinal\":%d,\"ok\":%s,\"hip_error\":%d,\"mismatches\":%d,\"nonce\":%u,\"xcc_id\":%u,"
             "\"hw_id\":%u,\"iters\":%d,\"dispatches\":%d,\"kfd_node_id\":%d,\"runtime\":\"%s\","
             "\"kernel_us\":%.3f,\"setup_us\":%.3f,\"total_us\":%.3f,"
             "\"phase_us\":{PHASES},"
             "\"pci_bus_id\":\"%s\","
             "\"arch\":\"%s\",\"name\":\"%s\",\"uuid\":\"%s\",\"pci_domain\":%d,\"pci_bus\":%d,"
             "\"pci_device\":%d,\"cu_count\":%d,\"total_mem\":%llu,\"late\":%s,\"pending_s\":%.3f,\"error\":\"%s\"}")
OLD_PHASES = {"probe": "\"code_object\":%.1f,\"queue\":%.1f,\"buffers\":%.1f,\"dispatch_wait\":%.1f",
              "probe_hip": "\"device\":%.1f,\"stream\":%.1f,\"buffers\":%.1f,\"dispatch_wait\":%.1f"}
OLD_HELLO = ("{\"serve\":true,\"ok\":%s,\"hip_device_count\":%d,\"concurrent\":%s,\"deadlines\":true,"
             "\"t_start_ns\":%llu,\"t_runtime_ns\":%llu}")
OLD_SERVE_HEAD = "{%s\"ok\":%s,\"hip_device_count\":%d,\"sweep\":%s,\"perf\":%s,\"t_ready_ns\":%llu,"
OLD_ONESHOT_CHECK = ("{\"ok\":%s,\"%s\":true,\"hip_device_count\":%d,\"t_start_ns\":%llu,\"t_runtime_ns\":%llu,"
                     "\"t_ready_ns\":%llu,\"devices\":%s}")
OLD_ONESHOT_PROBE = (
    "{\"ok\":%s,\"hip_device_count\":%d,\"identify\":%s,\"t_start_ns\":%llu,\"t_runtime_ns\":%llu,"
    "\"t_ready_ns\":%llu,\"cpu_ms_runtime\":%.2f,\"cpu_user_ms_runtime\":%.2f,\"cpu_ms_ready\":%.2f,\"read_syscalls_runtime\":%lld,"
    "\"init_us\":{\"dlopen\":%.1f,\"kfd_open\":%.1f,\"hsa_init\":%.1f,\"agents\":%.1f,\"pools\":%.1f},\"init_profile\":%s,"
    "\"view\":%s,\"devices\":%s}")
OLD_INIT_FAILED = ("{\"ok\":false,\"hip_device_count\":0,\"error\":\"GPU runtime init failed (%d)\",\"devices\":[],"
                   "\"t_start_ns\":%llu,\"t_ready_ns\":0,\"init_profile\":%s}")
T0, T1, T2 = 1000000001, 1000000002, 1000000003          # probe_contract_cli's clock


def c_format(fmt, *values):
    return fmt.replace("%llu", "%d").replace("%lld", "%d").replace("%u", "%d") % values


def test_the_probe_reply_is_byte_identical_to_before_the_move(replies_text, replies):
    for build in ("probe", "probe_hip"):
        line = next(ln for ln in replies_text.split("\n") if ln.startswith(f'"{build}":{{"blank":'))
        f = replies["devices"][build]["filled8"]
        ph = list(f["phase_us"].values())
        want = c_format(OLD_PROBE.replace("PHASES", OLD_PHASES[build]), f["ordinal"], "true", f["hip_error"],
                        f["mismatches"], f["nonce"], f["xcc_id"], f["hw_id"], f["iters"], f["dispatches"],
                        f["kfd_node_id"], "hsa", f["kernel_us"], f["setup_us"], f["total_us"], *ph, f["pci_bus_id"],
                        f["arch"], f["name"], f["uuid"], f["pci_domain"], f["pci_bus"], f["pci_device"], f["cu_count"],
                        f["total_mem"], "true", f["pending_s"], 'a \\"quoted\\" back\\\\slash')
        assert f',"filled8":{want},' in line, build
        zeros = c_format(OLD_PROBE.replace("PHASES", OLD_PHASES[build]), 0, "false", 0, 0, 0, 0, 0, 0, 0, 0, "", 0.0,
                         0.0, 0.0, 0.0, 0.0, 0.0, 0.0, "", "", "", "", 0, 0, 0, 0, 0, "false", 0.0, "")
        assert line.startswith(f'"{build}":{{"blank":{zeros},'), build


def test_hello_and_envelopes_are_byte_identical_to_before_the_move(replies_text):
    assert f'"hello":{{"ok":{c_format(OLD_HELLO, "true", 8, "true", T0, T1)},\n' in replies_text
    assert f'"failed":{c_format(OLD_HELLO, "false", 0, "false", T0, T1)}}}' in replies_text
    for kind in KINDS:
        key = f'"{kind}":true,' if kind.startswith("datapath") else ""
        sweep, perf = ("true" if kind == k else "false" for k in ("sweep", "perf"))
        untagged = c_format(OLD_SERVE_HEAD, "", "true", 8, sweep, perf, T2) + key + '"devices":[]}'
        tagged = c_format(OLD_SERVE_HEAD, '"id":5,', "false", 8, sweep, perf, T2) + key + '"devices":[]}'
        assert f'\n"{kind}":{{"untagged":{untagged},\n"tagged":{tagged}}}' in replies_text, kind
        if kind != "probe":
            assert f'\n"{kind}":{c_format(OLD_ONESHOT_CHECK, "true", kind, 8, T0, T1, T2, "[]")}' in replies_text, kind
    times = (T0, T1, T2, 1.25, 2.25, 3.25, 4, 5.5, 6.5, 7.5, 8.5, 9.5, "null", "null", "[]")
    assert f'\n"probe":{c_format(OLD_ONESHOT_PROBE, "true", 8, "false", *times)}' in replies_text
    assert f'\n"identify":{c_format(OLD_ONESHOT_PROBE, "false", 8, "true", *times)}' in replies_text
    assert '"bad_request":{"untagged":{"ok":false,"error":"bad request","devices":[]},\n' in replies_text
    assert '"tagged":{"id":5,"ok":false,"error":"bad request","devices":[]}}' in replies_text
    assert f'"runtime_init_failed":{c_format(OLD_INIT_FAILED, 4096, T0, "null")}\n' in replies_text


def test_the_check_replies_differ_from_before_only_by_the_two_identity_keys(replies_text):
    """BEFORE holds the four printers' lines for the same results, printed by
    the printers as they were before kfd_node_id and pci_bus_id were added."""
    before = BEFORE.read_text()
    for kind in CHECKS:
        line = next(ln for ln in replies_text.split("\n") if ln.startswith(f'"{kind}":{{"blank":'))
        stripped, n = re.subn(r'"kfd_node_id":-?\d+,"pci_bus_id":"[^"]*",(?="error")', "", line)
        assert n == 3, kind
        old = next(ln for ln in before.split("\n") if ln.startswith(f'"{kind}":{{"blank":'))
        assert stripped.rstrip(",}") == old.rstrip(",}"), kind
        assert stripped != line


# ---- the stub's replies ------------------------------------------------------------------------
def as_json(d):
    return json.loads(json.dumps(d))


def stub_device(kind, *args, **kwargs):
    return getattr(stub_probe, f"_{kind}_device")(*args, **kwargs)


@pytest.mark.parametrize("kind", CHECKS)
def test_stub_check_reply_has_the_printers_shape_in_every_mode(replies, kind, monkeypatch):
    monkeypatch.delenv("MI355X_STUB_PROBE_LOG", raising=False)
    real = replies["devices"][kind]["filled8"]
    for mode in probe_contract.MODES[kind] + (("fail", "stale") if kind == "sweep" else ()):
        same_device_shape(kind, as_json(stub_device(kind, 3, mode, 77)), real, (kind, mode))
    d = as_json(stub_probe._not_completed(kind, 3, 77, None, 1.5, "earlier chip sweep / check still in flight"))
    same_device_shape(kind, d, real, (kind, "not completed"))
    assert d["ok"] is False and d["hsa_error"] == -1 and d["in_flight_s"] == 1.5


def test_stub_probe_reply_has_the_printers_shape_in_every_mode(replies):
    real = replies["devices"]["probe"]["filled8"]
    for mode in ("ok", "fail", "stale"):
        d = as_json(stub_probe._device(3, mode, 77))
        assert [k for k in d] == [k for k in real] and shape(d) == shape(real), mode


def serve(lines, control=None, tmp_path=None, timeout=60, extra_env=None):
    """One --serve --keep session of the stub over `lines` (then quit): the hello and the replies."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MI355X_STUB_")}
    env.pop("ROCR_VISIBLE_DEVICES", None)
    if control is not None:
        path = tmp_path / "control.json"
        path.write_text(json.dumps(control))
        env["MI355X_STUB_PROBE_CONTROL"] = str(path)
    env.update(extra_env or {})
    text = "".join(ln if ln.endswith("\n") else ln + "\n" for ln in lines) + "quit\n"
    r = subprocess.run([sys.executable, str(STUB), "--serve", "--keep"], input=text, capture_output=True, text=True,
                       env=env, timeout=timeout)
    docs = [json.loads(ln) for ln in r.stdout.splitlines()]
    return r.returncode, docs[0], docs[1:]


REQUESTS = {"probe": "probe 4 10 0:1 1:2", "sweep": "sweep 4 10 0:1 1:2", "perf": "perf 1024 10 64 0:1 1:2",
            "datapath": "datapath 10 0:1 1:2", "datapath_i8": "datapath_i8 10 0:1 1:2"}


def test_stub_hello_and_serve_envelopes_have_the_real_shape(replies, tmp_path):
    lines = [REQUESTS[k] for k in KINDS] + [f"@{7 + i} " + REQUESTS[k] for i, k in enumerate(KINDS)]
    rc, hello, docs = serve(lines)
    assert rc == 0 and len(docs) == 10
    assert shape(hello) == shape(replies["hello"]["ok"])
    untagged = dict(zip(KINDS, docs[:5]))
    tagged = {KINDS[d["id"] - 7]: d for d in docs[5:]}
    for kind in KINDS:
        assert envelope_shape(untagged[kind]) == envelope_shape(replies["serve"][kind]["untagged"]), kind
        assert envelope_shape(tagged[kind]) == envelope_shape(replies["serve"][kind]["tagged"]), kind
        for doc in (untagged[kind], tagged[kind]):
            assert ("id" in doc) == (doc is tagged[kind])
            assert doc["sweep"] is (kind == "sweep") and doc["perf"] is (kind == "perf")
            for dk in ("datapath", "datapath_i8"):
                assert (dk in doc) == (dk == kind), (kind, dk)
            assert [(d["ordinal"], d["nonce"]) for d in doc["devices"]] == [(0, 1), (1, 2)]
            for d in doc["devices"]:
                same_device_shape(kind, d, replies["devices"][kind]["filled8"], kind)
    rc, hello, docs = serve([], control={"serve": "broken"}, tmp_path=tmp_path)
    assert rc == 2 and docs == [] and shape(hello) == shape(replies["hello"]["failed"]) and hello["ok"] is False


def oneshot(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MI355X_STUB_")}
    env.pop("ROCR_VISIBLE_DEVICES", None)
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, str(STUB), *args], capture_output=True, text=True, env=env, timeout=60)
    return r.returncode, json.loads(r.stdout.splitlines()[-1])


ONESHOT_FLAGS = {"probe": [], "sweep": ["--sweep"], "perf": ["--perf"], "datapath": ["--datapath"],
                 "datapath_i8": ["--datapath-i8"]}


@pytest.mark.parametrize("kind", KINDS)
def test_stub_one_shot_document_has_the_real_shape(replies, kind):
    rc, doc = oneshot(["--devices", "0", "--nonce", "9", "--iters", "4", *ONESHOT_FLAGS[kind]])
    assert rc == 0 and envelope_shape(doc) == envelope_shape(replies["oneshot"][kind]), kind
    (d,) = doc["devices"]
    same_device_shape(kind, d, replies["devices"][kind]["filled8"], kind)
    assert d["nonce"] == 9 and d["ok"] is True


def test_stub_sweep_of_a_faulty_or_waiting_device_is_sweep_shaped(replies, tmp_path):
    """What the plain modes of an ordinal do to a sweep request: a sweep-shaped
    reply that fails (fail), carries a wrong nonce (stale), passes beside a probe
    left pending on the kept slot (pending), or has not completed (timeout,
    slow): hsa_error -1, then in_flight_s for as long as the earlier dispatch
    is outstanding, as hsa_chip.cpp answers."""
    real = replies["devices"]["sweep"]["filled8"]
    control = {"1": "fail", "2": "stale", "3": "pending", "4": "timeout", "5": "slow", "slow_s": 30}
    sweep = "sweep 4 0.2 0:10 1:11 2:12 3:13 4:14 5:15"
    rc, _, (first, second) = serve([sweep, sweep], control=control, tmp_path=tmp_path)
    assert rc == 0 and first["sweep"] is True and first["ok"] is False
    for doc in (first, second):
        for d in doc["devices"]:
            same_device_shape("sweep", d, real, d["ordinal"])
    d = first["devices"]
    assert d[0]["ok"] is True and d[0]["nonce"] == 10
    assert d[1]["ok"] is False and d[1]["hsa_error"] == 0 and d[1]["tile_bad"] == 1 and "tile_bad=1" in d[1]["error"]
    assert d[2]["ok"] is True and d[2]["nonce"] == 13
    assert d[3]["ok"] is True and d[3]["nonce"] == 13 and second["devices"][3]["ok"] is True
    for x in d[4:]:
        assert x["ok"] is False and x["hsa_error"] == -1 and x["in_flight_s"] == 0, x
        assert x["error"] == "chip sweep did not complete within 0.2s" and x["records_ok"] == 0
    for x in second["devices"][4:]:
        assert x["ok"] is False and x["hsa_error"] == -1 and x["in_flight_s"] >= 0.2, x
        assert re.fullmatch(r"earlier chip sweep / check still in flight for \d+\.\ds \(not completed\)", x["error"])


def test_stub_probe_of_a_waiting_device_is_probe_shaped(replies, tmp_path):
    real = replies["devices"]["probe"]["filled8"]
    control = {"1": "fail", "2": "stale", "3": "pending", "4": "timeout", "5": "slow", "slow_s": 0.3}
    probe = "probe 4 0.2 0:10 1:11 2:12 3:13 4:14 5:15"
    again = "probe 4 0.2 0:20 1:21 2:22 3:23 4:24 5:25"
    rc, _, (first, second) = serve([probe, again], control=control, tmp_path=tmp_path)
    assert rc == 0
    for doc in (first, second):
        for d in doc["devices"]:
            assert [k for k in d] == [k for k in real] and shape(d) == shape(real), d
    assert first["devices"][3]["pending_s"] > 0 and first["devices"][5]["pending_s"] > 0
    late = second["devices"][5]
    assert late["ok"] is True and late["late"] is True and late["nonce"] == 15


def test_a_device_the_server_does_not_have(replies):
    rc, _, docs = serve(["probe 4 10 99:7", "sweep 4 10 99:7", "perf 1 10 64 99:7", "datapath 10 99:7",
                         "datapath_i8 10 99:7"])
    for kind, doc in zip(KINDS, docs):
        (d,) = doc["devices"]
        assert doc["ok"] is False and d["ok"] is False and d["ordinal"] == 99 and d["error"] == "no such GPU (count=8)"
        blank = replies["devices"][kind]["blank"]
        # what run_batch / run_on_each print for it: the blank result with the ordinal and the reason
        assert d == {**blank, "ordinal": 99, "error": d["error"]}, kind


# ---- fault modes say what the real verdict says ------------------------------------------------
@pytest.mark.parametrize("kind", CHECKS)
def test_stub_fault_modes_carry_the_shipped_verdicts_figures(kind, tmp_path, monkeypatch):
    monkeypatch.delenv("MI355X_STUB_PROBE_LOG", raising=False)
    real = probe_contract.real_replies(kind, tmp_path)
    assert set(real) == set(probe_contract.MODES[kind])
    for mode, want in real.items():
        args = (0, mode, probe_contract.NONCE)
        got = as_json(stub_device(kind, *args, iters=probe_contract.ITERS) if kind == "sweep"
                      else stub_device(kind, *args))
        for key in probe_contract.KEYS[kind]:
            assert type(got[key]) is type(want[key]) and got[key] == want[key], (kind, mode, key, got[key], want[key])
        assert got["nonce"] == want["nonce"] == probe_contract.NONCE
        assert (mode == "ok") or (got["ok"] is False) or kind == "perf", (kind, mode)
        if kind == "perf":      # the rates and clocks the engine's floors judge, as printed
            for key in ("hbm_write_gbps", "hbm_read_gbps", "mfma_tflops", "clock_mhz_min", "clock_mhz_median",
                        "clock_mhz_max", "fill_us", "check_us", "check2_us", "mfma_us"):
                assert abs(got[key] - want[key]) <= 0.05 + 1e-9 * abs(want[key]), (mode, key, got[key], want[key])
            assert got["xcd_clock_mhz"] == want["xcd_clock_mhz"], mode


# ---- the request grammar -----------------------------------------------------------------------
CORPUS = [
    # every kind, tagged and untagged
    "probe 4 10 0:1", "sweep 4 10 0:1", "perf 65536 10 4096 0:1", "datapath 10 0:1", "datapath_i8 10 0:1",
    "@1 probe 4 10 0:1", "@2 sweep 4 10 0:1", "@3 perf 65536 10 4096 0:1", "@4 datapath 10 0:1",
    "@18446744073709551615 datapath_i8 10 0:1",
    # per-device deadlines
    "probe 4 10 0:1:2.5", "probe 4 10 0:1:0", "probe 4 10 0:1:-3", "probe 4 9.75 0:1:0.25 1:2 2:3:1e-3",
    # nonces
    "probe 4 10 0:0x10", "probe 4 10 0:0x80000000", "probe 4 10 0:0xFFFFFFFF", "probe 4 10 0:4294967295", "probe 4 10 0:010",
    # several devices, trailing blanks, CRLF
    "sweep 1 10 0:1 1:2 2:3 3:4 4:5 5:6 6:7 7:8", "probe 4 10 0:1   1:2  ", "probe 4 10 0:1 \r\n", "datapath 10 3:9\r\n",
    "probe 4 10 -1:5", "probe 4 10 99:7",
    # refused
    "@7probe 4 10 0:1", "@x probe 4 10 0:1", "@ probe 4 10 0:1", "@7", "nonsense", "nonsense 4 10 0:1", "probe", "probe ",
    "probe 4", "probe 4 ", "sweep 4 0:1", "perf 65536 10 0:1", "perf 65536 10", "datapath", "datapath_i8",
    "quitx", "PROBE 4 10 0:1", " probe 4 10 0:1",
    # datapath_i8 against the "datapath " prefix
    "datapath_i8 10 0:6", "datapath _i8 10 0:6", "datapath_i810 0:6", "datapath_i 10 0:6",
    # an empty device list
    "probe 4 10", "probe 4 10 ", "@9 sweep 4 10", "datapath 10", "perf 65536 10 4096",
    # a malformed device token, alone, last, and between two good ones
    "probe 4 10 0", "probe 4 10 0:", "probe 4 10 :1", "probe 4 10 0:1:", "probe 4 10 0:1 x", "probe 4 10 0:1 1:2 x",
    "probe 4 10 0:1 x 1:2", "probe 4 10 0:1 1 2:3", "probe 4 10 0:1 1: 2:3", "probe 4 10 0:1,1:2", "probe 4 10 0:1:2:3",
    "probe 4 10 0:1\t",
]


def test_the_stub_parses_a_request_line_as_the_server_does(cli):
    real = contract_cli.probe_parse(cli, CORPUS)
    mine = [stub_probe._parse(ln) for ln in CORPUS]
    for line, r, m in zip(CORPUS, real, mine):
        assert m == r, (line, m, r)
    by_line = dict(zip(CORPUS, real))
    # what the corpus is there to pin
    assert by_line["probe 4 10 0:1:0"]["devices"] == [[0, 1, 10]] and by_line["probe 4 10 0:1:-3"]["devices"] == [[0, 1, 10]]
    assert by_line["probe 4 10 0:0x80000000"]["devices"] == [[0, 0x80000000, 10]]
    assert by_line["probe 4 10 0:0xFFFFFFFF"]["devices"] == [[0, 0xFFFFFFFF, 10]]
    assert by_line["probe 4 9.75 0:1:0.25 1:2 2:3:1e-3"]["devices"] == [[0, 1, 0.25], [1, 2, 9.75], [2, 3, 0.001]]
    assert by_line["datapath_i8 10 0:6"]["kind"] == "datapath_i8" and by_line["datapath_i8 10 0:6"]["iters"] == 0
    assert by_line["@4 datapath 10 0:1"] == {"tagged": True, "id": 4, "kind": "datapath", "iters": 0, "timeout": 10,
                                             "mib": 0, "devices": [[0, 1, 10]]}
    assert by_line["perf 65536 10 4096 0:1"]["mib"] == 4096
    for line in ("@7probe 4 10 0:1", "@x probe 4 10 0:1", "nonsense", "probe 4", "perf 65536 10 0:1"):
        assert by_line[line] == "bad request", line
    # an empty device list is a request (answered not ok, with no devices)
    for line in ("probe 4 10", "probe 4 10 ", "@9 sweep 4 10", "datapath 10", "perf 65536 10 4096"):
        assert by_line[line] != "bad request" and by_line[line]["devices"] == [], line
    # text left over after the device list refuses the line: no answer for a part of the devices
    for line in ("probe 4 10 0:1 x 1:2", "probe 4 10 0:1 1:2 x", "probe 4 10 0:1 1 2:3", "probe 4 10 0:1:2:3"):
        assert by_line[line] == "bad request", line


def test_a_bad_line_does_not_end_the_stub(replies):
    rc, _, docs = serve(["nonsense", "@7 nonsense", "probe 4 10 0:1 x 1:2", "probe 4 10", "@8 probe 4 10 0:5"])
    assert rc == 0 and len(docs) == 5
    assert docs[0] == replies["bad_request"]["untagged"] == {"ok": False, "error": "bad request", "devices": []}
    assert docs[1] == {**replies["bad_request"]["tagged"], "id": 7}
    assert [k for k in docs[1]] == [k for k in replies["bad_request"]["tagged"]]
    assert docs[2] == docs[0]
    assert docs[3]["ok"] is False and docs[3]["devices"] == [] and "error" not in docs[3]     # no devices: not ok
    assert docs[4]["id"] == 8 and docs[4]["ok"] is True and docs[4]["devices"][0]["nonce"] == 5


# ---- recorded truth ----------------------------------------------------------------------------
def test_recorded_replies_from_an_mi355x_have_the_printers_shape(replies):
    """profiles/probe_contract_box.json: the transcript of tests/test_gpu_probe_contract.py as a real
    probe answered it. Present once that test has run on an MI355X; the stub is held to it too."""
    if not BOX.exists():
        return
    box = json.loads(BOX.read_text())
    assert shape(box["hello"]) == shape(replies["hello"]["ok"])
    seen = set()
    for entry in box["serve"]:
        doc, kind = entry["reply"], entry["kind"]
        if kind is None:
            assert doc == replies["bad_request"]["untagged"]
            continue
        seen.add(kind)
        assert envelope_shape(doc) == envelope_shape(replies["serve"][kind]["tagged" if "id" in doc else "untagged"])
        for d in doc["devices"]:
            same_device_shape(kind, d, replies["devices"][kind]["filled8"], entry["request"])
    assert seen == set(KINDS)
    for kind, doc in box["oneshot"].items():
        assert envelope_shape(doc) == envelope_shape(replies["oneshot"][kind]), kind
        for d in doc["devices"]:
            same_device_shape(kind, d, replies["devices"][kind]["filled8"], kind)
    _, _, stub_docs = serve([e["request"] for e in box["serve"]])
    for entry, mine in zip(box["serve"], stub_docs):
        assert envelope_shape(mine) == envelope_shape(entry["reply"]), entry["request"]
        for a, b in zip(mine["devices"], entry["reply"]["devices"]):
            assert [k for k in a] == [k for k in b] and shape(a) == shape(b), entry["request"]


# ---- the program itself under the sanitizers ---------------------------------------------------
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]


def test_the_contract_program_under_the_address_and_undefined_sanitizers(cli, replies_text, tmp_path):
    cxx = contract_cli.host_compiler()
    one = tmp_path / "one.cpp"
    one.write_text("int main() { return 0; }\n")
    if not cxx or subprocess.run([cxx, *SANITIZE, str(one), "-o", str(tmp_path / "one")], capture_output=True,
                                 timeout=120).returncode != 0 or \
            subprocess.run([str(tmp_path / "one")], capture_output=True, timeout=60).returncode != 0:
        pytest.skip(f"a one-line program does not build and run with {SANITIZE[0]}")
    exe = contract_cli.compile_cli(tmp_path / "probe_contract_cli_san", SANITIZE, source=contract_cli.PROBE_SOURCE)
    assert contract_cli.probe_replies_text(exe) == replies_text
    long_line = "probe 4 10 " + " ".join(f"{i % 8}:{i}" for i in range(3000))       # past the server's line buffer
    corpus = CORPUS + ["@" + "9" * 40 + " probe 4 10 0:1", "probe 4 10 0:99999999999999999999999"]
    assert contract_cli.probe_parse(exe, corpus) == contract_cli.probe_parse(cli, corpus)
    r = subprocess.run([str(exe), "parse"], input=(long_line + "\n").encode(), capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-2000:]

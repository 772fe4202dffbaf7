"""The datapath_f16 kind of testing/stub_probe.py held to the real probe's
reply contract, CPU only, as tests/test_probe_contract.py holds the other five
kinds (and keeps them): the printers' own output (`probe_contract_cli
replies-f16`), the shipped verdict's figures for every fault mode
(testing/probe_contract.py), and the replies an MI355X gave
(tests/golden/probe_contract_f16_box.json, recorded by
tests/test_gpu_probe_contract_f16.py)."""
import json

import pytest

from rocm_k8s_device_plugin_amd.testing import contract_cli, probe_contract, stub_probe

from test_probe_contract import REPO, as_json, envelope_shape, oneshot, serve, shape

KIND = "datapath_f16"
BOX = REPO / "tests" / "golden" / "probe_contract_f16_box.json"
REQUEST = "datapath_f16 10 0:1 1:2"


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return contract_cli.probe_contract_cli(tmp_path_factory.mktemp("probe_contract_cli"))


@pytest.fixture(scope="module")
def replies(cli):
    return json.loads(contract_cli.probe_replies_text(cli, "replies-f16"))


@pytest.fixture(scope="module")
def five_kinds(cli):
    return json.loads(contract_cli.probe_replies_text(cli))


def same_device_shape(got, real, what):
    assert [k for k in got] == [k for k in real], (what, "keys or their order")
    assert shape(got) == shape(real), what
    assert len(got["stage_bad"]) == 7, what


def test_the_printer_has_the_int8_checks_keys_seven_stage_counts_and_an_envelope_key_of_its_own(replies, five_kinds):
    """The result struct is the int8 check's but for stage_bad[7], so the device object has the same keys in
    the same order with seven stage counts; the envelope's key tells the kinds apart, and `replies` (the
    five kinds, recorded) does not know this one."""
    for which, dev in replies["devices"][KIND].items():
        i8 = five_kinds["devices"]["datapath_i8"][which]
        assert list(dev) == list(i8), which
        assert shape({**dev, "stage_bad": []}) == shape({**i8, "stage_bad": []}), which
        assert len(dev["stage_bad"]) == 7 and len(i8["stage_bad"]) == 5
    assert KIND not in json.dumps(five_kinds)
    blank, f8, f16 = (replies["devices"][KIND][k] for k in ("blank", "filled8", "filled16"))
    assert shape(f8) == shape(f16) and [k for k in blank] == [k for k in f8] and len(f8["stage_bad"]) == 7
    assert blank["kfd_node_id"] == -1 and blank["pci_bus_id"] == "" and blank["first_bad_wg"] == -1
    assert list(f8)[-3:] == ["kfd_node_id", "pci_bus_id", "error"]      # the identity sits where the siblings put it
    for tag in ("untagged", "tagged"):
        doc, i8 = replies["serve"][KIND][tag], five_kinds["serve"]["datapath_i8"][tag]
        assert doc["datapath_f16"] is True and "datapath" not in doc and "datapath_i8" not in doc
        assert [k.replace("datapath_f16", "datapath_i8") for k in doc] == list(i8)
        assert ("id" in doc) == (tag == "tagged")
    one = replies["oneshot"][KIND]
    assert one["datapath_f16"] is True and list(one)[:2] == ["ok", "datapath_f16"]
    assert [k.replace("datapath_f16", "datapath_i8") for k in one] == list(five_kinds["oneshot"]["datapath_i8"])


def test_stub_reply_has_the_printers_shape_in_every_mode(replies, monkeypatch):
    monkeypatch.delenv("MI355X_STUB_PROBE_LOG", raising=False)
    real = replies["devices"][KIND]["filled8"]
    for mode in probe_contract.MODES[KIND]:
        same_device_shape(as_json(stub_probe._datapath_f16_device(3, mode, 77)), real, mode)
    d = as_json(stub_probe._not_completed(KIND, 3, 77, None, 1.5, "earlier chip sweep / check still in flight"))
    same_device_shape(d, real, "not completed")
    assert d["ok"] is False and d["hsa_error"] == -1 and d["in_flight_s"] == 1.5


def test_stub_fault_modes_carry_the_shipped_verdicts_figures(tmp_path, monkeypatch):
    monkeypatch.delenv("MI355X_STUB_PROBE_LOG", raising=False)
    real = probe_contract.real_replies(KIND, tmp_path)
    assert set(real) == set(probe_contract.MODES[KIND]) == {"ok", "stuck_bit", "missing", "device_bad"}
    for mode, want in real.items():
        got = as_json(stub_probe._datapath_f16_device(0, mode, probe_contract.NONCE))
        for key in probe_contract.KEYS[KIND]:
            assert type(got[key]) is type(want[key]) and got[key] == want[key], (mode, key, got[key], want[key])
        assert got["nonce"] == want["nonce"] == probe_contract.NONCE
        assert (mode == "ok") == got["ok"], mode
    assert "stage 4 word" in real["stuck_bit"]["error"] and "(bit 30)" in real["stuck_bit"]["error"]


def test_stub_serve_envelopes_and_one_shot_have_the_real_shape(replies):
    rc, hello, docs = serve([REQUEST, "@7 " + REQUEST, "datapath_f16 10 99:7", "datapath_f1610 0:1"])
    assert rc == 0 and len(docs) == 4
    (tagged,) = [d for d in docs if "id" in d]        # answered on a thread of its own: it may come later
    untagged, absent, refused = [d for d in docs if "id" not in d]
    for doc, tag in ((untagged, "untagged"), (tagged, "tagged")):
        assert envelope_shape(doc) == envelope_shape(replies["serve"][KIND][tag]), tag
        assert doc["datapath_f16"] is True and doc["sweep"] is False and doc["perf"] is False
        assert "datapath" not in doc and "datapath_i8" not in doc
        assert [(d["ordinal"], d["nonce"]) for d in doc["devices"]] == [(0, 1), (1, 2)]
        for d in doc["devices"]:
            same_device_shape(d, replies["devices"][KIND]["filled8"], tag)
    assert tagged["id"] == 7 and "id" not in untagged
    (d,) = absent["devices"]                      # what run_on_each prints: the blank result, the ordinal, the reason
    assert absent["ok"] is False and d == {**replies["devices"][KIND]["blank"], "ordinal": 99,
                                           "error": "no such GPU (count=8)"}
    assert refused == {"ok": False, "error": "bad request", "devices": []}
    rc, doc = oneshot(["--devices", "0", "--nonce", "9", "--datapath-f16"])
    assert rc == 0 and envelope_shape(doc) == envelope_shape(replies["oneshot"][KIND])
    (d,) = doc["devices"]
    same_device_shape(d, replies["devices"][KIND]["filled8"], "one-shot")
    assert d["nonce"] == 9 and d["ok"] is True


def test_recorded_replies_from_an_mi355x_hold_the_printers_and_the_stub(replies, five_kinds):
    """The golden transcript: the printers' documents have the recorded replies' shape (a printer changed
    since the recording shows here), and so has the stub, request by request."""
    box = json.loads(BOX.read_text())
    assert shape(box["hello"]) == shape(five_kinds["hello"]["ok"])
    kinds = [e["kind"] for e in box["serve"]]
    assert kinds.count(KIND) == 3 and None in kinds
    for entry in box["serve"]:
        doc, kind = entry["reply"], entry["kind"]
        if kind is None:
            assert doc == five_kinds["bad_request"]["untagged"]
            continue
        printers = replies if kind == KIND else five_kinds
        assert envelope_shape(doc) == envelope_shape(printers["serve"][kind]["tagged" if "id" in doc else "untagged"])
        assert (KIND in doc) == (kind == KIND), entry["request"]
        for d in doc["devices"]:
            real = printers["devices"][kind]["filled8"]
            assert [k for k in d] == [k for k in real] and shape(d) == shape(real), entry["request"]
    checked = [e["reply"]["devices"][0] for e in box["serve"] if e["kind"] == KIND]
    assert [d["ok"] for d in checked] == [True, True, False] and checked[2]["ordinal"] == 99
    for d in checked[:2]:
        assert d["kept_queue"] is True and d["records_ok"] == d["grid"] == 256 and d["stage_bad"] == [0] * 7
    one = box["oneshot"][KIND]
    assert envelope_shape(one) == envelope_shape(replies["oneshot"][KIND])
    _, hello, stub_docs = serve([e["request"] for e in box["serve"]])
    assert shape(hello) == shape(box["hello"])
    stub_docs = sorted(stub_docs, key=lambda d: "id" in d)          # a tagged reply may overtake
    recorded = sorted(box["serve"], key=lambda e: "id" in e["reply"])
    for entry, mine in zip(recorded, stub_docs):
        assert envelope_shape(mine) == envelope_shape(entry["reply"]), entry["request"]
        for a, b in zip(mine["devices"], entry["reply"]["devices"]):
            assert [k for k in a] == [k for k in b] and shape(a) == shape(b), entry["request"]
    _, mine = oneshot(["--devices", "0", "--nonce", "9", "--datapath-f16"])
    assert envelope_shape(mine) == envelope_shape(one)
    assert [k for k in mine["devices"][0]] == [k for k in one["devices"][0]]

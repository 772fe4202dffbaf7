"""The printers' bytes of the datapath_f64, datapath_f6f4, datapath_sparse, datapath_gemm, datapath_splitk and
datapath_attn kinds, CPU only, as tests/test_probe_contract.py pins the first five kinds': `probe_contract_cli
replies-rest` prints each kind's device object (blank, filled with num_xcc 8 and 16) and its serve and one-shot
envelopes, with the fields only the GEMM, split-K and attention results have filled as well. The recording
(tests/golden/probe_contract_replies_rest.json) was taken from the eleven hand-written printers, before they became
one: a swapped argument, another precision or a moved key shows as a changed byte."""
import json

import pytest

from rocm_k8s_device_plugin_amd.testing import contract_cli

from test_probe_contract import REPO, shape

GOLDEN = REPO / "tests" / "golden" / "probe_contract_replies_rest.json"
STAGES = {"datapath_f64": 7, "datapath_f6f4": 8, "datapath_sparse": 10, "datapath_gemm": 3, "datapath_splitk": 4,
          "datapath_attn": 4}
EXTRAS = {"datapath_gemm": {"ksteps", "fill_us", "verify_us"},
          "datapath_splitk": {"tiles", "splits", "ksteps", "ledger_bad", "xccs_per_tile_min", "fill_us", "drain_us",
                              "verify_us"},
          "datapath_attn": {"heads", "qblocks", "kblocks", "exp_inexact", "fill_us", "verify_us"}}


@pytest.fixture(scope="module")
def replies_text(tmp_path_factory):
    cli = contract_cli.probe_contract_cli(tmp_path_factory.mktemp("probe_contract_cli"))
    return contract_cli.probe_replies_text(cli, "replies-rest")


def test_replies_are_the_recorded_bytes(replies_text):
    """Any change to a printer (a renamed key, another precision, another order) shows here first."""
    assert replies_text == GOLDEN.read_text()


def test_the_printers_obey_their_own_length_rule(replies_text):
    replies = json.loads(replies_text)
    assert list(replies["devices"]) == list(replies["serve"]) == list(replies["oneshot"]) == list(STAGES)
    common = None
    for kind, stages in STAGES.items():
        blank, f8, f16 = (replies["devices"][kind][k] for k in ("blank", "filled8", "filled16"))
        assert shape(f8) == shape(f16) and [k for k in blank] == [k for k in f8]
        assert (f8["num_xcc"], f16["num_xcc"], blank["num_xcc"]) == (8, 16, 0)
        for d in (blank, f8, f16):
            assert len(d["stage_bad"]) == stages, kind
        assert blank["kfd_node_id"] == -1 and blank["pci_bus_id"] == "" and blank["first_bad_wg"] == -1
        assert f8["error"] == 'a "quoted" back\\slash'
        numbers = [v for k, v in f8.items() if shape(v) == "number" and k != "num_xcc"]
        numbers += [x for v in f8.values() if isinstance(v, list) for x in v]
        assert 0 not in numbers and len(set(numbers)) == len(numbers), kind    # a swapped argument would show
        rest = [k for k in f8 if k not in EXTRAS.get(kind, ())]
        assert set(f8) - set(rest) == EXTRAS.get(kind, set()), kind
        common = common or rest
        assert rest == common, kind                                     # the siblings' keys, in the siblings' order
        for tag in ("untagged", "tagged"):
            doc = replies["serve"][kind][tag]
            assert doc[kind] is True and [k for k in doc if k.startswith("datapath")] == [kind]
            assert ("id" in doc) == (tag == "tagged")
        assert list(replies["oneshot"][kind])[:2] == ["ok", kind] and replies["oneshot"][kind][kind] is True

"""The MX quantise check above the kernel, without a GPU: the header's operands and image against the reference's, the
shipped verdict on a flipped word of each stage, the stub probe's replies against the shipped verdict's, the Engine's
series over the stub, and the request grammar in the server's parser."""
import json
from contextlib import closing

import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.testing import contract_cli, probe_contract, stub_probe
from rocm_k8s_device_plugin_amd.testing import datapath_mxquant_reference as db

from test_native_datapath_f16_daemon import _engine
from test_native_datapath_gemm import _series


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return contract_cli.datapath_mxquant_cli(tmp_path_factory.mktemp("datapath_mxquant_contract"))


@pytest.mark.parametrize("grid,hsteps,nonce", [(1, 1, 0xFFFFFFFF), (1, 3, 0xDEADBEEF), (2, 2, 7), (1, 4, 0x5EED142F)])
def test_the_header_and_the_reference_give_one_image(cli, grid, hsteps, nonce):
    assert contract_cli.datapath_mxquant_image(cli, grid, nonce, hsteps, "operands") == db.operand_bytes(grid, nonce, hsteps)
    got = np.frombuffer(contract_cli.datapath_mxquant_image(cli, grid, nonce, hsteps), dtype="<u4")
    want = np.frombuffer(db.image_bytes(*db.healthy(grid, nonce, hsteps)), dtype="<u4")
    assert got.size == want.size and np.argwhere(got != want).tolist() == []


# (workgroup, stage, word of the workgroup's stage, bit): fold words of both feeds, a code dword, a scale dword, Y's
# first and last words
FLIPS = [(0, 0, 0, 0), (1, 0, 7, 31), (1, 1, 2, 9), (0, 1, 15, 16), (0, 2, 0, 3), (1, 2, 2 * 2048 + 2 * 77 + 1, 8),
         (0, 3, 0, 31), (1, 3, 16383, 0), (1, 3, 77 * 128 + 5, 23)]
PER_WG = {0: 16, 1: 16, 2: db.img_words(2), 3: 16384}


@pytest.mark.parametrize("wg,stage,word,bit", FLIPS)
def test_the_verdict_passes_the_image_and_names_a_flipped_bit(cli, tmp_path, wg, stage, word, bit):
    parts = db.healthy(2, 0xDEADBEEF, 2)
    for flip in (False, True):
        if flip:
            target = (parts[stage - 1], word) if stage >= 2 else (parts[0], db.fold_slot(stage, word))
            want = int(target[0][wg, target[1]])
            target[0][wg, target[1]] ^= np.uint32(1 << bit)
        r = contract_cli.datapath_mxquant_verdict(cli, db.image_bytes(*parts), 2, 0xDEADBEEF, 2, tmp_path)
        assert r.returncode == 0, r.stderr
        g = json.loads(r.stdout)
        assert g["ok"] is not flip and g["records_ok"] == 2 - flip and g["error"].startswith("1/2" if flip else ""), g
        assert g["stage_bad"] == [int(flip and s == stage) for s in range(4)], g
        assert (g["mfma_bad"], g["tile_bad"]) == (int(flip and stage < 2), int(flip and stage == 3)), g
    numbered = wg * PER_WG[stage] + word
    assert (g["first_bad_wg"], g["first_bad_stage"], g["first_bad_word"]) == (wg, stage, numbered), g
    assert (g["first_bad_want"], g["first_bad_xor"]) == (want, 1 << bit), g
    assert g["error"].endswith(f"first bad: wg {wg} stage {stage} word {numbered} xor 0x{1 << bit:08x} (bit {bit})"), g


def test_the_stub_answers_what_the_shipped_verdict_says_of_the_same_faults(tmp_path):
    real = probe_contract.real_replies("datapath_mxquant", tmp_path)
    assert set(real) == {"ok", "stuck_bit", "missing", "device_bad"}
    for mode, want in real.items():
        got = json.loads(json.dumps(stub_probe._datapath_mxquant_device(0, mode, probe_contract.NONCE)))
        assert sorted(got) == sorted(want), mode                          # the printer's fields, no more, no fewer
        for key in probe_contract.KEYS["datapath_mxquant"]:
            if not key.endswith("_covered"):                              # the image names no placement
                assert got[key] == want[key], (mode, key, got[key], want[key])
    replies = contract_cli.probe_replies_text(contract_cli.datapath_mxquant_cli(tmp_path)).splitlines()
    blank, oneshot, serve, probe = (json.loads(ln) for ln in replies)
    assert blank == {**stub_probe._blank("datapath_mxquant", 99, 7000), "error": "no such GPU (count=1)"}
    assert oneshot["datapath_mxquant"] is serve["datapath_mxquant"] is True and "datapath_mxquant" not in probe
    assert serve["id"] == 5 and [k for k in serve if k.startswith("datapath")] == ["datapath_mxquant"]


def test_a_failure_is_unhealthy_with_series_of_its_own_and_off_sends_nothing(tmp_path):
    _, ctl, log, eng, dev = _engine(tmp_path, {"datapath_mxquant": {"2": "stuck_bit"}}, datapath_mxquant_check_every=2)
    with closing(eng):
        before = _series()
        eng.sweep()                                   # sweep 0: checked, device 2 fails
        snap = eng.snapshot()
        assert {d for d, (ok, _) in snap.items() if not ok} == {dev[2]}
        assert snap[dev[2]][1][0].startswith("datapath mxquant check: 255/256 workgroups exact (feed_bad=0 quant_bad=0 "
                                             "y_bad=128); first bad: wg 17 stage 3 word 278528 xor 0x40000000 (bit 30)")
        ctl.write_text("{}")
        eng.sweep()                                   # sweep 1: no check, the verdict stands
        eng.sweep()                                   # sweep 2: checked again, passes
        st = eng.stats()
        assert st["datapath_mxquant_checks"] == 2 and st["datapath_mxquant_failures"] == 1 and st["datapath_mxgemm_checks"] == 0
        assert all(ok for ok, _ in eng.snapshot().values())
        assert {ln.split(":")[0] for ln in log.read_text().split() if ln.startswith("datapath")} == {"datapath_mxquant"}
        assert {k for k, v in _series().items() if v != before.get(k, 0)} == {
            "mi355x_dp_datapath_mxquant_checks_total", f'mi355x_dp_datapath_mxquant_check_failures_total{{device="{dev[2]}"}}'}
    _, _, log, eng, _ = _engine(tmp_path / "off", {"datapath_mxquant": {"2": "stuck_bit"}})   # default cadence: off
    with closing(eng):
        eng.sweep()
        assert all(ok for ok, _ in eng.snapshot().values()) and eng.stats()["datapath_mxquant_checks"] == 0
        assert not [ln for ln in log.read_text().split() if ln.startswith("datapath")]


GRAMMAR = ["datapath_mxquant 10 0:1", "@4 datapath_mxquant 9.5 0:1:2.5 3:0x10", "datapath_mxquant 10",
           "datapath_mxquant10 0:1", "datapath_mxquant", "datapath_mxquant x 0:1", "datapath_mxquant 10 0:1 x",
           "datapath_mxquant 10 0", "DATAPATH_MXQUANT 10 0:1", "@7datapath_mxquant 10 0:1", "datapath_mxquant_ 10 0:1"]


def test_request_grammar_in_the_servers_parser_and_in_the_stub(tmp_path):
    got = contract_cli.probe_parse(contract_cli.probe_contract_cli(tmp_path), GRAMMAR)
    assert got == [stub_probe._parse(ln) for ln in GRAMMAR] and got[3:] == ["bad request"] * 8
    assert got[0] == {"tagged": False, "id": 0, "kind": "datapath_mxquant", "iters": 0, "timeout": 10, "mib": 0,
                      "devices": [[0, 1, 10]]}
    assert got[1]["id"] == 4 and got[1]["devices"] == [[0, 1, 2.5], [3, 16, 9.5]] and got[2]["devices"] == []

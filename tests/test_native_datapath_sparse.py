"""The sparse (2:4) MFMA datapath check above the kernel, without a GPU: the header's image against the
reference's, the shipped verdict on a flipped word, the Engine's cadence, failures, reason and series over the stub
probe, and the request grammar in the server's parser."""
import json
from contextlib import closing

import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.ops.native import core
from rocm_k8s_device_plugin_amd.testing import contract_cli, stub_probe
from rocm_k8s_device_plugin_amd.testing import datapath_sparse_reference as db

from test_native_datapath_f16_daemon import _engine


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return contract_cli.datapath_sparse_cli(tmp_path_factory.mktemp("datapath_sparse_contract"))


@pytest.mark.parametrize("grid,nonce", [(g, n) for g in (1, 3) for n in (0xFFFFFFFF, 0xDEADBEEF)])
def test_the_header_and_the_reference_give_one_image(cli, grid, nonce):
    got = np.frombuffer(contract_cli.datapath_sparse_image(cli, grid, nonce), dtype="<u4")
    want = np.frombuffer(db.image_bytes(*db.healthy(grid, nonce)), dtype="<u4")
    assert got.size == want.size and np.argwhere(got != want).tolist() == []


# (workgroup, stage, word of the stage, bit): one per stage; bits 0 and 31, first and last words, the last workgroup
FLIPS = [(0, 0, 513, 31), (1, 1, 2, 0), (2, 2, 1023, 19), (0, 3, 1000, 31), (2, 4, 0, 0), (1, 5, 130, 7), (2, 6, 255, 30),
         (2, 7, 777, 23), (0, 8, 129, 14), (1, 9, 1023, 1)]


@pytest.mark.parametrize("wg,stage,word,bit", FLIPS)
def test_the_verdict_passes_the_image_and_names_a_flipped_bit(cli, tmp_path, wg, stage, word, bit):
    recs, tiles = db.healthy(3, 0xDEADBEEF)
    for flip in (False, True):
        if flip:
            want = int(tiles[wg, db.TILE_OFFSET[stage] + word])
            tiles[wg, db.TILE_OFFSET[stage] + word] ^= np.uint32(1 << bit)
            recs[wg, db.REC_BAD + stage] = 1                           # what the device's comparator adds
        r = contract_cli.datapath_sparse_verdict(cli, db.image_bytes(recs, tiles), 3, 0xDEADBEEF, tmp_path)
        assert r.returncode == 0, r.stderr
        g = json.loads(r.stdout)
        assert g["ok"] is not flip and g["tile_bad"] == g["mfma_bad"] == int(flip) and g["records_ok"] == 3 - flip, g
        assert g["stage_bad"] == [int(flip and s == stage) for s in range(10)], g
    assert (g["first_bad_wg"], g["first_bad_stage"], g["first_bad_word"]) == (wg, stage, word), g
    assert (g["first_bad_want"], g["first_bad_xor"]) == (want, 1 << bit) and f"(bit {bit})" in g["error"], g

def _series():                                      # the datapath series of /metrics: name -> value
    rows = (ln.rsplit(" ", 1) for ln in core().metrics_render().splitlines() if ln.startswith("mi355x_dp_datapath"))
    return {name: float(v) for name, v in rows}


def test_every_second_sweep_checks_and_a_failure_is_unhealthy_with_series_of_its_own(tmp_path):
    _, ctl, log, eng, dev = _engine(tmp_path, {"datapath_sparse": {"2": "stuck_bit"}}, datapath_sparse_check_every=2)
    with closing(eng):
        before = _series()
        eng.sweep()                                   # sweep 0: checked, device 2 fails
        snap = eng.snapshot()
        assert {d for d, (ok, _) in snap.items() if not ok} == {dev[2]}
        assert snap[dev[2]][1][0].startswith("datapath sparse check: 255/256 workgroups exact") and \
            f"stage 3 word {stub_probe.STUCK_SPARSE[1]} xor 0x40000000 (bit 30)" in snap[dev[2]][1][0], snap[dev[2]]
        ctl.write_text("{}")
        eng.sweep()                                   # sweep 1: no check, the verdict stands
        assert eng.stats()["datapath_sparse_checks"] == 1 and not eng.snapshot()[dev[2]][0]
        eng.sweep()                                   # sweep 2: checked again, passes
        st = eng.stats()
        assert st["datapath_sparse_checks"] == 2 and st["datapath_sparse_failures"] == 1
        assert all(ok for ok, _ in eng.snapshot().values())
        assert {ln.split(":")[0] for ln in log.read_text().split() if ln.startswith("datapath")} == {"datapath_sparse"}
        assert {k for k, v in _series().items() if v != before.get(k, 0)} == {
            "mi355x_dp_datapath_sparse_checks_total", f'mi355x_dp_datapath_sparse_check_failures_total{{device="{dev[2]}"}}'}


def test_flag_at_zero_never_sends_the_verb(tmp_path):
    _, ctl, log, eng, dev = _engine(tmp_path, {"datapath_sparse": {"2": "stuck_bit"}}, datapath_check_every=1)
    with closing(eng):
        eng.sweep()
        eng.sweep()
        assert "datapath_sparse" not in log.read_text() and "datapath:0" in log.read_text().split()
        assert all(ok for ok, _ in eng.snapshot().values()) and eng.stats()["datapath_sparse_checks"] == 0


GRAMMAR = ["datapath_sparse 10 0:1", "@4 datapath_sparse 9.5 0:1:2.5 3:0x10", "datapath_sparse 10",
           "datapath_sparse10 0:1", "datapath_sparse", "datapath_sparse x 0:1", "datapath_sparse 10 0:1 x", "datapath_sparse 10 0",
           "DATAPATH_SPARSE 10 0:1", "@7datapath_sparse 10 0:1", "datapath_sparse_ 10 0:1"]


def test_request_grammar_in_the_servers_parser_and_in_the_stub(tmp_path):
    got = contract_cli.probe_parse(contract_cli.probe_contract_cli(tmp_path), GRAMMAR)
    assert got == [stub_probe._parse(ln) for ln in GRAMMAR] and got[3:] == ["bad request"] * 8
    assert got[0] == {"tagged": False, "id": 0, "kind": "datapath_sparse", "iters": 0, "timeout": 10, "mib": 0,
                      "devices": [[0, 1, 10]]}
    assert got[1]["id"] == 4 and got[1]["devices"] == [[0, 1, 2.5], [3, 16, 9.5]] and got[2]["devices"] == []

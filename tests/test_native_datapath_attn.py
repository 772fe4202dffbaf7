"""The fused attention check above the kernel, without a GPU: the header's image against the reference's, the shipped
verdict on a flipped word of each stage, the stub probe's replies against the shipped verdict's, and the Engine's
cadence and separate failure set over the stub."""
import json
from contextlib import closing

import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.ops.native import core
from rocm_k8s_device_plugin_amd.testing import contract_cli, probe_contract, stub_probe
from rocm_k8s_device_plugin_amd.testing import datapath_attn_reference as da

from test_native_datapath_f16_daemon import _engine

SIZES, NONCE = (2, 2, 3), 0xDEADBEEF                   # heads, qblocks, kblocks of the verdict cases


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return contract_cli.datapath_attn_cli(tmp_path_factory.mktemp("datapath_attn_contract"))


@pytest.mark.parametrize("heads,qblocks,kblocks,nonce", [(1, 1, 1, 0xFFFFFFFF), (2, 2, 2, NONCE), (1, 1, 8, NONCE)])
def test_the_header_and_the_reference_give_one_image(cli, heads, qblocks, kblocks, nonce):
    got = np.frombuffer(contract_cli.datapath_attn_image(cli, heads, qblocks, kblocks, nonce), dtype="<u4")
    want = np.frombuffer(da.image_bytes(*da.healthy(heads, qblocks, kblocks, nonce)), dtype="<u4")
    assert got.size == want.size and np.argwhere(got != want).tolist() == []


def _verdict(cli, tmp_path, image):
    r = contract_cli.datapath_attn_verdict(cli, da.image_bytes(*image), *SIZES, NONCE, tmp_path)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


# (stage, word as the verdict numbers it, bit): fold words of both feeds (wg * 8 + wave * 2 + {xor, sum}), m / l words
# (wg * 256 + query * 2 + {m, l}), O words (wg * 8192 + query * 64 + d)
FLIPS = [(0, 0, 0), (0, 3 * 8 + 7, 31), (1, 2 * 8 + 2, 9), (2, 0, 31), (2, 256 + 77 * 2 + 1, 23), (2, 4 * 256 - 1, 0),
         (3, 0, 31), (3, 8192 + 77 * 64 + 5, 23), (3, 4 * 8192 - 1, 0)]


@pytest.mark.parametrize("stage,word,bit", FLIPS)
def test_the_verdict_passes_the_image_and_names_a_flipped_bit(cli, tmp_path, stage, word, bit):
    recs, ml, o = da.healthy(*SIZES, NONCE)
    g = _verdict(cli, tmp_path, (recs, ml, o))
    assert g["ok"] is True and g["records_ok"] == g["grid"] == 4 and g["stage_bad"] == [0] * 4 and g["error"] == "", g
    target = (recs.reshape(-1), word // 8 * da.REC_WORDS + da.fold_slot(stage, word % 8)) if stage < 2 else \
        ((ml, o)[stage - 2].reshape(-1), word)
    want = int(target[0][target[1]])
    target[0][target[1]] ^= np.uint32(1 << bit)
    wg = word // {0: 8, 1: 8, 2: da.ML_WORDS, 3: da.O_WORDS}[stage]
    g = _verdict(cli, tmp_path, (recs, ml, o))
    assert g["ok"] is False and g["records_ok"] == 3 and g["stage_bad"] == [int(s == stage) for s in range(4)], g
    assert (g["mfma_bad"], g["tile_bad"]) == (int(stage < 2), int(stage >= 2)), g
    assert (g["first_bad_wg"], g["first_bad_stage"], g["first_bad_word"]) == (wg, stage, word), g
    assert (g["first_bad_want"], g["first_bad_xor"]) == (want, 1 << bit), g
    assert g["error"] == (f"3/4 workgroups exact (feed_bad={int(stage < 2)} stat_bad={int(stage == 2)} o_bad={int(stage == 3)}); "
                          f"first bad: workgroup {wg} stage {stage} word {word} xor 0x{1 << bit:08x} (bit {bit})"), g


def test_the_stub_answers_what_the_shipped_verdict_says_of_the_same_faults(tmp_path):
    real = probe_contract.real_replies("datapath_attn", tmp_path)
    assert set(real) == {"ok", "stuck_bit", "missing", "device_bad"}
    for mode, want in real.items():
        got = json.loads(json.dumps(stub_probe._datapath_attn_device(0, mode, probe_contract.NONCE)))
        assert sorted(got) == sorted(want), mode                          # the printer's fields, no more, no fewer
        for key in probe_contract.KEYS["datapath_attn"]:
            if not key.endswith("_covered"):                              # the image names no placement
                assert got[key] == want[key], (mode, key, got[key], want[key])
    replies = contract_cli.probe_replies_text(contract_cli.datapath_attn_cli(tmp_path)).splitlines()
    blank, oneshot, serve, probe = (json.loads(ln) for ln in replies)
    assert blank == {**stub_probe._blank("datapath_attn", 99, 7000), "error": "no such GPU (count=1)"}
    assert oneshot["datapath_attn"] is serve["datapath_attn"] is True and "datapath_attn" not in probe
    assert serve["id"] == 5 and [k for k in serve if k.startswith("datapath")] == ["datapath_attn"]


def _series():                                      # the datapath series of /metrics: name -> value
    rows = (ln.rsplit(" ", 1) for ln in core().metrics_render().splitlines() if ln.startswith("mi355x_dp_datapath"))
    return {name: float(v) for name, v in rows}


def test_every_second_sweep_checks_and_a_failure_is_unhealthy_with_series_of_its_own(tmp_path):
    _, ctl, log, eng, dev = _engine(tmp_path, {"datapath_attn": {"2": "stuck_bit"}, "datapath_splitk": {"1": "stuck_bit"}},
                                    datapath_attn_check_every=2)
    with closing(eng):
        before = _series()
        eng.sweep()                                   # sweep 0: checked, device 2 fails; the split-K check is off
        snap = eng.snapshot()
        assert {d for d, (ok, _) in snap.items() if not ok} == {dev[2]}
        assert snap[dev[2]][1][0].startswith("datapath attn check: 255/256 workgroups exact (feed_bad=0 stat_bad=0 o_bad=36); "
                                             "first bad: workgroup 17 stage 3 word 139264 xor 0x40000000 (bit 30)"), snap[dev[2]]
        ctl.write_text("{}")
        eng.sweep()                                   # sweep 1: no check, the verdict stands
        assert eng.stats()["datapath_attn_checks"] == 1 and not eng.snapshot()[dev[2]][0]
        eng.sweep()                                   # sweep 2: checked again, passes
        st = eng.stats()
        assert st["datapath_attn_checks"] == 2 and st["datapath_attn_failures"] == 1 and st["datapath_splitk_checks"] == 0
        assert all(ok for ok, _ in eng.snapshot().values())
        assert {ln.split(":")[0] for ln in log.read_text().split() if ln.startswith("datapath")} == {"datapath_attn"}
        assert {k for k, v in _series().items() if v != before.get(k, 0)} == {
            "mi355x_dp_datapath_attn_checks_total", f'mi355x_dp_datapath_attn_check_failures_total{{device="{dev[2]}"}}'}


def test_request_grammar_in_the_servers_parser_and_in_the_stub(tmp_path):
    grammar = ["datapath_attn 10 0:1", "@4 datapath_attn 9.5 0:1:2.5 3:0x10", "datapath_attn10 0:1",
               "datapath_attn", "datapath_attn_ 10 0:1", "DATAPATH_ATTN 10 0:1"]
    got = contract_cli.probe_parse(contract_cli.probe_contract_cli(tmp_path), grammar)
    assert got == [stub_probe._parse(ln) for ln in grammar] and got[2:] == ["bad request"] * 4
    assert got[0]["kind"] == got[1]["kind"] == "datapath_attn" and got[1]["devices"] == [[0, 1, 2.5], [3, 16, 9.5]]

"""The split-K GEMM check above the kernel, without a GPU: the header's image against the reference's, the shipped
verdict on a flipped word of each stage and on an image that lacks one split's partial, the stub probe's replies
against the shipped verdict's, and the Engine's cadence and separate failure set over the stub."""
import json
from contextlib import closing

import numpy as np
import pytest

from rocm_k8s_device_plugin_amd.ops.native import core
from rocm_k8s_device_plugin_amd.testing import contract_cli, probe_contract, stub_probe
from rocm_k8s_device_plugin_amd.testing import datapath_gemm_reference as dg
from rocm_k8s_device_plugin_amd.testing import datapath_splitk_reference as ds

from test_native_datapath_f16_daemon import _engine

SIZES, NONCE = (2, 3, 2), 0xDEADBEEF                   # tiles, splits, ksteps of the verdict cases


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return contract_cli.datapath_splitk_cli(tmp_path_factory.mktemp("datapath_splitk_contract"))


@pytest.mark.parametrize("tiles,splits,ksteps,nonce", [(1, 1, 1, 0xFFFFFFFF), (*SIZES, NONCE), (2, 8, 1, NONCE)])
def test_the_header_and_the_reference_give_one_image(cli, tiles, splits, ksteps, nonce):
    got = np.frombuffer(contract_cli.datapath_splitk_image(cli, tiles, splits, ksteps, nonce), dtype="<u4")
    want = np.frombuffer(ds.image_bytes(*ds.healthy(tiles, splits, ksteps, nonce)), dtype="<u4")
    assert got.size == want.size and np.argwhere(got != want).tolist() == []


def _verdict(cli, tmp_path, image):
    r = contract_cli.datapath_splitk_verdict(cli, ds.image_bytes(*image), *SIZES, NONCE, tmp_path)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


# (stage, word as the verdict numbers it, bit): fold words of both feeds (wg * 8 + wave * 2 + {xor, sum}), D words
# (tile * 16384 + row * 128 + column), ledger words (tile * 8 + word)
FLIPS = [(0, 0, 0), (0, 5 * 8 + 7, 31), (1, 2 * 8 + 2, 9), (2, 0, 31), (2, 16384 + 77 * 128 + 5, 23), (2, 2 * 16384 - 1, 0),
         (3, 0, 1), (3, 8 + 1, 30), (3, 8 + 5, 4), (3, 7, 0)]


@pytest.mark.parametrize("stage,word,bit", FLIPS)
def test_the_verdict_passes_the_image_and_names_a_flipped_bit(cli, tmp_path, stage, word, bit):
    recs, d, led = ds.healthy(*SIZES, NONCE)
    g = _verdict(cli, tmp_path, (recs, d, led))
    assert g["ok"] is True and g["records_ok"] == g["tiles"] == 2 and g["stage_bad"] == [0] * 4 and g["error"] == "", g
    target = (recs.reshape(-1), word // 8 * ds.REC_WORDS + ds.fold_slot(stage, word % 8)) if stage < 2 else \
        ((d, led)[stage - 2].reshape(-1), word)
    want = int(target[0][target[1]])
    target[0][target[1]] ^= np.uint32(1 << bit)
    tile = {0: word // 8 // SIZES[1], 1: word // 8 // SIZES[1], 2: word // ds.TILE_WORDS, 3: word // 8}[stage]
    g = _verdict(cli, tmp_path, (recs, d, led))
    assert g["ok"] is False and g["records_ok"] == 1 and g["stage_bad"] == [int(s == stage) for s in range(4)], g
    assert (g["mfma_bad"], g["tile_bad"], g["ledger_bad"]) == (int(stage < 2), int(stage == 2), int(stage == 3)), g
    assert (g["first_bad_wg"], g["first_bad_stage"], g["first_bad_word"]) == (tile, stage, word), g
    assert (g["first_bad_want"], g["first_bad_xor"]) == (want, 1 << bit), g
    assert g["error"] == (f"1/2 tiles exact (feed_bad={int(stage < 2)} tile_bad={int(stage == 2)} ledger_bad={int(stage == 3)}); "
                          f"first bad: tile {tile} stage {stage} word {word} xor 0x{1 << bit:08x} (bit {bit})"), g


def test_an_image_that_lacks_one_splits_partial_fails_in_the_d_words_and_in_the_ledger(cli, tmp_path):
    tiles, splits, ksteps = SIZES
    recs, d, led = ds.healthy(*SIZES, NONCE)
    d[1] = dg.f32_words(ds.integers(NONCE, 1, splits, ksteps, skip=(2,)), dg.qx(NONCE, 1)).reshape(-1)
    led[1] = ds.ledger(NONCE, 1, splits, ksteps, skip=(2,))
    g = _verdict(cli, tmp_path, (recs, d, led))
    assert g["ok"] is False and g["records_ok"] == 1 and g["stage_bad"][:2] == [0, 0], g
    short = np.flatnonzero(ds.partial(NONCE, 1, splits, ksteps, 2))        # an even count of odd products: rarely zero
    assert g["stage_bad"][2] == short.size > 16000, g
    assert g["stage_bad"][3] == 6, g                                       # arrivals, who, and the four fold words
    assert (g["first_bad_wg"], g["first_bad_stage"], g["first_bad_word"]) == (1, 2, ds.TILE_WORDS + int(short[0])), g
    d[1] = ds.healthy(*SIZES, NONCE)[1][1]                                  # the D words right, the ledger still short
    g = _verdict(cli, tmp_path, (recs, d, led))
    assert g["stage_bad"] == [0, 0, 0, 6] and (g["first_bad_stage"], g["first_bad_word"]) == (3, 8), g
    assert (g["first_bad_got"], g["first_bad_want"]) == (splits - 1, splits), g


def test_the_stub_answers_what_the_shipped_verdict_says_of_the_same_faults(tmp_path):
    real = probe_contract.real_replies("datapath_splitk", tmp_path)
    assert set(real) == {"ok", "stuck_bit", "missing", "device_bad"}
    for mode, want in real.items():
        got = json.loads(json.dumps(stub_probe._datapath_splitk_device(0, mode, probe_contract.NONCE)))
        assert sorted(got) == sorted(want), mode                          # the printer's fields, no more, no fewer
        for key in probe_contract.KEYS["datapath_splitk"]:
            if not key.endswith("_covered"):                              # the image names no placement
                assert got[key] == want[key], (mode, key, got[key], want[key])
    replies = contract_cli.probe_replies_text(contract_cli.datapath_splitk_cli(tmp_path)).splitlines()
    blank, oneshot, serve, probe = (json.loads(ln) for ln in replies)
    assert blank == {**stub_probe._blank("datapath_splitk", 99, 7000), "error": "no such GPU (count=1)"}
    assert oneshot["datapath_splitk"] is serve["datapath_splitk"] is True and "datapath_splitk" not in probe
    assert serve["id"] == 5 and [k for k in serve if k.startswith("datapath")] == ["datapath_splitk"]


def _series():                                      # the datapath series of /metrics: name -> value
    rows = (ln.rsplit(" ", 1) for ln in core().metrics_render().splitlines() if ln.startswith("mi355x_dp_datapath"))
    return {name: float(v) for name, v in rows}


def test_every_second_sweep_checks_and_a_failure_is_unhealthy_with_series_of_its_own(tmp_path):
    _, ctl, log, eng, dev = _engine(tmp_path, {"datapath_splitk": {"2": "stuck_bit"}, "datapath_gemm": {"1": "stuck_bit"}},
                                    datapath_splitk_check_every=2)
    with closing(eng):
        before = _series()
        eng.sweep()                                   # sweep 0: checked, device 2 fails; the gemm check is off
        snap = eng.snapshot()
        assert {d for d, (ok, _) in snap.items() if not ok} == {dev[2]}
        assert snap[dev[2]][1][0].startswith("datapath splitk check: 31/32 tiles exact (feed_bad=0 tile_bad=128 ledger_bad=0); "
                                             "first bad: tile 17 stage 2 word 278528 xor 0x40000000 (bit 30)"), snap[dev[2]]
        ctl.write_text("{}")
        eng.sweep()                                   # sweep 1: no check, the verdict stands
        assert eng.stats()["datapath_splitk_checks"] == 1 and not eng.snapshot()[dev[2]][0]
        eng.sweep()                                   # sweep 2: checked again, passes
        st = eng.stats()
        assert st["datapath_splitk_checks"] == 2 and st["datapath_splitk_failures"] == 1 and st["datapath_gemm_checks"] == 0
        assert all(ok for ok, _ in eng.snapshot().values())
        assert {ln.split(":")[0] for ln in log.read_text().split() if ln.startswith("datapath")} == {"datapath_splitk"}
        assert {k for k, v in _series().items() if v != before.get(k, 0)} == {
            "mi355x_dp_datapath_splitk_checks_total", f'mi355x_dp_datapath_splitk_check_failures_total{{device="{dev[2]}"}}'}


def test_request_grammar_in_the_servers_parser_and_in_the_stub(tmp_path):
    grammar = ["datapath_splitk 10 0:1", "@4 datapath_splitk 9.5 0:1:2.5 3:0x10", "datapath_splitk10 0:1",
               "datapath_splitk", "datapath_splitk_ 10 0:1", "DATAPATH_SPLITK 10 0:1"]
    got = contract_cli.probe_parse(contract_cli.probe_contract_cli(tmp_path), grammar)
    assert got == [stub_probe._parse(ln) for ln in grammar] and got[2:] == ["bad request"] * 4
    assert got[0]["kind"] == got[1]["kind"] == "datapath_splitk" and got[1]["devices"] == [[0, 1, 2.5], [3, 16, 9.5]]

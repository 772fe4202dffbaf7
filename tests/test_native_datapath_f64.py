"""The f64 MFMA datapath check above the kernel, without a GPU: the Engine's cadence, failures, reason and series
over the stub probe, and the request grammar in the server's parser."""
from contextlib import closing

from rocm_k8s_device_plugin_amd.ops.native import core
from rocm_k8s_device_plugin_amd.testing import contract_cli, stub_probe

from test_native_datapath_f16_daemon import _engine

def _series():                                      # the datapath series of /metrics: name -> value
    rows = (ln.rsplit(" ", 1) for ln in core().metrics_render().splitlines() if ln.startswith("mi355x_dp_datapath"))
    return {name: float(v) for name, v in rows}


def test_every_second_sweep_checks_and_a_failure_is_unhealthy_with_series_of_its_own(tmp_path):
    _, ctl, log, eng, dev = _engine(tmp_path, {"datapath_f64": {"2": "stuck_bit"}}, datapath_f64_check_every=2)
    with closing(eng):
        before = _series()
        eng.sweep()                                   # sweep 0: checked, device 2 fails
        snap = eng.snapshot()
        assert {d for d, (ok, _) in snap.items() if not ok} == {dev[2]}
        assert snap[dev[2]][1][0].startswith("datapath f64 check: 255/256 workgroups exact") and \
            "stage 3 word 4 xor 0x40000000 (bit 30)" in snap[dev[2]][1][0], snap[dev[2]]
        ctl.write_text("{}")
        eng.sweep()                                   # sweep 1: no check, the verdict stands
        assert eng.stats()["datapath_f64_checks"] == 1 and not eng.snapshot()[dev[2]][0]
        eng.sweep()                                   # sweep 2: checked again, passes
        st = eng.stats()
        assert st["datapath_f64_checks"] == 2 and st["datapath_f64_failures"] == 1
        assert all(ok for ok, _ in eng.snapshot().values())
        assert {ln.split(":")[0] for ln in log.read_text().split() if ln.startswith("datapath")} == {"datapath_f64"}
        assert {k for k, v in _series().items() if v != before.get(k, 0)} == {
            "mi355x_dp_datapath_f64_checks_total", f'mi355x_dp_datapath_f64_check_failures_total{{device="{dev[2]}"}}'}


def test_flag_at_zero_never_sends_the_verb(tmp_path):
    _, ctl, log, eng, dev = _engine(tmp_path, {"datapath_f64": {"2": "stuck_bit"}}, datapath_check_every=1)
    with closing(eng):
        eng.sweep()
        eng.sweep()
        assert "datapath_f64" not in log.read_text() and "datapath:0" in log.read_text().split()
        assert all(ok for ok, _ in eng.snapshot().values()) and eng.stats()["datapath_f64_checks"] == 0


GRAMMAR = ["datapath_f64 10 0:1", "@4 datapath_f64 9.5 0:1:2.5 3:0x10", "datapath_f64 10",
           "datapath_f6410 0:1", "datapath_f64", "datapath_f64 x 0:1", "datapath_f64 10 0:1 x", "datapath_f64 10 0",
           "DATAPATH_F64 10 0:1", "@7datapath_f64 10 0:1", "datapath_f64_ 10 0:1"]


def test_request_grammar_in_the_servers_parser_and_in_the_stub(tmp_path):
    got = contract_cli.probe_parse(contract_cli.probe_contract_cli(tmp_path), GRAMMAR)
    assert got == [stub_probe._parse(ln) for ln in GRAMMAR] and got[3:] == ["bad request"] * 8
    assert got[0] == {"tagged": False, "id": 0, "kind": "datapath_f64", "iters": 0, "timeout": 10, "mib": 0,
                      "devices": [[0, 1, 10]]}
    assert got[1]["id"] == 4 and got[1]["devices"] == [[0, 1, 2.5], [3, 16, 9.5]] and got[2]["devices"] == []

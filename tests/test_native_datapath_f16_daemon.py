"""-datapath_f16_check_every: the f16 MFMA datapath check in the native health
engine and the daemon, over the stub probe (CPU only). The same rules as the
f32 check (idle GPUs only, none while the busy state is unknown, the cadence),
failures of its own that neither an f32 nor an int8 pass clears (and that
clear none of theirs), a reply from another agent dropped, and with the default
nothing changes: no datapath_f16 request, no series, no word on stderr. The
kernel and the real verdict run in tests/test_gpu_datapath_f16.py."""
import asyncio
import json
import os
import shutil
import subprocess
import sys
import urllib.request

import pytest

from rocm_k8s_device_plugin_amd.ops.native import core
from rocm_k8s_device_plugin_amd.testing.fake_kubelet import FakeKubelet
from rocm_k8s_device_plugin_amd.testing.fixtures import make_mi355x_node
from rocm_k8s_device_plugin_amd.topology import discover

from test_native_health import EXE, STUB, _bus_id, _busy_gpu, _by_ordinal, _stop
from test_native_metrics import _free_port, _series

STUCK = {"datapath_f16": {"2": "stuck_bit"}}


@pytest.fixture(scope="module", autouse=True)
def _built():
    from rocm_k8s_device_plugin_amd import _build
    _build.ensure_built(hip=False)


def _engine(tmp_path, control, **opts):
    fi = make_mi355x_node(tmp_path / "n")
    ctl, log = tmp_path / "ctl.json", tmp_path / "stub.log"
    ctl.write_text(json.dumps(control))
    log.write_text("")
    o = dict(dev_root=str(fi.dev), liveness=True, probe_exe=STUB, argv_prefix=[sys.executable], probe_timeout_s=3.0,
             extra_env={"MI355X_STUB_PROBE_CONTROL": str(ctl), "MI355X_STUB_PROBE_LOG": str(log)}, fail_threshold=1)
    o.update(opts)
    eng = core().HealthEngine(str(fi.sysfs), o)
    return fi, ctl, log, eng, _by_ordinal(eng)


def _requests(log, prefix="datapath_f16:"):
    """The host ordinals that got a request of that kind (a failed one is asked
    twice: the prober confirms a server's failure in a fresh process)."""
    return sorted({int(ln.split(":")[1]) for ln in log.read_text().split() if ln.startswith(prefix)})


def test_failed_verdict_is_unhealthy_with_stage_word_and_xor_and_healthy_after_a_pass(tmp_path):
    fi, ctl, log, eng, dev = _engine(tmp_path, STUCK, datapath_f16_check_every=1)
    try:
        eng.sweep()
        snap = eng.snapshot()
        assert {d for d, (ok, _) in snap.items() if not ok} == {dev[2]}
        reason = snap[dev[2]][1][0]
        assert reason.startswith("datapath f16 check: ")
        assert "stage 4 word 0 xor 0x40000000 (bit 30)" in reason
        st = eng.stats()
        assert st["datapath_f16_checks"] == 1 and st["datapath_f16_failures"] == 1
        assert st["datapath_checks"] == 0 and st["datapath_failures"] == 0
        assert _requests(log) == list(range(8)) and _requests(log, "datapath:") == []
        text = core().metrics_render()
        assert "mi355x_dp_datapath_f16_checks_total" in text
        assert f'mi355x_dp_datapath_f16_check_failures_total{{device="{dev[2]}"}}' in text
        ctl.write_text("{}")                            # the next check passes: Healthy again
        eng.sweep()
        assert all(ok for ok, _ in eng.snapshot().values())
        assert eng.stats()["datapath_f16_checks"] == 2 and eng.stats()["datapath_f16_failures"] == 1
    finally:
        eng.close()


@pytest.mark.parametrize("mode,want", [("missing", "254/256 workgroups exact"), ("device_bad", "device_bad=12")])
def test_other_failed_verdicts(tmp_path, mode, want):
    fi, ctl, log, eng, dev = _engine(tmp_path, {"datapath_f16": {"6": mode}}, datapath_f16_check_every=1)
    try:
        eng.sweep()
        snap = eng.snapshot()
        assert {d for d, (ok, _) in snap.items() if not ok} == {dev[6]} and want in snap[dev[6]][1][0]
    finally:
        eng.close()


def test_only_idle_gpus_are_checked(tmp_path):
    fi, ctl, log, eng, dev = _engine(tmp_path, {"datapath_f16": {"5": "stuck_bit"}}, datapath_f16_check_every=1)
    try:
        _busy_gpu(fi, discover(str(fi.sysfs)), dev[5])
        eng.sweep()
        assert _requests(log) == [0, 1, 2, 3, 4, 6, 7]
        assert all(ok for ok, _ in eng.snapshot().values())
        assert eng.stats()["datapath_f16_checks"] == 1 and eng.stats()["datapath_f16_failures"] == 0
    finally:
        eng.close()


def test_no_check_while_busy_state_is_unknown(tmp_path):
    fi, ctl, log, eng, dev = _engine(tmp_path, STUCK, datapath_f16_check_every=1)
    proc = fi.sysfs / "class/kfd/kfd/proc"
    if proc.is_dir():
        shutil.rmtree(proc)
    proc.write_text("")                       # a process list that cannot be listed: who is busy is unknown
    try:
        eng.sweep()
        assert not eng.stats()["busy_state_known"]
        assert _requests(log) == [] and eng.stats()["datapath_f16_checks"] == 0
        assert all(ok for ok, _ in eng.snapshot().values())
    finally:
        eng.close()


def test_cadence_and_the_verdict_stands_between_checks(tmp_path):
    fi, ctl, log, eng, dev = _engine(tmp_path, STUCK, datapath_f16_check_every=3)
    try:
        eng.sweep()                                   # sweep 0: checked
        assert not eng.snapshot()[dev[2]][0]
        ctl.write_text("{}")
        eng.sweep()                                   # sweeps 1, 2: no check, the verdict stands
        eng.sweep()
        assert eng.stats()["datapath_f16_checks"] == 1 and not eng.snapshot()[dev[2]][0]
        eng.sweep()                                   # sweep 3: checked again, passes
        assert eng.stats()["datapath_f16_checks"] == 2 and eng.snapshot()[dev[2]][0]
    finally:
        eng.close()


def test_an_int8_pass_does_not_clear_a_f16_failure_nor_the_reverse(tmp_path):
    fi, ctl, log, eng, dev = _engine(tmp_path, STUCK, datapath_f16_check_every=1, datapath_i8_check_every=1,
                                     datapath_check_every=1)
    try:
        eng.sweep()
        eng.sweep()                                   # f32 and int8 pass twice on GPU 2: the f16 failure stands
        ok, reasons = eng.snapshot()[dev[2]]
        assert not ok and [r.split(":")[0] for r in reasons] == ["datapath f16 check"]
        assert _requests(log, "datapath_i8:") == list(range(8)) and _requests(log, "datapath:") == list(range(8))
        ctl.write_text(json.dumps({"datapath_i8": {"2": "stuck_bit"}, "datapath": {"3": "missing"}}))
        eng.sweep()                                   # f16 passes everywhere: it clears its own failure, no other
        snap = eng.snapshot()
        assert {d for d, (ok, _) in snap.items() if not ok} == {dev[2], dev[3]}
        assert [r.split(":")[0] for r in snap[dev[2]][1]] == ["datapath i8 check"]
        assert [r.split(":")[0] for r in snap[dev[3]][1]] == ["datapath check"]
        st = eng.stats()
        assert (st["datapath_f16_checks"], st["datapath_f16_failures"]) == (3, 2)
        assert (st["datapath_i8_checks"], st["datapath_i8_failures"]) == (3, 1)
        ctl.write_text(json.dumps({"datapath_i8": {"2": "stuck_bit"}, "datapath_f16": {"2": "missing"},
                                   "datapath": {"2": "device_bad"}}))
        eng.sweep()                                   # all three reasons side by side
        assert sorted(r.split(":")[0] for r in eng.snapshot()[dev[2]][1]) == \
            ["datapath check", "datapath f16 check", "datapath i8 check"]
    finally:
        eng.close()


def test_a_reply_from_another_agent_is_dropped(tmp_path):
    """The map is stale where no probe reply shows it (probe replies name no agent), but the check
    replies name theirs: agent 3's failed f16 check is dropped, not written to the device the map
    puts at ordinal 3; with agents that are where the map has them the same fault is a verdict."""
    fi = make_mi355x_node(tmp_path / "n")
    inv = discover(str(fi.sysfs))
    eng = core().HealthEngine(str(fi.sysfs), {"dev_root": str(fi.dev)})
    dev = _by_ordinal(eng)
    eng.close()
    ident = {str(o): {"kfd_node_id": inv.by_id[d].node_id, "pci_bus_id": _bus_id(inv.by_id[d])} for o, d in dev.items()}
    for swapped in (True, False):
        who = dict(ident)
        if swapped:
            who["2"], who["3"] = ident["3"], ident["2"]                # agents 2 and 3 are each other's devices
        ctl, log = tmp_path / f"ctl{swapped}.json", tmp_path / f"stub{swapped}.log"
        ctl.write_text(json.dumps({"datapath_f16": {"3": "stuck_bit"}}))
        log.write_text("")
        eng = core().HealthEngine(str(fi.sysfs), dict(
            dev_root=str(fi.dev), liveness=True, probe_exe=STUB, argv_prefix=[sys.executable], probe_timeout_s=3.0,
            fail_threshold=1, datapath_f16_check_every=1,
            extra_env={"MI355X_STUB_PROBE_CONTROL": str(ctl), "MI355X_STUB_PROBE_LOG": str(log),
                       "MI355X_STUB_PROBE_IDENTITY": json.dumps(who), "MI355X_STUB_PROBE_ANONYMOUS": "probe"}))
        try:
            eng.sweep()
            bad = {d for d, (ok, _) in eng.snapshot().items() if not ok}
            st = eng.stats()
            assert st["identity_remaps"] == 0 and st["datapath_f16_checks"] == 1
            assert (bad, st["datapath_f16_failures"]) == ((set(), 0) if swapped else ({dev[3]}, 1)), eng.snapshot()
        finally:
            eng.close()


def test_the_two_checks_keep_failures_of_their_own(tmp_path):
    """An f32 pass does not clear a f16 failure, nor the reverse; both reasons stand side by side."""
    control = {"datapath_f16": {"2": "stuck_bit"}}
    fi, ctl, log, eng, dev = _engine(tmp_path, control, datapath_f16_check_every=1, datapath_check_every=1)
    try:
        eng.sweep()                                   # f32 passes on every GPU, f16 fails on GPU 2
        ok, reasons = eng.snapshot()[dev[2]]
        assert not ok and len(reasons) == 1 and reasons[0].startswith("datapath f16 check: ")
        assert _requests(log, "datapath:") == list(range(8))
        eng.sweep()                                   # and again: the passing f32 check has cleared nothing
        assert not eng.snapshot()[dev[2]][0]
        st = eng.stats()
        assert (st["datapath_checks"], st["datapath_failures"]) == (2, 0)
        assert (st["datapath_f16_checks"], st["datapath_f16_failures"]) == (2, 2)
        ctl.write_text(json.dumps({"datapath": {"2": "stuck_bit"}, "datapath_f16": {"4": "missing"}}))
        eng.sweep()                                   # the reverse: f16 passes on GPU 2 while f32 fails there
        snap = eng.snapshot()
        assert {d for d, (ok, _) in snap.items() if not ok} == {dev[2], dev[4]}
        assert [r.split(":")[0] for r in snap[dev[2]][1]] == ["datapath check"]
        assert [r.split(":")[0] for r in snap[dev[4]][1]] == ["datapath f16 check"]
        ctl.write_text(json.dumps({"datapath": {"2": "stuck_bit"}, "datapath_f16": {"2": "device_bad"}}))
        eng.sweep()
        assert sorted(r.split(":")[0] for r in eng.snapshot()[dev[2]][1]) == ["datapath check", "datapath f16 check"]
    finally:
        eng.close()


def test_default_sends_no_datapath_f16_request(tmp_path):
    fi, ctl, log, eng, dev = _engine(tmp_path, STUCK, datapath_check_every=1)
    try:
        for _ in range(3):
            eng.sweep()
        assert _requests(log) == [] and "datapath_f16" not in log.read_text()
        assert _requests(log, "datapath:") == list(range(8))           # the f32 check runs as it did
        assert all(ok for ok, _ in eng.snapshot().values())
        st = eng.stats()
        assert st["datapath_f16_checks"] == 0 and st["datapath_f16_failures"] == 0 and st["datapath_checks"] == 3
    finally:
        eng.close()


def test_spawn_mode_runs_the_one_shot_probe(tmp_path):
    fi, ctl, log, eng, dev = _engine(tmp_path, STUCK, datapath_f16_check_every=1, persistent=False)
    try:
        eng.sweep()
        snap = eng.snapshot()
        assert {d for d, (ok, _) in snap.items() if not ok} == {dev[2]} and "stage 4 word 0" in snap[dev[2]][1][0]
        assert _requests(log) == list(range(8))
    finally:
        eng.close()


def _run_daemon(tmp_path, name, control, *flags):
    """The daemon over the stub until kubelet has its list and one more pulse has
    run: (ordinal -> device, device -> health, metric series, stub log, stderr)."""
    fi = make_mi355x_node(tmp_path / name / "n")
    ctl, log = tmp_path / name / "ctl.json", tmp_path / name / "stub.log"
    ctl.write_text(json.dumps(control))
    log.write_text("")
    eng = core().HealthEngine(str(fi.sysfs), {"dev_root": str(fi.dev)})
    dev = _by_ordinal(eng)
    eng.close()
    kdir = str(tmp_path / name / "dp")
    port = _free_port()

    async def go():
        k = FakeKubelet(kdir)
        await k.start()
        p = subprocess.Popen([EXE, "-kubelet_dir", kdir, "-sysfs_root", str(fi.sysfs), "-dev_root", str(fi.dev),
                              "-exporter_socket", "", "-pulse", "1", "-liveness", "-liveness_probe", STUB,
                              "-liveness_fail_threshold", "1", "-liveness_timeout", "3", "-metrics_port", str(port),
                              *flags],
                             stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True,
                             env=dict(os.environ, MI355X_STUB_PROBE_CONTROL=str(ctl), MI355X_STUB_PROBE_LOG=str(log)))
        series = {}
        try:
            st = await k.wait_for_resource("amd.com/gpu", 8, timeout=20)
            for _ in range(100):                       # the sweep before the first list, and one pulse more
                with urllib.request.urlopen(f"http://127.0.0.1:{port}/metrics", timeout=5) as r:
                    series = _series(r.read().decode())
                if series.get("mi355x_dp_health_sweep_seconds_count", 0) >= 2:
                    break
                await asyncio.sleep(0.1)
            assert series.get("mi355x_dp_health_sweep_seconds_count", 0) >= 2, sorted(series)
        finally:
            rc, err = await asyncio.to_thread(_stop, p)
            await k.stop()
        assert rc == 0, err[-3000:]
        return dev, dict(st.devices), series, log.read_text(), err

    return asyncio.run(asyncio.wait_for(go(), 60))


def test_daemon_flag_makes_the_device_unhealthy_and_default_changes_nothing(tmp_path):
    dev, devices, series, log, err = _run_daemon(tmp_path, "on", STUCK, "-datapath_f16_check_every", "1")
    assert {d for d, h in devices.items() if h == "Unhealthy"} == {dev[2]}
    assert "datapath f16 check: " in err and "stage 4 word 0 xor 0x40000000" in err
    assert series["mi355x_dp_datapath_f16_checks_total"] >= 1
    assert series[f'mi355x_dp_datapath_f16_check_failures_total{{device="{dev[2]}"}}'] >= 1
    assert "datapath_f16:2" in log.split() and not any(ln.startswith("datapath:") for ln in log.split())
    assert not any(s.startswith("mi355x_dp_datapath_check") for s in series)       # the f32 check stayed off
    assert not any(s.startswith("mi355x_dp_datapath_i8") for s in series)          # and the int8 check
    # flag unset: the same fixture and the same fault knob, and kubelet's list is the one a daemon without
    # the feature sends: every device Healthy, no request, no series, no word on stderr
    dev0, devices0, series0, log0, err0 = _run_daemon(tmp_path, "off", STUCK)
    assert devices0 == {d: "Healthy" for d in dev0.values()} and len(devices0) == 8
    assert "datapath_f16" not in log0 and "datapath_f16" not in err0 and "datapath f16" not in err0
    assert not any("datapath_f16" in s for s in series0)
    # ... and with the f32 check on alone, still none
    _, devices1, series1, log1, err1 = _run_daemon(tmp_path, "f32", STUCK, "-datapath_check_every", "1")
    assert devices1 == devices0
    assert "datapath_f16" not in log1 and "datapath_f16" not in err1 and not any("datapath_f16" in s for s in series1)
    assert series1["mi355x_dp_datapath_checks_total"] >= 1


def test_daemon_refuses_the_flag_without_liveness():
    p = subprocess.run([EXE, "-datapath_f16_check_every", "1"], capture_output=True, text=True, timeout=20)
    assert p.returncode == 1 and "datapath_f16_check_every needs -liveness" in p.stderr
    f32 = subprocess.run([EXE, "-datapath_check_every", "1"], capture_output=True, text=True, timeout=20)
    tail = lambda err: err[err.index("datapath"):]                                            # noqa: E731
    assert tail(p.stderr).replace("datapath_f16_check_every", "datapath_check_every") == tail(f32.stderr)  # same wording
    p = subprocess.run([EXE, "-h"], capture_output=True, text=True, timeout=20)
    assert "-datapath_f16_check_every N" in p.stdout + p.stderr and "-datapath_check_every N" in p.stdout + p.stderr


def test_chart_renders_the_flag_only_when_set():
    from rocm_k8s_device_plugin_amd.testing.helm_lite import rendered_objects
    chart = os.path.join(os.path.dirname(__file__), "..", "helm", "amd-gpu")

    def dp_args(values):
        for obj in rendered_objects(chart, values):
            if obj.get("kind") == "DaemonSet" and "device-plugin" in obj["metadata"]["name"]:
                return obj["spec"]["template"]["spec"]["containers"][0]["args"]
        raise AssertionError("no device plugin DaemonSet")

    unset = dp_args({"dp": {"pulse": 2, "liveness": {"enabled": True}}})
    assert not any("datapath" in a for a in unset)
    # 0 (the chart's default) is unset: the rendered arguments are the same
    assert dp_args({"dp": {"pulse": 2, "liveness": {"enabled": True, "datapathF16CheckEvery": 0}}}) == unset
    on = dp_args({"dp": {"pulse": 2, "liveness": {"enabled": True, "datapathF16CheckEvery": 30}}})
    assert "-datapath_f16_check_every=30" in on and [a for a in on if "datapath" not in a] == unset
    assert not any(a.startswith("-datapath_check_every") for a in on)
    assert not any(a.startswith("-datapath_i8_check_every") for a in on)
    both = dp_args({"dp": {"pulse": 2, "liveness": {"enabled": True, "datapathF16CheckEvery": 30,
                                                    "datapathCheckEvery": 7}}})
    assert "-datapath_f16_check_every=30" in both and "-datapath_check_every=7" in both
    # without liveness the value renders nothing (the daemon would refuse the flag)
    assert not any("datapath" in a for a in dp_args({"dp": {"liveness": {"datapathF16CheckEvery": 30}}}))
